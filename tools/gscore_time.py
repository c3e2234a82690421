"""Timing of the Gaussian family scorer (gscore.hip behind fbn_gscore_families).

    python tools/gscore_time.py [--out profiles/hc/gscore_time.json] [--workloads gs_n64_k3,gs_n1000_k1]

Workloads, both on 2,000 samples of independent standard normals mixed along a band:
  * gs_n64_k3:   64 variables, every family with at most 3 parents (2,670,592 families in four buckets): the
                 shape of a lattice learner's score table.
  * gs_n1000_k1: 1,000 variables, the 999,000 one-parent families of a hill-climbing first sweep.
Each workload runs in a child process of its own under a time limit; no further child is started after one that
did not exit 0.  Per workload and score (bic, bge), on one context: WARM untimed batches, then REPEATS timed
ones, the two scores alternating batch by batch.  The time is HIP events around the bucket kernels alone
(fbn_gci_last_kernel_ms): no copies, no host bucketing.  Reported: median, min and max.  (The LDS-staging variant
this tool was first written to compare lost at gs_n64_k3 and is gone: DESIGN.md 5.20 keeps its numbers.)"""
import argparse
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LIMITS = {"gs_n64_k3": 240, "gs_n1000_k1": 240}
WARM, REPEATS = 3, 20


def families(name):
    """(fam_off int64, fam_cols int32, count)"""
    if name == "gs_n1000_k1":
        v, q = np.divmod(np.arange(1000 * 999), 999)
        cols = np.stack([v, q + (q >= v)], 1).astype(np.int32)
        return np.arange(0, 2 * len(cols) + 1, 2, dtype=np.int64), np.ascontiguousarray(cols.ravel()), len(cols)
    rows, sizes = [], []
    for k in range(4):
        P = np.array(list(itertools.combinations(range(64), k)), np.int32) if k else np.zeros((1, 0), np.int32)
        v = np.repeat(np.arange(64, dtype=np.int32), len(P))
        fam = np.concatenate([v[:, None], np.tile(P, (64, 1))], 1)
        fam = fam[~(fam[:, 1:] == fam[:, :1]).any(1)]
        rows.append(fam.ravel())
        sizes.append(np.full(len(fam), k + 1, np.int64))
    off = np.concatenate([[0], np.cumsum(np.concatenate(sizes))]).astype(np.int64)
    return off, np.ascontiguousarray(np.concatenate(rows)), len(off) - 1


def child(name):
    import fastbn_amd as F
    from fastbn_amd import api as A
    n = 1000 if name == "gs_n1000_k1" else 64
    rng = np.random.default_rng(1)
    Z = rng.standard_normal((n, 2000))
    X = Z + 0.5 * np.roll(Z, 1, 0) + 0.25 * np.roll(Z, 2, 0)
    ci = F.GaussianIndependenceTest(F.ContinuousDataset(columns=X))
    off, cols, nfam = families(name)
    ll, sc = np.zeros(nfam), np.zeros(nfam)
    rec = {"workload": name, "nvars": n, "nsamples": 2000, "families": nfam, "warm_up": WARM, "repeats": REPEATS, "scores": {}}
    scores = {k: A._gauss_score(k, 2000) for k in ("bic", "bge")}
    times = {k: [] for k in scores}
    for rep in range(WARM + REPEATS):
        for k, g in scores.items():
            A.lib.fbn_gscore_families(ci._h, C.byref(g), nfam, A._p(off), A._p(cols), A._p(ll), A._p(sc))
            if rep >= WARM:
                times[k].append(ci.last_kernel_ms())
    for k in scores:
        rec["scores"][k] = {"kernel_ms": {"median": float(np.median(times[k])), "min": min(times[k]), "max": max(times[k])}}
    rec["degenerate"] = ci.score_info()["degenerate"]
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hc", "gscore_time.json"))
    ap.add_argument("--workloads", default=",".join(LIMITS))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    results = []
    for name in a.workloads.split(","):
        rec = {"workload": name, "time_limit_s": LIMITS[name]}
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True, text=True,
                               timeout=LIMITS[name])
            rec["exit_code"] = r.returncode
            rec["stderr_tail"] = [ln for ln in r.stderr.strip().split("\n") if ln and "amdgpu.ids" not in ln][-8:]
            lines = [ln for ln in r.stdout.split("\n") if ln.startswith("{")]
            if r.returncode == 0 and lines:
                rec.update(json.loads(lines[-1]))
        except subprocess.TimeoutExpired as e:
            rec["exit_code"] = "time limit"
            err = e.stderr.decode() if isinstance(e.stderr, bytes) else (e.stderr or "")
            rec["stderr_tail"] = err.strip().split("\n")[-8:]
        results.append(rec)
        print(json.dumps(rec), flush=True)
        if rec["exit_code"] != 0:
            break  # nothing more is started on a device a child may have left in a bad state
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/gscore_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
