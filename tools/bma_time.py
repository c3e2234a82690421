"""Timing of exact arc posteriors (exact_bma.hip behind fbn_bma_run) beside the host twin and the exact search.

    python tools/bma_time.py [--out profiles/exact/bma_time.json] [--sizes 12,16,20,24] [--tile-bits 4,6,...]

Workloads: the first n columns of tests/golden/alarm/alarm_s5000.txt (5,000 samples) for n = 12, 16, 20, 24
with at most 3 parents under BDeu (iss 1), the uniform prior.  Each size runs in a child process of its own
under a time limit; its exit code and last stderr lines are recorded, and no further child is started after one
that did not exit 0.

Per size, from fbn_bma_info (median over the timed runs after one warm-up run): device time of the scorer, the
alpha transform, the levels, the Gamma transform and the q transform (HIP events around each phase's launches),
the wall time of each phase and of the whole run; from the same process the exact search's subset-max transform
and sink recursion under the same score, the yardstick for what the exp / ln costs over the compare; the three
transforms again under every --tile-bits value (n >= 20; the runs alternate over the values, the matrix compared
with the default's bit for bit); the host twin's wall time per phase for n <= 20 (one run, its result compared
with the device's bit for bit)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LIMITS = {12: 120, 16: 120, 20: 300, 24: 600}
RUNS = 5
SWEEP_RUNS = 3
SWEEP_MIN = 20
MAX_PARENTS = 3
HOST_TWIN_MAX = 20
PHASES = ("score_kernel_ms", "alpha_kernel_ms", "level_kernel_ms", "gamma_kernel_ms", "q_kernel_ms", "score_wall_ms",
          "upload_wall_ms", "alpha_wall_ms", "level_wall_ms", "gamma_wall_ms", "q_wall_ms", "wall_ms")
TRANSFORMS = ("alpha_kernel_ms", "gamma_kernel_ms", "q_kernel_ms")


def child(n, tile_bits):
    import fastbn_amd as F
    full = F.Dataset(os.path.join(REPO, "tests", "golden", "alarm", "alarm_s5000.txt"))
    ds = F.Dataset(columns=np.ascontiguousarray(full.columns[:n]), dims=np.ascontiguousarray(full.dims[:n]))
    ci = F.IndependenceTest(ds)
    ap = F.ArcPosterior("bde", max_parents=MAX_PARENTS)
    ap.learn(ci)  # warm-up: code objects, the scorer's tables
    infos = [dict(ap.learn(ci).info) for _ in range(RUNS)]
    rec = {"nvars": n, "nsamples": ds.num_instance, "max_parents": MAX_PARENTS, "score_name": "bde", "prior": 0,
           "timed_runs": RUNS, "log_z": ap.log_z, "b_full": ap.b_full, "arcs_at_least_half": int((ap.arc_prob >= 0.5).sum()),
           "q_empty_max_dev": float(np.abs(ap.q_empty - 1).max()), "families_scored": infos[0]["families_scored"],
           "lattice_bytes": infos[0]["lattice_bytes"], "tile_bits": infos[0]["tile_bits"], "passes": infos[0]["passes"],
           "device": {k: float(np.median([i[k] for i in infos])) for k in PHASES}}
    ex = F.ExactSearch("bde", max_parents=MAX_PARENTS)
    ex.learn(ci)
    xinfos = [dict(ex.learn(ci).exact_info) for _ in range(RUNS)]
    rec["exact_search"] = {k: float(np.median([i[k] for i in xinfos])) for k in ("transform_kernel_ms", "sink_kernel_ms", "wall_ms")}
    rec["exact_search"].update(tile_bits=xinfos[0]["tile_bits"], passes=xinfos[0]["passes"])
    sweep = {t: [] for t in tile_bits if t < n} if n >= SWEEP_MIN else {}
    for _ in range(SWEEP_RUNS):  # alternating, so that drift falls on every value alike
        for t in sweep:
            F.ArcPosterior.set_tuning(ci, t)
            got = F.ArcPosterior("bde", max_parents=MAX_PARENTS).learn(ci)
            assert got.arc_prob.tobytes() == ap.arc_prob.tobytes() and got.log_z == ap.log_z, f"tile_bits {t} changes the result"
            sweep[t].append(got.info)
    F.ArcPosterior.set_tuning(ci, 0)
    rec["tile_bits_sweep"] = [dict({k: float(np.median([i[k] for i in v])) for k in TRANSFORMS}, tile_bits=t, passes=v[0]["passes"],
                                   transforms_kernel_ms=float(np.median([sum(i[k] for k in TRANSFORMS) for i in v])))
                              for t, v in sweep.items()]
    if n <= HOST_TWIN_MAX:
        host = F.ArcPosterior("bde", max_parents=MAX_PARENTS).learn(ds, host=True)
        assert host.arc_prob.tobytes() == ap.arc_prob.tobytes() and host.log_z == ap.log_z, "device differs from the host twin"
        rec["host_twin"] = {k: host.info[k] for k in PHASES if k.endswith("wall_ms")}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "exact", "bma_time.json"))
    ap.add_argument("--sizes", default=",".join(str(n) for n in LIMITS))
    ap.add_argument("--tile-bits", default="4,6,8,10,12,13")
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    tile_bits = [int(t) for t in a.tile_bits.split(",") if t]
    if a.child:
        child(a.child, tile_bits)
        return 0
    results = []
    for n in [int(x) for x in a.sizes.split(",")]:
        rec = {"workload": f"bma_alarm{n}_5000", "time_limit_s": LIMITS[n]}
        try:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--tile-bits", a.tile_bits]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[n])
            rec["exit_code"] = r.returncode
            err = [ln for ln in r.stderr.strip().split("\n") if ln and "amdgpu.ids" not in ln]  # libdrm's notice
            rec["stderr_tail"] = err[-8:]
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
        json.dump({"tool": "tools/bma_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
