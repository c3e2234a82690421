"""Timing of exact score-optimal structure learning (exact_dp.hip behind fbn_exact_run) beside its host twin.

    python tools/exact_time.py [--out profiles/exact/exact_time.json] [--sizes 12,16,20,24] [--tile-bits 8,9,...]

Workloads: the first n columns of tests/golden/alarm/alarm_s5000.txt (5,000 samples) for n = 12, 16, 20, 24
with at most 3 parents under BIC.  Each size runs in a child process of its own under a time limit; its exit
code and last stderr lines are recorded, and no further child is started after one that did not exit 0.

Per size, from fbn_exact_info (median over the timed runs after one warm-up run): device time of the
scorer, of the subset-max transform and of the sink recursion (HIP events around each phase's launches), the
wall time of each phase and of the whole search, the lattice bytes and the transform's passes; the transform
again under every --tile-bits value (the runs alternate over the values, the result compared with the default's);
the host twin's wall time for n <= 20 (one run, its result compared with the device's); hill climbing's
score beside the optimum."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LIMITS = {12: 120, 16: 120, 20: 240, 24: 600}
RUNS = 5
MAX_PARENTS = 3
HOST_TWIN_MAX = 20
PHASES = ("score_kernel_ms", "transform_kernel_ms", "sink_kernel_ms", "score_wall_ms", "upload_wall_ms",
          "transform_wall_ms", "sink_wall_ms", "trace_wall_ms", "wall_ms")


def child(n, tile_bits):
    import fastbn_amd as F
    full = F.Dataset(os.path.join(REPO, "tests", "golden", "alarm", "alarm_s5000.txt"))
    ds = F.Dataset(columns=np.ascontiguousarray(full.columns[:n]), dims=np.ascontiguousarray(full.dims[:n]))
    ci = F.IndependenceTest(ds)
    ex = F.ExactSearch("bic", max_parents=MAX_PARENTS)
    ex.learn(ci)  # warm-up: code objects, the n ln n table
    infos = [dict(ex.learn(ci).exact_info) for _ in range(RUNS)]
    rec = {"nvars": n, "nsamples": ds.num_instance, "max_parents": MAX_PARENTS, "score_name": "bic", "timed_runs": RUNS,
           "score": ex.score, "arcs": sum(len(p) for p in ex.parents), "families_scored": infos[0]["families_scored"],
           "lattice_bytes": infos[0]["lattice_bytes"], "tile_bits": infos[0]["tile_bits"], "passes": infos[0]["passes"],
           "device": {k: float(np.median([i[k] for i in infos])) for k in PHASES}}
    sweep = {t: [] for t in tile_bits if t < n}
    for _ in range(RUNS):  # alternating, so that drift falls on every value alike
        for t in sweep:
            F.ExactSearch.set_tuning(ci, t)
            got = F.ExactSearch("bic", max_parents=MAX_PARENTS).learn(ci)
            assert got.parents == ex.parents and got.score == ex.score, f"tile_bits {t} changes the result"
            sweep[t].append((got.exact_info["transform_kernel_ms"], got.exact_info["passes"]))
    F.ExactSearch.set_tuning(ci, 0)
    rec["tile_bits_sweep"] = [{"tile_bits": t, "passes": v[0][1], "transform_kernel_ms": float(np.median([x[0] for x in v])),
                               "min": min(x[0] for x in v), "max": max(x[0] for x in v)} for t, v in sweep.items()]
    hc = F.HillClimbing("bic", max_parents=MAX_PARENTS).learn(ci)
    rec["hill_climbing"] = {"score": hc.score, "arcs": sum(len(p) for p in hc.parents), "wall_ms": hc.info["wall_ms"],
                            "below_optimum": ex.score - hc.score}
    if n <= HOST_TWIN_MAX:
        host = F.ExactSearch("bic", max_parents=MAX_PARENTS).learn(ds, host=True)
        assert host.parents == ex.parents and host.score == ex.score, "device differs from the host twin"
        rec["host_twin"] = {k: host.exact_info[k] for k in PHASES if k.endswith("wall_ms")}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "exact", "exact_time.json"))
    ap.add_argument("--sizes", default=",".join(str(n) for n in LIMITS))
    ap.add_argument("--tile-bits", default="8,9,10,11,12,13")
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    tile_bits = [int(t) for t in a.tile_bits.split(",") if t]
    if a.child:
        child(a.child, tile_bits)
        return 0
    results = []
    for n in [int(x) for x in a.sizes.split(",")]:
        rec = {"workload": f"exact_alarm{n}_5000", "time_limit_s": LIMITS[n]}
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
        json.dump({"tool": "tools/exact_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
