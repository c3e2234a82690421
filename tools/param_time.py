"""Timing of fbn_param_counts (all family tables of a DAG in one launch) beside what the library could
do before it: one synchronous fbn_ci_counts launch per family with a parent, np.bincount for roots.

    python tools/param_time.py [--out profiles/param/param_counts.json] [--workloads alarm,c5]

Workloads: `alarm` = ALARM-5000 with the DAG extension of its PC-stable CPDAG (37 families);
`c5` = the 1,000-variable x 100,000-sample synthetic column store of bench.py's config 5 with a
seeded DAG (up to 3 parents per node, from lower indices).  Each workload runs in a child process of
its own under a time limit; its exit code and last stderr lines are recorded, so a child that dies
shows in the JSON, and no further child is started after one that did not exit 0.

Per workload: kernel ms (fbn_ci_last_kernel_ms: table zeroing + counting, median of the timed calls),
wall ms per synchronous fbn_param_counts call (20 warm-up + 100 timed calls, host clock around calls
that end in a stream synchronise), the bytes model sum_v (1 + k_v) N + 8 cells and its share of
8 TB/s at the kernel time, and the baseline's wall ms per pass over all families (2 warm-up + 10 timed
passes; one fbn_ci_counts call per family -- a single call with a preallocated buffer, not
IndependenceTest.counts' size query + call, which would launch twice).  Both sides are checked
against np.bincount before anything is timed."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BYTES_PER_S = 8e12
LIMITS = {"alarm": 240, "c5": 420}  # seconds per child


def bincount_counts(cols, dims, parents):
    out = []
    for v, ps in enumerate(parents):
        ps = sorted(ps)
        npc = int(np.prod(dims[ps], dtype=np.int64))
        key = cols[v].astype(np.int64) * npc
        stride = 1
        for q in reversed(ps):
            key += stride * cols[q].astype(np.int64)
            stride *= int(dims[q])
        out.append(np.bincount(key, minlength=int(dims[v]) * npc).astype(np.int64))
    return out


def workload(name):
    import fastbn_amd as F
    from fastbn_amd import synth
    if name == "alarm":
        ds = F.Dataset(os.path.join(REPO, "tests", "golden", "alarm", "alarm_s5000.txt"))
        ci = F.IndependenceTest(ds)
        pc = F.PCStable(0.05, 1000).StructLearnCompData(ci)
        return ds.columns, ds.dims, F.pdag_to_dag(ds.num_vars, pc.oriented), ci
    cols, dims = synth.config5_dataset()
    rng = np.random.default_rng(20251019)
    parents = [sorted(int(q) for q in rng.choice(v, size=int(rng.integers(0, min(3, v) + 1)), replace=False))
               for v in range(cols.shape[0])]
    return cols, dims, parents, F.IndependenceTest(F.Dataset(columns=cols, dims=dims))


def child(name):
    import fastbn_amd as F
    from fastbn_amd.api import lib, _p, _csr_parents
    cols, dims, parents, ci = workload(name)
    dims = np.ascontiguousarray(dims, np.int32)
    V, N = cols.shape
    ref = bincount_counts(cols, dims, parents)
    pl = F.ParameterLearning(ci)
    got = pl.counts(parents)
    assert all(np.array_equal(g.reshape(-1), r) for g, r in zip(got, ref)), "fbn_param_counts differs from np.bincount"
    cells = int(sum(r.size for r in ref))
    off, par = _csr_parents(parents, V)
    buf = np.zeros(cells, np.int64)
    total = C.c_int64()

    def one_call():
        lib.fbn_param_counts(ci._h, _p(off), _p(par), _p(buf), cells, C.byref(total))

    for _ in range(20):
        one_call()
    wall, kern = [], []
    for _ in range(100):
        t0 = time.perf_counter()
        one_call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(pl.last_kernel_ms())

    # the baseline: one synchronous launch per family with a parent (x = the node, y = its first
    # parent, z = the rest), np.bincount for roots
    fam = [(v, sorted(ps)) for v, ps in enumerate(parents) if ps]
    roots = [v for v, ps in enumerate(parents) if not ps]
    zs = [np.ascontiguousarray(ps[1:] or [0], np.int32) for _, ps in fam]
    outs = [np.zeros(r.size, np.int32) for r in (ref[v] for v, _ in fam)]
    nc = C.c_int64()

    def baseline_pass():
        for (v, ps), z, o in zip(fam, zs, outs):
            lib.fbn_ci_counts(ci._h, v, ps[0], _p(z) if len(ps) > 1 else None, len(ps) - 1, _p(o), o.size, C.byref(nc))
        return [np.bincount(cols[v], minlength=int(dims[v])) for v in roots]

    rc = baseline_pass()
    assert all(np.array_equal(a, ref[v]) for a, v in zip(rc, roots))
    for (v, ps), o in zip(fam, outs):  # N[z][x][y] -> counts[x][y, z...]: the same multiset per family
        shape = [int(dims[q]) for q in ps[1:]] + [int(dims[v]), int(dims[ps[0]])]
        k = len(ps) - 1
        t = o.reshape(shape).transpose([k, k + 1] + list(range(k))).reshape(-1)
        assert np.array_equal(t, ref[v]), f"fbn_ci_counts differs from np.bincount at family {v}"
    baseline_pass()
    base = []
    for _ in range(10):
        t0 = time.perf_counter()
        baseline_pass()
        base.append((time.perf_counter() - t0) * 1e3)

    model = int(sum((1 + len(ps)) * N for ps in parents) + 8 * cells)
    kms, wms, bms = float(np.median(kern)), float(np.median(wall)), float(np.median(base))
    print(json.dumps({
        "workload": name, "nvars": int(V), "nsamples": int(N), "families_with_parents": len(fam), "roots": len(roots),
        "max_parents": max(len(ps) for ps in parents), "cells": cells, "largest_family_cells": int(max(r.size for r in ref)),
        "kernel_ms_median": kms, "kernel_ms_min": float(np.min(kern)),
        "wall_ms_per_call_median": wms, "wall_ms_per_call_min": float(np.min(wall)), "timed_calls": len(wall),
        "model_bytes": model, "model_gb_per_s_at_kernel_ms": model / (kms * 1e-3) / 1e9,
        "fraction_of_8tbps": model / (kms * 1e-3) / HBM_BYTES_PER_S,
        "baseline_wall_ms_per_pass_median": bms, "baseline_wall_ms_per_pass_min": float(np.min(base)),
        "baseline_passes": len(base), "baseline_launches_per_pass": len(fam),
        "speedup_wall_baseline_over_new": bms / wms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "param", "param_counts.json"))
    ap.add_argument("--workloads", default="alarm,c5")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    results = []
    for name in a.workloads.split(","):
        rec = {"workload": name, "time_limit_s": LIMITS[name]}
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True,
                               text=True, timeout=LIMITS[name])
            rec["exit_code"] = r.returncode
            rec["stderr_tail"] = r.stderr.strip().split("\n")[-8:] if r.stderr.strip() else []
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
        json.dump({"tool": "tools/param_time.py", "hbm_bytes_per_s": HBM_BYTES_PER_S, "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
