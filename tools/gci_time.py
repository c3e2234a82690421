"""Timing of the Gaussian CI path (gci_corr.hip, gci_test.hip behind fbn_gci_*).

    python tools/gci_time.py [--out profiles/gci/gci_time.json] [--nvars 1000] [--nsamples 100000]

Workload: a seeded sparse linear-Gaussian SEM (about 1.5 parents per variable) of --nvars variables x
--nsamples samples, float64.  The measurement runs in a child process under a time limit; its exit code and last
stderr lines are recorded.

Reported, each the median of RUNS timed repetitions after one warm-up: the kernel time of the column means, the
Gram and the reduce (HIP events around each launch; the automatic tile and split-K, and every --tiles x --splits
setting, the repetitions alternating over the settings); torch.matmul in float64 on the same centred matrix on
the same device (torch events; the library GEMM does the full square, the Gram kernel the upper tiles only);
a PC-stable run of levels 0..3 on the resident context (wall, device kernels, tests per level)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

RUNS = 5
DEPTH = 4  # levels 0..3 of the PC run (at 100,000 samples the sparse SEM's skeleton search goes deeper than 8)
LIMIT_S = 900


def sem(nvars, N, seed):
    rng = np.random.default_rng(seed)
    X = np.zeros((nvars, N))
    for j in range(nvars):
        X[j] = rng.standard_normal(N)
        for i in rng.choice(j, size=min(j, rng.poisson(1.5)), replace=False) if j else ():
            X[j] += rng.uniform(0.4, 0.9) * rng.choice([-1.0, 1.0]) * X[i]
    return X


def child(nvars, N, tiles, splits):
    import torch

    import fastbn_amd as F
    X = sem(nvars, N, seed=1)
    t0 = time.perf_counter()
    ci = F.GaussianIndependenceTest(F.ContinuousDataset(columns=X))
    rec = {"nvars": nvars, "nsamples": N, "timed_runs": RUNS, "upload_and_first_R_wall_s": time.perf_counter() - t0}
    settings = [(0, 0)] + [(s, t) for t in tiles for s in splits]
    times = {st: [] for st in settings}
    ref = None
    for rep in range(RUNS + 1):  # alternating, so that drift falls on every setting alike; repetition 0 warms up
        for st in settings:
            ci.set_tuning(*st)
            if rep:
                times[st].append(ci.corr_kernel_ms() + (ci.info()["split_k"], ci.info()["tile"]))
            if st == (0, 0) and ref is None:
                ref = ci.correlation()
    rec["corr"] = [{"split_k": v[0][3], "tile": v[0][4], "requested": list(st), "means_ms": float(np.median([x[0] for x in v])),
                    "gram_ms": float(np.median([x[1] for x in v])), "reduce_ms": float(np.median([x[2] for x in v]))}
                   for st, v in times.items()]
    rec["max_abs_dev_from_numpy"] = float(np.abs(ref - np.corrcoef(X)).max()) if nvars * N <= 2e8 else None
    ci.set_tuning(0, 0)
    # the library GEMM on the same centred matrix
    dev = torch.device("cuda", 0)
    Xc = torch.from_numpy(X - X.mean(axis=1, keepdims=True)).to(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    mm = []
    for rep in range(RUNS + 1):
        ev[0].record()
        G = torch.matmul(Xc, Xc.T)
        ev[1].record()
        torch.cuda.synchronize()
        if rep:
            mm.append(ev[0].elapsed_time(ev[1]))
    rec["torch_matmul_f64_ms"] = float(np.median(mm))
    del G, Xc
    pcs = []
    for rep in range(RUNS + 1):
        t0 = time.perf_counter()
        pc = F.PCStable(0.05, depth=DEPTH).StructLearnCompData(ci)
        if rep:
            pcs.append((time.perf_counter() - t0, pc.kernel_s))
    rec["pc"] = {"depth": DEPTH, "wall_s": float(np.median([p[0] for p in pcs])), "kernel_s": float(np.median([p[1] for p in pcs])),
                 "tests_per_level": [int(t) for t in pc.tests_per_level], "launched_per_level": [int(t) for t in pc.launched_per_level],
                 "edges": len(pc.edges), "min_margin": pc.min_margin, "degenerate": pc.result.degenerate}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gci", "gci_time.json"))
    ap.add_argument("--nvars", type=int, default=1000)
    ap.add_argument("--nsamples", type=int, default=100000)
    ap.add_argument("--tiles", default="32,64")
    ap.add_argument("--splits", default="1,2,4,8")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.nvars, a.nsamples, [int(t) for t in a.tiles.split(",") if t], [int(s) for s in a.splits.split(",") if s])
        return 0
    rec = {"workload": f"gci_sem{a.nvars}_{a.nsamples}", "time_limit_s": LIMIT_S}
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--nvars", str(a.nvars), "--nsamples", str(a.nsamples),
               "--tiles", a.tiles, "--splits", a.splits]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S)
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
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/gci_time.py", "workloads": [rec]}, f, indent=1)
        f.write("\n")
    return 0 if rec["exit_code"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
