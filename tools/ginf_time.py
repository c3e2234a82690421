"""Timing of exact Gaussian inference (ginf.hip behind fbn_ginf_*).

    python tools/ginf_time.py [--out profiles/ginf/ginf_time.json] [--nvars 1000] [--observed 32] [--ncases 4096]

Workload: a seeded sparse linear-Gaussian network of --nvars variables (at most two parents a node), --ncases
evidence rows with --observed observed variables each, every row a pattern of its own.  The measurement runs in a
child process under a time limit; its exit code and last stderr lines are recorded.

Reported: the kernel time of the batch on device buffers (HIP events around the launch), the median of RUNS timed
repetitions after one warm-up, with the launch's LDS bytes, tile and grid; the wall time of the same batch through
host buffers; and the wall time of the host twin on the first --twin-cases rows, whose bits are compared."""
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
LIMIT_S = 600


def network(n, rng):
    parents, coef = [[]], [[]]
    for v in range(1, n):
        ps = rng.choice(np.arange(max(0, v - 8), v), size=min(v, int(rng.integers(0, 3))), replace=False)
        parents.append([int(p) for p in ps])
        coef.append(list(rng.uniform(0.3, 1.0, len(ps)) * rng.choice([-1.0, 1.0], len(ps))))
    return parents, rng.normal(size=n), coef, rng.uniform(0.5, 2.0, n)


def child(n, m, ncases, twin_cases):
    import torch

    import fastbn_amd as F
    rng = np.random.default_rng(1)
    net = F.GaussianNetwork(*network(n, rng))
    mu, S = net.joint()
    ev = np.full((ncases, n), np.nan)
    for c in range(ncases):
        E = rng.permutation(n)[:m]
        ev[c, E] = mu[E] + np.sqrt(np.diag(S)[E]) * rng.normal(size=m)
    dev = F.GaussianInference(net)
    d_ev = torch.from_numpy(ev).cuda()
    d_mean, d_var = torch.empty_like(d_ev), torch.empty_like(d_ev)
    d_logp = torch.empty(ncases, dtype=torch.float64, device="cuda")
    ms = []
    for rep in range(RUNS + 1):
        dev.run_device(d_ev.data_ptr(), ncases, d_mean.data_ptr(), d_var.data_ptr(), d_logp.data_ptr())
        torch.cuda.synchronize()
        if rep:
            ms.append(dev.last_kernel_ms())
    rec = {"nvars": n, "observed": m, "ncases": ncases, "timed_runs": RUNS, "kernel_ms": float(np.median(ms)), **dev.info()}
    t0 = time.perf_counter()
    out = dev.infer(ev)
    rec["host_buffers_wall_s"] = time.perf_counter() - t0
    k = min(twin_cases, ncases)
    t0 = time.perf_counter()
    ref = F.GaussianInference(net, device=-1).infer(ev[:k])
    rec["twin_cases"], rec["twin_wall_s"] = k, time.perf_counter() - t0
    rec["twin_bits_equal"] = bool(all((o[:k].view(np.int64) == r.view(np.int64)).all() for o, r in zip(out, ref)))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ginf", "ginf_time.json"))
    ap.add_argument("--nvars", type=int, default=1000)
    ap.add_argument("--observed", type=int, default=32)
    ap.add_argument("--ncases", type=int, default=4096)
    ap.add_argument("--twin-cases", type=int, default=64)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.nvars, a.observed, a.ncases, a.twin_cases)
        return 0
    rec = {"workload": f"ginf_n{a.nvars}_m{a.observed}_c{a.ncases}", "time_limit_s": LIMIT_S}
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--nvars", str(a.nvars), "--observed", str(a.observed),
               "--ncases", str(a.ncases), "--twin-cases", str(a.twin_cases)]
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
        json.dump({"tool": "tools/ginf_time.py", "workloads": [rec]}, f, indent=1)
        f.write("\n")
    return 0 if rec["exit_code"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
