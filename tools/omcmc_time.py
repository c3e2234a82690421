"""Timing of order MCMC (order_mcmc.hip behind fbn_omcmc_run) on full ALARM, with a sanity figure against the
exact arc posteriors.

    python tools/omcmc_time.py [--out profiles/exact/omcmc_time.json] [--chains 64,1024,4096,16384] [--steps 1000]

Workload: all 37 columns of tests/golden/alarm/alarm_s5000.txt (5,000 samples), at most 3 parents under BDeu
(iss 1), the uniform prior: about 289k families in the lists.  Each chain count runs --steps steps per chain
(burn-in 0, one sample every 100 steps) after one warm-up run of the same shape; the figure is the chain kernel's
device time (HIP events around its launches, fbn_omcmc_info.chain_kernel_ms), median over the timed runs, per
1,000 steps of every chain and per chain-step.  The sanity figure: the first 20 columns, 256 chains of 4,000 steps,
max |arc_prob - ArcPosterior.arc_prob| beside the largest standard error.  Everything runs in one child process
under a time limit; its exit code and last stderr lines are recorded."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LIMIT = 900
RUNS = 3
MAX_PARENTS = 3
SANITY = dict(nvars=20, chains=256, burn_in=2000, thin=20, samples=100, seed=1)


def child(chains, steps):
    import fastbn_amd as F
    full = F.Dataset(os.path.join(REPO, "tests", "golden", "alarm", "alarm_s5000.txt"))
    ci = F.IndependenceTest(full)
    rec = {"nvars": full.num_vars, "nsamples": full.num_instance, "max_parents": MAX_PARENTS, "score_name": "bde", "prior": 0,
           "steps": steps, "timed_runs": RUNS, "chains": []}
    for ch in chains:
        m = F.OrderMCMC("bde", max_parents=MAX_PARENTS, chains=ch, burn_in=0, thin=100, samples=max(steps // 100, 1), seed=1)
        m.learn(ci)  # warm-up: code objects, the scorer's tables
        infos = [dict(m.learn(ci).info) for _ in range(RUNS)]
        ms = float(np.median([i["chain_kernel_ms"] for i in infos]))
        rec["families"] = infos[0]["families"]
        rec["chains"].append({"chains": ch, "chains_per_group": infos[0]["chains_per_group"], "steps": infos[0]["steps"],
                              "chain_kernel_ms": ms, "chain_kernel_ms_runs": [i["chain_kernel_ms"] for i in infos],
                              "kernel_ms_per_1000_steps": ms * 1000.0 / infos[0]["steps"],
                              "ns_per_chain_step": ms * 1e6 / (infos[0]["steps"] * ch),
                              "score_kernel_ms": float(np.median([i["score_kernel_ms"] for i in infos])),
                              "wall_ms": float(np.median([i["wall_ms"] for i in infos])), "accept_rate": float(m.accept_rate.mean())})
    n = SANITY["nvars"]
    part = F.Dataset(columns=np.ascontiguousarray(full.columns[:n]), dims=np.ascontiguousarray(full.dims[:n]))
    pci = F.IndependenceTest(part)
    exact = F.ArcPosterior("bde", max_parents=MAX_PARENTS).learn(pci).arc_prob
    kw = {k: v for k, v in SANITY.items() if k != "nvars"}
    m = F.OrderMCMC("bde", max_parents=MAX_PARENTS, **kw).learn(pci)
    rec["sanity"] = dict(SANITY, max_abs_dev=float(np.abs(m.arc_prob - exact).max()), max_se=float(m.arc_se.max()),
                         chain_kernel_ms=m.info["chain_kernel_ms"], accept_rate=float(m.accept_rate.mean()))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "exact", "omcmc_time.json"))
    ap.add_argument("--chains", default="64,1024,4096,16384")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child([int(c) for c in a.chains.split(",") if c], a.steps)
        return 0
    rec = {"workload": "omcmc_alarm37_5000", "time_limit_s": LIMIT}
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--chains", a.chains, "--steps", str(a.steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT)
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
        json.dump({"tool": "tools/omcmc_time.py", "workloads": [rec]}, f, indent=1)
        f.write("\n")
    return 0 if rec["exit_code"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
