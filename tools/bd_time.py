"""Timing of the Bayesian Dirichlet reduction (hc_bd.hip behind fbn_hc_run_bd) beside the BIC reduction.

    python tools/bd_time.py [--out profiles/hc/bd_time.json] [--workloads bd_alarm_5000,bd_config5_100k]

Method and workloads are tools/hc_time.py's: ALARM-5000 (37 variables, the whole search from the empty graph)
and config 5 (synth.config5_dataset(): 1,000 variables x 100,000 samples, the search capped at MAX_ITER
operations).  Each workload runs in a child process of its own under a time limit; no further child is
started after one that did not exit 0.

Per workload, on one context and in one process, the scores alternating run by run after one warm-up run
each (medians over the timed runs):
  * the whole search under "bic" and under "bde" (iss = 1): first-sweep kernel ms (HIP events around zeroing +
    counting + reduction of the one batch of all one-parent families), kernel ms of all batches, wall ms of
    the search.  The events do not separate the reduction from the counting it follows, so the reduction
    alone is not measured; bde_minus_bic_first_sweep_kernel_ms is the difference of two sweeps that count
    the same tables.
  * the first sweep alone (max_iter = 0) under "bde" with fbn_bd_set_tuning's pack = 0 (one wave per family)
    and pack = 1 (narrow families packed into one wave), alternating, SWEEPS repeats each; the node scores of
    the two are compared bit for bit."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LIMITS = {"bd_alarm_5000": 120, "bd_config5_100k": 500}
MAX_ITER = 5000
RUNS = {"bd_alarm_5000": 5, "bd_config5_100k": 2}
SWEEPS = {"bd_alarm_5000": 20, "bd_config5_100k": 5}


def med(infos, key):
    return float(np.median([i[key] for i in infos]))


def child(name):
    import fastbn_amd as F
    from fastbn_amd import synth
    if name == "bd_alarm_5000":
        ds = F.Dataset(os.path.join(REPO, "tests", "golden", "alarm", "alarm_s5000.txt"))
        max_iter = None
    else:
        cols, dims = synth.config5_dataset()
        ds = F.Dataset(columns=cols, dims=dims)
        max_iter = MAX_ITER
    ci = F.IndependenceTest(ds)
    learners = {"bic": F.HillClimbing("bic", max_iter=max_iter), "bde": F.HillClimbing(("bde", 1), max_iter=max_iter)}
    for hc in learners.values():
        hc.learn(ci)  # warm-up: code objects, the n ln n table, the buffers at their final sizes
    infos = {k: [] for k in learners}
    for _ in range(RUNS[name]):
        for k, hc in learners.items():
            infos[k].append(dict(hc.learn(ci).info))
    rec = {"workload": name, "nvars": ds.num_vars, "nsamples": ds.num_instance, "max_iter": max_iter,
           "timed_runs": RUNS[name], "warm_up_runs": 1, "search": {}}
    for k, hc in learners.items():
        rec["search"][k] = {"iterations": hc.iterations, "arcs": sum(len(p) for p in hc.parents), "score": hc.score,
                            "families_scored": hc.families_scored, "batches": hc.info["batches"],
                            "first_sweep_kernel_ms": med(infos[k], "first_sweep_kernel_ms"),
                            "kernel_ms": med(infos[k], "kernel_ms"), "search_wall_ms": med(infos[k], "wall_ms")}
    rec["bde_minus_bic_first_sweep_kernel_ms"] = (rec["search"]["bde"]["first_sweep_kernel_ms"] -
                                                  rec["search"]["bic"]["first_sweep_kernel_ms"])
    sweep = F.HillClimbing(("bde", 1), max_iter=0)
    times, scores = {0: [], 1: []}, {}
    try:
        for rep in range(SWEEPS[name] + 1):  # repeat 0 warms both paths up
            for pack in (0, 1):
                F.HillClimbing.set_bd_tuning(ci, pack)
                sweep.learn(ci)
                scores[pack] = sweep.node_scores.tobytes()
                if rep:
                    times[pack].append(sweep.info["first_sweep_kernel_ms"])
    finally:
        F.HillClimbing.set_bd_tuning(ci, 1)
    assert scores[0] == scores[1], "pack = 0 and pack = 1 differ"
    rec["first_sweep_bde"] = {"families": sweep.families_scored, "repeats": SWEEPS[name],
                              "pack0_kernel_ms": {"median": float(np.median(times[0])), "min": min(times[0]), "max": max(times[0])},
                              "pack1_kernel_ms": {"median": float(np.median(times[1])), "min": min(times[1]), "max": max(times[1])}}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hc", "bd_time.json"))
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
        json.dump({"tool": "tools/bd_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
