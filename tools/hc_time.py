"""Timing of score-based structure learning (hc_score.hip behind fbn_hc_run) beside its host twin.

    python tools/hc_time.py [--out profiles/hc/hc_time.json] [--workloads hc_alarm_5000,hc_config5_100k]

Workloads: hc_alarm_5000 = tests/golden/alarm/alarm_s5000.txt (37 variables, 5,000 samples), the whole
search under BIC from the empty graph; hc_config5_100k = synth.config5_dataset() (1,000 variables, 100,000
samples), the search capped at MAX_ITER operations (each operation scans the 10^6 cached deltas on the host);
the record says whether the cap was reached.  Each workload runs in a child process of its own under a time limit; its exit code
and last stderr lines are recorded, and no further child is started after one that did not exit 0.

Per workload, from fbn_hc_info (median over the timed runs after one warm-up run): kernel and wall ms of the
first sweep (all one-parent families, one batch), of the rescoring batches after it (per batch), the wall
time inside the scorer, and of the whole search; the host loop's share is the rest.  The host twin
(fbn_hc_run_host, one thread) runs the same search on ALARM, where its trace is checked against the
device's; on config5 only one row of its first sweep is timed (the 999 one-parent families of node 0) and
the sweep's time is that row's times 1,000 -- scaled, not measured."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LIMITS = {"hc_alarm_5000": 120, "hc_config5_100k": 400}
MAX_ITER = 5000
RUNS = {"hc_alarm_5000": 5, "hc_config5_100k": 1}


def summary(infos):
    med = lambda k: float(np.median([i[k] for i in infos]))  # noqa: E731
    b = infos[0]["batches"]
    rest_k = med("kernel_ms") - med("first_sweep_kernel_ms")
    rest_w = med("score_wall_ms") - med("first_sweep_wall_ms")
    return {"batches": b, "families_scored": infos[0]["families_scored"], "iterations": infos[0]["iterations"],
            "arcs": infos[0]["narcs"], "score": infos[0]["score"],
            "first_sweep_kernel_ms": med("first_sweep_kernel_ms"), "first_sweep_wall_ms": med("first_sweep_wall_ms"),
            "rescoring_kernel_ms_per_batch": rest_k / max(b - 1, 1), "rescoring_wall_ms_per_batch": rest_w / max(b - 1, 1),
            "kernel_ms": med("kernel_ms"), "scorer_wall_ms": med("score_wall_ms"), "search_wall_ms": med("wall_ms"),
            "host_loop_wall_ms": med("wall_ms") - med("score_wall_ms")}


def child(name):
    import fastbn_amd as F
    from fastbn_amd import synth
    if name == "hc_alarm_5000":
        ds = F.Dataset(os.path.join(REPO, "tests", "golden", "alarm", "alarm_s5000.txt"))
        max_iter = None
    else:
        cols, dims = synth.config5_dataset()
        ds = F.Dataset(columns=cols, dims=dims)
        max_iter = MAX_ITER
    t0 = time.perf_counter()
    ci = F.IndependenceTest(ds)
    upload_ms = (time.perf_counter() - t0) * 1e3
    hc = F.HillClimbing("bic", max_iter=max_iter)
    if name == "hc_alarm_5000":
        hc.learn(ci)  # warm-up: the n ln n table is built and uploaded by the first call
    infos = []
    for _ in range(RUNS[name]):
        infos.append(dict(hc.learn(ci).info))
    rec = {"workload": name, "nvars": ds.num_vars, "nsamples": ds.num_instance, "score_name": "bic",
           "max_iter": max_iter, "capped_by_max_iter": bool(max_iter is not None and hc.iterations == max_iter),
           "timed_runs": RUNS[name], "warm_up_runs": 1 if name == "hc_alarm_5000" else 0, "upload_wall_ms": upload_ms,
           "device": summary(infos)}
    if name == "hc_alarm_5000":
        host = F.HillClimbing("bic")
        hinfos = [dict(host.learn(ds, host=True).info) for _ in range(RUNS[name])]
        assert host.trace == hc.trace and host.score == hc.score, "device differs from the host twin"
        rec["host_twin"] = summary(hinfos)
    else:
        fams = [(0, x) for x in range(1, ds.num_vars)]
        dev = F.family_scores(ci, fams, F.hc_penalty("bic", ds.num_instance))
        t0 = time.perf_counter()
        ref = F.family_scores(ds, fams, F.hc_penalty("bic", ds.num_instance))
        row_ms = (time.perf_counter() - t0) * 1e3
        assert dev[1].tobytes() == ref[1].tobytes(), "device differs from the host twin"
        rec["host_twin"] = {"first_sweep_row_wall_ms": row_ms, "first_sweep_wall_ms_scaled": row_ms * ds.num_vars,
                            "note": "one row of 999 one-parent families timed (fbn_score_families_host, which also "
                                    "checks the column store and builds the n ln n table); the sweep is that times "
                                    "1,000, scaled, not measured; the whole search was not run on the host"}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hc", "hc_time.json"))
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
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
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
        json.dump({"tool": "tools/hc_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
