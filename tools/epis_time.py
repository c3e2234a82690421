"""Timing of EPIS-BN (lbp.hip's pre-propagation, then epis.hip's sample_epis_kernel) beside likelihood
weighting (sample.hip) at the same samples per case, and its accuracy where an exact answer is cheap.

    python tools/epis_time.py [--out profiles/epis/epis_time.json] [--workloads epis_alarm_100k,...]

Workloads: epis_alarm_100k = ALARM, 100,000 cases x 64 samples; epis_alarm_1k = ALARM, 1,000 cases x
10,000 samples; epis_munin = Munin-like (1041 variables), 1,000 cases x 1,024 samples.  20 LBP
iterations (10 for Munin-like), default cutoff.  Evidence: the seeded generator's cases (7 observed
for ALARM, 208 for Munin-like).  Each workload runs in a child process of its own under a time limit;
its exit code and last stderr lines are recorded, and no further child is started after one that did
not exit 0.

Per workload: the LBP and the sampling kernel ms (fbn_epis_last_kernel_ms: HIP events, median of 5
timed calls after 2 warm-up calls), wall ms per synchronous call with host buffers (it includes the
copy of the result to the host), the same two figures for likelihood weighting, the median ess / S of
both, and for ALARM the average Hellinger distance of both to the junction tree's exact marginals on
the first 1,000 cases.  The first 16 cases are checked against the host twin bit for bit (log_evidence
to 1e-15 relative) before anything is timed."""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GOLD = os.path.join(REPO, "tests", "golden")
# name -> (network, cases, samples per case, LBP iterations, observed per case)
WORK = {"epis_alarm_100k": ("alarm", 100_000, 64, 20, 7), "epis_alarm_1k": ("alarm", 1_000, 10_000, 20, 7),
        "epis_munin": ("munin", 1_000, 1_024, 10, 208)}
LIMITS = {"epis_alarm_100k": 240, "epis_alarm_1k": 240, "epis_munin": 300}


def network(name, tmp):
    import fastbn_amd as F
    if name == "alarm":
        return F.Network(os.path.join(GOLD, "alarm", "alarm.xml"))
    xml = os.path.join(tmp, name + ".xml")
    with gzip.open(os.path.join(GOLD, "munin_like", "munin_like.xml.gz"), "rb") as f, open(xml, "wb") as g:
        g.write(f.read())
    return F.Network(xml)


def timed(run, kernel_ms, warm=2, reps=5):
    for _ in range(warm):
        run()
    wall, kern = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(kernel_ms())
    return float(np.median(wall)), np.median(np.array(kern, np.float64), axis=0)


def child(name):
    import fastbn_amd as F
    which, ncases, S, iters, k = WORK[name]
    with tempfile.TemporaryDirectory() as tmp:
        net = network(which, tmp)
    ev = net.evidence_cases(ncases, k, seed=1)
    dev = F.EPISBN(net, S, iterations=iters, seed=0)
    host = F.EPISBN(net, S, iterations=iters, seed=0, device=-1)
    lab, marg = dev.infer(ev[:16])
    hlab, hmarg = host.infer(ev[:16])
    assert np.array_equal(lab, hlab) and np.array_equal(marg.view(np.uint64), hmarg.view(np.uint64)), \
        "device differs from the host twin"
    assert np.array_equal(dev.stats[1], host.stats[1]) and np.array_equal(dev.stats[2], host.stats[2])
    assert np.allclose(dev.stats[0], host.stats[0], rtol=1e-15, atol=0)
    wall, kern = timed(lambda: dev.infer(ev), dev.last_kernel_ms)
    le, ess, used, res = dev.stats
    lw = F.LikelihoodWeighting(net, S, seed=0)
    lw_wall, lw_kern = timed(lambda: lw.infer(ev), lw.last_kernel_ms)
    rec = {"workload": name, "nvars": net.num_nodes, "ncases": ncases, "samples_per_case": S, "lbp_iterations": iters,
           "observed_per_case": k, **dev.info(),
           "lbp_kernel_ms_median": float(kern[0]), "sampling_kernel_ms_median": float(kern[1]),
           "wall_ms_per_call_median": wall,
           "samples_per_s_sampling_kernel": ncases * S / (float(kern[1]) * 1e-3),
           "lw_kernel_ms_median": float(lw_kern), "lw_wall_ms_per_call_median": lw_wall,
           "ratio_sampling_over_lw_kernel": float(kern[1]) / float(lw_kern),
           "ess_over_S_median": float(np.median(ess)) / S, "lw_ess_over_S_median": float(np.median(lw.stats[1])) / S,
           "lbp_failed_cases": int(np.isinf(res).sum()), "lbp_iterations_used_median": float(np.median(used)),
           "log_evidence_min": float(le.min()), "lw_log_evidence_min": float(lw.stats[0].min())}
    if which == "alarm":  # accuracy against the exact marginals of the junction tree
        n = min(ncases, 1000)
        _, exact = F.JunctionTree(net).infer(ev[:n])
        rec["hd_average_first_1000"] = F.score_marginals(net, dev.infer(ev[:n])[1], exact)[1] / n
        rec["lw_hd_average_first_1000"] = F.score_marginals(net, lw.infer(ev[:n])[1], exact)[1] / n
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "epis", "epis_time.json"))
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
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True,
                               text=True, timeout=LIMITS[name])
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
        json.dump({"tool": "tools/epis_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
