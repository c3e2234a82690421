"""Timing of the adaptive samplers (ais.hip's sample_ais_kernel) beside likelihood weighting
(sample.hip) and EPIS-BN's sampling kernel (epis.hip) at the same total draws per case.

    python tools/ais_time.py [--out profiles/ais/ais_time.json] [--workloads ais_alarm_100k,...]

Workloads (tools/epis_time.py's three, with a schedule each): ais_alarm_100k = ALARM, 100,000 cases, S = 64
after 2 stages of 64; ais_alarm_1k = ALARM, 1,000 cases, S = 10,000 after the reference's default 10
stages of 2,500; ais_munin = Munin-like (1041 variables), 1,000 cases, S = 1,024 after 4 stages of 256.
Default cutoff.  Evidence: the seeded generator's cases (7 observed for ALARM, 208 for Munin-like).
Each workload runs in a child process of its own under a time limit; its exit code and last stderr
lines are recorded, and no further child is started after one that did not exit 0.

Per workload: AIS-BN's kernel ms (fbn_ais_last_kernel_ms: HIP events, median of 5 timed calls after 2
warm-up calls), draws/s over all T = m l + S draws per case, wall ms per synchronous call with host
buffers; the same kernel with m = 0 and S = T (no count phase, no update: the difference is the share
of the two learning phases); SIS at S = T with the same m and l; likelihood weighting and EPIS-BN's
sampling kernel (no pre-propagation) at S = T; the state's home and the grid; the median ess / S of
AIS-BN's counted samples, of its first stage and of LW.  The first 16 cases are checked against the
host twin bit for bit (log_evidence to 1e-15 relative) before anything is timed."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from epis_time import network, timed  # noqa: E402

# name -> (network, cases, S, m, l, observed per case)
WORK = {"ais_alarm_100k": ("alarm", 100_000, 64, 2, 64, 7), "ais_alarm_1k": ("alarm", 1_000, 10_000, 10, 2_500, 7),
        "ais_munin": ("munin", 1_000, 1_024, 4, 256, 208)}
LIMITS = {"ais_alarm_100k": 240, "ais_alarm_1k": 240, "ais_munin": 400}


def child(name):
    import fastbn_amd as F
    which, ncases, S, m, l, k = WORK[name]
    with tempfile.TemporaryDirectory() as tmp:
        net = network(which, tmp)
    ev = net.evidence_cases(ncases, k, seed=1)
    dev = F.AISBN(net, S, max_updates=m, interval=l, seed=0)
    T = dev.draws_per_case
    for cls in (F.AISBN, F.SelfImportanceSampling):
        d, h = cls(net, S, m, l, seed=0), cls(net, S, m, l, seed=0, device=-1)
        lab, marg = d.infer(ev[:16])
        hlab, hmarg = h.infer(ev[:16])
        assert np.array_equal(lab, hlab) and np.array_equal(marg.view(np.uint64), hmarg.view(np.uint64)), \
            "device differs from the host twin"
        assert all(np.array_equal(d.stats[i], h.stats[i]) for i in (1, 2, 3))
        assert np.allclose(d.stats[0], h.stats[0], rtol=1e-15, atol=0)
        d.close()
    wall, kern = timed(lambda: dev.infer(ev), dev.last_kernel_ms)
    le, ess, upd, ess0 = dev.stats
    flat = F.AISBN(net, T, max_updates=0, interval=l, seed=0)  # the same draws without the learning phases
    _, flat_kern = timed(lambda: flat.infer(ev), flat.last_kernel_ms)
    sis = F.SelfImportanceSampling(net, T, max_updates=m, interval=l, seed=0)
    _, sis_kern = timed(lambda: sis.infer(ev), sis.last_kernel_ms)
    lw = F.LikelihoodWeighting(net, T, seed=0)
    _, lw_kern = timed(lambda: lw.infer(ev), lw.last_kernel_ms)
    ep = F.EPISBN(net, T, iterations=0, seed=0)
    _, ep_kern = timed(lambda: ep.infer(ev), ep.last_kernel_ms)
    kern, flat_kern, sis_kern, lw_kern, ep_kern = float(kern), float(flat_kern), float(sis_kern), float(lw_kern), float(ep_kern[1])
    rec = {"workload": name, "nvars": net.num_nodes, "ncases": ncases, "samples_per_case": S, "max_updates": m,
           "interval": l, "draws_per_case": T, "observed_per_case": k, **dev.info(ncases),
           "kernel_ms_median": kern, "wall_ms_per_call_median": wall, "draws_per_s_kernel": ncases * T / (kern * 1e-3),
           "kernel_ms_no_learning_same_draws": flat_kern, "learning_phases_share": (kern - flat_kern) / kern,
           "sis_kernel_ms_same_draws": sis_kern, "lw_kernel_ms_same_draws": lw_kern,
           "epis_sampling_kernel_ms_same_draws": ep_kern, "ratio_over_lw_kernel": kern / lw_kern,
           "ratio_over_epis_sampling_kernel": kern / ep_kern,
           "ess_over_S_median": float(np.median(ess)) / S, "first_stage_ess_over_n_median": float(np.median(ess0)),
           "lw_ess_over_T_median": float(np.median(lw.stats[1])) / T, "updates_applied_median": float(np.median(upd)),
           "log_evidence_min": float(le.min())}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ais", "ais_time.json"))
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
        json.dump({"tool": "tools/ais_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
