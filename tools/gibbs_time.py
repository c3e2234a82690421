"""Timing and accuracy of Gibbs sampling (gibbs.hip) beside likelihood weighting and AIS-BN at equal draws.

    python tools/gibbs_time.py [--out profiles/gibbs/gibbs_time.json]

Workloads, both on ALARM with chains = 64, burn_in = 64, sweeps = 256 unless said otherwise:
  gibbs_alarm_1k     the fixture's 1,000 cases (testing_alarm_1k_p20).  Draws per case: chains * (burn_in +
                     sweeps) = 20,480 sweeps of the unobserved variables; likelihood weighting gets S = 20,480
                     samples, AIS-BN 10 updates of 512 samples and 15,360 counted ones (20,480 in all).
                     Accuracy: the average Hellinger distance (fbn_score_marginals) to the junction tree's exact
                     marginals of the same cases, and the accuracy of the query label.
  gibbs_one_case_64k one case (the fixture's first) with 2^16 chains: 1,024 units, the same work as 1,024 cases.
Every Gibbs figure is taken twice, with the parent-configuration cache off and on (set_tuning), the two
alternating call by call: kernel ms (fbn_gibbs_last_kernel_ms: HIP events around the sampling launch and its
finish; median and minimum of 8 timed calls after 2 warm-up calls) and the wall ms of the synchronous call
with host buffers.  Rates are chain-sweeps (one chain, one sweep of the unobserved variables) per second of
kernel time.  The first 8 cases are checked against the host twin bit for bit before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ALARM = os.path.join(REPO, "tests", "golden", "alarm")
CHAINS, BURN_IN, SWEEPS = 64, 64, 256


def timed(calls, warm=2, reps=8):
    """calls: name -> (run, kernel_ms); alternates them call by call -> name -> dict of medians and minima."""
    for _ in range(warm):
        for run, _ in calls.values():
            run()
    wall = {k: [] for k in calls}
    kern = {k: [] for k in calls}
    for _ in range(reps):
        for k, (run, ms) in calls.items():
            t0 = time.perf_counter()
            run()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            kern[k].append(ms())
    return {k: {"kernel_ms_median": float(np.median(kern[k])), "kernel_ms_min": float(np.min(kern[k])),
                "wall_ms_per_call_median": float(np.median(wall[k]))} for k in calls}


def gibbs_pair(F, net, ev, chains):
    """Two handles, the cache off and on -> (their timing records with info and rate, the handles)."""
    hs = {}
    for name, pc in (("pc_cache_off", 0), ("pc_cache_on", 1)):
        h = F.GibbsSampling(net, chains, SWEEPS, BURN_IN, seed=0)
        h.set_tuning(pc_cache=pc)
        hs[name] = h
    rec = timed({k: ((lambda h=h: h.infer(ev)), h.last_kernel_ms) for k, h in hs.items()})
    for k, h in hs.items():
        rec[k].update(h.info(len(ev)))
        rec[k]["chain_sweeps_per_s_kernel"] = len(ev) * chains * (BURN_IN + SWEEPS) / (rec[k]["kernel_ms_median"] * 1e-3)
    return rec, hs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gibbs", "gibbs_time.json"))
    a = ap.parse_args()
    import fastbn_amd as F
    net = F.Network(os.path.join(ALARM, "alarm.xml"))
    ev, truth = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), net.num_nodes)
    n, draws = len(ev), CHAINS * (BURN_IN + SWEEPS)
    host = F.GibbsSampling(net, CHAINS, 5, 3, seed=0, device=-1).infer(ev[:8], states=True)
    dev = F.GibbsSampling(net, CHAINS, 5, 3, seed=0).infer(ev[:8], states=True)
    assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(host, dev)), \
        "device differs from the host twin"
    _, exact = F.JunctionTree(net).infer(ev)

    def accuracy(lab, marg):
        return {"hd_average": F.score_marginals(net, marg, exact)[1] / n, "label_accuracy": float(np.mean(lab == truth))}

    one, hs = gibbs_pair(F, net, ev, CHAINS)
    one["pc_cache_on"].update(accuracy(*hs["pc_cache_on"].infer(ev)))  # the setting does not change the bits
    lw = F.LikelihoodWeighting(net, draws, seed=0)
    ais = F.AISBN(net, draws - 10 * 512, max_updates=10, interval=512, seed=0)
    others = timed({"likelihood_weighting": (lambda: lw.infer(ev), lw.last_kernel_ms), "ais_bn": (lambda: ais.infer(ev), ais.last_kernel_ms)})
    others["likelihood_weighting"].update(accuracy(*lw.infer(ev)), ess_over_S_median=float(np.median(lw.stats[1])) / draws)
    others["ais_bn"].update(accuracy(*ais.infer(ev)), ess_over_S_median=float(np.median(ais.stats[1])) / (draws - 5120))
    big, _ = gibbs_pair(F, net, ev[:1], 1 << 16)
    out = {"tool": "tools/gibbs_time.py", "network": "alarm", "nvars": net.num_nodes, "chains": CHAINS, "burn_in": BURN_IN,
           "sweeps": SWEEPS, "draws_per_case": draws,
           "workloads": [{"workload": "gibbs_alarm_1k", "ncases": n, "gibbs": one, **others},
                         {"workload": "gibbs_one_case_64k", "ncases": 1, "chains": 1 << 16, "gibbs": big}]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
