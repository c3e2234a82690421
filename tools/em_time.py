"""Timing of the expectation-maximisation E-step (jt_em.hip) beside the most probable explanation
(jt_mpe.hip) on the same cases, and beside its own host twin (jt_em_host.cpp).

    python tools/em_time.py [--out profiles/em/em_time.json] [--workloads em_alarm_100k_p20,...]

Workloads: em_alarm_100k_p20 / _p70 = ALARM, 100,000 rows with 7 / 26 of 37 variables observed (20 % / 70 %);
em_munin_125k = Munin-like (1041 variables), 125,000 rows with 208 observed.  Rows: the seeded generator's
evidence cases (unobserved = missing).  Each workload runs in a child process of its own under a time limit;
its exit code and last stderr lines are recorded, and no further child is started after one that did not
exit 0.

Per workload: the E-step kernel ms (fbn_em_last_kernel_ms: HIP events around the E-step kernel alone, median
of 8 timed calls after 2 warm-up calls) and rows/s, wall ms per synchronous estep with host buffers (upload,
data check, E-step, reduction, download), MostProbableExplanation's kernel ms on the same cases (median of
8 after 2) and the ratio -- the E-step makes more sweeps than MPE (Collect, the parents' pass for the
downward messages, one pass for Z and one per hosted family against Collect and a partial back-trace) -- and
the host twin's wall ms on the first 4,096 rows scaled to the whole set.  The first 64 rows are checked
against the host twin byte for byte before anything is timed."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from mpe_time import network  # noqa: E402

# name -> (network, rows, observed per row)
WORK = {"em_alarm_100k_p20": ("alarm", 100_000, 7), "em_alarm_100k_p70": ("alarm", 100_000, 26),
        "em_munin_125k": ("munin", 125_000, 208)}
LIMITS = {"em_alarm_100k_p20": 240, "em_alarm_100k_p70": 240, "em_munin_125k": 600}
HOST_ROWS = 4096


def child(name):
    import fastbn_amd as F
    which, ncases, k = WORK[name]
    with tempfile.TemporaryDirectory() as tmp:
        net = network(which, tmp)
    ev = net.evidence_cases(ncases, k, seed=1)
    dev = F.ExpectationMaximization(net)
    host = F.ExpectationMaximization(net, device=-1)
    assert dev.debug_posteriors(ev[:64]).tobytes() == host.debug_posteriors(ev[:64]).tobytes(), "device differs from the host twin"
    for _ in range(2):
        dev.estep_flat(ev)
    wall, kern = [], []
    for _ in range(8):
        t0 = time.perf_counter()
        counts, value = dev.estep_flat(ev)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(dev.last_kernel_ms())
    t0 = time.perf_counter()
    host.estep_flat(ev[:HOST_ROWS])
    host_ms = (time.perf_counter() - t0) * 1e3 * ncases / HOST_ROWS
    mpe = F.MostProbableExplanation(net)
    for _ in range(2):
        mpe.value_parts(ev)
    mk = []
    for _ in range(8):
        mpe.value_parts(ev)
        mk.append(mpe.last_kernel_ms())
    kms, mms = float(np.median(kern)), float(np.median(mk))
    rec = {"workload": name, "nvars": net.num_nodes, "ncases": ncases, "observed_per_case": k, **dev.info(),
           "mean_log_p": float(np.mean(np.log(value[:, 0]) + value[:, 1] * np.log(2.0))),
           "counts_total_over_rows": float(counts.sum() / ncases),
           "estep_kernel_ms_median": kms, "estep_kernel_ms_min": float(np.min(kern)),
           "estep_kernel_ms_all": [float(x) for x in kern],
           "rows_per_s_kernel": ncases / (kms * 1e-3),
           "wall_ms_per_call_median": float(np.median(wall)),
           "mpe_kernel_ms_median": mms, "mpe_kernel_ms_min": float(np.min(mk)),
           "ratio_estep_over_mpe_kernel": kms / mms,
           "host_twin_wall_ms_scaled": host_ms, "host_threads": min(16, os.cpu_count() or 1),
           "ratio_host_over_device_kernel": host_ms / kms}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "em", "em_time.json"))
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
        json.dump({"tool": "tools/em_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
