"""Timing of the most probable explanation (jt_mpe.hip) beside the junction tree's interpreter kernel
(jt_interp_kernel, JunctionTree.set_variant(1)) on the same cases and beside its own host twin
(jt_mpe_host.cpp, 16 threads).

    python tools/mpe_time.py [--out profiles/mpe/mpe_time.json] [--workloads mpe_alarm_100k,mpe_munin_125k]

Workloads: mpe_alarm_100k = ALARM, 100,000 cases with 7 observed variables; mpe_munin_125k = Munin-like
(1041 variables), 125,000 cases with 208 observed.  Evidence: the seeded generator's cases.  Each workload
runs in a child process of its own under a time limit; its exit code and last stderr lines are recorded,
and no further child is started after one that did not exit 0.

Per workload: MPE kernel ms (fbn_mpe_last_kernel_ms: HIP events, median of 8 timed calls after 2 warm-up
calls) and cases/s, wall ms per synchronous call with host buffers, the interpreter's kernel ms on the
same cases (median of 5 after one warm-up; it computes something else -- all posterior marginals, Collect
and Distribute -- so the ratio says what a max-product pass costs next to a sum-product one, nothing more),
the host twin's wall ms (median of 3 after one warm-up), and the three ratios.  The first 64 cases are
checked against the host twin byte for byte before anything is timed.  The interpreter is skipped (with
its error recorded) where its workspace does not fit."""
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
# name -> (network, cases, observed per case)
WORK = {"mpe_alarm_100k": ("alarm", 100_000, 7), "mpe_munin_125k": ("munin", 125_000, 208)}
LIMITS = {"mpe_alarm_100k": 240, "mpe_munin_125k": 600}


def network(name, tmp):
    import fastbn_amd as F
    if name == "alarm":
        return F.Network(os.path.join(GOLD, "alarm", "alarm.xml"))
    xml = os.path.join(tmp, name + ".xml")
    with gzip.open(os.path.join(GOLD, "munin_like", "munin_like.xml.gz"), "rb") as f, open(xml, "wb") as g:
        g.write(f.read())
    return F.Network(xml)


def child(name, skip_jt):
    import fastbn_amd as F
    which, ncases, k = WORK[name]
    with tempfile.TemporaryDirectory() as tmp:
        net = network(which, tmp)
    ev = net.evidence_cases(ncases, k, seed=1)
    dev = F.MostProbableExplanation(net)
    host = F.MostProbableExplanation(net, device=-1)
    a, v = dev.value_parts(ev[:64])
    ha, hv = host.value_parts(ev[:64])
    assert a.tobytes() == ha.tobytes() and v.tobytes() == hv.tobytes(), "device differs from the host twin"
    for _ in range(2):
        dev.value_parts(ev)
    wall, kern = [], []
    for _ in range(8):
        t0 = time.perf_counter()
        _, value = dev.value_parts(ev)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(dev.last_kernel_ms())
    host.value_parts(ev)
    hw = []
    for _ in range(3):
        t0 = time.perf_counter()
        host.value_parts(ev)
        hw.append((time.perf_counter() - t0) * 1e3)
    kms = float(np.median(kern))
    rec = {"workload": name, "nvars": net.num_nodes, "ncases": ncases, "observed_per_case": k, **dev.info(),
           "mean_log_p": float(np.mean(np.log(value[:, 0]) + value[:, 1] * np.log(2.0))),
           "kernel_ms_median": kms, "kernel_ms_min": float(np.min(kern)),
           "cases_per_s_kernel": ncases / (kms * 1e-3),
           "wall_ms_per_call_median": float(np.median(wall)), "wall_ms_per_call_min": float(np.min(wall)),
           "host_twin_wall_ms_median": float(np.median(hw)), "host_twin_wall_ms_min": float(np.min(hw)),
           "host_threads": min(16, os.cpu_count() or 1),
           "ratio_host_over_device_kernel": float(np.median(hw)) / kms}
    rec["jt_interp_kernel_ms_median"] = None
    if not skip_jt:
        try:  # the sum-product interpreter on the same cases (labels only: no marginal copy to time)
            jt = F.JunctionTree(net)
            jt.set_variant(1)
            if which == "munin":
                # its workspace is 151 MB per wave (every clique table of 64 cases): 2 waves per CU, ~77 GB,
                # instead of the default that fills 80 % of the free memory
                jt.set_waves_per_cu(2)
                rec["jt_interp_waves_per_cu"] = 2
            jt.infer(ev, marginals=False)
            jt_ms = []
            for _ in range(5):
                jt.infer(ev, marginals=False)
                jt_ms.append(jt.last_kernel_ms())
            rec["jt_interp_kernel_ms_median"] = float(np.median(jt_ms))
            rec["ratio_jt_interp_over_mpe_kernel"] = float(np.median(jt_ms)) / kms
        except F.FastBNError as e:
            rec["jt_error"] = str(e)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mpe", "mpe_time.json"))
    ap.add_argument("--workloads", default=",".join(LIMITS))
    ap.add_argument("--skip-jt", action="store_true", help="MPE and its host twin only")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.skip_jt)
        return 0
    results = []
    for name in a.workloads.split(","):
        rec = {"workload": name, "time_limit_s": LIMITS[name]}
        try:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name] + (["--skip-jt"] if a.skip_jt else [])
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
        json.dump({"tool": "tools/mpe_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
