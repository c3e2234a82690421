"""Timing of loopy belief propagation (lbp.hip) beside its host twin (lbp_host.cpp, 16 threads) and,
for context, beside the junction tree's kernel time on the same cases (not a comparison of equals: LBP
is approximate on a loopy graph and runs on any DAG).

    python tools/lbp_time.py [--out profiles/lbp/lbp_time.json] [--workloads lbp_alarm_100k,...]

Workloads: lbp_alarm_100k = ALARM, 100,000 cases x 20 iterations; lbp_alarm_tol = ALARM, 1,000 cases x
up to 200 iterations with tol = 1e-9; lbp_munin = Munin-like (1041 variables), 1,000 cases x 10
iterations.  Evidence: the seeded generator's cases (7 observed for ALARM, 208 for Munin-like).  Each
workload runs in a child process of its own under a time limit; its exit code and last stderr lines
are recorded, and no further child is started after one that did not exit 0.

Per workload: kernel ms (fbn_lbp_last_kernel_ms: HIP events, median of 8 timed calls after 2 warm-up
calls), wall ms per synchronous call with host buffers (it includes the copy of the result to the
host), the host twin's wall ms on the same batch (median of 3 after one warm-up), the iterations
actually run, and a work model: per iteration every table cell is visited once per slot of its
factor and multiplied by the other slots' messages -- cells x slots x (slots - 1) fp64 multiplies
and as many LDS (or workspace) reads, plus cells x slots 8-byte table gathers -- over kernel time.
The first 64 cases are checked against the host twin bit for bit before anything is timed."""
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
# name -> (network, cases, iterations, tol, observed per case)
WORK = {"lbp_alarm_100k": ("alarm", 100_000, 20, 0.0, 7), "lbp_alarm_tol": ("alarm", 1_000, 200, 1e-9, 7),
        "lbp_munin": ("munin", 1_000, 10, 0.0, 208)}
LIMITS = {"lbp_alarm_100k": 240, "lbp_alarm_tol": 180, "lbp_munin": 300}


def network(name, tmp):
    import fastbn_amd as F
    if name == "alarm":
        return F.Network(os.path.join(GOLD, "alarm", "alarm.xml"))
    xml = os.path.join(tmp, name + ".xml")
    with gzip.open(os.path.join(GOLD, "munin_like", "munin_like.xml.gz"), "rb") as f, open(xml, "wb") as g:
        g.write(f.read())
    return F.Network(xml)


def work_model(net):
    """(multiplies, table gathers) of one iteration's factor -> variable half-step, one case, no evidence."""
    mults = gathers = 0
    for v in range(net.num_nodes):
        par, cnt = net.node_counts(v)
        cells, slots = cnt.size, len(par) + 1
        mults += cells * slots * (slots - 1)
        gathers += cells * slots
    return int(mults), int(gathers)


def child(name):
    import fastbn_amd as F
    which, ncases, iters, tol, k = WORK[name]
    with tempfile.TemporaryDirectory() as tmp:
        net = network(which, tmp)
    ev = net.evidence_cases(ncases, k, seed=1)
    dev = F.LoopyBeliefPropagation(net, iterations=iters, tol=tol)
    host = F.LoopyBeliefPropagation(net, iterations=iters, tol=tol, device=-1)
    lab, marg = dev.infer(ev[:64])
    hlab, hmarg = host.infer(ev[:64])
    assert np.array_equal(lab, hlab) and np.array_equal(marg.view(np.uint64), hmarg.view(np.uint64)), \
        "device differs from the host twin"
    assert np.array_equal(dev.stats[0], host.stats[0])
    for _ in range(2):
        dev.infer(ev)
    wall, kern = [], []
    for _ in range(8):
        t0 = time.perf_counter()
        dev.infer(ev)
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(dev.last_kernel_ms())
    used, res = dev.stats
    host.infer(ev)
    hw = []
    for _ in range(3):
        t0 = time.perf_counter()
        host.infer(ev)
        hw.append((time.perf_counter() - t0) * 1e3)
    rec = {"workload": name, "nvars": net.num_nodes, "ncases": ncases, "iterations": iters, "tol": tol,
           "observed_per_case": k, **dev.info(),
           "kernel_ms_median": float(np.median(kern)), "kernel_ms_min": float(np.min(kern)),
           "wall_ms_per_call_median": float(np.median(wall)), "wall_ms_per_call_min": float(np.min(wall)),
           "iterations_used_median": float(np.median(used)), "iterations_used_max": int(used.max()),
           "iterations_used_total": int(used.sum()), "converged_cases": int((res <= tol).sum()) if tol > 0 else None,
           "case_iterations_per_s_kernel": float(used.sum()) / (np.median(kern) * 1e-3),
           "host_twin_wall_ms_median": float(np.median(hw)), "host_twin_wall_ms_min": float(np.min(hw)),
           "host_threads": min(16, os.cpu_count() or 1),
           "ratio_host_over_device_wall": float(np.median(hw)) / float(np.median(wall)),
           "ratio_host_over_device_kernel": float(np.median(hw)) / float(np.median(kern))}
    mults, gathers = work_model(net)
    rec["model_multiplies_per_case_iteration"] = mults
    rec["model_table_gathers_per_case_iteration"] = gathers
    rec["model_gmults_per_s_at_kernel_ms"] = mults * float(used.sum()) / (np.median(kern) * 1e-3) / 1e9
    try:  # context: the junction tree's kernel on the same cases, where one exists
        jt = F.JunctionTree(net)
        jt.infer(ev)
        jt_ms = []
        for _ in range(5):
            jt.infer(ev)
            jt_ms.append(jt.last_kernel_ms())
        rec["jt_kernel_ms_same_cases_median"] = float(np.median(jt_ms))
    except F.FastBNError as e:
        rec["jt_kernel_ms_same_cases_median"] = None
        rec["jt_error"] = str(e)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lbp", "lbp_time.json"))
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
        json.dump({"tool": "tools/lbp_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
