"""Timing of the sampling engine (sample.hip): forward sampling on the device beside the host
generator it matches bit for bit (fbn_synth_forward_sample, 16 threads), and likelihood weighting
beside the junction tree's kernel time on the same cases (context, not a comparison of equals: one is
approximate and runs on any DAG).

    python tools/sample_time.py [--out profiles/sample/sample_time.json] [--workloads fwd_alarm,...]

Workloads: fwd_alarm = ALARM x 100,000 samples; fwd_munin = Munin-like (1041 variables) x 125,000;
fwd_c5 = the 1,000-variable network behind bench.py's config 5 dataset x 100,000; lw_alarm_64 = ALARM,
100,000 cases x 64 samples; lw_alarm_10k = ALARM, 1,000 cases x 10,000 samples; lw_munin = Munin-like,
1,000 cases x 1,024 samples.  Evidence: the seeded generator's cases (7 observed for ALARM, 208 for
Munin-like).  Each workload runs in a child process of its own under a time limit; its exit code and
last stderr lines are recorded, and no further child is started after one that did not exit 0.

Per workload: kernel ms (fbn_sampler_last_kernel_ms, median of the timed calls after warm-up), wall
ms per synchronous call with host buffers (host clock around calls that end in a synchronise; it
includes the copy of the result to the host), the host generator's wall ms (forward sampling), and a
bytes model: the table cells a sample gathers -- the whole cdf row of every sampled variable, one
probability of every observed one (an upper bound: the scan stops at the selected value) -- plus the
stores, over kernel time.  Results are checked (device = host generator / host path) before anything
is timed."""
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
LIMITS = {"fwd_alarm": 180, "fwd_munin": 240, "fwd_c5": 300, "lw_alarm_64": 240, "lw_alarm_10k": 240, "lw_munin": 300}
FWD = {"fwd_alarm": ("alarm", 100_000), "fwd_munin": ("munin", 125_000), "fwd_c5": ("c5", 100_000)}
LW = {"lw_alarm_64": ("alarm", 100_000, 64, 7), "lw_alarm_10k": ("alarm", 1_000, 10_000, 7),
      "lw_munin": ("munin", 1_000, 1_024, 208)}


def network(name, tmp):
    import fastbn_amd as F
    from fastbn_amd import synth
    if name == "alarm":
        return F.Network(os.path.join(GOLD, "alarm", "alarm.xml"))
    xml = os.path.join(tmp, name + ".xml")
    if name == "munin":
        with gzip.open(os.path.join(GOLD, "munin_like", "munin_like.xml.gz"), "rb") as f, open(xml, "wb") as g:
            g.write(f.read())
    else:  # synth.config5_dataset's network
        synth.random_network(1000, seed=1000, window=50, parent_probs=(1, 1, 1), dom=(2, 4), path=xml, k_min=0)
    return F.Network(xml)


def median_ms(fn, warm, timed, kernel_ms):
    for _ in range(warm):
        fn()
    wall, kern = [], []
    for _ in range(timed):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(kernel_ms())
    return float(np.median(wall)), float(np.min(wall)), float(np.median(kern)), float(np.min(kern))


def child_forward(name):
    import fastbn_amd as F
    which, n = FWD[name]
    with tempfile.TemporaryDirectory() as tmp:
        net = network(which, tmp)
    smp = F.Sampler(net)
    ref = net.forward_sample(n, 1)
    assert np.array_equal(smp.forward_sample(n, 1), ref), "device forward sampling differs from the host generator"
    wall, wall_min, kern, kern_min = median_ms(lambda: smp.forward_sample(n, 1), 3, 10, smp.last_kernel_ms)
    host = []
    for _ in range(4):
        t0 = time.perf_counter()
        net.forward_sample(n, 1)
        host.append((time.perf_counter() - t0) * 1e3)
    host = host[1:]
    V = net.num_nodes
    gather = int(8 * np.sum(net.dims, dtype=np.int64) * n)
    print(json.dumps({
        "workload": name, "nvars": V, "nsamples": n, "lds_bytes_per_wave": 64 * V,
        "kernel_ms_median": kern, "kernel_ms_min": kern_min, "samples_per_s_kernel": n / (kern * 1e-3),
        "device_wall_ms_per_call_median": wall, "device_wall_ms_per_call_min": wall_min,
        "host_generator_wall_ms_median": float(np.median(host)), "host_generator_wall_ms_min": float(np.min(host)),
        "host_threads": min(16, os.cpu_count() or 1),
        "ratio_host_over_device_wall": float(np.median(host)) / wall,
        "ratio_host_over_device_kernel": float(np.median(host)) / kern,
        "model_gather_bytes": gather, "model_store_bytes": V * n,
        "model_gb_per_s_at_kernel_ms": (gather + V * n) / (kern * 1e-3) / 1e9}))


def child_lw(name):
    import fastbn_amd as F
    which, ncases, S, k = LW[name]
    with tempfile.TemporaryDirectory() as tmp:
        net = network(which, tmp)
    ev = net.evidence_cases(ncases, k, seed=1)
    lw = F.LikelihoodWeighting(net, S, seed=0)
    lab, marg = lw.infer(ev[:64])
    hlab, hmarg = F.LikelihoodWeighting(net, S, seed=0, device=-1).infer(ev[:64])
    assert np.array_equal(lab, hlab) and np.array_equal(marg, hmarg), "device differs from the host path"
    wall, wall_min, kern, kern_min = median_ms(lambda: lw.infer(ev), 2, 8, lw.last_kernel_ms)
    ess = lw.stats[1]
    jt = F.JunctionTree(net)
    jt.infer(ev)
    jt_ms = []
    for _ in range(5):
        jt.infer(ev)
        jt_ms.append(jt.last_kernel_ms())
    dims = net.dims.astype(np.int64)
    obs = ev >= 0
    per_case = (8 * dims[None, :] * ~obs).sum(1) + 8 * obs.sum(1)
    gather = int(per_case.sum()) * S
    SD = int(dims.sum())
    samples = ncases * S
    print(json.dumps({
        "workload": name, "nvars": net.num_nodes, "ncases": ncases, "samples_per_case": S, "observed_per_case": k,
        "lds_bytes_per_wave": 64 * net.num_nodes, "waves": ncases,
        "kernel_ms_median": kern, "kernel_ms_min": kern_min, "samples_per_s_kernel": samples / (kern * 1e-3),
        "sample_variables_per_s_kernel": samples * net.num_nodes / (kern * 1e-3),
        "wall_ms_per_call_median": wall, "wall_ms_per_call_min": wall_min,
        "ess_median": float(np.median(ess)), "ess_min": float(np.min(ess)),
        "jt_kernel_ms_same_cases_median": float(np.median(jt_ms)), "jt_variant": jt.refresh_info()["variant"],
        "model_gather_bytes": gather, "model_output_bytes": ncases * SD * 8 * max(1, (S + 63) // 64),
        "model_gather_gb_per_s_at_kernel_ms": gather / (kern * 1e-3) / 1e9}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sample", "sample_time.json"))
    ap.add_argument("--workloads", default=",".join(LIMITS))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        (child_forward if a.child in FWD else child_lw)(a.child)
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
        json.dump({"tool": "tools/sample_time.py", "workloads": results}, f, indent=1)
        f.write("\n")
    return 0 if all(r["exit_code"] == 0 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
