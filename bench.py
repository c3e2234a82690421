#!/usr/bin/env python3
"""Benchmark of the two FastBN hot paths on MI355X (BASELINE.json metric).

Headline `value` = junction-tree test cases / s on ALARM (BASELINE config 2: 100k synthetic cases
per GPU per step, 7 evidence variables per case, inputs resident in HBM, labels + all marginals
written back to HBM).  A "step" is one pass of the batched JT kernel over the 100k cases.  With
--gpus N (torchrun, one process per GPU) every rank processes its own 100k-case shard (seed +
rank, no data-path collective) -> weak scaling; `value` = all cases / max-over-ranks time.

A plain run sets up, warms up, times the --steps steps and prints the line (`ms_per_step` = wall
time of the timed region / steps; the headline kernel's roofline from the committed counter
summaries under profiles/).  --dump-outputs DIR writes the last timed step's labels and marginals
as DIR/*.npy (`dump_outputs`); the inputs are seeded, so two builds can be compared output for output.

With --full, also (rank 0, N = 1): the oracle and full-batch checks of the last step's outputs,
PC-stable CI-tests / s on alarm_s5000.txt (BASELINE config 3,
reference-equivalent test count), the dominant kernel's HBM roofline (algorithmic bytes per case =
16*(sum clique + separator entries) + 8*sum dom + V = 22,877 B) and the CPU baseline
(the unmodified reference's per-case loop, oracle/_ref, timed on this host on a bounded sample);
at N > 1 the Munin-like and PC-stable legs over the ranks.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
from fastbn_amd import shard  # noqa: E402
ALARM = os.path.join(REPO, "tests", "golden", "alarm")
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md)
CASES_PER_GPU = 100_000
EVIDENCE_PER_CASE = 7
MAX_LABEL_SLICES = 4096  # per-step label buffers of a one-GPU run (1.6 GB at 100k cases)
DUMP_BUDGET_BYTES = 48 << 20  # --dump-outputs: marginal rows written (float64), labels beside them
DUMP_SEED = 20250131


def log(*a):
    print(*a, file=sys.stderr, flush=True)


REF_DUMP = os.path.join(REPO, "oracle", "_ref", "ref_dump")


def host_info():
    """CPU model, visible CPUs, the CPUs this process may run on and the thread sweep used for
    every cpu_baseline (t in {1, cores/2, cores})."""
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    cpus = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))
    affinity = len(cpus)
    # physical cores among the CPUs this process may use: distinct (package, core) pairs (SMT
    # siblings counted once); the driver's OMP_NUM_THREADS (the box's CPU share) does not cap it
    phys = set()
    for c in cpus:
        try:
            base = f"/sys/devices/system/cpu/cpu{c}/topology/"
            phys.add((open(base + "physical_package_id").read().strip(), open(base + "core_id").read().strip()))
        except OSError:
            phys.add(("?", str(c)))
    cores = max(1, len(phys))
    omp = os.environ.get("OMP_NUM_THREADS")
    share = int(omp) if omp and omp.isdigit() and 0 < int(omp) < cores else None
    sweep = {1, max(1, cores // 2), cores} | ({share} if share else set())
    return {"cpu_model": model, "nproc": os.cpu_count(), "affinity_cpus": affinity, "physical_cores": cores,
            "omp_num_threads_env": omp, "cores": cores, "sweep": sorted(sweep),
            "note": "sweep = {1, cores/2, cores} over the physical cores of the CPUs usable here, plus the "
                    "driver's OMP_NUM_THREADS share; each reference run gets OMP_NUM_THREADS = t"}


def _ref_env(threads):
    env = dict(os.environ)
    env["OMP_NUM_THREADS"] = str(threads)
    return env


def _libsvm(path, ev):
    with open(path, "w") as f:
        for r in ev:
            f.write("0 " + " ".join(f"{v}:{r[v]}" for v in range(r.size) if r[v] >= 0) + " \n")


def _jt_sweep(xml, tree_set, ev_path, cases_at, hi):
    """ref_dump jtbench at every thread count of the sweep -> (best, per-thread list)."""
    sweep = []
    for t in hi["sweep"]:
        log(f"bench: reference JT baseline, {t} threads")
        n = cases_at(t)
        out = subprocess.run([REF_DUMP, "jtbench", xml, tree_set, ev_path, str(n), str(t)], check=True,
                             capture_output=True, text=True, env=_ref_env(t)).stdout.split()
        secs = float(out[3])
        sweep.append({"threads": t, "cases": n, "seconds": round(secs, 3), "value": n / secs})
    best = max(sweep, key=lambda r: r["value"])
    return best, sweep


def cpu_baseline_jt(budget_cases=40_000):
    """The unmodified reference's per-case loop (oracle/_ref/ref_dump jtbench: JunctionTree::
    PredictUseJTInfer with num_threads = t) on a bounded sample of the ALARM workload, t swept."""
    from fastbn_amd import synth
    hi = host_info()
    net = synth.read_xmlbif(os.path.join(ALARM, "alarm.xml"))
    ev = synth.evidence_cases(net, budget_cases, EVIDENCE_PER_CASE, seed=20250131)
    if os.path.exists(REF_DUMP):
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "ev.libsvm")
            _libsvm(path, ev)
            # the reference slows down with threads on ALARM (fork/join per tree level): fewer cases
            best, sweep = _jt_sweep(os.path.join(ALARM, "alarm.xml"), os.path.join(ALARM, "testing_alarm_1k_p20"),
                                    path, lambda t: budget_cases if t == 1 else budget_cases // (4 if t <= 16 else 16),
                                    hi)
        return {"value": best["value"], "unit": "cases/s", "cores": best["threads"], "kind": "reference",
                "cpu": hi, "sweep": sweep,
                "sample": f"{best['cases']} ALARM cases (7 evidence vars, seed 20250131) through the reference's "
                          f"per-case loop, best of threads {hi['sweep']}: {best['seconds']} s at t={best['threads']}"}
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import oracle as O
    o = O.OracleJT(os.path.join(ALARM, "alarm.xml"))
    t0 = time.perf_counter()
    o.infer(ev)
    secs = time.perf_counter() - t0
    return {"value": budget_cases / secs, "unit": "cases/s", "cores": 1, "kind": "port", "cpu": hi,
            "sample": f"{budget_cases} ALARM cases, restatement at t=1 (oracle/_ref absent), {secs:.2f} s"}


def cpu_baseline_munin(xml, ev, cases=1000, other=128):
    """The reference's per-case loop on the Munin-like network (ref_dump jtbench), t swept, on the
    first `cases` cases of the GPU workload at t = 1 (its best: the reference slows down with
    threads on this tree) and the first `other` at the other thread counts (~20 s per 1,000 cases)."""
    hi = host_info()
    if not os.path.exists(REF_DUMP):
        return None
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "ev.libsvm")
        _libsvm(path, ev[:cases])
        best, sweep = _jt_sweep(xml, path, path, lambda t: cases if t == 1 else other, hi)
    return {"value": best["value"], "unit": "cases/s", "cores": best["threads"], "kind": "reference", "cpu": hi,
            "sweep": sweep,
            "sample": f"first {best['cases']} Munin-like cases of the GPU shard (208 evidence vars) through the "
                      f"reference's per-case loop, best of threads {hi['sweep']} ({cases} cases at t=1, {other} "
                      f"at the others): {best['seconds']} s at t={best['threads']}"}


def _pc_sweep(src, depth, reps, hi):
    """ref_dump pcbench (the reference's PC-stable skeleton: its Counts*/Edge/ChoiceGenerator/
    Network code and OpenMP structure, driver + G^2 restated) at every thread count -> per-thread
    medians of the end-to-end step-1 time and of the time inside the CI rounds."""
    sweep = []
    for t in hi["sweep"]:
        log(f"bench: reference PC baseline ({os.path.basename(src)}), {t} threads")
        runs = []
        for _ in range(reps):
            out = subprocess.run([REF_DUMP, "pcbench", src, "0.05", str(depth), "1", str(t)], check=True,
                                 capture_output=True, text=True, env=_ref_env(t)).stdout
            tests = [int(v) for v in out.split("|")[0].split()[1:]]
            kv = out.split("|")[2].split()
            runs.append((float(kv[1]), float(kv[3]), float(kv[5])))
        tot, ci, er = (float(np.median([r[i] for r in runs])) for i in range(3))
        n = sum(tests)
        sweep.append({"threads": t, "tests": n, "total_s": round(tot, 4), "ci_s": round(ci, 4),
                      "erase_s": round(er, 4), "value": n / tot, "ci_only_value": n / ci})
    return sweep


def cpu_baseline_pc_alarm(reps=5):
    hi = host_info()
    if not os.path.exists(REF_DUMP):
        sys.path.insert(0, os.path.join(REPO, "oracle"))
        import oracle as O
        ds = O.OracleDataset(csv=os.path.join(ALARM, "alarm_s5000.txt"))
        t0 = time.perf_counter()
        for _ in range(reps):
            r = ds.pc_stable(0.05, 1000, 1)
        secs = (time.perf_counter() - t0) / reps
        return {"value": r["num_ci_test"] / secs, "unit": "CI-tests/s", "cores": 1, "kind": "port", "cpu": hi,
                "sample": f"{reps} restatement runs on alarm_s5000 (oracle/_ref absent), {secs * 1e3:.1f} ms/run"}
    sweep = _pc_sweep(os.path.join(ALARM, "alarm_s5000.txt"), 1000, reps, hi)
    best = max(sweep, key=lambda r: r["value"])
    return {"value": best["value"], "unit": "CI-tests/s", "cores": best["threads"], "kind": "reference",
            "ci_only_value": max(r["ci_only_value"] for r in sweep), "cpu": hi, "sweep": sweep,
            "sample": f"PC-stable skeleton (levels 0-4, {best['tests']} tests) on alarm_s5000, the reference's "
                      f"counting / edge / OpenMP code (ref_dump pcbench; PCStable/IndependenceTest restated: "
                      f"stats/gcem absent), median of {reps} runs per t, best of threads {hi['sweep']}: "
                      f"{best['total_s'] * 1e3:.1f} ms end-to-end at t={best['threads']}"}


def cpu_baseline_pc_c5(cols, dims, depth, nvars=160, reps=1):
    """Config 5 on the first `nvars` variables (all 100k samples): end-to-end step-1 (with the
    reference's O(E^2) vec_edges.erase loops) and CI-only rates, t swept."""
    import struct
    hi = host_info()
    if not os.path.exists(REF_DUMP):
        return None
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "c5.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<iq", nvars, cols.shape[1]))
            f.write(np.asarray(dims[:nvars], np.int32).tobytes())
            f.write(np.ascontiguousarray(cols[:nvars]).tobytes())
        sweep = _pc_sweep("cols:" + path, depth, reps, hi)
    best = max(sweep, key=lambda r: r["value"])
    return {"value": best["value"], "unit": "CI-tests/s", "cores": best["threads"], "kind": "reference",
            "ci_only_value": max(r["ci_only_value"] for r in sweep), "cpu": hi, "sweep": sweep,
            "sample": f"PC-stable levels 0-{depth - 1} on the first {nvars} variables of the config-5 dataset "
                      f"(100k samples, {best['tests']} tests) with the reference's counting / edge / OpenMP code "
                      f"(ref_dump pcbench), best of threads {hi['sweep']}: {best['total_s']:.2f} s end-to-end at "
                      f"t={best['threads']}; the O(E^2) erase loop grows quadratically with the edge count, so "
                      f"the full 1000-variable end-to-end rate is far lower (SURVEY: 826 s for level 0 at 10k "
                      f"samples)"}


def cpu_baseline_pc_c5_full(cols, dims, depth):
    """Config 5 at full size (all 1000 variables, 100k samples, levels 0-5: the 801,354 tests the GPU
    runs) through the reference's counting / edge / OpenMP code (ref_dump pcbench), with its O(E^2)
    vec_edges.erase loops replaced by one stable compaction per level ("noerase": the same edges in
    the same order, so the same tests) -- the reference's CI work on the measured workload.  ~20-40 s
    per thread count on a 16-CPU share, so only the upper half of the sweep runs."""
    import struct
    hi = host_info()
    if not os.path.exists(REF_DUMP):
        return None
    threads = sorted({t for t in hi["sweep"] if t >= max(hi["sweep"]) // 2})
    sweep = []
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "c5.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<iq", cols.shape[0], cols.shape[1]))
            f.write(np.asarray(dims, np.int32).tobytes())
            f.write(np.ascontiguousarray(cols).tobytes())
        for t in threads:
            log(f"bench: reference PC baseline (config 5, all {cols.shape[0]} variables, noerase), {t} threads")
            out = subprocess.run([REF_DUMP, "pcbench", "cols:" + path, "0.05", str(depth), "1", str(t), "noerase"],
                                 check=True, capture_output=True, text=True, env=_ref_env(t)).stdout
            tests = [int(v) for v in out.split("|")[0].split()[1:]]
            kv = out.split("|")[2].split()
            tot, ci = float(kv[1]), float(kv[3])
            sweep.append({"threads": t, "tests": sum(tests), "tests_per_level": tests, "total_s": round(tot, 3),
                          "ci_s": round(ci, 3), "value": sum(tests) / tot, "ci_only_value": sum(tests) / ci})
    best = max(sweep, key=lambda r: r["value"])
    return {"value": best["value"], "unit": "CI-tests/s", "cores": best["threads"], "kind": "reference",
            "ci_only_value": best["ci_only_value"], "tests_per_level": best["tests_per_level"], "cpu": hi,
            "sweep": sweep,
            "sample": f"the whole config-5 workload (1000 variables x 100k samples, levels 0-{depth - 1}, "
                      f"{best['tests']} tests = the GPU's) through the reference's Counts2D / Counts3D / Edge / "
                      f"ChoiceGenerator / OpenMP code (ref_dump pcbench noerase: the O(E^2) erase loop replaced by "
                      f"one stable compaction), best of threads {threads}: {best['total_s']} s at t={best['threads']}"}


def bench_pc(steps, warmup):
    import fastbn_amd as F
    ds = F.Dataset(os.path.join(ALARM, "alarm_s5000.txt"))
    ci = F.IndependenceTest(ds)  # column store resident in HBM (uploaded once, outside the timing)
    pc = F.PCStable(0.05, 1000)
    for _ in range(max(1, warmup)):
        pc.StructLearnCompData(ci)
    t = []
    import ctypes
    h = ctypes.c_void_p()
    ci.set_kernel_timing(False)  # kernel time comes from the warm-up run above; no events when timed
    for _ in range(steps):  # the C-ABI call: skeleton (device CI sweep) + orientation, as the reference's
        t0 = time.perf_counter()  # "pc-stable" timer; the Python result conversion is not timed
        F.lib.fbn_pc_stable(ci._h, 0.05, 1000, 1, ctypes.byref(h))
        t.append(time.perf_counter() - t0)
        F.lib.fbn_pc_result_destroy(h)
    ci.set_kernel_timing(True)
    ms = 1e3 * float(np.median(t))
    # SURVEY §8(d) byte model: every reference-equivalent test streams its x, y, z_1..z_d uint8
    # columns once, B_test(d) = N (d + 2) -> 80.3 MB per ALARM-5000 run
    n_samples = int(ds.num_instance)
    model_bytes = n_samples * sum(int(c) * (d + 2) for d, c in enumerate(pc.tests_per_level.tolist()))
    achieved = model_bytes / (ms * 1e-3) / 1e9
    kernel_ms = 1e3 * pc.kernel_s
    return {"metric": "PC-stable CI-tests/sec (alarm_s5000, levels 0-4)", "value": pc.num_ci_test / (ms * 1e-3),
            "unit": "CI-tests/s", "tests": pc.num_ci_test, "tests_per_level": pc.tests_per_level.tolist(),
            "launched_per_level": pc.launched_per_level.tolist(), "ms_per_run": ms,
            "kernel_ms_per_run": kernel_ms, "edges": len(pc.edges),
            "device_resident": os.environ.get("FBN_PC_NO_SMALL") is None,
            "roofline": {"bound": "latency", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "model_bytes_per_run": model_bytes,
                         "achieved_kernel_only": model_bytes / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else None,
                         "kernel_ms_per_run": kernel_ms, "wall_ms_per_run": ms,
                         "column_bytes_read_per_run": pc.device_bytes, **pc_small_traffic(),
                         "note": "achieved = SURVEY 8(d) byte model (N (d + 2) bytes per reference-equivalent test, "
                                 "80.3 MB per run) / C-ABI wall time.  The whole skeleton search is ONE device launch "
                                 "(pc_small.hip: five levels, one grid barrier each) over a column store that stays "
                                 "in cache (185 KB): a latency chain of five dependent levels, not bound by HBM or "
                                 "VALU, so frac is small by construction (DESIGN.md 5.4)"}}


def pc_small_traffic():
    """Measured L2<->fabric bytes of one device-resident search launch (rocprofv3 FETCH_SIZE +
    WRITE_SIZE, calibrated; committed summary profiles/r05/pmc_pc_small_traffic.json from
    tools/profile_r05_final.sh)."""
    path = _first_profile("r06/pmc_pc_small_traffic.json", "r05/pmc_pc_small_traffic.json", "r04/pmc_pc_small_traffic.json")
    if path is None:
        return {"traffic": None}
    with open(path) as f:
        t = json.load(f)
    return {"traffic": t["hbm_bytes_per_launch"], "traffic_source": os.path.relpath(path, REPO)}


def _first_profile(*names):
    """The first existing committed profile summary under profiles/ (this round's before older ones)."""
    for n in names:
        p = os.path.join(REPO, "profiles", n)
        if os.path.exists(p):
            return p
    return None


N_VARS_C5 = 1000


INT_VALU_PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9  # MI355X: a wave64 32-bit VALU instruction issues in 2 cycles


def pc_roofline(kernel_s, device_bytes, byte_column_bytes, world=1):
    """Config 5's CI kernels against the bounds they can hit: 32-bit VALU issue (popcount / AND
    for the bit-sliced kernels, the binning for the histogram kernel) and L2<->fabric traffic, per
    PC run; VALU instructions and fabric bytes per run from the committed PMC profile
    (profiles/r05/pc5_kernels.json: rocprofv3 --pmc SQ_INSTS_VALU / FETCH_SIZE / WRITE_SIZE, calibrated),
    the kernel time measured live (HIP events around every CI batch of a run).  world > 1: the run's
    work is split over the ranks, so the whole run's instructions / bytes are taken over the slowest
    rank's kernel time against `world` GPUs' peak."""
    path = _first_profile("r06/pc5_kernels.json", "r05/pc5_kernels.json", "pc5_kernels.json")
    out = {"kernel_ms_per_run": 1e3 * kernel_s, "column_bytes_read_per_run": device_bytes,
           "model": {"bytes_per_run": byte_column_bytes,
                     "model_frac": byte_column_bytes / kernel_s / (HBM_PEAK_GBS * 1e9),
                     "note": "informational: SURVEY 8(d)'s byte-column model (every test streams N (d + 2) "
                             "uint8 bytes); the bit-sliced / FP4 kernels read packed masks from L2 instead, so "
                             "this ratio is not a bound (it exceeds 1)"}}
    if path is None:
        return {"bound": None, **out}
    with open(path) as f:
        prof = json.load(f)
    ks = {k: v for k, v in prof["kernels"].items()
          if k not in ("ci_cols_check", "ci_bits_build", "ci_bits_rowcount")}  # once per dataset
    ops = sum(v["valu_lane_ops_per_run"] for v in ks.values())
    fab = sum(v["fabric_bytes_per_run"] for v in ks.values())
    valu = ops / kernel_s / (world * INT_VALU_PEAK_LANE_OPS)
    fabric = fab / kernel_s / (world * HBM_PEAK_GBS * 1e9)
    top = max(ks, key=lambda k: ks[k]["time_ms_per_run"])
    if valu >= fabric:
        r = {"bound": "valu", "achieved": ops / kernel_s / 1e12, "peak": world * INT_VALU_PEAK_LANE_OPS / 1e12,
             "unit": "Tlane-op/s", "frac": valu}
    else:
        r = {"bound": "hbm", "achieved": fab / kernel_s / 1e9, "peak": world * HBM_PEAK_GBS, "unit": "GB/s",
             "frac": fabric}
    if world > 1:
        r["per_gpu_peak_x"] = world
    return {**r, "traffic": fab, "valu_frac": valu, "fabric_frac": fabric, **out,
            "dominant_kernel": {top: ks[top]}, "source": os.path.relpath(path, REPO),
            "note": "all CI kernels of one run: PMC VALU lane-ops and calibrated L2<->fabric bytes per run over the "
                    "live kernel time; neither bound is reached: the popcount kernels are bound by v_bcnt issue "
                    "(half rate on gfx950, tools/micro/valu_rate.hip) and latency, the level-0 Gram is a hand-written "
                    "FP4 MFMA kernel on the matrix cores (ci_gram_mfma.hip, DESIGN.md 5.3)"}


def synth_c5(nvars=N_VARS_C5, nsamples=100_000):
    """SURVEY §8(d) config 5 dataset (fastbn_amd.synth.config5_dataset)."""
    from fastbn_amd import synth
    return synth.config5_dataset(nvars, nsamples)


def bench_pc_synth(steps, depth=6, cpu_vars=160, with_baseline=True):
    """SURVEY §8(d) config 5 on one GPU: PC-stable (levels 0..5) on the synthetic 1000-variable x
    100k-sample dataset; CI-tests/s over the C-ABI call (skeleton + orientation), column store
    resident.  CPU baseline: the reference's PC-stable (ref_dump pcbench) on the first `cpu_vars`
    variables of the same data, thread sweep."""
    import ctypes
    import fastbn_amd as F
    cols, dims = synth_c5()
    N = cols.shape[1]
    ci = F.IndependenceTest(F.Dataset(columns=cols, dims=dims))
    pc = F.PCStable(0.05, depth)
    pc.StructLearnCompData(ci)  # warm-up: per-dataset stores (bit-sliced / one-hot) and library init
    pc.StructLearnCompData(ci)  # the kernel time / bytes of a steady-state run
    t, ks = [], []
    h = ctypes.c_void_p()
    ci.set_kernel_timing(False)  # kernel time / bytes come from the second warm-up run above
    for _ in range(steps):
        t0 = time.perf_counter()
        F.lib.fbn_pc_stable(ci._h, 0.05, depth, 1, ctypes.byref(h))
        t.append(time.perf_counter() - t0)
        F.lib.fbn_pc_result_destroy(h)
    ci.set_kernel_timing(True)
    ms = 1e3 * float(np.median(t))
    tests = pc.num_ci_test
    launched = pc.launched_per_level.tolist()
    kern_s = pc.kernel_s
    alg = pc.device_bytes  # column bytes the kernels must read per launched test, in their format
    out = {"metric": "PC-stable CI-tests/sec (synthetic 1000 vars x 100k samples, levels 0-5, BASELINE config 5)",
           "value": tests / (ms * 1e-3), "unit": "CI-tests/s", "tests": tests,
           "tests_per_level": pc.tests_per_level.tolist(), "launched_per_level": launched, "ms_per_run": ms,
           "kernel_ms_per_run": 1e3 * kern_s, "edges": len(pc.edges),
           "roofline": pc_roofline(kern_s, alg, sum(n_d * N * (d + 2) for d, n_d in enumerate(launched)))}
    # the same workload through the native multi-GPU session at world size 1 (bench.py --gpus N
    # runs it on N ranks): the per-level partition / record / apply overhead of the N > 1 path
    from fastbn_amd import pc_dist
    ci.set_kernel_timing(False)
    td = []
    for _ in range(steps):
        t0 = time.perf_counter()
        res, dtests, _ = pc_dist.pc_stable_distributed(ci, N_VARS_C5, 0.05, depth)
        td.append(time.perf_counter() - t0)
    ci.set_kernel_timing(True)
    out["session_world1"] = {"ms_per_run": 1e3 * float(np.median(td)), "tests": int(sum(dtests)),
                             "same_skeleton": res.edges == pc.edges and res.sepset == pc.sepset,
                             "note": "fbn_pc_dist_* session (the N > 1 path) at world size 1, Python level "
                                     "loop + records included"}
    if with_baseline:
        full = cpu_baseline_pc_c5_full(cols, dims, depth)
        if full is not None:  # the measured workload itself: the line's cpu_baseline
            out["cpu_baseline"] = full
            out["cpu_baseline_ratio"] = out["value"] / full["value"]
        part = cpu_baseline_pc_c5(cols, dims, depth, nvars=cpu_vars)
        if part is not None:  # end-to-end with the reference's erase loops, on the first cpu_vars variables
            out["cpu_baseline_end_to_end_subset" if full is not None else "cpu_baseline"] = part
    return out


def _pc_broadcast_ctx(load, rank, device):
    """Rank 0 loads the column store (`load()` -> (cols, dims)) and one RCCL broadcast puts it in
    every rank's HBM -> (IndependenceTest, collective device or None for gloo, nvars)."""
    import torch
    import torch.distributed as dist
    from fastbn_amd import pc_dist
    dev = torch.device("cuda", device)
    cols, dims = load() if rank == 0 else (None, None)
    meta = [list(cols.shape) if rank == 0 else None, dims.tolist() if rank == 0 else None]
    dist.broadcast_object_list(meta, 0)
    dims = np.array(meta[1], np.int32)
    if dist.get_backend() == "nccl":  # RCCL: broadcast straight into device memory, records on the GPU
        ci = pc_dist.independence_test_broadcast(cols, dims, meta[0], 0.05, device)
        coll = dev
    else:  # gloo rehearsal (ranks sharing a GPU): collectives on the CPU
        import fastbn_amd as F
        t = pc_dist.broadcast_columns(cols, meta[0]).to(dev)
        torch.cuda.synchronize(dev)
        ci = F.IndependenceTest.from_device(t.data_ptr(), meta[0][0], meta[0][1], dims, 0.05, device)
        ci._cols_keepalive = t
        coll = None
    ci.num_samples = int(meta[0][1])
    return ci, coll, meta[0][0]


def _pc_dist_timed(load, steps, rank, world, device, depth):
    """PC-stable through the distributed session on N ranks: the column store broadcast once
    (`_pc_broadcast_ctx`); each level's edges are partitioned over the ranks (fbn_pc_dist_*), one
    all-gather of the records per level (+ the level-0 pair tables).  Timed on the wall clock
    between barriers, max over ranks, median of `steps` runs -> (PCResult, tests, launched, ms)."""
    import torch
    import torch.distributed as dist
    from fastbn_amd import pc_dist
    dev = torch.device("cuda", device)
    ci, coll, nvars = _pc_broadcast_ctx(load, rank, device)
    # warm-up, with this rank's kernel time recorded (HIP events around every CI batch of its ranges)
    res, tests, launched = pc_dist.pc_stable_distributed(ci, nvars, 0.05, depth, device=coll)
    kernel_s = shard.max_over_ranks(res.kernel_s, dev)
    ci.set_kernel_timing(False)
    t = []
    for _ in range(steps):
        dist.barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res, tests, launched = pc_dist.pc_stable_distributed(ci, nvars, 0.05, depth, device=coll)
        torch.cuda.synchronize(dev)
        dist.barrier()
        t.append(shard.max_over_ranks(time.perf_counter() - t0, dev))
    return res, tests, launched, 1e3 * float(np.median(t)), kernel_s


def bench_pc_alarm_dist(steps, rank, world, device):
    """BASELINE config 3 (alarm_s5000, PC-stable levels 0-4) on N GPUs.  The graph is small enough
    for the one-launch device-resident search, so the ranks run REPLICAS: every rank
    runs the whole search on its own broadcast copy of the column store and one broadcast of rank
    0's result record reaches every rank (each checks it against its own).  Cutting five dependent
    levels over N GPUs would add an all-gather per level to a 0.14 ms chain; replicas keep the
    single-GPU time plus one broadcast.  Timed: the search + record + broadcast, wall clock between
    barriers, max over ranks, median of runs."""
    import torch
    import torch.distributed as dist
    from fastbn_amd import pc_dist

    def load():
        import fastbn_amd as F
        ds = F.Dataset(os.path.join(ALARM, "alarm_s5000.txt"))
        return ds.columns, ds.dims
    dev = torch.device("cuda", device)
    ci, coll, nvars = _pc_broadcast_ctx(load, rank, device)
    ci.set_kernel_timing(False)
    if not pc_dist.small_eligible(ci):  # (not ALARM: a larger graph takes the partitioned session)
        del ci
        res, tests, launched, ms, kern_s = _pc_dist_timed(load, steps, rank, world, device, 1000)
        return {"metric": "PC-stable CI-tests/sec (alarm_s5000, levels 0-4)", "value": sum(tests) / (ms * 1e-3),
                "unit": "CI-tests/s", "n_gpus": world, "tests": int(sum(tests)), "tests_per_level": tests,
                "launched_per_level": launched, "ms_per_run": ms, "edges": len(res.edges),
                "parallelism": f"edge ranges per level x{world}, one all-gather per level",
                "roofline": pc_roofline(kern_s, res.device_bytes, 0, world)}
    mode = f"replicas x{world} (one-launch device-resident search per rank) + one broadcast of rank 0's record"
    for _ in range(3):  # warm-up
        res, rec0 = pc_dist.pc_stable_replicas(ci, 0.05, 1000, device=coll)
    t = []
    for _ in range(steps):
        dist.barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res, rec0 = pc_dist.pc_stable_replicas(ci, 0.05, 1000, device=coll, check=False)
        torch.cuda.synchronize(dev)
        dist.barrier()
        t.append(shard.max_over_ranks(time.perf_counter() - t0, dev))
    res, rec0 = pc_dist.pc_stable_replicas(ci, 0.05, 1000, device=coll, check=True)  # every rank == rank 0
    ms = 1e3 * float(np.median(t))
    tests = rec0["tests_per_level"]
    # each replica runs the whole search: the single-GPU roofline (SURVEY 8(d) byte model of the
    # reference-equivalent tests over one rank's run time; measured launch traffic beside it)
    model_bytes = int(ci.num_samples) * sum(int(c) * (d + 2) for d, c in enumerate(tests))
    ach = model_bytes / (ms * 1e-3) / 1e9
    roof = {"bound": "latency", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
            "model_bytes_per_run": model_bytes, "per": "one replica (every rank runs the whole search)",
            **pc_small_traffic(),
            "note": "one launch of five dependent levels over a cache-resident column store (DESIGN.md 5.3): "
                    "a latency chain, frac small by construction; wall time includes the record broadcast"}
    return {"metric": "PC-stable CI-tests/sec (alarm_s5000, levels 0-4)", "value": sum(tests) / (ms * 1e-3),
            "unit": "CI-tests/s", "n_gpus": world, "tests": int(sum(tests)), "tests_per_level": tests,
            "launched_per_level": res.launched_per_level.tolist(), "ms_per_run": ms, "edges": len(rec0["edges"]),
            "parallelism": mode, "scaling": "replicas only (a small graph's search does not shard)",
            "timing": "wall clock between barriers, max over ranks, median of runs",
            "matches_single_gpu": int(sum(tests)) == 5206 and len(rec0["edges"]) == 44, "roofline": roof,
            "note": "one launch of five dependent levels (0.14 ms on one GPU): N GPUs cannot shorten it, so "
                    "each rank runs it and rank 0's result record is broadcast (DESIGN.md 6)"}


def bench_pc_synth_dist(steps, rank, world, device, depth=6):
    """BASELINE config 5 on N GPUs (`_pc_dist_timed` over the 1000 x 100k synthetic store); the
    skeleton is checked against the committed fixture (tests/golden/pc_c5.json) on rank 0."""
    res, tests, launched, ms, kern_s = _pc_dist_timed(synth_c5, steps, rank, world, device, depth)
    N = 100_000
    out = {"metric": "PC-stable CI-tests/sec (synthetic 1000 vars x 100k samples, levels 0-5, BASELINE config 5)",
           "value": sum(tests) / (ms * 1e-3), "unit": "CI-tests/s", "n_gpus": world, "tests": int(sum(tests)),
           "tests_per_level": tests, "launched_per_level": launched, "ms_per_run": ms,
           "edges": len(res.edges), "parallelism": f"edge ranges per level x{world}, one all-gather per level",
           "timing": "wall clock between barriers, max over ranks, median of runs",
           "roofline": pc_roofline(kern_s, res.device_bytes, sum(n_d * N * (d + 2) for d, n_d in enumerate(launched)),
                                   world)}
    if rank == 0:
        import json as _json
        sys.path.insert(0, os.path.join(REPO, "tests"))
        from conftest import pc_digest
        ref = _json.load(open(os.path.join(REPO, "tests", "golden", "pc_c5.json")))
        out["matches_fixture"] = (tests == ref["tests_per_level"] and pc_digest(res.edges, res.sepset) ==
                                  {k: ref[k] for k in ("edges_sha256", "sepsets_sha256")})
    return out


def bench_loaders(munin_xml=None):
    """SURVEY §8(f) rank 4 at BASELINE scale: the native seeded generators (numpy-PCG64-identical,
    multi-threaded) against synth.py's numpy versions, and the block-streamed, threaded text
    loaders on a 100k x 1000 CSV (config 5) and a 1M-case LIBSVM test set (config 4: Munin-like,
    208 evidence variables per case), each checked against what was written."""
    import fastbn_amd as F
    from fastbn_amd import synth
    out = {"cpu": host_info()}
    with tempfile.TemporaryDirectory() as td:
        t0 = time.perf_counter()
        cols, dims = synth.config5_dataset()
        out["config5_numpy_generate_s"] = time.perf_counter() - t0
        xml = os.path.join(td, "pc_c5.xml")
        synth.random_network(N_VARS_C5, seed=1000, window=50, parent_probs=(1, 1, 1), dom=(2, 4), path=xml, k_min=0)
        t0 = time.perf_counter()
        cols_n = F.Network(xml).forward_sample(cols.shape[1], 1000)
        out["config5_native_generate_s"] = time.perf_counter() - t0
        out["config5_native_equals_numpy"] = bool(np.array_equal(cols_n, cols))
        csv = os.path.join(td, "c5.csv")
        t0 = time.perf_counter()
        F.write_csv(csv, cols)
        out["csv_write_s"] = time.perf_counter() - t0
        out["csv_bytes"] = os.path.getsize(csv)
        t0 = time.perf_counter()
        ds = F.Dataset(csv)
        out["csv_load_s"] = time.perf_counter() - t0
        out["csv_shape"] = list(ds.columns.shape)
        out["csv_load_GBs"] = out["csv_bytes"] / out["csv_load_s"] / 1e9
        ok = ds.columns.shape == cols.shape
        for v in range(0, cols.shape[0], 97):  # first-appearance recoding, spot columns
            vals, first = np.unique(cols[v], return_index=True)
            m = np.zeros(256, np.uint8)
            m[vals[np.argsort(first)]] = np.arange(len(vals))
            ok = ok and bool(np.array_equal(ds.columns[v], m[cols[v]]))
        out["csv_coding_ok"] = ok
        del ds, cols, cols_n
        os.remove(csv)
        if munin_xml is None:
            munin_xml = os.path.join(td, "munin_like.xml")
            synth.random_network(1041, seed=1041, window=12, path=munin_xml, name="munin_like")
        net = F.Network(munin_xml)
        t0 = time.perf_counter()
        ev = net.evidence_cases(1_000_000, 208, 20250131)
        out["munin_1M_native_generate_s"] = time.perf_counter() - t0
        lib = os.path.join(td, "m1m.libsvm")
        t0 = time.perf_counter()
        F.write_libsvm(lib, ev)
        out["libsvm_write_s"] = time.perf_counter() - t0
        out["libsvm_bytes"] = os.path.getsize(lib)
        t0 = time.perf_counter()
        ev2, _ = F.load_libsvm(lib, net.num_nodes)
        out["libsvm_load_s"] = time.perf_counter() - t0
        out["libsvm_load_GBs"] = out["libsvm_bytes"] / out["libsvm_load_s"] / 1e9
        out["libsvm_rows"] = int(ev2.shape[0])
        out["libsvm_roundtrip_ok"] = bool(np.array_equal(ev, ev2))
    return out


def jt_full_batch_properties(d_ev, d_lab, d_marg, dims, chunk=16384):
    """Size-independent checks over EVERY case of a timed JT batch (not timed; the oracle sample
    beside it covers the values): an evidence variable's marginal row is zero, every other row sums
    to 1 within 1e-12 with entries in [0, 1], and the label is the first strict maximum of variable
    0's marginal, 0 when variable 0 is evidence (InferenceUsingJT / ArgMax, src/Inference.cpp:92-102;
    oracle/jt_oracle.cpp:398-449).  A label that differs where variable 0's top two lie within 1e-12
    relative is counted as a near-tie, any other difference as a mismatch."""
    import torch
    dev = d_marg.device
    dims = np.asarray(dims, np.int64)
    V, d0, n = len(dims), int(dims[0]), d_marg.shape[0]
    col_var = torch.repeat_interleave(torch.arange(V, device=dev), torch.as_tensor(dims, device=dev))
    worst, bad_ev, bad_range, mism, ties = 0.0, 0, 0, 0, 0
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        m, obs = d_marg[a:b], d_ev[a:b] >= 0
        sums = torch.zeros((b - a, V), dtype=m.dtype, device=dev).index_add_(1, col_var, m)
        bad_ev += int((m[obs[:, col_var]] != 0).sum())
        if bool((~obs).any()):
            worst = max(worst, float((sums[~obs] - 1).abs().max()))
        bad_range += int(((m < 0) | (m > 1)).sum())
        m0 = m[:, :d0]
        want = torch.where(obs[:, 0], torch.zeros_like(d_lab[a:b], dtype=torch.long), torch.argmax(m0, 1))
        diff = d_lab[a:b].long() != want
        if bool(diff.any()):
            top = torch.topk(m0[diff], min(2, d0), dim=1).values
            tie = (top[:, 0] - top[:, -1]) <= 1e-12 * top[:, 0]
            ties, mism = ties + int(tie.sum()), mism + int((~tie).sum())
    ok = bad_ev == 0 and worst <= 1e-12 and bad_range == 0 and mism == 0
    return {"cases": int(n), "ok": bool(ok), "evidence_rows_zero": bad_ev == 0, "max_abs_row_sum_err": worst,
            "entries_outside_0_1": bad_range, "label_mismatches": mism, "label_near_ties": ties}


def oracle_sample(n, head, spread):
    """Case indices the oracle checks: the first `head` and `spread` more evenly over the batch, the
    last case included."""
    return np.unique(np.concatenate([np.arange(min(head, n)), np.linspace(0, n - 1, spread).astype(np.int64)]))


def dump_outputs(dirname, d_lab, d_marg, budget=DUMP_BUDGET_BYTES, seed=DUMP_SEED):
    """--dump-outputs: what the last timed step left in its output buffers, as the caller of
    fbn_jt_run_device reads them -- labels.npy (float32 [cases], every case) and marginals.npy
    (float64 [rows][sum_dom], case-major rows whatever the device layout).  All cases' marginals
    where they fit `budget` bytes; else a seeded sample of the cases (ascending, the same for the
    same case count, row size and seed), whose indices go to marginal_cases.npy (float64, exact)."""
    import torch
    os.makedirs(dirname, exist_ok=True)
    n, width = d_marg.shape
    rows = min(n, max(1, budget // (8 * width)))
    if rows < n:
        pick = np.sort(np.random.Generator(np.random.PCG64(seed)).choice(n, size=rows, replace=False))
    else:
        pick = np.arange(n)
    marg = d_marg[torch.from_numpy(pick).to(d_marg.device)].cpu().numpy().astype(np.float64, copy=False)
    files = {"labels": d_lab.cpu().numpy().astype(np.float32), "marginals": np.ascontiguousarray(marg),
             "marginal_cases": pick.astype(np.float64)}
    for name, a in files.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    return {"dir": dirname, "files": {k: list(a.shape) for k, a in files.items()},
            "bytes": int(sum(a.nbytes for a in files.values())),
            "marginal_rows": "all" if rows == n else f"{rows} of {n} cases (PCG64 seed {seed}, ascending)"}


def bench_munin(steps, warmup, cases=125_000, rank=0, world=1, device=0, with_baseline=False, exact=None):
    """the seeded Munin-like 1041-variable network at 20 % evidence (208
    variables per case), 125k cases per GPU -- on 8 GPUs the 1M-case job sharded by rank (seed
    20250131 + rank).  N = 1: kernel time (HIP events); N > 1: wall clock between barriers, max
    over ranks, all ranks' cases."""
    import tempfile
    import torch
    import fastbn_amd as F
    from fastbn_amd import synth
    dev = torch.device("cuda", device)
    tdir = tempfile.TemporaryDirectory()  # holds the XMLBIF until the CPU baseline has run
    path = os.path.join(tdir.name, "munin_like.xml")
    synth.random_network(1041, seed=1041, window=12, path=path, name="munin_like")
    t0 = time.perf_counter()
    fnet = F.Network(path)
    jt = F.JunctionTree(fnet, device=device)
    jt.set_exact(exact)
    plan_s = time.perf_counter() - t0
    # native generator (bit-identical to synth.evidence_cases, multi-threaded)
    ev = fnet.evidence_cases(cases, 208, shard.synthetic_seed(20250131, rank))
    pick = oracle_sample(cases, 16, 48)  # ~20 ms of the oracle per Munin-like case
    if rank == 0:
        sys.path.insert(0, os.path.join(REPO, "oracle"))
        import oracle as O
        olab, omarg = O.OracleJT(path).infer(ev[pick])
    d_ev = torch.from_numpy(ev).to(dev)
    d_lab = torch.empty(cases, dtype=torch.int32, device=dev)
    d_marg = torch.empty((cases, jt.info["sum_dom"]), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    # the evidence buffer is validated once (device-side range check); the timed runs reuse it
    jt.validate_device(d_ev.data_ptr(), cases, stream)
    jt.set_evidence_check(False)
    for _ in range(max(1, warmup)):
        jt.run_device(d_ev.data_ptr(), cases, d_lab.data_ptr(), d_marg.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    ok, rel = True, None
    if rank == 0:  # auto arithmetic order for this plan = fast (fbn_jt_set_exact): labels equal, marginals ~1e-15
        ip = torch.from_numpy(pick).to(dev)
        gm = d_marg[ip].cpu().numpy()
        rel = float(np.max(np.abs(gm - omarg) / np.maximum(np.abs(omarg), 1e-300)))
        ok = bool((d_lab[ip].cpu().numpy() == olab).all() and rel <= 1e-12)
    props = jt_full_batch_properties(d_ev, d_lab, d_marg, fnet.dims)
    ms = []
    all_lab = None
    if world > 1:
        import torch.distributed as dist
        nccl = dist.get_backend() == "nccl"
        all_lab = torch.empty(world * cases, dtype=torch.int32, device=dev if nccl else "cpu")
        dist.barrier()
    torch.cuda.synchronize(dev)
    w0 = time.perf_counter()
    for _ in range(steps):
        jt.run_device(d_ev.data_ptr(), cases, d_lab.data_ptr(), d_marg.data_ptr(), stream)
        ms.append(jt.last_kernel_ms())
        if all_lab is not None:  # the final gather of every rank's labels (north_star), inside the timing
            if nccl:
                dist.all_gather_into_tensor(all_lab, d_lab)
            else:
                dist.all_gather(list(all_lab.view(world, cases)), d_lab.cpu())
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    wall = shard.max_over_ranks(time.perf_counter() - w0, dev)
    k = float(np.median(ms))
    bpc = jt.info["algorithmic_bytes_per_case"]
    cb = cpu_baseline_munin(path, ev) if (rank == 0 and world == 1 and with_baseline) else None
    tdir.cleanup()
    value = cases / (k * 1e-3) if world == 1 else world * cases * steps / wall
    return {"metric": "JT test-cases/sec (Munin-like 1041 vars, 20 % evidence)", "value": value,
            "unit": "cases/s", "n_gpus": world, "cases": cases * world, "cases_per_gpu": cases, "kernel_ms": k,
            "wall_ms_per_step": 1e3 * wall / steps, "plan_s": plan_s,
            "kernel_variant": jt.refresh_info()["variant"],
            "arithmetic_order": "exact" if exact else "fast (normalizations cancel; labels equal, marginals within 1e-12)",
            "parity_vs_oracle": {"cases": int(len(pick)), "sample": "first 16 + 48 spread over the batch",
                                 "labels_equal_and_marg_within_1e-12": bool(ok), "max_rel_err": rel},
            "full_batch_properties": props,
            "cliques": jt.info["num_cliques"], "clique_entries": jt.info["clique_entries"],
            "roofline": {"bound": "hbm", "achieved": bpc * cases / (k * 1e-3) / 1e9, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": bpc * cases / (k * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "algorithmic_bytes_per_case": bpc, **munin_traffic(cases, k),
                         "valu": valu_roofline("munin", cases, k)},
            **({"cpu_baseline": cb} if cb else {})}


def munin_traffic(cases, kernel_ms):
    """Measured L2<->fabric bytes of the streamed kernel (rocprofv3 FETCH_SIZE + WRITE_SIZE, calibrated;
    committed summary profiles/r06/munin_traffic.json from tools/profile_r06_munin.sh), scaled to this launch,
    and the rate they imply at this launch's kernel time."""
    path = _first_profile("r06/munin_traffic.json", "r05/munin_traffic.json", "munin_traffic.json")
    if path is None:
        return {"traffic": None}
    with open(path) as f:
        t = json.load(f)
    b = t["hbm_bytes_per_launch"] * cases / t["cases_per_launch"]
    return {"traffic": b, "traffic_rate_GBs": b / (kernel_ms * 1e-3) / 1e9,
            "traffic_frac": b / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "traffic_note": "the tiled kernel recomputes every clique entry from its initial potential and the "
                            "separator messages instead of storing clique tables; its measured traffic is the "
                            "message rows re-read from L2 misses plus the per-wave message store (DESIGN.md 5.2)"}


VALU_PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9  # MI355X: CUs x SIMDs x lanes x clock (fp64 FMA full rate)


def valu_roofline(which, cases, kernel_ms):
    """The VALU roofline of a JT kernel: measured fp64 VALU instructions per launch (rocprofv3
    SQ_INSTS_VALU_{ADD,MUL,FMA,TRANS}_F64, committed summary profiles/r05/jt_valu.json from
    tools/profile_r05.sh) scaled to this launch, as wave64 lane-ops per second against the fp64
    vector peak (a wave64 fp64 instruction holds its SIMD 4 cycles, so frac <= 1 by construction);
    all VALU instructions (SQ_INSTS_VALU, incl. 32-bit selects / integer ops) beside it."""
    for path in (os.path.join(REPO, "profiles", r, "jt_valu.json") for r in ("r06", "r05", ".")):
        if os.path.exists(path):
            break
    else:
        return None
    with open(path) as f:
        t = json.load(f)[which]
    sc = cases / t["cases_per_launch"]
    insts = t["valu_insts_per_launch"] * sc
    f64 = t.get("f64_insts_per_launch")
    if f64 is None:  # (older profile: total VALU only)
        ach = insts * 64 / (kernel_ms * 1e-3)
        return {"bound": "valu", "achieved": ach / 1e12, "peak": VALU_PEAK_LANE_OPS / 1e12, "unit": "Tlane-op/s",
                "frac": ach / VALU_PEAK_LANE_OPS, "valu_insts": insts, "source": os.path.relpath(path, REPO)}
    f64 *= sc
    ach = f64 * 64 / (kernel_ms * 1e-3)
    return {"bound": "valu_f64", "achieved": ach / 1e12, "peak": VALU_PEAK_LANE_OPS / 1e12, "unit": "Tlane-op/s",
            "frac": ach / VALU_PEAK_LANE_OPS, "f64_insts": f64, "valu_insts": insts,
            "all_valu_frac": insts * 64 / (kernel_ms * 1e-3) / VALU_PEAK_LANE_OPS,
            "source": os.path.relpath(path, REPO)}


def load_traffic(cases):
    """Measured HBM bytes per launch (rocprofv3 FETCH_SIZE + WRITE_SIZE, calibrated; committed
    summary profiles/r05/jt_traffic.json, else profiles/jt_traffic.json), scaled to this launch's cases."""
    for path in (os.path.join(REPO, "profiles", r, "jt_traffic.json") for r in ("r06", "r05", ".")):
        if os.path.exists(path):
            break
    else:
        return None
    with open(path) as f:
        t = json.load(f)
    b = t.get("hbm_bytes_per_launch")
    return None if b is None else b * cases / t.get("cases_per_launch", CASES_PER_GPU)


def alarm_roofline(info, cases, kernel_ms, traffic):
    """The ALARM kernel's (fbn_jt_gen, variant 3) roofline against the resource it uses most
    (DESIGN.md 5.1).  It keeps every clique table in registers / LDS, so it moves the compulsory
    bytes (evidence in, marginals + labels out: V + 8 sum_dom + 4 B per case) plus the message rows
    its per-wave workspace sends past L2; `traffic` = those measured L2<->fabric bytes (calibrated
    PMC FETCH + WRITE per launch, scaled to this launch).  The other candidate bound is the issue of
    its fp64 VALU instructions (measured per launch, against the fp64 vector peak).  `bound` is
    whichever of the two fractions is higher; the other stands beside it.  SURVEY 8(d)'s
    materialized-table bytes (every table written and read once) are kept as `model`, informational:
    this design does not move them, so that ratio exceeds 1."""
    comp = info["num_nodes"] + 8 * info["sum_dom"] + 4
    t = kernel_ms * 1e-3
    hbm = {"compulsory_bytes_per_case": comp, "compulsory_achieved": comp * cases / t / 1e9,
           "compulsory_frac": comp * cases / t / 1e9 / HBM_PEAK_GBS, "traffic": traffic,
           "traffic_per_case": traffic / cases if traffic else None,
           "achieved": traffic / t / 1e9 if traffic else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": traffic / t / 1e9 / HBM_PEAK_GBS if traffic else None}
    bpc = info["algorithmic_bytes_per_case"]
    model = {"bytes_per_case": bpc, "achieved": bpc * cases / t / 1e9, "model_frac": bpc * cases / t / 1e9 / HBM_PEAK_GBS,
             "note": "informational: SURVEY 8(d)'s materialized-table bytes, which this kernel does not move"}
    v = valu_roofline("alarm", cases, kernel_ms)
    base = {"kernel_ms": kernel_ms, "traffic": traffic, "hbm": hbm, "model": model, "valu": v}
    if hbm["frac"] is not None and (v is None or hbm["frac"] >= v["frac"]):
        return {"bound": "hbm", "achieved": hbm["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": hbm["frac"],
                **base, "note": "measured L2<->fabric traffic per launch over the kernel time (the higher of the "
                                "two fractions; fp64 VALU issue beside it in `valu`)"}
    if v is None:
        return {"bound": "hbm", "achieved": hbm["compulsory_achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": hbm["compulsory_frac"], **base}
    return {**{k: v[k] for k in ("bound", "achieved", "peak", "unit", "frac")}, **base,
            "note": "fp64 VALU issue (the higher of the two fractions; measured traffic beside it in `hbm`)"}


def summary(out):
    """Every workload's headline number in a few hundred bytes (the end of the JSON line)."""
    def r(x, n=4):
        return None if x is None else float(f"{x:.{n}g}")
    sm = {"alarm_jt": {"cases_s": r(out["value"]), "kernel_ms": r(out["roofline"]["kernel_ms"]),
                       "frac": r(out["roofline"]["frac"], 3), "bound": out["roofline"]["bound"]}}
    pc = out.get("pc_stable")
    if pc:
        sm["alarm5000_pc"] = {"ms_call": r(pc["ms_per_run"]), "tests_s": r(pc["value"]),
                              "frac": r(pc.get("roofline", {}).get("frac"), 3),
                              "parallelism": "replicas" if "replicas" in pc.get("parallelism", "replicas") else "split"}
    mu = out.get("munin_like")
    if mu:
        tr = mu["roofline"].get("traffic")
        sm["munin_jt"] = {"cases_s": r(mu["value"]), "kernel_ms": r(mu["kernel_ms"]), "frac": r(mu["roofline"]["frac"], 3),
                          "traffic_MB_case": r(tr / mu["cases_per_gpu"] / 1e6, 3) if tr else None,
                          "variant": mu.get("kernel_variant")}
    c5 = out.get("pc_synthetic")
    if c5:
        sm["config5_pc"] = {"ms_run": r(c5["ms_per_run"]), "tests_s": r(c5["value"]),
                            "frac": r(c5.get("roofline", {}).get("frac"), 3), "bound": c5.get("roofline", {}).get("bound")}
    return sm


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n, argv):
    """`bench.py --gpus N` started without a launcher (no WORLD_SIZE in the environment): start N
    rank processes -- the same torch.distributed.run command the driver uses, one process per GPU,
    rendezvous on 127.0.0.1 -- and return their exit code.  Called before this process touches torch
    or the GPU; the ranks are children (no exec), rank 0's JSON line reaches stdout unchanged."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    log(f"bench: --gpus {n} without WORLD_SIZE: launching {n} ranks ({' '.join(cmd[1:6])} ...)")
    return subprocess.run(cmd, env=dict(os.environ)).returncode


def launcher_check(world, rank):
    """--launcher-check: the rank plumbing alone, on the CPU (gloo), no GPU and no workload -- every
    rank joins the group, the barrier / max-over-ranks timing runs, and rank 0 prints the world size
    the group reports and the ranks it saw (tests/test_bench_checks.py).  Not a measurement."""
    import torch
    import torch.distributed as dist
    t0 = time.perf_counter()
    dist.barrier()
    elapsed = shard.max_over_ranks(time.perf_counter() - t0)
    seen = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(seen, torch.tensor([rank], dtype=torch.int64))
    if rank == 0:
        print(json.dumps({"launcher_check": True, "n_gpus": world, "world_size_seen": dist.get_world_size(),
                          "ranks_seen": [int(s.item()) for s in seen], "backend": dist.get_backend(),
                          "barrier_s": elapsed}), flush=True)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: 100 timed steps (12 ms at N = 1) after 100 warm-up steps -- a cold MI355X needs
    # ~15 ms of work to reach steady clocks (tools/alarm_knob_probe.py: 0.124 ms per step over the first
    # 50 steps, 0.117 from ~150 on); the driver's own --steps / --warmup take precedence
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--cases", type=int, default=CASES_PER_GPU)
    ap.add_argument("--waves-per-cu", type=int, default=0)
    ap.add_argument("--full", action="store_true",
                    help="after the headline: the oracle / full-batch checks of the last step, the PCIe-inclusive "
                         "rate, PC-stable, Munin-like JT, loaders and the CPU baselines (minutes); --no-* trim it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's labels and marginals to DIR/<name>.npy (rank 0)")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-pc", action="store_true")
    ap.add_argument("--no-munin", action="store_true")
    ap.add_argument("--no-loaders", action="store_true")
    ap.add_argument("--launcher-check", action="store_true",
                    help="CPU-only check of the rank launch (gloo, no workload); not a measurement")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    # --gpus N is the number of rank processes.  Under a launcher (torchrun sets WORLD_SIZE) the two
    # must agree; without one, N > 1 starts the ranks here, before anything touches the GPU.
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))
    world = int(env_world) if env_world is not None else 1
    if world != args.gpus:
        log(f"ERROR: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
        sys.exit(2)

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.launcher_check:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        launcher_check(world, rank)
        return
    # FBN_BENCH_BACKEND=gloo + more ranks than GPUs: a rehearsal of the N > 1 path on a small box
    # (ranks share GPUs round-robin); the measured runs use RCCL, one rank per GPU
    backend = os.environ.get("FBN_BENCH_BACKEND", "nccl")
    if backend == "nccl" and world > torch.cuda.device_count():
        log(f"ERROR: {world} ranks over RCCL need {world} GPUs; {torch.cuda.device_count()} visible "
            f"(FBN_BENCH_BACKEND=gloo rehearses ranks sharing a GPU)")
        sys.exit(2)
    if backend != "nccl":
        local = local % max(1, torch.cuda.device_count())
    if world > 1 or os.environ.get("FBN_BENCH_FORCE_GATHER") == "1":
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))  # (world 1: no launcher set one)
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(0)

    import fastbn_amd as F
    from fastbn_amd import synth

    alarm_net = F.Network(os.path.join(ALARM, "alarm.xml"))
    # native generator (bit-identical to synth.evidence_cases, multi-threaded)
    ev = alarm_net.evidence_cases(args.cases, EVIDENCE_PER_CASE, shard.synthetic_seed(20250131, rank))
    jt = F.JunctionTree(alarm_net, device=local)
    if args.waves_per_cu:
        jt.set_waves_per_cu(args.waves_per_cu)
    info = jt.info
    dev = torch.device("cuda", local)
    d_ev = torch.from_numpy(ev).to(dev)
    d_lab = torch.empty(args.cases, dtype=torch.int32, device=dev)
    # marginals variable-major [sum_dom][cases] on the device (fbn_jt_set_output_layout 1: every
    # store of the kernel writes 64 consecutive cases of one value, each line written once); the
    # checks below read them through the transposed view (case-major rows, the reference's vectors)
    layout = 0 if os.environ.get("FBN_BENCH_CASE_MAJOR") == "1" else 1
    jt.set_output_layout(layout)
    d_marg_buf = torch.empty(args.cases * info["sum_dom"], dtype=torch.float64, device=dev)
    d_marg = (d_marg_buf.view(info["sum_dom"], args.cases).t() if layout == 1
              else d_marg_buf.view(args.cases, info["sum_dom"]))
    stream = torch.cuda.current_stream(dev)
    # the evidence buffer is validated once (device-side range check, fbn_jt_evidence_validate);
    # the timed steps reuse the unchanged buffer without the per-call check (fully asynchronous)
    jt.validate_device(d_ev.data_ptr(), args.cases, stream.cuda_stream)
    jt.set_evidence_check(False)
    jt.set_kernel_timing(False)  # (the steps are timed with events on the stream below: no extra markers)

    # N > 1: north_star's "final gather" -- every step's labels (4 B per case) stay on the device
    # (one slice per timed step) and ONE all-gather at the end of the timed region sends every
    # rank's labels of every step to every rank (RCCL on the device; the gloo rehearsal stages
    # through the host).  Marginals stay on the device; there is no golden table for
    # synthetic cases, so no MSE / HD sum to reduce.  (A per-step all-gather measured +24 us per
    # step at world size 1 even asynchronous: the collective's call overhead.)
    # (FBN_BENCH_FORCE_GATHER=1: the gather at world size 1 too -- a test of the RCCL path)
    gathering = world > 1 or (os.environ.get("FBN_BENCH_FORCE_GATHER") == "1" and dist.is_initialized())
    # (without the gather nothing reads the older slices: at most MAX_LABEL_SLICES, reused in turn, so
    # a long --steps run does not grow with its step count)
    slices = args.steps if gathering else min(args.steps, MAX_LABEL_SLICES)
    step_labs = torch.empty((slices, args.cases), dtype=torch.int32, device=dev)
    all_labs = torch.empty(world * step_labs.numel(), dtype=torch.int32, device=dev) if gathering else None

    def step(i=0):
        lab = step_labs[i % step_labs.shape[0]]
        jt.run_device(d_ev.data_ptr(), args.cases, lab.data_ptr(), d_marg_buf.data_ptr(), stream.cuda_stream)

    def final_gather():
        if not gathering:
            return
        if backend == "nccl":
            dist.all_gather_into_tensor(all_labs, step_labs.view(-1))
        else:
            parts = [torch.empty(step_labs.numel(), dtype=torch.int32) for _ in range(world)]
            dist.all_gather(parts, step_labs.view(-1).cpu())
            all_labs.copy_(torch.cat(parts))

    for i in range(args.warmup):
        step(i)
    final_gather()
    torch.cuda.synchronize(dev)
    # one event pair on the launch stream around the K steps (per-step pairs would add two markers
    # to every step): kernel_ms = the steps' average device time, launch gaps and the fixup check
    # included, so it bounds rocprofv3's fbn_jt_gen average from above
    ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    ev_a.record(stream)
    for i in range(args.steps):
        step(i)
    ev_b.record(stream)
    final_gather()  # part of the timed region
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    elapsed = shard.max_over_ranks(elapsed, dev)  # identity at N = 1
    kernel_ms = ev_a.elapsed_time(ev_b) / max(1, args.steps)

    d_lab = step_labs[(args.steps - 1) % step_labs.shape[0]]  # the last step's labels (checked below)
    if gathering:  # the gathered labels hold every rank's labels of every step, in rank order
        n1 = step_labs.numel()
        assert torch.equal(all_labs[rank * n1:(rank + 1) * n1], step_labs.view(-1)), "label all-gather"
    dumped = dump_outputs(args.dump_outputs, d_lab, d_marg) if (args.dump_outputs and rank == 0) else None
    checks = {}
    if args.full:
        # sanity: labels of the last step agree with a CPU recomputation on a few cases (not timed)
        if rank == 0:
            sys.path.insert(0, os.path.join(REPO, "oracle"))
            import oracle as O
            pick = oracle_sample(args.cases, 256, 1792)
            olab, omarg = O.OracleJT(os.path.join(ALARM, "alarm.xml")).infer(ev[pick])
            # default (fast) arithmetic order: labels equal, marginals within 1e-12 relative
            ip = torch.from_numpy(pick).to(dev)
            gm = d_marg[ip].cpu().numpy()
            alarm_rel = float(np.max(np.abs(gm - omarg) / np.maximum(np.abs(omarg), 1e-300)))
            ok = (d_lab[ip].cpu().numpy() == olab).all() and alarm_rel <= 1e-12
            if not ok:
                log("ERROR: GPU results differ from the oracle")
                sys.exit(1)
        # every case of the last step: size-independent properties (each rank its own shard)
        alarm_props = jt_full_batch_properties(d_ev, d_lab, d_marg, alarm_net.dims)
        if not alarm_props["ok"]:
            log(f"ERROR: full-batch properties violated: {alarm_props}")
            sys.exit(1)
        checks = {"parity_vs_oracle": {"cases": int(len(pick)) if rank == 0 else None,
                                       "sample": "first 256 + 1792 spread over the batch", "labels_equal": True,
                                       "max_rel_err": alarm_rel if rank == 0 else None},
                  "full_batch_properties": alarm_props}

    total_cases = args.cases * args.steps * world
    value = total_cases / elapsed
    traffic = load_traffic(args.cases)
    roof = alarm_roofline(info, args.cases, kernel_ms, traffic)
    out = {
        "metric": "JT test-cases/sec (ALARM, Munin) + PC-stable CI-tests/sec, 1/2/4/8 GPU",
        "value": value,
        "unit": "cases/s",
        "n_gpus": world,
        "world_size_seen": dist.get_world_size() if dist.is_initialized() else 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "full": args.full,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic (ALARM forward samples, seed 20250131+rank)",
        "config": {"workload": "ALARM (37 vars) JT inference, 100k synthetic cases per GPU @ 7 evidence vars "
                               "(BASELINE config 2)", "cases_per_gpu": args.cases,
                   "evidence_per_case": EVIDENCE_PER_CASE,
                   "marginal_layout": ("variable-major [sum_dom][cases] (fbn_jt_set_output_layout 1)" if layout == 1
                                       else "case-major [cases][sum_dom]"),
                   "parallelism": f"case-sharded x{world}" + (" + one labels all-gather of every step (final gather)"
                                                              if world > 1 else "")},
        "roofline": {**roof, "kernel_variant": jt.refresh_info()["variant"],
                     "arithmetic_order": "fast (normalizations cancel; labels equal, marginals within 1e-12)",
                     **checks},
    }
    if dumped:
        out["dumped_outputs"] = dumped
    # everything below is beside the headline: --full only
    if args.full and world > 1 and not args.no_munin:
        # BASELINE config 4 at its real scale: 125k Munin-like cases per rank (1M on 8 GPUs)
        out["munin_like"] = bench_munin(3, 1, rank=rank, world=world, device=local)
    if args.full and world > 1 and not args.no_pc:
        # BASELINE configs 3 and 5 on N GPUs: edge ranges per level, one all-gather per level
        out["pc_stable"] = bench_pc_alarm_dist(10, rank, world, local)
        out["pc_synthetic"] = bench_pc_synth_dist(5, rank, world, local)
    if args.full and rank == 0 and world == 1:
        # PCIe-inclusive rate (host evidence in, host labels + marginals out through fbn_jt_run):
        # reported beside the metric, never as `value`
        log("bench: PCIe-inclusive JT rate")
        t_host = []
        for _ in range(3):
            t0 = time.perf_counter()
            jt.infer(ev)
            t_host.append(time.perf_counter() - t0)
        out["pcie_inclusive"] = {"value": args.cases / float(np.median(t_host)), "unit": "cases/s",
                                 "note": "fbn_jt_run from host buffers: evidence H2D, kernel, labels + "
                                         f"{info['sum_dom']} marginals per case D2H"}
        if not args.no_pc:
            log("bench: PC-stable ALARM-5000")
            out["pc_stable"] = bench_pc(max(50, args.steps), args.warmup)  # 0.3 ms per call: 50 calls for a stable median
        if not args.no_munin:
            log("bench: Munin-like JT")
            out["munin_like"] = bench_munin(3, 1, with_baseline=not args.no_baseline)
        if not args.no_pc:
            log("bench: PC-stable config 5")
            out["pc_synthetic"] = bench_pc_synth(5, with_baseline=not args.no_baseline)
        if not args.no_loaders:
            log("bench: loaders")
            out["loaders"] = bench_loaders()
        if not args.no_baseline:
            log("bench: reference JT baseline (ALARM)")
            out["cpu_baseline"] = cpu_baseline_jt()
            if "pc_stable" in out:
                out["pc_stable"]["cpu_baseline"] = cpu_baseline_pc_alarm()
    if rank == 0:
        out["summary"] = summary(out)  # last key: survives a tail-truncated record of this line
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
