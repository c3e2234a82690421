"""Timing of exact posterior sampling (jt_psample.hip) beside the two kernels that walk the same Collect on
the same cases: most probable explanation (jt_mpe.hip) and the E-step (jt_em.hip).

    python tools/psample_time.py [--out profiles/psample/psample_time.json] [--workloads a,b]
                                 [--u-sweep 1=lib1.so,2=lib2.so,4=lib4.so]

Workloads: ALARM, 100,000 cases with 7 observed variables, 1 and 16 draws per case; ALARM, one case, 2^20
draws (the item remap and the chunked path); Munin-like (1041 variables), 125,000 cases with 208 observed,
1 draw.  Evidence: the seeded generator's cases.  Each workload runs in a child process of its own under a
time limit; its exit code and last stderr lines are recorded, and no further child is started after one
that did not exit 0.

Per workload: kernel ms (fbn_psample_last_kernel_ms: HIP events, median of 5 timed calls after 2 warm-up
calls), draws/s, and the kernel ms of MPE and of the E-step on the same cases (median of 3 after one
warm-up).  They compute other things (one arg-max trace; a Distribute pass and family posteriors), so the
ratios say what the draws cost next to a pass over the same forest, nothing more.  The first 64 cases are
checked against the host twin byte for byte before anything is timed.

--u-sweep: builds of the library that differ in kPsampleU (jt_psample_program.h), the draws a lane keeps in
flight; the 16-draw and the one-case workloads are timed with each through FBN_LIB_PATH."""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GOLD = os.path.join(REPO, "tests", "golden")
# name -> (network, cases, observed per case, draws per case)
WORK = {"psample_alarm_100k_s1": ("alarm", 100_000, 7, 1), "psample_alarm_100k_s16": ("alarm", 100_000, 7, 16),
        "psample_alarm_1case_s1m": ("alarm", 1, 7, 1 << 20), "psample_munin_125k_s1": ("munin", 125_000, 208, 1)}
LIMITS = {"psample_alarm_100k_s1": 240, "psample_alarm_100k_s16": 240, "psample_alarm_1case_s1m": 240,
          "psample_munin_125k_s1": 600}
SWEEP = ("psample_alarm_100k_s16", "psample_alarm_1case_s1m")


def network(name, tmp):
    import fastbn_amd as F
    if name == "alarm":
        return F.Network(os.path.join(GOLD, "alarm", "alarm.xml"))
    xml = os.path.join(tmp, name + ".xml")
    with gzip.open(os.path.join(GOLD, "munin_like", "munin_like.xml.gz"), "rb") as f, open(xml, "wb") as g:
        g.write(f.read())
    return F.Network(xml)


def kernel_ms(call, handle, warm, reps):
    for _ in range(warm):
        call()
    ms = []
    for _ in range(reps):
        call()
        ms.append(handle.last_kernel_ms())
    return float(np.median(ms)), float(np.min(ms))


def child(name, yardsticks):
    import fastbn_amd as F
    which, ncases, k, draws = WORK[name]
    with tempfile.TemporaryDirectory() as tmp:
        net = network(which, tmp)
    ev = net.evidence_cases(max(ncases, 64), k, seed=1)
    dev = F.PosteriorSampler(net)
    s, v = dev.value_parts(ev[:64], 3, seed=1)
    hs, hv = F.PosteriorSampler(net, device=-1).value_parts(ev[:64], 3, seed=1)
    assert s.tobytes() == hs.tobytes() and v.tobytes() == hv.tobytes(), "device differs from the host twin"
    ev = ev[:ncases]
    med, low = kernel_ms(lambda: dev.value_parts(ev, draws, seed=1), dev, 2, 5)
    rec = {"workload": name, "nvars": net.num_nodes, "ncases": ncases, "observed_per_case": k, "draws_per_case": draws,
           **dev.info(), "kernel_ms_median": med, "kernel_ms_min": low, "draws_per_s_kernel": ncases * draws / (med * 1e-3)}
    if yardsticks:
        mpe = F.MostProbableExplanation(net)
        rec["mpe_kernel_ms_median"] = kernel_ms(lambda: mpe.value_parts(ev), mpe, 1, 3)[0]
        em = F.ExpectationMaximization(net)
        rec["estep_kernel_ms_median"] = kernel_ms(lambda: em.estep_flat(ev), em, 1, 3)[0]
        rec["ratio_psample_over_mpe"] = med / rec["mpe_kernel_ms_median"]
        rec["ratio_psample_over_estep"] = med / rec["estep_kernel_ms_median"]
    print(json.dumps(rec))


def run_child(name, extra, env=None):
    rec = {"workload": name, "time_limit_s": LIMITS[name]}
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name], env=env)
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
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "psample", "psample_time.json"))
    ap.add_argument("--workloads", default=",".join(LIMITS))
    ap.add_argument("--u-sweep", default="", help="U=library path, comma separated")
    ap.add_argument("--no-yardsticks", action="store_true")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        child(a.child, not a.no_yardsticks)
        return 0
    results, sweep = [], []
    ok = True
    for name in [w for w in a.workloads.split(",") if w]:
        results.append(run_child(name, []))
        ok = results[-1]["exit_code"] == 0
        if not ok:
            break  # nothing more is started on a device a child may have left in a bad state
    for item in [x for x in a.u_sweep.split(",") if x and ok]:
        u, path = item.split("=")
        for name in SWEEP:
            if not ok:
                break
            rec = run_child(name, ["--no-yardsticks"], dict(os.environ, FBN_LIB_PATH=os.path.abspath(path)))
            rec["draws_in_flight"] = int(u)
            sweep.append(rec)
            ok = rec["exit_code"] == 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/psample_time.py", "workloads": results, "u_sweep": sweep}, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
