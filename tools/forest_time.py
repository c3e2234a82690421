"""Cost of a junction forest beside the tree of its one large component.

    python tools/forest_time.py [--out profiles/forest/forest_time.json] [--cases 100000]

Workload: the network the documented pipeline learns from ALARM-5000 (PCStable(0.05) -> pdag_to_dag
-> ParameterLearning), 37 nodes of which node 12 has no edge.  `forest` = JunctionForest on all 37
nodes; `tree` = JunctionTree on the 36-node component, the same evidence columns (node 12
unobserved and left out).  Both device-resident (fbn_jt_run_device on buffers already on the
device, evidence validated once, the per-run check off), default variant and order, 10 warm-up + 100
timed runs each, the two plans alternating run by run, host clock around a run that ends in a stream
synchronise, and the kernel time of the library's own events.  The measurement runs in a child
process under a time limit; its exit code and last stderr lines are recorded.  Recorded, not gated:
a forest has no earlier equivalent.
Also recorded: the plans' clique / separator entry counts and the specialized kernel's message rows
per place, which is what a ratio away from 1 would have to be explained from."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
LIMIT = 300  # seconds


def child(ncases):
    import torch

    import fastbn_amd as F
    ds = F.Dataset(os.path.join(REPO, "tests", "golden", "alarm", "alarm_s5000.txt"))
    pc = F.PCStable(0.05, 1000).StructLearnCompData(ds)
    dag = F.pdag_to_dag(ds.num_vars, pc.oriented)
    learned = F.ParameterLearning(pc.ci).LearnParamsKnowStructCompData(dag, names=ds.names)
    forest = F.JunctionForest(learned, device=0)
    big = max(forest.components, key=len)
    idx = {v: i for i, v in enumerate(big)}
    sub = F.Network.from_counts(learned.dims[big], [[idx[int(q)] for q in learned.node_counts(v)[0]] for v in big],
                                [learned.node_counts(v)[1] for v in big])
    tree = F.JunctionTree(sub, device=0)
    ev = learned.evidence_cases(ncases, 7, seed=1)
    ev[:, [v for v in range(learned.num_nodes) if v not in idx]] = -1
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {"ncases": int(ncases), "components": [len(c) for c in forest.components]}
    margs, runs = {}, {}
    for name, jt, e in (("forest", forest, ev), ("tree", tree, np.ascontiguousarray(ev[:, big]))):
        n, SD = len(e), jt.info["sum_dom"]
        d_ev = torch.from_numpy(e).to(dev)
        d_lab = torch.empty(n, dtype=torch.int32, device=dev)
        d_marg = torch.empty((n, SD), dtype=torch.float64, device=dev)
        jt.validate_device(d_ev.data_ptr(), n, stream)
        jt.set_evidence_check(False)
        runs[name] = (jt, d_ev, d_lab, d_marg, [], [])
    for i in range(110):  # alternating, so that drift of the shared machine hits both alike
        for jt, d_ev, d_lab, d_marg, wall, kern in runs.values():
            t0 = time.perf_counter()
            jt.run_device(d_ev.data_ptr(), len(d_ev), d_lab.data_ptr(), d_marg.data_ptr(), stream)
            torch.cuda.synchronize(dev)
            if i >= 10:
                wall.append((time.perf_counter() - t0) * 1e3)
                kern.append(jt.last_kernel_ms())
    for name, (jt, d_ev, d_lab, d_marg, wall, kern) in runs.items():
        info = jt.refresh_info()
        margs[name] = d_marg.cpu().numpy()
        out[name] = {"variant": info["variant"], "wall_ms_median": float(np.median(wall)), "wall_ms_min": float(np.min(wall)),
                     "kernel_ms_median": float(np.median(kern)), "kernel_ms_min": float(np.min(kern)), "timed_runs": len(wall),
                     "flagged_blocks": jt.debug_flagged_blocks(),
                     **{k: int(info[k]) for k in ("num_cliques", "num_separators", "clique_entries", "separator_entries", "sum_dom")},
                     **{k: int(v) for k, v in info.items() if k.startswith("place_rows_")}}
    # the two agree on the large component's marginals
    off = np.concatenate([[0], np.cumsum(learned.dims)])
    cols = np.concatenate([np.arange(off[v], off[v + 1]) for v in big])
    a, b = margs["forest"][:, cols], margs["tree"]
    out["max_rel_diff"] = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))
    out["kernel_ratio_forest_over_tree"] = out["forest"]["kernel_ms_median"] / out["tree"]["kernel_ms_median"]
    out["wall_ratio_forest_over_tree"] = out["forest"]["wall_ms_median"] / out["tree"]["wall_ms_median"]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "forest", "forest_time.json"))
    ap.add_argument("--cases", type=int, default=100000)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.cases)
        return 0
    rec = {"tool": "tools/forest_time.py", "time_limit_s": LIMIT}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--cases", str(a.cases)],
                           capture_output=True, text=True, timeout=LIMIT)
        rec["exit_code"] = r.returncode
        rec["stderr_tail"] = r.stderr.strip().split("\n")[-8:] if r.stderr.strip() else []
        lines = [ln for ln in r.stdout.split("\n") if ln.startswith("{")]
        if r.returncode == 0 and lines:
            rec.update(json.loads(lines[-1]))
    except subprocess.TimeoutExpired as e:
        rec["exit_code"] = "time limit"
        err = e.stderr.decode() if isinstance(e.stderr, bytes) else (e.stderr or "")
        rec["stderr_tail"] = err.strip().split("\n")[-8:]
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0 if rec["exit_code"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
