"""Junction forests on the device: a plan from fbn_jt_forest_plan_create through every
kernel variant that takes it, both arithmetic orders and both output layouts, against enumeration
of the joint, against JunctionTree on each component alone, and end to end on the network PC-stable
learns from ALARM-5000 (node 12 isolated).  130 cases: two full blocks of 64 and a tail of 2."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ALARM, REPO

import fastbn_amd as F
import jt_forest_nets as N
from fastbn_amd import synth
from test_jt_forest_host import read_plan, special_cases
from test_lbp_host import brute_force, disconnected_network, net_tuple, polytree_cases

pytestmark = pytest.mark.gpu
TOL = 1e-12
NCASES = 130


def _close(marg, ref):
    np.testing.assert_allclose(marg, ref, rtol=TOL, atol=1e-300)


def run_device(jt, ev):
    """(labels, marginals [n][sum_dom]) through fbn_jt_run_device in the plan's output layout."""
    import torch
    n, SD, dev = len(ev), jt.info["sum_dom"], torch.device("cuda", 0)
    d_ev = torch.from_numpy(np.array(ev, np.int8)).to(dev)
    d_lab = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_marg = torch.full((n * SD,), float("nan"), dtype=torch.float64, device=dev)
    jt.run_device(d_ev.data_ptr(), n, d_lab.data_ptr(), d_marg.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    marg = d_marg.cpu().numpy()
    marg = marg.reshape(SD, n).T if jt.output_layout == 1 else marg.reshape(n, SD)
    return d_lab.cpu().numpy(), np.ascontiguousarray(marg)


@functools.lru_cache(maxsize=None)
def small():
    """disconnected_network(), its 130 cases and their enumerated posteriors (shared, read-only)."""
    dims, parents, counts = disconnected_network()
    ev = np.concatenate([polytree_cases(dims, NCASES - 3, 2), special_cases(dims)])
    tup = net_tuple(dims, parents, counts)
    exact = np.stack([brute_force(tup, e) for e in ev])
    # labels: the arg-max of the enumerated posterior (0 for an observed query); no case is a near-tie
    top = np.sort(exact[:, :2], axis=1)
    assert ((top[:, 1] - top[:, 0] > 1e-9) | (ev[:, 0] >= 0)).all()
    labels = np.where(ev[:, 0] >= 0, 0, np.argmax(exact[:, :2], axis=1)).astype(np.int32)
    for a in (ev, exact, labels):
        a.setflags(write=False)
    return dims, parents, counts, ev, exact, labels


@functools.lru_cache(maxsize=None)
def small_forest():
    dims, parents, counts = small()[:3]
    return F.JunctionForest(F.Network.from_counts(dims, parents, counts), device=0)


def sub_tree(net, nodes):
    """JunctionTree on the component `nodes` of `net` alone, in the interpreter (bit-identical to the
    reference's order; no kernel is compiled for it)."""
    jt = F.JunctionTree(F.Network.from_counts(*N.sub_network_args(net.node_counts, net.dims, nodes)), device=0)
    jt.set_variant(0)
    jt.set_exact(True)
    return jt


def offsets(dims):
    return np.concatenate([[0], np.cumsum(dims)])


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
def test_every_variant_against_brute_force(variant):
    _, _, _, ev, exact, labels = small()
    jf = small_forest()
    assert len(ev) == NCASES and jf.components == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10]]
    jf.set_variant(variant)  # the plan accepts every variant (test_jt_forest_host.py)
    try:
        for order in (None, True):
            for layout in (0, 1):
                jf.set_exact(order)
                jf.set_output_layout(layout)
                lab, marg = run_device(jf, ev)
                assert jf.refresh_info()["variant"] == variant
                np.testing.assert_array_equal(lab, labels)
                _close(marg, exact)
                assert (marg[ev[:, 10] >= 0][:, -3:] == 0).all()
        # the exact fixup of the kernels that flag blocks, forced on every block
        if variant >= 3:
            jf.set_exact(None)
            jf.set_output_layout(0)
            jf.debug_force_fixup(True)
            lab, marg = run_device(jf, ev)
            np.testing.assert_array_equal(lab, labels)
            _close(marg, exact)
    finally:
        jf.debug_force_fixup(False)
        jf.set_exact(None)
        jf.set_output_layout(0)
        jf.set_variant(-1)


def test_disconnected_network_with_real_cliques(tmp_path):
    path = str(tmp_path / "forest120.xml")
    synth.random_network(path=path, **N.RANDOM)
    net = F.Network(path)
    jf = F.JunctionForest(net, device=0)
    comps = jf.components
    assert len(comps) == 89 and sum(len(c) > 1 for c in comps) == 17 and len(comps[0]) == 4
    info = jf.info
    # a clique of 125 entries: more than one 64-lane row of a table
    assert max(int(np.prod(net.dims[vs])) for vs, _, _ in read_plan(jf, tmp_path, "forest120")[0]) == 125
    assert info["specialized_eligible"] == 1 and info["streamed_eligible"] == 1 and info["tiled_eligible"] == 1
    ev = net.evidence_cases(NCASES, 24, seed=5)
    ev[1] = -1  # nothing observed
    ev[2, comps[0][1:]] = 0  # all of the query's component but the query
    off = offsets(net.dims)
    ref = np.zeros((NCASES, info["sum_dom"]))
    ref_lab = None
    for nodes in comps:
        jt = sub_tree(net, nodes)
        assert len(nodes) == 1 or jt.info["tiled_eligible"] == 1
        lab, marg = jt.infer(ev[:, nodes])
        so = offsets(net.dims[nodes])
        for i, v in enumerate(nodes):
            ref[:, off[v]:off[v + 1]] = marg[:, so[i]:so[i + 1]]
        if nodes[0] == 0:
            ref_lab = lab
    assert np.isfinite(ref).all()
    for variant in (3, 4, 5):
        jf.set_variant(variant)
        lab, marg = jf.infer(ev)
        assert jf.refresh_info()["variant"] == variant
        np.testing.assert_array_equal(lab, ref_lab)
        _close(marg, ref)


def test_end_to_end_learned_alarm():
    """CSV -> PCStable -> pdag_to_dag -> ParameterLearning -> JunctionForest on all 37 nodes: the
    pipeline that used to stop at its last step (PC-stable leaves node 12 without an edge).  The
    learned structure has no prebuilt kernel, so the forest runs in the tiled kernel and in the
    interpreter, the 36-node tree in the interpreter."""
    ds = F.Dataset(os.path.join(ALARM, "alarm_s5000.txt"))
    pc = F.PCStable(0.05, 1000).StructLearnCompData(ds)
    dag = F.pdag_to_dag(ds.num_vars, pc.oriented)
    learned = F.ParameterLearning(pc.ci).LearnParamsKnowStructCompData(dag, names=ds.names)
    with pytest.raises(F.FastBNError):
        F.JunctionTree(learned, device=0)
    jf = F.JunctionForest(learned, device=0)
    rest = [v for v in range(37) if v != 12]
    assert jf.components == [rest, [12]]
    ev = learned.evidence_cases(NCASES, 7, seed=1)
    ev[:, 12] = -1
    tree = sub_tree(learned, rest)
    tlab, tmarg = tree.infer(ev[:, rest])
    off = offsets(learned.dims)
    cols = np.concatenate([np.arange(off[v], off[v + 1]) for v in rest])
    c12 = np.arange(off[12], off[13])
    _, cnt = learned.node_counts(12)
    prior = (cnt[:, 0] + 1.0) / (cnt.sum() + len(cnt))
    ev12 = ev.copy()
    ev12[::2, 12] = 0
    assert jf.info["tiled_eligible"] == 1
    for variant in (5, 0):
        jf.set_variant(variant)
        lab, marg = jf.infer(ev)
        np.testing.assert_array_equal(lab, tlab)
        _close(marg[:, cols], tmarg)
        _close(marg[:, c12], np.tile(prior, (NCASES, 1)))
        # observing node 12 changes no other marginal by a bit
        lab2, marg2 = jf.infer(ev12)
        np.testing.assert_array_equal(lab2, lab)
        np.testing.assert_array_equal(marg2[:, cols].view(np.int64), marg[:, cols].view(np.int64))
        assert (marg2[::2][:, c12] == 0).all()
        _close(marg2[1::2][:, c12], np.tile(prior, (NCASES // 2, 1)))


@pytest.mark.parametrize("variant", [-1, 4, 5])
def test_components_are_independent(variant):
    """Two runs that differ only in the evidence inside component 0: the marginals of components 1
    and 2 are the same bits (no block went through the exact fixup, which would change them)."""
    dims, _, _, ev, _, _ = small()
    jf = small_forest()
    a = ev.copy()
    a[:, :5] = -1
    a[:, 5:] = np.where(np.arange(NCASES)[:, None] % 3 == 0, -1, a[:, 5:])
    b = a.copy()
    b[:, 1] = np.arange(NCASES) % 3
    b[::2, 4] = 1
    cut = int(np.sum(dims[:5]))
    jf.set_variant(variant)
    try:
        out = []
        for e in (a, b):
            out.append(run_device(jf, e)[1])
            assert jf.debug_flagged_blocks() == 0
        assert jf.refresh_info()["variant"] == (3 if variant < 0 else variant)
    finally:
        jf.set_variant(-1)
    assert not np.array_equal(out[0][:, :cut], out[1][:, :cut])
    np.testing.assert_array_equal(out[0][:, cut:].view(np.int64), out[1][:, cut:].view(np.int64))


def test_underflowing_product_on_the_device():
    net = N.star_net()
    jf = F.JunctionForest(F.Network.from_counts(net.dims, net.parents, net.counts), device=0)
    ev = N.star_cases(net, NCASES)
    exact = np.stack([N.star_exact(net, e) for e in ev[:2]])[np.arange(NCASES) % 2]
    lab, marg = run_device(jf, ev)  # default variant and order
    assert jf.refresh_info()["variant"] == 3
    assert np.isfinite(marg).all()
    _close(marg, exact)
    np.testing.assert_array_equal(lab, np.argmax(exact[:, :2], axis=1))


def test_cli_on_a_disconnected_network(tmp_path):
    """`-a 2` on an XMLBIF with a disconnected moral graph: exit 0, one line naming the components,
    the accuracy JunctionForest.EvaluateAccuracy gives on the same files.  (The -f4 table is written
    here from the forest's own marginals: the project has no writer of that format)"""
    xml = str(tmp_path / "forest120.xml")
    synth.random_network(path=xml, **N.RANDOM)
    net = F.Network(xml)
    jf = F.JunctionForest(net, device=0)
    ev = net.evidence_cases(NCASES, 24, seed=6)
    lab, marg = jf.infer(ev)
    truth = np.where(np.arange(NCASES) % 5 == 0, (lab + 1) % int(net.dims[0]), lab).astype(np.int32)
    F.write_libsvm(str(tmp_path / "cases"), ev, truth)
    off = offsets(net.dims)
    with open(tmp_path / "pt", "w") as f:
        for c in range(NCASES):
            for v in range(net.num_nodes):
                f.write("\n" if ev[c, v] >= 0 else " ".join("%.17g" % x for x in marg[c, off[v]:off[v + 1]]) + " \n")
    ev2, truth2 = F.load_libsvm(str(tmp_path / "cases"), net.num_nodes)
    acc = jf.EvaluateAccuracy(ev2, truth2)
    assert acc == pytest.approx(104 / 130)
    cli = os.path.join(REPO, "fastbn_amd", "BayesianNetwork")
    out = subprocess.run([cli, "-a", "2", "-f0", "forest120.xml", "-f3", "cases", "-f4", "pt", "--prefix", str(tmp_path) + "/"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "junction forest of 89 components" in out.stdout, out.stdout
    got = float(re.search(r"accuracy = (\S+)", out.stdout).group(1))
    assert got == pytest.approx(acc, abs=1e-6)
