"""Junction forests on the host: fbn_jt_forest_plan_create builds one tree per
component of a disconnected moral graph, each the tree of that component alone, none joined to
another.  Host-only plans (device = -1): structure, the tiled kernel's program through
tests/tile_emulator.py against enumeration of the joint, the generated specialized kernel."""
import ctypes as C
import os

import numpy as np
import pytest
from conftest import ALARM

import fastbn_amd as F
import jt_forest_nets as N
import tile_emulator
from test_lbp_host import brute_force, disconnected_network, net_tuple, polytree_cases

TOL = 1e-12
XML = os.path.join(ALARM, "alarm.xml")


def special_cases(dims):
    """Nothing observed; all of component 0 observed; the isolated node 10 observed."""
    ev = np.full((3, len(dims)), -1, np.int8)
    ev[1, :5] = [1, 2, 0, 1, 1]
    ev[2, 10] = 2
    return ev


def forest_cases(dims):
    return np.concatenate([polytree_cases(dims, 10, 2), special_cases(dims)])


def read_plan(jt, tmp_path, tag):
    """fbn_jt_plan_dump parsed: cliques [(vars, up, down)], separators [(vars, up, down)], potentials."""
    plan, init = str(tmp_path / (tag + ".plan")), str(tmp_path / (tag + ".init"))
    jt.dump_plan(plan, init)
    cliques, seps = [], []
    for line in open(plan):
        t = line.split()
        if t[0] in ("c", "s") and len(t) > 2:
            nv = int(t[2])
            vs = [int(x) for x in t[4:4 + nv]]
            rest = t[4 + nv:]  # | up U | down D...
            up, down = int(rest[2]), [int(x) for x in rest[5:]]
            (cliques if t[0] == "c" else seps).append((vs, up, down))
    pots = [np.array(line.split()[3:], np.float64) for line in open(init)]
    return cliques, seps, pots


def test_refusal_and_creation():
    dims, parents, counts = disconnected_network()
    for a, b in zip(N.disconnected(), (dims, parents, counts)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    net = F.Network.from_counts(dims, parents, counts)
    with pytest.raises(F.FastBNError, match="moral graph is disconnected"):
        F.JunctionTree(net, device=-1)
    jf = F.JunctionForest(net, device=-1)
    assert isinstance(jf, F.JunctionTree)
    assert jf.components == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10]]
    # no separator joins two components: 7 cliques in 3 trees
    assert jf.info["num_cliques"] - jf.info["num_separators"] == 3


def test_tile_program_against_brute_force():
    dims, parents, counts = disconnected_network()
    jf = F.JunctionForest(F.Network.from_counts(dims, parents, counts), device=-1)
    assert jf.info["tiled_eligible"] == 1
    ev = forest_cases(dims)
    exact = np.stack([brute_force(net_tuple(dims, parents, counts), e) for e in ev])
    lab, marg = tile_emulator.run(jf.tile_program(), ev, int(dims.sum()))
    np.testing.assert_allclose(marg, exact, rtol=TOL, atol=1e-300)
    np.testing.assert_array_equal(lab[ev[:, 0] < 0], np.argmax(exact[:, :2], axis=1)[ev[:, 0] < 0])
    # the isolated node: its smoothed prior where unobserved, zeros where observed
    cnt = np.asarray(counts[10])[:, 0]
    np.testing.assert_allclose(marg[0, -3:], (cnt + 1.0) / (cnt.sum() + 3), rtol=TOL)
    assert (marg[-1, -3:] == 0).all()


def test_connected_network_unchanged(tmp_path):
    net = F.Network(XML)
    tree, forest = F.JunctionTree(net, device=-1), F.JunctionForest(net, device=-1)
    assert forest.components == [list(range(37))]
    paths = {}
    for tag, jt in (("tree", tree), ("forest", forest)):
        paths[tag] = (str(tmp_path / (tag + ".plan")), str(tmp_path / (tag + ".init")))
        jt.dump_plan(*paths[tag])
    for a, b in zip(paths["tree"], paths["forest"]):
        assert open(a, "rb").read() == open(b, "rb").read()
    # and so are the specialized kernel and its cache key
    assert tree.kernel_source() == forest.kernel_source()
    assert tree.kernel_cache_path() == forest.kernel_cache_path()


def test_components_equal_standalone_plans(tmp_path):
    dims, parents, counts = disconnected_network()
    net = F.Network.from_counts(dims, parents, counts)
    jf = F.JunctionForest(net, device=-1)
    fc, fs, fp = read_plan(jf, tmp_path, "forest")
    seen = 0
    for k, nodes in enumerate(jf.components):
        if len(nodes) < 2:
            continue
        sub = F.Network.from_counts(*N.sub_network_args(net.node_counts, dims, nodes))
        sc, ss, sp = read_plan(F.JunctionTree(sub, device=-1), tmp_path, "sub%d" % k)
        # the forest's cliques / separators of this component, in plan order, with their plan indices
        ci = [i for i, (vs, _, _) in enumerate(fc) if vs[0] in nodes]
        si = [i for i, (vs, _, _) in enumerate(fs) if vs[0] in nodes]
        assert len(ci) == len(sc) and len(si) == len(ss)
        cmap, smap = {-1: -1, **{j: i for j, i in enumerate(ci)}}, {-1: -1, **{j: i for j, i in enumerate(si)}}
        for j, (vs, up, down) in enumerate(sc):
            assert ([nodes[v] for v in vs], smap[up], [smap[d] for d in down]) == fc[ci[j]]
            np.testing.assert_array_equal(sp[j], fp[ci[j]])
        for j, (vs, up, down) in enumerate(ss):
            assert ([nodes[v] for v in vs], cmap[up], [cmap[d] for d in down]) == fs[si[j]]
        seen += 1
    assert seen == 2
    # the isolated node: a clique of its own, no separator
    assert [c for c in fc if c[0] == [10]] == [([10], -1, [])]


def test_many_components_underflowing_product():
    net = N.star_net()
    jf = F.JunctionForest(F.Network.from_counts(net.dims, net.parents, net.counts), device=-1)
    assert len(jf.components) == 60 and jf.components[7] == [21, 22, 23]
    assert jf.info["tiled_eligible"] == 1 and jf.info["streamed_eligible"] == 1 and jf.info["specialized_eligible"] == 1
    ev = N.star_cases(net)
    _, marg = tile_emulator.run(jf.tile_program(), ev, 2 * len(net.dims))
    assert np.isfinite(marg).all()
    exact = np.stack([N.star_exact(net, e) for e in ev])
    np.testing.assert_allclose(marg, exact, rtol=TOL, atol=1e-300)
    # the closed form against enumeration, on one component
    one = N.star_net(1)
    tup = net_tuple(one.dims, one.parents, one.counts)
    for row in (np.array([-1, 1, 1], np.int8), np.array([-1, 0, 1], np.int8), np.array([1, -1, 1], np.int8)):
        np.testing.assert_allclose(N.star_exact(one, row), brute_force(tup, row), rtol=1e-14)
    # the evidence likelihood of one component, and what the product over 60 would be
    px = (np.array(N.STAR_X)[:, 0] + 1.0) / 102.0
    py1 = (np.array(N.STAR_Y)[1] + 1.0) / (np.array(N.STAR_Y).sum(axis=0) + 2.0)
    pz1 = (np.array(N.STAR_Z)[1] + 1.0) / (np.array(N.STAR_Z).sum(axis=0) + 2.0)
    pe = float((px * py1 * pz1).sum())
    assert 9.2e-7 < pe < 9.22e-7 and 60 * np.log10(pe) < -323.4


def test_kernel_build_and_variant_honesty():
    dims, parents, counts = disconnected_network()
    jf = F.JunctionForest(F.Network.from_counts(dims, parents, counts), device=-1)
    assert jf.info["specialized_eligible"] == 1
    for exact in (None, True):
        jf.set_exact(exact)
        path = jf.build_kernel()
        assert os.path.getsize(path) > 0
        src = jf.kernel_source()
        # every clique is distributed; only cliques that send a message, and the root whose table
        # stays in registers, are collected
        assert src.count("// ---- distribute clique") == 7 and src.count("// ---- collect clique") == 5
    rows = jf.refresh_info()
    # four separators of 2 + 2 + 2 + 3 entries, two messages each, each placed exactly once or kept in
    # the registers of the op that forms it
    placed = sum(rows["place_rows_" + k] for k in ("global_collect", "global_distribute", "lds_collect",
                                                   "lds_distribute", "reg_collect", "reg_distribute"))
    assert 0 < placed <= 2 * 9
    # every variant takes a forest within its own limits: set_variant succeeds exactly
    # where the plan reports the variant eligible
    eligible = {0: 1, 1: 1, 2: 1, 3: rows["specialized_eligible"], 4: rows["streamed_eligible"], 5: rows["tiled_eligible"]}
    assert all(eligible.values())
    for v in range(6):
        jf.set_variant(v)
    # a forest with a component past the specialized kernel's limit (a 127-state variable) and more
    # than the streamed / tiled kernels' six children is refused by them, not run unguarded
    dims2 = [127, 2] + [2] * 10
    parents2 = [[], [0]] + [[]] + [[2]] * 9
    counts2 = [np.ones((127, 1), np.int64), np.ones((2, 127), np.int64), np.ones((2, 1), np.int64)] + [np.ones((2, 2), np.int64)] * 9
    big = F.JunctionForest(F.Network.from_counts(dims2, parents2, counts2), device=-1)
    assert big.components == [[0, 1], list(range(2, 12))]
    assert big.info["specialized_eligible"] == 0 and big.info["streamed_eligible"] == 0 and big.info["tiled_eligible"] == 0
    for v in (3, 4, 5):
        with pytest.raises(F.FastBNError, match="not eligible"):
            big.set_variant(v)
    for v in (0, 1, 2):
        big.set_variant(v)


def test_plan_components_errors():
    n = C.c_int32(-5)
    with pytest.raises(F.FastBNError):
        F.lib.fbn_jt_plan_components(None, None, C.byref(n))
    dims, parents, counts = disconnected_network()
    net = F.Network.from_counts(dims, parents, counts)
    jf = F.JunctionForest(net, device=-1)
    with pytest.raises(F.FastBNError):
        F.lib.fbn_jt_plan_components(jf._h, None, None)
    F.lib.fbn_jt_plan_components(jf._h, None, C.byref(n))  # NULL buffer: the count alone
    assert n.value == 3
    comp = np.full(11, -1, np.int32)
    F.lib.fbn_jt_plan_components(jf._h, comp.ctypes.data_as(C.c_void_p), C.byref(n))
    assert comp.tolist() == [0] * 5 + [1] * 5 + [2]
    # a plan from fbn_jt_plan_create reports one component
    tree = F.JunctionTree(F.Network(XML), device=-1)
    F.lib.fbn_jt_plan_components(tree._h, None, C.byref(n))
    assert n.value == 1
