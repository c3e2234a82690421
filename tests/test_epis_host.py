"""EPIS-BN's host twin (EPISBN with device=-1: epis_host.cpp over lbp_host.cpp and sample_host.cpp).

Yardsticks: LikelihoodWeighting's tested samples (no pre-propagation, no cutoff: the same values, bit
for bit), brute-force enumeration of the joint for log P(e) and the marginals, the zero-variance
property where LBP is exact, the estimator's own standard error for unbiasedness, and the exact
ALARM fixture alarm_1k_pt against likelihood weighting at equal S.  The networks and checks are
shared with test_gpu_epis.py."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
from conftest import ALARM, read_pt_file
from test_lbp_host import POLYTREE_SEED, disconnected_network, net_tuple, polytree_cases, random_polytree

import fastbn_amd as F
from fastbn_amd import synth

ARG, LIMIT = -1, -6  # fbn_err_t (include/fastbn.h)
XML = os.path.join(ALARM, "alarm.xml")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def alarm():
    return F.Network(XML), synth.read_xmlbif(XML)


@functools.lru_cache(maxsize=None)
def alarm_cases():
    ev, truth = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)
    ev.setflags(write=False)
    return ev, truth


def brute(tup, ev):
    """(posterior marginals [sum_dom], zeros for observed; log P(e)) of one case by enumerating the joint."""
    _, dims, parents, cpts = tup
    V = len(dims)
    joint = np.ones([int(d) for d in dims])
    for v in range(V):
        sc = [v] + list(parents[v])
        a = np.asarray(cpts[v], np.float64).reshape([dims[x] for x in sc])
        shape = [1] * V
        for x in sc:
            shape[x] = int(dims[x])
        joint = joint * a.transpose(np.argsort(sc)).reshape(shape)
        if ev[v] >= 0:
            keep = np.zeros(int(dims[v]))
            keep[ev[v]] = 1.0
            shape = [1] * V
            shape[v] = int(dims[v])
            joint = joint * keep.reshape(shape)
    pe = joint.sum()
    out = []
    for v in range(V):
        mv = joint.sum(axis=tuple(x for x in range(V) if x != v)) / pe
        out += [0.0] * int(dims[v]) if ev[v] >= 0 else mv.tolist()
    return np.array(out), math.log(pe)


# ---- H2's forest: every node has at most one parent, so LBP is exact and the weights are constant
FOREST_SEED = 5  # structure alone: three components, depth 4, a 1-state node, 4-state nodes (asserted below)


@functools.lru_cache(maxsize=None)
def forest():
    rng = np.random.default_rng(FOREST_SEED)
    n = 14
    dims = rng.integers(2, 5, n).astype(np.int32)
    dims[11] = 1
    parents = [[]] + [[int(rng.integers(max(0, i - 2), i))] for i in range(1, n)]
    parents[6] = []   # second component
    parents[13] = []  # an isolated node
    counts = [rng.integers(0, 40, (int(dims[v]), int(np.prod(dims[ps], dtype=np.int64)))) for v, ps in enumerate(parents)]
    depth = [0] * n
    for i in range(n):
        depth[i] = 1 + depth[parents[i][0]] if parents[i] else 0
    return dims, parents, counts, depth


@functools.lru_cache(maxsize=None)
def forest_cases():
    """16 cases observing c % 5 variables; from case 8 on the deepest node is among them.  A case that
    observes a non-root variable always observes one whose parent is unobserved and has >= 2 states
    (asserted), which is what makes likelihood weighting's weights differ between samples."""
    dims, parents, _, depth = forest()
    rng = np.random.default_rng(2)
    deepest = int(np.argmax(depth))
    ev = np.full((16, len(dims)), -1, np.int8)
    for c in range(16):
        k = c % 5
        pick = list(rng.choice(np.flatnonzero(dims > 1), k, replace=False))  # observing the 1-state node says nothing
        if c >= 8 and k and deepest not in pick:
            pick[0] = deepest
        for v in pick:
            ev[c, v] = rng.integers(0, dims[v])
    ev.setflags(write=False)
    return ev


def lw_varies(dims, parents, e):
    """Some observed non-root variable of case e has an unobserved parent with >= 2 states."""
    return any(e[v] >= 0 and parents[v] and e[parents[v][0]] < 0 and dims[parents[v][0]] >= 2 for v in range(len(dims)))


def check_zero_variance(device, S=4096):
    dims, parents, counts, depth = forest()
    assert max(depth) >= 4 and sum(1 for p in parents if not p) >= 3 and dims.min() == 1 and dims.max() == 4
    assert max(len(p) for p in parents) == 1
    ev = forest_cases()
    assert sorted(set((ev >= 0).sum(1))) == [0, 1, 2, 3, 4]
    net = F.Network.from_counts(dims, parents, counts)
    tup = net_tuple(dims, parents, counts)
    ep = F.EPISBN(net, S, iterations=max(depth) + 4, eps=0.0, seed=1, device=device)
    lab, marg = ep.infer(ev)
    le, ess, used, res = ep.stats
    lw = F.LikelihoodWeighting(net, S, seed=1, device=device)
    lw.infer(ev)
    nonroot = 0
    for c, e in enumerate(ev):
        exact, lpe = brute(tup, e)
        print("case", c, "ess/S", ess[c] / S, "log_evidence - log P(e)", le[c] - lpe, "max marginal error",
              np.abs(marg[c] - exact).max(), "LW ess/S", lw.stats[1][c] / S)
        assert ess[c] >= S * (1 - 1e-9)
        assert abs(le[c] - lpe) <= 1e-10
        assert np.abs(marg[c] - exact).max() <= 3 / math.sqrt(S)  # 6 sigma of an equal-weight estimate (sigma <= 1 / (2 sqrt S))
        assert res[c] == 0.0 and used[c] <= max(depth) + 4
        if any(e[v] >= 0 and parents[v] for v in range(len(dims))):
            nonroot += 1
            assert lw_varies(dims, parents, e)
            assert lw.stats[1][c] < ess[c]
    assert nonroot >= 8
    return ep, lab, marg


def test_zero_variance_where_lbp_is_exact():
    check_zero_variance(-1)


# ---- H1
@pytest.mark.parametrize("seed", [3, 8])
def test_reduces_to_likelihood_weighting(seed):
    """iterations=0, eps=0: g = P * 1.0 = P and c is the cdf row, so the values are LW's; the weight
    takes cdf[d - 1] (within an ulp of 1) per sampled variable, 37 at most: 1e-13 relative."""
    net, _ = alarm()
    ev = alarm_cases()[0][:16]
    ep = F.EPISBN(net, 130, iterations=0, eps=0.0, seed=seed, device=-1)
    lw = F.LikelihoodWeighting(net, 130, seed=seed, device=-1)
    val, m, e, lam = ep.debug_samples(ev, case_offset=5)
    lval, lm, le = lw.debug_samples(ev, case_offset=5)
    np.testing.assert_array_equal(val, lval)
    assert (lam == 1.0).all()
    w, lww = np.ldexp(m, e), np.ldexp(lm, le)
    assert (lww > 0).all() and (np.abs(w - lww) <= 1e-13 * lww).all()
    assert not np.array_equal(val, ep.debug_samples(ev, case_offset=6)[0])  # the offset moves the stream
    ep.infer(ev, case_offset=5)
    assert (ep.stats[2] == 0).all() and (ep.stats[3] == 0.0).all()


# ---- H3
# An 8-node network with loops (0 -> 1, 0 -> 2, {1, 2} -> 3, {2, 0} -> 4, {3, 4} -> 5, 5 -> 6, {6, 1} -> 7).
LOOPY_DIMS = np.array([2, 3, 2, 3, 2, 2, 3, 2], np.int32)
LOOPY_PARENTS = [[], [0], [0], [1, 2], [2, 0], [3, 4], [5], [6, 1]]
# Chosen here with the host twin (deterministic, and equal to the device): at these the estimate of
# every case lies inside its own 5 sigma, as it should for almost every seed.
UNBIASED_SEED, UNBIASED_S = 4, 2048


@functools.lru_cache(maxsize=None)
def loopy_network():
    rng = np.random.default_rng(33)
    counts = [rng.integers(0, 40, (int(LOOPY_DIMS[v]), int(np.prod(LOOPY_DIMS[ps], dtype=np.int64))))
              for v, ps in enumerate(LOOPY_PARENTS)]
    return LOOPY_DIMS, LOOPY_PARENTS, counts


@functools.lru_cache(maxsize=None)
def polytree_network():
    return random_polytree(12, POLYTREE_SEED)


@pytest.mark.parametrize("eps", [0.0, None])
@pytest.mark.parametrize("which", ["polytree", "loopy"])
def test_unbiased(which, eps):
    dims, parents, counts = polytree_network() if which == "polytree" else loopy_network()
    net = F.Network.from_counts(dims, parents, counts)
    tup = net_tuple(dims, parents, counts)
    ev = polytree_cases(dims, 16, 1)
    S = UNBIASED_S
    ep = F.EPISBN(net, S, iterations=10, eps=eps, seed=UNBIASED_SEED, device=-1)
    ep.infer(ev)
    le, ess = ep.stats[0], ep.stats[1]
    for c, e in enumerate(ev):
        lpe = brute(tup, e)[1]
        err, bound = abs(math.exp(le[c] - lpe) - 1.0), 5 * math.sqrt(max(S / ess[c] - 1.0, 0.0) / S) + 1e-9
        print(which, eps, "case", c, "relative error", err, "bound", bound, "ess/S", ess[c] / S)
        assert err <= bound


# ---- H4
def test_alarm_beats_likelihood_weighting():
    """First 64 fixture cases (7 observed variables), S = 1024, seed 0, 20 iterations, default cutoff,
    measured with the host twin:
        average Hellinger distance   EPIS-BN 0.017692   LW 0.072420   (gap 0.054728)
        median ess / S               EPIS-BN 0.67324    LW 0.041448   (gap 0.63179)
    The margins are those gaps halved."""
    net, tup = alarm()
    ev, truth = alarm_cases()
    gold = read_pt_file(os.path.join(ALARM, "alarm_1k_pt"), tup[1], len(ev))[:64]
    S = 1024
    ep = F.EPISBN(net, S, iterations=20, seed=0, device=-1)
    lw = F.LikelihoodWeighting(net, S, seed=0, device=-1)
    hd = F.score_marginals(net, ep.infer(ev[:64])[1], gold)[1] / 64
    lhd = F.score_marginals(net, lw.infer(ev[:64])[1], gold)[1] / 64
    med, lmed = np.median(ep.stats[1]) / S, np.median(lw.stats[1]) / S
    print("average HD: EPIS-BN", hd, "LW", lhd, "; median ess/S: EPIS-BN", med, "LW", lmed)
    assert hd <= lhd - 0.027364
    assert med >= lmed + 0.31589


# ---- H5
def test_lbp_failure_falls_back_to_lambda_one():
    """A binary root with 1100 unobserved binary children: the product of their 1100 messages (1/2
    each) is 2^-1100 = 0 in fp64, so LBP fails the case; the draws are then likelihood weighting's."""
    n = 1101
    dims = [2] * n
    parents = [[]] + [[0]] * (n - 1)
    counts = [[[2], [0]]] + [[[3, 1], [0, 1]]] * (n - 1)
    net = F.Network.from_counts(dims, parents, counts)
    ev = np.full((2, n), -1, np.int8)
    ev[1, 5] = 1
    ep = F.EPISBN(net, 70, iterations=3, seed=2, device=-1)
    lab, marg = ep.infer(ev)
    le, ess, used, res = ep.stats
    assert np.isinf(res).all() and (res > 0).all() and (used >= 1).all()
    assert np.isfinite(marg).all() and np.isfinite(le).all() and np.isfinite(ess).all() and (lab >= 0).all()
    val, m, e, lam = ep.debug_samples(ev)
    assert (lam == 1.0).all()
    lval = F.LikelihoodWeighting(net, 70, seed=2, device=-1).debug_samples(ev)[0]
    np.testing.assert_array_equal(val, lval)


def test_all_and_nothing_observed_and_a_one_state_node():
    dims, parents, counts, _ = forest()
    net = F.Network.from_counts(dims, parents, counts)
    tup = net_tuple(dims, parents, counts)
    ev = np.full((3, len(dims)), -1, np.int8)
    ev[1] = [d - 1 for d in dims]
    ev[2, 11] = 0  # the 1-state node observed
    S = 256
    ep = F.EPISBN(net, S, iterations=8, eps=0.0, seed=3, device=-1)
    lab, marg = ep.infer(ev)
    le, ess = ep.stats[0], ep.stats[1]
    assert np.isfinite(marg).all() and (marg[1] == 0).all() and lab[1] == 0
    off = int(np.sum(dims[:11]))
    assert abs(marg[0, off] - 1.0) <= 1e-12 and marg[2, off] == 0.0
    for c in range(3):
        assert abs(le[c] - brute(tup, ev[c])[1]) <= 1e-10  # a forest, no cutoff: every weight is P(e)
    assert abs(le[0]) <= 1e-10 and ess[1] == S


def test_batch_split_and_repeat():
    net, _ = alarm()
    ev = alarm_cases()[0][:37]
    ep = F.EPISBN(net, 100, iterations=6, seed=9, device=-1)
    lab, marg = ep.infer(ev)
    st = np.stack([np.asarray(s, np.float64) for s in ep.stats])
    la, ma = ep.infer(ev[:20])
    sa = np.stack([np.asarray(s, np.float64) for s in ep.stats])
    lb, mb = ep.infer(ev[20:], case_offset=20)
    sb = np.stack([np.asarray(s, np.float64) for s in ep.stats])
    np.testing.assert_array_equal(lab, np.concatenate([la, lb]))
    np.testing.assert_array_equal(bits(marg), bits(np.concatenate([ma, mb])))
    np.testing.assert_array_equal(bits(st), bits(np.concatenate([sa, sb], axis=1)))
    np.testing.assert_array_equal(bits(ep.infer(ev)[1]), bits(marg))
    assert not np.array_equal(ep.infer(ev[20:])[1], mb)  # the offset moves the stream
    assert ep.infer(ev[:3], marginals=False)[1] is None


def test_arguments(tmp_path):
    net, _ = alarm()
    ev = alarm_cases()[0][:4].copy()
    ref = F.EPISBN(net, 64, device=-1).infer(ev)
    for kw in (dict(num_samples=0), dict(iterations=-1), dict(tol=-1e-3), dict(tol=math.nan), dict(damping=1.0),
               dict(damping=-0.1), dict(damping=math.nan), dict(eps=1.0), dict(eps=math.nan)):
        with pytest.raises(F.FastBNError) as e:
            F.EPISBN(net, **{"num_samples": 64, "device": -1, **kw}).infer(ev)
        assert e.value.code == ARG, kw
    with pytest.raises(F.FastBNError) as e:
        F.EPISBN(net, 64, eps=-0.5, device=-1)
    assert e.value.code == ARG
    ep = F.EPISBN(net, 64, device=-1)
    with pytest.raises(F.FastBNError) as e:
        ep.infer(ev, case_offset=-1)
    assert e.value.code == ARG
    bad = ev.copy()
    bad[2, 5] = net.dims[5]  # one past the last state
    with pytest.raises(F.FastBNError, match="case 2.*node 5") as e:
        ep.infer(bad)
    assert e.value.code == ARG
    bad[2, 5] = -2
    with pytest.raises(F.FastBNError) as e:
        ep.debug_samples(bad)
    assert e.value.code == ARG
    with pytest.raises(F.FastBNError) as e:  # the debug cap, 2^22 samples
        F.EPISBN(net, (1 << 22) // 4 + 1, device=-1).debug_samples(ev)
    assert e.value.code == LIMIT
    with pytest.raises(F.FastBNError) as e:  # stream positions beyond 2^63
        ep.infer(ev, case_offset=1 << 61)
    assert e.value.code == ARG
    with pytest.raises(F.FastBNError, match="host-only") as e:
        ep.run_device(1, 4, 1)
    np.testing.assert_array_equal(bits(ep.infer(ev)[1]), bits(ref[1]))  # the handle stays usable
    # fbn_network_create refuses a cycle itself; the XMLBIF loader does not
    var = "<VARIABLE><NAME>%s</NAME><TYPE>discrete</TYPE><VALUE>0</VALUE><VALUE>1</VALUE></VARIABLE>\n"
    prob = "<PROBABILITY><FOR>%s</FOR><GIVEN>%s</GIVEN><TABLE>0.5 0.5 0.5 0.5 </TABLE></PROBABILITY>\n"
    xml = tmp_path / "cyclic.xml"
    xml.write_text('<?xml version="1.0"?>\n<BIF><NETWORK><NAME>c</NAME>\n' + var % "A" + var % "B" + prob % ("A", "B")
                   + prob % ("B", "A") + "</NETWORK></BIF>\n")
    with pytest.raises(F.FastBNError, match="cycle") as e:
        F.EPISBN(F.Network(str(xml)), device=-1)
    assert e.value.code == ARG
    # 2049 parentless binary nodes: one past the sampler's variable limit
    with pytest.raises(F.FastBNError) as e:
        F.EPISBN(F.Network.from_counts([2] * 2049, [[]] * 2049, [[[1], [1]]] * 2049), device=-1)
    assert e.value.code == LIMIT
    # 25 binary roots and one binary child of all of them: 2^26 cells, the cap, plus the roots' 50.
    # The count array is never written (zero pages), only read by fbn_network_create.
    V = 26
    dims = np.full(V, 2, np.int32)
    off = np.zeros(V + 1, np.int32)
    off[V] = 25
    par = np.arange(25, dtype=np.int32)
    cnt = np.zeros(50 + (1 << 26), np.int64)
    h = C.c_void_p()
    F.lib.fbn_network_create(V, dims.ctypes.data, off.ctypes.data, par.ctypes.data, cnt.ctypes.data, None, C.byref(h))
    big = F.Network(_handle=h)
    del cnt
    with pytest.raises(F.FastBNError) as e:
        F.EPISBN(big, device=-1)
    assert e.value.code == LIMIT
    big.close()


# ---- H6
def check_disconnected(device, S=4096):
    """Two polytrees with a two-parent node each and an isolated node.  Cases 0-5 observe only
    variables that, like all their ancestors, have at most one parent (0, 1, 5, 6, 7, 10): seen from the
    evidence the network is a forest of such nodes, LBP is exact and the weights are constant.  Cases
    6-15 observe anything: the estimate stays inside its own 5 sigma."""
    dims, parents, counts = disconnected_network()
    net = F.Network.from_counts(dims, parents, counts)
    with pytest.raises(F.FastBNError):
        F.JunctionTree(net, device=-1)
    tup = net_tuple(dims, parents, counts)
    ev = np.full((16, len(dims)), -1, np.int8)
    for c, obs in enumerate([{6: 1}, {6: 0, 10: 2}, {0: 1, 6: 1, 7: 0}, {1: 2, 5: 1, 10: 0}, {10: 1}, {6: 1, 1: 0, 0: 0, 7: 1}]):
        for v, x in obs.items():
            ev[c, v] = x
    ev[6:] = polytree_cases(dims, 10, 2)
    ep = F.EPISBN(net, S, iterations=16, eps=0.0, seed=UNBIASED_SEED, device=device)
    lab, marg = ep.infer(ev)
    le, ess = ep.stats[0], ep.stats[1]
    assert np.isfinite(marg).all()
    for c, e in enumerate(ev):
        exact, lpe = brute(tup, e)
        if c < 6:
            assert ess[c] >= S * (1 - 1e-9) and abs(le[c] - lpe) <= 1e-10
            assert np.abs(marg[c] - exact).max() <= 3 / math.sqrt(S)
        else:
            assert abs(math.exp(le[c] - lpe) - 1.0) <= 5 * math.sqrt(max(S / ess[c] - 1.0, 0.0) / S) + 1e-9
    return lab, marg


def test_disconnected_network():
    check_disconnected(-1)
