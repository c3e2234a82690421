"""Every inference engine on probability networks (Network.from_cpts: what ExpectationMaximization.network()
hands on), on the device.

The junction-tree kernels are held to the restatement built from the same tables (OracleJT.from_cpts, which
tests/test_probnet_host.py holds to exact rationals): exact order bit for bit, fast order labels equal and
marginals within test_gpu_jt_fast.TOL.  MPE, EM, LBP and the samplers are held to their host twins byte for
byte (the twins to the rationals and restatements in test_probnet_host.py), MPE and EM to the rationals
directly as well.  Networks: tests/prob_nets.py.  70 cases: one full block and a ragged one."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import em_nets as E
import fastbn_amd as F
import mpe_nets as M
import oracle as O
import prob_nets as P
from fastbn_amd import synth
from test_gpu_jt_counts import KERNELS
from test_gpu_jt_fast import TOL
from test_gpu_sample import check_device as check_lw_device
from test_ais_host import CLASSES
from test_probnet_host import TWIN_NETS, check_em, check_mpe, check_value_underflow, twin_cases

pytestmark = pytest.mark.gpu
NCASES = 70


def forest_oracle(net, ev):
    """The restatement on every component of the graph alone (it builds a single tree): labels of node 0's
    component, marginals side by side."""
    dims, parents, cpts = net
    off = np.concatenate([[0], np.cumsum(dims)])
    marg, lab = np.zeros((len(ev), off[-1])), None
    for nodes in P.components(parents):
        l, m = O.OracleJT.from_cpts(*P.sub_network(dims, parents, cpts, nodes)).infer(np.ascontiguousarray(ev[:, nodes]))
        o = 0
        for v in nodes:
            marg[:, off[v]:off[v + 1]] = m[:, o:o + dims[v]]
            o += dims[v]
        if 0 in nodes:
            lab = l
    return lab, marg


# name -> (network, the class that plans it, whether the plan is eligible for the specialized kernel (variant
# 3)).  That kernel depends on the plan's structure alone, so four are requested in this file and prebuilt by
# fastbn_amd/prebuild.py: the 7-node network (either concentration), its forest, ALARM's structure, votes.
JT_NETS = {"small-benign": (lambda: P.small("benign"), F.JunctionTree, True),
           "small-skewed": (lambda: P.small("skewed"), F.JunctionTree, True),
           "small-forest": (lambda: P.small_forest("skewed"), F.JunctionForest, True),
           "shapes": (P.shapes, F.JunctionForest, False),
           "learned": (P.learned, F.JunctionTree, True)}


@functools.lru_cache(maxsize=None)
def _setup(key):
    make, cls, special = JT_NETS[key]
    net = make()
    ev = P.cases(net[0], NCASES, 11, p_observed=0.2 if key == "learned" else 0.4)
    if key == "shapes":
        ev[2, 13], ev[3, 12] = 100, 0  # a state past 64 of the 127-state node; the 1-state node observed
    s = SimpleNamespace(net=net, ev=ev, special=special, jt=cls(F.Network.from_cpts(*net), device=0))
    assert s.jt.info["specialized_eligible"] == int(special)
    assert s.jt.info["streamed_eligible"] == 1 and s.jt.info["tiled_eligible"] == 1
    s.lab, s.marg = forest_oracle(net, ev)
    if cls is F.JunctionTree:  # one component: the restatement takes the network as it is
        lab, marg = O.OracleJT.from_cpts(*net).infer(ev)
        assert lab.tobytes() == s.lab.tobytes() and marg.tobytes() == s.marg.tobytes()
    return s


def _reset(jt):
    jt.set_variant(-1)
    jt.set_exact(None)


def _check(s, lab, marg, exact):
    np.testing.assert_array_equal(lab, s.lab)
    if exact:
        np.testing.assert_array_equal(marg, s.marg)
    else:
        np.testing.assert_allclose(marg, s.marg, rtol=TOL, atol=1e-300)


JT_RUNS = [(k, v, e) for k in sorted(JT_NETS) for v, e in KERNELS]


@pytest.mark.parametrize("key,variant,exact", JT_RUNS)
def test_jt_every_kernel_vs_restatement(key, variant, exact):
    s = _setup(key)
    jt = s.jt
    if variant == 3 and not s.special:
        assert jt.info["specialized_eligible"] == 0
        with pytest.raises(F.FastBNError, match="not eligible for the specialized kernel"):
            jt.set_variant(3)
        return
    try:
        jt.set_variant(variant)
        jt.set_exact(exact)
        lab, marg = jt.infer(s.ev)
        assert jt.refresh_info()["variant"] == variant
        if variant >= 3:
            assert jt.debug_flagged_blocks() == 0  # the kernel's own values
    finally:
        _reset(jt)
    _check(s, lab, marg, exact)


@pytest.mark.parametrize("exact", [None, True])
@pytest.mark.parametrize("key", sorted(JT_NETS))
def test_jt_auto_mode_picks_a_working_kernel(key, exact):
    s = _setup(key)
    jt = s.jt
    try:
        jt.set_variant(-1)
        jt.set_exact(exact)
        lab, marg = jt.infer(s.ev)
        picked = jt.refresh_info()["variant"]
        assert picked == (3 if s.special else (4 if exact else 5))
        assert jt.debug_flagged_blocks() == 0
    finally:
        _reset(jt)
    _check(s, lab, marg, exact)


# ---- the range guards of DESIGN.md section 4, tripped by single table entries
@functools.lru_cache(maxsize=None)
def _votes():
    b = P.votes_blocks()
    s = SimpleNamespace(ev=np.concatenate([b.benign, b.tripping]), deep=b.deep_cases)
    s.jt = F.JunctionTree(F.Network.from_cpts(*b.guard), device=0)
    s.deep_jt = F.JunctionTree(F.Network.from_cpts(*b.deep), device=0)
    s.lab, s.marg = O.OracleJT.from_cpts(*b.guard).infer(s.ev)
    s.deep_lab, s.deep_marg = O.OracleJT.from_cpts(*b.deep).infer(s.deep)
    return s


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_votes_exact_order_bit_identical_and_one_block_flagged(variant):
    s = _votes()
    try:
        s.jt.set_variant(variant)
        s.jt.set_exact(True)
        lab, marg = s.jt.infer(s.ev)
        assert s.jt.refresh_info()["variant"] == variant
        flagged = s.jt.debug_flagged_blocks() if variant >= 3 else 1
    finally:
        _reset(s.jt)
    np.testing.assert_array_equal(lab, s.lab)
    np.testing.assert_array_equal(marg, s.marg)
    assert flagged == 1  # the tripping block, and only it


@pytest.mark.parametrize("variant", [3, 4, 5])
def test_votes_fast_order(variant):
    s = _votes()
    try:
        s.jt.set_variant(variant)
        s.jt.set_exact(None)
        lab, marg = s.jt.infer(s.ev)
        assert s.jt.refresh_info()["variant"] == variant
        flagged = s.jt.debug_flagged_blocks()
    finally:
        _reset(s.jt)
    print("variant %d fast order: %d of 2 blocks flagged" % (variant, flagged))
    assert flagged <= 1
    np.testing.assert_array_equal(lab, s.lab)
    np.testing.assert_allclose(marg, s.marg, rtol=TOL, atol=1e-300)


def test_votes_deep_block_through_the_tiled_kernel():
    """Denominators near 2^-920: past the tiled kernel's own range [2^-900, 2^900] too."""
    s = _votes()
    try:
        s.deep_jt.set_variant(5)
        s.deep_jt.set_exact(None)
        lab, marg = s.deep_jt.infer(s.deep)
        assert s.deep_jt.refresh_info()["variant"] == 5
        print("variant 5, deep block: %d of 1 block flagged" % s.deep_jt.debug_flagged_blocks())
    finally:
        _reset(s.deep_jt)
    np.testing.assert_array_equal(lab, s.deep_lab)
    np.testing.assert_allclose(marg, s.deep_marg, rtol=TOL, atol=1e-300)


# ---- MPE and EM: device = host twin in bytes; device against the rationals
SETTINGS = [(1, 0), (64, 0), (65, 0), (130, 1)]  # (cases, max_workgroups)


@functools.lru_cache(maxsize=None)
def _twin_workload(key):
    net = TWIN_NETS[key]
    base = twin_cases(key)
    ev = np.concatenate([base, P.cases(net[0], 130 - len(base), 23)])
    ev.setflags(write=False)
    pn = F.Network.from_cpts(*net)
    mpe, em = F.MostProbableExplanation(pn, device=-1), F.ExpectationMaximization(pn, device=-1)
    return pn, ev, mpe.value_parts(ev), em.debug_posteriors(ev), em.estep_flat(ev)[1], {n: em.estep_flat(ev[:n])[0] for n, _ in SETTINGS}


@pytest.mark.parametrize("key", sorted(TWIN_NETS))
def test_mpe_device_equals_host_twin_and_the_rationals(key):
    pn, ev, (assign, value), _, _, _ = _twin_workload(key)
    dev = F.MostProbableExplanation(pn, device=0)
    for n, groups in SETTINGS:
        dev.set_tuning(max_workgroups=groups)
        a, v = dev.value_parts(ev[:n])
        assert a.tobytes() == assign[:n].tobytes() and v.tobytes() == value[:n].tobytes(), (key, n, groups)
    k = len(twin_cases(key))
    a, v = dev.value_parts(ev[:k])
    assert check_mpe(TWIN_NETS[key], ev[:k], a, v) >= k // 2
    dev.close()


@pytest.mark.parametrize("key", sorted(TWIN_NETS))
def test_em_device_equals_host_twin_and_the_rationals(key):
    pn, ev, _, post, value, counts = _twin_workload(key)
    dev = F.ExpectationMaximization(pn, device=0)
    b = E.bound(dev)
    for n, groups in SETTINGS:
        dev.set_tuning(max_workgroups=groups)
        assert dev.debug_posteriors(ev[:n]).tobytes() == post[:n].tobytes(), (key, n, groups)
        c, v = dev.estep_flat(ev[:n])
        assert v.tobytes() == value[:n].tobytes(), (key, n, groups)
        want = counts[n]
        assert ((want == 0) == (c == 0)).all() and (np.abs(c - want) <= (b + n * E.U) * want).all(), (key, n, groups)
    k = len(twin_cases(key))
    check_em(TWIN_NETS[key], ev[:k], dev.debug_posteriors(ev[:k]), dev.estep_flat(ev[:k])[1], b)
    dev.close()


@pytest.mark.parametrize("k", [341, 400])
def test_underflowing_clique_potential_is_refused_on_the_device(k):
    pn = F.Network.from_cpts(*P.underflow(k))
    for cls in (F.MostProbableExplanation, F.ExpectationMaximization, F.JunctionTree, F.JunctionForest):
        with pytest.raises(F.FastBNError, match="underflows") as e:
            cls(pn, device=0)
        assert e.value.code == -6
    em = F.ExpectationMaximization(F.Network.from_cpts(*P.underflow(300)), device=0)
    before = E.network_bits(em.network())
    with pytest.raises(F.FastBNError, match="underflows"):
        em.set_parameters(pn)
    counts, value = em.estep_flat(P.UNDERFLOW_ROWS)
    assert E.network_bits(em.network()) == before and np.isfinite(counts).all()
    np.testing.assert_array_equal(value[:3], [[0.5, -899.0], [0.5, -599.0], [0.5, -299.0]])


def test_em_fit_on_the_device_stops_at_parameters_that_underflow():
    """test_probnet_host.test_em_never_reports_nan_or_a_zero_mantissa's fit, on the device."""
    rows = np.zeros((5, 3), np.int8)
    start = F.Network.from_cpts(*P.underflow(300))
    em = F.ExpectationMaximization(start, pseudo_count=1e-310, device=0)
    with pytest.raises(F.FastBNError, match="underflows") as e:
        em.fit(rows, max_iters=3, tol=0)
    assert e.value.code == -6 and E.network_bits(em.network()) == E.network_bits(start)
    counts, value = em.estep_flat(P.UNDERFLOW_ROWS)
    assert np.isfinite(counts).all() and (value[:, 0] >= 0.5).all()
    host = F.ExpectationMaximization(start, pseudo_count=1e-300, device=-1)
    em = F.ExpectationMaximization(start, pseudo_count=1e-300, device=0)
    assert em.fit(rows, max_iters=3, tol=0).tobytes() == host.fit(rows, max_iters=3, tol=0).tobytes()
    assert E.network_bits(em.network()) == E.network_bits(host.network())


# ---- LBP and the samplers: device = host twin bit for bit, what the check_device helpers of test_gpu_lbp.py,
# test_gpu_ais.py and test_gpu_epis.py assert, here on a (network, cases) pair
PROB_WORKLOADS = ("shapes", "learned")


@functools.lru_cache(maxsize=None)
def _workload(key):
    net = P.shapes() if key == "shapes" else P.learned()
    ev = P.cases(net[0], 8, 31, p_observed=0.25)
    if key == "shapes":
        ev[2, 13], ev[3, 12] = 100, 0
    ev.setflags(write=False)
    return net, F.Network.from_cpts(*net), ev


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(dev_arrays, host_arrays):
    """floating arrays bit for bit, integer arrays equal"""
    for d, h in zip(dev_arrays, host_arrays):
        if np.asarray(h).dtype.kind == "f":
            np.testing.assert_array_equal(bits(d), bits(h))
        else:
            np.testing.assert_array_equal(d, h)


def _log_evidence_close(dle, hle):
    """the two `log` implementations differ: 1e-15 relative (as the engines' own GPU tests)"""
    fin = np.isfinite(hle)
    assert (np.isfinite(dle) == fin).all() and (dle[~fin] == hle[~fin]).all()
    assert (np.abs(dle[fin] - hle[fin]) <= 1e-15 * np.abs(hle[fin])).all()


@pytest.mark.parametrize("damping", [0.0, 0.5])
@pytest.mark.parametrize("key", PROB_WORKLOADS)
def test_lbp_device_equals_host_twin(key, damping):
    _, pn, ev = _workload(key)
    dev = F.LoopyBeliefPropagation(pn, iterations=5, damping=damping, device=0)
    host = F.LoopyBeliefPropagation(pn, iterations=5, damping=damping, device=-1)
    _same([dev.debug_messages(ev, 5)], [host.debug_messages(ev, 5)])
    _same(dev.infer(ev), host.infer(ev))
    _same(dev.stats, host.stats)  # iterations used, residual
    assert dev.last_kernel_ms() > 0.0
    dev.close()


@pytest.mark.parametrize("method", ["lw", "pls"])
@pytest.mark.parametrize("S", [64, 65])
@pytest.mark.parametrize("key", PROB_WORKLOADS)
def test_lw_pls_device_equals_host_twin_and_restatement(key, S, method):
    net, pn, ev = _workload(key)
    check_lw_device(pn, P.net_tuple(*net), ev, S, 5, method)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("S", [64, 65])
@pytest.mark.parametrize("key", PROB_WORKLOADS)
def test_ais_device_equals_host_twin(key, S, method):
    _, pn, ev = _workload(key)
    dev, host = (CLASSES[method](pn, S, max_updates=2, interval=33, seed=5, device=d) for d in (0, -1))
    _same(dev.debug_samples(ev, case_offset=3), host.debug_samples(ev, case_offset=3))  # values, m, e, the ICPT
    _same(dev.infer(ev, case_offset=3), host.infer(ev, case_offset=3))
    _same(dev.stats[1:], host.stats[1:])  # ess, updates applied, the first stage's ess
    _log_evidence_close(dev.stats[0], host.stats[0])
    assert dev.last_kernel_ms() > 0.0
    dev.close()


@pytest.mark.parametrize("S", [64, 65])
@pytest.mark.parametrize("key", PROB_WORKLOADS)
def test_epis_device_equals_host_twin(key, S):
    _, pn, ev = _workload(key)
    dev, host = (F.EPISBN(pn, S, iterations=6, eps=None, seed=5, device=d) for d in (0, -1))
    _same(dev.debug_samples(ev, case_offset=3), host.debug_samples(ev, case_offset=3))  # values, m, e, lambda rows
    _same(dev.infer(ev, case_offset=3), host.infer(ev, case_offset=3))
    _same(dev.stats[1:], host.stats[1:])  # ess, LBP iterations, residual
    _log_evidence_close(dev.stats[0], host.stats[0])
    lbp_ms, sample_ms = dev.last_kernel_ms()
    assert sample_ms > 0.0 and lbp_ms > 0.0
    dev.close()


def test_a_value_that_underflows_inside_a_clique_is_refused_on_the_device():
    check_value_underflow(0)


def test_forward_sampling_on_tables():
    net = P.shapes()
    pn = F.Network.from_cpts(*net)
    got = F.Sampler(pn).forward_sample(257, 2)
    np.testing.assert_array_equal(got, pn.forward_sample(257, 2))
    np.testing.assert_array_equal(got, synth.forward_sample(P.net_tuple(*net), 257, 2))
    assert (got[12] == 0).all() and got[13].max() > 64


# ---- fit, then infer, all on the device
def test_fit_then_infer_on_the_device():
    em = P.learned_em(F, M.XML, device=0)
    net = em.network()
    tables = P.from_network(net)
    # (the device sums the counts over its waves, the host twin in case order: theta agrees to rounding, not
    # in bytes -- test_gpu_em.py holds the device's fit to the manual chain -- so the yardsticks below take
    # the device's own tables)
    print("device fit vs host twin, largest relative difference of theta: %.3g"
          % max(float(np.max(np.abs(a - b) / b)) for a, b in zip(tables[2], P.learned()[2])))
    ev = M.alarm_cases()
    # the junction tree on the fitted tables = the restatement
    jt = F.JunctionTree(net, device=0)
    olab, omarg = O.OracleJT.from_cpts(*tables).infer(ev)
    lab, marg = jt.infer(ev)
    np.testing.assert_array_equal(lab, olab)
    np.testing.assert_allclose(marg, omarg, rtol=TOL, atol=1e-300)
    jt.set_exact(True)
    lab, marg = jt.infer(ev)
    assert lab.tobytes() == olab.tobytes() and marg.tobytes() == omarg.tobytes()
    # the forest's marginals = EM's family posteriors marginalised (test_gpu_em.py's bound)
    em2 = F.ExpectationMaximization(net, device=0)
    tb, b = E.Tables(net), E.bound(em2)
    post = em2.debug_posteriors(ev)
    _, fmarg = F.JunctionForest(net, device=0).infer(ev)
    moff = np.concatenate([[0], np.cumsum(tb.dims)])
    for c in range(len(ev)):
        fam = E.split_cells(tb, post[c])
        for v in range(tb.V):
            if ev[c, v] < 0:
                m = fmarg[c, moff[v]:moff[v + 1]]
                assert (np.abs(fam[v].sum(axis=1) - m) <= (2 * b + 1e-12) * np.maximum(m, 1.0)).all(), (c, v)
    # log P(x*, e) <= log P(e), and >= the max-sum elimination less its tolerance
    ex = P.ExactProb(*tables)
    assign, log_p = F.MostProbableExplanation(net, device=0).infer(ev)
    log_e = em2.log_likelihood(ev)
    for c in range(len(ev)):
        ve = M.max_sum_ve(ex, ev[c])
        assert log_p[c] <= log_e[c] + 1e-12 * abs(log_e[c])
        assert log_p[c] >= ve - M.ve_tolerance(ex, ve), (c, log_p[c], ve)
