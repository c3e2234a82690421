"""The sampling engine's host path (Sampler / LikelihoodWeighting with device=-1: sample_host.cpp, the
kernels' algorithm chunk for chunk on CPU threads).

Yardsticks: the existing generators (synth.forward_sample, Network.forward_sample) for forward
sampling, bit for bit; a numpy restatement of likelihood weighting / logic sampling (below) for
values and scaled weights, bit for bit, and for the sums within a derived bound; the oracle's exact
junction tree for convergence.  The restatement and the helpers are shared with test_gpu_sample.py."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
from conftest import ALARM

import fastbn_amd as F
import oracle as O
from fastbn_amd import synth

ARG, LIMIT = -1, -6  # fbn_err_t (include/fastbn.h)
U = 2.0 ** -53
XML = os.path.join(ALARM, "alarm.xml")


def restate(net, ev, S, seed, pls=False, case_offset=0):
    """Likelihood weighting (pls: logic sampling) of the cases ev [C][V] with S samples each, in
    numpy: sample i = (case_offset + c) * S + s takes row i of PCG64(seed)'s doubles drawn as
    [.., V] (the inference map), variable by variable in synth._topo order, synth.forward_sample's
    selection rule; weights as (m, e) by frexp.  -> dict(val [V][C*S], m, e, marg, sumw, ess, le, lab)."""
    names, dims, parents, cpts = net
    V, Cn = len(dims), len(ev)
    n = Cn * S
    bg = np.random.PCG64(seed)
    bg.advance(case_offset * S * V)
    u = np.random.Generator(bg).random((n, V))
    evr = np.repeat(np.asarray(ev, np.int64), S, axis=0)
    val = np.zeros((V, n), np.int64)
    m, e = np.ones(n), np.zeros(n, np.int64)
    for k, v in enumerate(synth._topo(parents)):
        rows = cpts[v].reshape(dims[v], -1)  # [value][parent config], GIVEN order, last fastest
        pc = np.zeros(n, np.int64)
        for g in parents[v]:
            pc = pc * dims[g] + val[g]
        pr = rows[:, pc]
        cdf = np.cumsum(pr, axis=0)
        samp = np.minimum(((u[:, k] * cdf[-1])[None] >= cdf).sum(0), dims[v] - 1)
        obs = evr[:, v] >= 0
        if pls:
            val[v] = samp
            m = np.where(obs & (samp != evr[:, v]), 0.0, m)
        else:
            val[v] = np.where(obs, evr[:, v], samp)
            if obs.any():
                mm, de = np.frexp(m * pr[val[v], np.arange(n)])
                m, e = np.where(obs, mm, m), np.where(obs, e + de, e)
    emax = e.reshape(Cn, S).max(1)
    w = np.ldexp(m, (e - emax.repeat(S)).astype(np.int32)).reshape(Cn, S)
    sumw = w.sum(1)
    off = np.concatenate([[0], np.cumsum(dims)])
    marg = np.zeros((Cn, off[-1]))
    with np.errstate(divide="ignore", invalid="ignore"):
        for v in range(V):
            vv = val[v].reshape(Cn, S)
            for q in range(dims[v]):
                marg[:, off[v] + q] = (w * (vv == q)).sum(1) / sumw
            marg[np.asarray(ev)[:, v] >= 0, off[v]:off[v + 1]] = 0
        marg[sumw == 0] = 0
        ess = np.where(sumw > 0, sumw ** 2 / (w ** 2).sum(1), 0.0)
        le = np.where(sumw > 0, np.log(sumw / S) + emax * math.log(2.0), -np.inf)
    lab = np.array([-1 if sumw[c] == 0 else _argmax(marg[c, :dims[0]]) for c in range(Cn)], np.int32)
    return dict(val=val.astype(np.uint8), m=m, e=e.astype(np.int32), marg=marg, sumw=sumw, ess=ess, le=le, lab=lab)


def _argmax(row):
    lab, mp = 0, 0.0  # strict '>' from state 0, as fbn_jt_run
    for q, p in enumerate(row):
        if p > mp:
            mp, lab = p, q
    return lab


def net_tuple(dims, parents, counts):
    """synth's (names, dims, parents, cpts) of a Network.from_counts network: counts[v] is
    [value][configurations of the ASCENDING parents]; cpts[v] is [value, GIVEN parents...]."""
    dims = np.asarray(dims, np.int32)
    cpts = []
    for v, ps in enumerate(parents):
        asc = sorted(ps)
        a = np.asarray(counts[v], np.int64).reshape([dims[v]] + [dims[q] for q in asc])
        a = a.transpose([0] + [1 + asc.index(g) for g in ps])
        cpts.append((a + 1.0) / (a.sum(axis=0, keepdims=True) + 1.0 * dims[v]))
    return ["X%d" % v for v in range(len(dims))], dims, [list(p) for p in parents], cpts


def check_against_restatement(lw, net, ev, S, seed, pls=False):
    """Values and (m, e) bit-equal; marginals within 4 S u relative (numerator and denominator are
    sums of S non-negative terms: either order is within (S - 1) u of exact, u = 2^-53), zeros where
    the restatement has zeros; log_evidence = log(sumw / S) + emax ln 2 within 4 S u (sumw) plus
    8 u |log_evidence| (two correctly rounded-to-1-ulp logs, one product, one sum); ess =
    sumw^2 / sum w^2 within 8 S u relative (twice sumw's bound plus sum w^2's); labels equal."""
    r = restate(net, ev, S, seed, pls)
    val, m, e = lw.debug_samples(ev)
    np.testing.assert_array_equal(val, r["val"])
    np.testing.assert_array_equal(m.view(np.uint64), r["m"].view(np.uint64))
    np.testing.assert_array_equal(e, r["e"])
    lab, marg = lw.infer(ev)
    le, ess = lw.stats
    assert np.isfinite(marg).all()
    assert ((marg == 0) == (r["marg"] == 0)).all()
    assert (np.abs(marg - r["marg"]) <= 4 * S * U * np.abs(r["marg"])).all()
    np.testing.assert_array_equal(lab, r["lab"])
    dead = r["sumw"] == 0
    assert (le[dead] == -np.inf).all() and (ess[dead] == 0).all()
    live = ~dead
    assert (np.abs(le[live] - r["le"][live]) <= 4 * S * U + 8 * U * np.abs(r["le"][live])).all()
    assert (np.abs(ess[live] - r["ess"][live]) <= 8 * S * U * r["ess"][live]).all()
    return r, lab, marg


@functools.lru_cache(maxsize=None)
def alarm():
    return F.Network(XML), synth.read_xmlbif(XML)


@functools.lru_cache(maxsize=None)
def alarm_cases():
    ev, _ = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)
    ev.setflags(write=False)
    return ev


# one unobserved binary root (P(1) = 1/4) and 60 observed binary children with
# P(child = 1 | root = 0) = 1 / (10^6 + 2), P(child = 1 | root = 1) = 1/2: the weight of a root = 0
# sample is 10^-360, below fp64
UF_DIMS = [2] * 61
UF_PARENTS = [[]] + [[0]] * 60
UF_COUNTS = [[[2], [0]]] + [[[10 ** 6, 1], [0, 1]]] * 60
UF_EV = np.array([[-1] + [1] * 60], np.int8)


@functools.lru_cache(maxsize=None)
def underflow_net():
    return F.Network.from_counts(UF_DIMS, UF_PARENTS, UF_COUNTS), net_tuple(UF_DIMS, UF_PARENTS, UF_COUNTS)


def check_underflow(lw, S=256):
    """The root's posterior in closed form, in logs: n1 p1^60 / (n0 p0^60 + n1 p1^60) with the
    restatement's root counts."""
    net, tup = underflow_net()
    r = restate(tup, UF_EV, S, lw.seed)
    n1 = int(r["val"][0].sum())
    n0 = S - n1
    l0 = (math.log(n0) if n0 else -math.inf) + 60 * math.log(1.0 / (10 ** 6 + 2))
    l1 = (math.log(n1) if n1 else -math.inf) + 60 * math.log(0.5)
    tot = np.logaddexp(l0, l1)
    lab, marg = lw.infer(UF_EV)
    le, ess = lw.stats
    assert np.isfinite(marg).all() and np.isfinite(le).all() and np.isfinite(ess).all()
    assert abs(marg[0, 0] - math.exp(l0 - tot)) <= 1e-12 and abs(marg[0, 1] - math.exp(l1 - tot)) <= 1e-12
    assert (marg[0, 2:] == 0).all()
    assert le[0] >= -829 * math.log(10.0) and abs(le[0] - (tot - math.log(S))) <= 1e-9
    assert 0 < n1 < S and lab[0] == 1


@pytest.mark.parametrize("n", [1, 63, 65, 4097])
def test_forward_parity(n):
    net, tup = alarm()
    got = F.Sampler(net, device=-1).forward_sample(n, 11)
    assert got.dtype == np.uint8 and got.shape == (37, n)
    np.testing.assert_array_equal(got, synth.forward_sample(tup, n, 11))
    np.testing.assert_array_equal(got, net.forward_sample(n, 11))


@pytest.mark.parametrize("method", ["lw", "pls"])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 200])
def test_lw_pls_equal_restatement(S, method):
    net, tup = alarm()
    ev = alarm_cases()[:8]
    lw = F.LikelihoodWeighting(net, S, seed=5, device=-1, method=method)
    check_against_restatement(lw, tup, ev, S, 5, pls=method == "pls")


def test_convergence_against_exact_inference():
    """32 cases, S = 4096, seed 7: every unobserved entry within 5 sqrt(p (1 - p) / ess) of the exact
    marginal; evidence-free cases have every weight 1 and ess == S exactly."""
    net, tup = alarm()
    S = 4096
    full = synth.forward_sample(tup, 32, 3)
    ev = np.full((32, 37), -1, np.int8)
    for c in range(16, 32):
        v = 1 + (7 * c) % 36
        ev[c, v] = full[v, c]
    lw = F.LikelihoodWeighting(net, S, seed=7, device=-1)
    lab, marg = lw.infer(ev)
    le, ess = lw.stats
    _, exact = O.OracleJT(XML).infer(ev)
    assert (ess[:16] == S).all() and (le[:16] == 0).all()
    _, m, e = lw.debug_samples(ev[:2])
    assert (m == 1.0).all() and (e == 0).all()
    off = np.concatenate([[0], np.cumsum(tup[1])])
    worst = 0.0
    for c in range(32):
        for v in range(37):
            if ev[c, v] >= 0:
                assert (marg[c, off[v]:off[v + 1]] == 0).all()
                continue
            p, ph = exact[c, off[v]:off[v + 1]], marg[c, off[v]:off[v + 1]]
            z = np.abs(ph - p) / np.sqrt(p * (1 - p) / ess[c])
            worst = max(worst, float(z.max()))
    print("worst z", worst, "min ess", ess.min())
    assert worst <= 5.0
    assert ess.min() > 1000


def test_underflow_is_scaled_away():
    net, _ = underflow_net()
    check_underflow(F.LikelihoodWeighting(net, 256, seed=1, device=-1))


def test_pls_without_an_accepted_sample():
    net, tup = underflow_net()
    lw = F.LikelihoodWeighting(net, 256, seed=1, device=-1, method="pls")
    lab, marg = lw.infer(UF_EV)
    assert lab[0] == -1 and (marg == 0).all()
    assert lw.stats[0][0] == -np.inf and lw.stats[1][0] == 0
    check_against_restatement(lw, tup, UF_EV, 256, 1, pls=True)


def test_batch_split_invariance():
    net, _ = alarm()
    ev = alarm_cases()[:37]
    lw = F.LikelihoodWeighting(net, 100, seed=9, device=-1)
    lab, marg = lw.infer(ev)
    st = np.stack(lw.stats)
    la, ma = lw.infer(ev[:20])
    sa = np.stack(lw.stats)
    lb, mb = lw.infer(ev[20:], case_offset=20)
    sb = np.stack(lw.stats)
    np.testing.assert_array_equal(lab, np.concatenate([la, lb]))
    np.testing.assert_array_equal(marg.view(np.uint64), np.concatenate([ma, mb]).view(np.uint64))
    np.testing.assert_array_equal(st.view(np.uint64), np.concatenate([sa, sb], axis=1).view(np.uint64))
    l2, m2 = lw.infer(ev)
    np.testing.assert_array_equal(marg.view(np.uint64), m2.view(np.uint64))
    assert not np.array_equal(lw.infer(ev[20:])[1], mb)  # the offset moves the stream


def test_errors():
    net, _ = alarm()
    ev = alarm_cases()[:4].copy()
    lw = F.LikelihoodWeighting(net, 16, device=-1)
    ref = lw.infer(ev)
    bad = ev.copy()
    bad[2, 5] = net.dims[5]  # one past the last state
    with pytest.raises(F.FastBNError, match="case 2.*node 5") as e:
        lw.infer(bad)
    assert e.value.code == ARG
    bad[2, 5] = -2
    with pytest.raises(F.FastBNError) as e:
        lw.debug_samples(bad)
    assert e.value.code == ARG
    with pytest.raises(F.FastBNError) as e:
        F.LikelihoodWeighting(net, 0, device=-1).infer(ev)
    assert e.value.code == ARG
    with pytest.raises(F.FastBNError):
        F.LikelihoodWeighting(net, 16, device=-1, method="ais")
    np.testing.assert_array_equal(lw.infer(ev)[1], ref[1])  # the handle stays usable
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
        F.Sampler(big, device=-1)
    assert e.value.code == LIMIT
    big.close()


def test_score_marginals_equals_jt_score():
    net, tup = alarm()
    rng = np.random.default_rng(4)
    SD = int(np.sum(tup[1]))
    marg = rng.random((50, SD))
    gold = rng.random((50, SD))
    off = np.concatenate([[0], np.cumsum(tup[1])])[:-1]
    for c in range(50):
        for v in rng.choice(37, 7, replace=False):
            gold[c, off[v]] = -1  # evidence nodes, as read_pt_file marks them
    a = F.JunctionTree(net, device=-1).score(marg, gold)
    b = F.score_marginals(net, marg, gold)
    assert a == b and np.isfinite(a).all() and a[0] > 0
