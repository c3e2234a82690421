"""Gibbs sampling on the host twin (GibbsSampling(device=-1); gibbs_host.cpp over gibbs_model.h).

Yardstick: prob_nets.ExactProb, the tables as exact rationals.  The conditional of a variable given all
the others is a ratio of joint probabilities; the posterior marginals come from its enumeration.

A network with a zero table entry cannot be built through the library (Network.from_cpts refuses it, counts
are smoothed), so the dead-end rule (tot == 0 keeps the value) is driven on a hand-built model by
tools/gibbs_host_check.cpp, not here."""
import functools
from fractions import Fraction

import numpy as np
import prob_nets as PN
import pytest

import fastbn_amd as F

ARG, LIMIT = -1, -6  # fbn_err_t (include/fastbn.h)
NETS = {"benign": lambda: PN.small("benign"), "skewed": lambda: PN.small("skewed"), "shapes": PN.shapes}
CHAINS, BURN_IN, SWEEPS = 4096, 64, 128


@functools.lru_cache(maxsize=None)
def benign_reference():
    """small("benign"), its 16 cases and their exact marginals [16][sum_dom] (zeros for observed variables)."""
    dims, parents, cpts = PN.small("benign")
    ev = PN.cases(dims, 16, 3)
    ex = PN.ExactProb(dims, parents, cpts)
    p = np.array([[float(q) for row in ex.enumerate(e).marg for q in row] for e in ev])
    return (dims, parents, cpts), ev, p


def check_marginal_bound(dims, ev, marg, p):
    """Every unobserved entry within 5 sigma of `CHAINS` independent draws: under stationarity a chain's sweep
    average has at most one draw's variance, Rao-Blackwellising only lowers it, the chains are independent."""
    free = np.repeat(ev < 0, dims, axis=1)
    assert free.any(axis=1).sum() >= 15
    assert (np.abs(marg - p)[free] <= (5 * np.sqrt(p * (1 - p) / CHAINS) + 1e-12)[free]).all()
    assert (marg[~free] == 0).all()


@pytest.mark.parametrize("name", list(NETS))
def test_conditionals_against_enumeration(name):
    """Relative error <= (f + r + 1) 2^-52 per entry, f factors (1 + children), r states: f - 1 roundings in
    the product, at most that plus r - 1 in the sum, one in the division.  Catches a wrong stride, child
    order or base index."""
    dims, parents, cpts = NETS[name]()
    ex = PN.ExactProb(dims, parents, cpts)
    xs = (np.random.default_rng(len(dims)).integers(0, 1 << 30, (32, len(dims))) % dims).astype(np.int8)
    got = F.GibbsSampling(F.Network.from_cpts(dims, parents, cpts), device=-1).conditionals(xs)
    off = np.concatenate([[0], np.cumsum(dims)])
    for x, row in zip(xs, got):
        for v, r in enumerate(dims):
            fam = [v] + ex.children[v]
            joint = [ex.prob(np.concatenate([x[:v], [k], x[v + 1:]]), fam) for k in range(r)]
            for k in range(r):
                want = joint[k] / sum(joint)
                assert abs(Fraction(float(row[off[v] + k])) - want) <= want * (len(fam) + int(r) + 1) * Fraction(1, 2 ** 52)


def test_marginals_against_enumeration():
    (dims, parents, cpts), ev, p = benign_reference()
    g = F.GibbsSampling(F.Network.from_cpts(dims, parents, cpts), CHAINS, SWEEPS, BURN_IN, seed=0, device=-1)
    labels, marg = g.infer(ev)
    check_marginal_bound(dims, ev, marg, p)
    np.testing.assert_array_equal(labels[ev[:, 0] < 0], np.argmax(marg[:, :dims[0]], axis=1)[ev[:, 0] < 0])


def test_split_and_clamping():
    """A batch split with case_offset equals one call bit for bit; observed rows are zero, observed states clamped."""
    dims, parents, cpts = PN.shapes()
    ev = PN.cases(dims, 7, 5)
    g = F.GibbsSampling(F.Network.from_cpts(dims, parents, cpts), chains=70, sweeps=4, burn_in=2, seed=3, device=-1)
    lab, marg, st = g.infer(ev, states=True)
    parts = [g.infer(ev[:3], states=True), g.infer(ev[3:], states=True, case_offset=3)]
    for whole, k in ((lab, 0), (marg.view(np.uint64), 1), (st, 2)):
        np.testing.assert_array_equal(whole, np.concatenate([np.asarray(p[k]).view(whole.dtype) for p in parts]))
    assert (marg[np.repeat(ev >= 0, dims, axis=1)] == 0).all()
    assert (np.abs(marg.reshape(7, -1)[:, :dims[0]].sum(axis=1)[ev[:, 0] < 0] - 1) < 1e-12).all()
    clamp = np.broadcast_to(ev[:, None, :], st.shape)
    assert (st[clamp >= 0] == clamp[clamp >= 0]).all() and (st >= 0).all() and (st < dims).all()
    assert len({bytes(r) for r in st[0]}) > 1  # the chains differ
    assert g.infer(ev, marginals=False)[1] is None


def test_refusals():
    """A star whose hub's family products can underflow is refused by name; so are bad run arguments."""
    n = 9  # the hub's smallest entry times eight children's 1e-40: below 2^-969
    dims = np.full(n, 2, np.int32)
    tiny = np.array([[1e-40, 0.5], [1 - 1e-40, 0.5]])
    with pytest.raises(F.FastBNError, match="node 0") as e:
        F.GibbsSampling(F.Network.from_cpts(dims, [[]] + [[0]] * (n - 1), [np.array([[0.5], [0.5]])] + [tiny] * (n - 1)), device=-1)
    assert e.value.code == LIMIT
    dims, parents, cpts = PN.small()
    net = F.Network.from_cpts(dims, parents, cpts)
    for kw in (dict(chains=0), dict(sweeps=0), dict(burn_in=-1)):
        with pytest.raises(F.FastBNError) as e:
            F.GibbsSampling(net, device=-1, **kw).infer(PN.cases(dims, 2, 1))
        assert e.value.code == ARG
