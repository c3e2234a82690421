"""Exact posterior sampling, the host twin (PosteriorSampler(net, device=-1)), against yardsticks that know
no junction tree: em_nets' brute-force family posteriors, mpe_nets / prob_nets' exact rationals, and the
E-step's value bytes.  The count bound is derived in psample_nets.py.

Network.from_cpts refuses a CPT entry that is not > 0, so no network of this project has a zero entry; the
support check runs on the skewed probability network instead, whose entries go down to 1e-40."""
import itertools

import numpy as np
import pytest
from em_nets import Tables, brute_posteriors
from mpe_nets import ExactNet, alarm_cases, alarm_net, chain_cases, chain_net
from psample_nets import DIST_NETS, S_DIST, assert_binomial, family_cells, net_cases

import fastbn_amd as F
import prob_nets


def _skewed():
    dims, parents, cpts = prob_nets.small("skewed")
    return F.Network.from_cpts(dims, parents, cpts), prob_nets.cases(dims, 8, 3), prob_nets.ExactProb(dims, parents, cpts)


@pytest.mark.parametrize("key", DIST_NETS + ("skewed",))
def test_evidence_support_complete_rows(key):
    net, ev, en = _skewed() if key == "skewed" else net_cases(key) + (None,)
    en = en or ExactNet(net)
    samples, log_p = F.PosteriorSampler(net, device=-1).sample(ev, draws=24, seed=2)
    assert samples.shape == (len(ev), 24, net.num_nodes) and np.isfinite(log_p).all()
    assert (samples >= 0).all() and (samples < np.asarray(net.dims)).all()
    for c in range(len(ev)):
        assert ((ev[c] < 0) | (samples[c] == ev[c])).all(), c  # every sample carries its evidence
        if (ev[c] >= 0).all():
            assert (samples[c] == ev[c]).all(), c  # a complete row returns itself
        for x in np.unique(samples[c], axis=0):
            assert en.prob(x) > 0, (c, x)


@pytest.mark.parametrize("key", DIST_NETS + ("chain2000", "alarm"))
def test_value_is_the_estep_value(key):
    if key == "chain2000":
        net, ev = chain_net(2000)[0], chain_cases(2000)
    elif key == "alarm":
        net, ev = alarm_net()[0], alarm_cases()
    else:
        net, ev = net_cases(key)
    _, value = F.PosteriorSampler(net, device=-1).value_parts(ev, draws=1)
    _, want = F.ExpectationMaximization(net, device=-1).estep(ev)
    assert value.tobytes() == want.tobytes()
    if key == "chain2000":
        assert value[2, 1] < -1074 and 0.5 <= value[2, 0] < 1  # mantissa and exponent survive


@pytest.mark.parametrize("case", [0, 3, 6])  # nothing, one and three variables observed
@pytest.mark.parametrize("key", DIST_NETS)
def test_family_cell_frequencies(key, case):
    net, ev = net_cases(key)
    tb = Tables(net)
    post, _ = brute_posteriors(tb, ev[case])
    samples, _ = F.PosteriorSampler(net, device=-1).sample(ev[case:case + 1], draws=S_DIST, seed=1234 + case)
    n = family_cells(samples[0], tb)
    assert (n[post == 0] == 0).all()
    assert_binomial(n, post, S_DIST, (key, case))
    if key == "tiny":  # the full joint over complete assignments
        en = ExactNet(net)
        states = list(itertools.product(*[range(d) for d in tb.dims]))
        p = np.array([float(en.prob(x)) if all(e < 0 or e == v for e, v in zip(ev[case], x)) else 0.0 for x in states])
        index = np.ravel_multi_index(samples[0].T.astype(np.int64), tb.dims)
        assert_binomial(np.bincount(index, minlength=len(states)), p / p.sum(), S_DIST, ("joint", case))


def test_stream_positions_are_numpy_pcg64():
    """Three isolated nodes with one CPT: three root cliques, so draw (c, s) takes the numbers at positions
    ((case_offset + c) * S + s) * 3 + i of numpy's own PCG64 and the stated rule picks the states."""
    cnt = np.array([[5], [1], [9]])
    net = F.Network.from_counts(np.full(3, 3, np.int32), [[], [], []], [cnt] * 3)
    S, seed, off = 4, 12, 3
    samples, _ = F.PosteriorSampler(net, device=-1).value_parts(np.full((2, 3), -1, np.int8), S, seed, off)
    u = np.random.Generator(np.random.PCG64(seed)).random((off + 2) * S * 3).reshape(off + 2, S, 3)[off:]
    p = (cnt[:, 0] + 1.0) / (cnt.sum() + 3.0)
    t = u * ((p[0] + p[1]) + p[2])
    want = (p[0] <= t).astype(np.int8) + (p[0] + p[1] <= t)
    assert any((samples == want[:, :, list(perm)]).all() for perm in itertools.permutations(range(3)))


def test_split_with_case_offset_changes_nothing():
    net, ev = net_cases("star")
    ps = F.PosteriorSampler(net, device=-1)
    samples, value = ps.value_parts(ev, draws=5, seed=9, case_offset=3)
    for cut in range(1, len(ev)):
        a, va = ps.value_parts(ev[:cut], draws=5, seed=9, case_offset=3)
        b, vb = ps.value_parts(ev[cut:], draws=5, seed=9, case_offset=3 + cut)
        assert np.concatenate([a, b]).tobytes() == samples.tobytes() and np.concatenate([va, vb]).tobytes() == value.tobytes()
    assert ps.value_parts(ev, draws=5, seed=10, case_offset=3)[0].tobytes() != samples.tobytes()


def test_arguments_and_zero_cases():
    net, ev = net_cases("tiny")
    ps = F.PosteriorSampler(net, device=-1)
    assert ps.sample(ev[:0], draws=3)[0].shape == (0, 3, 5)
    for kw in (dict(draws=0), dict(draws=1, case_offset=-1)):
        with pytest.raises(F.FastBNError) as e:
            ps.value_parts(ev, **kw)
        assert e.value.code == -1, kw
    bad = ev.copy()
    bad[2, 1] = 3
    with pytest.raises(F.FastBNError, match="case 2.*node 1"):
        ps.sample(bad)
