"""Expectation-maximisation, host twin (ExpectationMaximization with device=-1: jt_em_plan.cpp, jt_em_host.cpp)
and probability networks (Network.from_cpts / node_probs).  Yardsticks and bounds: em_nets.py.  The same
checks run on the device's own output in test_gpu_em.py.  ParameterLearning counts on the device, so the
complete-data checks here use the same counts formed in numpy (test_gpu_em.py uses ParameterLearning)."""
import numpy as np
import oracle as O
import pytest
from em_nets import (ARG, SMALL_NETS, U, Tables, alarm_cases, alarm_complete, alarm_incomplete, alarm_net, alarm_parents,
                     assert_monotone, bits, bound, chain_net, check_against_brute_force,
                     check_against_fractions, check_chain, family_counts, manual_chain, mixed_cases, network_bits, small_net,
                     split_cells, sum_product_ve, tiny_net, uniform_start)
from mpe_nets import XML

import fastbn_amd as F


def test_tiny_net_against_fractions():
    net, en = tiny_net()
    ev = mixed_cases(net, 71)
    em = F.ExpectationMaximization(net, device=-1)
    _, value = em.estep(ev)
    check_against_fractions(net, en, ev, em.debug_posteriors(ev), value, bound(em))


@pytest.mark.parametrize("key", sorted(SMALL_NETS))
def test_brute_force(key):
    net, ev = small_net(key)
    assert sorted(set((ev >= 0).sum(1))) == sorted({0, 1, 3, net.num_nodes})
    em = F.ExpectationMaximization(net, device=-1)
    counts, value = em.estep(ev)
    post = em.debug_posteriors(ev)
    check_against_brute_force(net, ev, post, value, bound(em))
    # the counts are the posteriors added in case order
    flat = np.zeros(post.shape[1])
    for c in range(len(ev)):
        flat = flat + post[c]
    assert bits(counts) == flat.tobytes()


def test_alarm_evidence_probability_and_marginals():
    net, _ = alarm_net()
    ev = alarm_cases()
    tb = Tables(net)
    em = F.ExpectationMaximization(net, device=-1)
    assert em.info() == {"cliques": 27, "entries": 1110, "store_rows": em.info()["store_rows"], "cells": tb.cells, "components": 1}
    b = bound(em)
    log_p = em.log_likelihood(ev)
    post = em.debug_posteriors(ev)
    # JunctionForest infers on a device only (test_gpu_em.py uses it); here the CPU restatement of the
    # reference's junction tree gives the marginals
    _, marg = O.OracleJT(XML).infer(ev)
    moff = np.concatenate([[0], np.cumsum(tb.dims)])
    for c in range(len(ev)):
        want = np.log(sum_product_ve(tb, ev[c]))
        assert abs(log_p[c] - want) <= 2 * b + tb.V * U * abs(want), (c, log_p[c], want)
        fam = split_cells(tb, post[c])
        for v in range(tb.V):
            if ev[c, v] >= 0:
                continue
            m = marg[c, moff[v]:moff[v + 1]]
            assert (np.abs(fam[v].sum(axis=1) - m) <= (2 * b + 1e-12) * np.maximum(m, 1.0)).all(), (c, v)


def test_complete_data():
    """On complete rows the E-step counts, exactly; one iteration with alpha = 1 is count-based learning."""
    rows, dims = alarm_complete()
    parents = alarm_parents()
    want = family_counts(rows, dims, parents)
    em = F.ExpectationMaximization(uniform_start(dims, parents), device=-1)
    counts, value = em.estep(rows)
    for v in range(len(dims)):
        np.testing.assert_array_equal(counts[v], want[v].astype(np.float64))
    assert (value[:, 0] >= 0.5).all() and (value[:, 0] < 1).all()
    obj = em.fit(rows, max_iters=1, tol=0)
    assert obj.shape == (1, 2)
    learned = F.Network.from_counts(dims, parents, want)  # what LearnParamsKnowStructCompData builds
    assert network_bits(em.network()) == network_bits(learned)


def test_fit_equals_the_manual_chain():
    net, _ = alarm_net()
    parents = alarm_parents()
    data = alarm_incomplete()[:300]
    start = uniform_start(net.dims, parents)
    em = F.ExpectationMaximization(start, pseudo_count=0.5, device=-1)
    obj = em.fit(data, max_iters=3, tol=0)
    assert obj.shape == (3, 2)
    chain = F.ExpectationMaximization(start, pseudo_count=0.5, device=-1)
    theta = manual_chain(chain, data, parents, 3, 0.5)
    assert network_bits(em.network()) == bits(theta) == network_bits(chain.network())
    # the objective rows are those of the parameters each E-step ran with
    ll = F.ExpectationMaximization(start, device=-1).log_likelihood(data)
    assert abs(obj[0, 0] - ll.sum()) <= 1e-9 * abs(obj[0, 0])
    assert obj[0, 1] < obj[0, 0]  # the pseudo-count term is negative


def test_set_parameters_rebuilds_the_plan_potentials():
    net, _ = alarm_net()
    data = alarm_incomplete()[:64]
    fresh = F.ExpectationMaximization(net, device=-1)
    c0, v0 = fresh.estep(data)
    p0 = fresh.debug_posteriors(data)
    em = F.ExpectationMaximization(net, device=-1)
    em.fit(data, max_iters=2, tol=0)
    assert em.debug_posteriors(data).tobytes() != p0.tobytes()
    em.set_parameters(net)
    c1, v1 = em.estep(data)
    assert bits(c1) == bits(c0) and v1.tobytes() == v0.tobytes() and em.debug_posteriors(data).tobytes() == p0.tobytes()


def test_objective_never_decreases():
    net, _ = alarm_net()
    data = alarm_incomplete()
    assert len(data) == 2000 and 0.28 < (data < 0).mean() < 0.32
    em = F.ExpectationMaximization(uniform_start(net.dims, alarm_parents()), device=-1)
    obj = em.fit(data, max_iters=30, tol=0)
    assert obj.shape == (30, 2)
    assert_monotone(em, obj, len(data))
    # an early stop: a loose tolerance ends the loop before max_iters
    em2 = F.ExpectationMaximization(uniform_start(net.dims, alarm_parents()), device=-1)
    obj2 = em2.fit(data, max_iters=30, tol=1e-3)
    assert 2 <= len(obj2) < 30 and obj2.tobytes() == obj[:len(obj2)].tobytes()


def test_underflow_chain():
    check_chain(F.ExpectationMaximization(chain_net(2000)[0], device=-1), 2000)


def test_probability_networks():
    net, en = tiny_net()
    tb = Tables(net)
    # a count network's node_probs are (count + 1) / (total + |dom|)
    for v in range(tb.V):
        par, cnt = net.node_counts(v)
        np.testing.assert_array_equal(net.node_probs(v)[1], (cnt + 1.0) / (cnt.sum(axis=0) + 1.0 * tb.dims[v]))
    cpts = [net.node_probs(v)[1] for v in range(tb.V)]
    pn = F.Network.from_cpts(net.dims, en.parents, cpts, names=["n%d" % v for v in range(tb.V)])
    assert pn.name(3) == "n3" and network_bits(pn) == network_bits(net)
    # every consumer reads the entries: the E-step of the two networks is the same, to the byte
    ev = mixed_cases(net, 71)
    a = F.ExpectationMaximization(net, device=-1).debug_posteriors(ev)
    b = F.ExpectationMaximization(pn, device=-1).debug_posteriors(ev)
    assert a.tobytes() == b.tobytes()
    with pytest.raises(F.FastBNError, match="probability network holds no counts") as e:
        pn.node_counts(0)
    assert e.value.code == ARG
    bad = [c.copy() for c in cpts]
    bad[2][0, 1] += 1e-6
    with pytest.raises(F.FastBNError, match="node 2: .*sum to") as e:
        F.Network.from_cpts(net.dims, en.parents, bad)
    assert e.value.code == ARG
    bad = [c.copy() for c in cpts]
    bad[1][:, 0] = [0.0, 0.5, 0.5]
    with pytest.raises(F.FastBNError, match="node 1: .*not finite and > 0") as e:
        F.Network.from_cpts(net.dims, en.parents, bad)
    assert e.value.code == ARG


def test_arguments(tmp_path):
    net, _ = alarm_net()
    for alpha in (0.0, -1.0):
        with pytest.raises(F.FastBNError, match="pseudo-count") as e:
            F.ExpectationMaximization(net, pseudo_count=alpha, device=-1)
        assert e.value.code == ARG
    em = F.ExpectationMaximization(net, device=-1)
    em.pseudo_count = 0.0  # the C entry refuses it as well
    with pytest.raises(F.FastBNError, match="pseudo-count") as e:
        em.fit(alarm_cases()[:4], 1, 0)
    assert e.value.code == ARG
    em.pseudo_count = 1.0
    ev = alarm_cases()[:4].copy()
    ev[2, 5] = 9
    with pytest.raises(F.FastBNError, match="case 2: evidence 9 for node 5") as e:
        em.estep(ev)
    assert e.value.code == ARG
    with pytest.raises(F.FastBNError, match="case 2: evidence 9 for node 5"):
        em.fit(ev, 2, 0)
    with pytest.raises(F.FastBNError, match="structure|nodes") as e:
        em.set_parameters(tiny_net()[0])
    assert e.value.code == ARG
    parents = alarm_parents()
    other = [list(p) for p in parents]
    leaf = next(v for v in range(37) if not parents[v])
    donor = next(u for u in range(37) if u != leaf and leaf not in parents[u] and not parents[u])
    other[leaf] = [donor]
    with pytest.raises(F.FastBNError, match="node %d differs" % leaf) as e:
        em.set_parameters(uniform_start(net.dims, other))
    assert e.value.code == ARG
    var = "<VARIABLE><NAME>%s</NAME><TYPE>discrete</TYPE><VALUE>0</VALUE><VALUE>1</VALUE></VARIABLE>\n"
    prob = "<PROBABILITY><FOR>%s</FOR><GIVEN>%s</GIVEN><TABLE>0.5 0.5 0.5 0.5 </TABLE></PROBABILITY>\n"
    xml = tmp_path / "cyclic.xml"
    xml.write_text('<?xml version="1.0"?>\n<BIF><NETWORK><NAME>c</NAME>\n' + var % "A" + var % "B" + prob % ("A", "B")
                   + prob % ("B", "A") + "</NETWORK></BIF>\n")
    with pytest.raises(F.FastBNError, match="cycle") as e:
        F.ExpectationMaximization(F.Network(str(xml)), device=-1)
    assert e.value.code == ARG
    need = em.info()["store_rows"] * 512 + em.info()["cells"] * 8  # one wave's store and its accumulator
    with pytest.raises(F.FastBNError, match="budget") as e:
        em.set_tuning(store_bytes_max=need - 1)
    assert e.value.code == -6
    em.set_tuning(max_workgroups=3, store_bytes_max=need)
    with pytest.raises(F.FastBNError) as e:
        em.estep_device(0x1000, 4, 0x1000, 0x1000)
    assert e.value.code == -5
    counts, value = em.estep(np.zeros((0, 37), np.int8))
    assert value.shape == (0, 2) and all((c == 0).all() for c in counts)
