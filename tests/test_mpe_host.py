"""Most probable explanation, host twin (MostProbableExplanation with device=-1: jt_mpe_plan.cpp,
jt_mpe_host.cpp).  Yardsticks and bounds: mpe_nets.py (exact rationals from the networks' counts, bound
3 * V * 2^-53; brute-force enumeration, an exact Viterbi, a numpy max-sum variable elimination).  The same
checks run on the device's own output in test_gpu_mpe.py."""
import numpy as np
import pytest
from conftest import synth_net_cases, tie_network
from mpe_nets import (ARG, CHAIN_SIZES, LIMIT, NODEV, ExactNet, alarm_cases, alarm_net, bound, chain_cases,
                      chain_net, check_alarm, check_brute_force, check_case, check_chain, disconnected_net, log_of, mixed_cases, shapes_net,
                      tree_viterbi, value_fraction)

import fastbn_amd as F
from fastbn_amd import synth

# synth.random_network(12 nodes, states 2..3, k_min = 0): the first is connected; the second has a
# disconnected moral graph (components of 4, 1 and 7 nodes: an isolated node among them), asserted below
RANDOM_NETS = {"connected": dict(n_nodes=12, seed=3, window=4, parent_probs=(0.2, 0.5, 0.3), dom=(2, 3), k_min=0),
               "disconnected": dict(n_nodes=12, seed=4, window=3, parent_probs=(0.45, 0.35, 0.2), dom=(2, 3), k_min=0)}


def random_net(tmp_path, name):
    xml = str(tmp_path / (name + ".xml"))
    _, parents, _ = synth.random_network(path=xml, name=name, **RANDOM_NETS[name])
    net = F.Network(xml)
    return net, ExactNet(net), parents


def brute_force_share(net, en, seed, device=-1):
    ev = mixed_cases(net, seed)
    assert sorted(set((ev >= 0).sum(1))) == sorted({0, 1, min(3, en.V - 1), en.V})
    mpe = F.MostProbableExplanation(net, device=device)
    assign, value = mpe.value_parts(ev)
    nclear = check_brute_force(en, ev, assign, value)
    assert nclear >= 0.9 * len(ev), nclear
    return mpe


def test_brute_force_shapes_graph():
    """A 1-state node, a 127-state node, a six-parent family, a descending parent order; three components."""
    net, en = shapes_net()
    mpe = brute_force_share(net, en, 11)
    assert mpe.info()["components"] == 3 == len(en.components())


@pytest.mark.parametrize("name", ["connected", "disconnected"])
def test_brute_force_random_networks(tmp_path, name):
    net, en, parents = random_net(tmp_path, name)
    comps = en.components()
    if name == "connected":
        assert len(comps) == 1
    else:
        assert len(comps) > 1 and any(len(c) == 1 for c in comps)
    mpe = brute_force_share(net, en, 21)
    assert mpe.info()["components"] == len(comps)


def test_brute_force_two_polytrees_and_an_isolated_node():
    net, en = disconnected_net()
    brute_force_share(net, en, 31)


@pytest.mark.parametrize("n", CHAIN_SIZES)
def test_underflow_chain(n):
    """P(x*, e) is far below fp64's smallest subnormal; mantissa and exponent still carry it exactly."""
    net, _ = chain_net(n)
    mpe = F.MostProbableExplanation(net, device=-1)
    assign, value = mpe.value_parts(chain_cases(n))
    assert check_chain(n, assign, value) >= 1
    _, log_p = mpe.infer(chain_cases(n))
    assert np.isfinite(log_p).all() and log_p[2] < -745  # exp(log_p) would be 0.0


def tie_setup(tmp_path):
    xml = tie_network(str(tmp_path / "tie.xml"))
    net = F.Network(xml)
    return net, ExactNet(net), synth_net_cases("tie", xml)


def check_ties(net, en, ev, assign, value):
    exact_ties = 0
    for c in range(len(ev)):
        best, _, unique = tree_viterbi(en, ev[c])
        exact_ties += not unique
        p = check_case(en, ev[c], assign[c], value[c])
        assert abs(value_fraction(value[c]) - best) <= bound(en.V) * best
        assert p <= best and best - p <= bound(en.V) * best  # the assignment attains the maximum
    assert exact_ties >= 1  # at least the case that observes nothing ties exactly


def test_ties(tmp_path):
    net, en, ev = tie_setup(tmp_path)
    mpe = F.MostProbableExplanation(net, device=-1)
    assign, value = mpe.value_parts(ev)
    check_ties(net, en, ev, assign, value)
    a2, v2 = mpe.value_parts(ev)
    assert assign.tobytes() == a2.tobytes() and value.tobytes() == v2.tobytes()
    parts = [mpe.value_parts(ev[lo:hi]) for lo, hi in ((0, 1), (1, 23), (23, len(ev)))]
    assert np.concatenate([p[0] for p in parts]).tobytes() == assign.tobytes()
    assert np.concatenate([p[1] for p in parts]).tobytes() == value.tobytes()


def test_alarm_against_max_sum_elimination():
    net, _ = alarm_net()
    mpe = F.MostProbableExplanation(net, device=-1)
    assign, value = mpe.value_parts(alarm_cases())
    a2, log_p = mpe.infer(alarm_cases())
    assert a2.tobytes() == assign.tobytes()
    np.testing.assert_array_equal(log_p, log_of(value))
    check_alarm(assign, value, log_p)
    i = mpe.info()
    assert i["cliques"] == 27 and i["components"] == 1 and i["store_rows"] < i["entries"]
    msg, exps = mpe.debug_messages(alarm_cases()[:3])
    assert msg.shape == (3, i["store_rows"] - 2 * i["cliques"] + 1) and exps.shape == (3, 26)
    assert (msg >= 0).all() and (msg < 1).all()  # every separator's maximum is scaled into [0.5, 1)


def test_arguments(tmp_path):
    net, _ = alarm_net()
    mpe = F.MostProbableExplanation(net, device=-1)
    ev = alarm_cases()[:4].copy()
    ev[2, 5] = 9
    with pytest.raises(F.FastBNError, match="case 2: evidence 9 for node 5") as e:
        mpe.infer(ev)
    assert e.value.code == ARG
    ev[2, 5] = -2
    with pytest.raises(F.FastBNError, match="case 2: evidence -2 for node 5") as e:
        mpe.infer(ev)
    assert e.value.code == ARG
    # fbn_network_create refuses a cycle itself; the XMLBIF loader does not
    var = "<VARIABLE><NAME>%s</NAME><TYPE>discrete</TYPE><VALUE>0</VALUE><VALUE>1</VALUE></VARIABLE>\n"
    prob = "<PROBABILITY><FOR>%s</FOR><GIVEN>%s</GIVEN><TABLE>0.5 0.5 0.5 0.5 </TABLE></PROBABILITY>\n"
    xml = tmp_path / "cyclic.xml"
    xml.write_text('<?xml version="1.0"?>\n<BIF><NETWORK><NAME>c</NAME>\n' + var % "A" + var % "B" + prob % ("A", "B")
                   + prob % ("B", "A") + "</NETWORK></BIF>\n")
    with pytest.raises(F.FastBNError, match="cycle") as e:
        F.MostProbableExplanation(F.Network(str(xml)), device=-1)
    assert e.value.code == ARG
    # one wave's store: store_rows rows of 64 fp64
    need = mpe.info()["store_rows"] * 512
    with pytest.raises(F.FastBNError, match="budget") as e:
        mpe.set_tuning(store_bytes_max=need - 1)
    assert e.value.code == LIMIT
    mpe.set_tuning(max_workgroups=3, store_bytes_max=need)  # fits exactly
    a, _ = mpe.infer(alarm_cases()[:4])
    assert a.shape == (4, 37)
    with pytest.raises(F.FastBNError) as e:
        mpe.run_device(0x1000, 4, 0x1000, 0x1000)
    assert e.value.code == NODEV
    a, lp = mpe.infer(np.zeros((0, 37), np.int8))
    assert a.shape == (0, 37) and lp.shape == (0,)
