"""Most probable explanation on the device (jt_mpe.hip behind MostProbableExplanation).

The device is held to the host twin byte for byte -- assignment, both value doubles, the stored messages
and exponents -- at the case counts at which the kernel can go wrong (1: one lane and 63 tail lanes; 63,
64, 65: around a full wave; 130 with max_workgroups=1: one wave recycling its store over three blocks,
the last ragged; 130 again on the default grid), and to the yardsticks of mpe_nets.py on its own output
(brute force, the exact Viterbi, exact rationals, a numpy max-sum variable elimination), so it is not
only compared with its twin."""
import functools
import gzip
import os

import numpy as np
import pytest
from conftest import ALARM, SYNTH_NETS, synth_net_cases
from mpe_nets import (CHAIN_SIZES, UNDERFLOW, ExactNet, alarm_cases, alarm_net, chain_cases, chain_net, check_alarm,
                      check_brute_force, check_case, check_chain, disconnected_net, log_of, max_sum_ve, mixed_cases,
                      shapes_net, ve_tolerance)

import fastbn_amd as F

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def tie_net():
    import tempfile
    with gzip.open(os.path.join(SYNTH_NETS, "tie.xml.gz"), "rb") as f, \
            tempfile.NamedTemporaryFile("wb", suffix=".xml") as g:
        g.write(f.read())
        g.flush()
        net = F.Network(g.name)
        ev = synth_net_cases("tie", g.name)
    return net, np.concatenate([ev, ev, ev[:2]])  # the fixture's 64 cases (several tie exactly), repeated


def _cases(net, k, seed):
    """130 cases: nothing observed, everything observed, then k observed variables each."""
    full = net.forward_sample(1, seed).T.astype(np.int8)
    return np.concatenate([np.full((1, net.num_nodes), -1, np.int8), full, net.evidence_cases(128, k, seed + 1)])


@functools.lru_cache(maxsize=None)
def workload(key):
    if key == "shapes":
        net, ev = shapes_net()[0], _cases(shapes_net()[0], 3, 41)
    elif key == "disconnected":
        net, ev = disconnected_net()[0], _cases(disconnected_net()[0], 2, 42)
    elif key == "tie":
        net, ev = tie_net()
    elif key == "chain":
        net, ev = chain_net(1200)[0], _cases(chain_net(1200)[0], 120, 43)
    else:
        net = alarm_net()[0]
        ev = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)[0][:130]
    assert len(ev) == 130
    ev.setflags(write=False)
    host = F.MostProbableExplanation(net, device=-1)
    assign, value = host.value_parts(ev)
    msg, exps = host.debug_messages(ev)
    return net, ev, assign, value, msg, exps


@pytest.mark.parametrize("key", ["shapes", "disconnected", "tie", "chain", "alarm"])
def test_device_equals_host_twin(key):
    net, ev, assign, value, msg, exps = workload(key)
    dev = F.MostProbableExplanation(net, device=0)
    host_info = F.MostProbableExplanation(net, device=-1).info()
    assert dev.info() == host_info
    for n, groups in [(n, 1) for n in COUNTS] + [(130, 0)]:
        dev.set_tuning(max_workgroups=groups)
        a, v = dev.value_parts(ev[:n])
        assert a.tobytes() == assign[:n].tobytes(), (key, n, groups)
        assert v.tobytes() == value[:n].tobytes(), (key, n, groups)
        m, e = dev.debug_messages(ev[:n])
        assert m.tobytes() == msg[:n].tobytes() and e.tobytes() == exps[:n].tobytes(), (key, n, groups)
    assert dev.last_kernel_ms() > 0.0
    dev.close()


def test_device_brute_force_shapes_graph():
    net, en = shapes_net()
    ev = mixed_cases(net, 11)
    assign, value = F.MostProbableExplanation(net, device=0).value_parts(ev)
    assert check_brute_force(en, ev, assign, value) >= 0.9 * len(ev)


@pytest.mark.parametrize("n", CHAIN_SIZES)
def test_device_underflow_chain(n):
    assign, value = F.MostProbableExplanation(chain_net(n)[0], device=0).value_parts(chain_cases(n))
    assert check_chain(n, assign, value) >= 1


def test_device_alarm_against_max_sum_elimination():
    mpe = F.MostProbableExplanation(alarm_net()[0], device=0)
    assign, value = mpe.value_parts(alarm_cases())
    a2, log_p = mpe.infer(alarm_cases())
    assert a2.tobytes() == assign.tobytes()
    check_alarm(assign, value, log_p)


def test_munin_like(munin_fixture):
    """1041 variables, 956 cliques, 48,564 store rows.  96 cases: the 32 of the fixture (208 observed) and the
    64 extra ones (0 / 52 / 208 / 520 observed).  The max-sum elimination takes ~0.1 s per case, so it runs
    on every 6th case (16 cases, four of each block).  The exponent: the most probable explanation of this
    network is about 2^-808 with nothing observed and 2^-950 with 208 observed -- inside fp64's range; it
    is below 2^-1074 for the 520-observed cases, which is where the assertion on ex applies."""
    net = F.Network(munin_fixture["xml"])
    en = ExactNet(net)
    ev = np.concatenate([F.load_libsvm(munin_fixture[k], net.num_nodes)[0] for k in ("libsvm", "extra_libsvm")])
    assert len(ev) == 96 and sorted(set((ev >= 0).sum(1))) == [0, 52, 208, 520]
    host = F.MostProbableExplanation(net, device=-1)
    dev = F.MostProbableExplanation(net, device=0)
    assign, value = dev.value_parts(ev)
    ha, hv = host.value_parts(ev)
    assert assign.tobytes() == ha.tobytes() and value.tobytes() == hv.tobytes()
    m, e = dev.debug_messages(ev[:3])
    hm, he = host.debug_messages(ev[:3])
    assert m.tobytes() == hm.tobytes() and e.tobytes() == he.tobytes()
    log_p = log_of(value)
    below = 0
    for c in range(96):
        p = check_case(en, ev[c], assign[c], value[c])
        if p < UNDERFLOW:
            below += 1
            assert value[c, 1] < -1074
        if c % 6 == 0:
            ve = max_sum_ve(en, ev[c])
            assert log_p[c] >= ve - ve_tolerance(en, ve), (c, log_p[c], ve)
    assert below >= 8
    dev.close()


def test_run_device_on_a_side_stream():
    import torch
    net = alarm_net()[0]
    ev = alarm_cases()[:37].copy()
    mpe = F.MostProbableExplanation(net, device=0)
    assign, value = mpe.value_parts(ev)
    side = torch.cuda.Stream()
    d_ev = torch.from_numpy(ev).to("cuda")
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        with torch.cuda.stream(side):
            d_a = torch.full((37, 37), -7, dtype=torch.int8, device="cuda")
            d_v = torch.full((37, 2), -1.0, dtype=torch.float64, device="cuda")
            mpe.run_device(d_ev.data_ptr(), 37, d_a.data_ptr(), d_v.data_ptr(), stream_ptr=side.cuda_stream)
        side.synchronize()
        outs.append((d_a.cpu().numpy(), d_v.cpu().numpy()))
    assert mpe.last_kernel_ms() > 0.0
    for a, v in outs:
        assert a.tobytes() == assign.tobytes() and v.tobytes() == value.tobytes()
    # a bad code in a device buffer is refused before the kernel runs; the handle stays usable
    bad = ev.copy()
    bad[3, 4] = 100
    d_bad = torch.from_numpy(bad).to("cuda")
    with torch.cuda.stream(side):
        d_a = torch.full((37, 37), -7, dtype=torch.int8, device="cuda")
    side.synchronize()
    with pytest.raises(F.FastBNError, match="case 3.*node 4") as e:
        mpe.run_device(d_bad.data_ptr(), 37, d_a.data_ptr(), d_v.data_ptr(), stream_ptr=side.cuda_stream)
    assert e.value.code == -1
    side.synchronize()
    assert (d_a.cpu().numpy() == -7).all()  # nothing was launched
    a, v = mpe.value_parts(ev)
    assert a.tobytes() == assign.tobytes() and v.tobytes() == value.tobytes()
    mpe.close()
