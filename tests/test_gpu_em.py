"""Expectation-maximisation on the device (jt_em.hip behind ExpectationMaximization).

The device is held to the host twin byte for byte on the per-case posteriors and values, at the case counts
at which the kernel can go wrong (1: one lane and 63 tail lanes; 63, 64, 65: around a full wave; 130 with
max_workgroups=1: one wave recycling its store over three blocks, the last ragged; 130 again on the default
grid); its summed counts to the twin's within B + n u (the device adds a lane's cases, then waves, then
lanes; the twin adds the cases in order), to itself byte for byte on a second run, and to exact integers on
fully observed rows; and to the yardsticks of em_nets.py on its own output (brute force, exact rationals, a
numpy variable elimination), so it is not only compared with its twin."""
import functools
import os

import numpy as np
import pytest
from conftest import ALARM
from em_nets import (SMALL_NETS, U, Tables, alarm_cases, alarm_complete, alarm_incomplete, alarm_net, alarm_parents,
                     assert_monotone, bits, bound, chain_net, check_against_brute_force, check_against_fractions,
                     check_chain, disconnected_net, manual_chain, mixed_cases, network_bits, nine_net, shapes_net,
                     small_net, split_cells, star_net, sum_product_ve, tiny_net, uniform_start)

import fastbn_amd as F

pytestmark = pytest.mark.gpu

SETTINGS = [(1, 1), (63, 1), (64, 1), (65, 1), (130, 1), (130, 0)]  # (cases, max_workgroups)


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
    elif key == "nine":
        net, ev = nine_net(), _cases(nine_net(), 3, 44)
    elif key == "star":
        net, ev = star_net(), _cases(star_net(), 2, 45)
    elif key == "chain":
        net, ev = chain_net(1200)[0], _cases(chain_net(1200)[0], 120, 43)
    else:
        net = alarm_net()[0]
        ev = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)[0][:130]
    assert len(ev) == 130
    ev.setflags(write=False)
    host = F.ExpectationMaximization(net, device=-1)
    post = host.debug_posteriors(ev)
    _, value = host.estep_flat(ev)
    counts = {n: host.estep_flat(ev[:n])[0] for n in sorted({n for n, _ in SETTINGS})}
    full = net.forward_sample(130, 77).T.astype(np.int8)
    return net, ev, post, value, counts, full, host.estep_flat(full)[0], host.info(), bound(host)


@pytest.mark.parametrize("key", ["shapes", "disconnected", "nine", "star", "chain", "alarm"])
def test_device_equals_host_twin(key):
    net, ev, post, value, counts, full, full_counts, info, b = workload(key)
    dev = F.ExpectationMaximization(net, device=0)
    assert dev.info() == info
    for n, groups in SETTINGS:
        dev.set_tuning(max_workgroups=groups)
        assert dev.debug_posteriors(ev[:n]).tobytes() == post[:n].tobytes(), (key, n, groups)
        c, v = dev.estep_flat(ev[:n])
        assert v.tobytes() == value[:n].tobytes(), (key, n, groups)
        want = counts[n]
        assert ((want == 0) == (c == 0)).all()
        assert (np.abs(c - want) <= (b + n * U) * want).all(), (key, n, groups, float(np.max(np.abs(c - want) / np.maximum(want, 1e-300))))
        c2, _ = dev.estep_flat(ev[:n])
        assert c2.tobytes() == c.tobytes(), (key, n, groups)
        # fully observed rows: exact integers, the complete-data counts
        cf, _ = dev.estep_flat(full[:n])
        assert (cf == np.round(cf)).all() and cf.sum() == n * net.num_nodes, (key, n, groups)
        if n == 130:
            assert cf.tobytes() == full_counts.tobytes(), (key, groups)
    assert dev.last_kernel_ms() > 0.0
    dev.close()


def test_device_against_fractions():
    net, en = tiny_net()
    ev = mixed_cases(net, 71)
    em = F.ExpectationMaximization(net, device=0)
    _, value = em.estep(ev)
    check_against_fractions(net, en, ev, em.debug_posteriors(ev), value, bound(em))


@pytest.mark.parametrize("key", sorted(SMALL_NETS))
def test_device_brute_force(key):
    net, ev = small_net(key)
    em = F.ExpectationMaximization(net, device=0)
    _, value = em.estep(ev)
    check_against_brute_force(net, ev, em.debug_posteriors(ev), value, bound(em))


def test_device_underflow_chain():
    check_chain(F.ExpectationMaximization(chain_net(2000)[0], device=0), 2000)


def test_device_alarm_evidence_probability_and_marginals():
    net, _ = alarm_net()
    ev = alarm_cases()
    tb = Tables(net)
    em = F.ExpectationMaximization(net, device=0)
    b = bound(em)
    log_p = em.log_likelihood(ev)
    post = em.debug_posteriors(ev)
    _, marg = F.JunctionForest(net, device=0).infer(ev)
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


def test_device_complete_data_equals_parameter_learning():
    rows, dims = alarm_complete()
    parents = alarm_parents()
    ds = F.Dataset(os.path.join(ALARM, "alarm_s5000.txt"))
    pl = F.ParameterLearning(ds, device=0)
    want = pl.counts(parents)
    em = F.ExpectationMaximization(uniform_start(dims, parents), device=0)
    counts, _ = em.estep(rows)
    for v in range(len(dims)):
        np.testing.assert_array_equal(counts[v], want[v].astype(np.float64))
    em.fit(rows, max_iters=1, tol=0)
    assert network_bits(em.network()) == network_bits(pl.LearnParamsKnowStructCompData(parents))


def test_device_fit_equals_the_manual_chain():
    net, _ = alarm_net()
    parents = alarm_parents()
    data = alarm_incomplete()[:300]
    start = uniform_start(net.dims, parents)
    em = F.ExpectationMaximization(start, pseudo_count=0.5, device=0)
    obj = em.fit(data, max_iters=3, tol=0)
    assert obj.shape == (3, 2)
    chain = F.ExpectationMaximization(start, pseudo_count=0.5, device=0)
    theta = manual_chain(chain, data, parents, 3, 0.5)
    assert network_bits(em.network()) == bits(theta) == network_bits(chain.network())
    # the loop left its potentials behind as well: one more E-step on each gives the same bytes
    assert em.estep_flat(data)[0].tobytes() == chain.estep_flat(data)[0].tobytes()


def test_device_objective_never_decreases():
    net, _ = alarm_net()
    data = alarm_incomplete()
    em = F.ExpectationMaximization(uniform_start(net.dims, alarm_parents()), device=0)
    obj = em.fit(data, max_iters=10, tol=0)
    assert obj.shape == (10, 2)
    assert_monotone(em, obj, len(data))
    assert em.last_kernel_ms() > 0.0


def test_estep_device_with_torch_buffers():
    import torch
    net, _ = alarm_net()
    data = alarm_incomplete()[:130].copy()
    em = F.ExpectationMaximization(net, device=0)
    counts, value = em.estep_flat(data)
    side = torch.cuda.Stream()
    d_data = torch.from_numpy(data).to("cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_c = torch.full((em.info()["cells"],), -1.0, dtype=torch.float64, device="cuda")
        d_v = torch.full((130, 2), -1.0, dtype=torch.float64, device="cuda")
        em.estep_device(d_data.data_ptr(), 130, d_c.data_ptr(), d_v.data_ptr(), stream_ptr=side.cuda_stream)
    side.synchronize()
    assert d_c.cpu().numpy().tobytes() == counts.tobytes() and d_v.cpu().numpy().tobytes() == value.tobytes()
    bad = data.copy()
    bad[3, 4] = 100
    d_bad = torch.from_numpy(bad).to("cuda")
    with pytest.raises(F.FastBNError, match="case 3.*node 4") as e:
        em.estep_device(d_bad.data_ptr(), 130, d_c.data_ptr(), d_v.data_ptr(), stream_ptr=side.cuda_stream)
    assert e.value.code == -1
    side.synchronize()
    assert em.estep_flat(data)[0].tobytes() == counts.tobytes()
    em.close()


def test_munin_like_global_accumulator(munin_fixture):
    """1041 variables, 25,061 cells: past the workgroup's share of the LDS, so each wave accumulates in its
    private global row.  96 rows (0 / 52 / 208 / 520 observed) and 70 complete ones."""
    net = F.Network(munin_fixture["xml"])
    ev = np.concatenate([F.load_libsvm(munin_fixture[k], net.num_nodes)[0] for k in ("libsvm", "extra_libsvm")])
    host = F.ExpectationMaximization(net, device=-1)
    dev = F.ExpectationMaximization(net, device=0)
    assert dev.info() == host.info() and dev.info()["cells"] * 8 > 160 * 1024 // 8
    b = bound(host)
    assert dev.debug_posteriors(ev[:5]).tobytes() == host.debug_posteriors(ev[:5]).tobytes()
    want, hv = host.estep_flat(ev)
    for groups in (1, 0):
        dev.set_tuning(max_workgroups=groups)
        c, v = dev.estep_flat(ev)
        assert v.tobytes() == hv.tobytes()
        assert ((want == 0) == (c == 0)).all() and (np.abs(c - want) <= (b + len(ev) * U) * want).all()
        assert dev.estep_flat(ev)[0].tobytes() == c.tobytes()
    full = net.forward_sample(70, 3).T.astype(np.int8)
    cf, _ = dev.estep_flat(full)
    assert cf.tobytes() == host.estep_flat(full)[0].tobytes() and cf.sum() == 70 * net.num_nodes
    dev.close()
