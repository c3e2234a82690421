"""EPIS-BN on the device (lbp.hip's lambda rows, then epis.hip's sample_epis_kernel, behind EPISBN).

The device is held to the host twin bit for bit -- values, mantissas, exponents, lambda rows,
marginals, labels, ess, LBP iterations and residual; log_evidence to 1e-15 relative, the two `log`
implementations differ -- and the host twin to the yardsticks of test_epis_host.py.  Shapes are the
smallest at which the kernel can go wrong: one lane, one exact chunk, two chunks and a two-lane
tail, domains above 4 states (the d loop and every cutoff class), a 1-state node, and both homes of
the lambda row (LDS, global memory)."""
import functools
import gzip
import os
import tempfile

import numpy as np
import pytest
from conftest import SYNTH_NETS
from test_epis_host import alarm, alarm_cases, bits, check_disconnected, check_zero_variance, forest, forest_cases

import fastbn_amd as F

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def bigdom():
    with gzip.open(os.path.join(SYNTH_NETS, "bigdom.xml.gz"), "rb") as f, \
            tempfile.NamedTemporaryFile("wb", suffix=".xml") as g:
        g.write(f.read())
        g.flush()
        net = F.Network(g.name)
    return net, np.load(os.path.join(SYNTH_NETS, "bigdom.ev.npy"))[[0, 17, 33, 47]]


def forest_workload():
    dims, parents, counts, _ = forest()
    return F.Network.from_counts(dims, parents, counts), forest_cases()


WORKLOADS = {"alarm": lambda: (alarm()[0], alarm_cases()[0][:64]), "alarm16": lambda: (alarm()[0], alarm_cases()[0][:16]),
             "bigdom": bigdom, "forest": forest_workload}


@functools.lru_cache(maxsize=None)
def host_results(key, S, eps, iters):
    """(debug samples, labels, marginals, stats) of the host twin, computed once per workload."""
    net, ev = WORKLOADS[key]()
    h = F.EPISBN(net, S, iterations=iters, eps=eps, seed=5, device=-1)
    lab, marg = h.infer(ev, case_offset=3)
    return h.debug_samples(ev, case_offset=3), lab, marg, h.stats


def check_device(key, S, eps, iters=6, lds_bytes_max=0, path=None):
    net, ev = WORKLOADS[key]()
    dev = F.EPISBN(net, S, iterations=iters, eps=eps, seed=5, device=0)
    dev.set_tuning(lds_bytes_max)
    if path is not None:
        assert dev.info()["path"] == path
    (val, m, e, lam), lab, marg, (le, ess, used, res) = host_results(key, S, eps, iters)
    dval, dm, de, dlam = dev.debug_samples(ev, case_offset=3)
    np.testing.assert_array_equal(bits(dlam), bits(lam))
    np.testing.assert_array_equal(dval, val)
    np.testing.assert_array_equal(bits(dm), bits(m))
    np.testing.assert_array_equal(de, e)
    dlab, dmarg = dev.infer(ev, case_offset=3)
    np.testing.assert_array_equal(dlab, lab)
    np.testing.assert_array_equal(bits(dmarg), bits(marg))
    np.testing.assert_array_equal(bits(dev.stats[1]), bits(ess))
    np.testing.assert_array_equal(dev.stats[2], used)
    np.testing.assert_array_equal(bits(dev.stats[3]), bits(res))
    assert (np.abs(dev.stats[0] - le) <= 1e-15 * np.abs(le)).all()
    lbp_ms, sample_ms = dev.last_kernel_ms()
    assert sample_ms > 0.0 and (lbp_ms > 0.0) == (iters > 0)
    dev.close()
    return marg


@pytest.mark.parametrize("eps", [0.0, None])
@pytest.mark.parametrize("S", [1, 64, 130])
def test_alarm_equals_host_twin(S, eps):
    check_device("alarm", S, eps, path=0)


@pytest.mark.parametrize("eps", [0.0, None])
def test_bigdom_equals_host_twin(eps):
    """120 variables of 2 to 21 states: the d loop beyond 4 states and all three default cutoffs."""
    net, _ = bigdom()
    assert net.dims.max() == 21 and ((net.dims >= 5) & (net.dims <= 8)).any() and (net.dims < 5).any()
    check_device("bigdom", 70, eps)


@pytest.mark.parametrize("eps", [0.0, None])
def test_forest_equals_host_twin(eps):
    check_device("forest", 130, eps, iters=8)


def test_no_prepropagation_equals_host_twin():
    marg = check_device("alarm16", 70, 0.0, iters=0)
    net, ev = WORKLOADS["alarm16"]()
    lval = F.LikelihoodWeighting(net, 70, seed=5, device=0).debug_samples(ev, case_offset=3)[0]
    np.testing.assert_array_equal(host_results("alarm16", 70, 0.0, 0)[0][0], lval)
    assert np.isfinite(marg).all()


@pytest.mark.parametrize("budget,path", [("default", 0), ("forced", 1), ("fits", 0), ("one short", 1)])
def test_lambda_placement(budget, path):
    net, _ = alarm()
    need = 37 * 64 + 8 * int(net.dims.sum())  # the values, then the lambda row
    lds_bytes_max = {"default": 0, "forced": -1, "fits": need, "one short": need - 1}[budget]
    check_device("alarm16", 130, None, lds_bytes_max=lds_bytes_max, path=path)


def test_device_buffers_and_splits():
    import torch
    net, _ = alarm()
    ev = alarm_cases()[0][:37].copy()
    ep = F.EPISBN(net, 100, iterations=6, seed=9, device=0)
    lab, marg = ep.infer(ev)
    st = np.stack([np.asarray(s, np.float64) for s in ep.stats], axis=1)
    SD = marg.shape[1]
    stream = torch.cuda.current_stream().cuda_stream
    d_ev = torch.from_numpy(ev).to("cuda")
    for _ in range(2):  # a second run on the same handle equals the first
        d_lab = torch.full((37,), -7, dtype=torch.int32, device="cuda")
        d_marg = torch.full((37, SD), -1.0, dtype=torch.float64, device="cuda")
        d_st = torch.full((37, 4), -1.0, dtype=torch.float64, device="cuda")
        ep.run_device(d_ev.data_ptr(), 37, d_lab.data_ptr(), d_marg.data_ptr(), d_st.data_ptr(), stream_ptr=stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d_lab.cpu().numpy(), lab)
        np.testing.assert_array_equal(bits(d_marg.cpu().numpy()), bits(marg))
        np.testing.assert_array_equal(bits(d_st.cpu().numpy()), bits(st))
    # labels only (no marginals, no stats buffer)
    d_lab = torch.full((37,), -7, dtype=torch.int32, device="cuda")
    ep.run_device(d_ev.data_ptr(), 37, d_lab.data_ptr(), stream_ptr=stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_lab.cpu().numpy(), lab)
    # a case_offset split over two calls equals one call
    d_lab.fill_(-7)
    d_marg.fill_(-1.0)
    d_st.fill_(-1.0)
    ep.run_device(d_ev.data_ptr(), 20, d_lab.data_ptr(), d_marg.data_ptr(), d_st.data_ptr(), stream_ptr=stream)
    ep.run_device(d_ev[20:].data_ptr(), 17, d_lab[20:].data_ptr(), d_marg[20:].data_ptr(), d_st[20:].data_ptr(),
                  case_offset=20, stream_ptr=stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_lab.cpu().numpy(), lab)
    np.testing.assert_array_equal(bits(d_marg.cpu().numpy()), bits(marg))
    np.testing.assert_array_equal(bits(d_st.cpu().numpy()), bits(st))
    # a bad code in a device buffer is refused before anything is launched; the handle stays usable
    bad = ev.copy()
    bad[3, 4] = 100
    d_bad = torch.from_numpy(bad).to("cuda")
    d_lab.fill_(-7)
    with pytest.raises(F.FastBNError, match="case 3.*node 4") as e:
        ep.run_device(d_bad.data_ptr(), 37, d_lab.data_ptr(), stream_ptr=stream)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert (d_lab.cpu().numpy() == -7).all()
    np.testing.assert_array_equal(bits(ep.infer(ev)[1]), bits(marg))


def test_zero_variance_on_the_device():
    check_zero_variance(0)


def test_disconnected_network_on_the_device():
    check_disconnected(0)
