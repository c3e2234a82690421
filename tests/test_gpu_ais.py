"""AIS-BN and SIS on the device (ais.hip's sample_ais_kernel behind AISBN / SelfImportanceSampling).

The device is held to the host twin bit for bit -- values, mantissas, exponents, the importance CPT
after the last update, marginals, labels, ess, the first stage's ess / n, the updates applied;
log_evidence to 1e-15 relative, the two `log` implementations differ -- and the host twin to the
restatement and yardsticks of test_ais_host.py.  Shapes are the smallest at which the kernel can go
wrong: one lane, exact chunks, a two-lane tail in every stage, domains above 4 states (the d loop and
every cutoff class), a 1-state node, both homes of the state (LDS, the global workspace) and a grid
smaller than the batch (a workgroup runs several cases and resets its state between them)."""
import functools

import numpy as np
import pytest
from test_ais_host import CLASSES
from test_epis_host import alarm, alarm_cases, bits
from test_gpu_epis import bigdom, forest_workload

import fastbn_amd as F

pytestmark = pytest.mark.gpu

WORKLOADS = {"alarm16": lambda: (alarm()[0], alarm_cases()[0][:16]), "alarm5": lambda: (alarm()[0], alarm_cases()[0][:5]),
             "bigdom": bigdom, "forest": forest_workload}


@functools.lru_cache(maxsize=None)
def host_results(key, method, S, l, m, eps):
    """(debug samples, labels, marginals, stats) of the host twin, computed once per workload."""
    net, ev = WORKLOADS[key]()
    h = CLASSES[method](net, S, max_updates=m, interval=l, eps=eps, seed=5, device=-1)
    lab, marg = h.infer(ev, case_offset=3)
    return h.debug_samples(ev, case_offset=3), lab, marg, h.stats


def check_device(key, method, S, l, m, eps=None, lds_bytes_max=0, max_workgroups=0, path=None, grid=None):
    net, ev = WORKLOADS[key]()
    dev = CLASSES[method](net, S, max_updates=m, interval=l, eps=eps, seed=5, device=0)
    dev.set_tuning(lds_bytes_max, max_workgroups)
    info = dev.info(len(ev))
    if path is not None:
        assert info["path"] == path
    if grid is not None:
        assert info["grid"] == grid
    (val, mm, e, icpt), lab, marg, (le, ess, upd, ess0) = host_results(key, method, S, l, m, eps)
    dval, dm, de, dicpt = dev.debug_samples(ev, case_offset=3)
    np.testing.assert_array_equal(dval, val)
    np.testing.assert_array_equal(bits(dm), bits(mm))
    np.testing.assert_array_equal(de, e)
    np.testing.assert_array_equal(bits(dicpt), bits(icpt))
    dlab, dmarg = dev.infer(ev, case_offset=3)
    np.testing.assert_array_equal(dlab, lab)
    np.testing.assert_array_equal(bits(dmarg), bits(marg))
    np.testing.assert_array_equal(bits(dev.stats[1]), bits(ess))
    np.testing.assert_array_equal(dev.stats[2], upd)
    np.testing.assert_array_equal(bits(dev.stats[3]), bits(ess0))
    assert (np.abs(dev.stats[0] - le) <= 1e-15 * np.abs(le)).all()
    assert dev.last_kernel_ms() > 0.0
    dev.close()
    return icpt


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("S,l,m", [(1, 1, 1), (64, 64, 2), (130, 70, 2)])
def test_alarm_equals_host_twin(S, l, m, method):
    """One lane; exact chunks; a two-lane tail in every stage (70 = 64 + 6, 130 = 128 + 2; SIS: 70, then 60)."""
    icpt = check_device("alarm16", method, S, l, m, path=0)
    if S == 130:
        assert not np.array_equal(icpt[0], icpt[1])  # something was learned, per case


@pytest.mark.parametrize("method", [0, 1])
def test_bigdom_equals_host_twin(method):
    """120 variables of 2 to 21 states: the d loop beyond 4 states and all three default cutoffs."""
    net, _ = bigdom()
    assert net.dims.max() == 21 and ((net.dims >= 5) & (net.dims <= 8)).any() and (net.dims < 5).any()
    check_device("bigdom", method, 70, 70, 2)


@pytest.mark.parametrize("method", [0, 1])
def test_forest_equals_host_twin(method):
    """Three components, an isolated node and a 1-state node."""
    check_device("forest", method, 130, 40, 2)


@pytest.mark.parametrize("budget,path", [("default", 0), ("forced", 1), ("fits", 0), ("one short", 1)])
def test_state_home(budget, path):
    net, _ = alarm()
    h = F.AISBN(net, 16, 1, 16, device=0)
    info = h.info()
    h.close()
    need = 37 * 64 + 512 + 40 + info["state_bytes"]  # values, weights, 37 flags padded to 8, ICPT and counts
    assert info["lds_bytes"] == need and info["state_bytes"] % 16 == 0 and info["state_bytes"] > 0
    lds_bytes_max = {"default": 0, "forced": -1, "fits": need, "one short": need - 1}[budget]
    check_device("alarm16", 0, 130, 70, 2, lds_bytes_max=lds_bytes_max, path=path, grid=16)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("lds_bytes_max,path", [(0, 0), (-1, 1)])
def test_persistent_loop_resets_per_case(lds_bytes_max, path, method):
    """Two workgroups, five cases: a workgroup runs cases 0, 2, 4 (1, 3) in turn on the same state."""
    check_device("alarm5", method, 130, 70, 2, lds_bytes_max=lds_bytes_max, max_workgroups=2, path=path, grid=2)


def test_device_buffers_and_splits():
    import torch
    net, _ = alarm()
    ev = alarm_cases()[0][:37].copy()
    h = F.AISBN(net, 100, max_updates=2, interval=40, seed=9, device=0)
    lab, marg = h.infer(ev)
    st = np.stack([np.asarray(s, np.float64) for s in h.stats], axis=1)
    SD = marg.shape[1]
    stream = torch.cuda.current_stream().cuda_stream
    d_ev = torch.from_numpy(ev).to("cuda")
    for _ in range(2):  # a second run on the same handle equals the first
        d_lab = torch.full((37,), -7, dtype=torch.int32, device="cuda")
        d_marg = torch.full((37, SD), -1.0, dtype=torch.float64, device="cuda")
        d_st = torch.full((37, 4), -1.0, dtype=torch.float64, device="cuda")
        h.run_device(d_ev.data_ptr(), 37, d_lab.data_ptr(), d_marg.data_ptr(), d_st.data_ptr(), stream_ptr=stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d_lab.cpu().numpy(), lab)
        np.testing.assert_array_equal(bits(d_marg.cpu().numpy()), bits(marg))
        np.testing.assert_array_equal(bits(d_st.cpu().numpy()), bits(st))
    # labels only (no marginals, no stats buffer)
    d_lab = torch.full((37,), -7, dtype=torch.int32, device="cuda")
    h.run_device(d_ev.data_ptr(), 37, d_lab.data_ptr(), stream_ptr=stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_lab.cpu().numpy(), lab)
    # a case_offset split over two calls equals one call
    d_lab.fill_(-7)
    d_marg.fill_(-1.0)
    d_st.fill_(-1.0)
    h.run_device(d_ev.data_ptr(), 20, d_lab.data_ptr(), d_marg.data_ptr(), d_st.data_ptr(), stream_ptr=stream)
    h.run_device(d_ev[20:].data_ptr(), 17, d_lab[20:].data_ptr(), d_marg[20:].data_ptr(), d_st[20:].data_ptr(),
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
        h.run_device(d_bad.data_ptr(), 37, d_lab.data_ptr(), stream_ptr=stream)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert (d_lab.cpu().numpy() == -7).all()
    np.testing.assert_array_equal(bits(h.infer(ev)[1]), bits(marg))
