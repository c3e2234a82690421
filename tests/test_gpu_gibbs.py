"""Gibbs sampling on the device (gibbs.hip's kernels behind GibbsSampling).

The device is held to the host twin bit for bit -- labels, marginals, the chains' last states, the
conditionals -- and the host twin to enumeration by test_gibbs_host.py.  Shapes are the smallest at which
the kernel can go wrong: one lane, a tail lane short of a chunk, an exact chunk, one lane into a second
chunk, three chunks with a tail; a 1-state node, a 127-state node and a six-parent node; no counted sweep
but one; both homes of the accumulators, the parent-configuration cache on and off, and grids smaller
than the units (a workgroup runs several units on the same LDS)."""
import functools

import numpy as np
import prob_nets as PN
import pytest
from test_epis_host import alarm, alarm_cases, bits
from test_gibbs_host import BURN_IN, CHAINS, SWEEPS, benign_reference, check_marginal_bound

import fastbn_amd as F

pytestmark = pytest.mark.gpu


def from_cpts(make, ncases):
    dims, parents, cpts = make()
    return F.Network.from_cpts(dims, parents, cpts), PN.cases(dims, ncases, 11)


WORKLOADS = {"small": lambda: from_cpts(PN.small, 5), "shapes": lambda: from_cpts(PN.shapes, 5),
             "alarm": lambda: (alarm()[0], alarm_cases()[0][:8])}


@functools.lru_cache(maxsize=None)
def host_results(key, chains, burn_in, sweeps):
    net, ev = WORKLOADS[key]()
    return F.GibbsSampling(net, chains, sweeps, burn_in, seed=5, device=-1).infer(ev, states=True, case_offset=3)


@pytest.mark.parametrize("lds_bytes_max,pc_cache,max_workgroups", [(0, 1, 3), (0, 0, 1), (-1, 1, 1), (-1, 0, 3)])
@pytest.mark.parametrize("burn_in,sweeps", [(0, 1), (3, 5)])
@pytest.mark.parametrize("chains", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("key", list(WORKLOADS))
def test_equals_host_twin(key, chains, burn_in, sweeps, lds_bytes_max, pc_cache, max_workgroups):
    net, ev = WORKLOADS[key]()
    dev = F.GibbsSampling(net, chains, sweeps, burn_in, seed=5, device=0)
    dev.set_tuning(lds_bytes_max, max_workgroups, pc_cache)
    info = dev.info(len(ev))
    assert (info["path"], info["pc_cache"], info["grid"]) == (int(lds_bytes_max < 0), pc_cache, max_workgroups)
    lab, marg, st = host_results(key, chains, burn_in, sweeps)
    dlab, dmarg, dst = dev.infer(ev, states=True, case_offset=3)
    np.testing.assert_array_equal(dlab, lab)
    np.testing.assert_array_equal(bits(dmarg), bits(marg))
    np.testing.assert_array_equal(dst, st)
    assert dev.last_kernel_ms() > 0.0
    dev.close()


@pytest.mark.parametrize("pc_cache", [0, 1])
def test_conditionals_equal_host_twin(pc_cache):
    dims, parents, cpts = PN.shapes()
    net = F.Network.from_cpts(dims, parents, cpts)
    xs = (np.random.default_rng(2).integers(0, 1 << 30, (70, len(dims))) % dims).astype(np.int8)
    dev = F.GibbsSampling(net, device=0)
    dev.set_tuning(pc_cache=pc_cache)
    np.testing.assert_array_equal(bits(dev.conditionals(xs)), bits(F.GibbsSampling(net, device=-1).conditionals(xs)))


def test_run_device_equals_infer():
    import torch
    net, ev = WORKLOADS["alarm"]()
    g = F.GibbsSampling(net, chains=70, sweeps=5, burn_in=3, seed=9, device=0)
    lab, marg, st = g.infer(ev, states=True)
    stream = torch.cuda.current_stream().cuda_stream
    d_ev = torch.from_numpy(ev.copy()).to("cuda")
    d_lab = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    d_marg = torch.full(marg.shape, -1.0, dtype=torch.float64, device="cuda")
    d_st = torch.full(st.shape, -1, dtype=torch.int8, device="cuda")
    # a case_offset split over two calls into caller buffers equals one infer call
    g.run_device(d_ev.data_ptr(), 3, d_lab.data_ptr(), d_marg.data_ptr(), d_st.data_ptr(), stream_ptr=stream)
    g.run_device(d_ev[3:].data_ptr(), 5, d_lab[3:].data_ptr(), d_marg[3:].data_ptr(), d_st[3:].data_ptr(), case_offset=3,
                 stream_ptr=stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_lab.cpu().numpy(), lab)
    np.testing.assert_array_equal(bits(d_marg.cpu().numpy()), bits(marg))
    np.testing.assert_array_equal(d_st.cpu().numpy(), st)
    # labels only
    d_lab.fill_(-7)
    g.run_device(d_ev.data_ptr(), 8, d_lab.data_ptr(), stream_ptr=stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_lab.cpu().numpy(), lab)


def test_marginals_against_enumeration_on_device():
    (dims, parents, cpts), ev, p = benign_reference()
    g = F.GibbsSampling(F.Network.from_cpts(dims, parents, cpts), CHAINS, SWEEPS, BURN_IN, seed=0, device=0)
    check_marginal_bound(dims, ev, g.infer(ev)[1], p)
