"""The denominator range guard of the junction-tree kernels, tripped.

Every kernel forms x / den as Markstein's two-fma division and checks den against [2^-600, 2^600]
(the tiled kernel its totals against [2^-900, 2^900]); a 64-case block outside is flagged and
recomputed by the IEEE-division interpreter.  The conflict networks of tests/jt_nets.py reach
denominators of 2^-617 .. 2^-870 (the "tripping" block) and 2^-926 (the "deep" block) with every
marginal a normal double and every divided entry above 2^-940; tests/test_jt_counts_host.py asserts
those figures from the restatement and holds the restatement to exact rational posteriors.

Cases 0..63 are benign (every denominator above 2^-100, marginals down to 2^-867), cases 64..127
trip the guard.  Exact order: every variant equals the restatement bit for bit, and variants 3 and 4
flag exactly one block -- the exact order uses the restatement's denominators, so the tripping block
must be flagged and the benign block must keep the kernel's own result.  Fast order: labels equal,
marginals within 1e-12, at most one block flagged.  Both plans are eligible for the specialized (3),
streamed (4) and tiled (5) kernels."""
import functools

import numpy as np
import pytest
from types import SimpleNamespace

import fastbn_amd as F
import jt_nets as J
import oracle as O
from test_gpu_jt_fast import TOL

pytestmark = pytest.mark.gpu
FORMS = sorted(J.CONFLICT_FORMS)


@functools.lru_cache(maxsize=None)
def _setup(form, tmp):
    net = J.conflict_net(*J.CONFLICT_FORMS[form])
    if net.xml is not None:  # the XMLBIF form goes through the loaders
        path = tmp / "conflict.xml"
        path.write_text(net.xml)
        pn, oj = F.Network(str(path)), O.OracleJT(str(path))
    else:
        pn = F.Network.from_counts(net.dims, net.parents, net.counts)
        oj = O.OracleJT.from_counts(net.dims, net.parents, net.counts)
    blocks = J.conflict_blocks(net)
    ev = J.conflict_cases(net, blocks.benign + blocks.tripping)
    deep = J.conflict_cases(net, blocks.deep)
    s = SimpleNamespace(net=net, jt=F.JunctionTree(pn, device=0), ev=ev, deep=deep)
    s.lab, s.marg = oj.infer(ev)
    s.deep_lab, s.deep_marg = oj.infer(deep)
    return s


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("conflict")


@pytest.fixture(params=FORMS)
def plan(request, tmp):
    s = _setup(request.param, tmp)
    yield s
    s.jt.set_variant(-1)
    s.jt.set_exact(None)


def _close(marg, ref):
    np.testing.assert_allclose(marg, ref, rtol=TOL, atol=1e-300)


def test_plans_are_eligible_for_every_kernel(plan):
    info = plan.jt.info
    assert info["specialized_eligible"] == 1
    assert info["streamed_eligible"] == 1 and info["tiled_eligible"] == 1
    assert plan.ev.shape == (128, 2 + 2 * plan.net.K)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_exact_order_bit_identical_and_one_block_flagged(plan, variant):
    jt = plan.jt
    jt.set_variant(variant)
    jt.set_exact(True)
    lab, marg = jt.infer(plan.ev)
    assert jt.refresh_info()["variant"] == variant
    np.testing.assert_array_equal(lab, plan.lab)
    np.testing.assert_array_equal(marg, plan.marg)
    if variant >= 3:
        assert jt.debug_flagged_blocks() == 1  # the tripping block, and only it


@pytest.mark.parametrize("variant", [3, 4, 5])
def test_fast_order_within_1e12(plan, variant):
    jt = plan.jt
    jt.set_variant(variant)
    jt.set_exact(None)
    lab, marg = jt.infer(plan.ev)
    assert jt.refresh_info()["variant"] == variant
    print("variant %d fast order: %d of 2 blocks flagged" % (variant, jt.debug_flagged_blocks()))
    assert jt.debug_flagged_blocks() <= 1
    np.testing.assert_array_equal(lab, plan.lab)
    _close(marg, plan.marg)


def test_tiled_kernel_deep_block(plan):
    """Denominators near 2^-926: past the tiled kernel's own range [2^-900, 2^900] too."""
    jt = plan.jt
    jt.set_variant(5)
    jt.set_exact(None)
    lab, marg = jt.infer(plan.deep)
    assert jt.refresh_info()["variant"] == 5
    print("variant 5, deep block: %d of 1 block flagged" % jt.debug_flagged_blocks())
    np.testing.assert_array_equal(lab, plan.deep_lab)
    _close(marg, plan.deep_marg)


@pytest.mark.parametrize("variant,exact", [(3, True), (4, True), (3, None), (5, None)])
def test_flag_follows_the_block(plan, variant, exact):
    """The two blocks swapped: the results follow the cases, so the flag lands on the block index
    of the tripping cases, whichever it is."""
    jt = plan.jt
    jt.set_variant(variant)
    jt.set_exact(exact)
    swap = np.concatenate([np.arange(64, 128), np.arange(64)])
    lab, marg = jt.infer(plan.ev[swap])
    np.testing.assert_array_equal(lab, plan.lab[swap])
    if exact:
        np.testing.assert_array_equal(marg, plan.marg[swap])
        assert jt.debug_flagged_blocks() == 1
    else:
        _close(marg, plan.marg[swap])
        assert jt.debug_flagged_blocks() <= 1


@pytest.mark.parametrize("variant,exact", [(0, True), (3, True), (4, True), (3, None), (5, None)])
@pytest.mark.parametrize("n", [65, 128])
def test_device_buffers_variable_major_and_ragged_block(tmp, variant, exact, n):
    """run_device on device buffers, variable-major marginals; n = 65: a ragged second block that
    holds one tripping case.  (The counts form: its variable-major kernels are prebuilt.)"""
    import torch
    s = _setup("counts", tmp)
    jt, SD = s.jt, s.jt.info["sum_dom"]
    dev = torch.device("cuda", 0)
    d_ev = torch.from_numpy(np.ascontiguousarray(s.ev[:n])).to(dev)
    d_lab = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_marg = torch.full((n * SD,), float("nan"), dtype=torch.float64, device=dev)
    jt.set_variant(variant)
    jt.set_exact(exact)
    jt.set_output_layout(1)
    try:
        jt.run_device(d_ev.data_ptr(), n, d_lab.data_ptr(), d_marg.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        flagged = jt.debug_flagged_blocks()
        assert jt.refresh_info()["variant"] == variant
    finally:
        jt.set_output_layout(0)
        jt.set_variant(-1)
        jt.set_exact(None)
    lab, marg = d_lab.cpu().numpy(), d_marg.view(SD, n).t().cpu().numpy()
    np.testing.assert_array_equal(lab, s.lab[:n])
    if exact:
        np.testing.assert_array_equal(marg, s.marg[:n])
        assert variant < 3 or flagged == 1
    else:
        _close(marg, s.marg[:n])
        assert flagged <= 1
