"""Junction-tree kernels on networks built from count maps (Network.from_counts /
fbn_network_create: what parameter learning hands to JunctionTree), against the restatement built
from the same count map (OracleJT.from_counts), which tests/test_jt_counts_host.py holds to exact
enumeration.

The networks of tests/jt_nets.py carry what XMLBIF cannot express: counts near 1e6 and 1e12, unseen
parent configurations (uniform rows), a 1-state node, parent lists in descending order, and a wide
variable of 4, 32, 33 or 127 states -- 32 states in a clique of 256 entries is the specialized
kernel's last eligible plan, 33 its first ineligible one (the evidence bit words), 127 the most a
network takes.  70 cases: one full block and a ragged one.  Exact order: bit-identical; fast order:
labels equal, marginals within 1e-12; no block may go to the fixup pass (the denominators stay above
2^-45), so the values are each kernel's own."""
import functools

import numpy as np
import pytest
from types import SimpleNamespace

import fastbn_amd as F
import jt_nets as J
import oracle as O
from test_gpu_jt_fast import TOL

pytestmark = pytest.mark.gpu
VARIANTS = sorted(J.COUNTS_VARIANTS)
ELIGIBLE = {"small": 1, "dom32": 1, "dom33": 0, "dom127": 0}
# (kernel variant, exact order): the interpreters (0 - 2) have the exact order only, the tiled kernel
# (5) the fast order only; 3 is left out where the plan is not eligible
KERNELS = [(0, True), (1, True), (2, True), (3, True), (4, True), (3, None), (4, None), (5, None)]


@functools.lru_cache(maxsize=None)
def _setup(variant):
    net = J.counts_net(J.COUNTS_SEED, variant)
    s = SimpleNamespace(net=net, ev=J.counts_gpu_cases(net))
    s.jt = F.JunctionTree(F.Network.from_counts(net.dims, net.parents, net.counts), device=0)
    s.lab, s.marg = O.OracleJT.from_counts(net.dims, net.parents, net.counts).infer(s.ev)
    return s


@pytest.fixture(params=VARIANTS)
def plan(request):
    s = _setup(request.param)
    yield s
    s.jt.set_variant(-1)
    s.jt.set_exact(None)


def _check(s, lab, marg, exact):
    np.testing.assert_array_equal(lab, s.lab)
    if exact:
        np.testing.assert_array_equal(marg, s.marg)
    else:
        np.testing.assert_allclose(marg, s.marg, rtol=TOL, atol=1e-300)


def test_cases_and_eligibility(plan):
    net, ev = plan.net, plan.ev
    assert ev.shape == (70, len(net.dims))
    assert plan.jt.info["specialized_eligible"] == ELIGIBLE[net.variant]
    assert plan.jt.info["streamed_eligible"] == 1 and plan.jt.info["tiled_eligible"] == 1
    assert (ev[:, J.WIDE] == net.dims[J.WIDE] - 1).any() and (ev[:, J.ONE_STATE] == 0).any()
    # no query posterior of these cases is a near-tie, which the fast order would hand to the fixup pass
    top = np.sort(plan.marg[:, :net.dims[0]], axis=1)
    assert ((top[:, -1] - top[:, -2]) > 1e-9 * top[:, -1]).all()


@pytest.mark.parametrize("variant,exact", KERNELS)
def test_every_kernel_vs_restatement(plan, variant, exact):
    jt = plan.jt
    if variant == 3 and not ELIGIBLE[plan.net.variant]:
        with pytest.raises(F.FastBNError, match="not eligible for the specialized kernel"):
            jt.set_variant(3)
        return
    jt.set_variant(variant)
    jt.set_exact(exact)
    lab, marg = jt.infer(plan.ev)
    assert jt.refresh_info()["variant"] == variant
    if variant >= 3:
        assert jt.debug_flagged_blocks() == 0  # the kernel's own values
    _check(plan, lab, marg, exact)
    off = np.concatenate([[0], np.cumsum(plan.net.dims)])
    one = marg[:, off[J.ONE_STATE]]
    assert np.all(np.where(plan.ev[:, J.ONE_STATE] == 0, one == 0.0, np.abs(one - 1.0) <= TOL))  # the 1-state node


@pytest.mark.parametrize("exact", [None, True])
def test_auto_mode_picks_a_working_kernel(plan, exact):
    jt = plan.jt
    jt.set_variant(-1)
    jt.set_exact(exact)
    lab, marg = jt.infer(plan.ev)
    picked = jt.refresh_info()["variant"]
    assert picked == (3 if ELIGIBLE[plan.net.variant] else (4 if exact else 5))
    assert jt.debug_flagged_blocks() == 0
    _check(plan, lab, marg, exact)


@pytest.mark.parametrize("variant,exact", KERNELS)
def test_observed_query_gets_label_zero(variant, exact):
    """A case that observes the query itself gets label 0, the ArgMax of its row of zeros (the
    restatement's answer, and the sampling engines').  Every kernel has to write it: the label
    buffer starts at -7.  (The conflict blocks of test_gpu_jt_range.py observe the query too.)"""
    import torch
    s = _setup("small")
    ev = s.ev.copy()
    ev[::2, 0] = np.arange(35) % s.net.dims[0]
    olab, omarg = O.OracleJT.from_counts(s.net.dims, s.net.parents, s.net.counts).infer(ev)
    assert (olab[::2] == 0).all() and (olab[1::2] != 0).any()
    n, SD, dev = len(ev), s.jt.info["sum_dom"], torch.device("cuda", 0)
    d_ev = torch.from_numpy(ev).to(dev)
    d_lab = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_marg = torch.full((n, SD), float("nan"), dtype=torch.float64, device=dev)
    s.jt.set_variant(variant)
    s.jt.set_exact(exact)
    try:
        s.jt.run_device(d_ev.data_ptr(), n, d_lab.data_ptr(), d_marg.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
    finally:
        s.jt.set_variant(-1)
        s.jt.set_exact(None)
    np.testing.assert_array_equal(d_lab.cpu().numpy(), olab)
    marg = d_marg.cpu().numpy()
    if exact:
        np.testing.assert_array_equal(marg, omarg)
    else:
        np.testing.assert_allclose(marg, omarg, rtol=TOL, atol=1e-300)


def test_evidence_past_the_domain_is_refused():
    s = _setup("dom127")
    ev = s.ev.copy()
    ev[69, J.WIDE] = 127
    with pytest.raises(F.FastBNError, match=r"case 69: evidence 127 for node 5 \(domain 127\)"):
        s.jt.infer(ev)
    ev = s.ev.copy()
    ev[3, J.ONE_STATE] = 1
    with pytest.raises(F.FastBNError, match=r"case 3: evidence 1 for node 3 \(domain 1\)"):
        s.jt.infer(ev)
    lab, marg = s.jt.infer(s.ev)  # the plan stays usable
    _check(s, lab, marg, False)
