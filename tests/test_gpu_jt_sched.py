"""Load pipeline of the plan-specialized kernel (jt_gen_emit.cpp IvLoads, Levels, FBN_JT_SCHED): where
the scalar loads of the initial potentials stand -- the first batch of a fused product behind the
previous fused product, batch b + 1 behind batch b's first use, as volatile vector loads -- and the
product trees and Collect bin sums written level by level in pairs with named temporaries.  No
operand and no association changes, so the build with it agrees bitwise with the FBN_JT_SCHED=0
build (both with the register pool on: the default of the variable-major layout, FBN_JT_REG_POOL=256
in the case-major one), and with the oracle as the fast order always does (labels equal, marginals
within 1e-12 relative, no flagged block).  Shapes as in tests/test_gpu_jt_regpool.py: one lane, a
full block, a one-lane second block, and 256 * 64 + 1 cases on one wave per CU, where wave 0 runs a
second loop iteration -- the smallest shape where a batch requested in the previous block could be
read.  Evidence beyond that file's 7 observed variables, because the indicator factors multiply the
potentials the pipeline loads: none observed, all 37 observed (every marginal row zero, every label
0), 20 observed.  And one other eligible plan (prebuild.synth_small_xml), whose cliques have other
sizes and batch tails."""
import os

import numpy as np
import pytest
import torch
from conftest import GOLD

import fastbn_amd as F
import oracle as O
from fastbn_amd import prebuild, synth

pytestmark = pytest.mark.gpu
XML = os.path.join(GOLD, "alarm", "alarm.xml")
NBIG = 256 * 64 + 1
POOL = {0: {"FBN_JT_REG_POOL": "256"}, 1: {}}  # the pool on, by layout


def _run(jt, ev, layout):
    n = ev.shape[0]
    dev = torch.device("cuda", 0)
    jt.set_output_layout(layout)
    d_ev = torch.from_numpy(np.ascontiguousarray(ev)).to(dev)
    d_lab = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_marg = torch.full((n * jt.info["sum_dom"],), float("nan"), dtype=torch.float64, device=dev)
    jt.run_device(d_ev.data_ptr(), n, d_lab.data_ptr(), d_marg.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    marg = d_marg.view(jt.info["sum_dom"], n).t() if layout == 1 else d_marg.view(n, jt.info["sum_dom"])
    return d_lab.cpu().numpy(), marg.cpu().numpy()


def _make(xml, layout, sched):
    """A plan whose fast kernel of `layout` is generated with the pool on and FBN_JT_SCHED=`sched`
    (None: unset); the generator reads its options when the kernel is first needed."""
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("FBN_JT_REG_POOL", raising=False)
        mp.delenv("FBN_JT_SCHED", raising=False)
        for k, v in POOL[layout].items():
            mp.setenv(k, v)
        if sched is not None:
            mp.setenv("FBN_JT_SCHED", sched)
        jt = F.JunctionTree(F.Network(xml), device=0)
        jt.set_exact(None)
        jt.set_variant(3)
        _run(jt, np.full((1, jt.network.num_nodes), -1, np.int8), layout)
        info = jt.refresh_info()
        assert info["variant"] == 3
        assert info["place_rows_reg_collect"] + info["place_rows_reg_distribute"] > 0  # the pool is on
        path = jt.kernel_cache_path()
    return jt, path


@pytest.fixture(scope="module")
def builds():
    """layout -> (new, FBN_JT_SCHED=0)"""
    out = {}
    for layout in (0, 1):
        new, p_new = _make(XML, layout, None)
        old, p_old = _make(XML, layout, "0")
        assert p_new != p_old
        out[layout] = (new, old)
    return out


@pytest.fixture(scope="module")
def cases():
    """Evidence of the largest shape (the smaller ones are its prefixes) and the oracle's results on
    the cases the tests compare: the first 65, the last 65 and 256 spread over the batch."""
    ev = synth.evidence_cases(synth.read_xmlbif(XML), NBIG, 7, seed=17)
    pick = np.unique(np.concatenate([np.arange(65), np.arange(NBIG - 65, NBIG),
                                     np.linspace(65, NBIG - 66, 256).astype(np.int64)]))
    olab, omarg = O.OracleJT(XML).infer(ev[pick])
    return ev, pick, olab, omarg


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.int64), b[1].view(np.int64))  # bitwise


def _check(lab, marg, idx, cases):
    _, pick, olab, omarg = cases
    pos = np.searchsorted(pick, idx)
    assert np.array_equal(pick[pos], idx)
    np.testing.assert_array_equal(lab, olab[pos])
    np.testing.assert_allclose(marg, omarg[pos], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_sched_small_shapes(builds, cases, layout, n):
    new, old = builds[layout]
    ev = cases[0][:n]
    got = _run(new, ev, layout)
    assert new.refresh_info()["variant"] == 3 and new.debug_flagged_blocks() == 0
    _same(got, _run(old, ev, layout))
    _check(got[0], got[1], np.arange(n), cases)


@pytest.mark.parametrize("layout", [0, 1])
def test_sched_second_block_of_a_wave(builds, cases, layout):
    new, old = builds[layout]
    ev, pick = cases[0], cases[1]
    try:
        for jt in (new, old):
            jt.set_waves_per_cu(1)
        got = _run(new, ev, layout)
        assert new.debug_flagged_blocks() == 0
        ref = _run(old, ev, layout)
    finally:
        for jt in (new, old):
            jt.set_waves_per_cu(0)
    _same(got, ref)
    _check(got[0][pick], got[1][pick], pick, cases)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("nobs", [0, 20, 37])
def test_sched_evidence_counts(builds, layout, nobs):
    """65 cases with `nobs` observed variables each (0: one distinct case, repeated; 37: all)."""
    new, old = builds[layout]
    net = synth.read_xmlbif(XML)
    if nobs == 37:  # (evidence_cases never observes the query: whole forward samples)
        ev = np.ascontiguousarray(synth.forward_sample(net, 65, 23).T.astype(np.int8))
    else:
        ev = synth.evidence_cases(net, 65, nobs, seed=23)
    assert ev.shape == (65, 37) and ((ev >= 0).sum(axis=1) == nobs).all()
    got = _run(new, ev, layout)
    assert new.debug_flagged_blocks() == 0  # (sampled values: the evidence has positive probability)
    _same(got, _run(old, ev, layout))
    olab, omarg = O.OracleJT(XML).infer(ev)
    np.testing.assert_array_equal(got[0], olab)
    np.testing.assert_allclose(got[1], omarg, rtol=1e-12, atol=1e-300)
    if nobs == 37:
        assert not got[1].any() and not got[0].any()


def test_sched_forced_fixup(builds, cases):
    """The exact pass overwrites flagged blocks whatever the loads' places."""
    new = builds[1][0]
    ev = cases[0][:65]
    new.debug_force_fixup(True)
    try:
        lab, marg = _run(new, ev, 1)
    finally:
        new.debug_force_fixup(False)
    _check(lab, marg, np.arange(65), cases)


def test_sched_other_plan(tmp_path):
    """The synthetic 60-variable network: 777 cases, variant 3, variable-major (the pool's default)."""
    xml = prebuild.synth_small_xml(str(tmp_path))
    new, p_new = _make(xml, 1, None)
    old, p_old = _make(xml, 1, "0")
    assert p_new != p_old
    ev = synth.evidence_cases(synth.read_xmlbif(xml), 777, 7, seed=29)
    got = _run(new, ev, 1)
    assert new.refresh_info()["variant"] == 3 and new.debug_flagged_blocks() == 0
    _same(got, _run(old, ev, 1))
    olab, omarg = O.OracleJT(xml).infer(ev)
    np.testing.assert_array_equal(got[0], olab)
    np.testing.assert_allclose(got[1], omarg, rtol=1e-12, atol=1e-300)
