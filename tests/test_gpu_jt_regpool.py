"""Register pool of the plan-specialized kernel (jt_gen_place.cpp JtGenPlace, FBN_JT_REG_POOL):
message entries parked in registers the small cliques leave unused, and the child visit order the
placement picks.  Where a message lives and when a subtree is visited change no arithmetic: the
build with the pool agrees bitwise with the FBN_JT_REG_POOL=0 build (every message in LDS / global
rows, plan order) in both output layouts, and with the oracle as the fast order always does (labels
equal, marginals within 1e-12 relative).  The pool is the default of the variable-major kernel
(bench.py's); the case-major kernel takes it on request (FBN_JT_REG_POOL=256, the same cap), so the
"on" build here is the default in the one layout and that request in the other.  Shapes: one lane,
a full block, a one-lane second block, and 256 * 64 + 1 cases on one wave per CU -- a grid of 256
waves for 257 blocks, so wave 0 runs a second loop iteration with one active lane, the smallest
shape where a parked value left over from the previous block could be read."""
import os

import numpy as np
import pytest
import torch
from conftest import GOLD

import fastbn_amd as F
import oracle as O
from fastbn_amd import synth

pytestmark = pytest.mark.gpu
XML = os.path.join(GOLD, "alarm", "alarm.xml")
NBIG = 256 * 64 + 1


def _make(env):
    """A plan with both layouts' fast kernels loaded under `env` (the generator reads its options
    when a kernel is first needed)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("FBN_JT_REG_POOL", raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        jt = F.JunctionTree(F.Network(XML), device=0)
        jt.set_exact(None)
        jt.set_variant(3)
        ev = np.full((1, jt.network.num_nodes), -1, np.int8)
        place = {}
        for layout in (0, 1):
            _run(jt, ev, layout)
            place[layout] = jt.refresh_info()
    return jt, place


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


@pytest.fixture(scope="module")
def builds():
    on, place_on = _make({"FBN_JT_REG_POOL": "256"})
    off, place_off = _make({"FBN_JT_REG_POOL": "0"})
    return on, off, place_on, place_off


@pytest.fixture(scope="module")
def cases():
    """Evidence of the largest shape (the smaller ones are its prefixes) and the oracle's results on
    the cases the tests compare: the first 65, the last 65 and 256 spread over the batch."""
    ev = synth.evidence_cases(synth.read_xmlbif(XML), NBIG, 7, seed=17)
    pick = np.unique(np.concatenate([np.arange(65), np.arange(NBIG - 65, NBIG),
                                     np.linspace(65, NBIG - 66, 256).astype(np.int64)]))
    olab, omarg = O.OracleJT(XML).infer(ev[pick])
    return ev, pick, olab, omarg


def _check(lab, marg, idx, cases):
    """Results `lab`, `marg` of the cases `idx` (indices into the evidence) against the oracle."""
    _, pick, olab, omarg = cases
    pos = np.searchsorted(pick, idx)
    assert np.array_equal(pick[pos], idx)
    np.testing.assert_array_equal(lab, olab[pos])
    np.testing.assert_allclose(marg, omarg[pos], rtol=1e-12, atol=1e-300)


def test_pool_is_the_variable_major_default(builds):
    _, _, place_on, place_off = builds
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("FBN_JT_REG_POOL", raising=False)
        jt = F.JunctionTree(F.Network(XML), device=-1)
        jt.set_output_layout(1)
        default = jt.refresh_info()
        assert {k: v for k, v in default.items() if k.startswith("place_")} == \
               {k: v for k, v in place_on[1].items() if k.startswith("place_")}
        mp.setenv("FBN_JT_REG_POOL", "256")
        on_path = jt.kernel_cache_path()
        mp.delenv("FBN_JT_REG_POOL")
        assert jt.kernel_cache_path() == on_path  # the same source: the same code object
    for layout in (0, 1):
        assert place_on[layout]["place_rows_reg_collect"] + place_on[layout]["place_rows_reg_distribute"] > 0
        assert place_off[layout]["place_rows_reg_collect"] + place_off[layout]["place_rows_reg_distribute"] == 0
        assert place_on[layout]["place_rows_workspace"] < place_off[layout]["place_rows_workspace"]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n", [1, 64, 65])
def test_regpool_small_shapes(builds, cases, layout, n):
    on, off = builds[:2]
    ev = cases[0][:n]
    lab, marg = _run(on, ev, layout)
    assert on.refresh_info()["variant"] == 3 and on.debug_flagged_blocks() == 0
    lab0, marg0 = _run(off, ev, layout)
    np.testing.assert_array_equal(lab, lab0)
    assert np.array_equal(marg.view(np.int64), marg0.view(np.int64))  # bitwise
    _check(lab, marg, np.arange(n), cases)


@pytest.mark.parametrize("layout", [0, 1])
def test_regpool_second_block_of_a_wave(builds, cases, layout):
    on, off = builds[:2]
    ev, pick = cases[0], cases[1]
    try:
        for jt in (on, off):
            jt.set_waves_per_cu(1)
        lab, marg = _run(on, ev, layout)
        assert on.debug_flagged_blocks() == 0
        lab0, marg0 = _run(off, ev, layout)
    finally:
        for jt in (on, off):
            jt.set_waves_per_cu(0)
    np.testing.assert_array_equal(lab, lab0)
    assert np.array_equal(marg.view(np.int64), marg0.view(np.int64))  # bitwise
    _check(lab[pick], marg[pick], pick, cases)


def test_regpool_forced_fixup(builds, cases):
    """The exact pass overwrites flagged blocks whatever the placement."""
    on = builds[0]
    ev = cases[0][:65]
    on.debug_force_fixup(True)
    try:
        lab, marg = _run(on, ev, 0)
    finally:
        on.debug_force_fixup(False)
    _check(lab, marg, np.arange(65), cases)
