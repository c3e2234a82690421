"""The two G^2 passes of the bit-sliced CI path (ci_bits_g2.hip) against each other and against the
byte-column histogram kernel (ci_kernels.hip): a batch of at most 16,384 tests takes the four-lane
pass (ci_bits_g2q), a larger one the lane-per-test pass (ci_bits_g2); all three evaluate ci_g2.h's
term, df and decision, so g2, df, p and the decision must be equal bit for bit, with no tolerance."""
import os

import numpy as np
import pytest

import fastbn_amd as F

pytestmark = pytest.mark.gpu

ALPHA = 0.05
QUAD_MAX = 16384  # kG2QuadMax: the largest batch of the four-lane pass
DIMS = np.array([1, 2, 3, 4, 2, 3, 4, 4, 2, 3, 1, 4], np.int32)
NV = len(DIMS)


def _items(d):
    if d == 0:
        return np.array([[x, y] for x in range(NV) for y in range(x + 1, NV)], np.int32)
    return np.array([[x, y, z] for x in range(NV) for y in range(x + 1, NV) for z in range(NV)
                     if z != x and z != y], np.int32)


def _run(ci, items, d, knob):
    os.environ[knob] = "1"
    try:
        return ci.run(np.ascontiguousarray(items), d)
    finally:
        del os.environ[knob]


@pytest.fixture(scope="module", params=[33, 5000])
def paths(request):
    """Per d: the distinct items (66 pairs, 660 triples), the batch tiled to one test past the four-lane
    limit, and (g2, df, p, indep) of the four-lane pass on its first 16,384 tests, of the
    lane-per-test pass on all 16,385, and of the byte-column kernel on the distinct items."""
    ns = request.param
    rng = np.random.default_rng(ns)
    cols = np.stack([rng.integers(0, d, ns) for d in DIMS]).astype(np.uint8)
    cols[5] = (cols[4] + cols[5]) % 3  # some dependence
    ci = F.IndependenceTest(F.Dataset(columns=cols, dims=DIMS), ALPHA, device=0)
    out = {"ci": ci}
    for d in (0, 1):
        distinct = _items(d)
        tiled = np.tile(distinct, (QUAD_MAX // len(distinct) + 2, 1))[:QUAD_MAX + 1]
        out[d] = {"distinct": distinct, "tiled": tiled,
                  "quad": _run(ci, tiled[:QUAD_MAX], d, "FBN_CI_FORCE_BITS"),
                  "lane": _run(ci, tiled, d, "FBN_CI_FORCE_BITS"),
                  "byte": _run(ci, distinct, d, "FBN_CI_NO_BITS")}
    return out


@pytest.mark.parametrize("d", [0, 1])
def test_four_lane_and_lane_per_test_passes_agree(paths, d):
    for q, l in zip(paths[d]["quad"], paths[d]["lane"]):
        assert len(q) == QUAD_MAX and len(l) == QUAD_MAX + 1
        np.testing.assert_array_equal(q, l[:QUAD_MAX])


@pytest.mark.parametrize("d", [0, 1])
def test_both_passes_equal_the_byte_column_kernel(paths, d):
    m = len(paths[d]["distinct"])
    for q, l, b in zip(paths[d]["quad"], paths[d]["lane"], paths[d]["byte"]):
        np.testing.assert_array_equal(q, b[np.arange(QUAD_MAX) % m])
        np.testing.assert_array_equal(l, b[np.arange(QUAD_MAX + 1) % m])


@pytest.mark.parametrize("n", [1, 15, 16, 17, 65])
@pytest.mark.parametrize("d", [0, 1])
def test_four_lane_pass_ragged_last_group_wave_and_block(paths, d, n):
    """16 tests fill a wave and 64 a block of the four-lane pass: batches that end inside a wave, at
    its end, one past it and one past a block give the first n results of the full batch."""
    got = _run(paths["ci"], paths[d]["tiled"][:n], d, "FBN_CI_FORCE_BITS")
    for g, q in zip(got, paths[d]["quad"]):
        np.testing.assert_array_equal(g, q[:n])


@pytest.mark.parametrize("d", [0, 1])
def test_lane_per_test_pass_logs_the_decision_margin(paths, d):
    """The wave-reduced margin log of the lane-per-test pass: the minimum |p - alpha| over the batch
    and no test within 1e-9 of alpha."""
    ci = paths["ci"]
    ci.decision_margin(reset=True)
    _, _, p, _ = _run(ci, paths[d]["tiled"], d, "FBN_CI_FORCE_BITS")
    m, near = ci.decision_margin()
    assert (m, near) == (np.min(np.abs(p - ALPHA)), 0)
