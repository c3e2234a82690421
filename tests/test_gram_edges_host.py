"""The level-0 Gram edge tests' own instruments (tests/gram_edges.py), checked without a GPU: the
matmul reference against a brute-force bincount, the shape table against its own claims by the
restated split rule, and the datasets for the cells they were built to hold."""
import numpy as np
import pytest

import gram_edges as E

NAMES = list(E.SHAPES)


def sample_pairs(nv, seed, k=40):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, nv - 1, k)
    y = np.minimum(nv - 1, x + 1 + rng.integers(0, nv, k))
    return sorted({(int(a), int(b)) for a, b in zip(x, y)} | {(0, 1), (0, nv - 1), (nv - 2, nv - 1)})


def test_reference_equals_bincount_on_a_tiny_dataset():
    rng = np.random.default_rng(3)
    dims = np.array([1, 2, 3, 4, 4, 1, 3, 2], np.int32)
    cols = np.stack([rng.integers(0, d, 301) for d in dims]).astype(np.uint8)
    cols[4][cols[4] == 2] = 0  # a state that never occurs
    T = E.tables_from_gram(E.onehot_gram(cols, dims), dims)
    t = 0
    for x in range(8):
        for y in range(x + 1, 8):
            ref = E.bincount_table(cols, dims, x, y)
            np.testing.assert_array_equal(T[t, :len(ref)], ref)
            assert (T[t, len(ref):] == 0).all()
            assert t == E.pair_index(x, y, 8)
            t += 1
    assert t == len(T)


@pytest.mark.parametrize("name", NAMES)
def test_reference_tables_of_each_shape(name):
    """A sample of pairs equals the brute force; every table sums to N with the per-column bincounts
    as its marginals."""
    cols, dims = E.dataset(name)
    nv, N = cols.shape
    T = E.reference_tables(name)
    assert T.shape == (nv * (nv - 1) // 2, 16)
    for x, y in sample_pairs(nv, 5):
        ref = E.bincount_table(cols, dims, x, y)
        np.testing.assert_array_equal(T[E.pair_index(x, y, nv), :len(ref)], ref)
    assert (T.sum(1) == N).all()
    marg = [np.bincount(cols[v], minlength=dims[v]) for v in range(nv)]
    t = 0
    for x in range(nv):
        for y in range(x + 1, nv):
            tab = T[t, :dims[x] * dims[y]].reshape(dims[x], dims[y])
            assert (tab.sum(1) == marg[x]).all() and (tab.sum(0) == marg[y]).all(), (x, y)
            t += 1


@pytest.mark.parametrize("name", NAMES)
def test_shape_table_claims(name):
    mk, N, _, _, declared = E.SHAPES[name]
    cols, dims = E.dataset(name)
    assert cols.shape == (len(dims), N) and (cols.max(1) < dims).all()
    _, R = E.lead_offsets(dims)
    Rp = (R + E.TILE - 1) // E.TILE * E.TILE
    want = {"diag": (256, 256, 1, 1193), "r257": (257, 512, 3, 1183), "max": (400, 512, 3, 511),
            "max+1": (400, 512, 3, 512), "2x511": (400, 512, 3, 1022), "ragged3": (700, 768, 6, 161)}[name]
    assert (R, Rp, E.tiles_of(R), (N + E.STAGE - 1) // E.STAGE) == want
    assert float(R) * R * N >= E.MFMA_MIN  # the MFMA Gram is eligible ...
    if name in ("diag", "r257"):
        assert float(R) * R * (N - 100) < E.MFMA_MIN  # ... and these are the smallest N that are
    for splits, (S, lo, hi) in declared.items():
        KS, s, a, b = E.split_rule(N, E.tiles_of(R), splits)
        assert (s, a, b) == (S, lo, hi), (splits, (s, a, b))
        assert hi <= E.SLICE_CAP and hi * E.STAGE < 65536
        # the slices tile [0, KS) without gaps
        bounds = [k * KS // S for k in range(S + 1)]
        assert bounds[0] == 0 and bounds[-1] == KS and all(q > p for p, q in zip(bounds, bounds[1:]))


def test_slice_sweep_surrounds_the_ring():
    """diag's splits reach every slice length 1 .. RING + 3: below, at and above the ring depth."""
    lens = set()
    for S, lo, hi in E.SHAPES["diag"][4].values():
        lens |= {lo, hi}
    assert set(range(1, E.RING + 4)) <= lens
    assert E.SHAPES["max"][1] == E.SLICE_CAP * E.STAGE == 65408 and E.SHAPES["2x511"][1] == 2 * 65408


@pytest.mark.parametrize("name", ["max", "max+1", "2x511"])
def test_stress_columns_hold_their_cells(name):
    cols, dims = E.dataset(name)
    nv, N = cols.shape
    T = E.reference_tables(name)
    lead0, _ = E.lead_offsets(dims)
    for i, x in enumerate(E.CONST0):
        assert dims[x] > 1
        for y in E.CONST0[i + 1:]:
            assert T[E.pair_index(x, y, nv), 0] == N > 32767  # one Gram entry counts every sample
    # same quadrant, other quadrant of the panel, other panel
    q = [int(lead0[v]) // 128 for v in E.CONST0]
    assert q[0] == q[1] == 0 and q[2] == 1 and q[3] >= 2
    d = dims[E.CONST_LAST]
    assert d > 2 and (cols[E.CONST_LAST] == d - 1).all()  # every leading row empty
    t = T[E.pair_index(E.CONST_LAST, E.NEARLY0, nv), :d * dims[E.NEARLY0]].reshape(d, -1)
    assert (t[:-1] == 0).all() and t[-1, 0] == N - E.NEARLY0_HITS
    assert np.bincount(cols[E.NEARLY0])[0] == N - E.NEARLY0_HITS


@pytest.mark.parametrize("name,cuts", [("r257", [256]), ("ragged3", [256, 512])])
def test_ragged_columns_hold_their_edges(name, cuts):
    cols, dims = E.dataset(name)
    nv = len(dims)
    lead0, R = E.lead_offsets(dims)
    assert dims[0] == 1 and dims[-1] == 1 and (dims[1:-1] == 1).any()
    assert set(dims.tolist()) == {1, 2, 3, 4}
    for c in cuts:  # a variable with leading rows on both sides of the panel boundary
        assert any(lead0[v] < c < lead0[v] + dims[v] - 1 for v in range(nv)), c
    assert not (cols[E.EMPTY_STATE_VAR] == E.EMPTY_STATE).any() and dims[E.EMPTY_STATE_VAR] > E.EMPTY_STATE + 1
    if name == "r257":
        assert R - E.TILE == 1  # the second panel: one real row
    rs = E.pair_ranges(name)
    P = nv * (nv - 1) // 2
    starts = {E.row_start(x, nv) for x in range(nv - 1)}
    by = {lab: (p0, n) for lab, p0, n in rs}
    assert all(0 <= p0 and n >= 1 and p0 + n <= P for p0, n in by.values())
    assert by["whole"] == by["whole-again"] == (0, P) and by["last-pair"] == (P - 1, 1)
    assert by["mid-row"][0] not in starts and by["mid-row"][0] + by["mid-row"][1] not in starts
    assert by["last-panel"][0] in starts and by["last-panel"][0] > 0
    if name == "ragged3":
        x = max(v for v in range(nv - 1) if E.row_start(v, nv) <= by["last-panel"][0])
        assert lead0[x] >= 512


@pytest.mark.parametrize("N", E.SMALL_N)
def test_small_shapes_stay_below_the_mfma_threshold(N):
    cols, dims, T = E.small_dataset(N)
    _, R = E.lead_offsets(dims)
    assert R % 8 != 0 and float(R) * R * N < E.MFMA_MIN and len(dims) == 40
    assert (T.sum(1) == N).all()
    for x, y in sample_pairs(40, N, 12):
        ref = E.bincount_table(cols, dims, x, y)
        np.testing.assert_array_equal(T[E.pair_index(x, y, 40), :len(ref)], ref)
