"""The level-0 Gram kernels at their own edges (ci_gram_mfma.hip, ci_bits_gram.hip; shapes, reference and
restated split rule: tests/gram_edges.py).  Every pair table of the complete graph, through the
poisoned debug entry (IndependenceTest.level0_range_counts: an unwritten Gram entry reads -1), equals
the float64 one-hot matmul reference exactly, and level0_info() confirms the kernel and the split
each case means to reach:

* the FP4 MFMA Gram at split-K slices of 1 .. 8 stages (below, at and above its 5-buffer ring) on a
  single diagonal tile, on R = 257 (a panel of one real row), at 65,408-sample slices (the uint16
  bound), one sample past them, two full slabs, and on three ragged panels with 1-state variables,
  panel-straddling variables and an empty leading row;
* the popcount Gram and the tiled pairs kernel on the same datasets, and the popcount Gram's own
  partial 8 x 8 tasks / tail words on small shapes that stay below the MFMA threshold by themselves;
* ranged batches (pair0 > 0, tiles from panel I > 0, the cached task lists) back to back on one
  context and on fresh contexts;
* PC-stable's level 0 in chunks that split inside a panel against the restatement."""
import numpy as np
import pytest

import fastbn_amd as F
import gram_edges as E

pytestmark = pytest.mark.gpu

BACKEND_ENV = {"mfma": None, "popcount": "FBN_CI_GRAM_NO_MFMA", "tiled": "FBN_CI_NO_GRAM"}
BACKEND_PATH = {"mfma": 2, "popcount": 1, "tiled": 3}


def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def context(name):
    cols, dims = E.dataset(name)
    return F.IndependenceTest(F.Dataset(columns=cols, dims=dims))


def set_backend(monkeypatch, backend, splits=None):
    for var in ("FBN_CI_GRAM_NO_MFMA", "FBN_CI_NO_GRAM", "FBN_CI_GRAM4_SPLITS", "FBN_PC_L0CHUNK"):
        monkeypatch.delenv(var, raising=False)
    if BACKEND_ENV[backend]:
        monkeypatch.setenv(BACKEND_ENV[backend], "1")
    if splits is not None:
        monkeypatch.setenv("FBN_CI_GRAM4_SPLITS", str(splits))


def assert_tables(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    bad = np.flatnonzero((got != ref).any(1))
    assert bad.size == 0, "%s: %d of %d pair tables differ, first pair %d: got %s, reference %s" % (
        what, bad.size, len(ref), bad[0], got[bad[0]].tolist(), ref[bad[0]].tolist())


def assert_mfma_info(info, name, nt, splits, declared=None):
    """path 2 and the restated split of a launch of nt tiles; `declared`: the shape table's figures."""
    cols, dims = E.dataset(name)
    _, R = E.lead_offsets(dims)
    N = cols.shape[1]
    KS, S, lo, hi = E.split_rule(N, nt, splits, num_cu()) if nt else ((N + E.STAGE - 1) // E.STAGE, 0, 0, 0)
    want = {"path": 2, "R": R, "Rp": (R + E.TILE - 1) // E.TILE * E.TILE, "KS": KS, "nt": nt, "S": S,
            "shortest": lo, "longest": hi}
    assert info == want
    if declared is not None and (splits is not None or num_cu() == 256):
        assert (S, lo, hi) == declared


CASES = [(name, splits) for name, shape in E.SHAPES.items() for splits in shape[4]]


@pytest.mark.parametrize("name,splits", CASES, ids=["%s-S%s" % (n, "default" if s is None else s) for n, s in CASES])
def test_mfma_gram_every_pair_at_each_split(monkeypatch, name, splits):
    set_backend(monkeypatch, "mfma", splits)
    ci = context(name)
    ref = E.reference_tables(name)
    got = ci.level0_range_counts(0, len(ref))
    _, dims = E.dataset(name)
    assert_mfma_info(ci.level0_info(), name, E.tiles_of(E.lead_offsets(dims)[1]), splits, E.SHAPES[name][4][splits])
    assert_tables(got, ref, "%s, FBN_CI_GRAM4_SPLITS=%s" % (name, splits))


@pytest.mark.parametrize("name", list(E.SHAPES))
@pytest.mark.parametrize("backend", ["popcount", "tiled"])
def test_other_backends_every_pair(monkeypatch, name, backend):
    set_backend(monkeypatch, backend)
    ci = context(name)
    ref = E.reference_tables(name)
    got = ci.level0_range_counts(0, len(ref))
    info = ci.level0_info()
    assert info["path"] == BACKEND_PATH[backend]
    if backend == "popcount":
        assert info["R"] == E.lead_offsets(E.dataset(name)[1])[1] and info["nt"] > 0
    assert_tables(got, ref, "%s, %s" % (name, backend))


@pytest.mark.parametrize("N", E.SMALL_N)
def test_popcount_gram_partial_tasks_and_tail_words(monkeypatch, N):
    """Nothing set: 76 leading rows x ~4k samples stay on the popcount Gram by the threshold alone."""
    set_backend(monkeypatch, "mfma")
    cols, dims, ref = E.small_dataset(N)
    ci = F.IndependenceTest(F.Dataset(columns=cols, dims=dims))
    got = ci.level0_range_counts(0, len(ref))
    info = ci.level0_info()
    assert info["path"] == 1 and info["R"] == 76
    assert_tables(got, ref, "small N=%d" % N)
    # a range that starts mid-row, then the whole again: the popcount task cache in both directions
    assert_tables(ci.level0_range_counts(100, 333), ref[100:433], "small N=%d, pairs [100, 433)" % N)
    assert_tables(ci.level0_range_counts(0, len(ref)), ref, "small N=%d, whole again" % N)


def check_range(ci, name, backend, label, pair0, n):
    ref = E.reference_tables(name)
    got = ci.level0_range_counts(pair0, n)
    info = ci.level0_info()
    if backend == "mfma":
        assert_mfma_info(info, name, E.range_tiles(E.dataset(name)[1], pair0, n), None)
    else:
        assert info["path"] == 1
    assert_tables(got, ref[pair0:pair0 + n], "%s %s, range %s [%d, %d)" % (name, backend, label, pair0, pair0 + n))


@pytest.mark.parametrize("name", ["r257", "ragged3"])
@pytest.mark.parametrize("backend", ["mfma", "popcount"])
def test_ranged_batches_back_to_back_on_one_context(monkeypatch, name, backend):
    set_backend(monkeypatch, backend)
    ci = context(name)
    for label, pair0, n in E.pair_ranges(name):
        check_range(ci, name, backend, label, pair0, n)


@pytest.mark.parametrize("name", ["r257", "ragged3"])
@pytest.mark.parametrize("backend", ["mfma", "popcount"])
def test_ranged_batches_on_fresh_contexts(monkeypatch, name, backend):
    set_backend(monkeypatch, backend)
    for label, pair0, n in E.pair_ranges(name)[1:-1]:
        check_range(context(name), name, backend, label, pair0, n)


def test_range_entry_restores_the_pair_mode_and_checks_its_range(monkeypatch):
    """A debug launch between two uses of the recorded pair tables changes neither them nor the path
    the next batches take; a range outside the complete graph is refused."""
    set_backend(monkeypatch, "mfma")
    cols, dims, ref = E.small_dataset(4097)
    ci = F.IndependenceTest(F.Dataset(columns=cols, dims=dims))
    items = np.array([[2, 5, 9], [3, 30, 1], [10, 38, 20]], np.int32)
    before = ci.production_counts(items, 1)
    ci.level0_range_counts(50, 7)
    np.testing.assert_array_equal(ci.production_counts(items, 1), before)
    P = len(ref)
    assert ci.level0_range_counts(P, 0).shape == (0, 16)
    for pair0, n in [(-1, 2), (P - 1, 2), (P + 1, 0)]:
        with pytest.raises(F.api.FastBNError):
            ci.level0_range_counts(pair0, n)


@pytest.fixture(scope="module")
def ragged3_restatement():
    import oracle as O
    cols, dims = E.dataset("ragged3")
    return O.OracleDataset(columns=cols, dims=dims).pc_stable(0.05, 1, 1)


@pytest.mark.parametrize("chunk", [None, 10007])
def test_pc_level0_in_chunks_equals_restatement(monkeypatch, ragged3_restatement, chunk):
    """10,007 pairs per batch: every batch but the first starts inside a variable's row of pairs and
    inside a panel (28.5 rows of pairs of the 352 variables; panels end at variables 128 and 256)."""
    set_backend(monkeypatch, "mfma")
    if chunk:
        monkeypatch.setenv("FBN_PC_L0CHUNK", str(chunk))
    ci = context("ragged3")
    pc = F.PCStable(0.05, 1).StructLearnCompData(ci)
    ref = ragged3_restatement
    assert pc.tests_per_level.tolist() == ref["tests_per_level"]
    assert pc.edges == ref["edges"]
    assert pc.sepset == ref["sepset"]
    info = ci.level0_info()
    assert info["path"] == 2 and info["R"] == 700
    P = len(E.reference_tables("ragged3"))
    last0 = (P - 1) // chunk * chunk if chunk else 0  # the last batch is the one the record describes
    assert info["nt"] == E.range_tiles(E.dataset("ragged3")[1], last0, P - last0)
