"""The device-resident level-1 search of PC-stable (ci_l1.hip ci_l1_setup / ci_l1_gen /
ci_l1_resolve / l1_tile_scan, driven by capi_pc.hip CiLevel1Run) and the level 0 -> 1 hand-off
(ci_kept_count / ci_kept_scan / ci_kept_fill) at their round, clip, tile and 1,024-variable edges,
against the restatement at depth 2 (levels 0 and 1): tests per level, skeleton and sepsets.

The chunk schedule is moved with the four knobs CiLevel1Run reads on every call (FBN_PC_ROUND0,
FBN_PC_GROWTH, FBN_PC_L1_MAXCHUNK, FBN_PC_L1CAP); the datasets (tests/pc_l1_data.py) decide where
edges close.  tests/test_pc_l1_data_host.py pins, on the CPU, that the datasets and knob sets do
what these tests assume (edge counts, round-0 demand above the cap, emptied and candidate-less
edges, kept pairs around every 1,024 boundary)."""
import pytest
import pc_l1_data as D

import fastbn_amd as F
import oracle as O

pytestmark = pytest.mark.gpu

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _reference(cols, dims, alpha=0.05):
    r = O.OracleDataset(columns=cols, dims=dims).pc_stable(alpha, 2, 1)
    r["shape"] = D.level1_shape(len(dims), r["sepset"], r["tests_per_level"])
    return r


def _hub(name):
    """(cols, dims, restatement) of one hub dataset, computed once per module."""
    def make():
        cols, dims = D.hub_dataset(**D.HUB_SETS[name])
        return cols, dims, _reference(cols, dims)
    return _once(("hub", name), make)


def _run(monkeypatch, src, knobs, alpha=0.05):
    """One depth-2 run under `knobs` (set for this run only); src: (cols, dims) -> a fresh context,
    or an IndependenceTest."""
    with monkeypatch.context() as m:
        for k, v in knobs.items():
            m.setenv(k, v)
        ci = src if isinstance(src, F.IndependenceTest) else F.IndependenceTest(F.Dataset(columns=src[0], dims=src[1]), alpha)
        return F.PCStable(alpha, 2).StructLearnCompData(ci)


def _fields(pc):
    return {"tests": pc.tests_per_level.tolist(), "launched": pc.launched_per_level.tolist(), "edges": pc.edges,
            "sepset": pc.sepset, "oriented": pc.oriented}


def _assert_is_reference(pc, ref):
    assert pc.tests_per_level.tolist() == ref["tests_per_level"]
    assert pc.edges == ref["edges"]
    assert pc.sepset == ref["sepset"]


NO_SCREEN = {"FBN_PC_NO_MISCREEN": "1"}


@pytest.mark.parametrize("knob", D.KNOB_NAMES)
@pytest.mark.parametrize("hub", sorted(D.HUB_SETS))
def test_round_schedule_matrix(hub, knob, monkeypatch):
    """Hub first / middle / last / two hubs x every chunk schedule, with the information screen and
    without: always the restatement's result and the default schedule's orientation; without the
    screen counted <= launched <= cands, and launched == counted when the chunk is pinned at 1 (no
    speculation: a candidate run twice or skipped shows); the screen never launches more."""
    cols, dims, ref = _hub(hub)
    sh = ref["shape"]
    assert (sh["E"], sh["cands"], sh["counted"]) == D.HUB_PINNED[hub]
    base = _once(("default", hub), lambda: _run(monkeypatch, (cols, dims), {}))
    assert base.path == 3  # the device hand-off and, cands being above the threshold, the round machine
    knobs = D.knob_sets(sh["E"])[knob]
    on = _run(monkeypatch, (cols, dims), knobs)
    off = _run(monkeypatch, (cols, dims), dict(knobs, **NO_SCREEN))
    for pc in (on, off):
        assert pc.path == 3
        _assert_is_reference(pc, ref)
        assert pc.oriented == base.oriented
    counted, l_on, l_off = ref["tests_per_level"][1], int(on.launched_per_level[1]), int(off.launched_per_level[1])
    assert counted <= l_off <= sh["cands"]
    if knobs.get("FBN_PC_L1_MAXCHUNK") == "1":
        assert l_off == counted
    assert l_on <= l_off


BOTH_ENTRY_KNOBS = ("default", "chunk1", "cap256", "cut")


@pytest.mark.parametrize("knob", BOTH_ENTRY_KNOBS)
def test_both_entries(knob, monkeypatch):
    """CiLevel1Run's two entries -- the device hand-off (edge list and adjacency built by ci_kept_*)
    and CiLevel1Device with host-built lists (FBN_PC_HOST_L0L1) -- on fresh contexts: equal in every
    field, launched tests included, and equal to the restatement."""
    cols, dims, ref = _hub("middle")
    knobs = D.knob_sets(ref["shape"]["E"])[knob]
    a = _run(monkeypatch, (cols, dims), knobs)
    b = _run(monkeypatch, (cols, dims), dict(knobs, FBN_PC_HOST_L0L1="1"))
    assert a.path == 3 and b.path == 0
    assert _fields(a) == _fields(b)
    _assert_is_reference(a, ref)


# FBN_PC_NO_SMALL: the edge-count datasets have fewer than 65 variables; FBN_PC_FULLSPEC -1: the
# round machine takes level 1 whatever its size (E = 1 has no candidate at all)
SMALL = {"FBN_PC_NO_SMALL": "1", "FBN_PC_FULLSPEC": "-1"}


@pytest.mark.parametrize("E,knobs", [(1, {}), (1, {"FBN_PC_L1CAP": "1"}), (255, {}), (256, {}), (257, {}),
                                     (257, {"FBN_PC_L1CAP": "256"}), (257, {"FBN_PC_L1CAP": "1"})],
                         ids=lambda v: str(v) if isinstance(v, int) else "-".join(v.values()) or "default")
def test_tile_boundaries(E, knobs, monkeypatch):
    """E = 1, 255, 256, 257 edges: one tile, a full tile, a second tile with one live lane.  Cap 256
    at E = 257 spends round 0 inside tile 0 (the lone edge of tile 1 gets length 0 and stays open);
    cap 1 runs one test per round.  Edge (0, 1) has no candidate: kept, no test counted."""
    cols, dims = D.edge_count_dataset(E)
    ref = _once(("edges", E), lambda: _reference(cols, dims))
    sh = ref["shape"]
    assert sh["E"] == E and sh["L"][0] == 0 and sh["edges"][0] == (0, 1)
    for screen in ({}, NO_SCREEN):
        pc = _run(monkeypatch, (cols, dims), dict(SMALL, **knobs, **screen))
        assert pc.path == 3
        _assert_is_reference(pc, ref)
        assert (0, 1) in pc.edges and (0, 1) not in pc.sepset
        l1 = int(pc.launched_per_level[1])
        assert l1 <= sh["cands"]
        if screen:
            assert l1 >= ref["tests_per_level"][1]
            if knobs.get("FBN_PC_L1CAP") == "1":  # one test a round: nothing speculative
                assert l1 == ref["tests_per_level"][1]
        if E == 1:
            assert ref["tests_per_level"][1] == 0 and l1 == 0


def test_all_candidates_screened(monkeypatch):
    """Edge (0, 1) of screened_pair_dataset: the screen removes every candidate (P == 0 < L, status
    2 written by ci_l1_setup), yet all L count, as the restatement runs them.  Screened and
    unscreened runs equal the restatement; the screened one launches fewer tests."""
    cols, dims = D.screened_pair_dataset()
    ref = _reference(cols, dims)
    knobs = {"FBN_PC_FULLSPEC": "0"}
    on = _run(monkeypatch, (cols, dims), knobs)
    off = _run(monkeypatch, (cols, dims), dict(knobs, **NO_SCREEN))
    for pc in (on, off):
        assert pc.path == 3
        _assert_is_reference(pc, ref)
        assert (0, 1) in pc.edges
    assert on.oriented == off.oriented
    L01 = ref["shape"]["L"][0]
    assert L01 >= 6 and ref["tests_per_level"][1] >= L01
    # edge (0, 1) alone saves its L launches under the screen
    assert int(on.launched_per_level[1]) <= int(off.launched_per_level[1]) - L01


def test_reuse_across_schedules(monkeypatch):
    """One context, four runs back to back -- a clipped schedule, chunk 1, the cut chunk, the first
    again: the first and the last are identical in every field (no stale status word, ticket or
    ring slot), and every run gives the restatement's result."""
    cols, dims, ref = _hub("two")
    ks = D.knob_sets(ref["shape"]["E"])
    ci = F.IndependenceTest(F.Dataset(columns=cols, dims=dims))
    runs = [_run(monkeypatch, ci, ks[k]) for k in ("cap257", "chunk1", "cut", "cap257")]
    for pc in runs:
        assert pc.path == 3
        _assert_is_reference(pc, ref)
    assert _fields(runs[0]) == _fields(runs[3])


WIDE = {"FBN_CI_FORCE_BITS": "1", "FBN_PC_FULLSPEC": "0"}  # fewer than 4096 samples; level 1 is small


@pytest.mark.parametrize("gram", ["mfma", "no_mfma"])
@pytest.mark.parametrize("nv", D.WIDE_NV)
def test_handoff_above_1024_variables(nv, gram, monkeypatch):
    """1025 and 2049 variables: ci_kept_scan's second and third 1,024-variable block (one and two
    carries) and, with the matrix-core Gram, ci_onehot4_build past its grid.y cap.  The hand-off
    equals the host-built path in every field; 1025 also equals the restatement; at 2049 (the
    restatement's level 0 alone takes ~10 s) the planted structure is checked instead: every
    planted link kept, every chain's end pair removed by the chain's middle."""
    cols, dims = _once(("wide", nv), lambda: D.wide_dataset(nv, D.WIDE_NS[nv], D.WIDE_SEED))
    knobs = dict(WIDE, **({"FBN_CI_GRAM_NO_MFMA": "1"} if gram == "no_mfma" else {}))
    a = _run(monkeypatch, (cols, dims), knobs, D.WIDE_ALPHA)
    b = _once(("wide_host", nv), lambda: _run(monkeypatch, (cols, dims), dict(WIDE, FBN_PC_HOST_L0L1="1"), D.WIDE_ALPHA))
    assert a.path == 3 and b.path == 0
    assert a.ci.level0_info()["path"] == (2 if gram == "mfma" else 1)
    assert _fields(a) == _fields(b)
    assert a.tests_per_level[0] == nv * (nv - 1) // 2 and a.tests_per_level[1] > 0
    if nv == 1025:
        _assert_is_reference(a, _once(("wide_ref", nv), lambda: _reference(cols, dims, D.WIDE_ALPHA)))
    pairs, triples = D.wide_planted(nv)
    edges, sep = set(a.edges), a.sepset
    for v in pairs:
        assert (v, v + 1) in edges
    for v in triples:
        assert (v, v + 1) in edges and (v + 1, v + 2) in edges
        assert (v, v + 2) not in edges and sep[(v, v + 2)] == (v + 1,)
    for b0 in range(1024, nv, 1024):
        assert any(y >= b0 for _, y in edges)
