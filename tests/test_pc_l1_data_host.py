"""The datasets of tests/pc_l1_data.py against the restatement, on the CPU: the properties the GPU
tests of the device level-1 search (test_gpu_pc_l1_rounds.py) rely on -- exact edge counts, an edge
without candidates, an edge the screen empties, round-0 demand above the cap for every knob set
meant to clip, kept pairs on both sides of every 1,024-variable boundary.  If a generator drifts,
these fail here instead of the GPU tests passing vacuously."""
import numpy as np
import pytest
import pc_l1_data as D

import oracle as O


def _ref(cols, dims, alpha=0.05, keep_log=False):
    r = O.OracleDataset(columns=cols, dims=dims).pc_stable(alpha, 2, 1, keep_log=keep_log)
    return r, D.level1_shape(len(dims), r["sepset"], r["tests_per_level"])


@pytest.mark.parametrize("E", D.EDGE_COUNTS)
def test_edge_count_dataset_is_exact(E):
    cols, dims = D.edge_count_dataset(E)
    assert cols.dtype == np.uint8 and dims.min() >= 2 and dims.max() <= 4
    assert (cols.max(axis=1) + 1 == dims).all()
    r, sh = _ref(cols, dims, keep_log=True)
    assert sh["E"] == E
    # the margin: no level-0 decision anywhere near alpha (the design gives p = 1 or p ~ 0)
    p0 = np.array([t[6] for t in r["log"] if t[0] == 0])
    assert p0.size == len(dims) * (len(dims) - 1) // 2
    assert ((p0 < 1e-12) | (p0 > 0.999)).all() and int((p0 < 1e-12).sum()) == E
    # edge 0 = the isolated pair: no candidates, kept, no test counted for it
    assert sh["edges"][0] == (0, 1) and sh["L"][0] == 0 and (0, 1) in r["edges"]
    assert not any(t[0] == 1 and (t[1], t[2]) == (0, 1) for t in r["log"])
    if E > 1:  # the last edge (a tile of its own at E = 257) has candidates, and level 1 has work
        assert sh["L"][-1] == 42 and sh["counted"] > 0
        assert sh["cands"] == sum(sh["L"]) > 257


@pytest.mark.parametrize("name", sorted(D.HUB_SETS))
def test_hub_datasets_and_clip_conditions(name):
    cols, dims = D.hub_dataset(**D.HUB_SETS[name])
    assert dims.min() >= 2 and dims.max() <= 4 and len(dims) >= 65
    r, sh = _ref(cols, dims)
    E, cands, L = sh["E"], sh["cands"], np.array(sh["L"])
    # the numbers the GPU tests and the summary quote (pinned: a drifting generator shows here)
    assert (E, cands, sh["counted"]) == D.HUB_PINNED[name], (E, cands, sh["counted"])
    assert L.max() > 64  # the screen's ballot loop (64 candidates a step) takes a second step
    assert sh["deg"].max() > 64 or name == "two"
    assert cands > 16384  # above the full-speculation threshold: the round machine takes level 1
    assert cands < (1 << 19)  # the default cap equals cands: the default schedule never clips
    for kname, knobs in D.knob_sets(E).items():
        cap = min(cands, int(knobs.get("FBN_PC_L1CAP", 1 << 19)))
        c0 = D.chunk0(E, int(knobs.get("FBN_PC_ROUND0", 8192)))
        c0 = min(c0, int(knobs.get("FBN_PC_L1_MAXCHUNK", 1 << 16)))
        demand = int(np.minimum(L, c0).sum())  # round 0 without the screen
        if kname in D.CLIPPING:
            assert E * c0 > cap and demand > cap, (kname, E, c0, cap)
        else:
            assert demand <= cap, (kname, E, c0, cap)
        # under 2,000 rounds: a clipped round runs cap tests, and no more than cands tests run in all
        assert cands / cap < 2000, (kname, cands, cap)
    # whole tiles of length 0 under the cap of about E / 3: the cap is spent before tile 2 starts
    third = int(D.knob_sets(E)["cap_third"]["FBN_PC_L1CAP"])
    assert int(np.minimum(L[:512], D.chunk0(E)).sum()) > third and E > 768
    # one edge's chunk cut in the middle: the cap is no multiple of the chunk, every L >= the chunk
    cut = D.knob_sets(E)["cut"]
    assert int(cut["FBN_PC_L1CAP"]) % 32 != 0 and D.chunk0(E, int(cut["FBN_PC_ROUND0"])) == 32 and L[:8].min() >= 32
    # where the edges close: the hub's index decides (first candidate ... last candidate of adj(x))
    share = sh["counted"] / cands  # of every candidate set, the part the restatement runs
    if name == "first":
        assert share < 0.1
    if name == "last":
        assert share > 0.5


def test_screened_pair_dataset_has_an_emptied_edge():
    """Edge (0, 1): L > 0 candidates, none of which passes the screen (P == 0 < L), with the
    predicate as tests/test_mi_screen.py restates it; some other edge keeps candidates."""
    from test_mi_screen import _plausible
    cols, dims = D.screened_pair_dataset()
    n = cols.shape[1]
    r, sh = _ref(cols, dims, keep_log=True)
    V = len(dims)
    mi = np.zeros((V, V))
    for lvl, x, y, z, g2, df, p, ind in r["log"]:
        if lvl == 0:
            mi[x, y] = mi[y, x] = g2 / (2 * n)
    adj = {v: [] for v in range(V)}
    for x, y in sh["edges"]:
        adj[x].append(y)
        adj[y].append(x)
    cand01 = [z for z in adj[0] if z != 1] + [z for z in adj[1] if z != 0]
    assert sh["edges"][0] == (0, 1) and len(cand01) == sh["L"][0] >= 6
    assert not any(_plausible(mi, dims, n, 0, 1, z) for z in cand01)
    # by a wide margin (the device uses its band's upper end, test_mi_screen the quantile itself)
    assert max(max(mi[0, z], mi[1, z]) for z in cand01) < 0.25 * mi[0, 1]
    # the edge is kept and all its candidates count, as the restatement runs them
    assert (0, 1) in r["edges"]
    assert sum(1 for t in r["log"] if t[0] == 1 and (t[1], t[2]) == (0, 1)) == sh["L"][0]
    kept_some = sum(any(_plausible(mi, dims, n, x, y, z) for z in
                        [u for u in adj[x] if u != y] + [u for u in adj[y] if u != x]) for x, y in sh["edges"][1:])
    assert kept_some > 0
    assert sh["cands"] > 0


@pytest.mark.parametrize("nv", D.WIDE_NV)
def test_wide_dataset_has_kept_pairs_around_every_boundary(nv):
    """Every planted link is dependent at level 0 (alpha 1e-4) by a wide margin, and the links sit
    on both sides of -- and across -- every 1,024 boundary, so ci_kept_scan's carried offsets differ
    from the uncarried ones."""
    cols, dims = D.wide_dataset(nv, D.WIDE_NS[nv], D.WIDE_SEED)
    assert cols.shape == (nv, D.WIDE_NS[nv]) and dims.min() >= 2 and dims.max() <= 4
    # level 0 takes the matrix-core Gram (its one-hot build then walks past its 1,024-row grid)
    assert float((dims - 1).sum()) ** 2 * D.WIDE_NS[nv] >= 1e10
    pairs, triples = D.wide_planted(nv)
    links = [(v, v + 1) for v in pairs] + [(v + k, v + k + 1) for v in triples for k in (0, 1)]
    assert len(set(links)) == len(links) >= 200
    od = O.OracleDataset(columns=cols, dims=dims)
    for x, y in links:
        t = od.ci_test(x, y, alpha=D.WIDE_ALPHA)
        assert not t["is_independent"] and t["p_value"] < 1e-3 * D.WIDE_ALPHA
    for v in triples:  # the chain's ends: dependent at level 0, separated by the middle at level 1
        assert not od.ci_test(v, v + 2, alpha=D.WIDE_ALPHA)["is_independent"]
        assert od.ci_test(v, v + 2, [v + 1], alpha=D.WIDE_ALPHA)["is_independent"]
    for b in range(1024, nv, 1024):
        assert any(y < b for _, y in links), b  # below the boundary
        assert any(x < b <= y for x, y in links), b  # across it
        assert any(y >= b for _, y in links), b  # variables at or past it have neighbours
    if nv > 2048:
        assert sum(x >= 1024 for x, _ in links) > 100  # many links wholly inside the second block
