"""Seeded datasets that steer the device level-1 search of PC-stable (ci_l1.hip's round machine:
ci_l1_setup / ci_l1_gen / ci_l1_resolve / l1_tile_scan, and the level 0 -> 1 hand-off ci_kept_*)
to its round, clip, tile and 1,024-variable edges.  Plain numpy: no project library, no GPU.

Every generator returns (cols uint8 [nv][ns], dims int32 [nv]) with every state count in 2..4.
tests/test_pc_l1_data_host.py pins the properties the GPU tests rely on against the restatement;
tests/test_gpu_pc_l1_rounds.py runs them through the device."""
import itertools

import numpy as np


def _noisy_copy(rng, src, d, ns, keep):
    """src % d with probability `keep`, else a uniform draw from d states."""
    return np.where(rng.random(ns) < keep, src % d, rng.integers(0, d, ns)).astype(np.uint8)


def hub_dataset(nv, ns, hubs, noise, seed):
    """`hubs`: the indices of the hub variables (independent, uniform, 4 states).  The last `noise`
    of the other variables are independent; every remaining variable copies one hub (round robin)
    through a noisy channel: hub % dims[v] with probability 0.7, else a uniform draw.

    All pairs under one hub are dependent at level 0 and independent given the hub, so the hub's
    index decides at which candidate position every such edge closes: index 0 -> the first candidate
    (round 0), index nv - 1 -> the last candidate of adj(x) (many rounds).  Hub-child edges never
    close (every candidate runs).  Degrees exceed 64 for nv >= 70 or so with one hub."""
    rng = np.random.default_rng(seed)
    hubs = [int(h) for h in hubs]
    assert len(set(hubs)) == len(hubs) and all(0 <= h < nv for h in hubs)
    dims = rng.integers(2, 5, nv).astype(np.int32)
    cols = np.empty((nv, ns), np.uint8)
    for h in hubs:
        dims[h] = 4
        cols[h] = rng.integers(0, 4, ns)
    others = [v for v in range(nv) if v not in hubs]
    assert 0 <= noise <= len(others)
    children = others[:len(others) - noise]
    for v in others[len(others) - noise:]:
        cols[v] = rng.integers(0, dims[v], ns)
    for k, v in enumerate(children):
        cols[v] = _noisy_copy(rng, cols[hubs[k % len(hubs)]], dims[v], ns, 0.7)
    return cols, dims


# ---- exact edge counts: a full factorial design
# The samples enumerate a 4^6 full factorial (ns = 4096: six 4-state factors, i.e. twelve index
# bits), so functions of different factors are independent *exactly* (G^2 = 0, p = 1), and two
# functions of one factor that each single out at least one of its states are dependent with
# G^2 in the thousands (p = 0): the level-0 edge count is exact at any alpha, with the widest
# margin there is.  No pseudo-random independence, hence no 5 % of spurious pairs.
_EDGE_GROUPS = {1: [2], 255: [2, 2, 23], 256: [2, 2, 2, 23], 257: [2, 3, 23]}  # clique sizes: sum C(k, 2) = E
EDGE_COUNT_NS = 4096


def _factor_functions():
    """Maps of a 4-state factor that single out at least one state (so any two are dependent):
    the 24 permutations (4 states), merges of two states (3 states), one state against the rest (2)."""
    perms = [list(p) for p in itertools.permutations(range(4))]
    merges = []
    for a, b in itertools.combinations(range(4), 2):
        rest = [s for s in range(4) if s not in (a, b)]
        m = [0] * 4
        m[a] = m[b] = 2
        m[rest[0]], m[rest[1]] = 0, 1
        merges.append(m)
    ones = [[int(s == a) for s in range(4)] for a in range(4)]
    return perms, merges, ones


def edge_count_dataset(E, ns=EDGE_COUNT_NS, seed=0):
    """Exactly E kept pairs after level 0 (E in 1, 255, 256, 257): disjoint cliques, each the
    functions of one factor of the design, and independent filler (single index bits).  Variables 0
    and 1 are an isolated dependent pair (an edge without candidates, L == 0, the first edge of the
    list); the 23-clique has the highest indices, so the last edge of the list has 42 candidates."""
    assert ns == EDGE_COUNT_NS and E in _EDGE_GROUPS
    rng = np.random.default_rng(seed)
    idx = np.arange(ns)
    sizes = _EDGE_GROUPS[E]
    assert sum(k * (k - 1) // 2 for k in sizes) == E
    perms, merges, ones = _factor_functions()
    cols, dims = [], []

    def clique(f, k):
        factor = (idx >> (2 * f)) & 3
        # at least every third member keeps the 4 states (such a z closes the clique's edges)
        for j in range(k):
            pool = perms if j % 3 == 0 else (perms, merges, ones)[int(rng.integers(0, 3))]
            m = np.asarray(pool[int(rng.integers(0, len(pool)))])
            cols.append(m[factor].astype(np.uint8))
            dims.append(int(m.max()) + 1)

    clique(0, sizes[0])  # the isolated pair: variables 0, 1
    for b in range(2 * len(sizes), 12):  # filler: the index bits no clique uses
        cols.append(((idx >> b) & 1).astype(np.uint8))
        dims.append(2)
    for f in range(1, len(sizes)):
        clique(f, sizes[f])
    return np.stack(cols), np.asarray(dims, np.int32)


def screened_pair_dataset(ns=4096, seed=0, nv=70, weak=6):
    """Variables 0 and 1: a strongly dependent pair (1 copies 0 with probability 0.9); variables
    2 .. 2 + weak copy variable 0 with probability 0.1 only -- dependent at level 0, but with far
    less information than the pair shares, so the level-1 screen removes every candidate of edge
    (0, 1): P == 0 < L.  The rest is independent filler."""
    rng = np.random.default_rng(seed)
    dims = rng.integers(2, 5, nv).astype(np.int32)
    dims[:2 + weak] = 4
    cols = np.stack([rng.integers(0, d, ns) for d in dims]).astype(np.uint8)
    cols[1] = _noisy_copy(rng, cols[0], 4, ns, 0.9)
    for v in range(2, 2 + weak):
        cols[v] = _noisy_copy(rng, cols[0], 4, ns, 0.1)
    return cols, dims


def wide_planted(nv):
    """The planted structure of wide_dataset: the first variables v of the chains (v, v + 1) and
    (v, v + 1, v + 2).  One chain crosses every 1,024 boundary and another lies next to it (when the
    boundary is the last variable, both end at or just below it); of the rest, three quarters lie
    above index 1,024 when there is room (nv = 2049)."""
    pairs, triples = [], []
    for b in range(1024, nv, 1024):
        if b + 1 <= nv - 1:
            pairs.append(b - 1)  # (b - 1, b): one endpoint on each side
            triples.append(b + 2 if b + 4 < nv else b - 5)
        else:  # b is the last variable (nv = b + 1): both chains end on it
            triples.append(b - 2)  # (b - 2, b - 1, b)
            pairs.append(b - 6)
    used = set()
    for v in pairs:
        used.update((v, v + 1))
    for v in triples:
        used.update((v, v + 1, v + 2))
    rng = np.random.default_rng(nv)
    want_pairs, want_triples = 200, 12
    while len(pairs) < want_pairs or len(triples) < want_triples:
        tri = len(triples) < want_triples
        n = 3 if tri else 2
        v = int(rng.integers(1026, nv - 8)) if nv > 2048 and rng.random() < 0.75 else int(rng.integers(0, 1016))
        if any(u in used for u in range(v - 1, v + n + 1)):  # one free variable between chains
            continue
        used.update(range(v, v + n))
        (triples if tri else pairs).append(v)
    return sorted(pairs), sorted(triples)


def wide_dataset(nv, ns, seed):
    """nv in 1025, 2049 (one and two carries of ci_kept_scan's 1,024-variable blocks): independent
    variables with planted chains v -> v + 1 (-> v + 2), each link a copy with probability 0.9, so
    the degree offsets off[] / upoff[] past every block boundary are non-zero.  Meant for alpha =
    1e-4 (spurious level-0 edges stay rare)."""
    rng = np.random.default_rng(seed)
    dims = rng.integers(2, 5, nv).astype(np.int32)
    pairs, triples = wide_planted(nv)
    for v in pairs:
        dims[v:v + 2] = 4
    for v in triples:
        dims[v:v + 3] = 4
    cols = np.stack([rng.integers(0, d, ns) for d in dims]).astype(np.uint8)
    for v in pairs:
        cols[v + 1] = _noisy_copy(rng, cols[v], 4, ns, 0.9)
    for v in triples:
        cols[v + 1] = _noisy_copy(rng, cols[v], 4, ns, 0.9)
        cols[v + 2] = _noisy_copy(rng, cols[v + 1], 4, ns, 0.9)
    return cols, dims


# ---- the restatement's numbers of a level-1 edge list, from its result (no code under test)
def level1_shape(nv, sepset, tests_per_level):
    """From a depth-2 restatement result: the level-1 edge list (pairs level 0 kept = all pairs
    minus the empty sepsets), E, cands = sum_e (deg x + deg y - 2) and every edge's L."""
    removed0 = {k for k, z in sepset.items() if len(z) == 0}
    edges = [(x, y) for x in range(nv) for y in range(x + 1, nv) if (x, y) not in removed0]
    deg = np.zeros(nv, np.int64)
    for x, y in edges:
        deg[x] += 1
        deg[y] += 1
    L = [int(deg[x] + deg[y] - 2) for x, y in edges]
    return {"edges": edges, "E": len(edges), "cands": int(sum(L)), "L": L, "deg": deg,
            "counted": int(tests_per_level[1]) if len(tests_per_level) > 1 else 0}


def chunk0(E, round0=8192):
    """The first round's per-edge chunk (capi_pc.hip CiLevel1Run; round0 = FBN_PC_ROUND0)."""
    return max(1, min(32, round0 // E))


# ---- the cases of the GPU tests (shared with the host test that pins them)
EDGE_COUNTS = (1, 255, 256, 257)
WIDE_NV = (1025, 2049)
# samples per width: the fewest (a multiple of 256) at which level 0 takes the matrix-core Gram, which
# wants leading rows^2 x samples >= 1e10 (capi_ci.hip CiGram0Mfma) -- below the bit-sliced path's
# 4096, so the tests force that path (FBN_CI_FORCE_BITS)
WIDE_NS = {1025: 2048, 2049: 768}
WIDE_SEED, WIDE_ALPHA = 3, 1e-4

# one hub dataset per hub position: 72 variables (67 or 66 children: degrees above 64), 4096 samples
HUB_SETS = {name: dict(nv=72, ns=4096, hubs=hubs, noise=4, seed=7)
            for name, hubs in (("first", [0]), ("middle", [36]), ("last", [71]), ("two", [0, 71]))}
# (E, cands, counted level-1 tests) of each, from the restatement at alpha 0.05, depth 2
HUB_PINNED = {"first": (2294, 302934, 27934), "middle": (2286, 301788, 100134), "last": (2306, 304966, 163717),
              "two": (1195, 80522, 25877)}


def knob_sets(E):
    """The chunk schedules of the round machine under test (environment knobs of capi_pc.hip
    CiLevel1Run); E: the level's edge count from the restatement, for the cap of about E / 3."""
    return {
        "default": {},
        "chunk1": {"FBN_PC_ROUND0": "1", "FBN_PC_L1_MAXCHUNK": "1"},  # chunk 1 forever: the most rounds
        "growth4": {"FBN_PC_ROUND0": "1", "FBN_PC_GROWTH": "4"},
        "maxchunk3": {"FBN_PC_L1_MAXCHUNK": "3"},
        "cap255": {"FBN_PC_L1CAP": "255"},
        "cap256": {"FBN_PC_L1CAP": "256"},
        "cap257": {"FBN_PC_L1CAP": "257"},
        "cap_third": {"FBN_PC_L1CAP": str(E // 3)},  # whole 256-edge tiles get length 0
        "cut": {"FBN_PC_ROUND0": str(1 << 20), "FBN_PC_L1CAP": "200"},  # chunk 32: the 7th edge is cut at 8
        "chunk1_cap256": {"FBN_PC_ROUND0": "1", "FBN_PC_L1_MAXCHUNK": "1", "FBN_PC_L1CAP": "256"},
    }


CLIPPING = ("cap255", "cap256", "cap257", "cap_third", "cut", "chunk1_cap256")
KNOB_NAMES = tuple(knob_sets(3))
