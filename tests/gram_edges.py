"""Datasets, reference and shape table of the level-0 Gram edge tests (test_gram_edges_host.py,
test_gpu_gram_edges.py).  A plain module: nothing here touches the library.

Reference: the one-hot matrix O [sum dims][N] over ALL states of all variables as float64 and
G = O @ O.T (exact: every entry is an integer <= N, far below 2^53); the table of the pair (x, y) is
the block G[off_x : off_x + dx, off_y : off_y + dy].  It shares nothing with the kernels, which work
on the leading states only and derive the last row / column.

Split rule: split_rule() restates the host's choice of the split-K slices of the FP4 MFMA Gram
(capi_ci.hip CiGram0Mfma): KS = ceil(N / 128) stages, S = max(1, FBN_CI_GRAM4_SPLITS or CUs / tiles),
raised to ceil(KS / 511) (a slice of <= 511 stages = 65,408 samples keeps a partial in 16 bits),
capped at KS; slice k covers the stages [k KS / S, (k + 1) KS / S).  Each shape declares, per value
of FBN_CI_GRAM4_SPLITS, the (S, shortest, longest slice) it is there to reach."""
import functools

import numpy as np

TILE = 256        # rows of a Gram tile (ci_gram_mfma.hip kTile)
STAGE = 128       # samples of a pipeline stage (kStageS)
RING = 5          # stage buffers of the kernel's pipeline (kNBuf)
SLICE_CAP = 511   # stages per slice: 511 * 128 = 65,408 <= 65,535
MFMA_MIN = 1e10   # the MFMA Gram runs from R * R * N >= 1e10 on


def split_rule(N, nt, splits=None, num_cu=256):
    """(KS, S, shortest, longest) of a launch of nt tiles; splits = FBN_CI_GRAM4_SPLITS (None: unset)."""
    KS = (N + STAGE - 1) // STAGE
    S = max(1, num_cu // nt if splits is None else splits)
    S = max(S, (KS + SLICE_CAP - 1) // SLICE_CAP)
    S = min(S, KS)
    lens = [(k + 1) * KS // S - k * KS // S for k in range(S)]
    return KS, S, min(lens), max(lens)


def tiles_of(R):
    """Tiles (I, J >= I) of the whole pair range: nt."""
    nb = (R + TILE - 1) // TILE
    return nb * (nb + 1) // 2


_PAT = (2, 3, 4, 3)  # 8 leading rows per 4 variables


def _dims_r257():
    # 1-state variables at the start, in the middle and at the end; the last multi-state variable
    # (4 states) holds the leading rows 254, 255 | 256: the second panel has that one real row
    d = [1] + list(_PAT) * 15 + [1] + list(_PAT) * 16 + [4, 4, 4, 1, 1]
    return np.array(d, np.int32)


SMALL_N = (4096, 4097, 4127, 4129)  # bit-sliced rows: full words, 1 / 31 tail bits, a word past the pad to 4


@functools.lru_cache(maxsize=None)
def small_dataset(N):
    """40 variables of 1-4 states, 76 leading rows (the popcount Gram's last 8 x 8 tasks are partial),
    far below the MFMA threshold -> (cols, dims, reference tables [P][16])."""
    dims = np.array([1] + list(_PAT) * 9 + [2, 4, 1], np.int32)
    cols, _ = _columns(dims, N, 1000 + N)
    return cols, dims, tables_from_gram(onehot_gram(cols, dims), dims)


def _dims_ragged3():
    # rows 255 | 256, 257 in one 4-state variable, rows 511 | 512 in one 3-state variable, 1-state
    # variables at the start, after each straddling variable and at the end
    d = ([1] + list(_PAT) * 31 + [4, 4, 2, 4, 1] + list(_PAT) * 31 + [4, 3, 3, 1] + list(_PAT) * 23 + [4, 1])
    return np.array(d, np.int32)


def _dims_max():
    return np.array(list(_PAT) * 50, np.int32)  # R = 400


# max / max+1 / 2x511: variables constant at state 0 (their common cell counts all N samples): two
# in one 128-row quadrant, one in the other quadrant of the same panel, one in the second panel
CONST0 = (1, 2, 70, 150)
CONST_LAST = 9   # constant at its last state: every leading row empty
NEARLY0 = 20     # state 0 except a handful of samples
NEARLY0_HITS = 7
# r257 / ragged3: state 1 of this (4-state) variable never occurs
EMPTY_STATE_VAR, EMPTY_STATE = 7, 1


def _columns(dims, N, seed, group=None):
    """Mildly dependent columns (as conftest.gram_dataset): 30 % a shared base, else noise.  group:
    a base per `group` consecutive variables and a skewed noise distribution per variable instead --
    uneven tables, but a sparse skeleton (PC-stable's host orientation takes minutes on a
    near-complete graph of a few hundred variables)."""
    rng = np.random.default_rng(seed)
    cols = np.empty((len(dims), N), np.uint8)
    base = rng.integers(0, 4, N)
    for v, d in enumerate(dims):
        if group and v % group == 0:
            base = rng.integers(0, 4, N)
        noise = rng.choice(d, N, p=rng.dirichlet(2.0 * np.ones(d))) if group else rng.integers(0, d, N)
        keep = rng.random(N) < 0.3
        cols[v] = np.where(keep, base % d, noise)
    return cols, rng


# name -> (dims builder, N, seed, kind, {splits: (S, shortest, longest)}).  splits None: the device
# default (num_cu // nt), declared for a 256-CU device and asserted through split_rule(num_cu) on others.
SHAPES = {
    "diag": (lambda: np.full(128, 3, np.int32), 152601, 11, "plain",
             {1193: (1193, 1, 1), 597: (597, 1, 2), 400: (400, 2, 3), 300: (300, 3, 4), 240: (240, 4, 5),
              200: (200, 5, 6), 171: (171, 6, 7), 150: (150, 7, 8), 1: (3, 397, 398)}),
    "r257": (_dims_r257, 151405, 12, "ragged", {600: (600, 1, 2), 250: (250, 4, 5), None: (85, 13, 14)}),
    "max": (_dims_max, 65408, 13, "stress", {1: (1, 511, 511)}),
    "max+1": (_dims_max, 65409, 13, "stress", {1: (2, 256, 256)}),
    "2x511": (_dims_max, 130816, 13, "stress", {1: (2, 511, 511)}),
    "ragged3": (_dims_ragged3, 20481, 14, "ragged", {None: (42, 3, 4), 1: (1, 161, 161)}),
}


@functools.lru_cache(maxsize=None)
def dataset(name):
    """-> (cols uint8 [nvars][N], dims int32); read-only."""
    mk, N, seed, kind, _ = SHAPES[name]
    dims = mk()
    cols, rng = _columns(dims, N, seed, group=8 if kind == "ragged" else None)
    if kind == "stress":
        for v in CONST0:
            cols[v] = 0
        cols[CONST_LAST] = dims[CONST_LAST] - 1
        cols[NEARLY0] = 0
        hits = rng.choice(N, NEARLY0_HITS, replace=False)
        cols[NEARLY0, hits] = 1 + np.arange(NEARLY0_HITS) % (dims[NEARLY0] - 1)
    if kind == "ragged":
        assert dims[EMPTY_STATE_VAR] == 4
        c = cols[EMPTY_STATE_VAR]
        c[c == EMPTY_STATE] = 0
    cols.setflags(write=False)
    dims.setflags(write=False)
    return cols, dims


def lead_offsets(dims):
    """First leading row of every variable (dims - 1 leading rows each) and R."""
    lead0 = np.concatenate([[0], np.cumsum(np.asarray(dims, np.int64) - 1)])
    return lead0[:-1], int(lead0[-1])


def state_offsets(dims):
    off = np.concatenate([[0], np.cumsum(np.asarray(dims, np.int64))])
    return off[:-1], int(off[-1])


def onehot_gram(cols, dims):
    """G = O O^T over all states, float64 (exact)."""
    off, SD = state_offsets(dims)
    N = cols.shape[1]
    O = np.zeros((SD, N), np.float64)
    ar = np.arange(N)
    for v in range(len(dims)):
        O[off[v] + cols[v].astype(np.int64), ar] = 1.0
    return O @ O.T


@functools.lru_cache(maxsize=None)
def reference_gram(name):
    cols, dims = dataset(name)
    G = onehot_gram(cols, dims)
    G.setflags(write=False)
    return G


def pair_index(x, y, nv):
    return x * nv - x * (x + 1) // 2 + (y - x - 1)


def tables_from_gram(G, dims):
    """Every pair (x < y) of the complete graph in lexicographic order -> int32 [P][16], the table of
    x (rows) by y (columns) flattened, cells beyond dx * dy zero."""
    nv = len(dims)
    off, _ = state_offsets(dims)
    P = nv * (nv - 1) // 2
    out = np.zeros((P, 16), np.int32)
    Gi = np.rint(G).astype(np.int64)
    assert (Gi == G).all()
    t = 0
    for x in range(nv):
        dx = int(dims[x])
        rows = Gi[off[x]:off[x] + dx]
        for y in range(x + 1, nv):
            dy = int(dims[y])
            out[t, :dx * dy] = rows[:, off[y]:off[y] + dy].ravel()
            t += 1
    return out


@functools.lru_cache(maxsize=None)
def reference_tables(name):
    _, dims = dataset(name)
    T = tables_from_gram(reference_gram(name), dims)
    T.setflags(write=False)
    return T


def bincount_table(cols, dims, x, y):
    """Brute force: the (x, y) table by np.bincount over the joint code."""
    dx, dy = int(dims[x]), int(dims[y])
    return np.bincount(cols[x].astype(np.int64) * dy + cols[y], minlength=dx * dy)


def row_start(x, nv):
    """Index of the pair (x, x + 1)."""
    return pair_index(x, x + 1, nv)


def range_tiles(dims, pair0, n):
    """nt of the MFMA launch for the pairs [pair0, pair0 + n): the tiles (I, J >= I) of the panels I
    that hold a leading row of the range's x variables (0: those have one state each)."""
    nv = len(dims)
    lead0, R = lead_offsets(dims)
    u0 = max(x for x in range(nv - 1) if row_start(x, nv) <= pair0)
    u1 = max(x for x in range(nv - 1) if row_start(x, nv) <= pair0 + n - 1)
    r0, r1 = int(lead0[u0]), int(lead0[u1] + dims[u1] - 1)
    if r1 <= r0:
        return 0
    nb = (R + TILE - 1) // TILE
    return sum(nb - I for I in range(r0 // TILE, (r1 - 1) // TILE + 1))


def pair_ranges(name):
    """The ranged batches of test_gpu_gram_edges.py on `name` (r257, ragged3): [(label, pair0, n)].
    whole; from the middle of one variable's row of pairs to the middle of a later one's; the rows
    of pairs of the variables of the last panel (ragged3: lead0 >= 512; r257, whose second panel
    holds one row of the straddling variable: that variable's row of pairs, both panels); the row of
    pairs of a 1-state variable (no leading row: no Gram tile at all); the single last pair; whole."""
    _, dims = dataset(name)
    nv = len(dims)
    P = nv * (nv - 1) // 2
    lead0, R = lead_offsets(dims)
    last_panel = (R - 1) // TILE * TILE
    multi = [v for v in range(nv - 1) if dims[v] > 1]
    inside = [v for v in multi if lead0[v] >= last_panel]
    xs = inside if inside else [v for v in multi if lead0[v] + dims[v] - 1 > last_panel]
    one = [v for v in range(1, nv - 1) if dims[v] == 1][0]
    a = row_start(nv // 5, nv) + (nv - nv // 5 - 1) // 2
    b = row_start(nv // 2, nv) + 3
    return [("whole", 0, P), ("mid-row", a, b - a), ("last-panel", row_start(xs[0], nv), P - row_start(xs[0], nv)),
            ("one-state-row", row_start(one, nv), nv - one - 1), ("last-pair", P - 1, 1), ("whole-again", 0, P)]
