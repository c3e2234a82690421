"""The byte-column CI kernel on variables with more than four states (up to 256).

One variable with five states makes every fast path decline (bit-sliced, 2-bit packed, derived,
Gram, device-resident search): the whole skeleton search then runs through the host-driven level
loop and the plain byte-column instantiation of ci_g2_kernel (ci_kernels.hip).  Each shape below is
the smallest that reaches one branch of that kernel's table storage; every result is held to
references computed here on the CPU, independent of the code under test:

  counts   np.bincount of the raveled index ((z_1 .. z_d last fastest) * dx + x) * dy + y, and the
           reference's own Counts2D / Counts3D tables (tests/golden/widedom.ci.gz)
  df       the reference's rule (src/IndependenceTest.cpp:96-112) on the exact counts
  G^2      the terms 2 o ln(o n_k / (r c)) from the exact integer marginals at 40 digits (mpmath)
  p        1 - P(df / 2, G^2 / 2) at 40 digits, at the device's own G^2 and df
  oracle   the CPU restatement (oracle/pc_oracle.cpp): df, decisions, skeleton, sepsets

Tolerances (derived, not tuned; u = 2^-53):
  G^2 vs mpmath   an in-order double sum of n nonzero terms, each term's log good to a few ulp:
                  |err| <= (n + 8) u sum|t|
                  asserted as it stands on every shape (MI355X: worst ratio 0.55).  Beyond the shape
                  table (the decisions dataset's tests, the 2^24-sample tables) it is missed on
                  tables close to independence: the reference's formula rounds the log's argument
                  twice, 4 u O per term whatever the log's size -- the 2 x 2 pair (1, 6) at 6007
                  samples has G^2 = 0.541, error 3.6e-13 against 1.5e-13.  Those tests allow
                  4 u N on top (g2_bound) and report the ratio to the bare bound.
  G^2 vs oracle   the suite's G2_TOL max(1, |G^2|) (same terms, same order; only log's last bit)
  p               the cancellation in -x + a ln x - lgamma(a) dominates:
                  |err| <= 8 u (x + a |ln x| + |lgamma(a)|) + 4 u
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
from conftest import GOLD, fnv1a_columns, read_ci_blocks

import fastbn_amd as F
import oracle as O
import widedom_data as W

mpmath = pytest.importorskip("mpmath")

pytestmark = pytest.mark.gpu

G2_TOL = 1e-12  # test_gpu_pc.py's bound against the oracle
U = 2.0 ** -53
DPS = 40
LIMIT = -6  # FBN_ERR_LIMIT (include/fastbn.h)

# largest error / bound seen per df decade, printed by the last test of the module
RATIO = {"g2": {}, "g2-beyond-shapes": {}, "p": {}}


def _note(kind, df, ratio):
    dec = 10 ** int(math.floor(math.log10(max(df, 1))))
    RATIO[kind][dec] = max(RATIO[kind].get(dec, 0.0), float(ratio))


# ---- references -------------------------------------------------------------------------------
def ref_table(cols, dims, it):
    """[dimz][dx][dy] in the item's own order: z_1 most significant, z_d fastest (Counts3D)."""
    x, y, z = it[0], it[1], it[2:]
    idx = np.zeros(cols.shape[1], np.int64)
    for v in z:
        idx = idx * int(dims[v]) + cols[v]
    idx = (idx * int(dims[x]) + cols[x]) * int(dims[y]) + cols[y]
    dimz = int(np.prod([int(dims[v]) for v in z], dtype=np.int64)) if len(z) else 1
    return np.bincount(idx, minlength=dimz * int(dims[x]) * int(dims[y])).reshape(dimz, int(dims[x]), int(dims[y]))


def ref_df(T):
    alx = np.maximum(1, (T.sum(axis=2) > 0).sum(axis=1))
    aly = np.maximum(1, (T.sum(axis=1) > 0).sum(axis=1))
    return int(((alx - 1) * (aly - 1)).sum())


_LN = {}


def ref_g2(T):
    """(sum of the terms, sum of their magnitudes, number of nonzero cells) at 40 digits; the log of
    the exact ratio of integers, so a cell with o n_k = r c contributes exactly 0."""
    ni, nj, nk = T.sum(axis=2), T.sum(axis=1), T.sum(axis=(1, 2))
    k, i, j = np.nonzero(T)
    with mpmath.workdps(DPS):
        s = a = mpmath.mpf(0)
        for o, r, c, n in zip(T[k, i, j].tolist(), ni[k, i].tolist(), nj[k, j].tolist(), nk[k].tolist()):
            key = (o * n, r * c)
            ln = _LN.get(key)
            if ln is None:
                ln = _LN[key] = mpmath.log(mpmath.mpf(key[0]) / key[1])
            t = 2 * o * ln
            s += t
            a += abs(t)
    return s, a, len(k)


def ref_p(g2, df):
    with mpmath.workdps(DPS):
        return 1 - mpmath.gammainc(mpmath.mpf(df) / 2, 0, mpmath.mpf(g2) / 2, regularized=True)


def p_bound(g2, df):
    a, x = 0.5 * df, 0.5 * g2
    lnx = abs(math.log(x)) if x > 0 else 0.0
    return 8 * U * (x + a * lnx + abs(math.lgamma(a))) + 4 * U


def g2_bound(nnz, sum_abs, samples=0):
    """(n + 8) u sum|t|: the in-order sum of n terms whose logs are good to a few ulp.  With
    `samples` > 0 also the rounding of the log's ARGUMENT: the kernel forms o / e with e = r c / n_k
    as the reference does (src/IndependenceTest.cpp:112-137), two roundings before the log, each a
    relative u in the argument, i.e. an absolute u in ln and 2 o u in the term 2 o ln(o / e) --
    4 u sum(o) = 4 u N over the table.  On a table close to independence (every ln near 0) that
    exceeds the first part; see the module's shape tests for where the first part alone is
    asserted."""
    return (nnz + 8) * U * float(sum_abs) + 4 * U * samples


def check_test(cols, dims, od, it, g2, df, p, ind, alpha=0.05, arg_rounding=False):
    """One test's device results against every reference.  arg_rounding: G^2 against the 40-digit
    sum with the rounding of the log's argument allowed for (g2_bound), for the tests beyond the
    shape table, which include 2 x 2 tables close to independence."""
    it = [int(v) for v in it]
    g2, df, p, ind = float(g2), int(df), float(p), bool(ind)
    T = ref_table(cols, dims, it)
    rdf = ref_df(T)
    assert df == rdf, (it, df, rdf)
    s, sa, nnz = ref_g2(T)
    err, bound = abs(float(mpmath.mpf(g2) - s)), g2_bound(nnz, sa)
    print("g2 %s df %d nnz %d err %.3e bound %.3e" % (it, df, nnz, err, bound))
    if arg_rounding:
        assert err <= g2_bound(nnz, sa, cols.shape[1]), (it, g2, float(s), err, bound)
    else:
        assert err <= bound, (it, g2, float(s), err, bound)
    _note("g2-beyond-shapes" if arg_rounding else "g2", df, err / bound if bound else 0.0)
    r = od.ci_test(it[0], it[1], it[2:], alpha=alpha)
    assert df == r["df"]
    assert abs(g2 - r["g2"]) <= G2_TOL * max(1.0, abs(r["g2"]))
    assert bool(ind) == r["is_independent"]
    if df == 0:
        assert p == 1.0 and ind
        return
    perr, pb = abs(float(mpmath.mpf(p) - ref_p(g2, df))), p_bound(g2, df)
    print("p  %s df %d g2 %.6g p %.6g err %.3e bound %.3e" % (it, df, g2, p, perr, pb))
    assert perr <= pb, (it, g2, df, p, perr, pb)
    _note("p", df, perr / pb)
    assert bool(ind) == (p > alpha)


def widen(items, n=513):
    """The batch repeated to at least n tests: past kWideTests (512) the kernel runs 256-thread
    workgroups, up to it 1024-thread ones."""
    items = np.asarray(items, np.int32)
    return np.tile(items, (-(-n // len(items)), 1))


def same(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


# ---- the shape datasets, one per sample count, shared by the tests ----------------------------
_ENV = {}


def env(n_samples):
    e = _ENV.get(n_samples)
    if e is None:
        cols, dims, items, byst = W.shape_dataset(n_samples)
        e = _ENV[n_samples] = {
            "cols": cols, "dims": dims, "items": items, "byst": byst,
            "ci": F.IndependenceTest(F.Dataset(columns=cols, dims=dims), 0.05, device=0),
            "od": O.OracleDataset(columns=cols, dims=dims)}
    return e


def with_bystander(e, it):
    """[the test, a test of the 5-state bystander against the same x and z]: the batch keeps the
    byte columns whatever the test's own state counts are."""
    return np.array([it, [e["byst"], it[0]] + list(it[2:])], np.int32)


@pytest.mark.parametrize("shape", W.SHAPE_IDS)
@pytest.mark.parametrize("n_samples", W.SAMPLE_COUNTS)
def test_shape_counts_g2_df_p(n_samples, shape):
    """Every storage branch x every sample loop: the table through ci.counts, then G^2, df, p and the
    decision from a batch of 2 (1024-thread workgroups) and of 514 (256-thread), which must agree
    bit for bit, against the references."""
    e = env(n_samples)
    it = e["items"][shape]
    d = len(it) - 2
    np.testing.assert_array_equal(e["ci"].counts(it[0], it[1], it[2:]),
                                  ref_table(e["cols"], e["dims"], it).reshape(-1))
    items = with_bystander(e, it)
    narrow = e["ci"].run(items, d)
    wide = e["ci"].run(widen(items), d)
    for k in range(2):
        same([a[k::2] for a in wide], [np.full(len(wide[0]) // 2, a[k], a.dtype) for a in narrow])
        check_test(e["cols"], e["dims"], e["od"], items[k], *(a[k] for a in narrow))


def _lds_bytes(dx, dy):
    h = F.lib.load()
    h.fbn_ci_lds_bytes.restype = ctypes.c_size_t
    h.fbn_ci_lds_bytes.argtypes = [ctypes.c_int] * 3
    return h.fbn_ci_lds_bytes(1, dx, dy)


def _static_lds():
    h = F.lib.load()
    h.fbn_ci_static_lds_bytes.restype = ctypes.c_size_t
    h.fbn_ci_static_lds_bytes.argtypes = []
    return h.fbn_ci_static_lds_bytes()


@functools.lru_cache(maxsize=None)
def lds_boundary_shapes():
    """(dx, dy) at d = 0 around the 160 KiB switch from LDS to global tables, from the library's own
    layout size: the largest layout that still fits with the kernel's static LDS, the largest that
    would fit without it (a launch in LDS would exceed the workgroup's 160 KiB), the smallest
    beyond 160 KiB."""
    budget, static = 160 * 1024, _static_lds()
    best = {}
    for dx in range(180, 257):
        for dy in range(150, dx + 1):
            b = _lds_bytes(dx, dy)
            for key, ok, want_max in (("lds-last", b + static <= budget, True),
                                      ("lds-static-window", b <= budget, True), ("global-first", b > budget, False)):
                if ok and (key not in best or (b > best[key][0] if want_max else b < best[key][0])):
                    best[key] = (b, dx, dy)
    return best


@pytest.mark.parametrize("n_samples", [1024, 3001])
def test_lds_to_global_switch(n_samples):
    """The last table in LDS and the first in global memory, by fbn_ci_lds_bytes (the layout contract
    the host sizes the launch by): counts, G^2, df, p for both workgroup sizes."""
    best = lds_boundary_shapes()
    assert best["lds-last"][0] + _static_lds() <= 160 * 1024 < best["global-first"][0]
    assert best["lds-last"][0] > 160 * 1024 - 2048 and best["global-first"][0] < 160 * 1024 + 2048
    shapes = [(k, best[k][1], best[k][2], ()) for k in ("lds-last", "lds-static-window", "global-first")]
    dims, items, byst = W.shape_layout(shapes)
    cols = W.columns(dims, n_samples, 77 + n_samples)
    ci = F.IndependenceTest(F.Dataset(columns=cols, dims=dims), 0.05, device=0)
    od = O.OracleDataset(columns=cols, dims=dims)
    for sid, it in items.items():
        print(sid, best[sid])
        np.testing.assert_array_equal(ci.counts(it[0], it[1]), ref_table(cols, dims, it).reshape(-1))
        batch = np.array([it, [byst, it[0]]], np.int32)
        narrow = ci.run(batch, 0)
        wide = ci.run(widen(batch), 0)
        same([a[0::2] for a in wide], [np.full(len(wide[0]) // 2, a[0], a.dtype) for a in narrow])
        check_test(cols, dims, od, it, *(a[0] for a in narrow))


@pytest.mark.parametrize("n_samples", W.SAMPLE_COUNTS)
def test_batches_mixing_table_sizes_equal_single_tests(n_samples):
    """Tests of one batch share one lds_bytes (the largest layout) while each picks its own number
    of sub-histogram copies: a batch across all classes must return what each test returns alone.
    d = 0 twice: every shape (the 256 x 256 table moves the whole batch to global tables) and the
    shapes that fit LDS."""
    e = env(n_samples)
    by_d = {}
    for sid in W.SHAPE_IDS:
        by_d.setdefault(len(e["items"][sid]) - 2, []).append(e["items"][sid])
    batches = [(d, its) for d, its in sorted(by_d.items())]
    batches.append((0, [it for it in by_d[0] if _lds_bytes(int(e["dims"][it[0]]), int(e["dims"][it[1]])) < 150 * 1024]))
    assert len(batches[-1][1]) < len(by_d[0])
    for d, its in batches:
        items = np.array(its + [[e["byst"], its[0][0]] + its[0][2:]], np.int32)
        for batch in (items, widen(items)):
            got = e["ci"].run(batch, d)
            for k, it in enumerate(its):
                alone = e["ci"].run(with_bystander(e, it), d)
                same([a[k::len(items)] for a in got], [np.full(len(batch) // len(items), a[0], a.dtype) for a in alone])


@pytest.mark.parametrize("n_samples", W.SAMPLE_COUNTS)
def test_production_counts_and_item_order(n_samples):
    """Every test's table of a batch (fbn_ci_debug_counts, d >= 2: the histogram kernel writing
    through cstride), for the items as laid out, with x and y exchanged and with the conditioning
    variables reversed: the table follows the item's order, as Counts3D does.  G^2, df and p of the
    reordered items against the references."""
    e = env(n_samples)
    for sid in ("chunk-two-7x5|11,3", "deep-3x21|2,11,5", "deep-1state-z-6x4|3,1,7,2"):
        it = e["items"][sid]
        d = len(it) - 2
        variants = [it, [it[1], it[0]] + it[2:], it[:2] + it[2:][::-1], [it[1], it[0]] + it[2:][::-1],
                    [e["byst"], it[0]] + it[2:]]
        cap = max(int(np.prod(e["dims"][v])) for v in variants) + 3
        for batch in (np.array(variants, np.int32), widen(variants)):
            got = e["ci"].production_counts(batch, d, cap)
            for k, v in enumerate(batch.tolist()):
                T = ref_table(e["cols"], e["dims"], v).reshape(-1)
                np.testing.assert_array_equal(got[k, :T.size], T)
                assert not got[k, T.size:].any()
        res = e["ci"].run(np.array(variants, np.int32), d)
        for k, v in enumerate(variants):
            check_test(e["cols"], e["dims"], e["od"], v, *(a[k] for a in res))
        # x <-> y leaves G^2's terms in another order, df unchanged
        assert res[1][0] == res[1][1] and res[1][2] == res[1][3]


def test_tables_vs_reference_fixture():
    """The unmodified reference's Counts2D / Counts3D::FillTable (tests/golden/widedom.ci.gz, written
    by make_golden_synth.py widedom) on the shapes of at most 5000 cells, asymmetric and
    unequal-radix ones included, as laid out, with x and y exchanged and with z reversed: the cell
    order for unequal state counts, pinned by the reference itself."""
    blocks = read_ci_blocks(os.path.join(GOLD, "widedom.ci.gz"))
    assert sorted(k[1] for k in blocks) == sorted(W.FIXTURE_SAMPLE_COUNTS)
    total = 0
    for (nvars, n_samples, seed), (fdims, colhash, tests) in blocks.items():
        e = env(n_samples)
        assert seed == W.SHAPE_SEED + n_samples and nvars == len(e["dims"]) and fdims == e["dims"].tolist()
        h = fnv1a_columns(e["cols"])
        assert all(colhash[v] == int(h[v]) for v in range(nvars))
        assert [[x, y] + z for x, y, z, _ in tests] == W.fixture_tests(e["items"])
        by_d = {}
        for x, y, z, counts in tests:
            np.testing.assert_array_equal(e["ci"].counts(x, y, z), counts)
            np.testing.assert_array_equal(ref_table(e["cols"], e["dims"], [x, y] + z).reshape(-1), counts)
            if len(z) >= 2:
                by_d.setdefault(len(z), []).append(([x, y] + z, counts))
        for d, lst in by_d.items():
            cap = max(c.size for _, c in lst)
            got = e["ci"].production_counts(np.array([it for it, _ in lst], np.int32), d, cap)
            for k, (_, c) in enumerate(lst):
                np.testing.assert_array_equal(got[k, :c.size], c)
        total += len(tests)
    assert total >= 60


# ---- decisions --------------------------------------------------------------------------------
_DEC = {}


def decision_env(n_samples, tmp_path_factory):
    e = _DEC.get(n_samples)
    if e is None:
        cols, dims = W.decision_dataset(n_samples, str(tmp_path_factory.mktemp("widedom") / "net.xml"))
        e = _DEC[n_samples] = {"cols": cols, "dims": dims, "od": O.OracleDataset(columns=cols, dims=dims),
                               "ci": F.IndependenceTest(F.Dataset(columns=cols, dims=dims), 0.05, device=0), "ref": {}}
    return e


def oracle_run(e, alpha, gs):
    key = (alpha, gs)
    if key not in e["ref"]:
        e["ref"][key] = e["od"].pc_stable(alpha, 1000, gs, keep_log=True)
    return e["ref"][key]


@pytest.mark.parametrize("gs", [1, 3])
@pytest.mark.parametrize("alpha", [0.001, 0.05, 0.2])
@pytest.mark.parametrize("n_samples", [6007, 6008])
def test_pc_stable_wide_domains(n_samples, alpha, gs, tmp_path_factory, monkeypatch):
    """PC-stable on 24 variables with 1 .. 64 states (scalar and dword sample loops): the host-driven
    level loop over the byte-column kernel, decisions by the band and -- df > 256 from level 0 on --
    by p at both ends of the tree sum's error interval; the same with p evaluated for every test
    (FBN_CI_NO_BAND).  Tests per level, skeleton, sepsets: the restatement's; orientation:
    orient.orient's."""
    import orient
    e = decision_env(n_samples, tmp_path_factory)
    ref = oracle_run(e, alpha, gs)
    assert sorted(set(e["dims"].tolist())) == [1, 2, 3, 5, 7, 11, 21, 64]
    # the branch past the band's df range must have run (else: change the dataset)
    big = [t for t in ref["log"] if t[5] > 256]
    assert big and any(t[7] for t in big) and any(not t[7] for t in big)
    for band in (True, False):
        if not band:
            monkeypatch.setenv("FBN_CI_NO_BAND", "1")
        pc = F.PCStable(alpha, 1000).StructLearnCompData(F.Dataset(columns=e["cols"], dims=e["dims"]), group_size=gs)
        assert pc.path == 0  # host-driven levels
        assert pc.tests_per_level.tolist() == ref["tests_per_level"]
        assert pc.edges == ref["edges"]
        assert pc.sepset == ref["sepset"]
        assert pc.oriented == orient.orient(24, pc.edges, pc.sepset)


@pytest.mark.parametrize("n_samples", [6007, 6008])
def test_level_equals_per_test_decisions(n_samples, tmp_path_factory):
    """IndependenceTest.level (decisions only: tree sum, band, df > nband branch) at d = 0 and 1
    against the decisions run() returns test by test (in-order sum, p evaluated), and run()'s
    G^2, df, p against the references for a sample of the tests, df > 256 included."""
    e = decision_env(n_samples, tmp_path_factory)
    ci, nv = e["ci"], 24
    pairs = np.array([[x, y] for x in range(nv) for y in range(x + 1, nv)], np.int32)
    g2, df, p, ind = ci.run(pairs, 0)
    rm, seps, counted, _ = ci.level(0, pairs, 0, len(pairs))
    np.testing.assert_array_equal(rm, ind)
    assert counted == len(pairs) and (df > 256).any()
    order = np.argsort(df, kind="stable")
    for k in order[::max(1, len(order) // 12)].tolist() + [int(order[-1])]:
        check_test(e["cols"], e["dims"], e["od"], pairs[k], g2[k], df[k], p[k], ind[k], arg_rounding=True)
    edges = pairs[~ind]
    adj = {v: sorted(set(edges[edges[:, 0] == v, 1].tolist()) | set(edges[edges[:, 1] == v, 0].tolist()))
           for v in range(nv)}
    items, owner = [], []
    for k, (x, y) in enumerate(edges.tolist()):
        for z in [z for z in adj[x] if z != y] + [z for z in adj[y] if z != x]:
            items.append([x, y, z])
            owner.append(k)
    g2, df, p, ind = ci.run(np.array(items, np.int32), 1)
    want_rm, want_sep = np.zeros(len(edges), bool), [None] * len(edges)
    for t, k in enumerate(owner):
        if ind[t] and not want_rm[k]:
            want_rm[k], want_sep[k] = True, (items[t][2],)
    rm, seps, _, _ = ci.level(1, edges, 0, len(edges))
    np.testing.assert_array_equal(rm, want_rm)
    assert seps == want_sep
    order = np.argsort(df, kind="stable")
    for k in order[::max(1, len(order) // 12)].tolist() + [int(order[-1])]:
        check_test(e["cols"], e["dims"], e["od"], items[k], g2[k], df[k], p[k], ind[k], arg_rounding=True)


def test_band_delta_far_above_p_error():
    """The decision band trusts p to within delta = alpha / 1024 of alpha for df <= 256 (kBandDfMax):
    delta must exceed 10^6 x the derived bound on p's error at df = 256, at the default alpha, taken
    at the G^2 where p = alpha (the band's edges lie within a few percent of it).  At alpha = 0.001
    the ratio delta / bound is 8.3e5 (printed; the measured error is far smaller, see the report)."""
    for alpha, asserted in ((0.05, True), (0.2, True), (0.001, False)):
        lo, hi = 0.0, 2000.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if ref_p(mid, 256) > alpha else (lo, mid)
        bound = p_bound(1.05 * hi, 256)
        print("alpha %g: G^2 at p = alpha %.2f, p bound %.3e, delta / bound %.3e" % (alpha, hi, bound, alpha / 1024 / bound))
        if asserted:
            assert alpha / 1024 > 1e6 * bound


# ---- 2^24 samples: the packed 16-bit register counters ----------------------------------------
@pytest.mark.parametrize("n_samples", [(1 << 24) - 1024, 1 << 24, (1 << 24) + 4])
def test_packed_counters_at_2_pow_24_samples(n_samples):
    """Tables of <= 16 cells count in 16-bit fields per lane.  In a 256-thread workgroup (batches
    past 512 tests) a lane bins N / 256 samples: 65 536 at N = 2^24, which wraps its field when they
    all fall in one cell.  x: 5 states, y and z1: 1 state, z2: 3 states; first every sample in cell 0,
    then x = 1 on the last 1000 samples and z2 = 1 on the last 500."""
    dims = np.array([5, 1, 1, 3], np.int32)
    cols = np.zeros((4, n_samples), np.uint8)
    item = [0, 1, 2, 3]
    ci = F.IndependenceTest(F.Dataset(columns=cols, dims=dims), 0.05, device=0)
    for batch in (widen([item]), np.array([item, item], np.int32)):
        got = ci.production_counts(batch, 2, 16)
        want = np.zeros(16, np.int32)
        want[0] = n_samples
        np.testing.assert_array_equal(got, np.tile(want, (len(batch), 1)))
    del ci
    cols[0, -1000:] = 1
    cols[3, -500:] = 1
    ci = F.IndependenceTest(F.Dataset(columns=cols, dims=dims), 0.05, device=0)
    # y has one state: df = 0 and every term's log is ln 1; with z2 as y (5 x 3 | 1, 1, packed as
    # well) x and z2 are strongly dependent
    pair = [item, [0, 3, 1, 2]]
    refs = []
    for it in pair:
        T = ref_table(cols, dims, it)
        refs.append((T, ref_df(T)) + ref_g2(T))
    assert refs[0][0].reshape(-1)[[0, 1, 6]].tolist() == [n_samples - 1000, 500, 500]
    assert refs[0][1] == 0 and refs[1][1] == 1
    for batch in (widen(pair), np.array(pair, np.int32)):
        got = ci.production_counts(batch, 2, 16)
        g2, df, p, ind = ci.run(batch, 2)
        for k, (T, rdf, s, sa, nnz) in enumerate(refs):
            np.testing.assert_array_equal(got[k::2, :15], np.tile(T.reshape(-1), (len(batch) // 2, 1)))
            assert (df[k::2] == rdf).all() and (g2[k::2] == g2[k]).all() and (p[k::2] == p[k]).all()
            # (the second item's big cells have ln(o / e) near 0: the argument's rounding counts)
            assert abs(float(mpmath.mpf(float(g2[k])) - s)) <= g2_bound(nnz, sa, n_samples if k else 0)
        assert ind[0] and p[0] == 1.0 and not ind[1]
        assert abs(float(mpmath.mpf(float(p[1])) - ref_p(float(g2[1]), 1))) <= p_bound(float(g2[1]), 1)


# ---- tables beyond the kernel's 32-bit cell indexing ------------------------------------------
def test_oversized_tables_are_refused():
    """dimz * dx * dy past the kernel's int arithmetic: refused on the host with the limit code,
    before any allocation or launch, by run, counts and production_counts; the context still answers
    a small test (256 x 256, value 255 present) afterwards."""
    rng = np.random.default_rng(9)
    dims = np.full(6, 256, np.int32)
    cols = rng.integers(0, 256, (6, 16)).astype(np.uint8)
    cols[:, 0] = 255
    ci = F.IndependenceTest(F.Dataset(columns=cols, dims=dims), 0.05, device=0)
    calls = [lambda: ci.run([[0, 1, 2, 3, 4]], 3), lambda: ci.counts(0, 1, (2, 3, 4)),
             lambda: ci.production_counts([[0, 1, 2, 3, 4]], 3, 16), lambda: ci.run([[0, 1, 2, 3]], 2),
             lambda: ci.run([[0, 1, 2, 3, 4, 5, 0, 1, 2, 3]], 8)]
    for call in calls:
        with pytest.raises(F.FastBNError) as ei:
            call()
        assert ei.value.code == LIMIT
    assert "32-bit" in str(ei.value) or "too large" in str(ei.value)
    it = [0, 1]
    np.testing.assert_array_equal(ci.counts(0, 1), ref_table(cols, dims, it).reshape(-1))
    g2, df, p, ind = ci.run([it], 0)
    check_test(cols, dims, O.OracleDataset(columns=cols, dims=dims), it, g2[0], df[0], p[0], ind[0])


def test_zz_error_ratios_report():
    """Largest error / bound per df decade over this module's run (G^2 against the 40-digit sum,
    p against the 40-digit incomplete gamma): all within 1 by the assertions above; printed for the
    record (DESIGN.md §3 quotes the MI355X figures)."""
    for kind in ("g2", "g2-beyond-shapes", "p"):
        for dec in sorted(RATIO[kind]):
            print("ratio %s df %d..%d: %.3f" % (kind, dec, 10 * dec - 1, RATIO[kind][dec]))
            # (beyond the shape table the ratio is to (n + 8) u sum|t| alone and may pass 1: g2_bound)
            assert RATIO[kind][dec] <= 1.0 or kind == "g2-beyond-shapes"
