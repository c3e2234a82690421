"""The Bayesian Dirichlet scores (BDeu, K2) on the host: hc_bd.h's D and the host twin against a 40-digit
mpmath evaluation, score equivalence of BDeu, the exact zeros.  Bound, the project's for the BIC scorer:
1e-12 of the summed magnitudes, here sum over the non-zero terms of |lnGamma(a + n)| + |lnGamma(a)|.
Worst measured ratio |twin - ref| / (summed magnitudes): 8.7e-16 (D alone: 2.7e-16); DESIGN.md 5.15.

test_gpu_bd.py imports the dataset, the families and the reference of this file."""
import functools

import numpy as np
import pytest

import fastbn_amd as F
from hc_data import ARG, bits_equal

#                   0  1    2  3  4   5   6   7   8   9  10 11
BD_DIMS = np.array([2, 3, 256, 2, 3, 31, 32, 33, 64, 65, 64, 1], np.int32)
BD_NS = [1, 15, 5000]
BD_SCORES = ["k2", ("bde", 1), ("bde", 0.5)]
# q = 1, 2, 3, 31, 32, 33, 64, 65, 4096 for the children with r = 2, 3, 256; then a child with r = 1
BD_FAMILIES = [(c, *ps) for c in (0, 1, 2) for ps in [(), (3,), (4,), (5,), (6,), (7,), (8,), (9,), (10, 8)]]
BD_FAMILIES += [(11,), (11, 3), (11, 8, 10)]


@functools.lru_cache(maxsize=None)
def bd_columns(N):
    rng = np.random.default_rng(7100 + N)
    cols = np.stack([rng.integers(0, d, N) for d in BD_DIMS]).astype(np.uint8)
    # dependent columns: tables far from uniform, large counters beside zeros
    cols[0] = np.where(rng.random(N) < 0.7, cols[8] % 2, cols[0])
    cols[1] = np.where(rng.random(N) < 0.6, (cols[5] + cols[3]) % 3, cols[1])
    cols[2] = np.where(rng.random(N) < 0.5, cols[8] * np.uint8(4), cols[2])
    cols[4] = np.where(rng.random(N) < 0.5, cols[1], cols[4])
    cols.setflags(write=False)
    return cols


def bd_dataset(N):
    return F.Dataset(columns=bd_columns(N), dims=BD_DIMS)


def table(cols, dims, fam):
    """The r x q counts of a family, the parents ascending, by np.bincount."""
    child, ps = fam[0], sorted(fam[1:])
    key, q = np.zeros(cols.shape[1], np.int64), 1
    for p in ps:
        key, q = key * int(dims[p]) + cols[p], q * int(dims[p])
    r = int(dims[child])
    return np.bincount(cols[child].astype(np.int64) * q + key, minlength=r * q).reshape(r, q)


def alphas(score, r, q):
    name, iss = score if isinstance(score, tuple) else (score, 1.0)
    return (1.0, float(r)) if name == "k2" else (iss / (float(r) * float(q)), iss / float(q))


def mp_family(t, score):
    """(score, summed magnitudes) of a counted table from mpmath.loggamma at 40 digits."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 40
    a_cell, a_cfg = alphas(score, *t.shape)
    tot, mag = mp.mpf(0), mp.mpf(0)
    for sign, a, counts in ((1, a_cell, t[t > 0]), (-1, a_cfg, t.sum(0)[t.sum(0) > 0])):
        lga = mp.loggamma(mp.mpf(a))
        for n, times in zip(*np.unique(counts, return_counts=True)):
            lg = mp.loggamma(mp.mpf(a) + int(n))
            tot += sign * int(times) * (lg - lga)
            mag += int(times) * (abs(lg) + abs(lga))
    return tot, mag


@pytest.mark.parametrize("a", [2.0 ** -20, 1 / 1024, 0.5, 1.0, 256.0, 1e4])
def test_lgamma_difference_against_mpmath(a):
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp.clone()
    mp.dps = 40
    T = F.api._bd_lgamma_diff(0, a)[1]
    assert F.api._bd_lgamma_diff(0, a)[0] == 0.0
    for n in (1, 2, T - 1, T, T + 1, 2 ** 24):
        lg, lga = mp.loggamma(mp.mpf(a) + n), mp.loggamma(mp.mpf(a))
        d, mag = F.api._bd_lgamma_diff(n, a)[0], abs(lg) + abs(lga)
        print(f"D({n}, {a}): ratio {float(abs(d - (lg - lga)) / mag) if mag else 0.0:.3g}")
        assert abs(d - (lg - lga)) <= mp.mpf("1e-12") * mag, (n, a)


@pytest.mark.parametrize("score", BD_SCORES, ids=str)
@pytest.mark.parametrize("N", BD_NS)
def test_twin_against_mpmath(N, score):
    pytest.importorskip("mpmath")
    ll, sc = F.family_scores(bd_dataset(N), BD_FAMILIES, score=score)
    assert bits_equal(ll, F.family_scores(bd_dataset(N), BD_FAMILIES)[0])  # the BIC path's log-likelihood bits
    worst = 0.0
    for f, fam in enumerate(BD_FAMILIES):
        ref, mag = mp_family(table(bd_columns(N), BD_DIMS, fam), score)
        if BD_DIMS[fam[0]] == 1:
            assert sc[f] == 0.0  # a child with one state: every term cancels exactly
        assert abs(sc[f] - ref) <= 1e-12 * mag, (fam, sc[f], float(ref))
        worst = max(worst, float(abs(sc[f] - ref) / mag) if mag else 0.0)
    print(f"N = {N}, {score}: worst |twin - ref| / magnitudes = {worst:.3g}")


def check_score_equivalence(iss, wrap=lambda ds: ds):
    """BDeu totals of x -> y and y -> x, and of the three members of a chain's equivalence class, agree within
    the bound; wrap(ds) is the source that is scored (test_gpu_bd.py: an IndependenceTest)."""
    rng = np.random.default_rng(11)
    x = rng.integers(0, 2, 700)
    y = np.where(rng.random(700) < 0.6, x, rng.integers(0, 3, 700))
    z = np.where(rng.random(700) < 0.5, y % 2, rng.integers(0, 2, 700))
    cols = np.stack([x, y, z]).astype(np.uint8)
    ds = F.Dataset(columns=cols, dims=np.array([2, 3, 2], np.int32))
    source = wrap(ds)

    def total(fams):
        sc = F.family_scores(source, fams, score=("bde", iss))[1]
        mags = [mp_family(table(cols, ds.dims, fam), ("bde", iss))[1] for fam in fams]
        return float(sc.sum()), float(sum(mags))

    dags = [[(0,), (1, 0)], [(1,), (0, 1)]]  # x -> y, y -> x
    chain = [[(0,), (1, 0), (2, 1)], [(1,), (0, 1), (2, 1)], [(2,), (1, 2), (0, 1)]]  # x->y->z, x<-y->z, x<-y<-z
    for members in (dags, chain):
        s0, m0 = total(members[0])
        for s, m in [total(m) for m in members[1:]]:
            assert abs(s - s0) <= 1e-12 * (m + m0)


@pytest.mark.parametrize("iss", [1.0, 0.5, 10.0])
def test_bdeu_is_score_equivalent(iss):
    pytest.importorskip("mpmath")
    check_score_equivalence(iss)


@pytest.mark.parametrize("score", BD_SCORES, ids=str)
def test_exact_zeros(score):
    """A table without a sample, which no dataset gives, and a child with one state score exactly 0.0."""
    assert F.api._bd_score_table(np.zeros((3, 70), np.uint32), score) == (0.0, 0.0)
    assert F.api._bd_score_table(np.array([[5, 0, 700, 1]], np.uint32), score) == (0.0, 0.0)


def test_refusals():
    ds = bd_dataset(15)
    for bad in [("bde", 0.0), ("bde", -1.0), ("bde", float("nan")), ("bde", float("inf"))]:
        for call in (lambda: F.family_scores(ds, [(0,)], score=bad), lambda: F.HillClimbing(bad).learn(ds, host=True),
                     lambda: F.ExactSearch(bad, max_parents=1).learn(F.Dataset(columns=bd_columns(15)[:3], dims=BD_DIMS[:3]), host=True)):
            with pytest.raises(F.FastBNError) as e:
                call()
            assert e.value.code == ARG
    with pytest.raises(F.FastBNError):
        F.family_scores(ds, [(0,)], score="bdeu")
    with pytest.raises(F.FastBNError):
        F.family_scores(ds, [(0,)], score=("k2", 2.0))  # K2 has no equivalent sample size
    with pytest.raises(F.FastBNError):
        F.HillClimbing("bdeu").learn(ds, host=True)


def test_searches_on_the_host():
    """The twins' searches under BDeu: a local optimum of the scorer's own bits; the exact optimum is no worse,
    and every node score is family_scores' of the returned family."""
    ds = F.Dataset(columns=bd_columns(5000)[[0, 1, 3, 4, 5]], dims=BD_DIMS[[0, 1, 3, 4, 5]])
    hc = F.HillClimbing(("bde", 1), max_parents=2).learn(ds, host=True)
    ex = F.ExactSearch(("bde", 1), max_parents=2).learn(ds, host=True)
    for res in (hc, ex):
        fams = [(v, *ps) for v, ps in enumerate(res.parents)]
        ll, sc = F.family_scores(ds, fams, score=("bde", 1))
        assert bits_equal(sc, res.node_scores) and bits_equal(ll, res.node_logliks)
    assert hc.iterations > 0 and ex.score >= hc.score
