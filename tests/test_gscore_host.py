"""The Gaussian family scores' host twin (fbn_gscore_families_host, fbn_hc_run_gauss_host; no device): against a
40-digit reference, score equivalence, the refusals, and hill climbing against a plain greedy search."""
import itertools
import math

import mpmath
import numpy as np
import pytest

import fastbn_amd as F
import gci_data as G
from fastbn_amd import api as A

mp = mpmath.mpf
SCORES = ["bic", "bge", ("bge", 2.5, 14.0)]


def hyper(score, n, N):
    """(alpha_mu, alpha_w, penalty) of a score name."""
    if score == "bic":
        return None, None, math.log(N) / 2
    am = score[1] if isinstance(score, tuple) else 1.0
    return am, (score[2] if isinstance(score, tuple) else n + am + 1), None


def ref_score(R, ss, N, fam, score):
    """mpmath on the float64 R and ss the twin reads.  bic: ln sigma^2 from the ratio of two determinants.  bge: the
    ratio of the marginal likelihoods of P u v and P in their general form (Kuipers et al. 2014, eq. 2 with nu = the
    sample mean): multivariate gamma functions and det(t I + S)_YY."""
    n, (v, P) = len(ss), (fam[0], sorted(fam[1:]))
    am, aw, pen = hyper(score, n, N)
    if am is None:
        det = lambda Y: mpmath.det(mpmath.matrix(R[np.ix_(Y, Y)].tolist())) if Y else mp(1)
        s2 = mp(ss[v]) * det(P + [v]) / det(P) / N
        return -mp(N) / 2 * (mpmath.log(2 * mpmath.pi) + 1 + mpmath.log(s2)) - mp(pen) * (len(P) + 2)
    am, aw = mp(am), mp(aw)
    t = am * (aw - n - 1) / (am + 1)

    def lml(Y):
        l = len(Y)
        if not l:
            return mp(0)
        M = mpmath.matrix(l, l)
        for a, b in itertools.product(range(l), repeat=2):
            M[a, b] = mp(R[Y[a], Y[b]]) * mpmath.sqrt(mp(ss[Y[a]]) * mp(ss[Y[b]])) + (t if a == b else 0)
        lgam = lambda x: mp(l * (l - 1)) / 4 * mpmath.log(mpmath.pi) + sum(mpmath.loggamma(x - mp(j) / 2) for j in range(l))
        return (mp(l) / 2 * mpmath.log(am / (N + am)) + lgam((N + aw - n + l) / 2) - lgam((aw - n + l) / 2)
                - mp(l * N) / 2 * mpmath.log(mpmath.pi) + (aw - n + l) / 2 * l * mpmath.log(t)
                - (N + aw - n + l) / 2 * mpmath.log(mpmath.det(M)))

    return lml(P + [v]) - lml(P)


def bound(R, N, fam, score, value):
    """64 (p + 1)^2 kappa_2(R_FF) 2^-53 on each ln-pivot, times (c + p + 1) / 2 (bge) or N / 2, plus 8 ulp of
    |score| for the logarithms and sums."""
    p, Fv = len(fam) - 1, sorted(fam)
    am, aw, _ = hyper(score, R.shape[0], N)
    mult = N / 2 if am is None else (N + aw - R.shape[0] + p + 1) / 2
    return 64 * (p + 1) ** 2 * np.linalg.cond(R[np.ix_(Fv, Fv)], 2) * 2.0 ** -53 * mult + 8 * np.spacing(abs(value))


@pytest.fixture(scope="module")
def data10():
    ds = F.ContinuousDataset(columns=G.sem(10, 500, 3, 0.4))
    _, ss, R = A._host_moments(ds)
    rng = np.random.default_rng(5)
    fams = [[int(v) for v in rng.permutation(10)[:1 + p]] for p in range(9) for _ in range(3)]
    return ds, ss, R, fams


@pytest.mark.parametrize("score", SCORES, ids=str)
def test_twin_against_40_digits(data10, score):
    ds, ss, R, fams = data10
    ll, sc = F.family_scores(ds, fams, score=score, host=True)
    ll_bic = F.family_scores(ds, fams, score="loglik", host=True)[1]
    worst = 0.0
    for f, fam in enumerate(fams):
        err = abs(mp(sc[f]) - ref_score(R, ss, 500, fam, score))
        worst = max(worst, float(err) / bound(R, 500, fam, score, sc[f]))
    print(f"{score}: worst error / bound = {worst:.3g}")
    assert worst <= 1.0
    assert (ll.view(np.uint64) == ll_bic.view(np.uint64)).all()  # the loglik output is the Gaussian one under every score
    assert ds.degenerate == 0


@pytest.mark.parametrize("score", SCORES, ids=str)
def test_score_equivalence(score):
    if isinstance(score, tuple):
        score = ("bge", 2.5, 7.0)  # three variables: alpha_w > n + 1 = 4
    ds = F.ContinuousDataset(columns=G.sem(3, 500, 11, 1.0))
    _, ss, R = A._host_moments(ds)
    fams = [[0], [1], [1, 0], [0, 1], [2, 1]]
    sc = F.family_scores(ds, fams, score=score, host=True)[1]
    tol = sum(bound(R, 500, fam, score, s) for fam, s in zip(fams, sc))
    x, y, y_x, x_y, z_y = sc
    assert abs((y_x + x) - (x_y + y)) <= tol
    assert abs((x + y_x + z_y) - (y + x_y + z_y)) <= tol  # the chain x -> y -> z and the fork x <- y -> z


def test_refusals():
    X = G.sem(10, 300, 2, 0.4)
    X[4] = X[1]
    dup = F.ContinuousDataset(columns=X)
    for score in ("bic", "bge"):
        ll, sc = F.family_scores(dup, [[0, 1, 4], [0, 1], [4, 1, 2]], score=score, host=True)
        assert dup.degenerate == 2 and np.isneginf([ll[0], sc[0], ll[2], sc[2]]).all() and np.isfinite([ll[1], sc[1]]).all()
    cases = [(dup, [list(range(10))], "bic", -6),                                      # 9 parents
             (dup, [[0, 1]], ("bge", 1.0, 9.0), -1),                                   # alpha_w <= n - 1
             (F.ContinuousDataset(columns=G.sem(5, 4, 2, 0.4)), [[0, 1, 2]], "bic", -6)]  # N <= p + 2
    for ds, fams, score, code in cases:
        with pytest.raises(F.FastBNError) as e:
            F.family_scores(ds, fams, score=score, host=True)
        assert e.value.code == code
    with pytest.raises(F.FastBNError) as e:
        F.HillClimbing("bic", start=[[1, 4]] + [[]] * 9).learn(dup, host=True)
    assert e.value.code == -1
    with pytest.raises(F.FastBNError):
        F.HillClimbing("bde").learn(dup, host=True)
    with pytest.raises(F.FastBNError):
        F.HillClimbing("bge").learn(F.Dataset(columns=np.zeros((2, 8), np.uint8), dims=[2, 2]), host=True)


def plain_hc(R, ss, N, pen, allowed):
    """Greedy search over numpy-float64 scores with hc_search.cpp's move order (additions, deletions, reversals,
    each by (head y, tail x)) and tie rule (the first maximum) -> (parents, trace, smallest best - runner-up gap)."""
    n, cache = len(ss), {}

    def ls(v, P):
        k = (v, tuple(sorted(P)))
        if k not in cache:
            det = lambda Y: np.linalg.det(R[np.ix_(Y, Y)]) if Y else 1.0
            s2 = ss[v] * det(list(k[1]) + [v]) / det(list(k[1])) / N
            cache[k] = -N / 2 * (math.log(2 * math.pi) + 1 + math.log(s2)) - pen * (len(P) + 2)
        return cache[k]

    par, trace, gap = [set() for _ in range(n)], [], math.inf
    reach = lambda a, b, skip: a == b or any(reach(w, b, skip) for w in range(n) if a in par[w] and (a, w) != skip)
    while True:
        tog = lambda y, x: ls(y, par[y] ^ {x}) - ls(y, par[y])
        moves = [(tog(y, x), 0, x, y) for y in range(n) for x in range(n)
                 if x != y and x not in par[y] and y not in par[x] and allowed[x][y] and not reach(y, x, None)]
        moves += [(tog(y, x), 1, x, y) for y in range(n) for x in sorted(par[y])]
        moves += [(tog(y, x) + tog(x, y), 2, x, y) for y in range(n) for x in sorted(par[y])
                  if allowed[y][x] and not reach(x, y, (x, y))]
        best = max(moves, key=lambda m: m[0], default=(0.0,))
        if best[0] <= 0.0:
            return [sorted(p) for p in par], trace, gap
        gap = min(gap, best[0] - max([m[0] for m in moves if m is not best] + [0.0]))
        d, t, x, y = best
        trace.append((t, x, y))
        par[y] ^= {x}
        if t == 2:
            par[x] ^= {y}


def test_hill_climbing_takes_the_plain_path():
    """Arcs are allowed from the lower to the higher index only: with both directions open the additions x -> y and
    y -> x tie exactly (score equivalence), and no data set separates best from runner-up by the 1e-6 the comparison
    of two differently rounded searches needs."""
    ds = F.ContinuousDataset(columns=G.sem(8, 2000, 4, 0.4))
    _, ss, R = A._host_moments(ds)
    allowed = np.triu(np.ones((8, 8), np.uint8), 1)
    parents, trace, gap = plain_hc(R, ss, 2000, math.log(2000) / 2, allowed)
    assert gap > 1e-6 and len(trace) >= 5  # the precondition, on the reference alone
    hc = F.HillClimbing("bic", allowed=allowed).learn(ds, host=True)
    assert [m[:3] for m in hc.trace] == trace and hc.parents == parents
    assert abs(hc.score - sum(hc.node_scores)) <= 1e-9 * abs(hc.score)
