"""Exact arc posteriors, host twin (exact_bma_host.cpp over exact_lse.h): log Z and every arc against a plain
mpmath enumeration of all n! orders at 40 digits, the size edges, and the two functions of the arithmetic on
their own.  No GPU.

Bound (the issue's): errors of a log-sum-exp grow with chain depth, not breadth; the longest chain is two
transforms and n levels of at most n terms, each step losing a few units in the last place of a magnitude at
most sum_v max|ls_v|:  tol(logZ) = 4 (n^2 + 2n) 2^-53 sum_v max|ls_v| over the finite scores; an arc and
q_v[{}] add the 2^n roundings of the linear sum, 2^n 2^-53."""
import functools
import itertools
import math

import mpmath
import numpy as np
import pytest

import fastbn_amd as F
import hc_data as H
from test_exact_host import CONSTRAINTS, constraint_kwargs

mpmath.mp.dps = 40
INF = float("inf")


@functools.lru_cache(maxsize=None)
def order_reference(seed, score, kind, prior):
    """(log Z, P [n][n], sum_v max|ls_v|) by enumeration of every order of small_network(seed), in mpmath."""
    ds = H.small_network(seed)[0]
    n = ds.num_vars
    kw = constraint_kwargs(kind, n)
    cands = []  # (v, parent mask) of every candidate family, in one scorer call
    for v in range(n):
        for m in range(1 << n):
            ps = [x for x in range(n) if m >> x & 1]
            if m >> v & 1 or len(ps) > kw.get("max_parents", n) or ("allowed" in kw and not all(kw["allowed"][x][v] for x in ps)):
                continue
            cands.append((v, m))
    fams = [(v, *[x for x in range(n) if m >> x & 1]) for v, m in cands]
    bd = score in ("bde", "k2")
    sc = F.family_scores(ds, fams, 0.0 if bd else F.hc_penalty(score, ds.num_instance), score if bd else None)[1]
    ls, mag = {}, [0.0] * n
    for (v, m), s in zip(cands, sc):
        k = bin(m).count("1")
        ls[v, m] = mpmath.mpf(float(s)) - (mpmath.log(mpmath.binomial(n - 1, k)) if prior else 0)
        mag[v] = max(mag[v], abs(float(ls[v, m])))

    @functools.lru_cache(maxsize=None)
    def factor(v, pred, u):  # the sum of exp(ls_v[T]) over the candidates T within pred (with u in T unless u < 0)
        return mpmath.fsum(mpmath.exp(x) for (w, m), x in ls.items() if w == v and not m & ~pred and (u < 0 or m >> u & 1))

    Z, arc = mpmath.mpf(0), [[mpmath.mpf(0)] * n for _ in range(n)]
    for order in itertools.permutations(range(n)):
        pred, seen = {}, 0
        for v in order:
            pred[v], seen = seen, seen | 1 << v
        f = {v: factor(v, pred[v], -1) for v in range(n)}
        Z += mpmath.fprod(f.values())
        for v in range(n):
            rest = mpmath.fprod(f[w] for w in range(n) if w != v)
            for u in range(n):
                if pred[v] >> u & 1:
                    arc[u][v] += rest * factor(v, pred[v], u)
    return mpmath.log(Z), [[a / Z for a in row] for row in arc], sum(mag)


def check_against_orders(res, seed, score, kind, prior):
    """The assertions of a learned result against the order enumeration (also test_gpu_bma.py's)."""
    logZ, P, mag = order_reference(seed, score, kind, prior)
    n = len(P)
    bound = 4 * (n * n + 2 * n) * 2.0 ** -53 * mag
    pbound = bound + 2.0 ** n * 2.0 ** -53
    ez = abs(mpmath.mpf(res.log_z) - logZ)
    ep = max(abs(mpmath.mpf(float(res.arc_prob[u][v])) - P[u][v]) for u in range(n) for v in range(n))
    eq = max(abs(q - 1.0) for q in res.q_empty)
    print(f"seed {seed} {score} {kind} prior {prior}: logZ {res.log_z!r} err/bound {float(ez / bound):.3g}, "
          f"arcs {float(ep / pbound):.3g}, q {eq / pbound:.3g}, |B[V]-F[V]| {abs(res.b_full - res.log_z) / bound:.3g}")
    assert ez <= bound and abs(mpmath.mpf(res.b_full) - logZ) <= bound and abs(res.b_full - res.log_z) <= bound
    assert ep <= pbound and eq <= pbound
    assert (np.diag(res.arc_prob) == 0).all() and (res.skeleton_prob == res.arc_prob + res.arc_prob.T).all()
    kw = constraint_kwargs(kind, n)
    if "allowed" in kw:
        assert (res.arc_prob[kw["allowed"] == 0] == 0).all()  # exactly


@pytest.mark.parametrize("prior", [0, 1])
@pytest.mark.parametrize("kind", CONSTRAINTS)
@pytest.mark.parametrize("score", ["bde", "bic"])
@pytest.mark.parametrize("seed", H.SMALL_SEEDS)
def test_twin_is_order_enumeration(seed, score, kind, prior):
    ds = H.small_network(seed)[0]
    res = F.ArcPosterior(score, prior=prior, **constraint_kwargs(kind, ds.num_vars)).learn(ds, host=True)
    check_against_orders(res, seed, score, kind, prior)


def test_one_and_two_variables():
    cols = H.tie_columns()
    one = F.Dataset(columns=np.ascontiguousarray(cols[:1]), dims=np.full(1, 3, np.int32))
    r = F.ArcPosterior("bde").learn(one, host=True)
    assert r.arc_prob.tolist() == [[0.0]] and r.q_empty.tolist() == [1.0]
    assert r.log_z == r.b_full == F.family_scores(one, [(0,)], score="bde")[1][0]
    two = F.Dataset(columns=np.ascontiguousarray(cols[:2]), dims=np.full(2, 3, np.int32))
    r = F.ArcPosterior("bde").learn(two, host=True)
    s = [mpmath.mpf(float(x)) for x in F.family_scores(two, [(0,), (1,), (0, 1), (1, 0)], score="bde")[1]]
    e0, e1, a01, a10 = (mpmath.exp(x) for x in (s[0], s[1], s[3], s[2]))  # a01: the arc 0 -> 1, the family (1, 0)
    Z = e0 * (e1 + a01) + e1 * (e0 + a10)  # the orders (0, 1) and (1, 0)
    tol = 4 * 8 * 2.0 ** -53 * float(max(abs(s[0]), abs(s[2])) + max(abs(s[1]), abs(s[3])))
    assert abs(mpmath.mpf(r.log_z) - mpmath.log(Z)) <= tol and abs(r.b_full - r.log_z) <= tol
    assert abs(mpmath.mpf(float(r.arc_prob[0][1])) - e0 * a01 / Z) <= tol + 4 * 2.0 ** -53
    assert abs(mpmath.mpf(float(r.arc_prob[1][0])) - e1 * a10 / Z) <= tol + 4 * 2.0 ** -53
    assert r.arc_prob[0][0] == r.arc_prob[1][1] == 0 and max(abs(r.q_empty - 1)) <= tol + 4 * 2.0 ** -53


def test_more_than_26_variables_is_refused():
    ds = F.Dataset(columns=np.zeros((27, 4), np.uint8), dims=np.full(27, 2, np.int32))
    with pytest.raises(F.FastBNError) as e:
        F.ArcPosterior("bde").learn(ds, host=True)
    assert e.value.code == H.LIMIT and "bytes" in str(e.value)


LN2 = math.log(2.0)
# each cutoff and range-reduction boundary (k + 1/2) ln 2 from both sides, the ends of the range, a tiny argument
EXP_ARGS = [0.0, -2.0 ** -60, -1.0, -708.0, -707.999, -745.0] + [s * (k + 0.5) * LN2 for k in (0, 1, 52, 1020) for s in (-1 + 1e-15, -1 - 1e-15)]


@pytest.mark.parametrize("x", EXP_ARGS)
def test_lse_exp(x):
    """Within 1 ulp (2^-52 relative: the polynomial's stated error; the 2^k scaling is exact); 0 below -708."""
    y = F.api._lse_exp(x)
    assert y == 1.0 if x == 0 else 0 <= y <= 1
    assert y == 0.0 if x < -708.0 else abs(mpmath.mpf(y) - mpmath.exp(x)) <= 2.0 ** -52 * mpmath.exp(x)
    assert F.api._lse_exp(np.nextafter(-708.0, -INF)) == 0.0 and F.api._lse_exp(-INF) == 0.0


@pytest.mark.parametrize("a,b", [(0.0, -37.0), (-5.0, -5.0), (-3000.25, -3001.0), (-1.0, 1.0), (-1e4, -1e4 + 36.9), (2.0 ** -30, 0.0)])
def test_lse(a, b):
    """e^d within 2^-52, 1 + e rounded (2^-52), the logarithm's ulp and the last add: 2^-50 + 2^-52 |result|."""
    ref = mpmath.log(mpmath.exp(a) + mpmath.exp(b))
    assert abs(mpmath.mpf(F.api._lse(a, b)) - ref) <= 2.0 ** -50 + 2.0 ** -52 * abs(ref)
    assert F.api._lse(a, b) == F.api._lse(b, a)
    # the cutoffs: an absent operand, and a difference past -37 (e^-37 < 2^-53), return the larger unchanged
    assert F.api._lse(a, -INF) == a and F.api._lse(-INF, a) == a and F.api._lse(-INF, -INF) == -INF
    assert F.api._lse(a, np.nextafter(a - 37.0, -INF)) == a


@pytest.mark.parametrize("score", ["bic", "bde"])
def test_column_store_refusals(score):
    H.assert_host_prologue_refusals(lambda src: F.ArcPosterior(score=score).learn(src, host=True))
