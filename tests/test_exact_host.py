"""Exact score-optimal structure learning, host twin (exact_host.cpp): the optimum against a brute-force
maximum over every DAG that meets the constraint, and the size edges.  No GPU.

Bound: a family score is within 1e-12 of its summed magnitudes of numpy's (test_hc_host.py), no magnitude
exceeds 2 N ln N, and a DAG's score is the sum of n family scores: n * 1e-12 * 2 N ln N."""
import functools

import numpy as np
import pytest

import fastbn_amd as F
import hc_data as H

CONSTRAINTS = ("none", "max_parents", "mask")


def constraint_kwargs(kind, n):
    if kind == "max_parents":
        return {"max_parents": 1}
    if kind == "mask":  # no arc into variable 0, and not 1 -> 2
        allowed = np.ones((n, n), np.uint8)
        allowed[:, 0] = 0
        allowed[1, 2] = 0
        return {"allowed": allowed}
    return {}


@functools.lru_cache(maxsize=None)
def all_dags(n, kind):
    """Every DAG on n nodes that meets the constraint, [ndags][n] parent bit masks."""
    kw = constraint_kwargs(kind, n)
    options = []
    for v in range(n):
        ok = [m for m in range(1 << n) if not m >> v & 1]
        if "max_parents" in kw:
            ok = [m for m in ok if bin(m).count("1") <= kw["max_parents"]]
        if "allowed" in kw:
            ok = [m for m in ok if all(kw["allowed"][x][v] for x in range(n) if m >> x & 1)]
        options.append(np.array(ok, np.int64))
    pm = np.stack([g.ravel() for g in np.meshgrid(*options, indexing="ij")], axis=1)
    removed = np.zeros(len(pm), np.int64)  # peel off nodes whose parents are all removed, n times
    for _ in range(n):
        for v in range(n):
            removed |= ((pm[:, v] & ~removed) == 0).astype(np.int64) << v
    return pm[removed == (1 << n) - 1]


def brute_force_max(ds, penalty, kind):
    n = ds.num_vars
    dags = all_dags(n, kind)
    total = np.zeros(len(dags))
    for v in range(n):
        fs = {m: H.np_family(ds.columns, ds.dims, (v, *[x for x in range(n) if m >> x & 1]), penalty)[1]
              for m in np.unique(dags[:, v]).tolist()}
        total += np.array([fs[m] for m in dags[:, v].tolist()])
    return float(total.max())


def check_optimum(ex, ds, score, kind):
    """The assertions of a learned result against the brute-force maximum (also test_gpu_exact.py's)."""
    n, N = ds.num_vars, ds.num_instance
    pen = F.hc_penalty(score, N)
    best = brute_force_max(ds, pen, kind)
    bound = n * 1e-12 * 2 * N * np.log(N)
    print(f"n={n} {score} {kind}: score {ex.score!r}, brute force {best!r}, bound {bound:.3g}")
    assert abs(ex.score - best) <= bound
    assert H.is_acyclic(ex.parents) and all(p == sorted(p) for p in ex.parents)
    kw = constraint_kwargs(kind, n)
    assert all(len(p) <= kw.get("max_parents", n) for p in ex.parents)
    if "allowed" in kw:
        assert all(kw["allowed"][x][v] for v, p in enumerate(ex.parents) for x in p)
    ll, sc = F.family_scores(ds, H.families_of(ex.parents), pen)
    assert H.bits_equal(sc, ex.node_scores) and H.bits_equal(ll, ex.node_logliks)
    assert ex.iterations == 0 and ex.trace == []


def leading(ds, n):
    return F.Dataset(columns=np.ascontiguousarray(ds.columns[:n]), dims=np.ascontiguousarray(ds.dims[:n]))


@pytest.mark.parametrize("kind", CONSTRAINTS)
@pytest.mark.parametrize("score", ["bic", "aic"])
@pytest.mark.parametrize("n", [5, 4])
@pytest.mark.parametrize("seed", H.SMALL_SEEDS)
def test_optimum_is_brute_force_maximum(seed, n, score, kind):
    assert len(all_dags(5, "none")) == 29281 and len(all_dags(4, "none")) == 543  # the enumerator itself
    ds = leading(H.small_network(seed)[0], n)
    ex = F.ExactSearch(score, **constraint_kwargs(kind, n)).learn(ds, host=True)
    check_optimum(ex, ds, score, kind)


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_variables(n):
    cols = H.tie_columns()[:n]
    ds = F.Dataset(columns=np.ascontiguousarray(cols), dims=np.full(n, 3, np.int32))
    ex = F.ExactSearch("bic").learn(ds, host=True)
    check_optimum(ex, ds, "bic", "none")
    assert sum(len(p) for p in ex.parents) == n - 1  # identical columns: one arc, either way


def test_more_than_26_variables_is_refused():
    ds = F.Dataset(columns=np.zeros((27, 4), np.uint8), dims=np.full(27, 2, np.int32))
    with pytest.raises(F.FastBNError) as e:
        F.ExactSearch("bic").learn(ds, host=True)
    assert e.value.code == H.LIMIT and "bytes" in str(e.value)


@pytest.mark.parametrize("score", ["bic", "bde"])
def test_column_store_refusals(score):
    H.assert_host_prologue_refusals(lambda src: F.ExactSearch(score=score).learn(src, host=True))
