"""Order MCMC, host twin (order_mcmc_host.cpp behind fbn_omcmc_run_host): the scan's terms and arc features against
an mpmath evaluation at the edges of the scan, convergence to ArcPosterior's exact arc probabilities, and the
limits.  test_gpu_order_mcmc.py runs the same checks on the device and holds it to the twin bit for bit."""
import functools
import itertools
import math

import mpmath as mp
import numpy as np
import pytest

import fastbn_amd as F
import hc_data as H
from hc_data import ARG, LIMIT

U = 2.0 ** -53  # unit roundoff


@functools.lru_cache(maxsize=None)
def dataset(n, N=300, seed=1):
    """Seeded discrete columns, 2 or 3 states; every odd column leans on its predecessor."""
    rng = np.random.default_rng(seed)
    dims = rng.integers(2, 4, n).astype(np.int32)
    cols = np.stack([rng.integers(0, d, N) for d in dims]).astype(np.uint8)
    for v in range(1, n, 2):
        cols[v] = np.where(rng.random(N) < 0.6, cols[v - 1] % dims[v], cols[v])
    return F.Dataset(columns=cols, dims=dims)


def orders_of(n, seeded):
    rng = np.random.default_rng(n)
    return np.array([np.arange(n), np.arange(n)[::-1]] + [rng.permutation(n) for _ in range(seeded)], np.int32)


def reference(ds, order, k, allowed, prior):
    """(term [n], arcs [n][n], list lengths [n], largest |score|) of one order in 30-digit arithmetic: the subsets
    of pred(v) up to k parents, their scores from family_scores, the prior's term added exactly."""
    n = ds.num_vars
    fams, own = [], []
    for p, v in enumerate(order):
        cand = sorted(int(x) for x in order[:p] if allowed is None or allowed[x][v])
        mine = [(int(v),) + P for size in range(k + 1) for P in itertools.combinations(cand, size)]
        own.append((len(fams), len(mine)))
        fams += mine
    sc = F.family_scores(ds, fams, score="bde")[1]
    term, arcs, lens = [mp.mpf(0)] * n, np.zeros((n, n)), np.zeros(n, int)
    with mp.workdps(30):
        for (f0, cnt), v in zip(own, order):
            s = [mp.mpf(float(sc[f])) - (mp.log(mp.binomial(n - 1, len(fams[f]) - 1)) if prior else 0) for f in range(f0, f0 + cnt)]
            term[v] = mp.log(mp.fsum(mp.exp(x) for x in s))
            row = [mp.mpf(0)] * n
            for x, fam in zip(s, fams[f0:f0 + cnt]):
                for u in fam[1:]:
                    row[u] += mp.exp(x - term[v])
            arcs[:, v] = [float(x) for x in row]
            lens[v] = cnt
    return term, arcs, lens, float(np.abs(sc).max())


def term_bound(n, k, length, term, smax, prior):
    """the exps (below 1 ulp each, their arguments rounded once: at most (2 e^x + 1 / e) U absolute),
    ceil(len / 64) + 6 additions deep, S >= 1, the logarithm below 1 ulp, the final addition; with the indegree
    prior the score is a rounded sum with a logarithm of 1 ulp, which moves every entry of the list."""
    score_err = (smax + 2 * math.log(math.comb(n - 1, min(k, n - 1)))) * U if prior else 0.0
    return 1.01 * ((2 + 0.37 * length + math.ceil(length / 64) + 6 + 2 * math.log(length) + abs(term)) * U + score_err), score_err


# n, max_parents, the forbidden column, prior, seeded orders: lists shorter than a wave and a node with only the
# empty set; 93 entries, a ragged second chunk; exactly 64 entries with bit 63 in use; 2,017 entries, many chunks
SCAN_CASES = [(3, 2, None, 0, 4), (9, 3, None, 0, 4), (64, 1, None, 0, 3), (64, 2, None, 0, 1), (9, 3, 4, 0, 4), (9, 3, None, 1, 4)]


def check_scan(source, host, n, k, forbidden, prior, seeded):
    ds = dataset(n)
    allowed = None
    if forbidden is not None:
        allowed = np.ones((n, n), np.uint8)
        allowed[:, forbidden] = 0
    orders = orders_of(n, seeded)
    term, arcs = F.OrderMCMC("bde", max_parents=k, allowed=allowed, prior=prior).order_terms(orders, source(ds), host=host)
    for i, order in enumerate(orders):
        rt, ra, lens, smax = reference(ds, order, k, allowed, prior)
        for v in range(n):
            tb, score_err = term_bound(n, k, lens[v], float(rt[v]), smax, prior)
            assert abs(mp.mpf(float(term[i, v])) - rt[v]) <= tb, (i, v, term[i, v], rt[v], tb)
            # the weights: the term's error, their own exps, up to len additions in list order, each arc <= 1
            assert np.abs(arcs[i, :, v] - ra[:, v]).max() <= tb + score_err + 1.01 * (2 + 1.37 * lens[v]) * U, (i, v)
        if forbidden is not None:
            assert not arcs[i, :, forbidden].any() and lens[forbidden] == 1


@pytest.mark.parametrize("n,k,forbidden,prior,seeded", SCAN_CASES)
def test_terms_and_arcs_against_mpmath(n, k, forbidden, prior, seeded):
    check_scan(lambda ds: ds, True, n, k, forbidden, prior, seeded)


# chosen on the twin (DESIGN.md 5.18 lists the ratio deviation / se of other seeds)
CONVERGE = dict(max_parents=2, chains=512, burn_in=100, thin=5, samples=60, seed=3)


def check_converged(m, ds, prior):
    exact = F.ArcPosterior("bde", max_parents=2, prior=prior).learn(ds, host=True).arc_prob
    dev = np.abs(m.arc_prob - exact)
    print("largest deviation / se:", (dev[m.arc_se > 0] / m.arc_se[m.arc_se > 0]).max(), "largest se:", m.arc_se.max())
    tb = term_bound(5, 2, 11, 0.0, 1e4, prior)[0] * 4  # an arc feature's bound, generously: far below any se
    assert (dev <= 5 * m.arc_se + tb).all(), (dev / np.maximum(m.arc_se, 1e-300)).max()
    assert m.arc_se.max() < 0.01 and m.accept_rate.min() > 0 and np.isfinite(m.log_score).all()


@pytest.mark.parametrize("prior", ["uniform", "indegree"])
def test_converges_to_exact_posterior(prior):
    ds = dataset(5)
    check_converged(F.OrderMCMC("bde", prior=prior, **CONVERGE).learn(ds, host=True), ds, prior)


@pytest.mark.parametrize("n,kw,code", [(65, {}, LIMIT), (9, {"max_families": 10}, LIMIT), (9, {"chains": 0}, ARG),
                                       (9, {"samples": 0}, ARG), (9, {"thin": 0}, ARG), (9, {"prior": 7}, ARG)])
def test_limits_and_arguments(n, kw, code):
    m = F.OrderMCMC("bde", **{"max_parents": 3, "chains": 2, "burn_in": 1, "thin": 1, "samples": 1, **kw})
    with pytest.raises(F.FastBNError) as e:
        m.learn(dataset(n), host=True)
    assert e.value.code == code and not hasattr(m, "arc_prob")
    if "max_families" in kw:  # 9 nodes of 1 + 8 + 28 + 56 candidates: the count is carried
        assert "837 entries" in str(e.value)


@pytest.mark.parametrize("score", ["bic", "bde"])
def test_column_store_refusals(score):
    mc = F.OrderMCMC(score=score, chains=1, burn_in=0, samples=1, thin=1)
    H.assert_host_prologue_refusals(lambda src: mc.learn(src, host=True))
    H.assert_host_prologue_refusals(lambda src: mc.order_terms([[0, 1, 2]], src, host=True))
