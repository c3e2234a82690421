"""Score-based structure learning, host side (hc_search.cpp): the host scorer against numpy, and the
hill-climbing search over it -- the twin the device path (test_gpu_hc.py) is held to bit for bit.  No GPU.

Pinned on ALARM-5000 under BIC from the empty graph: 52 operations (51 additions, 1 deletion), 50 arcs, at
most 2 parents.  A numpy prototype found 53 operations and 51 arcs: the very first step is a tie in exact
arithmetic (adding 2 -> 4 against 4 -> 2), which float64 sums in another order resolve the other way, and
the paths part there.  test_alarm_trace_is_greedy_by_numpy replays the twin's trace against numpy's own
deltas, so the pinned path is checked step by step, not only recorded."""
import numpy as np
import pytest

import fastbn_amd as F
import hc_data as H

ALARM_TRACE_SHA256 = "f1703f2d84afe20fbd93cc2b71a81ff27e407b4bfc4e4df7d5c715c4bc50cd1a"


@pytest.fixture(scope="module")
def alarm():
    ds = F.Dataset(H.ALARM_CSV)
    return ds, F.HillClimbing("bic").learn(ds, host=True)


@pytest.mark.parametrize("N", H.EDGE_NS)
def test_host_score_equals_numpy(N):
    """Within 1e-12 of the summed magnitudes (the two sums cancel), the project's device-log against
    glibc figure for G^2; here both sides use the C library's log and differ in summation order only."""
    ds = H.edge_dataset(N)
    for name in ("bic", "aic", "loglik", 2.5):
        pen = F.hc_penalty(name, N)
        ll, sc = F.family_scores(ds, H.EDGE_FAMILIES, pen)
        for f, fam in enumerate(H.EDGE_FAMILIES):
            rl, rs, mag = H.np_family(ds.columns, ds.dims, fam, pen)
            assert abs(ll[f] - rl) <= 1e-12 * mag, (N, fam, ll[f], rl)
            assert abs(sc[f] - rs) <= 1e-12 * (mag + abs(rs - rl)), (N, fam, sc[f], rs)
    assert F.hc_penalty("bic", N) == np.log(N) / 2 and F.hc_penalty("aic", N) == 1.0 and F.hc_penalty("loglik", N) == 0.0


def test_score_is_a_function_of_the_family_alone():
    ds = H.edge_dataset(1003)
    pen = F.hc_penalty("bic", 1003)
    ll, sc = F.family_scores(ds, H.EDGE_FAMILIES, pen)
    for f in (0, 5, 13, len(H.EDGE_FAMILIES) - 1):
        fam = H.EDGE_FAMILIES[f]
        shuffled = (fam[0],) + tuple(reversed(fam[1:]))
        l1, s1 = F.family_scores(ds, [fam], pen)
        l3, s3 = F.family_scores(ds, [H.EDGE_FAMILIES[0], shuffled, fam], pen)
        assert H.bits_equal(l1, ll[f:f + 1]) and H.bits_equal(s1, sc[f:f + 1])
        assert H.bits_equal(l3[1:], [ll[f]] * 2) and H.bits_equal(s3[1:], [sc[f]] * 2)


def test_family_validation():
    ds = H.edge_dataset(15)
    for bad in ([()], [(13,)], [(0, 13)], [(0, 0)], [(0, 3, 3)], [(0, -1)]):
        with pytest.raises(F.FastBNError) as e:
            F.family_scores(ds, bad, 0.0)
        assert e.value.code == H.ARG, bad
    for pen in (-1.0, float("nan")):
        with pytest.raises(F.FastBNError) as e:
            F.family_scores(ds, [(0,)], pen)
        assert e.value.code == H.ARG
    with pytest.raises(F.FastBNError) as e:  # 256 * 63 * 64 * 65 * 2 cells: past the cap of 2^26
        F.family_scores(ds, [(0,), (2, 3, 4, 5, 0)], 0.0)
    assert e.value.code == H.LIMIT
    assert len(F.family_scores(ds, [], 0.0)[0]) == 0


def test_table_cap_by_sizing_alone():
    assert F.hc_table_bytes(5000) == 8 * 5001 and F.hc_table_bytes(1 << 24) == 8 * ((1 << 24) + 1)
    with pytest.raises(F.FastBNError) as e:
        F.hc_table_bytes((1 << 24) + 1)
    assert e.value.code == H.LIMIT
    with pytest.raises(F.FastBNError) as e:
        F.hc_table_bytes(0)
    assert e.value.code == H.ARG


def test_alarm_bic_pinned(alarm):
    ds, hc = alarm
    assert H.is_acyclic(hc.parents)
    assert hc.iterations == len(hc.trace) == 52
    assert sum(len(p) for p in hc.parents) == 50 and max(len(p) for p in hc.parents) == 2
    assert [t[0] for t in hc.trace].count(0) == 51 and [t[0] for t in hc.trace].count(1) == 1
    assert H.trace_digest(hc.trace) == ALARM_TRACE_SHA256
    assert all(p == sorted(p) for p in hc.parents)
    assert all(t[3] > 0 for t in hc.trace)
    # the total is the sum of the node scores in node order, and the scorer's values for the result
    ll, sc = F.family_scores(ds, H.families_of(hc.parents), F.hc_penalty("bic", ds.num_instance))
    assert H.bits_equal(sc, hc.node_scores) and H.bits_equal(ll, hc.node_logliks)
    total = 0.0
    for x in sc.tolist():
        total += x
    assert total == hc.score
    assert hc.info["batches"] == 53 and hc.families_scored == hc.info["families_scored"] > 37 * 37


def _no_positive_delta(ds, parents, pen, allowed=None, max_parents=None):
    """Exact: the deltas are formed from the scorer's own bits, by the search's own expressions."""
    _, fs = F.family_scores(ds, H.families_of(parents), pen)
    ops = H.neighbours(parents, allowed, max_parents)
    fams, where = [], []
    for t, x, y, new in ops:
        where.append(len(fams))
        fams.append((y, *new[y]))
        if t == 2:
            fams.append((x, *new[x]))
    _, ns = F.family_scores(ds, fams, pen)
    for (t, x, y, _), k in zip(ops, where):
        d = ns[k] - fs[y]
        if t == 2:
            d = d + (ns[k + 1] - fs[x])
        assert not d > 0, (t, x, y, d)
    return len(ops)


def test_alarm_trace_is_greedy_by_numpy(alarm):
    """Every operation of the pinned trace is, by an independent numpy evaluation of every legal operation's
    delta at that step, the best one up to rounding, and numpy finds nothing to improve at the end.  Bound: a
    family score is within 1e-12 of its summed magnitudes on either side (test_host_score_equals_numpy), a
    delta is made of at most four scores, and no magnitude exceeds 2 N ln N."""
    ds, hc = alarm
    n, N = ds.num_vars, ds.num_instance
    pen = F.hc_penalty("bic", N)
    tol = 2 * 4 * 1e-12 * 2 * N * np.log(N)
    memo = {}

    def fam(y, ps):
        k = (y, *sorted(ps))
        if k not in memo:
            memo[k] = H.np_family(ds.columns, ds.dims, k, pen)[1]
        return memo[k]

    def best(par):
        fs = [fam(y, par[y]) for y in range(n)]
        top = 0.0
        for y in range(n):
            for x in range(n):
                if x == y:
                    continue
                if x in par[y]:
                    d = fam(y, par[y] - {x}) - fs[y]
                    top = max(top, d)
                    r = d + fam(x, par[x] | {y}) - fs[x]
                    if r > top and H.is_acyclic([sorted(p - {x}) if v == y else sorted(p | {y}) if v == x else sorted(p)
                                                 for v, p in enumerate(par)]):
                        top = r
                else:
                    d = fam(y, par[y] | {x}) - fs[y]
                    if d > top and H.is_acyclic([sorted(p | {x}) if v == y else sorted(p) for v, p in enumerate(par)]):
                        top = d
        return top

    par = [set() for _ in range(n)]
    assert hc.trace[0][:3] == (0, 2, 4)
    assert abs((fam(4, {2}) - fam(4, ())) - (fam(2, {4}) - fam(2, ()))) <= tol  # the tie the prototype broke the other way
    for t, x, y, d in hc.trace:
        assert abs(best(par) - d) <= tol, (t, x, y, d)
        if t != 0:
            par[y].discard(x)
        if t == 0:
            par[y].add(x)
        elif t == 2:
            par[x].add(y)
    assert [sorted(p) for p in par] == hc.parents
    assert best(par) <= tol


def test_alarm_result_is_a_local_optimum(alarm):
    ds, hc = alarm
    assert _no_positive_delta(ds, hc.parents, F.hc_penalty("bic", ds.num_instance)) > 1000


@pytest.mark.parametrize("seed", H.SMALL_SEEDS)
@pytest.mark.parametrize("score", ["bic", "aic"])
def test_small_network_recovered(score, seed):
    ds, truth = H.small_network(seed)
    hc = F.HillClimbing(score).learn(ds, host=True)
    assert H.is_acyclic(hc.parents)
    assert H.skeleton(hc.parents) == H.skeleton(truth) and len(H.skeleton(truth)) >= 6
    pen = F.hc_penalty(score, ds.num_instance)
    assert _no_positive_delta(ds, hc.parents, pen) >= 10
    # every single-operation neighbour scores no higher, by numpy too (beyond the rounding of a total)
    def total(ps):
        return sum(H.np_family(ds.columns, ds.dims, fam, pen)[1] for fam in H.families_of(ps))
    here = total(hc.parents)
    assert abs(here - hc.score) <= 1e-9 * abs(here)
    for _, _, _, new in H.neighbours(hc.parents):
        assert total(new) <= here + 1e-9 * abs(here)


def test_options_are_honoured(alarm):
    ds, free = alarm
    n = ds.num_vars
    # max_iter: a prefix of the free run
    hc = F.HillClimbing("bic", max_iter=7).learn(ds, host=True)
    assert hc.trace == free.trace[:7] and hc.iterations == 7 and sum(len(p) for p in hc.parents) == 7
    assert F.HillClimbing("bic", max_iter=0).learn(ds, host=True).parents == [[] for _ in range(n)]
    # max_parents
    hc = F.HillClimbing("bic", max_parents=1).learn(ds, host=True)
    assert max(len(p) for p in hc.parents) == 1 and H.is_acyclic(hc.parents)
    assert _no_positive_delta(ds, hc.parents, F.hc_penalty("bic", ds.num_instance), max_parents=1) > 0
    assert F.HillClimbing("bic", max_parents=0).learn(ds, host=True).iterations == 0
    # max_family_cells: inadmissible, never an error
    hc = F.HillClimbing("bic", max_family_cells=12).learn(ds, host=True)
    cells = [int(ds.dims[v]) * int(np.prod(ds.dims[ps], dtype=np.int64)) for v, ps in enumerate(hc.parents)]
    assert max(cells) <= 12 and hc.iterations > 0 and max(int(d) ** 2 for d in ds.dims) > 12
    # allowed: arcs low -> high only (a white list), then nothing at all
    up = np.triu(np.ones((n, n), np.uint8), 1)
    hc = F.HillClimbing("bic", allowed=up).learn(ds, host=True)
    assert hc.iterations > 20 and all(q < v for v, ps in enumerate(hc.parents) for q in ps)
    assert all(t[0] != 2 for t in hc.trace)  # a reversal would add high -> low
    assert _no_positive_delta(ds, hc.parents, F.hc_penalty("bic", ds.num_instance), allowed=up) > 0
    assert F.HillClimbing("bic", allowed=np.zeros((n, n), np.uint8)).learn(ds, host=True).iterations == 0


def test_start_graph(alarm):
    ds, free = alarm
    # from its own result: nothing left to do
    again = F.HillClimbing("bic", start=free.parents).learn(ds, host=True)
    assert again.iterations == 0 and again.parents == free.parents and again.score == free.score
    # from a poor start (a chain 0 -> 1 -> ... in index order): arcs are deleted, the score improves
    chain = [[]] + [[v - 1] for v in range(1, ds.num_vars)]
    start_score = F.HillClimbing("bic", start=chain, max_iter=0).learn(ds, host=True)
    assert start_score.parents == chain
    hc = F.HillClimbing("bic", start=chain).learn(ds, host=True)
    assert hc.score > start_score.score and any(t[0] == 1 for t in hc.trace) and H.is_acyclic(hc.parents)
    assert _no_positive_delta(ds, hc.parents, F.hc_penalty("bic", ds.num_instance)) > 0
    # a start that breaks max_parents is kept; only additions are limited
    two = [[]] * 2 + [[0, 1]] + [[]] * (ds.num_vars - 3)
    hc = F.HillClimbing("loglik", start=two, max_parents=1, max_iter=0).learn(ds, host=True)
    assert hc.parents[2] == [0, 1]


@pytest.mark.parametrize("cap", [12, 2])
def test_start_family_above_max_family_cells(cap):
    """The option limits candidate operations only: a start family above it is scored as the table it is
    (here 27 cells against a cap of 12, then 2), never as a clamped size."""
    ds = F.Dataset(columns=H.tie_columns(), dims=np.array([3, 3, 3], np.int32))
    start = [[], [], [0, 1]]
    pen = F.hc_penalty("bic", ds.num_instance)
    at = F.HillClimbing("bic", start=start, max_family_cells=cap, max_iter=0).learn(ds, host=True)
    ll, sc = F.family_scores(ds, H.families_of(start), pen)
    assert at.parents == start and H.bits_equal(at.node_scores, sc) and H.bits_equal(at.node_logliks, ll)
    hc = F.HillClimbing("bic", start=start, max_family_cells=cap).learn(ds, host=True)
    assert H.is_acyclic(hc.parents) and hc.score >= at.score
    _, sc = F.family_scores(ds, H.families_of(hc.parents), pen)
    assert H.bits_equal(hc.node_scores, sc)
    for v, ps in enumerate(hc.parents):  # whatever changed fits the cap
        assert ps == start[v] or 3 ** (1 + len(ps)) <= cap
    if cap == 2:
        assert hc.iterations == 0  # any family a 3-state node could change to has 9 cells or more
    else:
        assert hc.iterations > 0 and all(t[0] != 0 or t[2] != 2 for t in hc.trace)


def test_errors():
    ds, _ = H.small_network(H.SMALL_SEEDS[0])
    cyc = [[1], [2], [0], [], []]
    for kw in (dict(start=cyc), dict(allowed=np.ones((5, 4))), dict(score=-0.5), dict(score=float("nan")),
               dict(start=[[0], [], [], [], []]), dict(start=[[7], [], [], [], []])):
        with pytest.raises(F.FastBNError) as e:
            F.HillClimbing(**kw).learn(ds, host=True)
        assert e.value.code == H.ARG, kw
    with pytest.raises(F.FastBNError) as e:
        F.hc_penalty("bdeu", 100)
    assert e.value.code == H.ARG
    bad = F.Dataset(columns=np.full((2, 8), 3, np.uint8), dims=np.array([2, 4], np.int32))
    with pytest.raises(F.FastBNError) as e:  # a code >= its state count would index past a table
        F.HillClimbing().learn(bad, host=True)
    assert e.value.code == H.ARG


def test_exact_ties_go_to_the_lowest_operation():
    """Columns 0 and 1 are identical: the families (0 | 1) and (1 | 0) have the same table, so their scores
    are the same bits, and adding 1 -> 0 ties exactly with adding 0 -> 1; the head 0 comes first.  Every
    family of column 2 over column 0 has a twin over column 1: x = 0 is scanned before x = 1."""
    ds = F.Dataset(columns=H.tie_columns(), dims=np.array([3, 3, 3], np.int32))
    pen = F.hc_penalty("bic", ds.num_instance)
    _, sc = F.family_scores(ds, [(0, 1), (1, 0), (0,), (1,), (2, 0), (2, 1)], pen)
    assert sc[0] == sc[1] and sc[2] == sc[3] and sc[4] == sc[5]
    hc = F.HillClimbing("bic").learn(ds, host=True)
    assert hc.trace[0][:3] == (0, 1, 0)
    assert hc.trace[0][3] == sc[0] - sc[2]
    assert len(hc.trace) >= 2 and (0, 1, 2) not in [t[:3] for t in hc.trace]
    assert H.skeleton(hc.parents) in ({(0, 1), (0, 2)}, {(0, 1), (1, 2)})
