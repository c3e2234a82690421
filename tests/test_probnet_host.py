"""Probability networks (Network.from_cpts, what ExpectationMaximization.network() returns) on the CPU:
the restatement of the junction tree built from tables (OracleJT.from_cpts) against exact rationals, the
host twins of the other engines against the same rationals or their restatements, and the range of a
clique's initial potential (include/fastbn.h above fbn_mpe_create / fbn_em_create).

Networks and the yardstick are in tests/prob_nets.py.  test_gpu_probnet.py holds the device kernels to the
restatement and to the host twins checked here."""
import functools
import math
import re
from fractions import Fraction

import numpy as np
import pytest
import em_nets as E
import fastbn_amd as F
import jt_nets as J
import mpe_nets as M
import oracle as O
import prob_nets as P
import test_ais_host as TA
import test_lbp_host as TL
import test_sample_host as TS

# The largest relative error of OracleJT.from_cpts against the exact rationals over every input of this file
# (each test prints its own figure): 1.15e-15 on the six-parent component of the shapes
# graph, 9.0e-16 on its first component, below 5e-16 on the 7-node networks, the 127-state component and the
# votes blocks.  The sums are short and all-positive; 4x covers another order of the same operations (as in
# test_jt_counts_host.py).
MEASURED_REL = 1.15e-15
BOUND = 4 * MEASURED_REL
LIMIT = -6


def _flat(marg):
    return [q for m in marg for q in m]


def _rel(got, exact):
    """Largest relative error of fp64 `got` against Fractions; zeros exactly where the exact value is zero."""
    worst = Fraction(0)
    for g, r in zip(got, exact):
        assert (g != 0) == (r != 0), (g, float(r))
        if r:
            worst = max(worst, abs(Fraction(float(g)) - r) / r)
    return float(worst)


def _label(marg0):
    """The exact label of the query (node 0) and whether its top two are more than 1e-9 (relative) apart."""
    top = sorted(marg0, reverse=True)
    clear = len(top) < 2 or top[0] - top[1] > Fraction(1, 10 ** 9) * top[0]
    return max(range(len(marg0)), key=lambda q: (marg0[q], -q)), clear


def _check_oracle(net, ev, exact_of):
    """-> (largest relative error, cases whose label could not be compared)."""
    lab, marg = O.OracleJT.from_cpts(*net).infer(ev)
    worst, left_out, cache = 0.0, 0, {}
    for i in range(len(ev)):
        key = ev[i].tobytes()
        if key not in cache:
            cache[key] = exact_of(ev[i])
        em = cache[key]
        worst = max(worst, _rel(marg[i], _flat(em)))
        want, clear = _label(em[0])
        if ev[i, 0] >= 0:
            assert lab[i] == 0
        elif clear:
            assert lab[i] == want, i
        else:
            left_out += 1
    return worst, left_out


# ---- the generators
def test_generators_are_what_they_say():
    dims, parents, cpts = P.small("skewed")
    assert len(dims) == 7 and int(np.prod(dims)) <= 2000 and 1 in dims and 4 in dims
    assert any(len(p) == 2 and p == sorted(p, reverse=True) for p in parents)
    assert parents[6] == [5, 4] and 5 not in parents[4] and 4 not in parents[5]  # a v-structure
    allp = np.concatenate([c.reshape(-1) for c in cpts])
    assert allp.min() >= 0.99 * P.FLOOR and (allp < 1e-30).any()
    assert np.concatenate([c.reshape(-1) for c in P.small("benign")[2]]).min() > 1e-6
    assert len(P.components(P.small_forest()[1])) == 2
    np.testing.assert_array_equal(P.SHAPES_DIMS, TL.DIMS)
    assert P.SHAPES_GRAPH == TL.GRAPH
    np.testing.assert_array_equal(P.learned_rows(F.Network(M.XML)), E.alarm_incomplete()[:300])
    for nv in P.WIDE_SIZES + (P.WIDE_REFUSED,):
        d = P.wide(nv)[0]
        assert [s for s in range(nv) if d[s] > 1] == sorted({s for s in P.WIDE_SLOTS if s < nv} | {nv - 1})
        assert int(np.prod(d)) <= 256 or nv == P.WIDE_REFUSED
    for net in (P.small("benign"), P.small("skewed"), P.small_forest(), P.shapes(), P.learned(), P.votes("guard"),
                P.votes("deep"), P.wide(33)) + tuple(P.underflow(k, c) for k in P.UNDERFLOW_EXPONENTS for c in (False, True)):
        pn = F.Network.from_cpts(*net)  # validation: finite, > 0, columns sum to 1
        for v in (0, len(net[0]) - 1):
            assert pn.node_probs(v)[1].tobytes() == np.ascontiguousarray(net[2][v], np.float64).tobytes()


def test_learned_tables_are_three_em_iterations_from_uniform():
    dims, parents, cpts = P.learned()
    em = F.ExpectationMaximization(E.uniform_start(dims, E.alarm_parents()), pseudo_count=0.5, device=-1)
    em.fit(E.alarm_incomplete()[:300], max_iters=3, tol=0)
    assert E.network_bits(em.network()) == E.bits(cpts)
    assert parents == E.alarm_parents() and len(dims) == 37


# ---- the restatement on tables
@pytest.mark.parametrize("kind", sorted(P.SMALL_CONCENTRATIONS))
def test_restatement_vs_exact_small(kind):
    net = P.small(kind)
    ex = P.ExactProb(*net)
    ev = np.concatenate([P.cases(net[0], 16, 3), P.cases(net[0], 8, 4, p_observed=0.8)])
    worst, left_out = _check_oracle(net, ev, lambda e: ex.enumerate(e).marg)
    print("small %s: restatement vs exact, largest relative error %.3g" % (kind, worst))
    assert left_out == 0 and worst <= BOUND


def test_restatement_vs_exact_shapes():
    """Each component of the shapes graph on its own (the restatement builds a single tree), 12 cases, node
    marginals by variable elimination in Fractions."""
    dims, parents, cpts = P.shapes()
    ev = P.cases(dims, 12, 5)
    ev[2, 13], ev[3, 12] = 100, 0  # a state past 64 of the 127-state node; the 1-state node observed
    worst = 0.0
    comps = P.components(parents)
    assert [len(c) for c in comps] == [6, 7, 2]
    for nodes in comps:
        sub = P.sub_network(dims, parents, cpts, nodes)
        ex = P.ExactProb(*sub)
        w, left_out = _check_oracle(sub, np.ascontiguousarray(ev[:, nodes]), lambda e: ex.marginals_ve(e)[0])
        print("shapes component %s: restatement vs exact, largest relative error %.3g" % (nodes, w))
        assert left_out == 0
        worst = max(worst, w)
    assert worst <= BOUND


def test_restatement_vs_exact_votes():
    b = P.votes_blocks()
    for name, net, ev in (("benign", b.guard, b.benign), ("tripping", b.guard, b.tripping), ("deep", b.deep, b.deep_cases)):
        ex = P.ExactProb(*net)
        worst, left_out = _check_oracle(net, ev, lambda e: ex.enumerate(e).marg)
        print("votes %s: restatement vs exact, largest relative error %.3g" % (name, worst))
        assert left_out == 0 and worst <= BOUND


def test_votes_blocks_meet_the_gpu_tests_conditions():
    """What test_gpu_probnet.py relies on, from the restatement's own Normalize statistics."""
    b = P.votes_blocks()
    guard, deep = O.OracleJT.from_cpts(*b.guard), O.OracleJT.from_cpts(*b.deep)
    st = {"benign": guard.infer_stats(b.benign), "tripping": guard.infer_stats(b.tripping), "deep": deep.infer_stats(b.deep_cases)}
    for name, (lab, marg, s) in st.items():
        print("votes %-8s smallest denominator 2^[%.1f, %.1f], largest 2^%.1f, smallest entry 2^%.1f"
              % (name, np.log2(s[:, 0].min()), np.log2(s[:, 0].max()), np.log2(s[:, 1].max()), np.log2(s[:, 2].min())))
        assert len(s) == 64 and np.isfinite(marg).all()
        assert (s[:, 2] > 2.0 ** -940).all()
    for ev in (b.benign, b.tripping):
        assert set(ev[:, 0]) == {-1, 0, 1}  # the query unobserved, at 0 and at 1
    assert (st["benign"][2][:, 0] > 2.0 ** -600).all()
    assert (st["tripping"][2][:, 0] < 2.0 ** -600).all() and (st["tripping"][2][:, 0] > 2.0 ** -900).all()
    assert (st["deep"][2][:, 0] < 2.0 ** -900).all()
    # the benign block reaches marginals below 2^-600 with every denominator in range
    m = st["benign"][1]
    assert m[m > 0].min() < 2.0 ** -600
    # every plan is eligible for the specialized, streamed and tiled kernels
    for net in (b.guard, b.deep):
        info = F.JunctionTree(F.Network.from_cpts(*net), device=-1).info
        assert info["specialized_eligible"] == 1 and info["streamed_eligible"] == 1 and info["tiled_eligible"] == 1


def test_from_cpts_of_a_count_network_reproduces_from_counts():
    net = J.counts_net(J.COUNTS_SEED, "small")
    pn = F.Network.from_counts(net.dims, net.parents, net.counts)
    ev = J.counts_cases(net, 16, 2, seed=3)
    a = O.OracleJT.from_counts(net.dims, net.parents, net.counts)
    b = O.OracleJT.from_cpts(net.dims, net.parents, [pn.node_probs(v)[1] for v in range(pn.num_nodes)])
    for x, y in zip(a.infer_stats(ev), b.infer_stats(ev)):
        assert x.tobytes() == y.tobytes()
    pn = F.Network(M.XML)
    ev = pn.evidence_cases(64, 7, 3)
    dims, parents, cpts = P.from_network(pn)
    for x, y in zip(O.OracleJT(M.XML).infer(ev), O.OracleJT.from_cpts(dims, parents, cpts).infer(ev)):
        assert x.tobytes() == y.tobytes()


# ---- host twins against the rationals
def _twin_nets():
    out = {"small-benign": P.small("benign"), "small-skewed": P.small("skewed")}
    out.update({"wide%d" % nv: P.wide(nv) for nv in P.WIDE_SIZES})
    out.update({"chain%d" % k: P.underflow(k, chain=True) for k in P.UNDERFLOW_EXPONENTS})
    return out


TWIN_NETS = _twin_nets()


@functools.lru_cache(maxsize=None)
def twin_cases(key):
    dims = TWIN_NETS[key][0]
    if key.startswith("chain"):
        return P.UNDERFLOW_ROWS
    ev = P.cases(dims, 10, len(dims))
    ev.setflags(write=False)
    return ev


def check_mpe(net, ev, assign, value):
    """Value = the exact maximum within mpe_nets.bound; the assignment's own exact probability likewise;
    the assignment is the arg-max where the exact runner-up is more than 1e-9 below.  -> cases compared."""
    ex = P.ExactProb(*net)
    b, nclear = M.bound(ex.V), 0
    for c in range(len(ev)):
        p = M.check_case(ex, ev[c], assign[c], value[c])
        r = ex.enumerate(ev[c])
        assert abs(M.value_fraction(value[c]) - r.best) <= b * r.best and p <= r.best
        if len(r.arg) == 1 and r.runner_up < r.best * (1 - Fraction(1, 10 ** 9)):
            nclear += 1
            np.testing.assert_array_equal(assign[c], r.arg[0])
    return nclear


def check_em(net, ev, post, value, b):
    """Family posteriors and P(e) within b (relative) of the rationals; zeros where the exact value is zero."""
    ex = P.ExactProb(*net)
    for c in range(len(ev)):
        r = ex.enumerate(ev[c])
        assert _rel(post[c], r.post) <= b, c
        assert abs(M.value_fraction(value[c]) - r.p_e) <= Fraction(b) * r.p_e, c


@pytest.mark.parametrize("key", sorted(TWIN_NETS))
def test_mpe_host_twin_vs_exact(key):
    net, ev = TWIN_NETS[key], twin_cases(key)
    mpe = F.MostProbableExplanation(F.Network.from_cpts(*net), device=-1)
    assign, value = mpe.value_parts(ev)
    assert check_mpe(net, ev, assign, value) >= len(ev) // 2


@pytest.mark.parametrize("key", sorted(TWIN_NETS))
def test_em_host_twin_vs_exact(key):
    net, ev = TWIN_NETS[key], twin_cases(key)
    em = F.ExpectationMaximization(F.Network.from_cpts(*net), device=-1)
    _, value = em.estep_flat(ev)
    check_em(net, ev, em.debug_posteriors(ev), value, E.bound(em))


def test_a_33_variable_clique_is_refused():
    pn = F.Network.from_cpts(*P.wide(P.WIDE_REFUSED))
    for make in (lambda: F.MostProbableExplanation(pn, device=-1), lambda: F.ExpectationMaximization(pn, device=-1)):
        with pytest.raises(F.FastBNError, match=r"clique with 33 variables \(max 32\)") as e:
            make()
        assert e.value.code == LIMIT


@pytest.mark.parametrize("key", sorted(TWIN_NETS))
def test_lbp_host_twin_vs_restatement(key):
    net = TWIN_NETS[key]
    lbp = F.LoopyBeliefPropagation(F.Network.from_cpts(*net), iterations=4, damping=0.0, device=-1)
    TL.check_against_restatement(lbp, TL.Graph(P.net_tuple(*net)), twin_cases(key)[:4], 4, 0.0)


@pytest.mark.parametrize("method", ["lw", "pls"])
@pytest.mark.parametrize("key", sorted(TWIN_NETS))
def test_lw_pls_host_twin_vs_restatement(key, method):
    net = TWIN_NETS[key]
    lw = F.LikelihoodWeighting(F.Network.from_cpts(*net), 65, seed=5, device=-1, method=method)
    TS.check_against_restatement(lw, P.net_tuple(*net), twin_cases(key)[:5], 65, 5, pls=method == "pls")


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("key", sorted(TWIN_NETS))
def test_ais_host_twin_vs_restatement(key, method):
    net = TWIN_NETS[key]
    h = TA.CLASSES[method](F.Network.from_cpts(*net), 70, max_updates=2, interval=33, seed=4, device=-1)
    TA.check_against_restatement(h, P.net_tuple(*net), twin_cases(key)[:4])


@pytest.mark.parametrize("key", sorted(TWIN_NETS))
def test_epis_host_twin_reduces_to_likelihood_weighting(key):
    """iterations = 0, eps = 0: g = P and c is the cdf row, so the values are LW's (test_epis_host.py's H1); the
    weight takes cdf[d - 1] (within an ulp of 1) per sampled variable: 1e-13 relative, exponents apart."""
    pn = F.Network.from_cpts(*TWIN_NETS[key])
    ev = twin_cases(key)
    val, m, e, lam = F.EPISBN(pn, 130, iterations=0, eps=0.0, seed=3, device=-1).debug_samples(ev, case_offset=5)
    lval, lm, le = F.LikelihoodWeighting(pn, 130, seed=3, device=-1).debug_samples(ev, case_offset=5)
    np.testing.assert_array_equal(val, lval)
    live = lm > 0
    assert (lam == 1.0).all() and ((m > 0) == live).all()
    assert (np.abs(np.ldexp(m[live], (e - le)[live]) - lm[live]) <= 1e-13 * lm[live]).all()


@pytest.mark.parametrize("k", P.UNDERFLOW_EXPONENTS)
def test_epis_host_twin_is_exact_on_the_chain(k):
    """The chain is a polytree, where LBP is exact: every sample weighs the same and log_evidence is log P(e) --
    2^-1200 for the row [1, 1, 1] at t = 2^-400."""
    net = TWIN_NETS["chain%d" % k]
    ex = P.ExactProb(*net)
    S = 1024
    ep = F.EPISBN(F.Network.from_cpts(*net), S, iterations=6, eps=0.0, seed=1, device=-1)
    lab, marg = ep.infer(P.UNDERFLOW_ROWS)
    le, ess, used, res = ep.stats
    for c, row in enumerate(P.UNDERFLOW_ROWS):
        r = ex.enumerate(row)
        lpe = math.log(r.p_e.numerator) - math.log(r.p_e.denominator)
        assert ess[c] >= S * (1 - 1e-9) and abs(le[c] - lpe) <= 1e-10 * max(1.0, abs(lpe)), (c, le[c], lpe)
        assert np.abs(marg[c] - np.array([float(q) for q in _flat(r.marg)])).max() <= 3 / math.sqrt(S)


# ---- the range of a clique's initial potential
def _net(k, chain=False):
    return F.Network.from_cpts(*P.underflow(k, chain))


CREATORS = {"mpe": lambda pn: F.MostProbableExplanation(pn, device=-1), "em": lambda pn: F.ExpectationMaximization(pn, device=-1),
            "jt": lambda pn: F.JunctionTree(pn, device=-1), "forest": lambda pn: F.JunctionForest(pn, device=-1)}


def test_single_clique_potential_in_range_gives_the_exact_value():
    """t = 2^-300: the potential t^3 = 2^-900 is a normal double, and the row [1, 1, 1] has that probability."""
    pn = _net(300)
    _, value = CREATORS["mpe"](pn).value_parts(P.UNDERFLOW_ROWS)
    np.testing.assert_array_equal(value[:3], [[0.5, -899.0], [0.5, -599.0], [0.5, -300.0]])
    em = CREATORS["em"](pn)
    counts, value = em.estep_flat(P.UNDERFLOW_ROWS)
    np.testing.assert_array_equal(value[:3], [[0.5, -899.0], [0.5, -599.0], [0.5, -299.0]])
    assert np.isfinite(counts).all() and np.isfinite(em.debug_posteriors(P.UNDERFLOW_ROWS)).all()
    check_em(P.underflow(300), P.UNDERFLOW_ROWS, em.debug_posteriors(P.UNDERFLOW_ROWS), value, E.bound(em))


@pytest.mark.parametrize("k", [341, 400])
@pytest.mark.parametrize("engine", sorted(CREATORS))
def test_underflowing_clique_potential_is_refused(engine, k):
    """Three nodes in one clique: its potential t^3 is subnormal (k = 341) or zero (k = 400).  Before the
    check, MPE returned the value {0.0, 0.0} for the row [1, 1, 1] and EM {0.0, 0.0} with NaN posteriors --
    three NaN cells in the summed counts of UNDERFLOW_ROWS.  Exact: 2^-1200 = {0.5, -1199} at k = 400."""
    reported = None
    try:
        h = CREATORS[engine](_net(k))
    except F.FastBNError as e:
        assert e.code == LIMIT and re.search(r"clique 0 \(3 variables, node 0 among them\).*underflows", str(e)), e
        return
    if engine == "mpe":
        reported = h.value_parts(P.UNDERFLOW_ROWS)[1][0].tolist()
    elif engine == "em":
        counts, value = h.estep_flat(P.UNDERFLOW_ROWS)
        reported = (value[0].tolist(), "%d NaN cells in the summed counts" % int(np.isnan(counts).sum()))
    pytest.fail("the network was accepted; the row [1, 1, 1] is reported as %s" % (reported,))


@pytest.mark.parametrize("k", P.UNDERFLOW_EXPONENTS)
def test_the_chain_form_does_not_underflow(k):
    """0 -> 1 -> 2: two cliques, no potential below t^2, P(1, 1, 1) = 2^-3k in (m, ex)."""
    pn = _net(k, chain=True)
    for engine in ("jt", "forest"):
        CREATORS[engine](pn)
    _, value = CREATORS["mpe"](pn).value_parts(P.UNDERFLOW_ROWS)
    np.testing.assert_array_equal(value[0], [0.5, 1.0 - 3 * k])
    em = CREATORS["em"](pn)
    counts, value = em.estep_flat(P.UNDERFLOW_ROWS)
    np.testing.assert_array_equal(value[:3], [[0.5, 1.0 - 3 * k], [0.5, 1.0 - 2 * k], [0.5, 1.0 - k]])
    assert np.isfinite(counts).all()


def test_em_never_reports_nan_or_a_zero_mantissa():
    """set_parameters refuses parameters whose potentials underflow and keeps its own; a fit that would pass
    through such parameters stops with the error and keeps the last parameters that passed."""
    em = CREATORS["em"](_net(300))
    before = E.network_bits(em.network())
    with pytest.raises(F.FastBNError, match="underflows") as e:
        em.set_parameters(_net(400))
    assert e.value.code == LIMIT and E.network_bits(em.network()) == before
    counts, value = em.estep_flat(P.UNDERFLOW_ROWS)
    assert np.isfinite(counts).all() and (value[:, 0] >= 0.5).all()
    # an M-step at pseudo-count 1e-310 on five rows that never show state 1: theta(1) = 1e-310 / 5 is a
    # subnormal, and so is the potential that holds it: refused, and the handle keeps the start
    rows = np.zeros((5, 3), np.int8)
    em = F.ExpectationMaximization(_net(300), pseudo_count=1e-310, device=-1)
    with pytest.raises(F.FastBNError, match="underflows") as e:
        em.fit(rows, max_iters=3, tol=0)
    assert e.value.code == LIMIT and E.network_bits(em.network()) == before
    counts, value = em.estep_flat(P.UNDERFLOW_ROWS)
    assert np.isfinite(counts).all() and (value[:, 0] >= 0.5).all()
    # the same fit at a pseudo-count that stays in range runs through
    em = F.ExpectationMaximization(_net(300), pseudo_count=1e-300, device=-1)
    assert len(em.fit(rows, max_iters=3, tol=0)) == 3
    counts, value = em.estep_flat(P.UNDERFLOW_ROWS)
    assert np.isfinite(counts).all() and (value[:, 0] >= 0.5).all()


def check_value_underflow(device):
    """votes("deep") passes every create (its potentials are normal doubles, down to about 2^-921), but with
    all four children observed at 1 every entry of one clique is a potential times a message entry 2^-300
    below its row's largest: 0 in fp64.  The exact P(e) is about 2^-1224 and max_x P(x, e) about 2^-1226, both
    within {m, ex}.  Before the check MPE returned FBN_OK with the value {0.0, 0.0}; now MPE and every EM entry
    that reads values refuse the batch with FBN_ERR_LIMIT naming the case, and EM keeps its parameters."""
    net = P.votes("deep")
    rows = P.VOTES_VALUE_UNDERFLOW_ROWS
    ex = P.ExactProb(*net)
    for row in rows:
        r = ex.enumerate(row)
        assert Fraction(1, 2 ** 1300) < r.best <= r.p_e < Fraction(1, 2 ** 1100)
    pn = F.Network.from_cpts(*net)
    benign = P.votes_cases("benign")[:3]
    mixed = np.concatenate([benign, rows])
    mpe = F.MostProbableExplanation(pn, device=device)
    em = F.ExpectationMaximization(pn, pseudo_count=0.5, device=device)
    before = E.network_bits(em.network())
    assert before == E.bits(net[2])
    calls = {"mpe": mpe.value_parts, "estep": em.estep_flat, "posteriors": em.debug_posteriors,
             "fit": lambda ev: em.fit(ev, max_iters=2, tol=0)}
    for name, call in calls.items():
        for ev, case in ((rows, 0), (mixed, 3)):
            with pytest.raises(F.FastBNError, match=r"case %d: the value underflows inside a clique" % case) as e:
                call(ev)
            assert e.value.code == LIMIT, name
            assert E.network_bits(em.network()) == before, name
    # the handles stay usable, and give what they gave before
    _, value = mpe.value_parts(benign)
    counts, evalue = em.estep_flat(benign)
    assert (value[:, 0] >= 0.5).all() and (evalue[:, 0] >= 0.5).all() and np.isfinite(counts).all()
    check_em(net, benign, em.debug_posteriors(benign), evalue, E.bound(em))
    assert check_mpe(net, benign, *mpe.value_parts(benign)) >= 1


def test_a_value_that_underflows_inside_a_clique_is_refused():
    check_value_underflow(-1)
