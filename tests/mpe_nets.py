"""Helpers shared by test_mpe_host.py, test_gpu_mpe.py and test_gpu_mpe_cli.py: exact yardsticks for the
most probable explanation (MostProbableExplanation, fbn_mpe).

A reported value (m, ex) is the exact rational m * 2^ex; it is compared with exact rationals built from
the network's counts (every CPT entry is (count + 1) / (total + |dom|)) with fractions.Fraction.  The
relative bound is 3 * V * 2^-53: at most V CPT divisions, V plan-time multiplies (the initial clique
potentials) and fewer than V message multiplies, each within half an ulp; nothing else rounds (the
rescaling is by powers of two, max and frexp are exact).

Yardsticks: brute-force enumeration of the joint (per component of the graph: the joint of a
disconnected network is the product of its components' joints, so its maximum is the product of their
maxima -- this is what makes the 127-state shapes graph enumerable without shrinking a domain), an exact
Viterbi in Fractions on forests in which every node has at most one parent, and a max-sum variable
elimination in numpy (log domain, greedy min-fill, factors as arrays with named axes)."""
import functools
import math
import os
from fractions import Fraction

import numpy as np
from conftest import ALARM
from test_lbp_host import DIMS, GRAPH, disconnected_network

import fastbn_amd as F

ARG, NODEV, LIMIT = -1, -5, -6  # fbn_err_t (include/fastbn.h)
XML = os.path.join(ALARM, "alarm.xml")


def bound(V):
    return Fraction(3 * V, 2 ** 53)


def value_fraction(value_row):
    """The exact rational m * 2^ex of one value row."""
    m, ex = float(value_row[0]), float(value_row[1])
    assert 0.5 <= m < 1.0 and ex == int(ex), (m, ex)
    return Fraction(m) * Fraction(2) ** int(ex)


class ExactNet:
    """The CPTs of a Network as exact rationals (and as the fp64 tables the library forms from them)."""

    def __init__(self, net):
        self.V = net.num_nodes
        self.dims = [int(d) for d in net.dims]
        self.parents, self.counts, self.totals = [], [], []
        for v in range(self.V):
            par, cnt = net.node_counts(v)
            self.parents.append([int(p) for p in par])  # ascending
            self.counts.append(cnt)
            self.totals.append(cnt.sum(axis=0))
        self.children = [[] for _ in range(self.V)]
        for v, ps in enumerate(self.parents):
            for p in ps:
                self.children[p].append(v)

    def p(self, v, x):
        pc = 0
        for q in self.parents[v]:
            pc = pc * self.dims[q] + int(x[q])
        return Fraction(int(self.counts[v][int(x[v]), pc]) + 1, int(self.totals[v][pc]) + self.dims[v])

    def prob(self, x, nodes=None):
        r = Fraction(1)
        for v in (range(self.V) if nodes is None else nodes):
            r *= self.p(v, x)
        return r

    def table(self, v):
        """fp64 [dims[v]] + [dims of the ascending parents]: (count + 1) / (total + |dom|), one division."""
        t = (self.counts[v] + 1.0) / (self.totals[v] + 1.0 * self.dims[v])
        return t.reshape([self.dims[v]] + [self.dims[q] for q in self.parents[v]])

    def components(self):
        comp = list(range(self.V))

        def find(a):
            while comp[a] != a:
                comp[a] = comp[comp[a]]
                a = comp[a]
            return a
        for v, ps in enumerate(self.parents):
            for q in ps:
                comp[find(v)] = find(q)
        groups = {}
        for v in range(self.V):
            groups.setdefault(find(v), []).append(v)
        return sorted(groups.values())


def check_case(en, ev, assign, value_row):
    """The assignment agrees with the evidence, is complete and in range, and its exact probability
    equals the reported value within the bound.  -> the exact probability."""
    ev, assign = np.asarray(ev), np.asarray(assign)
    assert ((ev < 0) | (assign == ev)).all()
    assert (assign >= 0).all() and (assign < np.asarray(en.dims)).all()
    p = en.prob(assign)
    got = value_fraction(value_row)
    assert abs(got - p) <= bound(en.V) * p, (float(got), float(p), float(abs(got - p) / p))
    return p


def brute_force(en, ev):
    """-> (exact maximum of P(x, e), the list of exact arg-max assignments (None if more than 64 tie),
    clear: the exact runner-up is below (1 - 1e-9) of the maximum in every component).  The fp64 joint
    of each component picks the candidates (within 1e-6 relative of its maximum); those are evaluated
    exactly."""
    best, arg, clear = Fraction(1), [np.zeros(en.V, np.int8)], True
    for comp in en.components():
        pos = {v: i for i, v in enumerate(comp)}
        joint = np.ones([en.dims[v] for v in comp])
        for v in comp:
            sc = [v] + en.parents[v]
            shape = [1] * len(comp)
            for x in sc:
                shape[pos[x]] = en.dims[x]
            joint = joint * en.table(v).transpose(np.argsort(sc)).reshape(shape)
        for v in comp:
            if ev[v] >= 0:
                keep = np.zeros(en.dims[v])
                keep[ev[v]] = 1.0
                shape = [1] * len(comp)
                shape[pos[v]] = en.dims[v]
                joint = joint * keep.reshape(shape)
        cand = np.argwhere(joint >= joint.max() * (1 - 1e-6))
        assert 0 < len(cand) <= 4096
        x = np.zeros(en.V, np.int8)
        exact = []
        for c in cand:
            x[comp] = c
            exact.append((en.prob(x, comp), tuple(int(i) for i in c)))
        exact.sort(key=lambda t: (-t[0], t[1]))
        top = [c for p, c in exact if p == exact[0][0]]
        best *= exact[0][0]
        others = [p for p, c in exact if p != exact[0][0]]
        if others and others[0] >= exact[0][0] * (1 - Fraction(1, 10 ** 9)):
            clear = False
        if arg is not None:
            new = []
            for a in arg:
                for c in top:
                    b = a.copy()
                    b[comp] = c
                    new.append(b)
            arg = new if len(new) <= 64 else None
    return best, arg, clear and arg is not None and len(arg) == 1


def tree_viterbi(en, ev):
    """Exact max-product in Fractions on a forest in which every node has at most one parent.
    -> (maximum of P(x, e), an arg-max assignment, unique: the arg-max was a strict one at every step)."""
    assert all(len(p) <= 1 for p in en.parents)
    order, seen = [], [False] * en.V
    for r in range(en.V):  # parents before children
        if en.parents[r]:
            continue
        stack = [r]
        while stack:
            v = stack.pop()
            order.append(v)
            seen[v] = True
            stack.extend(en.children[v])
    assert all(seen)
    allowed = [[int(ev[v])] if ev[v] >= 0 else list(range(en.dims[v])) for v in range(en.V)]
    cpt = []
    for v in range(en.V):
        tot = en.totals[v]
        cpt.append([[Fraction(int(en.counts[v][q, pc]) + 1, int(tot[pc]) + en.dims[v]) for q in range(en.dims[v])]
                    for pc in range(len(tot))])  # [parent value][value]
    down = [None] * en.V  # down[v][x_v] = max over v's subtree below v
    up = [None] * en.V    # up[v][x_parent] = max over x_v of P(x_v | x_parent) * down[v][x_v]
    for v in reversed(order):
        d = {}
        for q in allowed[v]:
            r = Fraction(1)
            for c in en.children[v]:
                r *= up[c][q]
            d[q] = r
        down[v] = d
        if en.parents[v]:
            up[v] = {pq: max(cpt[v][pq][q] * d[q] for q in allowed[v]) for pq in allowed[en.parents[v][0]]}
    x = np.zeros(en.V, np.int8)
    total, unique = Fraction(1), True
    for v in order:
        pq = int(x[en.parents[v][0]]) if en.parents[v] else 0
        score = {q: cpt[v][pq][q] * down[v][q] for q in allowed[v]}
        mx = max(score.values())
        top = [q for q in allowed[v] if score[q] == mx]
        unique = unique and len(top) == 1
        x[v] = top[0]
        if not en.parents[v]:
            total *= mx
    return total, x, unique


def max_sum_ve(en, ev):
    """log of max_x P(x, e) by variable elimination in numpy: log-domain factors (variables, array with
    one axis per variable), evidence sliced away, greedy min-fill order.  Independent of the junction
    tree: no cliques, no separators, no plan."""
    factors = []
    for v in range(en.V):
        sc = [v] + en.parents[v]
        a = np.log(en.table(v))
        keep = []
        for ax, x in reversed(list(enumerate(sc))):
            if ev[x] >= 0:
                a = np.take(a, int(ev[x]), axis=ax)
            else:
                keep.append(x)
        factors.append((tuple(reversed(keep)), a))
    const = sum(float(a) for sc, a in factors if not sc)
    factors = [(sc, a) for sc, a in factors if sc]
    nbr = {}
    for sc, _ in factors:
        for x in sc:
            nbr.setdefault(x, set()).update(y for y in sc if y != x)
    by_var = {x: [] for x in nbr}
    for i, (sc, _) in enumerate(factors):
        for x in sc:
            by_var[x].append(i)
    alive = [True] * len(factors)
    fill = {}

    def fill_of(x):
        ns = list(nbr[x])
        return sum(1 for i in range(len(ns)) for j in range(i) if ns[j] not in nbr[ns[i]])
    while nbr:
        for x in nbr:
            if x not in fill:
                fill[x] = fill_of(x)
        v = min(nbr, key=lambda x: (fill[x], x))
        ids = [i for i in by_var[v] if alive[i]]
        scope = sorted(set(x for i in ids for x in factors[i][0]))
        pos = {x: k for k, x in enumerate(scope)}
        acc = 0.0
        for i in ids:
            sc, a = factors[i]
            shape = [1] * len(scope)
            for x in sc:
                shape[pos[x]] = en.dims[x]
            acc = acc + a.transpose(np.argsort(sc)).reshape(shape)
            alive[i] = False
        out = acc.max(axis=pos[v])
        rest = tuple(x for x in scope if x != v)
        ns = nbr.pop(v)
        fill.pop(v, None)
        for x in ns:
            nbr[x].discard(v)
            nbr[x].update(y for y in ns if y != x)
        for x in ns:  # the fill of a neighbour, and of a neighbour's neighbour, may have changed
            fill.pop(x, None)
            for y in nbr[x]:
                fill.pop(y, None)
        if rest:
            factors.append((rest, out))
            alive.append(True)
            for x in rest:
                by_var[x].append(len(factors) - 1)
        else:
            const += float(out)
    return const


def ve_tolerance(en, log_p):
    """The number of log terms (one per variable) * 2^-53 * |log p|: every rounding of the max-sum
    elimination -- a log or an add -- is relative to a partial sum no larger than |log p|."""
    return en.V * 2.0 ** -53 * abs(log_p)


def check_no_flip_improves(en, ev, assign, p):
    """No single-variable change of an unobserved variable raises the exact probability (beyond the bound
    that an fp64 arg-max is entitled to)."""
    x = np.array(assign, np.int8)
    for v in range(en.V):
        if ev[v] >= 0:
            continue
        nodes = [v] + en.children[v]
        base = en.prob(x, nodes)
        for q in range(en.dims[v]):
            if q == assign[v]:
                continue
            x[v] = q
            assert en.prob(x, nodes) <= base * (1 + bound(en.V)), (v, q)
        x[v] = assign[v]


# ---- networks (each built once)
@functools.lru_cache(maxsize=None)
def shapes_net():
    """The 15-node shapes graph of test_lbp_host.py; counts in 0..3999 (its 0..39 would make most of the
    127 states of node 13 tie exactly, and an arg-max could not be compared)."""
    rng = np.random.default_rng(15)
    counts = [rng.integers(0, 4000, (int(DIMS[v]), int(np.prod(DIMS[ps], dtype=np.int64)))) for v, ps in enumerate(GRAPH)]
    net = F.Network.from_counts(DIMS, GRAPH, counts)
    return net, ExactNet(net)


@functools.lru_cache(maxsize=None)
def disconnected_net():
    """test_lbp_host.disconnected_network: two polytrees and an isolated node."""
    net = F.Network.from_counts(*disconnected_network())
    return net, ExactNet(net)


# Binary chains X0 -> X1 -> ... with seeded counts in 1..9.  On the 1,200-node chain the exact maximum is
# about 2^-785 with nothing observed, 2^-817 with every 10th node observed and 2^-1111 with all observed
# (a best step has probability ~0.63, a sampled one less): only the last is below 2^-1074, the smallest
# fp64 subnormal.  The 2,000-node chain puts all three cases below it (2^-1300 and less).
CHAIN_SIZES = (1200, 2000)
UNDERFLOW = Fraction(1, 2 ** 1074)


@functools.lru_cache(maxsize=None)
def chain_net(n=1200):
    rng = np.random.default_rng(n)
    dims = np.full(n, 2, np.int32)
    parents = [[]] + [[i - 1] for i in range(1, n)]
    counts = [rng.integers(1, 10, (2, 1 if v == 0 else 2)) for v in range(n)]
    net = F.Network.from_counts(dims, parents, counts)
    return net, ExactNet(net)


@functools.lru_cache(maxsize=None)
def chain_cases(n=1200):
    """None observed, every 10th node observed, all observed (a seeded forward sample)."""
    net, _ = chain_net(n)
    full = net.forward_sample(1, 5).T.astype(np.int8)[0]
    ev = np.full((3, n), -1, np.int8)
    ev[1, ::10] = full[::10]
    ev[2] = full
    ev.setflags(write=False)
    return ev


@functools.lru_cache(maxsize=None)
def chain_viterbi(n=1200):
    _, en = chain_net(n)
    return [tree_viterbi(en, e) for e in chain_cases(n)]


@functools.lru_cache(maxsize=None)
def alarm_net():
    net = F.Network(XML)
    return net, ExactNet(net)


@functools.lru_cache(maxsize=None)
def alarm_cases():
    ev, _ = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)
    ev = ev[:64].copy()
    ev.setflags(write=False)
    return ev


@functools.lru_cache(maxsize=None)
def alarm_ve():
    _, en = alarm_net()
    return [max_sum_ve(en, e) for e in alarm_cases()]


def mixed_cases(net, seed):
    """8 cases: none observed, all observed (two forward samples), k = 1 and k = 3 observed (three each;
    k = 3 clipped to the variables there are)."""
    V = net.num_nodes
    full = net.forward_sample(2, seed).T.astype(np.int8)
    ev = [np.full(V, -1, np.int8), full[0], full[1]]
    ev += list(net.evidence_cases(3, 1, seed + 1)) + list(net.evidence_cases(3, 3, seed + 2))
    ev = np.stack(ev).astype(np.int8)
    ev.setflags(write=False)
    return ev


def check_brute_force(en, ev, assign, value):
    """Value = the brute-force maximum within the bound; the assignment's own exact probability = the value
    within the bound; where the runner-up is clear of the maximum, the assignment is the arg-max.
    -> how many cases were clear."""
    nclear = 0
    for c in range(len(ev)):
        p = check_case(en, ev[c], assign[c], value[c])
        best, arg, clear = brute_force(en, ev[c])
        got = value_fraction(value[c])
        assert abs(got - best) <= bound(en.V) * best
        assert p <= best
        if clear:
            nclear += 1
            np.testing.assert_array_equal(assign[c], arg[0])
    return nclear


def check_chain(n, assign, value):
    """A chain against the exact Viterbi: the exponent is below fp64's range wherever the exact maximum is
    (all three cases at 2,000 nodes, the all-observed one at 1,200), the value is within the bound, and
    the assignment is Viterbi's where Viterbi's arg-max is unique at every step.  -> cases with a unique one."""
    _, en = chain_net(n)
    ev = chain_cases(n)
    nunique, below = 0, []
    for c in range(len(ev)):
        best, x, unique = chain_viterbi(n)[c]
        below.append(best < UNDERFLOW)
        if best < UNDERFLOW:
            assert value[c, 1] < -1074
        p = check_case(en, ev[c], assign[c], value[c])
        got = value_fraction(value[c])
        assert abs(got - best) <= bound(en.V) * best and p <= best
        if unique:
            nunique += 1
            np.testing.assert_array_equal(assign[c], x)
    assert below == ([True] * 3 if n >= 2000 else [False, False, True])
    return nunique


def check_alarm(assign, value, log_p):
    _, en = alarm_net()
    ev = alarm_cases()
    for c in range(len(ev)):
        ve = alarm_ve()[c]
        assert log_p[c] >= ve - ve_tolerance(en, ve), (c, log_p[c], ve)
        p = check_case(en, ev[c], assign[c], value[c])
        check_no_flip_improves(en, ev[c], assign[c], p)


def log_of(value):
    return np.log(value[:, 0]) + value[:, 1] * math.log(2.0)
