"""Probability networks (Network.from_cpts / fbn_network_create_cpt: what expectation-maximisation hands
to every inference engine) for test_probnet_host.py and test_gpu_probnet.py, with an exact yardstick.

Each generator is seeded and returns (dims, parents, cpts) in Network.from_cpts' layout: parents[v] in
the node's own order, cpts[v] fp64 [dims[v]][configurations of the ascending parents, last fastest].
A helper module like jt_nets.py: numpy and the standard library, plus the project's host twin for the
`learned` tables.

ExactProb holds every table entry as the exact rational of its double (Fraction(float)) and enumerates
the joint in Fractions: P(e), node marginals, family posteriors and the most probable explanation.  An
fp64 enumeration is no yardstick here: the networks live where its products underflow.

small      7 nodes, 288 joint states: a 1-state node, a 4-state node, two-parent families in descending
           parent order, a v-structure.  Dirichlet tables at concentration 1.0 (benign) or 0.05 (skewed:
           entries down to the floor of 1e-40, renormalised).
shapes     the 15-node shapes graph (1 state, 127 states, six parents, descending parents), Dirichlet(0.3).
learned    ALARM's structure with the theta of three EM iterations of the host twin on incomplete rows.
votes      X0 -> A -> C_0..C_3, all binary; a child observed at 1 costs one value of A a factor 2^-E * r
           with non-dyadic r in (0.2, 0.9).  Two children that vote against different values take a
           junction-tree denominator to about 2^-E: below the kernels' range guards
           with a single table entry per vote.
underflow  three binary nodes whose rare column is t = 2^-k: as one clique ([[], [0], [0, 1]]) the
           initial potential t^3 underflows for k >= 341; as a chain ([[], [0], [1]]) nothing does.
wide       one node with nv - 1 parents, all but a few of one state: a single clique of nv variables and
           at most 256 entries whose multi-state variables sit at slots 0, 7, 8, 15, 16, 23, 24, 31, so
           that every 8-variable digit word of the evidence mask carries evidence.
"""
import functools
import itertools
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

# the shapes graph of test_lbp_host.py / test_gpu_param.py (test_probnet_host.py asserts they are the same)
SHAPES_DIMS = np.array([5, 3, 7, 2, 4, 2, 2, 2, 2, 2, 2, 3, 1, 127, 6], np.int32)
SHAPES_GRAPH = [[], [0], [], [2, 0], [0, 1, 2], [], [], [], [], [], [], [5, 6, 7, 8, 9, 10], [], [12], [1]]

SMALL_DIMS = np.array([2, 3, 1, 4, 2, 3, 2], np.int32)
SMALL_GRAPH = [[], [0], [], [1, 0], [3, 2], [], [5, 4]]  # 3 and 4: descending parents; 5 -> 6 <- 4: a v-structure
SMALL_CONCENTRATIONS = {"benign": 1.0, "skewed": 0.05}
FLOOR = 1e-40

WIDE_SLOTS = (0, 7, 8, 15, 16, 23, 24, 31)
WIDE_SIZES = (17, 25, 32)  # digit words 3 and 4 of the evidence mask, and the last accepted width
WIDE_REFUSED = 33

UNDERFLOW_EXPONENTS = (300, 341, 400)  # t^3 = 2^-900 (normal), 2^-1023 (subnormal), 2^-1200 (zero)

VOTES_CHILDREN = 4
# r[i][a]: non-dyadic, in (0.2, 0.9)
VOTES_R = ((0.23, 0.81), (0.77, 0.31), (0.29, 0.67), (0.59, 0.43))
# Children 0 and 2 vote against A = 0, children 1 and 3 against A = 1: P(C_i = 1 | A = a) = 2^-E * r_ia on
# the side the child votes against, r_ia on the other; E is VOTES_EXP[net][i // 2], one exponent per pair.
# The junction tree normalises as it goes, so a denominator keeps only what both values of A cost: a pair
# observed at 1 leaves 2^-E, a lone vote leaves a tiny marginal and an ordinary denominator.  "guard": the
# second pair trips the 2^-600 guards; "deep": the same pair with the exponent lowered past 2^-900, the
# smallest entry divided staying above the 2^-960 hazard.
VOTES_EXP = {"guard": (300, 700), "deep": (300, 920)}


def npc_of(dims, ps):
    return int(np.prod(np.asarray(dims)[list(ps)], dtype=np.int64))


def dirichlet_cpts(dims, parents, concentration, seed):
    """One Dirichlet(concentration) column per parent configuration, entries floored at FLOOR and the
    column renormalised (a small concentration makes numpy return zeros)."""
    rng = np.random.default_rng(seed)
    out = []
    for v, ps in enumerate(parents):
        d = int(dims[v])
        t = rng.dirichlet(np.full(d, concentration), size=npc_of(dims, ps)).T if d > 1 else np.ones((1, npc_of(dims, ps)))
        t = np.maximum(np.nan_to_num(t, nan=0.0), FLOOR)
        out.append(np.ascontiguousarray(t / t.sum(axis=0)))
    return out


def small(kind="benign", seed=7):
    return SMALL_DIMS.copy(), [list(p) for p in SMALL_GRAPH], dirichlet_cpts(SMALL_DIMS, SMALL_GRAPH, SMALL_CONCENTRATIONS[kind], seed)


def small_forest(kind="benign", seed=7):
    """small with the edge 3 -> 4 removed: two components, {0, 1, 3} and {2, 4, 5, 6}."""
    dims, parents, cpts = small(kind, seed)
    parents[4] = [2]
    cpts[4] = dirichlet_cpts(dims, parents, SMALL_CONCENTRATIONS[kind], seed + 1)[4]
    return dims, parents, cpts


def shapes(seed=15):
    return SHAPES_DIMS.copy(), [list(p) for p in SHAPES_GRAPH], dirichlet_cpts(SHAPES_DIMS, SHAPES_GRAPH, 0.3, seed)


def components(parents):
    """The node sets of the graph's connected components, sorted."""
    comp = list(range(len(parents)))

    def find(a):
        while comp[a] != a:
            comp[a] = comp[comp[a]]
            a = comp[a]
        return a
    for v, ps in enumerate(parents):
        for q in ps:
            comp[find(v)] = find(q)
    groups = {}
    for v in range(len(parents)):
        groups.setdefault(find(v), []).append(v)
    return sorted(groups.values())


def sub_network(dims, parents, cpts, nodes):
    """The network on `nodes` (sorted, closed under parents), renumbered in increasing node order: what the
    single-tree yardstick takes of one component of a disconnected network."""
    idx = {int(v): i for i, v in enumerate(nodes)}
    return (np.asarray(dims, np.int32)[list(nodes)].copy(), [[idx[int(q)] for q in parents[v]] for v in nodes],
            [cpts[v] for v in nodes])


def from_network(net):
    """(dims, parents, cpts) of a Network of either kind, from node_probs (the parents come back ascending)."""
    dims = np.asarray(net.dims, np.int32).copy()
    parents, cpts = [], []
    for v in range(net.num_nodes):
        par, pr = net.node_probs(v)
        parents.append([int(q) for q in par])
        cpts.append(np.ascontiguousarray(pr, np.float64).reshape(int(dims[v]), -1))
    return dims, parents, cpts


LEARNED = dict(rows=300, iters=3, pseudo_count=0.5, sample_seed=17, mask_seed=18, missing=0.3, sampled=2000)


def learned_rows(alarm_net):
    """em_nets.alarm_incomplete()[:300]: forward-sampled ALARM rows with 30 % of the cells missing."""
    rows = alarm_net.forward_sample(LEARNED["sampled"], LEARNED["sample_seed"]).T.astype(np.int8)
    rows[np.random.default_rng(LEARNED["mask_seed"]).random(rows.shape) < LEARNED["missing"]] = -1
    return np.ascontiguousarray(rows[:LEARNED["rows"]])


def learned_em(F, alarm_xml, device=-1):
    """The fitted ExpectationMaximization handle: uniform start on ALARM's structure, three iterations at
    pseudo-count 0.5 on learned_rows.  device -1: the host twin."""
    net = F.Network(alarm_xml)
    parents = [[int(q) for q in net.node_counts(v)[0]] for v in range(net.num_nodes)]
    zeros = [np.zeros((int(net.dims[v]), npc_of(net.dims, ps)), np.int64) for v, ps in enumerate(parents)]
    em = F.ExpectationMaximization(F.Network.from_counts(net.dims, parents, zeros), pseudo_count=LEARNED["pseudo_count"],
                                   device=device)
    obj = em.fit(learned_rows(net), max_iters=LEARNED["iters"], tol=0)
    assert len(obj) == LEARNED["iters"]
    return em


@functools.lru_cache(maxsize=None)
def _learned(alarm_xml):
    import fastbn_amd as F
    dims, parents, cpts = from_network(learned_em(F, alarm_xml).network())
    for c in cpts:
        c.setflags(write=False)
    return dims, parents, cpts


def learned(alarm_xml=None):
    if alarm_xml is None:
        alarm_xml = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alarm", "alarm.xml")
    dims, parents, cpts = _learned(alarm_xml)
    return dims.copy(), [list(p) for p in parents], list(cpts)


def votes(which="guard"):
    """X0 = 0 (the query), A = 1, C_i = 2 + i; see VOTES_EXP.  The complement of a tiny entry is 1.0 in
    fp64 (the column sums to 1 within 2^-300)."""
    n = 2 + VOTES_CHILDREN
    dims = np.full(n, 2, np.int32)
    parents = [[], [0]] + [[1] for _ in range(VOTES_CHILDREN)]
    cpts = [np.array([[0.3], [0.7]]), np.array([[0.6, 0.2], [0.4, 0.8]])]
    for i, r in enumerate(VOTES_R):
        one = np.array(r, np.float64)
        one[i % 2] = np.ldexp(one[i % 2], -VOTES_EXP[which][i // 2])
        cpts.append(np.stack([1.0 - one, one]))
    return dims, parents, cpts


def votes_cases(block, n=64):
    """n cases of one block, cycling through its patterns in a fixed order.  A pattern gives every child
    (unobserved, 0 or 1) and X0 (unobserved, 0 or 1); `ones` are the children observed at 1.
    tripping: ones = {2, 3}, the second pair.  benign: ones within the first pair, or a single one, and the
    other pair's child that votes against the same value observed at 0 -- its own table holds the other
    exponent, and the two would add up in one entry, past 2^-960.  These blocks are the junction tree's: its
    kernels document table values below 2^-960 as out of range.  The patterns left out
    here are not left untested: VOTES_VALUE_UNDERFLOW_ROWS below takes the worst of them to MPE and EM, which
    must refuse it."""
    pats = []
    for x0 in (-1, 0, 1):
        for ch in itertools.product((-1, 0, 1), repeat=VOTES_CHILDREN):
            ones = {i for i, c in enumerate(ch) if c == 1}
            if block == "tripping":
                ok = ones == {2, 3}
            else:
                ok = (ones <= {0, 1} or len(ones) == 1) and all(ch[i ^ 2] == 0 for i in ones)
            if ok:
                pats.append((x0, -1) + ch)
    pats = np.array(pats, np.int8)
    order = np.random.default_rng(len(pats)).permutation(len(pats))
    return np.ascontiguousarray(pats[order[np.arange(n) % len(pats)]])


# All four children observed at 1, X0 unobserved and at 0, for votes("deep"): both values of A cost 2^-1220,
# so every entry of the clique where the messages meet is a potential near 2^-921 times a message entry
# 2^-300 below its row's largest -- 0 in fp64, while the exact P(e) = 2^-1224.1 fits {m, ex}.  No block above
# holds such a row (the junction-tree kernels cannot represent it either); MPE and EM must refuse it.
VOTES_VALUE_UNDERFLOW_ROWS = np.array([[-1, -1, 1, 1, 1, 1], [0, -1, 1, 1, 1, 1]], np.int8)


def votes_blocks():
    """-> namespace(guard, deep: the two networks; benign, tripping: 64 cases each for `guard`; deep_cases:
    the tripping cases, for `deep`)."""
    trip = votes_cases("tripping")
    return SimpleNamespace(guard=votes("guard"), deep=votes("deep"), benign=votes_cases("benign"), tripping=trip,
                           deep_cases=trip.copy())


def underflow(k, chain=False):
    """P(X0 = 1) = P(X1 = 1 | X0 = 1) = P(X2 = 1 | 1, 1) (chain: P(X2 = 1 | X1 = 1)) = t = 2^-k; the other
    columns are ordinary.  P(1, 1, 1) = t^3 in either form."""
    t = 2.0 ** -k
    dims = np.full(3, 2, np.int32)
    if chain:
        return dims, [[], [0], [1]], [np.array([[1 - t], [t]]), np.array([[0.6, 1 - t], [0.4, t]]),
                                       np.array([[0.7, 1 - t], [0.3, t]])]
    return dims, [[], [0], [0, 1]], [np.array([[1 - t], [t]]), np.array([[0.6, 1 - t], [0.4, t]]),
                                     np.array([[0.7, 0.2, 0.5, 1 - t], [0.3, 0.8, 0.5, t]])]


UNDERFLOW_ROWS = np.array([[1, 1, 1], [1, 1, -1], [1, -1, -1], [-1, -1, -1], [0, 1, 1]], np.int8)


def wide(nv, seed=None):
    """Node nv - 1 with the parents 0 .. nv - 2.  The variables at WIDE_SLOTS (below nv) have 2 states (slot
    0: 3 states up to nv = 25), every other one 1 state."""
    dims = np.ones(nv, np.int32)
    for s in WIDE_SLOTS:
        if s < nv:
            dims[s] = 2
    dims[nv - 1] = 2
    if nv <= 25:
        dims[0] = 3
    parents = [[] for _ in range(nv - 1)] + [list(range(nv - 1))]
    return dims, parents, dirichlet_cpts(dims, parents, 0.5, nv if seed is None else seed)


def cases(dims, n, seed, p_observed=0.4):
    """n evidence rows: row 0 observes nothing, row 1 everything, the others each variable with
    probability p_observed, at a uniform state."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims)
    ev = rng.integers(0, 1 << 30, (n, len(dims))) % dims
    hide = rng.random((n, len(dims))) >= p_observed
    hide[0], hide[1 % n] = True, False
    if n == 1:
        hide[0] = True
    ev[hide] = -1
    return ev.astype(np.int8)


def net_tuple(dims, parents, cpts):
    """The (names, dims, parents, cpts) tuple of synth.py's pure-Python samplers (synth.forward_sample and the
    restatements built on it, as test_lbp_host.net_tuple builds it from counts): cpts[v] is [value, GIVEN
    parents...], the entries unchanged."""
    dims = np.asarray(dims, np.int32)
    tabs = []
    for v, ps in enumerate(parents):
        asc = sorted(ps)
        t = np.asarray(cpts[v], np.float64).reshape([dims[v]] + [dims[q] for q in asc])
        tabs.append(np.ascontiguousarray(t.transpose([0] + [1 + asc.index(g) for g in ps])))
    return ["X%d" % v for v in range(len(dims))], dims, [list(p) for p in parents], tabs


class ExactProb:
    """The tables as exact rationals.  Duck-types mpe_nets.ExactNet (V, dims, parents, children, p, prob,
    table, components), so that module's checks take it."""

    def __init__(self, dims, parents, cpts):
        self.V = len(dims)
        self.dims = [int(d) for d in dims]
        self.parents = [sorted(int(q) for q in ps) for ps in parents]
        self.tab = [np.asarray(c, np.float64).reshape(self.dims[v], -1) for v, c in enumerate(cpts)]
        self.off = [0]
        for t in self.tab:
            self.off.append(self.off[-1] + t.size)
        self.cells = self.off[-1]
        self.children = [[] for _ in range(self.V)]
        for v, ps in enumerate(self.parents):
            for q in ps:
                self.children[q].append(v)
        self._frac = [[[Fraction(float(x)) for x in row] for row in t] for t in self.tab]

    @classmethod
    def from_network(cls, net):
        return cls(*from_network(net))

    def config(self, v, x):
        pc = 0
        for q in self.parents[v]:
            pc = pc * self.dims[q] + int(x[q])
        return pc

    def p(self, v, x):
        return self._frac[v][int(x[v])][self.config(v, x)]

    def prob(self, x, nodes=None):
        r = Fraction(1)
        for v in (range(self.V) if nodes is None else nodes):
            r *= self.p(v, x)
        return r

    def table(self, v):
        return self.tab[v].reshape([self.dims[v]] + [self.dims[q] for q in self.parents[v]])

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

    def states(self, ev):
        return itertools.product(*[[int(ev[v])] if ev[v] >= 0 else range(self.dims[v]) for v in range(self.V)])

    def enumerate(self, ev):
        """-> namespace(p_e; marg: per node a list of P(X_v = q | e), all 0 for an observed node (what the
        junction tree reports); post: the family posteriors [cells] in fbn_param_counts' layout; best: max_x
        P(x, e); arg: its arg-max assignments; runner_up: the largest P(x, e) below best, or 0)."""
        z = Fraction(0)
        marg = [[Fraction(0)] * d for d in self.dims]
        post = [Fraction(0)] * self.cells
        best, arg, runner = Fraction(-1), [], Fraction(0)
        npc = [t.shape[1] for t in self.tab]
        for x in self.states(ev):
            p = self.prob(x)
            z += p
            for v in range(self.V):
                marg[v][x[v]] += p
                post[self.off[v] + x[v] * npc[v] + self.config(v, x)] += p
            if p > best:
                runner, best, arg = max(best, Fraction(0)), p, [x]
            elif p == best:
                arg.append(x)
            elif p > runner:
                runner = p
        marg = [[Fraction(0)] * len(m) if ev[v] >= 0 else [q / z for q in m] for v, m in enumerate(marg)]
        return SimpleNamespace(p_e=z, marg=marg, post=[q / z for q in post], best=best,
                               arg=[np.array(a, np.int8) for a in arg], runner_up=runner)

    def marginals_ve(self, ev):
        """Node marginals given ev by variable elimination in Fractions, for graphs whose joint is too large
        to enumerate: for each unobserved node, the other unobserved nodes are summed out in min-degree
        order.  -> (per node a list of Fractions, all 0 for an observed node; P(e))."""
        base = []
        for v in range(self.V):
            sc = [v] + self.parents[v]
            keep = tuple(x for x in sc if ev[x] < 0)
            tab = {}
            for vals in itertools.product(*[range(self.dims[x]) for x in keep]):
                x = {u: int(ev[u]) for u in sc if ev[u] >= 0}
                x.update(zip(keep, vals))
                xs = [x.get(u, 0) for u in range(self.V)]
                tab[vals] = self.p(v, xs)
            base.append((keep, tab))

        def eliminate(factors, target):
            factors = list(factors)
            hidden = set(x for sc, _ in factors for x in sc) - {target}
            while hidden:
                nbr = {h: set() for h in hidden}
                for sc, _ in factors:
                    for h in sc:
                        if h in nbr:
                            nbr[h].update(sc)
                h = min(hidden, key=lambda u: (np.prod([self.dims[y] for y in nbr[u]] or [1]), u))
                mine = [f for f in factors if h in f[0]]
                factors = [f for f in factors if h not in f[0]]
                scope = tuple(sorted(set(x for sc, _ in mine for x in sc) - {h}))
                out = {}
                for vals in itertools.product(*[range(self.dims[x]) for x in scope]):
                    a = dict(zip(scope, vals))
                    s = Fraction(0)
                    for q in range(self.dims[h]):
                        a[h] = q
                        t = Fraction(1)
                        for sc, tab in mine:
                            t *= tab[tuple(a[x] for x in sc)]
                        s += t
                    out[vals] = s
                factors.append((scope, out))
                hidden.discard(h)
            res = [Fraction(1)] * (self.dims[target] if target is not None else 1)
            for sc, tab in factors:
                for q in range(len(res)):
                    res[q] *= tab[(q,) if sc else ()]
            return res

        marg, p_e = [], None
        for v in range(self.V):
            if ev[v] >= 0:
                marg.append([Fraction(0)] * self.dims[v])
                continue
            r = eliminate(base, v)
            z = sum(r)
            assert p_e is None or z == p_e
            p_e = z
            marg.append([q / z for q in r])
        if p_e is None:
            p_e = eliminate(base, None)[0]
        return marg, p_e
