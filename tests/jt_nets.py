"""Networks for the junction-tree range-guard and count-map tests (test_jt_counts_host.py,
test_gpu_jt_range.py, test_gpu_jt_counts.py), with exact rational references.  Plain Python and
numpy: no GPU, no library of the project.

conflict_net: two chains of binary variables vote against each other on one variable A.  Every
observed chain variable costs one value of A a factor of about 2^-31 (XMLBIF form) or exactly 2^-62
in doubles (counts form), so the clique where the two opinions meet is normalized by a denominator
of about 2^-(factor * min(b, c)) when the first b and c variables of the chains are observed: far
below the 2^-600 the kernels' fast division is checked against, while every
marginal stays a normal double.

counts_net: small seeded networks that XMLBIF cannot express: counts above 10000, all-zero parent
configurations, a 1-state node, a parent list in descending order, a 32 / 33 / 127-state variable.
"""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

CONFLICT_FORMS = {"xmlbif": (32, 31), "counts": (16, 62)}  # conflict_net(K, log2_factor) of the tests
XMLBIF_ENTRY = "200000"  # the TABLE entry of the XMLBIF form: count (int)(200000 * 10000) = 2e9


def _xml_count(tok):
    return int(float(tok) * 10000)  # the loader's truncation


def conflict_net(K, log2_factor):
    """The conflict network with chains of length K.  Variables: X0 = 0 (the query), A = 1,
    B0..B(K-1) = 2..K+1, C0..C(K-1) = K+2..2K+1, all binary.  log2_factor 31: the XMLBIF form (count
    2e9 written as TABLE entry 200000; .xml holds the document); any other value: the counts form
    with one count of 2**log2_factor per row (.xml is None).
    -> namespace(K, H, dims, parents, counts, xml, bits): bits = log2(H + 2), what one observed chain
    variable costs."""
    xmlform = log2_factor == 31
    H = _xml_count(XMLBIF_ENTRY) if xmlform else 2 ** log2_factor
    n = 2 + 2 * K
    dims = [2] * n
    prior = ["0.3", "0.7"]
    a_tab = ["0.6", "0.2", "0.4", "0.8"]  # [A][X0]
    parents = [[], [0]]
    counts = [np.array([[_xml_count(t)] for t in prior], np.int64),
              np.array([_xml_count(t) for t in a_tab], np.int64).reshape(2, 2)]
    tables = [prior, a_tab]
    for chain, likes in ((0, 1), (1, 0)):  # the B chain votes for A = 1, the C chain for A = 0
        for i in range(K):
            v = 2 + chain * K + i
            ps = [1] if i == 0 else [1, v - 1]
            reps = 1 if i == 0 else 2  # the previous chain variable does not matter
            # counts[value][A (, previous)]: value 1 has count H where A = likes, value 0 elsewhere
            row1 = [H if a == likes else 0 for a in (0, 1) for _ in range(reps)]
            row0 = [H - x for x in row1]
            parents.append(ps)
            counts.append(np.array([row0, row1], np.int64))
            tables.append([XMLBIF_ENTRY if x else "0" for x in row0 + row1])
    xml = None
    if xmlform:
        out = ['<?xml version="1.0" encoding="UTF-8"?>\n<BIF>\n<NETWORK>\n<NAME>conflict%d</NAME>\n' % K]
        for v in range(n):
            out.append("<VARIABLE>\n<NAME>X%d</NAME>\n<TYPE>discrete</TYPE>\n<VALUE>s0</VALUE>\n<VALUE>s1</VALUE>\n"
                       "</VARIABLE>\n" % v)
        for v in range(n):
            out.append("<PROBABILITY>\n<FOR>X%d</FOR>\n" % v)
            out += ["<GIVEN>X%d</GIVEN>\n" % p for p in parents[v]]
            out.append("<TABLE>%s </TABLE>\n</PROBABILITY>\n" % " ".join(tables[v]))
        out.append("</NETWORK>\n</BIF>\n")
        xml = "".join(out)
    return SimpleNamespace(K=K, H=H, dims=dims, parents=parents, counts=counts, xml=xml, bits=math.log2(H + 2))


def conflict_cases(net, cases):
    """Evidence int8 [len(cases)][2 + 2K]: case (b, c) observes B0..B(b-1) and C0..C(c-1) at 1; a
    case (b, c, x) observes the query X0 = x too."""
    ev = np.full((len(cases), 2 + 2 * net.K), -1, np.int8)
    for i, case in enumerate(cases):
        b, c = case[:2]
        ev[i, 2:2 + b] = 1
        ev[i, 2 + net.K:2 + net.K + c] = 1
        if len(case) > 2:
            ev[i, 0] = case[2]
    return ev


def conflict_exact(net, b, c, x0=-1):
    """The exact posteriors (X0, A) of case (b, c) or (b, c, x0) as Fractions (X0's are zeros when it
    is observed, as the junction tree reports them).  Given A, the observed prefixes are plain
    products and the unobserved suffixes sum to 1: a sum over four (X0, A) terms."""
    cx, ca, H = net.counts[0], net.counts[1], net.H
    px = [Fraction(int(cx[x, 0]) + 1, int(cx[:, 0].sum()) + 2) for x in (0, 1)]
    pa = [[Fraction(int(ca[a, x]) + 1, int(ca[:, x].sum()) + 2) for x in (0, 1)] for a in (0, 1)]  # [a][x]
    hi, lo = Fraction(H + 1, H + 2), Fraction(1, H + 2)
    like = [lo ** b * hi ** c, hi ** b * lo ** c]  # P(observed prefixes | A = a)
    w = [[px[x] * pa[a][x] * like[a] if x0 in (-1, x) else Fraction(0) for a in (0, 1)] for x in (0, 1)]  # [x][a]
    tot = sum(w[0]) + sum(w[1])
    post_x = [Fraction(0)] * 2 if x0 >= 0 else [sum(w[x]) / tot for x in (0, 1)]
    return post_x, [(w[0][a] + w[1][a]) / tot for a in (0, 1)]


def conflict_entry_bits(net, b, c):
    """-log2 of the smallest table entry a Normalize divides in case (b, c), to about a bit (the
    oracle's own figure is asserted in test_jt_counts_host.py).  The side that loses the vote holds
    2^-(bits * max(b, c)); and a clique {A, Bi, Bi+1} with neither chain variable observed holds the
    entry P(Bi = 1 | A = 0) P(Bi+1 = 1 | A = 0) = 2^-(2 bits) of its own, which the other chain's
    message multiplies: with min(b, c) < 2 that is the smaller one."""
    m, M = min(b, c), max(b, c)
    return net.bits * max(M + 0.1, M + 2 - m)


def conflict_blocks(net):
    """The blocks of 64 cases the range-guard tests use, by what the oracle's smallest Normalize
    denominator, about 2^-(bits * min(b, c)), is to be (test_jt_counts_host.py asserts it):
      benign   all denominators above 2^-100: one-sided and shallow prefixes, as long as the
               smallest divided entry allows (marginals down to 2^-867 and 2^-806);
      tripping below 2^-600 (and above 2^-900);
      deep     below 2^-900 and above 2^-1000.
    Every case keeps the smallest divided entry above 2^-940 (conflict_entry_bits), clear of the
    2^-960 that is the documented limit of the kernels' division; that leaves
    one deep (b, c).  Tripping and deep cases, and the benign ones too, come with the query
    unobserved, observed at 0 and observed at 1."""
    K, bits = net.K, net.bits
    shallow = int(90 // bits)  # min(b, c) * bits well inside 100
    pairs = [(b, c) for b in range(K + 1) for c in range(K + 1) if conflict_entry_bits(net, b, c) <= 940]
    with_x = lambda ps: [p + x for p in ps for x in ((), (0,), (1,))]  # noqa: E731
    benign = with_x([p for p in pairs if min(p) <= shallow])
    extreme = [p for p in benign if conflict_entry_bits(net, *p[:2]) > 900]
    tripping = with_x([p for p in pairs if 610 < min(p) * bits < 890])
    deep = with_x([p for p in pairs if 910 < min(p) * bits])
    assert extreme and len(extreme) < 32 and len(benign) >= 64 and len(tripping) >= 64 and deep
    benign = extreme + _spread([p for p in benign if p not in extreme], 64 - len(extreme))
    return SimpleNamespace(benign=benign, tripping=_spread(tripping, 64), deep=[deep[i % len(deep)] for i in range(64)])


def _spread(items, n):
    """n of the items, evenly spread, first and last included."""
    idx = sorted({round(i * (len(items) - 1) / (n - 1)) for i in range(n)})
    assert len(idx) == n
    return [items[i] for i in idx]


# ---------------------------------------------------------------------------------------------
# counts_net: ten variables, a tree of small cliques around one wide variable W = 5
#   0 (query) -> 1 -> 2 <- 0;  3 (one state) <- 2;  4 <- 3, 2;  W <- 4;  6 <- W;  7 <- W, 6;
#   8 <- 7;  9 <- 8, 7
# Parent lists [1, 0], [3, 2] and [8, 7] are given in descending order.
COUNTS_PARENTS = [[], [0], [1, 0], [2], [3, 2], [4], [5], [5, 6], [7], [8, 7]]
COUNTS_VARIANTS = {
    # all domains <= 4
    "small": [3, 2, 4, 1, 2, 4, 4, 2, 3, 2],
    # 32 states in the clique {5, 6, 7} of exactly 32 * 4 * 2 = 256 entries: the specialized
    # kernel's eligibility boundary in both limits
    "dom32": [2, 2, 4, 1, 2, 32, 4, 2, 2, 2],
    # 33 states: past the specialized kernel's evidence bit words
    "dom33": [2, 2, 4, 1, 2, 33, 4, 2, 2, 2],
    # 127 states: the most a network takes
    "dom127": [2, 2, 4, 1, 2, 127, 4, 2, 2, 2],
}
WIDE, ONE_STATE = 5, 3


def counts_net(seed, variant):
    """-> namespace(dims, parents, counts): counts[v] int64 [dims[v]][parent configurations] over
    the parents in ascending order, last fastest.  Counts are drawn from {0}, [1, 40] and, a few, from
    near 1e6 and 1e12; two parent configurations at least are unseen (all-zero: a uniform row)."""
    rng = np.random.Generator(np.random.PCG64([seed, sorted(COUNTS_VARIANTS).index(variant)]))
    dims = COUNTS_VARIANTS[variant]
    counts = []
    for v, ps in enumerate(COUNTS_PARENTS):
        npc = int(np.prod([dims[p] for p in ps])) if ps else 1
        c = rng.integers(1, 41, size=(dims[v], npc)).astype(np.int64)
        c[rng.random(c.shape) < 0.25] = 0
        big = rng.random(c.shape)
        c[big < 0.04] = 10 ** 6 + rng.integers(0, 1000)
        c[big < 0.02] = 10 ** 12 + rng.integers(0, 1000)
        counts.append(c)
    # unseen configurations: one of node 2 (two parents), one of node 7 (a child of the wide variable)
    counts[2][:, int(rng.integers(0, counts[2].shape[1]))] = 0
    counts[7][:, int(rng.integers(0, counts[7].shape[1]))] = 0
    counts[7][:, -1] = 0  # the last value of W with the last of 6
    return SimpleNamespace(dims=list(dims), parents=[list(p) for p in COUNTS_PARENTS], counts=counts, variant=variant)


COUNTS_SEED = 1  # (test_jt_counts_host.py: no query posterior of its cases ties within 1e-9)


def counts_gpu_cases(net):
    """The 70 cases (one full block and a ragged one) of the GPU tests: 0, 1, 2, 5 and 9 (all but
    the query) variables observed."""
    return np.concatenate([counts_cases(net, n, k, seed=7) for n, k in ((4, 0), (12, 1), (18, 2), (18, 5), (18, 9))])


def counts_cases(net, n, k, seed):
    """n evidence cases observing k variables other than the query, uniformly drawn values; every
    fourth case that observes the wide variable observes its last value, and the 1-state node is
    observed (at 0) whenever it is drawn."""
    rng = np.random.Generator(np.random.PCG64([seed, k]))
    V = len(net.dims)
    ev = np.full((n, V), -1, np.int8)
    for i in range(n):
        if k and i % 2 == 0:  # half of the cases observe the wide variable for sure
            obs = [WIDE] + rng.choice([v for v in range(1, V) if v != WIDE], size=k - 1, replace=False).tolist()
        else:
            obs = rng.choice(np.arange(1, V), size=k, replace=False).tolist()
        for v in obs:
            ev[i, v] = rng.integers(0, net.dims[v])
        if WIDE in obs and i % 4 == 0:
            ev[i, WIDE] = net.dims[WIDE] - 1
    return ev


class ExactJoint:
    """The joint distribution of a count-map network as exact integers: every CPT row
    (count + 1) / (total + states) is scaled by the least common multiple of its node's row
    denominators, so the weight of a joint state is a product of integers."""

    def __init__(self, dims, parents, counts):
        self.dims = [int(d) for d in dims]
        V = len(self.dims)
        joint = np.ones([1] * V, dtype=object)
        for v in range(V):
            asc = sorted(parents[v])
            c = np.asarray(counts[v], np.int64).reshape([self.dims[v]] + [self.dims[q] for q in asc])
            den = [int(t) + self.dims[v] for t in c.sum(axis=0).reshape(-1)]
            scale = math.lcm(*den)
            f = np.empty(c.size, dtype=object)
            flat = c.reshape(self.dims[v], -1)
            for q in range(self.dims[v]):
                for pc, d in enumerate(den):
                    f[q * len(den) + pc] = (int(flat[q, pc]) + 1) * (scale // d)
            shape = [1] * V
            axes = [v] + asc
            for a in axes:
                shape[a] = self.dims[a]
            # f is [v][asc...]: put its axes where the joint has them
            f = f.reshape([self.dims[a] for a in axes])
            order = np.argsort(axes)
            joint = joint * f.transpose(order).reshape(shape)
        self.joint = joint

    def marginals(self, ev):
        """(label, marginals [sum dims]) of one case as the junction tree reports them: exact sums,
        one rounding per value; zeros for observed variables; the label is the query's first largest
        value (strict '>' from 0), 0 if the query is observed.  Also .top2 = the relative gap of the
        query's two largest exact values."""
        V = len(self.dims)
        idx = tuple(slice(None) if ev[v] < 0 else slice(int(ev[v]), int(ev[v]) + 1) for v in range(V))
        sub = self.joint[idx]
        total = sub.sum()
        out, label = [], 0
        self.top2 = None
        for v in range(V):
            if ev[v] >= 0:
                out += [0.0] * self.dims[v]
                continue
            m = sub.sum(axis=tuple(a for a in range(V) if a != v)).tolist()
            out += [float(Fraction(int(x), int(total))) for x in m]
            if v == 0:
                best = 0
                for i, x in enumerate(m):
                    if x > best:
                        best, label = x, i
                s = sorted(m, reverse=True)
                self.top2 = float(Fraction(int(s[0] - s[1]), int(s[0]))) if len(s) > 1 else 1.0
        return label, np.array(out)


def exact_marginals(dims, parents, counts, ev):
    """(label, marginals) of one evidence case by enumeration of the joint in exact arithmetic."""
    return ExactJoint(dims, parents, counts).marginals(ev)
