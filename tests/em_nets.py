"""Helpers shared by test_em_host.py, test_gpu_em.py and test_gpu_em_cli.py: yardsticks for the E-step of
ExpectationMaximization (fbn_em) that know nothing of a junction tree, the networks, and the bounds.

Bounds.  u = 2^-53, E = info()["entries"], V the nodes, B = 4 * (E + 3 V) * u.  Every number the E-step
reports is a ratio of two sums of products of positive CPT entries; in non-negative arithmetic a rounding
costs at most a factor (1 +- u); no numerator or denominator passes through more than E additions and 3 V
multiplications or divisions (V CPT divisions, fewer than V potential-build multiplies, fewer than V
message multiplies on any path); the ratio doubles the count and the remaining factor 2 is margin.
Per-case posteriors and P(e) are held to exact rationals within relative B, to an fp64 numpy yardstick
within 2 B (it rounds as well), and counts summed over n cases within B + n u per cell.  A cell the
evidence rules out is exactly 0.0.

Yardsticks: brute-force enumeration of the joint per graph component in numpy (family marginals and the
component's evidence probability; mpe_nets.brute_force's construction), the same enumeration in
fractions.Fraction on a 5-node network of 72 joint states, and a numpy sum-product variable elimination
for P(e) (linear domain, greedy min-degree order)."""
import functools
import itertools
import os
from fractions import Fraction

import numpy as np
from conftest import ALARM
from mpe_nets import (ExactNet, alarm_cases, alarm_net, chain_cases, chain_net, disconnected_net, mixed_cases,  # noqa: F401
                      shapes_net, value_fraction)

import fastbn_amd as F

U = 2.0 ** -53
ARG, NODEV, LIMIT = -1, -5, -6


def bound(em):
    i = em.info()
    return 4 * (i["entries"] + 3 * em.num_nodes) * U


class Tables:
    """A network's CPTs as the fp64 arrays the library reads (Network.node_probs: either kind of network):
    tab[v] has shape [dims[v]] + [dims of the ascending parents]; off[v] is the family's first cell."""

    def __init__(self, net):
        self.V = net.num_nodes
        self.dims = [int(d) for d in net.dims]
        self.parents, self.tab, self.off = [], [], [0]
        for v in range(self.V):
            par, pr = net.node_probs(v)
            self.parents.append([int(p) for p in par])
            self.tab.append(pr.reshape([self.dims[v]] + [self.dims[q] for q in par]))
            self.off.append(self.off[-1] + pr.size)
        self.cells = self.off[-1]

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


def brute_posteriors(tb, ev):
    """-> (family posteriors fp64 [cells] in fbn_param_counts' layout, P(e)) by enumerating the joint of
    every component."""
    post = np.zeros(tb.cells)
    p_e = 1.0
    for comp in tb.components():
        pos = {v: i for i, v in enumerate(comp)}
        joint = np.ones([tb.dims[v] for v in comp])
        for v in comp:
            sc = [v] + tb.parents[v]
            shape = [1] * len(comp)
            for x in sc:
                shape[pos[x]] = tb.dims[x]
            joint = joint * tb.tab[v].transpose(np.argsort(sc)).reshape(shape)
        for v in comp:
            if ev[v] >= 0:
                keep = np.zeros(tb.dims[v])
                keep[ev[v]] = 1.0
                shape = [1] * len(comp)
                shape[pos[v]] = tb.dims[v]
                joint = joint * keep.reshape(shape)
        z = joint.sum()
        p_e *= z
        for v in comp:
            sc = [v] + tb.parents[v]
            other = tuple(i for i, x in enumerate(comp) if x not in sc)
            m = joint.sum(axis=other) if other else joint
            left = sorted(sc)  # the axes that remain, in component order
            m = m.transpose([left.index(x) for x in sc])
            post[tb.off[v]:tb.off[v + 1]] = (m / z).reshape(-1)
    return post, p_e


def exact_posteriors(en, tb, ev):
    """The same in Fractions from the network's counts (ExactNet): -> (list of Fraction [cells], P(e))."""
    post = [Fraction(0)] * tb.cells
    z = Fraction(0)
    ranges = [[int(ev[v])] if ev[v] >= 0 else range(en.dims[v]) for v in range(en.V)]
    for x in itertools.product(*ranges):
        p = en.prob(x)
        z += p
        for v in range(en.V):
            pc = 0
            for q in en.parents[v]:
                pc = pc * en.dims[q] + x[q]
            npc = (tb.off[v + 1] - tb.off[v]) // en.dims[v]
            post[tb.off[v] + x[v] * npc + pc] += p
    return [p / z for p in post], z


def sum_product_ve(tb, ev):
    """P(e) by variable elimination in numpy: factors (variables, array with one axis per variable),
    evidence sliced away, greedy min-degree order.  No cliques, no separators, no plan."""
    factors = []
    const = 1.0
    for v in range(tb.V):
        sc = [v] + tb.parents[v]
        a = tb.tab[v]
        keep = []
        for ax, x in reversed(list(enumerate(sc))):
            if ev[x] >= 0:
                a = np.take(a, int(ev[x]), axis=ax)
            else:
                keep.append(x)
        keep = tuple(reversed(keep))
        if keep:
            order = np.argsort(keep)
            factors.append((tuple(sorted(keep)), a.transpose(order)))
        else:
            const *= float(a)
    while factors:
        nbr = {}
        for sc, _ in factors:
            for x in sc:
                nbr.setdefault(x, set()).update(sc)
        v = min(nbr, key=lambda x: (len(nbr[x]), x))
        mine = [f for f in factors if v in f[0]]
        factors = [f for f in factors if v not in f[0]]
        scope = sorted(nbr[v])
        pos = {x: k for k, x in enumerate(scope)}
        acc = 1.0
        for sc, a in mine:
            shape = [1] * len(scope)
            for x in sc:
                shape[pos[x]] = tb.dims[x]
            acc = acc * a.reshape(shape)
        out = acc.sum(axis=pos[v])
        rest = tuple(x for x in scope if x != v)
        if rest:
            factors.append((rest, out))
        else:
            const *= float(out)
    return const


# ---- networks (each built once)
@functools.lru_cache(maxsize=None)
def tiny_net():
    """5 nodes, 72 joint states, a v-structure and a two-parent family: the Fractions yardstick's network."""
    dims = np.array([2, 3, 2, 2, 3], np.int32)
    parents = [[], [0], [0, 1], [2], [1, 3]]
    rng = np.random.default_rng(5)
    counts = [rng.integers(0, 50, (int(dims[v]), int(np.prod(dims[ps], dtype=np.int64)))) for v, ps in enumerate(parents)]
    net = F.Network.from_counts(dims, parents, counts)
    return net, ExactNet(net)


@functools.lru_cache(maxsize=None)
def nine_net():
    """One node with 8 binary parents: a 9-variable clique (a second digit word) and a family of 512 cells."""
    dims = np.full(9, 2, np.int32)
    parents = [[] for _ in range(8)] + [list(range(8))]
    rng = np.random.default_rng(9)
    counts = [rng.integers(0, 30, (2, 1 if v < 8 else 256)) for v in range(9)]
    return F.Network.from_counts(dims, parents, counts)


@functools.lru_cache(maxsize=None)
def star_net():
    """A centre family {0, 1, 2} -> 3 and one child of each of its four variables: the cliques {0, 4}, {1, 5},
    {2, 6}, {3, 7} share a variable with the centre clique alone, so wherever the root is, the centre clique
    has at least 3 children, and the downward message to one excludes it among several."""
    dims = np.array([2, 3, 2, 3, 2, 4, 3, 2], np.int32)
    parents = [[], [], [], [0, 1, 2], [0], [1], [2], [3]]
    rng = np.random.default_rng(8)
    counts = [rng.integers(0, 40, (int(dims[v]), int(np.prod(dims[ps], dtype=np.int64)))) for v, ps in enumerate(parents)]
    return F.Network.from_counts(dims, parents, counts)


SMALL_NETS = {"shapes": (lambda: shapes_net()[0], 11), "disconnected": (lambda: disconnected_net()[0], 31),
              "nine": (nine_net, 51), "star": (star_net, 61)}


def small_net(key):
    make, seed = SMALL_NETS[key]
    net = make()
    return net, mixed_cases(net, seed)


def check_against_brute_force(net, ev, post, value, b):
    """Posteriors and P(e) of every case within 2 b (relative) of the numpy enumeration; cells the evidence
    rules out exactly 0; every family's cells sum to 1."""
    tb = Tables(net)
    for c in range(len(ev)):
        want, p_e = brute_posteriors(tb, ev[c])
        got = post[c]
        assert ((want == 0) == (got == 0)).all(), c
        assert (np.abs(got - want) <= 2 * b * want).all(), (c, float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
        p = float(value_fraction(value[c]))
        assert abs(p - p_e) <= 2 * b * p_e, (c, p, p_e)
        for v in range(tb.V):
            assert abs(got[tb.off[v]:tb.off[v + 1]].sum() - 1.0) <= 2 * b + 4 * U


def check_against_fractions(net, en, ev, post, value, b):
    """Within b (relative) of the exact rationals."""
    tb = Tables(net)
    bf = Fraction(b)
    for c in range(len(ev)):
        want, z = exact_posteriors(en, tb, ev[c])
        for i in range(tb.cells):
            got = Fraction(float(post[c, i]))
            assert abs(got - want[i]) <= bf * want[i], (c, i, float(got), float(want[i]))
        assert abs(value_fraction(value[c]) - z) <= bf * z, c


def split_cells(tb, flat):
    return [flat[tb.off[v]:tb.off[v + 1]].reshape(tb.dims[v], -1) for v in range(tb.V)]


def mstep(counts, alpha, dims):
    """The stated M-step in numpy on a list of [dims[v], parent configs] arrays: T in ascending q from 0.0."""
    out = []
    for v, n in enumerate(counts):
        tot = np.zeros(n.shape[1])
        for q in range(n.shape[0]):
            tot = tot + n[q]
        out.append((n + alpha) / (tot + alpha * float(dims[v])))
    return out


def manual_chain(em, data, parents, iters, alpha):
    """estep, the numpy M-step, set_parameters -- iters times.  -> the last parameters (list of arrays)."""
    theta = None
    for _ in range(iters):
        counts, _ = em.estep(data)
        theta = mstep(counts, alpha, em.dims)
        em.set_parameters(F.Network.from_cpts(em.dims, parents, theta))
    return theta


def bits(arrays):
    return b"".join(np.ascontiguousarray(a, np.float64).tobytes() for a in arrays)


def network_bits(net):
    return bits([net.node_probs(v)[1] for v in range(net.num_nodes)])


# ---- ALARM data
@functools.lru_cache(maxsize=None)
def alarm_parents():
    net, _ = alarm_net()
    return [[int(q) for q in net.node_counts(v)[0]] for v in range(net.num_nodes)]


@functools.lru_cache(maxsize=None)
def alarm_complete():
    """alarm_s5000.txt as int8 rows (first-appearance codes) and the data's own state counts."""
    ds = F.Dataset(os.path.join(ALARM, "alarm_s5000.txt"))
    rows = np.ascontiguousarray(ds.columns.T.astype(np.int8))
    rows.setflags(write=False)
    return rows, ds.dims.copy()


def uniform_start(dims, parents):
    """All-zero counts: uniform CPTs."""
    zeros = [np.zeros((int(dims[v]), int(np.prod(np.asarray(dims)[ps], dtype=np.int64))), np.int64)
             for v, ps in enumerate(parents)]
    return F.Network.from_counts(dims, parents, zeros)


def family_counts(rows, dims, parents):
    """Complete-data family counts in numpy: int64 [dims[v]][parent configs] per node."""
    out = []
    for v, ps in enumerate(parents):
        pc = np.zeros(len(rows), np.int64)
        for q in sorted(ps):
            pc = pc * int(dims[q]) + rows[:, q]
        npc = int(np.prod(np.asarray(dims)[ps], dtype=np.int64))
        out.append(np.bincount(rows[:, v].astype(np.int64) * npc + pc, minlength=int(dims[v]) * npc).reshape(int(dims[v]), npc))
    return out


@functools.lru_cache(maxsize=None)
def alarm_incomplete(n=2000):
    """n forward-sampled ALARM rows with 30 % of the cells missing (seeded)."""
    net, _ = alarm_net()
    rows = net.forward_sample(n, 17).T.astype(np.int8)
    rows[np.random.default_rng(18).random(rows.shape) < 0.3] = -1
    rows.setflags(write=False)
    return rows


def assert_monotone(em, obj, ncases):
    """Q never falls by more than its own rounding: with n = ncases + cells terms, each log term errs by at
    most B + 4u absolutely and the summation adds at most n u |Q|."""
    b = bound(em)
    n = ncases + em.info()["cells"]
    assert np.isfinite(obj).all()
    for t in range(1, len(obj)):
        assert obj[t, 1] >= obj[t - 1, 1] - (n * (b + 4 * U) + n * U * abs(obj[t, 1])), (t, obj[t - 1, 1], obj[t, 1])
    assert obj[-1, 1] > obj[0, 1]  # and it did climb


def check_chain(em, n):
    """The n-node binary chain of mpe_nets (none observed, every 10th node observed, all observed).  Where MPE
    reports max_x P(x, e), the E-step reports P(e) = the sum over x: 1 with nothing observed and about
    2^-(n / 10) with every 10th node observed -- inside fp64's range however long the chain -- so only the
    fully observed case lies below 2^-1074, and there the two are the same number.  The exponent is held
    below -1074 where the exact P(e) is; the case that observes nothing is held to P(e) = 1 within B after
    n - 1 rescaled messages; the posteriors are finite and every family's cells sum to 1 within B."""
    net, en = chain_net(n)
    ev = chain_cases(n)
    b = bound(em)
    _, value = em.estep(ev)
    assert (value[:, 0] >= 0.5).all() and (value[:, 0] < 1).all()
    assert abs(value_fraction(value[0]) - 1) <= Fraction(b)
    exact = en.prob(ev[2])
    assert (exact < Fraction(1, 2 ** 1074)) == (n >= 2000) == bool(value[2, 1] < -1074)
    assert abs(value_fraction(value[2]) - exact) <= Fraction(b) * exact
    assert value[1, 1] < -n // 20 and np.isfinite(em.log_likelihood(ev)).all()
    post = em.debug_posteriors(ev)
    assert np.isfinite(post).all() and (post >= 0).all()
    tb = Tables(net)
    for c in range(len(ev)):
        sums = np.array([f.sum() for f in split_cells(tb, post[c])])
        assert (np.abs(sums - 1.0) <= b).all(), (c, float(np.abs(sums - 1.0).max()), b)
    # the fully observed case puts exactly 1.0 on one cell per family
    assert sorted(set(post[2])) == [0.0, 1.0] and post[2].sum() == n
    return value, post
