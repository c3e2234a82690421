"""Loopy belief propagation's host twin (LoopyBeliefPropagation with device=-1: lbp_host.cpp).

Yardsticks: a pure-Python restatement of the algorithm (below: Python floats, explicit loops in the
stated order, no numpy reductions) for messages, marginals, labels and stats, bit for bit; the
reference's own marginals on the tie tree and brute-force enumeration of the joint on polytrees,
where the flooding schedule is exact, within the 1e-12 relative that test_gpu_jt_fast.py holds the
fast JT order to.  The restatement and the networks are shared with test_gpu_lbp.py."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
from conftest import ALARM, have_gpu

import fastbn_amd as F
from fastbn_amd import synth

ARG, LIMIT = -1, -6  # fbn_err_t (include/fastbn.h)
XML = os.path.join(ALARM, "alarm.xml")
TOL = 1e-12

# the 15-node shapes graph of test_gpu_sample.py / test_gpu_param.py: a 1-state node (12), 127 states
# (13), six parents (11), a descending parent order (3)
DIMS = np.array([5, 3, 7, 2, 4, 2, 2, 2, 2, 2, 2, 3, 1, 127, 6], np.int32)
GRAPH = [[], [0], [], [2, 0], [0, 1, 2], [], [], [], [], [], [], [5, 6, 7, 8, 9, 10], [], [12], [1]]


def net_tuple(dims, parents, counts):
    """synth's (names, dims, parents, cpts) of a Network.from_counts network: counts[v] is
    [value][configurations of the ASCENDING parents]; cpts[v] is [value, GIVEN parents...]."""
    dims = np.asarray(dims, np.int32)
    cpts = []
    for v, ps in enumerate(parents):
        asc = sorted(ps)
        a = np.asarray(counts[v], np.int64).reshape([dims[v]] + [dims[q] for q in asc])
        a = a.transpose([0] + [1 + asc.index(g) for g in ps])
        cpts.append((a + 1.0) / (a.sum(axis=0, keepdims=True) + 1.0 * dims[v]))
    return ["X%d" % v for v in range(len(dims))], dims, [list(p) for p in parents], cpts


class Graph:
    """The factor graph of a synth network tuple in plain Python lists."""

    def __init__(self, net):
        _, dims, parents, cpts = net
        self.dims = [int(d) for d in dims]
        self.V = len(self.dims)
        self.scope, self.table, self.stride, self.edges, self.eid = [], [], [], [], {}
        for f in range(self.V):
            sc = [f] + [int(g) for g in parents[f]]
            a = np.asarray(cpts[f], np.float64).reshape([self.dims[x] for x in sc])
            self.table.append(np.moveaxis(a, 0, -1).reshape(-1).tolist())  # cell = pc * d + q
            st, s = [1] * len(sc), self.dims[f]
            for j in range(len(sc) - 1, 0, -1):
                st[j] = s
                s *= self.dims[sc[j]]
            self.scope.append(sc)
            self.stride.append(st)
            for j in range(len(sc)):
                self.eid[(f, j)] = len(self.edges)
                self.edges.append((f, j))
        self.on = [[e for e, (f, j) in enumerate(self.edges) if self.scope[f][j] == x] for x in range(self.V)]
        self.moff, o = [], 0
        for f, j in self.edges:
            self.moff.append(o)
            o += self.dims[self.scope[f][j]]
        self.M = o


def _bad(z):
    return not (z > 0.0 and z < math.inf)


def restate(g, ev, iters, tol, damping):
    """One case.  -> dict(m, mu: flat lists of M floats; marg; lab; used; res)."""
    dims = g.dims
    var = [g.scope[f][j] for f, j in g.edges]
    m = [[1.0 / dims[x]] * dims[x] for x in var]
    mu = [[(1.0 if q == ev[x] else 0.0) if ev[x] >= 0 else 1.0 / dims[x] for q in range(dims[x])] for x in var]
    bad, used, res = False, 0, 0.0
    for it in range(1, iters + 1):
        res = 0.0
        for e, (f, s) in enumerate(g.edges):  # factor -> variable
            x = var[e]
            if ev[x] >= 0:
                continue
            sc, st = g.scope[f], g.stride[f]
            raw = [0.0] * dims[x]
            for c, p in enumerate(g.table[f]):
                for u in range(len(sc)):
                    if u != s:
                        p = p * mu[g.eid[(f, u)]][(c // st[u]) % dims[sc[u]]]
                q = (c // st[s]) % dims[x]
                raw[q] = raw[q] + p
            z = 0.0
            for q in range(dims[x]):
                z = z + raw[q]
            if _bad(z):
                bad = True
                continue
            for q in range(dims[x]):
                nw = raw[q] / z
                if damping != 0.0:
                    nw = (1.0 - damping) * nw + damping * m[e][q]
                res = max(res, abs(nw - m[e][q]))
                m[e][q] = nw
        new_mu = {}
        for e in range(len(g.edges)):  # variable -> factor
            x = var[e]
            if ev[x] >= 0:
                continue
            raw = []
            for q in range(dims[x]):
                p = 1.0
                for h in g.on[x]:
                    if h != e:
                        p = p * m[h][q]
                raw.append(p)
            z = 0.0
            for q in range(dims[x]):
                z = z + raw[q]
            if _bad(z):
                bad = True
                continue
            new_mu[e] = [raw[q] / z for q in range(dims[x])]
        for e, row in new_mu.items():
            for q, nw in enumerate(row):
                res = max(res, abs(nw - mu[e][q]))
            mu[e] = row
        used = it
        if bad or res <= tol:
            break
    marg = []
    for x in range(g.V):
        if ev[x] >= 0:
            marg += [0.0] * dims[x]
            continue
        raw = []
        for q in range(dims[x]):
            p = 1.0
            for h in g.on[x]:
                p = p * m[h][q]
            raw.append(p)
        z = 0.0
        for q in range(dims[x]):
            z = z + raw[q]
        if _bad(z):
            bad = True
            marg += [0.0] * dims[x]
        else:
            marg += [raw[q] / z for q in range(dims[x])]
    lab = -1
    if bad:
        marg = [0.0] * len(marg)
        res = math.inf
    else:
        lab, mp = 0, 0.0  # strict '>' from state 0, as fbn_jt_run
        for q in range(dims[0]):
            if marg[q] > mp:
                mp, lab = marg[q], q
    return dict(m=[v for row in m for v in row], mu=[v for row in mu for v in row], marg=marg, lab=lab, used=used,
                res=res)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_against_restatement(lbp, g, ev, iters, damping):
    """debug_messages, marginals, labels and stats of `lbp` (tol 0) = the restatement, bit for bit."""
    msgs = lbp.debug_messages(ev, iters)
    lab, marg = lbp.infer(ev)
    used, res = lbp.stats
    assert msgs.shape == (len(ev), 2, g.M) and lbp.info()["msg_doubles"] == g.M and lbp.info()["edges"] == len(g.edges)
    for c in range(len(ev)):
        fixed = restate(g, ev[c].tolist(), iters, -1.0, damping)  # exactly `iters` iterations
        np.testing.assert_array_equal(bits(msgs[c, 0]), bits(fixed["m"]))
        np.testing.assert_array_equal(bits(msgs[c, 1]), bits(fixed["mu"]))
        r = restate(g, ev[c].tolist(), iters, 0.0, damping)
        np.testing.assert_array_equal(bits(marg[c]), bits(r["marg"]))
        assert lab[c] == r["lab"] and used[c] == r["used"]
        np.testing.assert_array_equal(bits(res[c]), bits(r["res"]))


@functools.lru_cache(maxsize=None)
def alarm():
    return F.Network(XML), synth.read_xmlbif(XML)


@functools.lru_cache(maxsize=None)
def alarm_cases():
    ev, _ = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)
    ev.setflags(write=False)
    return ev


@functools.lru_cache(maxsize=None)
def shapes_network():
    rng = np.random.default_rng(15)
    counts = [rng.integers(0, 40, (int(DIMS[v]), int(np.prod(DIMS[ps], dtype=np.int64)))) for v, ps in enumerate(GRAPH)]
    return F.Network.from_counts(DIMS, GRAPH, counts), net_tuple(DIMS, GRAPH, counts)


@functools.lru_cache(maxsize=None)
def shapes_cases():
    ev = synth.evidence_cases(shapes_network()[1], 8, 3, seed=4)
    ev[1, 13] = 100  # a value past 64 of the 127-state node
    ev[2, 12] = 0    # the 1-state node observed
    ev[3, :] = -1
    ev.setflags(write=False)
    return ev


@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_restatement_alarm(damping):
    net, tup = alarm()
    lbp = F.LoopyBeliefPropagation(net, iterations=5, damping=damping, device=-1)
    check_against_restatement(lbp, Graph(tup), alarm_cases()[:4], 5, damping)


@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_restatement_shapes(damping):
    net, tup = shapes_network()
    lbp = F.LoopyBeliefPropagation(net, iterations=5, damping=damping, device=-1)
    check_against_restatement(lbp, Graph(tup), shapes_cases()[:4], 5, damping)


def check_tie_tree(synth_nets, device):
    t = synth_nets["tie"]
    assert len(t["ev"]) == 64
    lbp = F.LoopyBeliefPropagation(F.Network(t["xml"]), iterations=64, tol=0.0, device=device)
    _, marg = lbp.infer(t["ev"])
    np.testing.assert_allclose(marg, t["marg"], rtol=TOL, atol=1e-300)
    used, res = lbp.stats
    assert (res == 0.0).all() and (used < 64).all()
    return lbp


def test_exact_on_the_tie_tree(synth_nets):
    check_tie_tree(synth_nets, -1)


def brute_force(tup, ev):
    """Posterior marginals [sum_dom] of one case by enumerating the joint (numpy), zeros for observed."""
    _, dims, parents, cpts = tup
    V = len(dims)
    joint = np.ones([int(d) for d in dims])
    for v in range(V):
        sc = [v] + list(parents[v])
        a = np.asarray(cpts[v], np.float64).reshape([dims[x] for x in sc])
        order = np.argsort(sc)
        shape = [1] * V
        for x in sc:
            shape[x] = int(dims[x])
        joint = joint * a.transpose(order).reshape(shape)
    for v in range(V):
        if ev[v] >= 0:
            keep = np.zeros(int(dims[v]), bool)
            keep[ev[v]] = True
            shape = [1] * V
            shape[v] = int(dims[v])
            joint = joint * keep.reshape(shape)
    joint = joint / joint.sum()
    out = []
    for v in range(V):
        mv = joint.sum(axis=tuple(x for x in range(V) if x != v))
        out += [0.0] * int(dims[v]) if ev[v] >= 0 else mv.tolist()
    return np.array(out)


def random_polytree(n, seed, max_parents=3):
    """A seeded polytree: node i takes up to max_parents parents among the earlier nodes, each from a
    different connected component, so the undirected graph stays a forest; state counts 1 to 3."""
    rng = np.random.default_rng(seed)
    dims = rng.integers(1, 4, n).astype(np.int32)
    comp = list(range(n))
    parents = []
    for i in range(n):
        ps = []
        for p in rng.permutation(i)[:int(rng.integers(0, max_parents + 1))]:
            if comp[p] != comp[i]:
                old = comp[p]
                comp = [comp[i] if c == old else c for c in comp]
                ps.append(int(p))
        parents.append(ps)
    counts = [rng.integers(0, 40, (int(dims[v]), int(np.prod(dims[ps], dtype=np.int64)))) for v, ps in enumerate(parents)]
    return dims, parents, counts


def polytree_cases(dims, ncases, seed):
    """Case c observes c % 5 variables (never the query)."""
    rng = np.random.default_rng(seed)
    ev = np.full((ncases, len(dims)), -1, np.int8)
    for c in range(ncases):
        for v in rng.choice(np.arange(1, len(dims)), c % 5, replace=False):
            ev[c, v] = rng.integers(0, dims[v])
    return ev


POLYTREE_SEED = 7  # brute force alone: the top two of variable 0 are further than 1e-9 apart in >= 14 of 16 cases


def check_exact(lbp, tup, ev, max_left_out):
    lab, marg = lbp.infer(ev)
    exact = np.stack([brute_force(tup, e) for e in ev])
    np.testing.assert_allclose(marg, exact, rtol=TOL, atol=1e-300)
    d0 = int(tup[1][0])
    top = np.sort(exact[:, :d0], axis=1)
    clear = (top[:, -1] - top[:, -2] > 1e-9) if d0 > 1 else np.ones(len(ev), bool)
    assert (~clear).sum() <= max_left_out
    np.testing.assert_array_equal(lab[clear], np.argmax(exact[:, :d0], axis=1)[clear])
    return marg


def test_exact_on_a_polytree_with_multi_parent_nodes():
    dims, parents, counts = random_polytree(12, POLYTREE_SEED)
    assert dims[0] >= 2 and max(len(p) for p in parents) >= 2 and dims.min() == 1
    net = F.Network.from_counts(dims, parents, counts)
    tup = net_tuple(dims, parents, counts)
    ev = polytree_cases(dims, 16, 1)
    assert sorted(set((ev >= 0).sum(1))) == [0, 1, 2, 3, 4]
    lbp = F.LoopyBeliefPropagation(net, iterations=32, tol=0.0, device=-1)
    check_exact(lbp, tup, ev, 2)
    assert (lbp.stats[1] == 0.0).all() and (lbp.stats[0] < 32).all()


def disconnected_network():
    """Two polytrees (nodes 0-4 and 5-9) and the isolated node 10."""
    dims = np.array([2, 3, 2, 3, 2, 3, 2, 2, 3, 2, 3], np.int32)
    parents = [[], [], [1, 0], [2], [2], [], [5], [], [7, 6], [8], []]
    rng = np.random.default_rng(21)
    counts = [rng.integers(0, 40, (int(dims[v]), int(np.prod(dims[ps], dtype=np.int64)))) for v, ps in enumerate(parents)]
    return dims, parents, counts


def test_disconnected_network():
    """LBP runs where the junction tree refuses the network, and is exact on every component."""
    dims, parents, counts = disconnected_network()
    net = F.Network.from_counts(dims, parents, counts)
    with pytest.raises(F.FastBNError):
        F.JunctionTree(net, device=-1)
    tup = net_tuple(dims, parents, counts)
    ev = polytree_cases(dims, 10, 2)
    marg = check_exact(F.LoopyBeliefPropagation(net, iterations=16, device=-1), tup, ev, 0)
    cnt = np.asarray(counts[10])[:, 0]
    np.testing.assert_allclose(marg[ev[:, 10] < 0][:, -3:], np.tile((cnt + 1.0) / (cnt.sum() + 3), (int((ev[:, 10] < 0).sum()), 1)),
                               rtol=TOL)
    if not have_gpu():
        return
    # with a device: the network PC-stable learns from ALARM-5000, its isolated node 12 included
    ds = F.Dataset(os.path.join(ALARM, "alarm_s5000.txt"))
    pc = F.PCStable(0.05, 1000).StructLearnCompData(ds)
    dag = F.pdag_to_dag(ds.num_vars, pc.oriented)
    assert dag[12] == [] and not any(12 in ps for ps in dag)
    learned = F.ParameterLearning(pc.ci).LearnParamsKnowStructCompData(dag, names=ds.names)
    with pytest.raises(F.FastBNError):
        F.JunctionTree(learned, device=0)
    ev = np.full((4, 37), -1, np.int8)
    ev[1:, 3] = 0
    lab, marg = F.LoopyBeliefPropagation(learned, iterations=40, device=-1).infer(ev)
    dlab, dmarg = F.LoopyBeliefPropagation(learned, iterations=40, device=0).infer(ev)
    np.testing.assert_array_equal(lab, dlab)
    np.testing.assert_array_equal(bits(marg), bits(dmarg))
    _, cnt = learned.node_counts(12)
    off = int(np.sum(ds.dims[:12]))
    np.testing.assert_allclose(marg[:, off:off + len(cnt)], np.tile((cnt[:, 0] + 1.0) / (cnt.sum() + len(cnt)), (4, 1)), rtol=TOL)
    assert np.allclose(marg.reshape(4, -1).sum(1), [37, 36, 36, 36])


def check_early_stop(device):
    net, _ = alarm()
    ev = alarm_cases()[:8]
    lbp = F.LoopyBeliefPropagation(net, iterations=200, tol=1e-9, device=device)
    lab, marg = lbp.infer(ev)
    used, res = lbp.stats
    print("iterations used", used.tolist(), "residuals", res.tolist())
    assert len(set(used.tolist())) > 1
    assert ((res <= 1e-9) | (used == 200)).all() and (used >= 1).all()
    lab2, marg2 = lbp.infer(ev)
    np.testing.assert_array_equal(lab, lab2)
    np.testing.assert_array_equal(bits(marg), bits(marg2))
    np.testing.assert_array_equal(bits(res), bits(lbp.stats[1]))
    lab3, marg3 = lbp.infer(ev[2:7])
    np.testing.assert_array_equal(lab3, lab[2:7])
    np.testing.assert_array_equal(bits(marg3), bits(marg[2:7]))
    np.testing.assert_array_equal(lbp.stats[0], used[2:7])
    return lab, marg, used, res


def test_early_stop():
    check_early_stop(-1)


def test_arguments(tmp_path):
    net, _ = alarm()
    ev = alarm_cases()[:4].copy()
    ref = F.LoopyBeliefPropagation(net, device=-1).infer(ev)
    for kw in (dict(iterations=0), dict(tol=-1e-3), dict(tol=math.nan), dict(damping=1.0), dict(damping=-0.1),
               dict(damping=math.nan)):
        with pytest.raises(F.FastBNError) as e:
            F.LoopyBeliefPropagation(net, device=-1, **kw).infer(ev)
        assert e.value.code == ARG, kw
    lbp = F.LoopyBeliefPropagation(net, device=-1)
    bad = ev.copy()
    bad[2, 5] = net.dims[5]  # one past the last state
    with pytest.raises(F.FastBNError, match="case 2.*node 5") as e:
        lbp.infer(bad)
    assert e.value.code == ARG
    bad[2, 5] = -2
    with pytest.raises(F.FastBNError) as e:
        lbp.debug_messages(bad, 2)
    assert e.value.code == ARG
    np.testing.assert_array_equal(bits(lbp.infer(ev)[1]), bits(ref[1]))  # the handle stays usable
    # fbn_network_create refuses a cycle itself; the XMLBIF loader does not
    var = "<VARIABLE><NAME>%s</NAME><TYPE>discrete</TYPE><VALUE>0</VALUE><VALUE>1</VALUE></VARIABLE>\n"
    prob = "<PROBABILITY><FOR>%s</FOR><GIVEN>%s</GIVEN><TABLE>0.5 0.5 0.5 0.5 </TABLE></PROBABILITY>\n"
    xml = tmp_path / "cyclic.xml"
    xml.write_text('<?xml version="1.0"?>\n<BIF><NETWORK><NAME>c</NAME>\n' + var % "A" + var % "B" + prob % ("A", "B")
                   + prob % ("B", "A") + "</NETWORK></BIF>\n")
    with pytest.raises(F.FastBNError, match="cycle") as e:
        F.LoopyBeliefPropagation(F.Network(str(xml)), device=-1)
    assert e.value.code == ARG
    # 25 binary roots and one binary child of all of them: 2^26 cells, the cap, plus the roots' 50.
    # The count array is never written (zero pages), only read by fbn_network_create.
    V = 26
    dims = np.full(V, 2, np.int32)
    off = np.zeros(V + 1, np.int32)
    off[V] = 25
    par = np.arange(25, dtype=np.int32)
    cnt = np.zeros(50 + (1 << 26), np.int64)
    h = C.c_void_p()
    F.lib.fbn_network_create(V, dims.ctypes.data, off.ctypes.data, par.ctypes.data, cnt.ctypes.data, None, C.byref(h))
    big = F.Network(_handle=h)
    del cnt
    with pytest.raises(F.FastBNError) as e:
        F.LoopyBeliefPropagation(big, device=-1)
    assert e.value.code == LIMIT
    big.close()
