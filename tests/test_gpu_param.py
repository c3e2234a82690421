"""Parameter learning on the device (param_counts.hip behind fbn_param_counts / fbn_param_learn).

The yardstick is a numpy restatement of DiscreteNode::AddCount (src/DiscreteNode.cpp:132-145):
np.add.at on the key q * npc + sum(stride * code), parents ascending, last fastest.  Counts are
integers: every comparison is exact equality."""
import functools
import os

import numpy as np
import pytest
from conftest import ALARM

import fastbn_amd as F

pytestmark = pytest.mark.gpu

ARG, LIMIT = -1, -6  # fbn_err_t (include/fastbn.h)

# One graph with every family shape the kernel distinguishes (15 nodes):
#   0, 2, 5..10, 12: no parents (12 has ONE state)        1: one parent
#   3: parents listed in DESCENDING order                   4: three parents of 5, 3, 7 states (420 cells)
#   11: six binary parents (192 cells)                      13: 127 states (code 126 occurs), a 1-state parent
#   14: 6 states of which value 4 never occurs (zero cells must stay zero)
DIMS = np.array([5, 3, 7, 2, 4, 2, 2, 2, 2, 2, 2, 3, 1, 127, 6], np.int32)
GRAPH = [[], [0], [], [2, 0], [0, 1, 2], [], [], [], [], [], [], [5, 6, 7, 8, 9, 10], [], [12], [1]]
# a second graph on the same variables: other parents, other table sizes and offsets
GRAPH2 = [[1], [], [0, 1], [], [3], [4, 3], [], [6], [], [], [9, 8, 7], [], [], [], [13, 12]]
NS = [1, 3, 255, 257, 1021, 70001]


@functools.lru_cache(maxsize=None)
def columns(N):
    rng = np.random.default_rng(1000 + N)
    cols = np.stack([rng.integers(0, d, N) for d in DIMS]).astype(np.uint8)
    cols[13, 0] = 126  # the last code of the 127-state node occurs
    cols[14] = np.array([0, 1, 2, 3, 5], np.uint8)[rng.integers(0, 5, N)]  # value 4 never does
    # mildly dependent columns, so the tables are far from uniform
    cols[1] = np.where(rng.random(N) < 0.5, cols[0] % 3, cols[1])
    cols[11] = np.where(rng.random(N) < 0.5, (cols[5] + cols[6] + cols[7]) % 3, cols[11])
    cols.setflags(write=False)
    return cols


def np_counts(cols, dims, parents):
    out = []
    for v, ps in enumerate(parents):
        ps = sorted(ps)
        npc = int(np.prod(dims[ps], dtype=np.int64))
        key = cols[v].astype(np.int64) * npc
        stride = 1
        for q in reversed(ps):
            key += stride * cols[q].astype(np.int64)
            stride *= int(dims[q])
        c = np.zeros(int(dims[v]) * npc, np.int64)
        np.add.at(c, key, 1)
        out.append(c.reshape(int(dims[v]), npc))
    return out


@functools.lru_cache(maxsize=None)
def reference(N, which=0):
    return np_counts(columns(N), DIMS, GRAPH2 if which else GRAPH)


def assert_counts_equal(got, ref):
    assert len(got) == len(ref)
    for v, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == np.int64 and g.shape == r.shape, v
        np.testing.assert_array_equal(g, r, err_msg=f"family {v}")


def learner(N):
    return F.ParameterLearning(F.Dataset(columns=columns(N), dims=DIMS))


@pytest.mark.parametrize("N", NS)
def test_counts_equal_numpy(N):
    """N = 1, 3: a tail shorter than one load; 255, 257, 1021: columns that start off a dword
    (N % 4 != 0) and fewer samples than one workgroup takes per step; 70001: many slices."""
    pl = learner(N)
    got = pl.counts(GRAPH)
    assert_counts_equal(got, reference(N))
    assert all(int(g.sum()) == N for g in got)
    assert got[14][4].sum() == 0 and got[13][126].sum() >= 1
    assert pl.last_kernel_ms() > 0.0


def test_both_paths_and_slices_at_small_n():
    N = 1021
    pl = learner(N)
    pl.set_tuning(samples_per_slice=300, lds_cells_max=0)  # four slices, the last one ragged (121)
    assert_counts_equal(pl.counts(GRAPH), reference(N))
    pl.set_tuning(samples_per_slice=300, lds_cells_max=16)  # families above 16 cells: global path
    assert sum(int(DIMS[v]) * int(np.prod(DIMS[ps])) > 16 for v, ps in enumerate(GRAPH)) >= 4
    assert_counts_equal(pl.counts(GRAPH), reference(N))
    pl.set_tuning(samples_per_slice=0, lds_cells_max=-1)  # every family on the global path, one slice
    assert_counts_equal(pl.counts(GRAPH), reference(N))
    pl.set_tuning()  # defaults
    assert_counts_equal(pl.counts(GRAPH), reference(N))


def test_second_call_sees_no_stale_counts():
    N = 257
    pl = learner(N)
    assert_counts_equal(pl.counts(GRAPH), reference(N))
    assert_counts_equal(pl.counts(GRAPH2), reference(N, 1))
    assert_counts_equal(pl.counts(GRAPH), reference(N))


def test_default_global_path_large_family():
    """Eight parents of 4 states: 4^9 = 2^18 cells, above the default LDS threshold (8192)."""
    N = 4096
    rng = np.random.default_rng(7)
    dims = np.full(9, 4, np.int32)
    cols = rng.integers(0, 4, (9, N)).astype(np.uint8)
    cols[8] = np.where(rng.random(N) < 0.6, (cols[0] + cols[3]) % 4, cols[8])
    parents = [[] for _ in range(8)] + [[7, 6, 5, 4, 3, 2, 1, 0]]
    got = F.ParameterLearning(F.Dataset(columns=cols, dims=dims)).counts(parents)
    assert got[8].shape == (4, 4 ** 8)
    assert_counts_equal(got, np_counts(cols, dims, parents))


def test_shared_context_with_ci_tests():
    N = 1021
    ds = F.Dataset(columns=columns(N), dims=DIMS)
    ci = F.IndependenceTest(ds)
    items0 = np.array([[0, 1], [5, 11], [13, 14]], np.int32)
    items1 = np.array([[0, 1, 2], [5, 11, 6], [3, 4, 0]], np.int32)
    before = ci.run(items0, 0), ci.run(items1, 1)
    pl = F.ParameterLearning(ci)
    assert pl.ci is ci
    got = pl.counts(GRAPH)
    assert_counts_equal(got, reference(N))
    assert_counts_equal(got, learner(N).counts(GRAPH))  # a fresh upload
    after = ci.run(items0, 0), ci.run(items1, 1)
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            np.testing.assert_array_equal(x, y)


def test_errors_are_refused_on_the_host_and_leave_the_context_usable():
    N = 64
    rng = np.random.default_rng(3)
    V = 28
    dims = np.full(V, 2, np.int32)
    cols = rng.integers(0, 2, (V, N)).astype(np.uint8)
    pl = F.ParameterLearning(F.Dataset(columns=cols, dims=dims))
    good = [[] for _ in range(V - 1)] + [[0, 1, 2]]
    ref = np_counts(cols, dims, good)
    bad = [list(ps) for ps in good]
    bad[3] = [V]  # a parent index >= nvars
    with pytest.raises(F.FastBNError) as e:
        pl.counts(bad)
    assert e.value.code == ARG
    assert_counts_equal(pl.counts(good), ref)
    big = [[] for _ in range(V - 1)] + [list(range(V - 1))]  # 2^28 cells: over the cap of 2^26
    with pytest.raises(F.FastBNError) as e:
        pl.counts(big)
    assert e.value.code == LIMIT
    with pytest.raises(F.FastBNError) as e:
        pl.LearnParamsKnowStructCompData(big)
    assert e.value.code == LIMIT
    assert_counts_equal(pl.counts(good), ref)


def test_end_to_end_csv_to_junction_tree():
    """CSV -> PCStable -> pdag_to_dag -> LearnParamsKnowStructCompData -> JunctionTree, one upload."""
    ds = F.Dataset(os.path.join(ALARM, "alarm_s5000.txt"))
    pc = F.PCStable(0.05, 1000).StructLearnCompData(ds)
    dag = F.pdag_to_dag(ds.num_vars, pc.oriented)
    assert sum(len(ps) for ps in dag) == len(pc.oriented) == 44
    pl = F.ParameterLearning(pc.ci)  # the context PC-stable ran on
    net = pl.LearnParamsKnowStructCompData(dag, names=ds.names)
    ref = np_counts(ds.columns, ds.dims, dag)
    assert net.num_nodes == 37 and net.name(5) == ds.names[5]
    for v in range(37):
        par, cnt = net.node_counts(v)
        assert par.tolist() == dag[v]
        np.testing.assert_array_equal(cnt, ref[v], err_msg=f"node {v}")
    # Inference on what was learned.  fbn_jt_plan_create builds a junction TREE and refuses a graph
    # whose moral graph is disconnected ("junction forest unsupported", jt_plan.cpp); the graph PC
    # learns from 5,000 ALARM samples leaves node 12 without any edge.  So inference runs on every
    # connected component of the moral graph that has an edge, the component's network taken from
    # the LEARNED network's count maps, against the same component built from the numpy counts.
    comps = _moral_components(dag)
    assert sorted(v for c in comps for v in c) == list(range(37))
    assert sum(len(c) for c in comps if len(c) > 1) >= 36
    for comp in (c for c in comps if len(c) > 1):
        new = {v: i for i, v in enumerate(comp)}
        sub_par = [[new[q] for q in dag[v]] for v in comp]
        learned = F.Network.from_counts(ds.dims[comp], sub_par, [net.node_counts(v)[1] for v in comp])
        expect = F.Network.from_counts(ds.dims[comp], sub_par, [ref[v] for v in comp])
        ev = learned.evidence_cases(256, 7, seed=1)
        out = []
        for n in (learned, expect):
            jt = F.JunctionTree(n, device=0)
            jt.set_variant(0)  # the interpreter: no kernel is compiled for this learned structure
            out.append(jt.infer(ev))
        np.testing.assert_array_equal(out[0][0], out[1][0])
        np.testing.assert_array_equal(out[0][1], out[1][1])
        assert np.isfinite(out[0][1]).all() and (out[0][1] >= 0).all()


def _moral_components(dag):
    """Connected components (sorted node lists) of the moral graph of a DAG given as parent lists."""
    n = len(dag)
    adj = [set() for _ in range(n)]
    for v, ps in enumerate(dag):
        for a in ps:
            adj[v].add(a)
            adj[a].add(v)
            adj[a].update(b for b in ps if b != a)
    seen, comps = set(), []
    for v in range(n):
        if v in seen:
            continue
        stack, comp = [v], []
        while stack:
            x = stack.pop()
            if x not in seen:
                seen.add(x)
                comp.append(x)
                stack.extend(adj[x] - seen)
        comps.append(sorted(comp))
    return comps
