"""Score-based structure learning on the device: hc_score.hip behind fbn_score_families, and fbn_hc_run's
search over it, against the host twin (hc_search.cpp; test_hc_host.py pins the twin itself).  Every
comparison of scores is equality of bits: the device gathers from the host-built n ln n table and adds in
the order of hc_score.h, as the twin does."""
import functools

import numpy as np
import pytest

import fastbn_amd as F
import hc_data as H

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def host_scores(N, name):
    ds = H.edge_dataset(N)
    ll, sc = F.family_scores(ds, H.EDGE_FAMILIES, F.hc_penalty(name, N))
    ll.setflags(write=False)
    sc.setflags(write=False)
    return ll, sc


def assert_bits(got, ref, what):
    for g, r, name in zip(got, ref, ("loglik", "score")):
        assert g.shape == r.shape, (what, name)
        bad = np.flatnonzero(g.view(np.int64) != r.view(np.int64))
        assert bad.size == 0, (what, name, int(bad[0]), float(g[bad[0]]), float(r[bad[0]]))


@pytest.mark.parametrize("N", H.EDGE_NS)
def test_kernel_edges_bit_identical(N):
    """q in {1, 2, 63, 64, 65, 4096}, r in {1, 2, 256}, the 12,288-cell family on the global counting path,
    never-occurring states, at sample counts that are no multiple of 4 or 16."""
    ci = F.IndependenceTest(H.edge_dataset(N))
    pen = F.hc_penalty("bic", N)
    got = F.family_scores(ci, H.EDGE_FAMILIES, pen)
    assert_bits(got, host_scores(N, "bic"), N)
    assert ci.last_kernel_ms() > 0.0
    # the log-likelihood does not depend on the penalty; the score of "loglik" is the log-likelihood
    ll0, sc0 = F.family_scores(ci, H.EDGE_FAMILIES, 0.0)
    assert_bits((ll0, sc0), (got[0], got[0]), (N, "loglik"))
    # an independent check that the bits are the right number
    for f in (2, 10, 12, 14, 16):
        rl, rs, mag = H.np_family(H.edge_columns(N), H.EDGE_DIMS, H.EDGE_FAMILIES[f], pen)
        assert abs(got[0][f] - rl) <= 1e-12 * mag and abs(got[1][f] - rs) <= 1e-12 * (mag + abs(rs - rl))


def test_counting_paths_and_slices():
    """The LDS and the global counting path forced, and multi-slice merging, at N = 1003."""
    N = 1003
    ci = F.IndependenceTest(H.edge_dataset(N))
    pl = F.ParameterLearning(ci)
    ref = host_scores(N, "aic")
    for slice_, lds in ((300, 0), (300, 16), (0, -1), (64, -1), (0, 0)):
        pl.set_tuning(samples_per_slice=slice_, lds_cells_max=lds)
        assert_bits(F.family_scores(ci, H.EDGE_FAMILIES, 1.0), ref, (slice_, lds))


@pytest.mark.parametrize("nfam", [1, 3, 5, 257])
def test_batch_sizes(nfam):
    """One wave per family, four families per workgroup: a lone family, a partial workgroup, one family into
    the second workgroup, and 64 workgroups and one wave."""
    N = 1003
    ci = F.IndependenceTest(H.edge_dataset(N))
    idx = [(7 * k + 3) % len(H.EDGE_FAMILIES) for k in range(nfam)]
    ref = host_scores(N, "bic")
    got = F.family_scores(ci, [H.EDGE_FAMILIES[i] for i in idx], F.hc_penalty("bic", N))
    assert_bits(got, (ref[0][idx], ref[1][idx]), nfam)


def test_chunks_and_position_in_the_batch():
    """The chunk cap lowered to 10,000 cells: the batch spans more than three chunks, the 12,288-, 16,384- and
    16,640-cell families sit alone in theirs.  A family alone, in the middle of a batch and repeated gives
    the same bits under either chunking."""
    N = 1003
    ci = F.IndependenceTest(H.edge_dataset(N))
    pen = F.hc_penalty("bic", N)
    ref = host_scores(N, "bic")
    cells = [int(np.prod(H.EDGE_DIMS[list(f)], dtype=np.int64)) for f in H.EDGE_FAMILIES]
    assert sum(cells) > 3 * 10_000 and sum(c > 10_000 for c in cells) == 3
    big = H.EDGE_FAMILIES.index((9, 6, 7, 8))
    try:
        for cap in (10_000, 1, 0):
            F.HillClimbing.set_tuning(ci, cap)
            assert_bits(F.family_scores(ci, H.EDGE_FAMILIES, pen), ref, cap)
            alone = F.family_scores(ci, [H.EDGE_FAMILIES[big]], pen)
            assert_bits(alone, (ref[0][big:big + 1], ref[1][big:big + 1]), (cap, "alone"))
            fams = [H.EDGE_FAMILIES[0], H.EDGE_FAMILIES[big], H.EDGE_FAMILIES[3], H.EDGE_FAMILIES[big], H.EDGE_FAMILIES[big]]
            idx = [0, big, 3, big, big]
            assert_bits(F.family_scores(ci, fams, pen), (ref[0][idx], ref[1][idx]), (cap, "repeated"))
    finally:
        F.HillClimbing.set_tuning(ci, 0)


def test_errors_are_refused_on_the_host_and_leave_the_context_usable():
    N = 15
    ci = F.IndependenceTest(H.edge_dataset(N))
    for bad, code in (([(0, 13)], H.ARG), ([(0, 0)], H.ARG), ([(0, 3, 3)], H.ARG), ([()], H.ARG),
                      ([(0,), (2, 3, 4, 5, 0)], H.LIMIT)):
        with pytest.raises(F.FastBNError) as e:
            F.family_scores(ci, bad, 0.0)
        assert e.value.code == code, bad
    with pytest.raises(F.FastBNError) as e:
        F.family_scores(ci, [(0,)], -1.0)
    assert e.value.code == H.ARG
    # the table cap, by the sizing path alone: no data of that size
    with pytest.raises(F.FastBNError) as e:
        F.hc_table_bytes((1 << 24) + 1)
    assert e.value.code == H.LIMIT
    assert_bits(F.family_scores(ci, H.EDGE_FAMILIES, 1.0), host_scores(N, "aic"), "after errors")


# ---------------------------------------------------------------- search parity
def assert_same_search(dev, host):
    assert dev.trace == host.trace, H.first_divergence(dev.trace, host.trace)  # deltas compared as floats: exact
    assert dev.parents == host.parents
    assert dev.score == host.score and dev.loglik == host.loglik
    assert H.bits_equal(dev.node_scores, host.node_scores) and H.bits_equal(dev.node_logliks, host.node_logliks)
    assert dev.iterations == host.iterations and dev.families_scored == host.families_scored
    assert dev.info["batches"] == host.info["batches"]


@pytest.fixture(scope="module")
def alarm():
    ds = F.Dataset(H.ALARM_CSV)
    return ds, F.IndependenceTest(ds), F.HillClimbing("bic").learn(ds, host=True)


def test_search_parity_alarm(alarm):
    ds, ci, host = alarm
    dev = F.HillClimbing("bic").learn(ci)
    assert dev.ci is ci
    assert_same_search(dev, host)
    assert dev.iterations == 52 and sum(len(p) for p in dev.parents) == 50
    assert dev.kernel_ms > 0.0 and dev.info["first_sweep_kernel_ms"] > 0.0
    # forced chunking (the first sweep's 1,369 families in chunks of at most 200 cells) and the global path
    pl = F.ParameterLearning(ci)
    try:
        F.HillClimbing.set_tuning(ci, 200)
        pl.set_tuning(samples_per_slice=1024, lds_cells_max=-1)
        assert_same_search(F.HillClimbing("bic").learn(ci), host)
    finally:
        F.HillClimbing.set_tuning(ci, 0)
        pl.set_tuning()


def test_search_parity_synth12():
    ds = H.synth12_dataset(1003)
    for score in ("bic", "aic"):
        host = F.HillClimbing(score).learn(ds, host=True)
        assert host.iterations >= 5 and H.is_acyclic(host.parents)
        assert_same_search(F.HillClimbing(score).learn(ds), host)


@pytest.mark.parametrize("cap", [12, 2])
def test_start_family_above_max_family_cells(cap):
    """A start family of 27 cells against max_family_cells = 12 and 2: counted and scored as the 27-cell table
    it is (the option limits candidate operations only), as the twin does."""
    ds = F.Dataset(columns=H.tie_columns(), dims=np.array([3, 3, 3], np.int32))
    start = [[], [], [0, 1]]
    for max_iter in (0, None):
        host = F.HillClimbing("bic", start=start, max_family_cells=cap, max_iter=max_iter).learn(ds, host=True)
        assert_same_search(F.HillClimbing("bic", start=start, max_family_cells=cap, max_iter=max_iter).learn(ds), host)
    _, sc = F.family_scores(ds, H.families_of(start), F.hc_penalty("bic", ds.num_instance))
    at = F.HillClimbing("bic", start=start, max_family_cells=cap, max_iter=0).learn(ds)
    assert H.bits_equal(at.node_scores, sc)


def test_search_within_pc_skeleton_and_from_pc_dag(alarm):
    ds, _, _ = alarm
    pc = F.PCStable(0.05, 1000).StructLearnCompData(ds)
    n = ds.num_vars
    mask = np.zeros((n, n), np.uint8)
    for x, y in pc.edges:
        mask[x, y] = mask[y, x] = 1
    host = F.HillClimbing("bic", allowed=mask).learn(ds, host=True)
    dev = F.HillClimbing("bic", allowed=mask).learn(pc.ci)  # the context PC-stable ran on
    assert dev.ci is pc.ci
    assert_same_search(dev, host)
    assert dev.iterations > 20 and H.skeleton(dev.parents) <= {tuple(sorted(e)) for e in pc.edges}
    dag = F.pdag_to_dag(n, pc.oriented)
    host = F.HillClimbing("bic", start=dag).learn(ds, host=True)
    dev = F.HillClimbing("bic", start=dag).learn(pc.ci)
    assert_same_search(dev, host)
    start = F.HillClimbing("bic", start=dag, max_iter=0).learn(pc.ci)
    assert start.parents == dag and dev.iterations > 0 and dev.score > start.score and H.is_acyclic(dev.parents)


def test_pipeline_learn_structure_parameters_infer(alarm):
    """HillClimbing -> ParameterLearning(hc.ci) -> JunctionForest.infer on one upload; the marginals against
    the oracle's junction tree on the learned network, component by component of its moral graph (the oracle
    builds a junction tree, not a forest)."""
    import oracle as O
    ds, ci, host = alarm
    hc = F.HillClimbing("bic").learn(ci)
    net = F.ParameterLearning(hc.ci).LearnParamsKnowStructCompData(hc.parents, names=ds.names)
    fam = [net.node_counts(v) for v in range(net.num_nodes)]
    assert [list(p) for p, _ in fam] == hc.parents
    ev = net.evidence_cases(64, 7, seed=1)
    jf = F.JunctionForest(net, device=0)
    jf.set_variant(0)  # the interpreter: no kernel is compiled for this learned structure
    lab, marg = jf.infer(ev)
    assert np.isfinite(marg).all() and (marg >= 0).all()
    off = np.concatenate([[0], np.cumsum(ds.dims)])
    comps = [c for c in jf.components if len(c) > 1]
    assert sum(len(c) for c in comps) >= 30
    for comp in comps:
        new = {v: i for i, v in enumerate(comp)}
        oj = O.OracleJT.from_counts(ds.dims[comp], [[new[q] for q in hc.parents[v]] for v in comp], [fam[v][1] for v in comp])
        _, om = oj.infer(ev[:, comp])
        got = np.concatenate([marg[:, off[v]:off[v + 1]] for v in comp], axis=1)
        np.testing.assert_allclose(got, om, rtol=1e-12, atol=1e-300)
