"""The Bayesian Dirichlet scores on the device: hc_bd.hip behind fbn_score_families_bd, and the searches over
it, against the host twin (test_bd_host.py holds the twin to mpmath).  Every comparison is equality of bits:
both sides evaluate hc_bd.h, and the packed sub-group fold performs the header's additions."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import GOLD, REPO

import fastbn_amd as F
import hc_data as H
from test_bd_host import BD_FAMILIES, BD_NS, BD_SCORES, bd_dataset, check_score_equivalence

pytestmark = pytest.mark.gpu

# 159 families, all seven width classes in one batch, none filled to a multiple of its pack factor, so each
# packed class has a partly filled last wave: 81 with q = 1 (w = 1: a full wave of 64 and 17 sub-groups of
# the next), 39 with q = 2 (w = 2: 32 + 7), 3 with q = 3 (w = 4: 3 of 16), 10 with q = 6 (w = 8: 8 + 2), 6 with
# q = 9 (w = 16: 4 + 2), 7 with q = 31, 32 (w = 32: three waves of 2 and 1), 13 with a wave each (q = 33, 64, 65,
# 4096); three have r = 1
MIXED = (BD_FAMILIES + [(c,) for c in range(11)] * 7 + [(c, 3) for c in (0, 1, 2, 4, 5)] * 7 + [(0, 5)]
         + [(0, 3, 4), (2, 3, 4)] * 5 + [(0, 1, 4), (2, 1, 4)] * 3)


@functools.lru_cache(maxsize=None)
def twin(N, score):
    ll, sc = F.family_scores(bd_dataset(N), MIXED, score=score)
    return ll, sc


def same_bits(got, ref):
    return all(H.bits_equal(g, r) for g, r in zip(got, ref))


@pytest.mark.parametrize("score", BD_SCORES, ids=str)
@pytest.mark.parametrize("N", BD_NS)
def test_device_equals_twin(N, score):
    ci = F.IndependenceTest(bd_dataset(N))
    got = F.family_scores(ci, MIXED, score=score)
    assert same_bits(got, twin(N, score))
    assert H.bits_equal(got[0], F.family_scores(ci, MIXED, 0.0)[0])  # the BIC path's log-likelihood bits
    assert ci.last_kernel_ms() > 0.0
    try:
        F.HillClimbing.set_bd_tuning(ci, 0)  # one wave per family
        assert same_bits(F.family_scores(ci, MIXED, score=score), twin(N, score))
    finally:
        F.HillClimbing.set_bd_tuning(ci, 1)


@pytest.mark.parametrize("pack", [1, 0])
def test_chunks_and_counting_paths(pack):
    N, score = 5000, ("bde", 1)
    ci = F.IndependenceTest(bd_dataset(N))
    pl = F.ParameterLearning(ci)
    F.HillClimbing.set_bd_tuning(ci, pack)
    for cap, slice_, lds in ((0, 300, 16), (0, 0, -1), (200, 1024, 0), (5000, 0, -1)):
        F.HillClimbing.set_tuning(ci, cap)
        pl.set_tuning(samples_per_slice=slice_, lds_cells_max=lds)
        assert same_bits(F.family_scores(ci, MIXED, score=score), twin(N, score)), (cap, slice_, lds)


def test_bdeu_is_score_equivalent_on_the_device():
    pytest.importorskip("mpmath")
    check_score_equivalence(1.0, F.IndependenceTest)


def assert_same_search(dev, host):
    assert dev.trace == host.trace, H.first_divergence(dev.trace, host.trace)
    assert dev.parents == host.parents and dev.score == host.score and dev.loglik == host.loglik
    assert H.bits_equal(dev.node_scores, host.node_scores) and H.bits_equal(dev.node_logliks, host.node_logliks)


@pytest.fixture(scope="module")
def alarm():
    ds = F.Dataset(H.ALARM_CSV)
    return ds, F.IndependenceTest(ds)


def test_hill_climbing_alarm(alarm):
    ds, ci = alarm
    host = F.HillClimbing("bde").learn(ds, host=True)
    dev = F.HillClimbing("bde").learn(ci)
    assert_same_search(dev, host)
    assert dev.iterations > 30 and H.is_acyclic(dev.parents) and dev.kernel_ms > 0.0
    assert_same_search(F.HillClimbing("k2").learn(ci), F.HillClimbing("k2").learn(ds, host=True))


def test_hill_climbing_within_pc_skeleton(alarm):
    ds, _ = alarm
    pc = F.PCStable(0.05, 1000).StructLearnCompData(ds)
    mask = np.zeros((ds.num_vars, ds.num_vars), np.uint8)
    for x, y in pc.edges:
        mask[x, y] = mask[y, x] = 1
    dev = F.HillClimbing("bde", allowed=mask).learn(pc.ci)
    assert_same_search(dev, F.HillClimbing("bde", allowed=mask).learn(ds, host=True))
    assert dev.iterations > 20 and H.skeleton(dev.parents) <= {tuple(sorted(e)) for e in pc.edges}


def test_exact_search_alarm10(alarm):
    ds, _ = alarm
    d10 = F.Dataset(columns=np.ascontiguousarray(ds.columns[:10]), dims=ds.dims[:10])
    ci = F.IndependenceTest(d10)
    dev = F.ExactSearch("bde", max_parents=2).learn(ci)
    assert_same_search(dev, F.ExactSearch("bde", max_parents=2).learn(d10, host=True))
    assert dev.score >= F.HillClimbing("bde", max_parents=2).learn(ci).score
    ll, sc = F.family_scores(ci, H.families_of(dev.parents), score="bde")
    assert H.bits_equal(sc, dev.node_scores) and H.bits_equal(ll, dev.node_logliks)


def test_refused(alarm):
    _, ci = alarm
    for bad in (("bde", 0), ("bde", float("nan"))):
        for call in (lambda: F.family_scores(ci, [(0,)], score=bad), lambda: F.HillClimbing(bad).learn(ci),
                     lambda: F.ExactSearch(bad).learn(ci)):
            with pytest.raises(F.FastBNError) as e:
                call()
            assert e.value.code == H.ARG
    with pytest.raises(F.FastBNError):
        F.HillClimbing("bdeu").learn(ci)


@pytest.mark.parametrize("algo, args, learner", [
    ("14", ["--score", "bde", "--iss", "1"], lambda ds: F.HillClimbing(("bde", 1)).learn(ds, host=True)),
    ("17", ["--score", "k2", "--max-parents", "2", "-f2", "alarm10.txt"], lambda ds: F.ExactSearch("k2", max_parents=2).learn(ds, host=True)),
])
def test_cli(tmp_path, alarm, algo, args, learner):
    ds, prefix = alarm[0], GOLD + "/"
    if algo == "17":  # the first 10 ALARM columns as a CSV of their own
        lines = open(H.ALARM_CSV).read().splitlines()
        (tmp_path / "alarm10.txt").write_text("\n".join(",".join(ln.split(",")[:10]) for ln in lines) + "\n")
        ds, prefix = F.Dataset(str(tmp_path / "alarm10.txt")), str(tmp_path) + "/"
    out_file = str(tmp_path / "dag.txt")
    run = subprocess.run([os.path.join(REPO, "fastbn_amd", "BayesianNetwork"), "-a", algo, *args, "--out", out_file,
                          "--prefix", prefix], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    host = learner(ds)
    m = re.search(r"^score = (\S+), log-likelihood = (\S+)", run.stdout, re.M)
    assert m.group(1) == "%.17g" % host.score and m.group(2) == "%.17g" % host.loglik
    assert [[int(x) for x in ln.split()][2:] for ln in open(out_file)] == host.parents
