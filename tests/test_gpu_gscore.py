"""The Gaussian family scorer on the device (gscore.hip) against its host twin, bit for bit;
hill climbing on a Gaussian context; `BayesianNetwork -a 14 --score bic-g`."""
import os
import subprocess

import numpy as np
import pytest
from conftest import REPO

import fastbn_amd as F
import gci_data as G

pytestmark = pytest.mark.gpu
bits = lambda a: np.asarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def ci12():
    X = G.sem(12, 400, 7, 0.4)
    X[11] = X[3]  # a duplicated column: the one degenerate family below holds both
    return F.GaussianIndependenceTest(F.ContinuousDataset(columns=X))


def mixed(seed):
    """Every size 0..8 interleaved over the variables 0..10, 40 families each, shuffled; one family holds 3 and 11."""
    rng = np.random.default_rng(seed)
    fams = [[int(v) for v in rng.permutation(11)[:1 + p]] for p in range(9) for _ in range(40)] + [[0, 3, 11]]
    return [fams[i] for i in rng.permutation(len(fams))]


def same_as_twin(ci, fams, score):
    dev = F.family_scores(ci, fams, score=score)
    ndeg = ci.degenerate
    twin = F.family_scores(ci, fams, score=score, host=True)
    assert (bits(dev[0]) == bits(twin[0])).all() and (bits(dev[1]) == bits(twin[1])).all()
    assert ndeg == ci.degenerate
    return ndeg


@pytest.mark.parametrize("score", ["bic", "bge"])
def test_device_equals_twin(ci12, score):
    for n in (0, 1, 255, 256, 257):  # the block edges of one bucket; the empty batch returns cleanly
        assert same_as_twin(ci12, [[f % 11, (f + 1) % 11, (f + 5) % 11] for f in range(n)], score) == 0
    assert same_as_twin(ci12, mixed(1), score) == 1  # bucketing and the scatter by out_index
    assert ci12.score_info() == {"families": 361, "launches": 9, "degenerate": 1}


def test_many_blocks_of_a_wide_context():
    """130 variables (R no longer a few cache lines per row), 40,000 families of every size: 157 blocks in all."""
    ci = F.GaussianIndependenceTest(F.ContinuousDataset(columns=G.sem(130, 300, 9, 0.05)))
    rng = np.random.default_rng(2)
    fams = [[int(v) for v in rng.permutation(130)[:1 + f % 9]] for f in range(40000)]
    assert same_as_twin(ci, fams, "bge") == 0


@pytest.mark.parametrize("score", ["bic", "bge"])
def test_hill_climbing_equals_twin(score):
    ci = F.GaussianIndependenceTest(F.ContinuousDataset(columns=G.sem(8, 2000, 4, 0.4)))
    dev, twin = F.HillClimbing(score).learn(ci), F.HillClimbing(score).learn(ci, host=True)
    assert dev.ci is ci and dev.parents == twin.parents and len(dev.trace) >= 5
    assert [m[:3] for m in dev.trace] == [m[:3] for m in twin.trace]
    assert (bits([m[3] for m in dev.trace]) == bits([m[3] for m in twin.trace])).all()
    assert (bits(dev.node_scores) == bits(twin.node_scores)).all()
    net = F.GaussianParameterLearning(dev.ci).LearnParamsKnowStructCompData(dev.parents)
    assert net.num_nodes == 8


def test_cli_a14_bic_g(tmp_path):
    X = G.sem(8, 2000, 4, 0.4)
    with open(tmp_path / "x.csv", "w") as f:
        f.write(",".join(f"v{i}" for i in range(8)) + "\n")
        f.writelines(",".join(repr(float(v)) for v in row) + "\n" for row in X.T)
    py = F.HillClimbing("bic").learn(F.ContinuousDataset(path=str(tmp_path / "x.csv")))
    out = str(tmp_path / "dag.txt")
    run = subprocess.run([os.path.join(REPO, "fastbn_amd", "BayesianNetwork"), "-a", "14", "--score", "bic-g", "-f2", "x.csv",
                          "--out", out, "--prefix", str(tmp_path) + "/"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert f"arcs = {sum(map(len, py.parents))}" in run.stdout and f"iterations = {py.iterations}" in run.stdout
    assert [list(map(int, ln.split()))[2:] for ln in open(out)] == py.parents
