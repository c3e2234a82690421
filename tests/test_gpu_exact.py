"""Exact score-optimal structure learning on the device (exact_dp.hip behind fbn_exact_run): bit for bit
the host twin for every tiling of the subset-max transform, the brute-force maximum on five variables, the
greedy learner's score dominated, and `BayesianNetwork -a 17`."""
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import REPO

import fastbn_amd as F
import hc_data as H
from test_exact_host import check_optimum, constraint_kwargs

pytestmark = pytest.mark.gpu

SYNTH_KW = {"max_parents": 3}  # 12 variables: 11 lattice bits, 12 * (1 + 11 + 55 + 165) = 2,784 candidate families


@pytest.fixture(scope="module")
def synth12():
    ds = H.synth12_dataset()
    return ds, F.IndependenceTest(ds), F.ExactSearch("bic", **SYNTH_KW).learn(ds, host=True)


def assert_same_result(dev, host):
    assert dev.parents == host.parents
    assert dev.score == host.score and dev.loglik == host.loglik  # score = R[V]
    assert H.bits_equal(dev.node_scores, host.node_scores) and H.bits_equal(dev.node_logliks, host.node_logliks)


# 0: the default, a single pass of 11 bits; 3: four passes, 3 + 3 + 3 + 2; 4: three passes, 4 + 4 + 3
@pytest.mark.parametrize("tile_bits,passes", [(0, 1), (3, 4), (4, 3)])
def test_device_equals_twin(synth12, tile_bits, passes):
    ds, ci, host = synth12
    try:
        F.ExactSearch.set_tuning(ci, tile_bits)
        dev = F.ExactSearch("bic", **SYNTH_KW).learn(ci)
    finally:
        F.ExactSearch.set_tuning(ci, 0)
    assert_same_result(dev, host)
    assert dev.exact_info["passes"] == passes and dev.exact_info["families_scored"] == 2784 + 12
    # every tie rule: two identical columns; and fewer lattice bits than a tile
    for small in (F.Dataset(columns=H.tie_columns(), dims=np.full(3, 3, np.int32)), H.small_network(24)[0]):
        sci = F.IndependenceTest(small)
        F.ExactSearch.set_tuning(sci, tile_bits)
        assert_same_result(F.ExactSearch("bic").learn(sci), F.ExactSearch("bic").learn(small, host=True))


@pytest.mark.parametrize("kind", ["none", "mask"])
@pytest.mark.parametrize("seed", H.SMALL_SEEDS)
def test_device_optimum_is_brute_force_maximum(seed, kind):
    ds = H.small_network(seed)[0]
    check_optimum(F.ExactSearch("bic", **constraint_kwargs(kind, 5)).learn(ds), ds, "bic", kind)


def test_optimum_dominates_hill_climbing(synth12):
    ds, ci, host = synth12
    ex = F.ExactSearch("bic", **SYNTH_KW)
    assert_same_result(ex.learn(ci), host)
    assert ex.ci is ci
    assert_same_result(F.ExactSearch("bic", **SYNTH_KW).learn(ds), host)  # from the Dataset: its own upload
    hc = F.HillClimbing("bic", **SYNTH_KW).learn(ci)
    N = ds.num_instance
    print(f"exact {ex.score!r}, hill climbing {hc.score!r}")
    assert ex.score >= hc.score - 12 * 1e-12 * 2 * N * np.log(N)


def test_cli_exact(synth12, tmp_path):
    ds = synth12[0]
    ten = F.Dataset(columns=np.ascontiguousarray(ds.columns[:10]), dims=np.ascontiguousarray(ds.dims[:10]))
    F.write_csv(str(tmp_path / "ten.csv"), ten.columns)
    loaded = F.Dataset(str(tmp_path / "ten.csv"))  # what the CLI reads: state counts from the data
    py = F.ExactSearch("bic", max_parents=2).learn(loaded)
    out_file = str(tmp_path / "dag.txt")
    run = subprocess.run([os.path.join(REPO, "fastbn_amd", "BayesianNetwork"), "-a", "17", "-f2", "ten.csv", "--score", "bic",
                          "--max-parents", "2", "--out", out_file, "--prefix", str(tmp_path) + "/"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "exact search (subset-lattice DP)" in run.stdout and "SHD" not in run.stdout
    assert int(re.search(r"^arcs = (\d+)", run.stdout, re.M).group(1)) == sum(len(p) for p in py.parents)
    m = re.search(r"^score = (\S+), log-likelihood = (\S+)", run.stdout, re.M)
    assert m.group(1) == "%.17g" % py.score and m.group(2) == "%.17g" % py.loglik
    rows = [[int(x) for x in ln.split()] for ln in open(out_file)]
    assert [r[0] for r in rows] == list(range(10)) and [r[2:] for r in rows] == py.parents
