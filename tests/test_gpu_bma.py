"""Exact arc posteriors on the device (exact_bma.hip behind fbn_bma_run): bit for bit the host twin for every
tiling of the three transforms, the mpmath order enumeration on five variables, and `BayesianNetwork -a 18`."""
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import REPO

import fastbn_amd as F
import hc_data as H
from test_bma_host import check_against_orders

pytestmark = pytest.mark.gpu

SYNTH_KW = {"max_parents": 3}  # 12 variables: 11 lattice bits, 232 of each lattice's 2,048 entries finite


@pytest.fixture(scope="module")
def synth12():
    ds = H.synth12_dataset()
    return ds, F.IndependenceTest(ds), F.ArcPosterior("bde", **SYNTH_KW).learn(ds, host=True)


def assert_same_result(dev, host):
    assert H.bits_equal(dev.arc_prob, host.arc_prob) and H.bits_equal(dev.q_empty, host.q_empty)
    assert dev.log_z == host.log_z and dev.b_full == host.b_full


# 0: the default, a single pass of 11 bits; 3: four passes, 3 + 3 + 3 + 2; 4: three passes, 4 + 4 + 3
@pytest.mark.parametrize("tile_bits,passes", [(0, 1), (3, 4), (4, 3)])
def test_device_equals_twin(synth12, tile_bits, passes):
    ds, ci, host = synth12
    try:
        F.ArcPosterior.set_tuning(ci, tile_bits)
        dev = F.ArcPosterior("bde", **SYNTH_KW).learn(ci)
    finally:
        F.ArcPosterior.set_tuning(ci, 0)
    assert_same_result(dev, host)
    assert dev.info["passes"] == passes and dev.info["levels"] == 13 and dev.info["families_scored"] == 2784
    # fewer lattice bits than a tile (3 variables, two identical columns), and five variables without a limit
    for small in (F.Dataset(columns=H.tie_columns(), dims=np.full(3, 3, np.int32)), H.small_network(24)[0]):
        sci = F.IndependenceTest(small)
        F.ArcPosterior.set_tuning(sci, tile_bits)
        for prior in (0, 1):
            assert_same_result(F.ArcPosterior("bic", prior=prior).learn(sci), F.ArcPosterior("bic", prior=prior).learn(small, host=True))


@pytest.mark.parametrize("score,prior", [("bde", 0), ("bic", 1)])
@pytest.mark.parametrize("seed", H.SMALL_SEEDS)
def test_device_is_order_enumeration(seed, score, prior):
    check_against_orders(F.ArcPosterior(score, prior=prior).learn(H.small_network(seed)[0]), seed, score, "none", prior)


def test_cli_arc_posteriors(synth12, tmp_path):
    ds = synth12[0]
    F.write_csv(str(tmp_path / "ten.csv"), np.ascontiguousarray(ds.columns[:10]))
    loaded = F.Dataset(str(tmp_path / "ten.csv"))  # what the CLI reads: state counts from the data
    py = F.ArcPosterior("bde", max_parents=2, prior="indegree").learn(loaded)
    out_file = str(tmp_path / "arcs.txt")
    run = subprocess.run([os.path.join(REPO, "fastbn_amd", "BayesianNetwork"), "-a", "18", "-f2", "ten.csv", "--score", "bde",
                          "--max-parents", "2", "--prior", "indegree", "--out", out_file, "--prefix", str(tmp_path) + "/"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.search(r"^logZ = (\S+),", run.stdout, re.M).group(1) == "%.17g" % py.log_z
    assert [ln.split() for ln in open(out_file)] == [["%.17g" % x for x in row] for row in py.arc_prob]
    listed = re.findall(r"^(\d+) -> (\d+) (\S+)$", run.stdout, re.M)
    assert listed == [(str(u), str(v), "%.17g" % py.arc_prob[u][v]) for u in range(10) for v in range(10) if py.arc_prob[u][v] >= 0.5]
