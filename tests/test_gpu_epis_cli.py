"""The drop-in CLI's `-a 6` (EPIS-BN) on the ALARM fixtures: the reference's header lines
(src/main.cpp:123-134), then the result lines of `-a 5` / `-a 7`, equal to EPISBN on the same inputs."""
import os
import re
import subprocess

import pytest
from conftest import ALARM, GOLD, REPO, read_pt_file
from test_epis_host import alarm, alarm_cases

import fastbn_amd as F

pytestmark = pytest.mark.gpu


def _cli(*args):
    cli = os.path.join(REPO, "fastbn_amd", "BayesianNetwork")
    out = subprocess.run([cli, *args, "--prefix", GOLD + "/"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_cli():
    out = _cli("-a", "6", "-q", "256", "-d", "20", "--seed", "0")
    assert "Algorithm: EPIS-BN for approximate inference" in out and "#samples = 256, propagation length = 20" in out
    acc = float(re.search(r"accuracy = (\S+)", out).group(1))
    mse = re.search(r"average MSE = (\S+)", out).group(1)
    hd = re.search(r"average HD = (\S+)", out).group(1)
    assert re.search(r"epis: device kernels lbp \S+ s, sampling \S+ s", out)
    net, tup = alarm()
    ev, truth = alarm_cases()
    gold = read_pt_file(os.path.join(ALARM, "alarm_1k_pt"), tup[1], len(ev))
    ep = F.EPISBN(net, 256, iterations=20, seed=0)
    pacc, pmse, phd = ep.EvaluateAccuracy(ev, truth, gold)
    assert "%g" % pmse == mse and "%g" % phd == hd  # iostream's default formatting is %g
    assert abs(acc - pacc) < 5e-7 and acc > 0.9  # accuracy = the share of equal labels: the labels agree
    assert "%g" % (ep.stats[1].sum() / len(ev)) == re.search(r"average ESS = (\S+)", out).group(1)
    # the long flags reach the run
    out2 = _cli("-a", "6", "-q", "64", "-d", "5", "--seed", "4", "--tol", "1e-6", "--damping", "0.5", "--eps", "0")
    p2 = F.EPISBN(net, 64, iterations=5, tol=1e-6, damping=0.5, eps=0.0, seed=4).EvaluateAccuracy(ev, truth, gold)
    assert "%g" % p2[1] == re.search(r"average MSE = (\S+)", out2).group(1)
    assert abs(float(re.search(r"accuracy = (\S+)", out2).group(1)) - p2[0]) < 5e-7
    # the neighbours still work
    assert "likelihood weighting (LW)" in _cli("-a", "5", "-q", "64")
    assert "loopy belief propagation (LBP)" in _cli("-a", "7", "-d", "3")
