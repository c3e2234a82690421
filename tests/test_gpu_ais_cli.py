"""The drop-in CLI's `-a 10` (AIS-BN) and `-a 8` (SIS) on the ALARM fixtures: the reference's header
lines (src/main.cpp:175-186, :149-160), then the result lines of `-a 5` / `-a 6`, equal to AISBN /
SelfImportanceSampling on the same inputs.  `-a 9` stays refused."""
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


@pytest.mark.parametrize("alg,cls,head,tag", [
    ("10", F.AISBN, "Algorithm: AIS-BN for approximate inference", "ais-bn"),
    ("8", F.SelfImportanceSampling, "Algorithm: self importance sampling (SIS) for approximate inference", "sis")])
def test_cli(alg, cls, head, tag):
    out = _cli("-a", alg, "-q", "256", "-m", "2", "-l", "96", "--seed", "0")
    assert head in out and "#samples = 256updating interval = 96maximum updating times = 2" in out
    acc = float(re.search(r"accuracy = (\S+)", out).group(1))
    mse = re.search(r"average MSE = (\S+)", out).group(1)
    hd = re.search(r"average HD = (\S+)", out).group(1)
    assert re.search(tag + r": device kernel \S+ s, \S+ samples/s", out)
    net, tup = alarm()
    ev, truth = alarm_cases()
    gold = read_pt_file(os.path.join(ALARM, "alarm_1k_pt"), tup[1], len(ev))
    h = cls(net, 256, max_updates=2, interval=96, seed=0)
    pacc, pmse, phd = h.EvaluateAccuracy(ev, truth, gold)
    assert "%g" % pmse == mse and "%g" % phd == hd  # iostream's default formatting is %g
    assert abs(acc - pacc) < 5e-7 and acc > 0.9  # accuracy = the share of equal labels: the labels agree
    assert "%g" % (h.stats[1].sum() / len(ev)) == re.search(r"average ESS = (\S+)", out).group(1)
    # the long flags reach the run
    out2 = _cli("-a", alg, "-q", "64", "-m", "1", "-l", "32", "--seed", "4", "--eps", "0.01")
    p2 = cls(net, 64, max_updates=1, interval=32, eps=0.01, seed=4).EvaluateAccuracy(ev, truth, gold)
    assert "%g" % p2[1] == re.search(r"average MSE = (\S+)", out2).group(1)
    assert abs(float(re.search(r"accuracy = (\S+)", out2).group(1)) - p2[0]) < 5e-7


def test_cli_refusals_and_neighbours():
    out = _cli("-a", "9")
    assert "SISv1" in out and "accuracy" not in out
    cli = os.path.join(REPO, "fastbn_amd", "BayesianNetwork")
    bad = subprocess.run([cli, "-a", "8", "-q", "64", "--eps", "0", "--prefix", GOLD + "/"], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode == 1 and "cutoff" in bad.stderr
    assert "likelihood weighting (LW)" in _cli("-a", "5", "-q", "64")
    assert "EPIS-BN" in _cli("-a", "6", "-q", "64", "-d", "3")
