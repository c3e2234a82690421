"""`BayesianNetwork -a 14` (hill climbing) on ALARM-5000: the arc count, the score and the iterations it
prints are the host twin's, --out writes the twin's parent lists, and -f1 adds the SHD of that graph through
fbn_shd_bif."""
import os
import re
import subprocess

import pytest
from conftest import ALARM, GOLD, REPO

import fastbn_amd as F
import hc_data as H

pytestmark = pytest.mark.gpu


def test_cli_hc_alarm(tmp_path):
    out_file = str(tmp_path / "dag.txt")
    cli = os.path.join(REPO, "fastbn_amd", "BayesianNetwork")
    run = subprocess.run([cli, "-a", "14", "-f1", "alarm/alarm.bif", "-f2", "alarm/alarm_s5000.txt", "--score", "bic",
                          "--out", out_file, "--prefix", GOLD + "/"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    text = run.stdout
    assert "Algorithm: hill climbing (HC) for score-based structure learning" in text and "alarm/alarm_s5000.txt" in text
    ds = F.Dataset(H.ALARM_CSV)
    host = F.HillClimbing("bic").learn(ds, host=True)
    assert int(re.search(r"^arcs = (\d+)", text, re.M).group(1)) == sum(len(p) for p in host.parents) == 50
    assert int(re.search(r"^iterations = (\d+)", text, re.M).group(1)) == host.iterations
    m = re.search(r"^score = (\S+), log-likelihood = (\S+)", text, re.M)
    assert m.group(1) == "%.17g" % host.score and m.group(2) == "%.17g" % host.loglik
    assert float(m.group(1)) == host.score  # 17 digits round-trip: the twin's bits
    assert re.search(r"hc: \d+ families scored in 53 batches, device kernel \S+ s", text)
    rows = [[int(x) for x in ln.split()] for ln in open(out_file)]
    assert [r[0] for r in rows] == list(range(37)) and all(r[1] == len(r) - 2 for r in rows)
    assert [r[2:] for r in rows] == host.parents
    shd = int(re.search(r"^SHD = (\d+)", text, re.M).group(1))
    assert shd == F.shd_bif(os.path.join(ALARM, "alarm.bif"), 37, host.oriented)
    # no -f1: no SHD line; another score and a parent limit reach the search
    run = subprocess.run([cli, "-a", "14", "--score", "aic", "--max-parents", "1", "--prefix", GOLD + "/"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "SHD" not in run.stdout
    host = F.HillClimbing("aic", max_parents=1).learn(ds, host=True)
    assert int(re.search(r"^arcs = (\d+)", run.stdout, re.M).group(1)) == sum(len(p) for p in host.parents)
    assert "score = aic, max parents = 1" in run.stdout
    assert re.search(r"^score = (\S+), log-likelihood", run.stdout, re.M).group(1) == "%.17g" % host.score
