"""`BayesianNetwork -a 12` (most probable explanation) on ALARM's 1k fixture: the assignments it writes with
--out are MostProbableExplanation.infer's, and the mean log P(x*, e) it prints is theirs to the digits
printed."""
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ALARM, GOLD, REPO

import fastbn_amd as F

pytestmark = pytest.mark.gpu


def test_cli_mpe_alarm(tmp_path):
    out_file = str(tmp_path / "mpe.libsvm")
    cli = os.path.join(REPO, "fastbn_amd", "BayesianNetwork")
    run = subprocess.run([cli, "-a", "12", "--out", out_file, "--prefix", GOLD + "/"], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    text = run.stdout
    assert "Algorithm: most probable explanation (MPE)" in text and "alarm/alarm.xml" in text
    net = F.Network(os.path.join(ALARM, "alarm.xml"))
    ev, _ = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)
    assign, log_p = F.MostProbableExplanation(net, device=0).infer(ev)
    assert int(re.search(r"cases = (\d+)", text).group(1)) == len(ev) == 1000
    got, labels = F.load_libsvm(out_file, 37)
    np.testing.assert_array_equal(got, assign)
    np.testing.assert_array_equal(labels, assign[:, 0])
    printed = re.search(r"mean log P\(x\*, e\) = (\S+)", text).group(1)
    total = 0.0
    for x in log_p.tolist():  # the CLI's sum: case order, one add per case
        total += x
    assert printed == "%.12g" % (total / len(ev))
    assert re.search(r"mpe: device kernel \S+ s, \S+ cases/s", text)
