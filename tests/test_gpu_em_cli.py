"""`BayesianNetwork -a 13` (expectation-maximisation) on 200 ALARM rows for 3 iterations: the objective lines
it prints are ExpectationMaximization.fit's values, and the CPTs it writes with --out parse back to
network().node_probs."""
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ALARM, REPO

import fastbn_amd as F

pytestmark = pytest.mark.gpu


def test_cli_em_alarm(tmp_path):
    net = F.Network(os.path.join(ALARM, "alarm.xml"))
    ev, lab = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)
    ev, lab = ev[:200], lab[:200]
    os.makedirs(tmp_path / "alarm")
    F.write_libsvm(str(tmp_path / "alarm" / "rows"), ev, lab)
    os.symlink(os.path.join(ALARM, "alarm.xml"), tmp_path / "alarm" / "alarm.xml")
    out_file = str(tmp_path / "cpts.txt")
    cli = os.path.join(REPO, "fastbn_amd", "BayesianNetwork")
    run = subprocess.run([cli, "-a", "13", "-d", "3", "--tol", "0", "-f3", "alarm/rows", "--out", out_file,
                          "--prefix", str(tmp_path) + "/"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    text = run.stdout
    assert "Algorithm: expectation-maximisation (EM)" in text and "cases = 200" in text
    back, _ = F.load_libsvm(str(tmp_path / "alarm" / "rows"), 37)
    np.testing.assert_array_equal(back, ev)
    em = F.ExpectationMaximization(net, device=0)
    obj = em.fit(ev, max_iters=3, tol=0)
    lines = re.findall(r"iteration (\d+): log-likelihood = (\S+), Q = (\S+)", text)
    assert [int(t) for t, _, _ in lines] == [0, 1, 2]
    got = np.array([[float(a), float(b)] for _, a, b in lines])
    assert got.tobytes() == obj.tobytes()
    assert re.search(r"em: last E-step kernel \S+ s, \S+ cases/s", text)
    learned = em.network()
    rows = [ln.split() for ln in open(out_file).read().splitlines()]
    k = 0
    for v in range(37):
        _, probs = learned.node_probs(v)
        for pc in range(probs.shape[1]):
            assert (int(rows[k][0]), int(rows[k][1])) == (v, pc)
            assert np.array([float(x) for x in rows[k][2:]]).tobytes() == probs[:, pc].tobytes()
            k += 1
    assert k == len(rows)
