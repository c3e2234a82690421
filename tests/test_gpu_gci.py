"""The Gaussian CI test on the device: the correlation kernel (gci_corr.hip) against an mpmath reference, the
test kernel (gci_test.hip) and the PC run bit for bit against the host twin on the device's own R, and
`BayesianNetwork -a 19`."""
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import REPO

import fastbn_amd as F
import gci_data as G

pytestmark = pytest.mark.gpu

Q = 2.0 ** 20


def shifted_sem(nvars, N, seed):
    """A sparse SEM quantised to multiples of 2^-20, column 0 (a root, sigma = 1) shifted by 10^6 sigma."""
    X = G.sem(nvars, N, seed, p_edge=2.5 / nvars)
    X[0] += 1e6
    X = np.round(X * Q) / Q
    assert np.abs(X).max() < Q
    return X


def corr_mp(X):
    """R at 40 digits from the exact integer moments of X (multiples of 2^-20 below 2^20): X 2^20 = H 2^20 + L
    with |H|, |L| < 2^20, so every float64 matmul below is a sum of integers under 2^53, exact in any order."""
    N = X.shape[1]
    Xi = X * Q
    H = np.trunc(Xi / Q)
    L = Xi - H * Q
    ints = lambda A: A.astype(np.int64).astype(object)
    gram = ints(H @ H.T) * (1 << 40) + (ints(H @ L.T) + ints(L @ H.T)) * (1 << 20) + ints(L @ L.T)
    s = ints(Xi.sum(axis=1))
    C = N * gram - np.outer(s, s)  # N^2 2^40 times the covariance, exactly
    sd = [G.mpmath.sqrt(G.mpmath.mpf(int(C[i, i]))) for i in range(len(C))]
    return [[G.mpmath.mpf(int(C[i, j])) / (sd[i] * sd[j]) for j in range(len(C))] for i in range(len(C))]


# one ragged tile; a diagonal and an off-diagonal tile with ragged edges; a forced split-K; N not a multiple of 4
# and several slices; the 64-wide tile with ragged edges
@pytest.mark.parametrize("nvars,N,split_k,tile", [(5, 7, 1, 0), (70, 1003, 1, 0), (70, 1003, 3, 0), (130, 4099, 5, 0),
                                                 (130, 4099, 5, 64)])
def test_correlation_against_mpmath(nvars, N, split_k, tile):
    """|dR| <= (N + 16) 2^-51 on every entry: a length-N dot product in any order errs by at most gamma_N
    sqrt(S_ii S_jj); a wrong mean enters in second order only (N e_i e_j, below the first-order term for
    |mu| / sigma <= 10^6 and N <= 4,099); doubled for the normalisation.  A one-pass formula misses it by about
    nine orders of magnitude on the shifted column."""
    X = shifted_sem(nvars, N, seed=nvars)
    ci = F.GaussianIndependenceTest(F.ContinuousDataset(columns=X))
    ci.set_tuning(split_k, tile)
    info = ci.info()
    assert info["split_k"] == split_k and info["tile"] == (tile or 32)
    R = ci.correlation()
    ref = corr_mp(X)
    bound = (N + 16) * 2.0 ** -51
    err = lambda A: max(abs(float(G.mpmath.mpf(float(A[i, j])) - ref[i][j])) for i in range(nvars) for j in range(nvars))
    e_dev, e_np = err(R), err(np.corrcoef(X))
    print(f"nvars={nvars} N={N} split_k={split_k} tile={info['tile']}: device {e_dev:.3g}, numpy {e_np:.3g}, bound {bound:.3g}")
    assert e_np <= bound  # numpy's own two-pass result
    assert e_dev <= bound
    assert (np.diag(R) == 1.0).all() and (R == R.T).all()
    ci.set_tuning(split_k, tile)  # the same tiling again: the same bits
    assert (ci.correlation().view(np.int64) == R.view(np.int64)).all()


@pytest.fixture(scope="module")
def sem70():
    X = G.sem(70, 1003, seed=11, p_edge=2.5 / 70)
    ci = F.GaussianIndependenceTest(F.ContinuousDataset(columns=X))
    return X, ci, ci.correlation()


@pytest.fixture(scope="module")
def sem12():
    X = G.sem(12, 2000, seed=3, p_edge=0.3)
    ci = F.GaussianIndependenceTest(F.ContinuousDataset(columns=X))
    return X, ci, ci.correlation()


@pytest.mark.parametrize("d", range(9))
def test_tests_equal_twin(sem70, d):
    X, ci, R = sem70
    items = G.random_items(70, d, 193, seed=200 + d)
    assert (items[:, 0] > items[:, 1]).any()
    r, z, p, ind = ci.run(items, d)
    hr, hz, hp, hind, _ = F.gci_host_run(R, X.shape[1], items, d)
    assert (r.view(np.int64) == hr.view(np.int64)).all() and (ind == hind).all()
    assert (z.view(np.int64) == hz.view(np.int64)).all() and (p.view(np.int64) == hp.view(np.int64)).all()


def assert_same_pc(dev, host, margin=True):
    assert dev.edges == host.edges and dev.sepset == host.sepset and dev.oriented == host.oriented
    assert list(dev.tests_per_level) == list(host.tests_per_level)
    if not margin:  # (the margin log covers the speculative tests too, which follow the schedule)
        return
    assert list(dev.launched_per_level) == list(host.launched_per_level)
    assert dev.min_margin == host.min_margin and dev.near_alpha == host.near_alpha and dev.degenerate == host.degenerate


@pytest.mark.parametrize("data", ["sem12", "sem70"])
@pytest.mark.parametrize("knobs", [{}, {"FBN_PC_ROUND0": "64", "FBN_PC_GROWTH": "2", "FBN_PC_FULLSPEC": "0"}])
def test_pc_equals_twin(request, monkeypatch, data, knobs):
    X, ci, R = request.getfixturevalue(data)
    plain = F.gci_host_pc_stable(R, X.shape[1])
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    host = F.gci_host_pc_stable(R, X.shape[1])  # the twin under the same schedule
    assert_same_pc(host, plain, margin=False)
    dev = F.PCStable(0.05).StructLearnCompData(F.ContinuousDataset(columns=X)).result
    assert_same_pc(dev, host)
    assert_same_pc(F.PCStable(0.05).StructLearnCompData(ci).result, host)  # the resident context
    if data == "sem70":
        assert len(dev.tests_per_level) >= 4  # reaches level 3


def test_cli_a19(sem12, tmp_path):
    X, ci, R = sem12
    with open(tmp_path / "x.csv", "w") as f:
        f.write(",".join(f"v{i}" for i in range(12)) + "\n")
        f.writelines(",".join(repr(float(v)) for v in row) + "\n" for row in X.T)
    py = F.PCStable(0.05).StructLearnCompData(F.ContinuousDataset(path=str(tmp_path / "x.csv"))).result
    assert_same_pc(py, F.gci_host_pc_stable(R, 2000))
    out = str(tmp_path / "pdag.txt")
    run = subprocess.run([os.path.join(REPO, "fastbn_amd", "BayesianNetwork"), "-a", "19", "-f2", "x.csv", "--out", out,
                          "--prefix", str(tmp_path) + "/"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    cum = [int(m) for m in re.findall(r"Level \d+\.\.\. # of CI-tests is (\d+)", run.stdout)]
    assert cum == list(np.cumsum(py.tests_per_level))
    assert f"# remaining edges = {len(py.edges)}" in run.stdout
    assert [tuple(map(int, ln.split())) for ln in open(out)] == py.oriented
