"""The Gaussian CI test on the host (gci_elim.h through fbn_gci_host_run / fbn_gci_host_pc_stable): the twin
against 40-digit partial correlations, the twin's PC-stable against a plain Python one, the degenerate rules.

Measured on the 12-variable SEM below (max |r - r_mp| over 40 items per d): the twin 8.2e-17
(d = 0) to 7.3e-16 (d = 8), numpy's inverse 7.8e-17 to 2.2e-16; the bound 8 x numpy with floor 2^-46 = 1.4e-14 held
throughout."""
import numpy as np
import pytest

import fastbn_amd as F
import gci_data as G

ARG, LIMIT = -1, -6  # fbn_err_t (include/fastbn.h)
N12 = 2000


@pytest.fixture(scope="module")
def sem12():
    X = G.sem(12, N12, seed=3, p_edge=0.3)
    return X, np.corrcoef(X)


@pytest.mark.parametrize("d", range(9))
def test_twin_against_mpmath(sem12, d):
    """r of the twin within 8 x the error of numpy's float64 inverse (floor 2^-46), both against mpmath on the
    same float64 R.  8: another elimination order, R_ZZ of condition number <= 100."""
    _, R = sem12
    items = G.random_items(12, d, 40, seed=100 + d)
    cond = max(np.linalg.cond(R[np.ix_(it[2:], it[2:])]) for it in items) if d else 1.0
    assert cond <= 100
    ref = [G.pcorr_mp(R, list(it)) for it in items]
    r, z, p, ind, deg = F.gci_host_run(R, N12, items, d)
    e_twin = max(abs(float(G.mpmath.mpf(float(a)) - b)) for a, b in zip(r, ref))
    e_np = max(abs(float(G.mpmath.mpf(G.pcorr_np(R, list(it))) - b)) for it, b in zip(items, ref))
    print(f"d={d}: twin {e_twin:.3g}, numpy {e_np:.3g}, cond {cond:.3g}")
    assert e_twin <= max(8 * e_np, 2.0 ** -46)
    assert deg == 0
    t = F.gci_tau(0.05, N12, d)
    assert abs(t - G.tau(0.05, N12, d)) <= 1e-15
    np.testing.assert_array_equal(ind, np.abs(r) <= t)
    np.testing.assert_allclose(z, np.sqrt(N12 - d - 3) * np.arctanh(r), rtol=1e-13)
    np.testing.assert_array_equal(ind, p > 0.05)  # the threshold form is the p-value decision


def test_twin_pc_against_plain_restatement(sem12):
    _, R = sem12
    res = F.gci_host_pc_stable(R, N12)
    assert res.min_margin > 1e-6 and res.near_alpha == 0 and res.degenerate == 0  # no decision rests on rounding
    edges, sepset, tests = G.plain_pc(R, N12)
    assert res.edges == edges and res.sepset == sepset and list(res.tests_per_level) == tests
    assert len(tests) >= 3 and 0 < len(edges) < 66
    assert res.oriented == F.orient_skeleton(12, edges, sepset).oriented


def test_degenerate_and_refusals(sem12):
    X, _ = sem12
    Y = X.copy()
    Y[3] = Y[1]  # a duplicated column: R_ZZ of Z = {1, 3} is singular
    r, z, p, ind, deg = F.gci_host_run(np.corrcoef(Y), N12, [[0, 2, 1, 3], [0, 2, 1, 4]], 2)
    assert np.isnan(r[0]) and np.isnan(p[0]) and not ind[0] and deg == 1
    assert np.isfinite(r[1])
    Y[5] = 7.25  # zero variance: refused before any device is touched
    with pytest.raises(F.FastBNError, match="variable 5 has zero variance") as e:
        F.GaussianIndependenceTest(F.ContinuousDataset(columns=Y))
    assert e.value.code == ARG
    with pytest.raises(F.FastBNError, match="samples") as e:  # N - d - 3 <= 0
        F.gci_host_run(np.corrcoef(X), 5, [[0, 2, 1, 3]], 2)
    assert e.value.code == LIMIT
    with pytest.raises(ValueError, match="group_size"):
        F.PCStable().StructLearnCompData(F.ContinuousDataset(columns=X), group_size=2)
