"""Linear-Gaussian networks on the host: the joint, parameter learning, the host twin of the inference kernel
against mpmath, its conventions and the errors of the C entries.  No device."""
import numpy as np
import pytest

import fastbn_amd as F
import ginf_nets as G

ARG, NODEV, LIMIT = -1, -5, -6


def network(n, seed):
    return F.GaussianNetwork(*G.make(n, seed))


def test_joint_against_matrix_inverse():
    """A collider 0 -> 2 <- 1, a chain 2 -> 3 -> 4 and the isolated node 5."""
    parents = [[], [], [1, 0], [2], [3], []]
    coef = [[], [], [0.8, -0.5], [0.6], [-0.9], []]
    b, s = np.array([1.0, -2.0, 0.5, 0.0, 3.0, -1.0]), np.array([1.0, 0.5, 2.0, 1.5, 0.7, 1.2])
    mu, S = F.GaussianNetwork(parents, b, coef, s).joint()
    mu_ref, S_ref = G.joint_np(parents, b, coef, s)
    assert np.abs(mu - mu_ref).max() <= 1e-14 * np.abs(mu_ref).max()
    assert np.abs(S - S_ref).max() <= 1e-14 * np.abs(S_ref).max()
    assert (S == S.T).all() and S[5, 5] == s[5] and (S[5, :5] == 0).all()


def test_parameter_learning_against_lstsq():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(5, 400)) * np.array([1.0, 3.0, 0.5, 2.0, 1.0])[:, None] + np.array([0, 5, -2, 1, 10.0])[:, None]
    X[2] += 0.7 * X[0]
    X[3] += 0.5 * X[1] - 1.2 * X[2]
    X[4] += 0.3 * X[3] + 0.9 * X[0] - 0.4 * X[1]
    parents = [[], [], [0], [2, 1], [3, 0, 1]]
    mean = X.mean(axis=1)
    Xc = X - mean[:, None]
    b, w, s = F.gnet_learn_host(mean, (Xc * Xc).sum(axis=1), np.corrcoef(X), 400, parents).params()
    for v, ps in enumerate(parents):
        beta = np.linalg.lstsq(Xc[ps].T, Xc[v], rcond=None)[0]
        res = Xc[v] - beta @ Xc[ps]
        assert np.allclose(w[v], beta, rtol=1e-11, atol=0)
        assert np.isclose(b[v], mean[v] - beta @ mean[ps], rtol=1e-11, atol=1e-12)
        assert np.isclose(s[v], res @ res / 400, rtol=1e-11, atol=0)


def test_twin_against_mpmath():
    """Measured over the 18 cases: the twin's worst error 5.5e-16 (mean), 3.0e-16 (variance), 3.4e-16 (log
    density); numpy.linalg.solve's 7.0e-16, 5.2e-16, 1.3e-16.  Mean errors are relative to |mean| + sd, variance
    errors to (|mean| + sd)^2, log-density errors to |logp| + 1.  The twin may exceed numpy's worst by a factor of
    8: headroom for a different but equally stable elimination order."""
    pytest.importorskip("mpmath")
    worst = np.zeros((2, 3))
    for n, m in [(12, 5), (37, 7)]:
        spec = G.make(n, seed=n)
        mu, S = F.GaussianNetwork(*spec).joint()
        ev = G.cases(mu, S, m, 9, seed=100 * n + m)
        mean, var, logp = F.GaussianInference(F.GaussianNetwork(*spec), device=-1).infer(ev)
        for c, x in enumerate(ev):
            U = np.flatnonzero(x != x)
            rm, rv, rl = G.condition_mp(mu, S, x)
            nm, nv, nl = G.condition_np(mu, S, x)
            scale = np.array([abs(float(a)) + float(b) ** 0.5 for a, b in zip(rm, rv)])
            for k, (gm, gv, gl) in enumerate([(mean[c, U], var[c, U], logp[c]), (nm, nv, nl)]):
                em = max(abs(float(a - b)) / q for a, b, q in zip(gm, rm, scale))
                evr = max(abs(float(a - b)) / q ** 2 for a, b, q in zip(gv, rv, scale))
                worst[k] = np.maximum(worst[k], [em, evr, abs(float(gl - rl)) / (abs(float(rl)) + 1)])
    print("twin", worst[0], "numpy", worst[1])
    assert (worst[0] <= 8 * worst[1]).all()


@pytest.mark.parametrize("kind", ["prior", "all_observed", "observed_exact", "duplicate"])
def test_conventions(kind):
    net = network(9, seed=9)
    mu, S = net.joint()
    inf = F.GaussianInference(net, device=-1)
    x = np.full(9, np.nan)
    if kind == "prior":
        mean, var, logp = inf.infer(x)
        assert (mean[0] == mu).all() and (var[0] == np.diag(S)).all() and logp[0] == 0.0 and not np.signbit(logp[0])
    elif kind == "all_observed":
        x[:] = mu + 0.5
        mean, var, logp = inf.infer(x)
        ref = -0.5 * (9 * np.log(2 * np.pi) + np.linalg.slogdet(S)[1] + 0.25 * np.linalg.inv(S).sum())
        assert (mean[0] == x).all() and (var[0] == 0).all() and np.isclose(logp[0], ref, rtol=1e-13)
    elif kind == "observed_exact":
        x[[2, 6]] = [0.25, -1.5]
        mean, var, _ = inf.infer(x)
        assert (mean[0, [2, 6]] == [0.25, -1.5]).all() and (var[0, [2, 6]] == 0).all()
        assert not np.signbit(var[0, [2, 6]]).any() and (var[0, [0, 1, 3, 4, 5, 7, 8]] > 0).all()
    else:
        # node 2 copies node 0 up to a variance that Sigma cannot hold: two collinear observed variables
        dup = F.GaussianNetwork([[], [0], [0]], [0.0, 1.0, 0.0], [[], [0.5], [1.0]], [1.0, 1.0, 1e-30])
        inf = F.GaussianInference(dup, device=-1)
        ev = np.array([[0.3, np.nan, 0.3], [0.3, np.nan, np.nan]])
        mean, var, logp = inf.infer(ev)
        assert inf.degenerate == 1 and inf.info()["degenerate"] == 1
        assert np.isnan(mean[0]).all() and np.isnan(var[0]).all() and np.isnan(logp[0])
        assert np.isfinite(mean[1]).all() and np.isfinite(logp[1])


def test_errors():
    def code(call):
        with pytest.raises(F.FastBNError) as e:
            call()
        return e.value.code

    assert code(lambda: F.GaussianNetwork([[1], [2], [0]], [0.0] * 3, [[1.0]] * 3, [1.0] * 3)) == ARG
    assert code(lambda: F.GaussianNetwork([[], [0]], [0.0, 0.0], [[], [1.0]], [1.0, 0.0])) == ARG
    net = network(130, seed=130)
    inf = F.GaussianInference(net, device=-1)
    x = np.full(130, np.nan)
    x[7] = np.inf
    assert code(lambda: inf.infer(x)) == ARG and "variable 7" in str(F.lib.fbn_last_error())
    x[:129] = 0.0
    assert code(lambda: inf.infer(x)) == LIMIT and "129" in str(F.lib.fbn_last_error())
    x[0] = np.nan
    assert np.isfinite(inf.infer(x)[2]).all()  # 128 observed: the cap itself
    assert code(lambda: inf.run_device(0, 1)) == NODEV
    X = np.random.default_rng(1).normal(size=(4, 50))
    X[3] = X[1]
    mean = X.mean(axis=1)
    ss = ((X - mean[:, None]) ** 2).sum(axis=1)
    assert code(lambda: F.gnet_learn_host(mean, ss, np.corrcoef(X), 50, [[], [], [1, 3], []])) == ARG
    assert "node 2" in str(F.lib.fbn_last_error())
    assert code(lambda: F.gnet_learn_host(mean, ss, np.corrcoef(X), 50, [[], [], [], [1]])) == ARG  # a copy of its parent
