"""Small linear-Gaussian networks and evidence batches shared by test_ginf_host.py and test_gpu_ginf.py, with
their plain references: the joint by matrix inverse (numpy) and the conditioning at 40 digits (mpmath)."""
import numpy as np

# Coefficients in +-[0.3, 1], variances in [0.5, 2], at most two parents among the eight nodes before a node (in
# a shuffled labelling, so Kahn's order is not the index order).  Largest condition number of Sigma_EE over every
# batch the two test files draw (numpy.linalg.cond when this module was written): 1.8e2, at (n, m) = (128, 128).


def make(n, seed):
    """(parents, intercept, coef, variance) of a seeded network over n nodes."""
    rng = np.random.default_rng(seed)
    label = rng.permutation(n)
    parents, coef = [[] for _ in range(n)], [[] for _ in range(n)]
    for k in range(1, n):
        lo = max(0, k - 8)
        ps = rng.choice(np.arange(lo, k), size=min(k - lo, int(rng.integers(0, 3))), replace=False)
        parents[label[k]] = [int(label[p]) for p in ps]
        coef[label[k]] = list(rng.uniform(0.3, 1.0, len(ps)) * rng.choice([-1.0, 1.0], len(ps)))
    return parents, rng.normal(size=n), coef, rng.uniform(0.5, 2.0, n)


def joint_np(parents, intercept, coef, variance):
    """mu = (I - W)^-1 b, Sigma = (I - W)^-1 diag(s) (I - W)^-T."""
    n = len(parents)
    W = np.zeros((n, n))
    for v in range(n):
        W[v, parents[v]] = coef[v]
    A = np.linalg.inv(np.eye(n) - W)
    return A @ np.asarray(intercept), A @ np.diag(variance) @ A.T


def cases(mu, S, m, ncases, seed):
    """ncases rows with exactly m observed values each (a pattern of its own per row), drawn around the prior."""
    rng = np.random.default_rng(seed)
    n = len(mu)
    ev = np.full((ncases, n), np.nan)
    for c in range(ncases):
        E = rng.permutation(n)[:m]
        ev[c, E] = mu[E] + np.sqrt(np.diag(S)[E]) * rng.normal(size=m)
    return ev


def condition(mu, S, x, solve, sub, ln2pi):
    """(mean, var, logp) of one case by the textbook formulas over a linear solver: numpy's or mpmath's."""
    E = [v for v in range(len(x)) if x[v] == x[v]]
    U = [v for v in range(len(x)) if x[v] != x[v]]
    mean, var = list(x), [0.0] * len(x)
    if not E:
        return [mu[v] for v in U], [S[v][v] for v in U], 0.0
    SEE = sub(S, E, E)
    delta = [x[e] - mu[e] for e in E]
    z, logdet = solve(SEE, delta)
    quad = sum(d * zz for d, zz in zip(delta, z))
    for u in U:
        col = [S[e][u] for e in E]
        k, _ = solve(SEE, col)
        mean[u] = mu[u] + sum(c * zz for c, zz in zip(col, z))
        var[u] = S[u][u] - sum(c * kk for c, kk in zip(col, k))
    return [mean[u] for u in U], [var[u] for u in U], -(len(E) * ln2pi + logdet + quad) / 2


def condition_np(mu, S, x):
    def solve(A, b):
        return np.linalg.solve(np.asarray(A), np.asarray(b)), np.linalg.slogdet(np.asarray(A))[1]
    return condition(mu, S, x, solve, lambda M, r, c: M[np.ix_(r, c)], np.log(2 * np.pi))


def condition_mp(mu, S, x):
    import mpmath
    mpmath.mp.dps = 40
    Sm = [[mpmath.mpf(float(a)) for a in row] for row in S]
    mm = [mpmath.mpf(float(a)) for a in mu]
    xm = [mpmath.mpf(float(a)) if a == a else a for a in x]

    def solve(A, b):
        A = mpmath.matrix(A)
        return list(mpmath.lu_solve(A, mpmath.matrix(b))), mpmath.log(mpmath.det(A))
    return condition(mm, Sm, xm, solve, lambda M, r, c: [[M[i][j] for j in c] for i in r], mpmath.log(2 * mpmath.pi))
