"""Data and plain references of the Gaussian CI tests (test_gci_host.py, test_gpu_gci.py): a seeded
linear-Gaussian SEM, partial correlations by matrix inverse (numpy float64 and mpmath at 40 digits) and a
plain Python PC-stable."""
import itertools
import math
from statistics import NormalDist

import mpmath
import numpy as np

mpmath.mp.dps = 40


def sem(nvars, N, seed, p_edge):
    """Columns [nvars][N] of x_j = sum_{i<j} w_ij x_i + e_j, |w| in [0.4, 0.9], each arc present with p_edge."""
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.4, 0.9, (nvars, nvars)) * rng.choice([-1.0, 1.0], (nvars, nvars))
    W = np.triu(W * (rng.random((nvars, nvars)) < p_edge), 1)
    X = np.zeros((nvars, N))
    for j in range(nvars):
        X[j] = W[:j, j] @ X[:j] + rng.standard_normal(N)
    return X


def random_items(nvars, d, n, seed):
    """n tests (x, y, z...) of distinct variables; x > y in about half of them."""
    rng = np.random.default_rng(seed)
    return np.array([rng.permutation(nvars)[:2 + d] for _ in range(n)], np.int32)


def pcorr_np(R, item):
    P = np.linalg.inv(R[np.ix_(item, item)])
    return -P[0, 1] / math.sqrt(P[0, 0] * P[1, 1])


def pcorr_mp(R, item):
    P = mpmath.matrix(R[np.ix_(item, item)].tolist()) ** -1
    return -P[0, 1] / mpmath.sqrt(P[0, 0] * P[1, 1])


def tau(alpha, N, d):
    return math.tanh(NormalDist().inv_cdf(1 - alpha / 2) / math.sqrt(N - d - 3))


def plain_pc(R, N, alpha=0.05, depth=1000):
    """Sequential PC-stable, group size 1 -> (edges, sepset, tests per level): level d works on a snapshot of the
    adjacencies; edge (x < y) tries the size-d subsets of adj(x) - {y} in lexicographic order, then those of
    adj(y) - {x}; the first independent one removes it; removals apply after the level; level 1 always runs and
    the search goes on while the largest degree - 1 exceeds d."""
    n = R.shape[0]
    adj = [set(range(n)) - {i} for i in range(n)]
    sepset, tests = {}, []
    for d in range(0, max(depth, 1)):
        snap = [sorted(a) for a in adj]
        t, count = tau(alpha, N, d), 0
        for x, y in [(i, j) for i in range(n) for j in snap[i] if i < j]:
            for a, b in ((x, y), (y, x)):
                found = None
                for Z in itertools.combinations([v for v in snap[a] if v != b], d):
                    count += 1
                    if abs(pcorr_np(R, [x, y, *Z])) <= t:
                        found = Z
                        break
                if found is not None or d == 0:
                    break
            if found is not None:
                adj[x].discard(y), adj[y].discard(x)
                sepset[(x, y)] = tuple(sorted(found))
        tests.append(count)
        if d >= 1 and not max(len(a) for a in adj) - 1 > d:
            break
    edges = [(i, j) for i in range(n) for j in sorted(adj[i]) if i < j]
    return edges, sepset, tests
