"""Helpers shared by test_psample_host.py and test_gpu_psample.py (PosteriorSampler, fbn_psample).

The bound on a count.  The S draws of a case are independent by construction (disjoint stream positions),
so the number n of draws that fall into a cell of posterior probability p is Binomial(S, p).  The tests
hold |n - S p| <= 6 sqrt(S p (1 - p)) + 1: a correct sampler misses 6 sigma with probability < 2e-9 per
cell (the + 1 covers the cells whose S p is far below 1, where the normal tail is no guide and a single hit
must pass).  The seeds are fixed: a miss is a finding.

test_gpu_psample.py takes its 130-case workloads from test_gpu_mpe.py (`_cases`, `tie_net`) so that both
engines see the same cases; the helpers would belong in mpe_nets.py, but existing test files stay as they are."""
import numpy as np
from em_nets import SMALL_NETS, Tables, family_counts, small_net, tiny_net  # noqa: F401
from mpe_nets import mixed_cases

DIST_NETS = ("tiny", "nine", "star", "shapes", "disconnected")
S_DIST = 65536


def net_cases(key):
    """(network, 9 evidence rows: none observed, two complete rows, three with 1 and three with 3 observed)"""
    if key == "tiny":
        return tiny_net()[0], mixed_cases(tiny_net()[0], 5)
    return small_net(key)


def assert_binomial(n, p, S, what):
    n, p = np.asarray(n, np.float64), np.asarray(p, np.float64)
    slack = 6.0 * np.sqrt(S * p * (1.0 - np.minimum(p, 1.0))) + 1.0
    bad = np.abs(n - S * p) > slack
    assert not bad.any(), (what, np.argwhere(bad)[:4].tolist(), n[bad][:4], (S * p)[bad][:4])


def family_cells(samples, tb):
    """the family-cell counts of samples [S][V] as one int64 [cells] array in fbn_param_counts' layout"""
    return np.concatenate([c.reshape(-1) for c in family_counts(samples.astype(np.int64), tb.dims, tb.parents)])
