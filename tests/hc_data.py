"""Data and independent references of the hill-climbing tests (test_hc_host.py, test_gpu_hc.py,
test_gpu_hc_cli.py): seeded column stores that reach every shape the score reduction distinguishes, a
numpy float64 evaluation of the family score, small generating networks, and graph helpers."""
import functools
import hashlib
import os

import numpy as np

import fastbn_amd as F

ARG, LIMIT = -1, -6  # fbn_err_t (include/fastbn.h)
ALARM_CSV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alarm", "alarm_s5000.txt")

# ---- kernel edges.  State counts chosen so that single parents give q = 2, 63, 64, 65 and three
# 16-state parents q = 4096; children with r = 1, 2, 256; variable 10 has a state (4) that never occurs,
# so its families hold all-zero rows (as a child) and all-zero configurations (as a parent).
#            0  1    2   3   4   5   6   7   8  9 10 11 12
EDGE_DIMS = np.array([2, 1, 256, 63, 64, 65, 16, 16, 16, 3, 6, 2, 5], np.int32)
EDGE_NS = [1, 15, 1003, 5000]
EDGE_FAMILIES = [
    (0,), (1,), (2,),                     # q = 1; r = 2, 1, 256
    (12, 0), (2, 0), (1, 11),             # q = 2; r = 5, 256, 1
    (0, 3), (0, 4), (0, 5),               # q = 63, 64, 65
    (1, 5), (2, 4), (2, 5),               # r = 1 x 65; r = 256 x 64 = 16,384 and x 65 = 16,640 cells (global path)
    (0, 6, 7, 8), (11, 8, 6, 7),          # q = 4096 (8,192 cells: the largest LDS table), parents unsorted
    (9, 6, 7, 8),                         # 3 x 16^3 = 12,288 cells: the global counting path by default
    (10,), (0, 10), (10, 12), (12, 10, 0), (10, 1),  # rows / configurations that never occur; a 1-state parent
    (3, 0, 11, 12), (5, 9, 10),
]


@functools.lru_cache(maxsize=None)
def edge_columns(N):
    rng = np.random.default_rng(4200 + N)
    cols = np.stack([rng.integers(0, d, N) for d in EDGE_DIMS]).astype(np.uint8)
    cols[10] = np.array([0, 1, 2, 3, 5], np.uint8)[rng.integers(0, 5, N)]  # value 4 never occurs
    # dependent columns, so the tables are far from uniform and the log-likelihoods far from 0
    cols[0] = np.where(rng.random(N) < 0.6, cols[6] % 2, cols[0])
    cols[9] = np.where(rng.random(N) < 0.5, (cols[6] + cols[7] + cols[8]) % 3, cols[9])
    cols[12] = np.where(rng.random(N) < 0.5, cols[10] % 5, cols[12])
    cols[2] = np.where(rng.random(N) < 0.5, cols[4] * np.uint8(4), cols[2])  # 64 states x 4 < 256
    cols.setflags(write=False)
    return cols


def edge_dataset(N):
    return F.Dataset(columns=edge_columns(N), dims=EDGE_DIMS)


def np_family(cols, dims, fam, penalty):
    """(loglik, score, magnitude) of one family by numpy alone: np.bincount and n * np.log(n) in float64;
    magnitude = sum_jk L[N_jk] + sum_j L[N_j], what the two cancelling sums are measured against."""
    child, ps = fam[0], sorted(fam[1:])
    key = np.zeros(cols.shape[1], np.int64)
    q = 1
    for p in ps:
        key = key * int(dims[p]) + cols[p]
        q *= int(dims[p])
    r = int(dims[child])
    t = np.bincount(cols[child].astype(np.int64) * q + key, minlength=r * q).reshape(r, q).astype(np.float64)

    def ell(a):
        return np.where(a > 0, a * np.log(np.maximum(a, 1.0)), 0.0)

    a, b = float(ell(t).sum()), float(ell(t.sum(0)).sum())
    return a - b, a - b - penalty * (r - 1) * q, a + b


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- graphs
def is_acyclic(parents):
    n = len(parents)
    indeg = [len(ps) for ps in parents]
    ch = [[] for _ in range(n)]
    for v, ps in enumerate(parents):
        for q in ps:
            ch[q].append(v)
    order = [v for v in range(n) if not indeg[v]]
    for v in order:
        for w in ch[v]:
            indeg[w] -= 1
            if not indeg[w]:
                order.append(w)
    return len(order) == n


def skeleton(parents):
    return {(min(v, q), max(v, q)) for v, ps in enumerate(parents) for q in ps}


def trace_digest(trace):
    """sha256 of the (type, from, to) int32 triples of an operation trace."""
    return hashlib.sha256(np.asarray([t[:3] for t in trace], np.int32).reshape(-1, 3).tobytes()).hexdigest()


def first_divergence(a, b):
    """A parity failure names its first diverging step."""
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"step {k}: {x} != {y}"
    return None if len(a) == len(b) else f"lengths {len(a)} != {len(b)}"


def neighbours(parents, allowed=None, max_parents=None):
    """Every legal single operation on a DAG: (type, x, y, new parent lists)."""
    n = len(parents)
    out = []

    def ok(ps):
        return is_acyclic(ps) and (max_parents is None or all(len(p) <= max_parents for p in ps))

    for y in range(n):
        for x in range(n):
            if x == y:
                continue
            if x in parents[y]:
                dele = [sorted(set(p) - {x}) if v == y else list(p) for v, p in enumerate(parents)]
                out.append((1, x, y, dele))
                if allowed is None or allowed[y][x]:
                    rev = [sorted(set(p) | {y}) if v == x else list(p) for v, p in enumerate(dele)]
                    if ok(rev):
                        out.append((2, x, y, rev))
            elif allowed is None or allowed[x][y]:
                add = [sorted(set(p) | {x}) if v == y else list(p) for v, p in enumerate(parents)]
                if ok(add):
                    out.append((0, x, y, add))
    return out


def families_of(parents):
    return [(v, *ps) for v, ps in enumerate(parents)]


# ---- brute-force-sized generating networks: 5-node synth.random_network draws (node i takes 1 or 2 parents
# among the earlier nodes, 2 or 3 states, Dirichlet(1) CPT columns), 4,000 forward samples each.  Of the
# seeds 1..39 the host twin recovers the generating skeleton under both BIC and AIC for 22; these two have
# the most arcs among them (7: three v-structures) and a node with two children and a two-parent child.
SMALL_SEEDS = (24, 34)
SMALL_N = 4000


@functools.lru_cache(maxsize=None)
def small_network(seed):
    """(Dataset, generating parent lists) of one of SMALL_SEEDS."""
    import tempfile

    from fastbn_amd import synth
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "hc5.xml")
        _, parents, _ = synth.random_network(n_nodes=5, seed=seed, window=4, parent_probs=(0.5, 0.5), dom=(2, 3), path=path)
        net = synth.read_xmlbif(path)
    cols = synth.forward_sample(net, SMALL_N, seed)
    cols.setflags(write=False)
    return F.Dataset(columns=cols, dims=np.array(net[1], np.int32)), [list(p) for p in parents]


# ---- the tie dataset: columns 0 and 1 are identical, 2 is a noisy copy
@functools.lru_cache(maxsize=None)
def tie_columns():
    rng = np.random.default_rng(5)
    N = 600
    a = rng.integers(0, 3, N)
    c = np.where(rng.random(N) < 0.7, a, rng.integers(0, 3, N))
    cols = np.stack([a, a, c]).astype(np.uint8)
    cols.setflags(write=False)
    return cols


def synth12_dataset(N=1003, seed=8):
    """N forward samples of a seeded 12-variable synth.random_network."""
    import tempfile

    from fastbn_amd import synth
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "hc12.xml")
        synth.random_network(path=path, name="hc12", n_nodes=12, seed=seed, window=5, parent_probs=(0.5, 0.3, 0.2), dom=(2, 4))
        net = synth.read_xmlbif(path)
        return F.Dataset(columns=synth.forward_sample(net, N, seed), dims=np.array(net[1], np.int32))
