"""Networks of the junction-forest tests (test_jt_forest_host.py, test_gpu_jt_forest.py) and of the
kernels fastbn_amd/prebuild.py compiles for them.  Plain Python and numpy: no GPU, no library of the
project.

disconnected: two polytrees and an isolated node (test_lbp_host.disconnected_network restated, so
that the prebuild can read it without pytest; test_jt_forest_host.py asserts the two are equal).

star_net: many components X -> Y, X -> Z whose evidence likelihoods multiply to less than the
smallest double, with the closed-form posterior of each component.

RANDOM: the arguments of synth.random_network for a disconnected network with real cliques.
"""
from types import SimpleNamespace

import numpy as np


def disconnected():
    """(dims, parents, counts): nodes 0-4 and 5-9 are polytrees, node 10 is isolated."""
    dims = np.array([2, 3, 2, 3, 2, 3, 2, 2, 3, 2, 3], np.int32)
    parents = [[], [], [1, 0], [2], [2], [], [5], [], [7, 6], [8], []]
    rng = np.random.default_rng(21)
    counts = [rng.integers(0, 40, (int(dims[v]), int(np.prod(dims[ps], dtype=np.int64)))) for v, ps in enumerate(parents)]
    return dims, parents, counts


# n = 120, seed = 13 (chosen on the CPU among seeds 1..29): 89 components, 17 of them with more than
# one node (the largest has 6), node 0 in a component of 4, a clique of 125 entries, and every
# component alone eligible for the tiled kernel; the forest is eligible for variants 3, 4 and 5
RANDOM = dict(n_nodes=120, seed=13, k_min=0)

STAR_COMPONENTS = 60
STAR_X = [[40], [60]]
STAR_Y = [[9998, 9990], [1, 9]]
STAR_Z = [[9997, 9985], [2, 14]]


def star_net(ncomp=STAR_COMPONENTS):
    """ncomp components X -> Y, X -> Z (nodes 3c, 3c + 1, 3c + 2), all binary, the same counts in
    each.  Observing Y = Z = 1 has likelihood 9.21e-7 per component: 60 of them multiply to about
    7e-363, below the smallest double."""
    dims = [2] * (3 * ncomp)
    parents, counts = [], []
    for c in range(ncomp):
        parents += [[], [3 * c], [3 * c]]
        counts += [np.array(STAR_X, np.int64), np.array(STAR_Y, np.int64), np.array(STAR_Z, np.int64)]
    return SimpleNamespace(ncomp=ncomp, dims=dims, parents=parents, counts=counts)


def star_cases(net, ncases=2):
    """Case 0: Y = Z = 1 in every component.  Case 1: the same with Y of component 0 at 0.  Further
    cases repeat the two."""
    ev = np.full((ncases, 3 * net.ncomp), -1, np.int8)
    ev[:, 1::3] = 1
    ev[:, 2::3] = 1
    ev[1::2, 1] = 0
    return ev


def star_exact(net, ev_row):
    """Marginals [6 ncomp] of one case in closed form: P(x | e) = P(x) P(y | x) P(z | x) / sum over x
    with an unobserved child summed out (its factor is 1); zeros for observed variables."""
    def cpt(counts):
        a = np.asarray(counts, np.float64)
        return (a + 1.0) / (a.sum(axis=0, keepdims=True) + a.shape[0])
    px, py, pz = cpt(STAR_X)[:, 0], cpt(STAR_Y), cpt(STAR_Z)  # py[y][x]
    out = []
    for c in range(net.ncomp):
        x, y, z = (int(v) for v in ev_row[3 * c:3 * c + 3])
        w = px.copy()  # weight of X = 0, 1 given the observed children
        if x >= 0:
            w = np.where(np.arange(2) == x, w, 0.0)
        if y >= 0:
            w = w * py[y]
        if z >= 0:
            w = w * pz[z]
        post_x = w / w.sum()
        # an unobserved child: its CPT against the weights of X (which then hold no factor of it)
        post_y = (py * w[None, :]).sum(axis=1)
        post_z = (pz * w[None, :]).sum(axis=1)
        out += ([0.0, 0.0] if x >= 0 else post_x.tolist())
        out += ([0.0, 0.0] if y >= 0 else (post_y / post_y.sum()).tolist())
        out += ([0.0, 0.0] if z >= 0 else (post_z / post_z.sum()).tolist())
    return np.array(out)


def sub_network_args(node_counts, dims, nodes):
    """The arguments of Network.from_counts for the sub-network on `nodes` (sorted; closed under
    parents), renumbered in increasing node order.  node_counts(v) -> (parents ascending, counts)."""
    idx = {int(v): i for i, v in enumerate(nodes)}
    parents, counts = [], []
    for v in nodes:
        ps, cnt = node_counts(int(v))
        parents.append([idx[int(q)] for q in ps])
        counts.append(np.asarray(cnt, np.int64))
    return np.asarray(dims, np.int32)[list(nodes)], parents, counts
