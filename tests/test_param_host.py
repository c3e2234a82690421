"""Host side of parameter learning (no GPU): family sizing / validation (fbn_param_family_sizes) and
the PDAG -> DAG extension (fbn_pdag_to_dag)."""
import os

import numpy as np
import pytest
from conftest import ALARM

import fastbn_amd as F
from fastbn_amd import synth

ARG, LIMIT = -1, -6  # fbn_err_t (include/fastbn.h)


def _code(fn, *a):
    with pytest.raises(F.FastBNError) as e:
        fn(*a)
    return e.value.code


# ---------------------------------------------------------------- family sizes
def test_family_sizes_ragged():
    dims = [5, 3, 7, 2]
    parents = [[], [0], [1, 0], [2, 0, 1]]  # cells 5, 3*5, 7*15, 2*105
    off, total = F.family_sizes(dims, parents)
    assert off.tolist() == [0, 5, 20, 125, 335] and total == 335
    # the order a node lists its parents in does not change the sizes
    off2, total2 = F.family_sizes(dims, [[], [0], [0, 1], [0, 1, 2]])
    assert off2.tolist() == off.tolist() and total2 == total
    # no edges at all: the state counts
    off3, total3 = F.family_sizes(dims, [[], [], [], []])
    assert off3.tolist() == [0, 5, 8, 15, 17] and total3 == 17


def test_family_sizes_rejects_bad_parent_lists():
    dims = [5, 3, 7, 2]
    assert _code(F.family_sizes, dims, [[], [4], [], []]) == ARG    # out of range
    assert _code(F.family_sizes, dims, [[], [-1], [], []]) == ARG   # out of range (negative)
    assert _code(F.family_sizes, dims, [[], [1], [], []]) == ARG    # self parent
    assert _code(F.family_sizes, dims, [[], [], [0, 1, 0], []]) == ARG  # repeated parent
    assert _code(F.family_sizes, [5, 0, 7, 2], [[], [], [], []]) == ARG  # a node without states


def test_family_sizes_limit_not_wrapped():
    # 40 parents of 4 states: 2 * 4^40 = 2^81 cells -- wraps to 0 in 64 bits if merely multiplied
    dims = [4] * 40 + [2]
    parents = [[] for _ in range(40)] + [list(range(40))]
    assert _code(F.family_sizes, dims, parents) == LIMIT
    # each family under the cap (2^25 cells), their sum over it (3 x 2^25 > 2^26)
    dims = [2] * 24 + [2, 2, 2]
    parents = [[] for _ in range(24)] + [list(range(24))] * 3
    assert _code(F.family_sizes, dims, parents) == LIMIT
    # one such family alone is under the cap and sized exactly
    dims = [2] * 24 + [2]
    parents = [[] for _ in range(24)] + [list(range(24))]
    off, total = F.family_sizes(dims, parents)
    assert total == 48 + 2 ** 25 and off[24] == 48


# ---------------------------------------------------------------- PDAG -> DAG
def _skeleton(parents):
    return sorted({(min(v, q), max(v, q)) for v, ps in enumerate(parents) for q in ps})


def _acyclic(parents):
    n = len(parents)
    indeg = [len(ps) for ps in parents]
    ch = [[] for _ in range(n)]
    for v, ps in enumerate(parents):
        for q in ps:
            ch[q].append(v)
    order = [v for v in range(n) if not indeg[v]]
    for x in order:
        for c in ch[x]:
            indeg[c] -= 1
            if not indeg[c]:
                order.append(c)
    return len(order) == n


def _colliders(parents):
    """Unshielded colliders (a, v, b), a < b both parents of v and not adjacent."""
    adj = set(_skeleton(parents))
    return {(a, v, b) for v, ps in enumerate(parents) for a in ps for b in ps
            if a < b and (a, b) not in adj}


def test_pdag_directed_dag_returns_itself():
    _, dims, parents, _ = synth.read_xmlbif(os.path.join(ALARM, "alarm.xml"))
    arcs = [(q, v, 1) for v, ps in enumerate(parents) for q in ps]
    assert len(arcs) == 46
    dag = F.pdag_to_dag(len(dims), arcs)
    assert dag == [sorted(ps) for ps in parents]


def test_pdag_undirected_chain_gains_no_collider():
    dag = F.pdag_to_dag(3, [(0, 1, 0), (1, 2, 0)])
    assert _skeleton(dag) == [(0, 1), (1, 2)]
    assert _acyclic(dag) and not _colliders(dag)
    assert dag == [[1], [2], []]  # node 0 goes first (lowest index), then 1: the chain 2 -> 1 -> 0


def test_pdag_v_structure_with_undirected_tail_is_kept():
    # 0 -> 2 <- 1 and 2 - 3 - 4: the tail must point away from the collider (no new one at 2 or 3)
    tri = [(0, 2, 1), (1, 2, 1), (2, 3, 0), (3, 4, 0)]
    dag = F.pdag_to_dag(5, tri)
    assert dag == [[], [], [0, 1], [2], [3]]
    assert _colliders(dag) == {(0, 2, 1)}


def test_pdag_without_extension_is_an_error():
    # a chordless undirected 4-cycle: any acyclic orientation has a new unshielded collider
    with pytest.raises(F.FastBNError) as e:
        F.pdag_to_dag(4, [(0, 1, 0), (1, 2, 0), (2, 3, 0), (0, 3, 0)])
    assert e.value.code == ARG and "0 1 2 3" in str(e.value)
    # a directed 3-cycle
    assert _code(F.pdag_to_dag, 3, [(0, 1, 1), (1, 2, 1), (2, 0, 1)]) == ARG


def test_pdag_rejects_duplicate_and_contradictory_edges():
    assert _code(F.pdag_to_dag, 3, [(0, 1, 1), (0, 1, 1)]) == ARG
    assert _code(F.pdag_to_dag, 3, [(0, 1, 1), (1, 0, 1)]) == ARG
    assert _code(F.pdag_to_dag, 3, [(0, 1, 1), (0, 1, 0)]) == ARG
    assert _code(F.pdag_to_dag, 3, [(0, 3, 1)]) == ARG
    assert _code(F.pdag_to_dag, 3, [(1, 1, 0)]) == ARG


def test_pdag_is_deterministic():
    tri = [(0, 2, 1), (1, 2, 1), (2, 3, 0), (3, 4, 0), (5, 6, 0), (6, 7, 0), (5, 7, 0)]
    assert F.pdag_to_dag(8, tri) == F.pdag_to_dag(8, tri)
    assert F.pdag_to_dag(8, tri) == F.pdag_to_dag(8, tri[::-1])  # nor does the edge order matter


def test_pdag_alarm5000_cpdag_extension():
    """The CPDAG of the CPU oracle's PC-stable run on ALARM-5000 (as tests/test_shard.py builds it):
    44 edges, 41 arcs and 3 undirected."""
    import oracle as O
    import orient
    ref = O.OracleDataset(csv=os.path.join(ALARM, "alarm_s5000.txt")).pc_stable(0.05, 1000, 1)
    cpdag = orient.orient(37, [tuple(e) for e in ref["edges"]], {k: tuple(v) for k, v in ref["sepset"].items()})
    arcs = [(a, b) for a, b, t in cpdag if t == 1]
    und = [(a, b) for a, b, t in cpdag if t == 0]
    assert (len(cpdag), len(arcs), len(und)) == (44, 41, 3)
    dag = F.pdag_to_dag(37, cpdag)
    assert _skeleton(dag) == sorted((min(a, b), max(a, b)) for a, b, _ in cpdag)  # same skeleton
    assert all(a in dag[b] for a, b in arcs)  # every arc kept
    assert _acyclic(dag)
    # no unshielded collider the CPDAG's arcs do not already hold
    arc_par = [[] for _ in range(37)]
    for a, b in arcs:
        arc_par[b].append(a)
    adj = set(_skeleton(dag))
    before = {(a, v, b) for v, ps in enumerate(arc_par) for a in ps for b in ps if a < b and (a, b) not in adj}
    assert _colliders(dag) == before
    assert max(len(ps) for ps in dag) <= 4
    assert all(ps == sorted(ps) for ps in dag)
