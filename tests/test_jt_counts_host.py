"""The CPU restatement of the junction tree (oracle/) on the inputs of test_gpu_jt_range.py and
test_gpu_jt_counts.py, against exact rational arithmetic (tests/jt_nets.py), and the conditions
those GPU tests rely on, from the restatement's per-case Normalize statistics.

The restatement is the GPU tests' yardstick; here it is itself held to (count + 1) / (total + states)
in integers and Fractions, rounded once: on networks built from count maps (counts far above what
XMLBIF's (int)(p * 10000) gives, unseen parent configurations, a 1-state node, 32 / 33 / 127 states)
and on the conflict networks whose denominators leave the range the kernels' fast division is checked
against."""
import numpy as np
import pytest

import fastbn_amd as F
import jt_nets as J
import oracle as O

# The largest relative error of the restatement against the rational value measured over every input
# of this file (each figure is printed by its test): 2.3e-15 on the XMLBIF
# conflict network (up to 30 factors (H + 1) / (H + 2) per chain), 1.8e-15 on the 127-state counts
# network, below 1e-15 on the others.  The sums are short and all-positive; 4x covers another order
# of the same operations.
MEASURED_REL = 2.3e-15
BOUND = 4 * MEASURED_REL
FORMS = J.CONFLICT_FORMS


def _rel(got, ref):
    nz = ref != 0
    np.testing.assert_array_equal(got != 0, nz)  # zeros exactly where the exact value is zero
    return float(np.max(np.abs(got[nz] - ref[nz]) / ref[nz])) if nz.any() else 0.0


@pytest.fixture(scope="module", params=sorted(FORMS))
def conflict(request):
    net = J.conflict_net(*FORMS[request.param])
    return net, O.OracleJT.from_counts(net.dims, net.parents, net.counts), J.conflict_blocks(net)


@pytest.fixture(scope="module", params=sorted(J.COUNTS_VARIANTS))
def counts(request):
    net = J.counts_net(J.COUNTS_SEED, request.param)
    return net, O.OracleJT.from_counts(net.dims, net.parents, net.counts), J.ExactJoint(net.dims, net.parents, net.counts)


def test_counts_net_is_what_xmlbif_cannot_express(counts):
    net = counts[0]
    dims, V = net.dims, len(net.dims)
    assert V <= 10 and int(np.prod(dims, dtype=np.int64)) <= 200_000
    assert dims[J.ONE_STATE] == 1 and dims[0] > 1
    assert max(dims) == {"small": 4, "dom32": 32, "dom33": 33, "dom127": 127}[net.variant] == max(dims[J.WIDE], 4)
    assert any(list(p) == sorted(p, reverse=True) and len(p) > 1 for p in net.parents)
    allc = np.concatenate([c.reshape(-1) for c in net.counts])
    assert (allc == 0).any() and ((allc >= 1) & (allc <= 40)).any()
    assert ((allc > 900_000) & (allc < 1_100_000)).any() and (allc > 10 ** 12 - 1).any()
    assert sum(int((c.sum(axis=0) == 0).sum()) for c in net.counts) >= 2  # unseen parent configurations
    if net.variant == "dom32":  # the wide variable sits in a clique of exactly 256 entries
        assert dims[5] * dims[6] * dims[7] == 256 and net.parents[7] == [5, 6]
    # what the product's planner makes of it (a host-only plan)
    jt = F.JunctionTree(F.Network.from_counts(net.dims, net.parents, net.counts), device=-1)
    assert jt.info["specialized_eligible"] == (1 if max(dims) <= 32 else 0)
    assert jt.info["sum_dom"] == sum(dims)


def test_restatement_vs_exact_enumeration_counts_nets(counts):
    """16 cases each at 0, 2 and half of the variables observed: marginals within BOUND of the exact
    enumeration; labels equal wherever the exact top two of the query differ by more than 1e-9."""
    net, oj, joint = counts
    worst = 0.0
    for k in (0, 2, len(net.dims) // 2):
        ev = J.counts_cases(net, 16, k, seed=k + 1)
        if net.variant == "dom127" and k:
            assert (ev[:, J.WIDE] == 126).any()
        lab, marg = oj.infer(ev)
        left_out, cache = 0, {}
        for i in range(16):
            key = ev[i].tobytes()
            if key not in cache:
                cache[key] = joint.marginals(ev[i]) + (joint.top2,)
            elab, emarg, gap = cache[key]
            worst = max(worst, _rel(marg[i], emarg))
            if gap > 1e-9:
                assert lab[i] == elab, (k, i)
            else:
                left_out += 1
        assert left_out <= 2, (k, left_out)
    print("counts_net %s: restatement vs exact, largest relative error %.3g" % (net.variant, worst))
    assert worst <= BOUND


def test_restatement_vs_exact_posteriors_conflict_nets(conflict):
    """X0 and A of every benign, tripping and deep case against the four-term rational posterior."""
    net, oj, blocks = conflict
    worst = 0.0
    for name in ("benign", "tripping", "deep"):
        cases = getattr(blocks, name)
        lab, marg = oj.infer(J.conflict_cases(net, cases))
        assert np.isfinite(marg).all()
        left_out = 0
        for i, case in enumerate(cases):
            px, pa = J.conflict_exact(net, *case)
            worst = max(worst, _rel(marg[i, :4], np.array([float(x) for x in px + pa])))
            if len(case) > 2:
                assert lab[i] == 0  # the query is observed
            elif abs(px[0] - px[1]) > 1e-9 * max(px):
                assert lab[i] == (0 if px[0] >= px[1] else 1), case
            else:
                left_out += 1
        assert left_out <= 2, (name, left_out)
    print("conflict_net K=%d: restatement vs exact, largest relative error %.3g" % (net.K, worst))
    assert worst <= BOUND


def test_conflict_blocks_meet_the_gpu_tests_conditions(conflict):
    """What test_gpu_jt_range.py relies on.  The largest denominator of every case is 4, not 1: the
    initial potential of an unobserved clique {A, Bi, Bi+1} sums to its four parent configurations."""
    net, oj, blocks = conflict
    st = {name: oj.infer_stats(J.conflict_cases(net, getattr(blocks, name)))[2]
          for name in ("benign", "tripping", "deep")}
    for name, s in st.items():
        print("conflict_net K=%d %-8s smallest denominator 2^[%.1f, %.1f], largest 2^%.1f, smallest entry 2^%.1f"
              % (net.K, name, np.log2(s[:, 0].min()), np.log2(s[:, 0].max()), np.log2(s[:, 1].max()),
                 np.log2(s[:, 2].min())))
        assert len(s) == 64
        assert (s[:, 2] >= 2.0 ** -960).all()  # the documented limit of the kernels' division
        assert (s[:, 1] <= 4).all()
    assert (st["benign"][:, 0] >= 2.0 ** -100).all()
    assert (st["tripping"][:, 0] < 2.0 ** -600).all() and (st["tripping"][:, 0] > 2.0 ** -900).all()
    assert (st["deep"][:, 0] < 2.0 ** -900).all() and (st["deep"][:, 0] > 2.0 ** -1000).all()
    # the benign block reaches marginal entries below 2^-800 with every denominator in range (the
    # entry limit stops one-sided prefixes two variables early: jt_nets.conflict_entry_bits)
    lab, marg = oj.infer(J.conflict_cases(net, blocks.benign))
    assert 2.0 ** -940 < marg[marg > 0].min() < 2.0 ** -800


def test_statistics_entry_point_leaves_results_alone(conflict):
    net, oj, blocks = conflict
    ev = J.conflict_cases(net, blocks.tripping[:8] + blocks.benign[:8])
    lab, marg = oj.infer(ev)
    slab, smarg, st = oj.infer_stats(ev)
    np.testing.assert_array_equal(slab, lab)
    np.testing.assert_array_equal(smarg, marg)
    assert st.shape == (16, 3) and (st[:, 0] <= st[:, 1]).all() and (st[:, 2] > 0).all()


def test_restatement_from_counts_equals_xmlbif(tmp_path, alarm_paths):
    """or_jt_create builds what or_jt_load builds: the XMLBIF conflict network given as its document
    and as its count map, and ALARM given as the count map the product's loader read."""
    net = J.conflict_net(*FORMS["xmlbif"])
    path = tmp_path / "conflict.xml"
    path.write_text(net.xml)
    ev = J.conflict_cases(net, J.conflict_blocks(net).tripping)
    a, b = O.OracleJT(str(path)), O.OracleJT.from_counts(net.dims, net.parents, net.counts)
    for x, y in zip(a.infer(ev), b.infer(ev)):
        np.testing.assert_array_equal(x, y)
    # the product reads the document the same way
    pn = F.Network(str(path))
    for v in range(pn.num_nodes):
        par, cnt = pn.node_counts(v)
        assert list(par) == sorted(net.parents[v])
        np.testing.assert_array_equal(cnt, net.counts[v])

    pn = F.Network(alarm_paths["xml"])
    fam = [pn.node_counts(v) for v in range(pn.num_nodes)]
    ev = pn.evidence_cases(64, 7, 3)
    a = O.OracleJT(alarm_paths["xml"])
    b = O.OracleJT.from_counts(pn.dims, [list(p) for p, _ in fam], [c for _, c in fam])
    for x, y in zip(a.infer(ev), b.infer(ev)):
        np.testing.assert_array_equal(x, y)
