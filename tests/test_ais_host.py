"""The adaptive samplers' host twin (AISBN / SelfImportanceSampling with device=-1: ais_host.cpp).

Yardsticks: a plain-Python restatement of the whole algorithm as include/fastbn.h states it (below; bit
for bit), LikelihoodWeighting's tested samples (no update: the same values), brute-force enumeration
of the joint for log P(e), the estimator's own standard error for unbiasedness, and the exact ALARM
fixture alarm_1k_pt against likelihood weighting at equal S.  The restatement, the networks and the
checks are shared with test_gpu_ais.py."""
import functools
import math
import os

import numpy as np
import pytest
from conftest import ALARM, read_pt_file
from test_epis_host import alarm, alarm_cases, bits, brute, forest, loopy_network, polytree_network
from test_lbp_host import net_tuple, polytree_cases

import fastbn_amd as F
from fastbn_amd import synth

ARG, LIMIT = -1, -6  # fbn_err_t (include/fastbn.h)
CLASSES = {0: F.AISBN, 1: F.SelfImportanceSampling}
LN2 = 0.6931471805599453
DBL_MAX = 1.7976931348623157e308


# ---- the restatement
def cutoff(eps, d):
    return eps if eps >= 0.0 else (0.006 if d < 5 else (0.001 if d <= 8 else 0.0005))


def ais_draw(P, I, eps, u):
    """fastbn.h's draw of a learnable variable -> (value, factor)."""
    d = len(P)
    z = 0.0
    for q in range(d):
        z = z + I[q]
    lw = not (0.0 < z <= DBL_MAX)
    g = P if lw else I
    if not lw and eps > 0.0:
        g = [max(x, eps * z) for x in g]
    c, run = [], 0.0
    for q in range(d):
        run = run + g[q]
        c.append(run)
    x = u * c[-1]
    q = min(sum(1 for t in c if x >= t), d - 1)
    return q, ((P[q] * c[-1]) / g[q] if g[q] > 0.0 else 0.0)


def butterfly(a):
    a = np.array(a, np.float64)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[idx ^ off]
    return float(a[0])


def stages(method, S, m, l):
    nupd = m if method == 0 else min(m, (S - 1) // l)
    last = S if method == 0 else S - nupd * l
    return nupd, last, nupd * l + last


def restate(tup, ev, method, S, m, l, eps, seed, eta, case_offset=0):
    """-> dict(val [V][C * T], m, e [C * T], icpt [C][cells], marg [C][SD], lab, ess, le, upd, ess0, grew):
    every quantity in the order fastbn.h states; grew = some chunk raised emax (counts rescaled)."""
    _, dims, parents, cpts = tup
    dims = [int(d) for d in dims]
    V, order = len(dims), synth._topo(parents)
    eps = -1.0 if eps is None else eps
    toff, prob = {}, []
    for v in order:
        toff[v] = len(prob)
        prob += np.asarray(cpts[v], np.float64).reshape(dims[v], -1).T.ravel().tolist()  # [pc][q], GIVEN order
    cells = len(prob)
    moff = np.concatenate([[0], np.cumsum(dims)]).tolist()
    nupd, last, T = stages(method, S, m, l)
    C_ = len(ev)
    out = dict(val=np.zeros((V, C_ * T), np.uint8), m=np.zeros(C_ * T), e=np.zeros(C_ * T, np.int32),
               icpt=np.zeros((C_, cells)), marg=np.zeros((C_, moff[-1])), lab=np.zeros(C_, np.int32), ess=np.zeros(C_),
               le=np.zeros(C_), upd=np.zeros(C_, np.int32), ess0=np.zeros(C_), grew=False)
    for c, ec in enumerate(np.asarray(ev).tolist()):
        bg = np.random.PCG64(seed)
        bg.advance((case_offset + c) * T * V)
        U = np.random.Generator(bg).random((T + 64, V)).tolist()  # position i * V + k
        desc = [False] * V
        for v in reversed(order):
            if ec[v] >= 0 or desc[v]:
                for p in parents[v]:
                    desc[p] = True
        lrn = [desc[v] and ec[v] < 0 for v in range(V)]
        I, N = list(prob), [0.0] * cells
        row = [0.0] * moff[-1]
        emax, upd, sumw, sumw2, ess0, first, tbase = 0, 0, 0.0, 0.0, 0.0, True, 0
        for st in range(nupd + 1):
            n = l if st < nupd else last
            counted, learn = method == 1 or st == nupd, st < nupd
            if method == 0 or st == 0:
                first, sumw, sumw2 = True, 0.0, 0.0
                if learn:
                    N = [0.0] * cells
            for s0 in range(0, n, 64):
                act = min(64, n - s0)
                xs, ms, es, cell = [], [], [], []
                for ln in range(act):
                    t = tbase + s0 + ln
                    x, mant, ee, cl = [0] * V, 1.0, 0, {}
                    for k, v in enumerate(order):
                        pc = 0
                        for g in parents[v]:
                            pc = pc * dims[g] + x[g]
                        r = toff[v] + pc * dims[v]
                        P = prob[r:r + dims[v]]
                        if ec[v] >= 0:
                            x[v] = ec[v]
                            mant, de = math.frexp(mant * P[x[v]])
                            ee += de
                        elif lrn[v]:
                            x[v], fac = ais_draw(P, I[r:r + dims[v]], cutoff(eps, dims[v]), U[t][k])
                            mant, de = math.frexp(mant * fac)
                            ee += de
                        else:
                            x[v], _ = ais_draw(P, P, 0.0, U[t][k])  # the cdf row and SelectValue's rule
                        cl[v] = r + x[v]
                    xs.append(x), ms.append(mant), es.append(ee), cell.append(cl)
                    out["val"][:, c * T + t] = x
                    out["m"][c * T + t], out["e"][c * T + t] = mant, ee
                cm, f = max(es), 1.0
                if first:
                    emax = cm
                elif cm > emax:
                    f, emax = math.ldexp(1.0, emax - cm), cm
                    out["grew"] = True
                w = [math.ldexp(ms[ln], es[ln] - emax) for ln in range(act)] + [0.0] * (64 - act)
                if counted:
                    for v in range(V):
                        for q in range(dims[v]):
                            acc = 0.0 if first else row[moff[v] + q] * f
                            for ln in range(act):
                                acc += w[ln] if xs[ln][v] == q else 0.0
                            row[moff[v] + q] = acc
                if learn:
                    N = [a * f for a in N]
                    for v in range(V):
                        if lrn[v]:
                            for ln in range(act):
                                N[cell[ln][v]] += w[ln]
                sumw = sumw * f + butterfly(w)
                sumw2 = sumw2 * f * f + butterfly([a * a for a in w])
                first = False
            if st == 0:
                ess0 = sumw * sumw / sumw2 / n if sumw > 0.0 else 0.0
            if learn:
                upd += sumw > 0.0
                for v in order:
                    if lrn[v]:
                        end = min([toff[x] for x in order if toff[x] > toff[v]] + [cells])
                        for r in range(toff[v], end, dims[v]):
                            tot = 0.0
                            for q in range(dims[v]):
                                tot = tot + N[r + q]
                            if 0.0 < tot <= DBL_MAX:
                                for q in range(dims[v]):
                                    I[r + q] = I[r + q] + eta[st] * (N[r + q] / tot - I[r + q])
            tbase += n
        out["icpt"][c] = I
        lab = -1
        if sumw > 0.0:
            for v in range(V):
                for j in range(moff[v], moff[v + 1]):
                    row[j] = 0.0 if ec[v] >= 0 else row[j] / sumw
            lab, mp = 0, 0.0
            for q in range(dims[0]):
                if row[q] > mp:
                    mp, lab = row[q], q
        else:
            row = [0.0] * moff[-1]
        out["marg"][c], out["lab"][c] = row, lab
        out["ess"][c] = sumw * sumw / sumw2 if sumw > 0.0 else 0.0
        out["le"][c] = math.log(sumw / S) + emax * LN2 if sumw > 0.0 else -math.inf
        out["upd"][c], out["ess0"][c] = upd, ess0
    return out


def check_against_restatement(h, tup, ev, case_offset=0):
    method = h._method
    r = restate(tup, ev, method, h.num_samples, h.max_updates, h.interval, h.eps, h.seed, h.eta(), case_offset)
    val, m, e, icpt = h.debug_samples(ev, case_offset=case_offset)
    np.testing.assert_array_equal(val, r["val"])
    np.testing.assert_array_equal(bits(m), bits(r["m"]))
    np.testing.assert_array_equal(e, r["e"])
    np.testing.assert_array_equal(bits(icpt), bits(r["icpt"]))
    lab, marg = h.infer(ev, case_offset=case_offset)
    le, ess, upd, ess0 = h.stats
    np.testing.assert_array_equal(bits(marg), bits(r["marg"]))
    np.testing.assert_array_equal(lab, r["lab"])
    np.testing.assert_array_equal(bits(ess), bits(r["ess"]))
    np.testing.assert_array_equal(bits(ess0), bits(r["ess0"]))
    np.testing.assert_array_equal(upd, r["upd"])
    assert (np.abs(le - r["le"]) <= 1e-15 * np.abs(r["le"])).all()
    return r


# A 1-state node and domains above 8: 0 -> 1, {0, 1} -> 2, 2 -> 3, {2, 3} -> 4, 4 -> 5.
WIDE_DIMS = np.array([3, 1, 9, 2, 10, 2], np.int32)
WIDE_PARENTS = [[], [0], [0, 1], [2], [2, 3], [4]]


@functools.lru_cache(maxsize=None)
def wide_network():
    rng = np.random.default_rng(21)
    counts = [rng.integers(0, 40, (int(WIDE_DIMS[v]), int(np.prod(WIDE_DIMS[ps], dtype=np.int64))))
              for v, ps in enumerate(WIDE_PARENTS)]
    return WIDE_DIMS, WIDE_PARENTS, counts


@pytest.mark.parametrize("method", [0, 1])
def test_restatement_loopy(method):
    """l = 70, m = 3, S = 130: a partial chunk at every stage end (70 = 64 + 6, 130 = 128 + 2; SIS: one
    update after 70, then 60), and an emax that grows within a scope."""
    dims, parents, counts = loopy_network()
    net = F.Network.from_counts(dims, parents, counts)
    ev = polytree_cases(dims, 8, 2)
    h = CLASSES[method](net, 130, max_updates=3, interval=70, seed=5, device=-1)  # a seed at which emax grows
    r = check_against_restatement(h, net_tuple(dims, parents, counts), ev, case_offset=2)
    assert r["grew"]
    assert (r["upd"] == (3 if method == 0 else 1)).all()


@pytest.mark.parametrize("method,eps", [(0, 0.0), (0, None), (1, None), (1, 0.05)])
def test_restatement_wide(method, eps):
    dims, parents, counts = wide_network()
    assert dims.min() == 1 and dims.max() > 8
    net = F.Network.from_counts(dims, parents, counts)
    ev = np.full((5, 6), -1, np.int8)
    ev[0, 5] = 1
    ev[1, [3, 5]] = 0, 1
    ev[2, [1, 4]] = 0, 7   # the 1-state node observed
    ev[3, 2] = 8           # the query is the only learnable node
    h = CLASSES[method](net, 100, max_updates=2, interval=33, eps=eps, seed=4, device=-1)
    check_against_restatement(h, net_tuple(dims, parents, counts), ev)


# ---- reduces to likelihood weighting
@pytest.mark.parametrize("method,eps", [(0, 0.0), (1, 1e-300)])
def test_reduces_to_likelihood_weighting(method, eps):
    """m = 0: the ICPT is the CPTs, c is the cdf row, so the values are LW's (a cutoff of 1e-300 raises
    nothing: ALARM's smallest CPT entry is far above it); the weight takes c(d - 1) (within an ulp of
    1) per learnable variable, 37 at most: 1e-13 relative."""
    net, _ = alarm()
    ev = alarm_cases()[0][:16]
    h = CLASSES[method](net, 130, max_updates=0, interval=50, eps=eps, seed=3, device=-1)
    lw = F.LikelihoodWeighting(net, 130, seed=3, device=-1)
    val, m, e, icpt = h.debug_samples(ev, case_offset=5)
    lval, lm, le = lw.debug_samples(ev, case_offset=5)
    np.testing.assert_array_equal(val, lval)
    w, lww = np.ldexp(m, e), np.ldexp(lm, le)
    assert (lww > 0).all() and (np.abs(w - lww) <= 1e-13 * lww).all()
    h.infer(ev, case_offset=5)
    assert (h.stats[2] == 0).all()
    np.testing.assert_array_equal(bits(h.stats[3]), bits(h.stats[1] / 130))  # one stage: the first is the run


def sampler_prob(tup):
    """The CPTs in the ICPT's layout."""
    _, dims, parents, cpts = tup
    return np.concatenate([np.asarray(cpts[v], np.float64).reshape(int(dims[v]), -1).T.ravel() for v in synth._topo(parents)])


@pytest.mark.parametrize("method", [0, 1])
def test_nothing_observed_has_no_learnable_node(method):
    net, tup = alarm()
    ev = np.full((2, 37), -1, np.int8)
    h = CLASSES[method](net, 200, max_updates=2, interval=64, seed=1, device=-1)
    icpt = h.debug_samples(ev)[3]
    prob = sampler_prob(tup)
    np.testing.assert_array_equal(bits(icpt), bits(np.stack([prob, prob])))
    h.infer(ev)
    assert (h.stats[2] == 2).all() and (h.stats[1] == 200).all() and (h.stats[3] == 1.0).all()


# ---- the learnable set
@pytest.mark.parametrize("method", [0, 1])
def test_only_ancestors_of_evidence_learn(method):
    net, tup = alarm()
    _, dims, parents, _ = tup
    ev = alarm_cases()[0][:8]
    h = CLASSES[method](net, 300, max_updates=2, interval=100, seed=2, device=-1)
    icpt = h.debug_samples(ev)[3]
    prob = sampler_prob(tup)
    order = synth._topo(parents)
    sizes = [int(np.asarray(tup[3][v]).size) for v in order]
    start = dict(zip(order, np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()))
    for c, e in enumerate(ev):
        anc = set()
        for v in reversed(order):
            if e[v] >= 0 or v in anc:
                anc.update(parents[v])
        moved = 0
        for v, n in zip(order, sizes):
            a, b = icpt[c, start[v]:start[v] + n], prob[start[v]:start[v] + n]
            if e[v] >= 0 or v not in anc:
                np.testing.assert_array_equal(bits(a), bits(b))
            else:
                moved += not np.array_equal(a, b)
        assert moved >= 1 and np.isfinite(icpt[c]).all() and (icpt[c] >= 0).all()


# ---- unbiased
# Chosen here with the host twin (deterministic, and equal to the device): at these the estimate of
# every case lies inside its own 5 sigma, as it should for almost every seed.
UNBIASED_SEED, UNBIASED_S = 4, 2048


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("which", ["polytree", "loopy"])
def test_unbiased(which, method):
    dims, parents, counts = polytree_network() if which == "polytree" else loopy_network()
    net = F.Network.from_counts(dims, parents, counts)
    tup = net_tuple(dims, parents, counts)
    ev = polytree_cases(dims, 16, 1)
    S = UNBIASED_S
    h = CLASSES[method](net, S, max_updates=4, interval=256, seed=UNBIASED_SEED, device=-1)
    h.infer(ev)
    le, ess = h.stats[0], h.stats[1]
    for c, e in enumerate(ev):
        lpe = brute(tup, e)[1]
        err, bound = abs(math.exp(le[c] - lpe) - 1.0), 5 * math.sqrt(max(S / ess[c] - 1.0, 0.0) / S) + 1e-9
        print(which, method, "case", c, "relative error", err, "bound", bound, "ess/S", ess[c] / S)
        assert err <= bound


# ---- learning helps
def test_alarm_beats_likelihood_weighting():
    """First 64 fixture cases (7 observed variables), S = 1024, seed 0, l = 512, m = 8, default cutoff,
    measured with the host twin:
        average Hellinger distance   AIS-BN 0.021042   LW 0.072420   (gap 0.051378)
        median ess / S               AIS-BN 0.66041    LW 0.041448   (gap 0.61896)
    The margins are those gaps halved."""
    net, tup = alarm()
    ev, truth = alarm_cases()
    gold = read_pt_file(os.path.join(ALARM, "alarm_1k_pt"), tup[1], len(ev))[:64]
    S = 1024
    h = F.AISBN(net, S, max_updates=8, interval=512, seed=0, device=-1)
    lw = F.LikelihoodWeighting(net, S, seed=0, device=-1)
    hd = F.score_marginals(net, h.infer(ev[:64])[1], gold)[1] / 64
    lhd = F.score_marginals(net, lw.infer(ev[:64])[1], gold)[1] / 64
    med, lmed = np.median(h.stats[1]) / S, np.median(lw.stats[1]) / S
    print("average HD: AIS-BN", hd, "LW", lhd, "; median ess/S: AIS-BN", med, "LW", lmed)
    assert hd <= lhd - 0.025689
    assert med >= lmed + 0.30948


# ---- edges and arguments
@pytest.mark.parametrize("method", [0, 1])
def test_edges(method):
    dims, parents, counts, _ = forest()
    net = F.Network.from_counts(dims, parents, counts)
    tup = net_tuple(dims, parents, counts)
    ev = np.full((3, len(dims)), -1, np.int8)
    ev[1] = [d - 1 for d in dims]  # all observed
    ev[2, [3, 9]] = 1, 0
    for S, m, l in ((1, 1, 1), (70, 3, 1), (5, 2, 1), (64, 2, 64), (64, 2, 100)):
        h = CLASSES[method](net, S, max_updates=m, interval=l, seed=3, device=-1)
        r = check_against_restatement(h, tup, ev)
        lab, marg = h.infer(ev)
        le, ess, upd, ess0 = h.stats
        assert np.isfinite(marg).all() and (marg[1] == 0).all() and lab[1] == 0 and abs(ess[1] - S) <= 1e-12 * S
        assert abs(le[1] - brute(tup, ev[1])[1]) <= 1e-10  # every weight is P(e)
        want = m if method == 0 else min(m, (S - 1) // l)  # SIS with S <= l: no update
        assert (upd == want).all(), (S, m, l)
        if want == 0:
            np.testing.assert_array_equal(bits(r["icpt"]), bits(np.stack([sampler_prob(tup)] * 3)))


@functools.lru_cache(maxsize=None)
def underflow_network():
    """A binary root R, P(R = 1) = 1 / 100, with 1100 binary children, P(child = 1 | R) = 1 / 5, 1 / 2: with
    every child observed at 1 a sample with R = 0 weighs 2^-1454 of one with R = 1, which is 0 in fp64."""
    n = 1101
    return [2] * n, [[]] + [[0]] * (n - 1), [[[98], [0]]] + [[[3, 1], [0, 1]]] * (n - 1)


ZERO_SEED = 3  # chosen with the host twin: R = 1 first appears after the first stage, and again in the last, in both methods


@pytest.mark.parametrize("method", [0, 1])
def test_weights_that_underflow_to_zero(method):
    """Every CPT entry of a network is positive ((count + 1) / (total + states)) and so is every draw's
    factor, so a weight is 0 only by underflow against the scope's emax: a stage whose weights are all 0
    with nothing before it cannot be reached through a Network and is driven in
    tools/ais_host_check.cpp on a hand-built model with zero entries.  What can be reached: the first
    stage draws only R = 0 and learns from it; once R = 1 is drawn emax grows by 1454 bits, the rescaling
    factor of the counts and the sums underflows to 0, and every R = 0 sample of the scope weighs exactly
    0 from then on.  Nothing becomes NaN, the restatement holds, the posterior of R = 0 is exactly 0."""
    dims, parents, counts = underflow_network()
    net = F.Network.from_counts(dims, parents, counts)
    ev = np.full((2, len(dims)), 1, np.int8)
    ev[:, 0] = -1
    h = CLASSES[method](net, 100, max_updates=6, interval=8, seed=ZERO_SEED, device=-1)
    r = check_against_restatement(h, net_tuple(dims, parents, counts), ev)
    T = h.draws_per_case
    assert method == 0 or r["grew"]  # AIS-BN's stages are single chunks here: R = 1 sets the chunk's own emax
    assert np.isfinite(r["icpt"]).all() and np.isfinite(r["marg"]).all() and np.isfinite(r["le"]).all()
    for c in range(2):
        one = r["val"][0, c * T:(c + 1) * T] == 1
        assert one.any() and not one[:8].any() and one[-100:].any()
        assert r["marg"][c, 0] == 0.0 and abs(r["marg"][c, 1] - 1.0) <= 1e-13  # two summation orders of the same terms
        assert r["lab"][c] == 1 and r["upd"][c] == 6 and r["ess0"][c] == 1.0


def test_batch_split_and_repeat():
    net, _ = alarm()
    ev = alarm_cases()[0][:37]
    for method in (0, 1):
        h = CLASSES[method](net, 100, max_updates=2, interval=40, seed=9, device=-1)
        lab, marg = h.infer(ev)
        st = np.stack([np.asarray(s, np.float64) for s in h.stats])
        la, ma = h.infer(ev[:20])
        sa = np.stack([np.asarray(s, np.float64) for s in h.stats])
        lb, mb = h.infer(ev[20:], case_offset=20)
        sb = np.stack([np.asarray(s, np.float64) for s in h.stats])
        np.testing.assert_array_equal(lab, np.concatenate([la, lb]))
        np.testing.assert_array_equal(bits(marg), bits(np.concatenate([ma, mb])))
        np.testing.assert_array_equal(bits(st), bits(np.concatenate([sa, sb], axis=1)))
        np.testing.assert_array_equal(bits(h.infer(ev)[1]), bits(marg))
        assert not np.array_equal(h.infer(ev[20:])[1], mb)  # the offset moves the stream
        assert h.infer(ev[:3], marginals=False)[1] is None


def test_arguments():
    net, _ = alarm()
    ev = alarm_cases()[0][:4].copy()
    ref = F.AISBN(net, 64, 1, 32, device=-1).infer(ev)
    for cls, kw, msg in ((F.SelfImportanceSampling, dict(eps=0.0), "cutoff"), (F.AISBN, dict(max_updates=1025), "updates"),
                         (F.AISBN, dict(max_updates=-1), "updates"), (F.AISBN, dict(interval=0), "interval"),
                         (F.AISBN, dict(num_samples=0), "samples"), (F.AISBN, dict(eps=1.0), "eps"),
                         (F.AISBN, dict(eps=math.nan), "eps"),
                         (F.AISBN, dict(max_updates=1024, interval=1 << 50), "stream position")):
        with pytest.raises(F.FastBNError, match=msg) as e:
            cls(net, **{"num_samples": 64, "max_updates": 1, "interval": 32, "device": -1, **kw}).infer(ev)
        assert e.value.code == ARG, kw
    with pytest.raises(F.FastBNError) as e:
        F.AISBN(net, 64, eps=-0.5, device=-1)
    assert e.value.code == ARG
    h = F.AISBN(net, 64, 1, 32, device=-1)
    with pytest.raises(F.FastBNError, match="stream position") as e:
        h.infer(ev, case_offset=1 << 61)
    assert e.value.code == ARG
    with pytest.raises(F.FastBNError) as e:
        h.infer(ev, case_offset=-1)
    assert e.value.code == ARG
    bad = ev.copy()
    bad[2, 5] = net.dims[5]  # one past the last state
    with pytest.raises(F.FastBNError, match="case 2.*node 5") as e:
        h.infer(bad)
    assert e.value.code == ARG
    with pytest.raises(F.FastBNError) as e:  # the debug cap, 2^22 draws
        F.AISBN(net, (1 << 22) // 4 + 1, 0, 1, device=-1).debug_samples(ev)
    assert e.value.code == LIMIT
    with pytest.raises(F.FastBNError, match="host-only"):
        h.run_device(1, 4, 1)
    np.testing.assert_array_equal(bits(h.infer(ev)[1]), bits(ref[1]))  # the handle stays usable
    a = F.AISBN(net, 64, 8, 32, device=-1).eta()
    assert a[0] == 0.4 and (np.diff(a) < 0).all() and a[-1] > 0.14
    assert (F.SelfImportanceSampling(net, 64, 8, 32, device=-1).eta() == 1.0).all()
