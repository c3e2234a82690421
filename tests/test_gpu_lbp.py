"""Loopy belief propagation on the device (lbp.hip behind LoopyBeliefPropagation).

The device is held to the host twin bit for bit -- messages, marginals, labels and stats -- and the
host twin to the pure-Python restatement, the reference's tie-tree marginals and brute force in
test_lbp_host.py.  Shapes are the smallest at which the kernel can go wrong: one case, fewer cases
than groups, a group that loops over cases with a ragged tail (max_groups=2), message counts that
are no multiple of 64, a 1-state node, 127 states, six parents, a 4,096-cell family, 1041
variables, and both homes of the messages (LDS, global workspace)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ALARM, GOLD, REPO
from test_lbp_host import alarm, alarm_cases, bits, check_early_stop, check_tie_tree, shapes_cases, shapes_network

import fastbn_amd as F

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def host_results(key, iters, damping):
    """(messages, labels, marginals, used, residual) of the host twin, computed once per workload."""
    net, ev = WORKLOADS[key]()
    h = F.LoopyBeliefPropagation(net, iterations=iters, damping=damping, device=-1)
    lab, marg = h.infer(ev)
    return h.debug_messages(ev, iters), lab, marg, h.stats[0], h.stats[1]


def check_device(key, iters, damping, lds_bytes_max=0, max_groups=0, path=None):
    net, ev = WORKLOADS[key]()
    dev = F.LoopyBeliefPropagation(net, iterations=iters, damping=damping, device=0)
    dev.set_tuning(lds_bytes_max=lds_bytes_max, max_groups=max_groups)
    if path is not None:
        assert dev.info()["path"] == path
    msgs, lab, marg, used, res = host_results(key, iters, damping)
    np.testing.assert_array_equal(bits(dev.debug_messages(ev, iters)), bits(msgs))
    dlab, dmarg = dev.infer(ev)
    np.testing.assert_array_equal(dlab, lab)
    np.testing.assert_array_equal(bits(dmarg), bits(marg))
    np.testing.assert_array_equal(dev.stats[0], used)
    np.testing.assert_array_equal(bits(dev.stats[1]), bits(res))
    assert dev.last_kernel_ms() > 0.0
    dev.close()


def _synth(name):
    from conftest import SYNTH_NETS
    import gzip
    import tempfile
    with gzip.open(os.path.join(SYNTH_NETS, name + ".xml.gz"), "rb") as f, \
            tempfile.NamedTemporaryFile("wb", suffix=".xml") as g:
        g.write(f.read())
        g.flush()
        net = F.Network(g.name)
    return net, np.load(os.path.join(SYNTH_NETS, name + ".ev.npy"))[[0, 17, 33, 47]]


WORKLOADS = {"shapes": lambda: (shapes_network()[0], shapes_cases()),
             "bigdom": functools.lru_cache(maxsize=None)(lambda: _synth("bigdom")),
             "wide": functools.lru_cache(maxsize=None)(lambda: _synth("wide"))}
for _n in (1, 3, 64, 65):
    WORKLOADS["alarm%d" % _n] = (lambda n: lambda: (alarm()[0], alarm_cases()[:n]))(_n)


@pytest.mark.parametrize("lds_bytes_max,path", [(0, 0), (-1, 1)])
@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_alarm_equals_host_twin(n, lds_bytes_max, path):
    """max_groups=2: a group loops over up to 33 cases and the two groups' tails differ."""
    for iters in (1, 5):
        for damping in (0.0, 0.5):
            check_device("alarm%d" % n, iters, damping, lds_bytes_max, 2, path)


@pytest.mark.parametrize("lds_bytes_max,path", [(0, 0), (-1, 1)])
def test_shapes_equal_host_twin(lds_bytes_max, path):
    for iters in (1, 5):
        for damping in (0.0, 0.5):
            check_device("shapes", iters, damping, lds_bytes_max, 0, path)


@pytest.mark.parametrize("name", ["bigdom", "wide"])
def test_synth_nets_equal_host_twin(name):
    """bigdom: 21 states, 3,078 message doubles (74 KB: the global workspace by default); wide: a
    12-variable family of 4,096 cells."""
    net, ev = WORKLOADS[name]()
    assert (net.dims.max() == 21) if name == "bigdom" else (net.dims.max() == 2)
    for iters in (1, 5):
        for damping in (0.0, 0.5):
            check_device(name, iters, damping, path=1 if name == "bigdom" else 0)


def test_munin_like(munin_fixture):
    """1041 variables, 8,143 message doubles: 195 KB per case, beyond the LDS budget, so the default
    is the global workspace."""
    net = F.Network(munin_fixture["xml"])
    ev, _ = F.load_libsvm(munin_fixture["libsvm"], 1041)
    ev = ev[:4]
    assert ((ev >= 0).sum(1) == 208).all()
    dev = F.LoopyBeliefPropagation(net, iterations=3, device=0)
    host = F.LoopyBeliefPropagation(net, iterations=3, device=-1)
    info = dev.info()
    assert info["msg_doubles"] == 8143 and info["lds_bytes"] > 160 * 1024 and info["path"] == 1
    np.testing.assert_array_equal(bits(dev.debug_messages(ev, 3)), bits(host.debug_messages(ev, 3)))
    lab, marg = dev.infer(ev)
    hlab, hmarg = host.infer(ev)
    np.testing.assert_array_equal(lab, hlab)
    np.testing.assert_array_equal(bits(marg), bits(hmarg))
    np.testing.assert_array_equal(dev.stats[0], host.stats[0])
    np.testing.assert_array_equal(bits(dev.stats[1]), bits(host.stats[1]))
    assert np.isfinite(marg).all() and (lab >= 0).all()


def test_tie_tree_on_the_device(synth_nets):
    check_tie_tree(synth_nets, 0)


def test_early_stop_iteration_counts():
    lab, marg, used, res = check_early_stop(0)
    net, _ = alarm()
    host = F.LoopyBeliefPropagation(net, iterations=200, tol=1e-9, device=-1)
    hlab, hmarg = host.infer(alarm_cases()[:8])
    np.testing.assert_array_equal(used, host.stats[0])
    np.testing.assert_array_equal(bits(res), bits(host.stats[1]))
    np.testing.assert_array_equal(lab, hlab)
    np.testing.assert_array_equal(bits(marg), bits(hmarg))


def test_device_buffers_and_bad_evidence():
    import torch
    net, _ = alarm()
    ev = alarm_cases()[:37].copy()
    lbp = F.LoopyBeliefPropagation(net, iterations=6, device=0)
    lab, marg = lbp.infer(ev)
    st = np.stack([lbp.stats[0].astype(np.float64), lbp.stats[1]], axis=1)
    SD = marg.shape[1]
    stream = torch.cuda.current_stream().cuda_stream
    d_ev = torch.from_numpy(ev).to("cuda")
    outs = []
    for _ in range(2):
        d_lab = torch.full((37,), -7, dtype=torch.int32, device="cuda")
        d_marg = torch.full((37, SD), -1.0, dtype=torch.float64, device="cuda")
        d_st = torch.full((37, 2), -1.0, dtype=torch.float64, device="cuda")
        lbp.run_device(d_ev.data_ptr(), 37, d_lab.data_ptr(), d_marg.data_ptr(), d_st.data_ptr(), stream_ptr=stream)
        torch.cuda.synchronize()
        outs.append((d_lab.cpu().numpy(), d_marg.cpu().numpy(), d_st.cpu().numpy()))
    assert lbp.last_kernel_ms() > 0.0
    for a, b, h in zip(outs[0], outs[1], (lab, marg, st)):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, h)
    # labels only (no marginals, no stats buffer)
    d_lab = torch.full((37,), -7, dtype=torch.int32, device="cuda")
    lbp.run_device(d_ev.data_ptr(), 37, d_lab.data_ptr(), 0, stream_ptr=stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_lab.cpu().numpy(), lab)
    # a bad code in a device buffer is refused before the kernel runs; the handle stays usable
    bad = ev.copy()
    bad[3, 4] = 100
    d_bad = torch.from_numpy(bad).to("cuda")
    d_lab.fill_(-7)
    with pytest.raises(F.FastBNError, match="case 3.*node 4") as e:
        lbp.run_device(d_bad.data_ptr(), 37, d_lab.data_ptr(), 0, stream_ptr=stream)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert (d_lab.cpu().numpy() == -7).all()  # nothing was launched
    with pytest.raises(F.FastBNError, match="case 3.*node 4"):
        lbp.infer(bad)
    lab2, marg2 = lbp.infer(ev)
    np.testing.assert_array_equal(lab2, lab)
    np.testing.assert_array_equal(bits(marg2), bits(marg))


def _cli(*args):
    cli = os.path.join(REPO, "fastbn_amd", "BayesianNetwork")
    out = subprocess.run([cli, *args, "--prefix", GOLD + "/"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_cli():
    out = _cli("-a", "7", "-d", "20")
    assert "loopy belief propagation (LBP)" in out and "propagation length = 20" in out
    acc = float(re.search(r"accuracy = (\S+)", out).group(1))
    mse = re.search(r"average MSE = (\S+)", out).group(1)
    hd = re.search(r"average HD = (\S+)", out).group(1)
    assert re.search(r"lbp: device kernel \S+ s", out)
    from conftest import read_pt_file
    net, tup = alarm()
    ev, truth = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)
    gold = read_pt_file(os.path.join(ALARM, "alarm_1k_pt"), tup[1], len(ev))
    pacc, pmse, phd = F.LoopyBeliefPropagation(net, iterations=20).EvaluateAccuracy(ev, truth, gold)
    assert "%g" % pmse == mse and "%g" % phd == hd  # iostream's default formatting is %g
    assert abs(acc - pacc) < 5e-7
    # the new long flags reach the run: damped, with a tolerance
    out2 = _cli("-a", "7", "-d", "20", "--tol", "1e-6", "--damping", "0.5")
    p2 = F.LoopyBeliefPropagation(net, iterations=20, tol=1e-6, damping=0.5).EvaluateAccuracy(ev, truth, gold)
    assert "%g" % p2[1] == re.search(r"average MSE = (\S+)", out2).group(1)
    # the neighbours still work
    assert "likelihood weighting (LW)" in _cli("-a", "5", "-q", "64")
    assert float(re.search(r"accuracy = (\S+)", _cli("-a", "2")).group(1)) > 0.9
