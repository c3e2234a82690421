"""Exact posterior sampling on the device (jt_psample.hip behind PosteriorSampler).

The device is held to the host twin byte for byte -- every sample and both value doubles -- over the product
of the case counts at which the kernel can go wrong (1: the item remap and the fence with one real case; 63,
64, 65: around a full wave, the last with a one-case block beside a full one; 130: three blocks, the last
ragged), the draws per case (1, 3, 64, 65: below, at and past one item per lane), one wave recycling its
store (max_workgroups=1) and the default grid, and sample_chunk 1, 2 and S.  One distribution check runs on
the device's own output, and the CLI is held to the Python interface."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ALARM, GOLD, REPO
from mpe_nets import alarm_net, chain_net, disconnected_net, shapes_net
from psample_nets import assert_binomial
from test_gpu_mpe import _cases, tie_net

import fastbn_amd as F

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 130)
DRAWS = (1, 3, 64, 65)
SEED, OFFSET = 77, 5


@functools.lru_cache(maxsize=None)
def workload(key):
    if key == "shapes":
        net, ev = shapes_net()[0], _cases(shapes_net()[0], 3, 41)
    elif key == "disconnected":
        net, ev = disconnected_net()[0], _cases(disconnected_net()[0], 2, 42)
    elif key == "tie":
        net, ev = tie_net()
    elif key == "chain":
        net, ev = chain_net(1200)[0], _cases(chain_net(1200)[0], 120, 43)
    else:
        net = alarm_net()[0]
        ev = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)[0][:130]
    assert len(ev) == 130
    return net, ev


@functools.lru_cache(maxsize=None)
def twin(key, draws):
    net, ev = workload(key)
    return F.PosteriorSampler(net, device=-1).value_parts(ev, draws, SEED, OFFSET)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("draws", DRAWS)
@pytest.mark.parametrize("key", ["shapes", "disconnected", "tie", "chain", "alarm"])
def test_device_equals_host_twin(key, draws, n):
    net, ev = workload(key)
    samples, value = twin(key, draws)
    dev = F.PosteriorSampler(net, device=0)
    for groups in (1, 0):
        for chunk in sorted({1, min(2, draws), draws}):
            dev.set_tuning(max_workgroups=groups, sample_chunk=chunk)
            s, v = dev.value_parts(ev[:n], draws, SEED, OFFSET)
            assert s.tobytes() == samples[:n].tobytes(), (groups, chunk)
            assert v.tobytes() == value[:n].tobytes(), (groups, chunk)
    assert dev.last_kernel_ms() > 0.0
    dev.close()


def test_split_default_chunk_and_info():
    net, ev = workload("alarm")
    samples, value = twin("alarm", 65)
    dev = F.PosteriorSampler(net, device=0)  # the chunk the host picks
    assert dev.info() == F.PosteriorSampler(net, device=-1).info()
    s, v = dev.value_parts(ev[64:], 65, SEED, OFFSET + 64)  # a split at a case boundary
    assert s.tobytes() == samples[64:].tobytes() and v.tobytes() == value[64:].tobytes()
    s, v = dev.value_parts(ev, 65, SEED, OFFSET)
    assert s.tobytes() == samples.tobytes() and v.tobytes() == value.tobytes()


def test_alarm_state_frequencies_against_junction_forest():
    net, ev = workload("alarm")
    S = 4096
    samples, log_p = F.PosteriorSampler(net, device=0).sample(ev, draws=S, seed=11)
    _, marg = F.JunctionForest(net, device=0).infer(ev)
    assert np.isfinite(log_p).all()
    off = 0
    for v, d in enumerate(net.dims):
        for q in range(int(d)):
            free = ev[:, v] < 0  # the forest reports zeros for an observed variable
            assert_binomial((samples[free, :, v] == q).sum(axis=1), marg[free, off + q], S, (v, q))
        off += int(d)
        assert (samples[~free, :, v] == ev[~free, v][:, None]).all()


def test_run_device_on_a_side_stream():
    import torch
    net, ev = workload("alarm")
    ev = np.ascontiguousarray(ev[:37])
    ps = F.PosteriorSampler(net, device=0)
    samples, value = ps.value_parts(ev, 3, SEED)
    side = torch.cuda.Stream()
    d_ev = torch.from_numpy(ev).to("cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_s = torch.full((37, 3, 37), -7, dtype=torch.int8, device="cuda")
        d_v = torch.full((37, 2), -1.0, dtype=torch.float64, device="cuda")
        ps.run_device(d_ev.data_ptr(), 37, 3, d_s.data_ptr(), d_v.data_ptr(), seed=SEED, stream_ptr=side.cuda_stream)
    side.synchronize()
    assert d_s.cpu().numpy().tobytes() == samples.tobytes() and d_v.cpu().numpy().tobytes() == value.tobytes()
    ps.close()


def test_cli_psample_alarm(tmp_path):
    out_file = str(tmp_path / "psample.libsvm")
    cli = os.path.join(REPO, "fastbn_amd", "BayesianNetwork")
    run = subprocess.run([cli, "-a", "15", "-q", "3", "--seed", "21", "--out", out_file, "--prefix", GOLD + "/"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    ev, _ = F.load_libsvm(os.path.join(ALARM, "testing_alarm_1k_p20"), 37)
    samples, log_p = F.PosteriorSampler(alarm_net()[0], device=0).sample(ev, draws=3, seed=21)
    got, labels = F.load_libsvm(out_file, 37)
    np.testing.assert_array_equal(got, samples.reshape(-1, 37))
    np.testing.assert_array_equal(labels, got[:, 0])
    total = 0.0
    for x in log_p.tolist():  # the CLI's sum: case order, one add per case
        total += x
    assert re.search(r"average log P\(e\) = (\S+)", run.stdout).group(1) == "%.12g" % (total / len(ev))
    assert re.search(r"psample: device kernel \S+ s, \S+ samples/s", run.stdout)
