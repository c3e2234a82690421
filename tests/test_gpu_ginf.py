"""Exact Gaussian inference on the device (ginf.hip) bit for bit against the host twin, the device-buffer entry,
a degenerate case inside a batch, parameter learning over a shared upload, and the continuous pipeline."""
import numpy as np
import pytest
import torch

import fastbn_amd as F
import gci_data as D
import ginf_nets as G

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.int64) == np.ascontiguousarray(b).view(np.int64)).all()


def batch(n, m):
    spec = G.make(n, seed=n)
    net = F.GaussianNetwork(*spec)
    mu, S = net.joint()
    return net, G.cases(mu, S, m, 9, seed=100 * n + m)


# one variable; one observed; a ragged first chunk; the wave edge in the ballot / prefix sum and in the row
# ownership (63, 64, 65); the cap with T = 64 over 72 unobserved variables (a full and a ragged tile); T = 256 over
# 280 (two tiles, the last ragged, two chunks of the index lists); everything observed at the cap
@pytest.mark.parametrize("n,m", [(1, 0), (1, 1), (5, 1), (37, 7), (70, 63), (70, 64), (70, 65), (200, 128), (300, 20),
                                 (128, 128)])
def test_device_equals_host_twin(n, m):
    net, ev = batch(n, m)
    assert ((ev == ev).sum(axis=1) == m).all()
    ref = F.GaussianInference(net, device=-1).infer(ev)
    dev = F.GaussianInference(net)
    for max_workgroups in (0, 1):  # one workgroup: the persistent stride over all nine cases
        dev.set_tuning(max_workgroups)
        out = dev.infer(ev)
        assert all(same_bits(o, r) for o, r in zip(out, ref))
        info = dev.info()
        assert info["workgroups"] == (max_workgroups or 9) and info["m_max"] == m and dev.degenerate == 0
    assert info["tile"] == {128: 64, 20: 256}.get(m, info["tile"])


def test_device_buffers():
    net, ev = batch(37, 7)
    dev = F.GaussianInference(net)
    with pytest.raises(F.FastBNError):
        dev.last_kernel_ms()
    ref = dev.infer(ev)
    stream = torch.cuda.Stream()
    d_ev = torch.from_numpy(ev).cuda()
    d_mean, d_var = (torch.full((9, 37), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    d_logp = torch.full((9,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev.run_device(d_ev.data_ptr(), 9, d_mean.data_ptr(), d_var.data_ptr(), d_logp.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert all(same_bits(o.cpu().numpy(), r) for o, r in zip((d_mean, d_var, d_logp), ref))
    assert dev.last_kernel_ms() > 0
    d_ev[4, 3] = float("inf")
    torch.cuda.synchronize()
    with pytest.raises(F.FastBNError, match="case 4.*variable 3") as e:
        dev.run_device(d_ev.data_ptr(), 9, d_mean.data_ptr(), d_var.data_ptr(), d_logp.data_ptr(), stream.cuda_stream)
    assert e.value.code == -1


def test_degenerate_case_inside_a_batch():
    # node 2 copies node 0 up to a variance that Sigma cannot hold: observing both is degenerate
    net = F.GaussianNetwork([[], [0], [0]], [0.0, 1.0, 0.0], [[], [0.5], [1.0]], [1.0, 1.0, 1e-30])
    ev = np.array([[0.3, np.nan, np.nan], [0.3, np.nan, 0.3], [np.nan, 0.2, np.nan]])
    dev = F.GaussianInference(net)
    alone = dev.infer(ev[[0, 2]])
    assert dev.degenerate == 0
    out = dev.infer(ev)
    assert dev.degenerate == 1 and dev.info()["degenerate"] == 1
    assert all(np.isnan(o[1]).all() and same_bits(o[[0, 2]], a) for o, a in zip(out, alone))
    assert all(same_bits(o, r) for o, r in zip(out, F.GaussianInference(net, device=-1).infer(ev)))


def pipeline_data():
    return D.sem(7, 1500, seed=28, p_edge=0.25)


def test_learning_shares_the_upload():
    ds = F.ContinuousDataset(columns=pipeline_data())
    parents = [[6], [3], [1], [4], [], [], []]
    ci = F.GaussianIndependenceTest(ds)
    shared = F.GaussianParameterLearning(ci)
    assert shared.ci is ci
    a, b = shared.LearnParamsKnowStructCompData(parents).params(), F.GaussianParameterLearning(ds).LearnParamsKnowStructCompData(parents).params()
    assert same_bits(a[0], b[0]) and same_bits(a[2], b[2]) and all(same_bits(x, y) for x, y in zip(a[1], b[1]))
    w = np.linalg.lstsq((ds.columns[[3]] - ds.columns[3].mean()).T, ds.columns[1] - ds.columns[1].mean(), rcond=None)[0]
    assert np.isclose(a[1][1][0], w[0], rtol=1e-11)


def test_continuous_pipeline():
    """PCStable -> pdag_to_dag -> GaussianParameterLearning -> GaussianInference.infer.  Without evidence the
    posterior is the fitted prior, whose means are the sample means and whose variances are the columns' N-divisor
    variances: exactly so where no node has two non-adjacent parents, as in the forest this fixture's PC run
    learns (between such parents the model's zero covariance would replace the sample's)."""
    X = pipeline_data()
    pc = F.PCStable(alpha=0.05)
    res = pc.StructLearnCompData(F.ContinuousDataset(columns=X))
    parents = F.pdag_to_dag(7, res.oriented)
    assert sum(map(len, parents)) >= 4
    net = F.GaussianParameterLearning(pc.ci).LearnParamsKnowStructCompData(parents)
    mean, var, logp = F.GaussianInference(net).infer(np.full((1, 7), np.nan))
    assert np.allclose(mean[0], X.mean(axis=1), rtol=0, atol=1e-12) and logp[0] == 0.0
    assert (np.abs(var[0] / X.var(axis=1) - 1) <= 1e-9).all()
