"""Order MCMC on the device (order_mcmc.hip behind fbn_omcmc_run): the scan against mpmath at its edges, the chains
bit for bit the host twin for every chain count, tuning and split of the chains, and convergence to ArcPosterior."""
import functools

import numpy as np
import pytest

import fastbn_amd as F
import hc_data as H
from test_order_mcmc_host import CONVERGE, SCAN_CASES, check_converged, check_scan, dataset

pytestmark = pytest.mark.gpu

RUN = dict(max_parents=2, burn_in=60, thin=7, samples=30, seed=11)  # 270 steps


@functools.lru_cache(maxsize=None)
def source(n):
    """(Dataset, its context): 9 seeded columns, or the 37 ALARM columns' first 500 rows."""
    if n == 9:
        ds = dataset(9)
    else:
        alarm = F.Dataset(H.ALARM_CSV)
        ds = F.Dataset(columns=np.ascontiguousarray(alarm.columns[:, :500]), dims=alarm.dims)
    return ds, F.IndependenceTest(ds)


@functools.lru_cache(maxsize=None)
def twin(n, chains, chain_offset=0):
    return F.OrderMCMC("bde", chains=chains, chain_offset=chain_offset, **RUN).learn(source(n)[0], host=True)


def assert_same_chains(dev, host):
    assert H.bits_equal(dev.chain_arc_prob, host.chain_arc_prob) and H.bits_equal(dev.log_score, host.log_score)
    assert np.array_equal(dev.orders, host.orders) and np.array_equal(dev.accepted, host.accepted)


@pytest.mark.parametrize("n,k,forbidden,prior,seeded", SCAN_CASES)
def test_terms_and_arcs_against_mpmath(n, k, forbidden, prior, seeded):
    check_scan(lambda ds: F.IndependenceTest(ds), False, n, k, forbidden, prior, seeded)


# 3 chains a workgroup: 70 = 23 x 3 + 1, a ragged last workgroup; 37 steps a launch: 270 = 7 x 37 + 11
@pytest.mark.parametrize("tuning", [(0, 0), (3, 37)])
@pytest.mark.parametrize("chains", [1, 5, 70])
@pytest.mark.parametrize("n", [9, 37])
def test_device_equals_twin(n, chains, tuning):
    ci = source(n)[1]
    try:
        F.OrderMCMC.set_tuning(ci, *tuning)
        dev = F.OrderMCMC("bde", chains=chains, **RUN).learn(ci)
    finally:
        F.OrderMCMC.set_tuning(ci)
    host = twin(n, chains)
    assert_same_chains(dev, host)
    assert H.bits_equal(dev.arc_prob, host.arc_prob)
    assert dev.info["launches"] == (8 if tuning[1] else 1) and dev.info["families"] == host.info["families"]


@pytest.mark.parametrize("n", [9, 37])
def test_split_chains_are_one_run(n):
    ci, whole = source(n)[1], twin(n, 70)
    for off in (0, 35):
        part = F.OrderMCMC("bde", chains=35, chain_offset=off, **RUN).learn(ci)
        for name in ("chain_arc_prob", "log_score", "orders", "accepted"):
            assert np.array_equal(getattr(part, name), getattr(whole, name)[off:off + 35]), (off, name)


@pytest.mark.parametrize("prior", ["uniform", "indegree"])
def test_converges_to_exact_posterior(prior):
    ds = dataset(5)
    dev = F.OrderMCMC("bde", prior=prior, **CONVERGE).learn(ds)
    assert_same_chains(dev, F.OrderMCMC("bde", prior=prior, **CONVERGE).learn(ds, host=True))
    check_converged(dev, ds, prior)
