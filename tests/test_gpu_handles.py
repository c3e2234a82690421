"""The lifecycle every handle with device state shares (fbn::DeviceHandle, fbn_device.h): the timing
events behind last_kernel_ms, the host-only handle (device=-1) refusing a device run, and destroy
draining the caller streams runs were queued on.

One case per class on ALARM, 65 cases of testing_alarm_1k_p20 (a full 64-case block and a one-case
tail), with the sampler / iteration / update settings of each class's own device-buffer test."""
import functools

import numpy as np
import pytest
from test_epis_host import alarm, alarm_cases

import fastbn_amd as F

pytestmark = pytest.mark.gpu

NODEV = -5  # fbn_err_t (include/fastbn.h)
N, OFFSET = 65, 3

CLASSES = {
    "JunctionTree": (F.JunctionTree, {}),
    "JunctionForest": (F.JunctionForest, {}),
    "LoopyBeliefPropagation": (F.LoopyBeliefPropagation, dict(iterations=6)),
    "LikelihoodWeighting": (F.LikelihoodWeighting, dict(num_samples=100, seed=9)),
    "EPISBN": (F.EPISBN, dict(num_samples=100, iterations=6, seed=9)),
    "AISBN": (F.AISBN, dict(num_samples=100, max_updates=2, interval=40, seed=9)),
    "MostProbableExplanation": (F.MostProbableExplanation, {}),
}
SAMPLERS = ("LikelihoodWeighting", "EPISBN", "AISBN")  # (their draws depend on the case's global index)
names = pytest.mark.parametrize("name", list(CLASSES))


def make(name, device):
    cls, kw = CLASSES[name]
    return cls(alarm()[0], device=device, **kw)


def cases():
    return alarm_cases()[0][:N]


def infer(h, name, ev):
    """The two outputs of the class's host-buffer run: (labels, marginals), for MPE (assignment, value)."""
    if name == "MostProbableExplanation":
        return h.value_parts(ev)
    return h.infer(ev, case_offset=OFFSET) if name in SAMPLERS else h.infer(ev)


@functools.lru_cache(maxsize=None)
def expected(name):
    """infer's outputs for the 65 cases on a device handle, computed once per class."""
    h = make(name, 0)
    a, b = infer(h, name, cases())
    h.close()
    return a.tobytes(), b.tobytes()


def device_outputs(name, n):
    """Poisoned device buffers of a run of n cases: (first, second) as infer returns them."""
    import torch
    V, SD = 37, int(np.sum(alarm()[0].dims))
    if name == "MostProbableExplanation":
        return (torch.full((n, V), -7, dtype=torch.int8, device="cuda"),
                torch.full((n, 2), -1.0, dtype=torch.float64, device="cuda"))
    return (torch.full((n,), -7, dtype=torch.int32, device="cuda"),
            torch.full((n, SD), -1.0, dtype=torch.float64, device="cuda"))


def run_device(h, name, d_ev, n, d_a, d_b, stream):
    if name in SAMPLERS:
        h.run_device(d_ev.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr(), case_offset=OFFSET, stream_ptr=stream)
    else:
        h.run_device(d_ev.data_ptr(), n, d_a.data_ptr(), d_b.data_ptr(), stream_ptr=stream)


def sampling_ms(h, name):
    ms = h.last_kernel_ms()
    return ms[1] if name == "EPISBN" else ms


@names
def test_last_kernel_ms_needs_a_timed_run(name):
    h = make(name, 0)
    with pytest.raises(F.FastBNError, match="no timed launch"):
        h.last_kernel_ms()
    infer(h, name, cases()[:1])
    assert sampling_ms(h, name) > 0.0
    h.close()


@names
def test_host_only_handle_refuses_a_device_run(name):
    """The argument checks come first and refuse null pointers, so the buffers are real."""
    import torch
    h = make(name, -1)
    d_ev = torch.from_numpy(cases()[:1].copy()).to("cuda")
    d_a, d_b = device_outputs(name, 1)
    torch.cuda.synchronize()
    with pytest.raises(F.FastBNError) as e:
        run_device(h, name, d_ev, 1, d_a, d_b, torch.cuda.current_stream().cuda_stream)
    assert e.value.code == NODEV
    torch.cuda.synchronize()
    # nothing ran and nothing was written: no timed launch, the outputs as they were
    with pytest.raises(F.FastBNError, match="no timed launch"):
        h.last_kernel_ms()
    assert (d_a == -7).all().item() and (d_b == -1.0).all().item()
    h.close()


@names
def test_destroy_drains_the_callers_stream(name):
    """A run queued on a side stream, the handle closed at once: its buffers outlive the kernels."""
    import torch
    want = expected(name)
    d_ev = torch.from_numpy(cases().copy()).to("cuda")
    d_a, d_b = device_outputs(name, N)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    h = make(name, 0)
    run_device(h, name, d_ev, N, d_a, d_b, side.cuda_stream)
    h.close()
    side.synchronize()
    assert d_a.cpu().numpy().tobytes() == want[0]
    assert d_b.cpu().numpy().tobytes() == want[1]
