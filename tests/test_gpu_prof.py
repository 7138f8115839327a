"""GPU: the profiling read-outs -- fosphor_amd_profile, fosphor_amd_kernel_times, fosphor_amd_kernel_busy, fosphor_amd_exchange_time --
all of which read the one event-pair timer of csrc/fosphor_prof.cpp (EventTimer, csrc/fosphor_instance.h).

Small on purpose: N = 1024, 128 bins, 16 spectra per batch, two calls of two batches.  Times are compared with each other only (and
with zero), never with a measured constant.  The state after the profiled calls is the oracle's (test_gpu_parity's compare_state and
bars): the timing events perturb nothing.  The exchange is timed on one rank in a child process, through the library's own RCCL
communicator, like test_gpu_dist's one-rank test."""
import os
import subprocess
import sys
import types

import pytest

from oracle_lib import Oracle, gaussian_iq, add_tone
from test_gpu_parity import amd, torch_cuda, compare_state	# noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BINS, BATCH, NBAT, CALLS = 1024, 128, 16, 2, 2
KINDS = ("K1", "K2", "K3")


@pytest.fixture(scope="module")
def two_calls(oracle_built):
    """(the samples of the two calls, the oracle's state after them as compare_state reads it, frozen)"""
    o = Oracle(n_bins=BINS)
    xs = []
    for k in range(CALLS):
        x = add_tone(gaussian_iq(NBAT * BATCH * N, 900 + k), 0.2, 0.07 + 0.03 * k, t0=k * NBAT * BATCH * N)
        for b in range(NBAT):
            assert o.process(x[b * BATCH * N:(b + 1) * BATCH * N], nthreads=4) == 0
        xs.append(x)
    return xs, types.SimpleNamespace(waterfall_pos=o.waterfall_pos, hitcount=o.hitcount, waterfall=o.waterfall,
                                     spectrum=o.spectrum, histogram=o.histogram)


def _run(amd, torch, xs, profile):
    """a fresh instance after the two calls, profiling set before the first"""
    f = amd.Fosphor(n_bins=BINS, max_spectra=NBAT * BATCH)
    f.profile(profile)
    keep = [torch.from_numpy(x).cuda() for x in xs]
    for d in keep:
        assert f.process_device(d, NBAT, BATCH) == 0
    return f, keep


def test_profiling_off_times_nothing(amd, torch_cuda, two_calls):
    xs, want = two_calls
    f, _ = _run(amd, torch_cuda, xs, False)
    ms, launches = f.kernel_times()
    assert launches == [0, 0, 0] and ms == [0.0, 0.0, 0.0], (ms, launches)
    assert f.kernel_busy() == [0.0, 0.0, 0.0]
    compare_state(f, want, "profiling off")
    f.close()


def test_profile_every_kernel(amd, torch_cuda, two_calls):
    """profile(1): every kind is timed; the union of a kind's intervals is positive and no longer than their sum; reading resets."""
    xs, want = two_calls
    f, _ = _run(amd, torch_cuda, xs, True)
    busy = f.kernel_busy()			# (first: kernel_times resets)
    ms, launches = f.kernel_times()
    print("busy ms %s, summed ms %s, launches %s" % (busy, ms, launches))
    for k, name in enumerate(KINDS):
        assert launches[k] >= 1 and ms[k] > 0.0, "%s: %d launches, %g ms" % (name, launches[k], ms[k])
        assert 0.0 < busy[k] <= ms[k] + 1e-3, "%s: busy %g ms against a sum of %g ms" % (name, busy[k], ms[k])
    ms2, launches2 = f.kernel_times()
    assert launches2 == [0, 0, 0] and ms2 == [0.0, 0.0, 0.0], "a second read right after the first: %s, %s" % (ms2, launches2)
    assert f.kernel_busy() == [0.0, 0.0, 0.0]
    compare_state(f, want, "profile(1)")
    f.close()


def test_profile_fft_kernel_only(amd, torch_cuda, two_calls):
    """profile(2): K1 only."""
    xs, want = two_calls
    f, _ = _run(amd, torch_cuda, xs, 2)
    ms, launches = f.kernel_times()
    assert launches[0] >= 1 and ms[0] > 0.0, (ms, launches)
    assert launches[1:] == [0, 0] and ms[1:] == [0.0, 0.0], (ms, launches)
    compare_state(f, want, "profile(2)")
    f.close()


def test_profiling_switched_between_calls(amd, torch_cuda, two_calls):
    """Only the launches made while profiling is on are timed, and the events of a read-out are used again by the next."""
    torch = torch_cuda
    xs, want = two_calls
    f = amd.Fosphor(n_bins=BINS, max_spectra=NBAT * BATCH)
    keep = [torch.from_numpy(x).cuda() for x in xs]
    f.profile(True)
    assert f.process_device(keep[0], NBAT, BATCH) == 0
    _, first = f.kernel_times()
    assert f.process_device(keep[1], NBAT, BATCH) == 0
    busy = f.kernel_busy()
    ms, second = f.kernel_times()
    assert second == first and min(first) >= 1, "the same call timed twice: %s, then %s launches" % (first, second)
    for k, name in enumerate(KINDS):
        assert 0.0 < busy[k] <= ms[k] + 1e-3, "%s: busy %g ms against a sum of %g ms" % (name, busy[k], ms[k])
    compare_state(f, want, "profiled, read between the calls")
    f.profile(False)
    assert f.process_device(keep[0], NBAT, BATCH) == 0
    assert f.kernel_times()[1] == [0, 0, 0]
    f.close()


EXCHANGE = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["FOSPHOR_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FOSPHOR_ROOT"], "tests"))
import torch
from _pkg import gr_fosphor_amd
from gr_fosphor_amd.dist import ShardedFosphor
from oracle_lib import Oracle, gaussian_iq, add_tone

# One rank, the library's own RCCL communicator: accumulate -> fosphor_amd_exchange -> merge, one frame of 16 spectra at a time.
torch.cuda.set_device(0)
N, BINS, TOTAL = 1024, 128, 16
sf = ShardedFosphor(gr_fosphor_amd.Fosphor, 0, 1, exchange="rccl", force_exchange=True, sliced=False, wire="u32",
                    n_bins=BINS, max_spectra=TOTAL)
assert sf.comm is not None
f, o = sf.f, Oracle(n_bins=BINS)
keep = []

def frame(k):
    x = add_tone(gaussian_iq(TOTAL * N, 950 + k), 0.2, 0.11 + 0.02 * k, t0=k * TOTAL * N)
    keep.append(torch.from_numpy(x).cuda())
    sf.frame(keep[-1], TOTAL)
    assert o.process(x, strict=False, nthreads=4) == 0

f.profile(True)
frame(0)
ms, count = f.exchange_time()
assert count == 1, "profiling on: %d exchanges timed" % count
ms, count = f.exchange_time()
assert (ms, count) == (0.0, 0), "a second read right after the first: %g ms, %d exchanges" % (ms, count)
f.profile(False)
frame(1)
ms, count = f.exchange_time()
assert (ms, count) == (0.0, 0), "profiling off: %g ms, %d exchanges" % (ms, count)
assert f.finish() >= 0
assert f.waterfall_pos == o.waterfall_pos
assert np.array_equal(f.hitcount, o.hitcount.T), "hit counts differ from the oracle"
assert np.allclose(f.histogram, o.histogram, rtol=1e-4, atol=2e-6)
assert np.allclose(f.spectrum[..., 1], o.spectrum[..., 1], rtol=1e-4, atol=1e-6)
sf.close()
print("exchange ok")
'''


def test_exchange_time_single_rank(amd, torch_cuda, oracle_built, tmp_path):
    """fosphor_amd_exchange_time around fosphor_amd_exchange on a real RCCL communicator of one rank: one exchange timed while
    profiling is on, none left after the read, none timed while it is off."""
    from gr_fosphor_amd.dist import NativeComm
    if not NativeComm.available(amd.load()):
        pytest.skip("no RCCL library can be bound in this process")
    script = tmp_path / "exchange_time.py"
    script.write_text(EXCHANGE)
    env = dict(os.environ, FOSPHOR_ROOT=ROOT)
    env.pop("FOSPHOR_AMD_WIRE", None)
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert p.returncode == 0 and "exchange ok" in p.stdout, p.stdout[-3000:]
