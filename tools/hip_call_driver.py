#!/usr/bin/env python3
"""A small walk over the host paths of the library, to be traced:

    rocprofv3 --hip-trace -f csv json -d OUT -o trace -- python3 tools/hip_call_driver.py

One instance per FFT length (1024 fp32, 8192 fp32, 65536 fp16), each called once (the two host paths three times: the staging ring
has two slots, the third call waits for the first) through fosphor_process, fosphor_amd_process_pinned, fosphor_amd_process_device
with one piece / with several pieces / with a batch of 2048 spectra (N = 1024: slab sums; N = 8192: one chunk),
fosphor_amd_process_device_overlap, fosphor_amd_accumulate_device with a single-launch shard and with a chunked one, each followed
by fosphor_amd_merge, and fosphor_amd_get_buffers after every path.  FOSPHOR_AMD_SUB_LOG2 is set so that a sub-launch holds 32
spectra.  Every input is allocated before the instance is made, and hipMemGetInfo -- which the library never calls -- is called
around fosphor_amd_init and around fosphor_release, so that tools/compare_hip_calls.py can tell the calls made inside those two
from the calls made between them.  FOSPHOR_AMD_LIB selects the library (gr-fosphor_amd/_lib.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mark(torch):
    torch.cuda.mem_get_info()


def walk(amd, torch, log2n, fmt):
    n = 1 << log2n
    os.environ["FOSPHOR_AMD_SUB_LOG2"] = str(log2n + 5)
    dtype, ttype = (np.float16, torch.float16) if fmt == "fp16" else (np.float32, torch.float32)
    rng = np.random.default_rng(log2n)
    host = (rng.standard_normal(16 * n * 2) * 0.05).astype(dtype)
    pinned = torch.from_numpy(host.copy()).pin_memory()
    long_batch = 2048
    dev = (torch.randn(long_batch * n * 2, device="cuda", dtype=torch.float32) * 0.05).to(ttype)
    torch.cuda.synchronize()

    mark(torch)
    f = amd.Fosphor(fft_len_log=log2n, n_bins=128, wf_rows=64, max_spectra=long_batch, max_batches=4, iq_format=fmt)
    mark(torch)

    def done(what):
        f.buffers()				# fosphor_amd_get_buffers: the hit-count view of the path just taken
        assert f.finish() >= 0, what

    for _ in range(3):
        assert f.process(host) == 0
        done("process")
    for _ in range(3):
        assert f.L.fosphor_amd_process_pinned(f.h, pinned.data_ptr(), 16 * n) == 0
        done("process_pinned")
    assert f.process_device(dev, 2, 16) == 0		# one piece
    done("process_device, one piece")
    assert f.process_device(dev, 4, 16) == 0		# two pieces of two batches
    done("process_device, two pieces")
    if log2n != 16:
        assert f.process_device(dev, 1, long_batch) == 0
        done("process_device, long batch")
    assert f.process_device_overlap(dev, 2, 16, 2) == 0
    done("process_device_overlap")
    assert f.accumulate_device(dev, 48, 16, 64) == 0 and f.merge(64) == 0		# a shard that goes out in one launch
    done("accumulate, single launch")
    assert f.accumulate_device(dev, long_batch, 0, long_batch) == 0 and f.merge(long_batch) == 0	# two pieces of 1024 spectra
    done("accumulate, chunked")
    assert f.process(host) == 0				# back on the pipelined path
    done("process after merge")
    print("N = %d: merge_stats %s, launch_stats %s" % (n, f.merge_stats(), f.launch_stats()))

    mark(torch)
    f.close()
    mark(torch)


def main():
    import torch
    from _pkg import gr_fosphor_amd as amd
    assert torch.cuda.is_available()
    for log2n, fmt in ((10, "fp32"), (13, "fp32"), (16, "fp16")):
        walk(amd, torch, log2n, fmt)
    print("driver done")


if __name__ == "__main__":
    main()
