#!/usr/bin/env python3
"""Time fosphor_amd_measure against the 8 bytes per sample it has to read.

Two calls over float32 IQ in device memory, each a shape of its own:
  wave   4096 jobs of 1024 samples   (one launch of k_measure_wave)
  split  16 jobs of 4 Mi samples     (k_measure_split, then k_measure_combine)
After warm-up the two are repeated alternately; per shape the median over the repetitions of
  call_ms  the whole call on the host clock (wait, table upload, launches, wait)
  gpu_ms   the same between two events on the instance's stream
and gb_per_s = 8 bytes * samples / gpu_ms.  One JSON line per shape, then a table.

  python tools/measure_bench.py [--reps 15] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("wave", 4096, 1024), ("split", 16, 4 << 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    from _pkg import gr_fosphor_amd
    F = gr_fosphor_amd.Fosphor
    f = F(n_bins=128, wf_rows=16)
    st = torch.cuda.ExternalStream(f.stream)
    n = max(n_jobs * per for _, n_jobs, per in SHAPES)
    d_iq = torch.randn((n, 2), device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = {}
    for name, n_jobs, per in SHAPES:
        jobs = np.zeros(n_jobs, F.MEASURE_JOB_DTYPE)
        jobs["offset"] = np.arange(n_jobs, dtype=np.int64) * per + 1		# odd: a single sample at either end of every job
        jobs["n"], jobs["threshold"] = per - 2, 1.0
        d_rec = torch.empty(n_jobs * F.MEASURE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        assert F.measure_form(per - 2) == name

        def call(jobs=jobs, d_rec=d_rec, n_jobs=n_jobs):
            t0 = time.perf_counter()
            e0.record(st)
            rv = f.L.fosphor_amd_measure(f.h, d_iq.data_ptr(), n, jobs.ctypes.data, n_jobs, d_rec.data_ptr())
            e1.record(st)
            e1.synchronize()
            assert rv == 0, rv
            return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

        calls[name] = call
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for rep in range(args.warmup + args.reps):
        for name, call in calls.items():				# alternating: both shapes see the same state of the machine
            t = call()
            if rep >= args.warmup:
                times[name].append(t)
    rows = []
    for name, n_jobs, per in SHAPES:
        call_ms, gpu_ms = (float(np.median([t[i] for t in times[name]])) for i in (0, 1))
        nbytes = 8 * n_jobs * (per - 2)
        row = dict(shape=name, n_jobs=n_jobs, n=per - 2, bytes=nbytes, call_ms=round(call_ms, 4), gpu_ms=round(gpu_ms, 4),
                   gb_per_s=round(nbytes / gpu_ms / 1e6, 1), reps=args.reps)
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| shape | jobs | n | bytes | call ms | gpu ms | GB/s over gpu ms |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %(shape)s | %(n_jobs)d | %(n)d | %(bytes)d | %(call_ms).3f | %(gpu_ms).3f | %(gb_per_s).0f |" % r)
    print("stats:", f.measure_stats())
    print("device:", torch.cuda.get_device_name(0))
    f.close()


if __name__ == "__main__":
    main()
