#!/usr/bin/env python3
"""Time fosphor_amd_extract against a device-to-device copy of the same bytes.

For 1, 64 and 4096 jobs, D in {4, 16, 64, 1024} with T = min(8 D + 1, 8192) taps, over a 64 Mi-sample sc16 and fp32 buffer: the
jobs cut the buffer into equal segments and each takes every output its segment allows.  Per shape, after warm-up, the median over
repeated calls of
  call_ms    the whole call on the host clock (wait, table upload, launch, wait)
  gpu_ms     the same between two events on the instance's stream
  copy_ms    a device-to-device copy of (input bytes the jobs span + output bytes), between two events
and ratio = gpu_ms / copy_ms.  One JSON line per shape, then a table.

  python tools/extract_bench.py [--samples-log2 26] [--reps 9] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    return float(np.median([fn() for _ in range(reps)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples-log2", type=int, default=26)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    from _pkg import gr_fosphor_amd
    F = gr_fosphor_amd.Fosphor
    n = 1 << args.samples_log2
    f = F(n_bins=128, wf_rows=16)
    st = torch.cuda.ExternalStream(f.stream)
    rows = []
    for fmt, dtype, bytes_per in (("sc16", torch.int16, 4), ("fp32", torch.float32, 8)):
        d_x = (torch.randn((n, 2), device="cuda") * (1000.0 if fmt == "sc16" else 1.0)).to(dtype)
        for n_jobs in (1, 64, 4096):
            for d in (4, 16, 64, 1024):
                t = min(8 * d + 1, F.EXTRACT_MAX_TAPS)
                seg = n // n_jobs
                n_out = (seg - t) // d + 1
                jobs = np.zeros(n_jobs, F.EXTRACT_DTYPE)
                jobs["first"] = np.arange(n_jobs, dtype=np.int64) * seg
                jobs["out_offset"] = np.arange(n_jobs, dtype=np.int64) * n_out
                jobs["n_out"], jobs["decim"], jobs["n_taps"] = n_out, d, t
                jobs["phase_inc"] = 0x12345679
                d_taps = torch.from_numpy(F.extract_design(d, t, 0.8)).cuda()
                cap = n_jobs * n_out
                d_out = torch.empty(cap, dtype=torch.complex64, device="cuda")
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                times = {}

                def call():
                    t0 = time.perf_counter()
                    e0.record(st)
                    rv = f.L.fosphor_amd_extract(f.h, d_x.data_ptr(), n, {"fp32": 0, "sc16": 2}[fmt], jobs.ctypes.data, n_jobs,
                                                 d_taps.data_ptr(), t, d_out.data_ptr(), cap)
                    e1.record(st)
                    e1.synchronize()
                    assert rv == 0, rv
                    times["gpu"] = e0.elapsed_time(e1)
                    return (time.perf_counter() - t0) * 1e3

                call_ms = median_ms(call, args.reps, args.warmup)
                gpu_ms = median_ms(lambda: (call(), times["gpu"])[1], args.reps, 0)
                nbytes = n_jobs * ((n_out - 1) * d + t) * bytes_per + cap * 8
                src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

                def copy():
                    e0.record()
                    dst.copy_(src)
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1)

                copy_ms = median_ms(copy, args.reps, args.warmup)
                del src, dst
                row = dict(fmt=fmt, n_jobs=n_jobs, decim=d, n_taps=t, form=F.extract_form(d, t), n_out_per_job=n_out, bytes=nbytes,
                           call_ms=round(call_ms, 4), gpu_ms=round(gpu_ms, 4), copy_ms=round(copy_ms, 4),
                           ratio=round(gpu_ms / copy_ms, 2))
                rows.append(row)
                print(json.dumps(row), flush=True)
        del d_x
    print("\n| format | jobs | D | T | form | bytes | call ms | gpu ms | copy ms | gpu / copy |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %(fmt)s | %(n_jobs)d | %(decim)d | %(n_taps)d | %(form)s | %(bytes)d | %(call_ms).3f | %(gpu_ms).3f | %(copy_ms).3f | %(ratio).2f |" % r)
    print("device:", torch.cuda.get_device_name(0))
    f.close()


if __name__ == "__main__":
    main()
