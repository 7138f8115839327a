#!/usr/bin/env python3
"""Time fosphor_amd_demod against the bytes it has to move, next to a plain torch expression for the same traces.

One call of 4096 jobs of 4096 samples each (16 Mi samples, 128 MiB of float32 IQ in device memory), in one mode with one L:
  demod  fosphor_amd_demod between two events on the instance's stream (table upload and the one kernel), and the whole call on
         the host clock (wait, table upload, launch, wait)
  torch  the same traces by a torch expression on the same device, between two events on torch's stream:
           power  x.abs() ** 2                          phase  torch.angle(x) / (2 pi)
           fm     torch.angle(x[:, 1:] * x[:, :-1].conj()) / (2 pi)
         and, for L > 1, v[:, :n_out * L].reshape(jobs, n_out, L).mean(-1)
After warm-up the two are repeated alternately; the medians are reported.  bytes = 8 per sample read + 4 per output written;
read_share = (8 * samples / gpu_ms) / 8 TB/s, the share of the HBM read roofline the call reaches.  The torch trace is also the
sanity check: the two must agree to 1e-5 (they are not bit-identical: torch's angle and mean are not pinned).
One JSON line.

  python tools/demod_bench.py --mode fm --avg 16 [--reps 15] [--warmup 3]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_JOBS, PER = 4096, 4096
HBM_READ = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["power", "phase", "fm"], required=True)
    ap.add_argument("--avg", type=int, default=1)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    from _pkg import gr_fosphor_amd
    F = gr_fosphor_amd.Fosphor
    f = F(n_bins=128, wf_rows=16)
    st = torch.cuda.ExternalStream(f.stream)
    L = args.avg
    n = N_JOBS * PER
    torch.manual_seed(1)
    d_iq = torch.randn((N_JOBS, PER, 2), device="cuda")
    x = torch.view_as_complex(d_iq)
    n_out = F.demod_n_out(args.mode, PER, L)
    jobs = np.zeros(N_JOBS, F.DEMOD_JOB_DTYPE)
    jobs["offset"] = np.arange(N_JOBS, dtype=np.int64) * PER
    jobs["out_offset"] = np.arange(N_JOBS, dtype=np.int64) * n_out
    jobs["n"], jobs["mode"], jobs["avg"] = PER, F.DEMOD_MODES[args.mode], L
    d_out = torch.empty(N_JOBS * n_out, dtype=torch.float32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0e, t1e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def demod():
        t0 = time.perf_counter()
        e0.record(st)
        rv = f.L.fosphor_amd_demod(f.h, d_iq.data_ptr(), n, jobs.ctypes.data, N_JOBS, d_out.data_ptr(), N_JOBS * n_out)
        e1.record(st)
        e1.synchronize()
        assert rv == 0, rv
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    def expression():
        if args.mode == "power":
            v = x.abs() ** 2
        elif args.mode == "phase":
            v = torch.angle(x) / (2.0 * math.pi)
        else:
            v = torch.angle(x[:, 1:] * x[:, :-1].conj()) / (2.0 * math.pi)
        return v if L == 1 else v[:, :n_out * L].reshape(N_JOBS, n_out, L).mean(-1)

    def yardstick():
        t0e.record()
        v = expression()
        t1e.record()
        t1e.synchronize()
        return t0e.elapsed_time(t1e), v

    torch.cuda.synchronize()
    times, torch_ms = [], []
    for rep in range(args.warmup + args.reps):				# alternating: both see the same state of the machine
        t = demod()
        ms, v = yardstick()
        if rep >= args.warmup:
            times.append(t)
            torch_ms.append(ms)
    d = (d_out.view(N_JOBS, n_out) - v).abs()
    if args.mode != "power":
        d = torch.minimum(d, 1.0 - d)					# -0.5 and 0.5 are one angle
    else:
        d = d / (1.0 + v)
    worst = float(d.max())
    assert worst <= 1e-5, worst
    call_ms, gpu_ms = (float(np.median([t[i] for t in times])) for i in (0, 1))
    read, written = 8 * n, 4 * N_JOBS * n_out
    row = dict(mode=args.mode, avg=L, form="direct" if L == 1 else "avg", n_jobs=N_JOBS, n=PER, n_out=n_out, bytes_read=read,
               bytes_written=written, call_ms=round(call_ms, 4), gpu_ms=round(gpu_ms, 4),
               gb_per_s=round((read + written) / gpu_ms / 1e6, 1), read_share=round(read / (gpu_ms * 1e-3) / HBM_READ, 4),
               torch_ms=round(float(np.median(torch_ms)), 4), worst_diff_to_torch=worst, reps=args.reps,
               stats=f.demod_stats(), device=torch.cuda.get_device_name(0))
    print(json.dumps(row), flush=True)
    f.close()


if __name__ == "__main__":
    main()
