#!/usr/bin/env python3
"""Time fosphor_amd_decide against the bytes it has to move.

Shapes over noisy QPSK symbols in device memory that sit still (what fosphor_amd_carrier leaves), every job with DIFF and a
32-symbol unique word searched over the whole job, so all four kernels run:
  jobs64, jobs1024, jobs4096   that many jobs of --per symbols each, back to back     (512 by default)
  long                         one job of 2^--long-log symbols                        (2^20 by default)
Per shape:
  gpu_us   the call between two events on the instance's stream (table upload, four kernels)
  call_us  the whole call on the host clock (wait, table upload, launches, wait)
  copy_us  a device-to-device copy of the bytes the pass cannot avoid, 8 per symbol read and 1 per symbol written, between two
           events on torch's stream: the floor of a pass that reads its input once (this one does)
After warm-up each is repeated; the medians and the spread (min .. max) of gpu_us are reported.  The first and the last job of a
shape are compared bit for bit with fosphor_amd_decide_host.  One JSON line per shape.

  python tools/decide_bench.py [--per 512] [--long-log 20] [--reps 9] [--warmup 3] [--shapes jobs64,jobs1024,jobs4096,long]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per", type=int, default=512)
    ap.add_argument("--long-log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="jobs64,jobs1024,jobs4096,long")
    args = ap.parse_args()

    import torch
    from _pkg import gr_fosphor_amd
    F = gr_fosphor_amd.Fosphor
    f = F(n_bins=128, wf_rows=16)
    st = torch.cuda.ExternalStream(f.stream)
    shapes = {"jobs64": (64, args.per), "jobs1024": (1024, args.per), "jobs4096": (4096, args.per), "long": (1, 1 << args.long_log)}
    order, uw_len, word_at = 4, 32, 100
    flags = F.DECIDE_FLAGS["diff"] | F.DECIDE_FLAGS["uw"]

    for name in args.shapes.split(","):
        n_jobs, per = shapes[name]
        n = n_jobs * per
        torch.manual_seed(1)
        idx = torch.randint(0, order, (n,), device="cuda")
        ph = 2.0 * np.pi * (idx.double() / order + 0.03)
        d_iq = (torch.stack([torch.cos(ph), torch.sin(ph)], 1) + 0.05 * torch.randn((n, 2), device="cuda", dtype=torch.float64)).float().contiguous()
        planted = idx[:per].cpu().numpy()					# job 0's: its differences from word_at on are the word
        uw = ((planted[word_at:word_at + uw_len] - planted[word_at - 1:word_at - 1 + uw_len]) & (order - 1)).astype(np.uint8)
        jobs = np.zeros(n_jobs, F.DECIDE_JOB_DTYPE)
        jobs["offset"] = np.arange(n_jobs, dtype=np.int64) * per
        jobs["out_offset"] = jobs["offset"]					# per is a multiple of 4
        jobs["n"], jobs["order"], jobs["flags"], jobs["uw_len"], jobs["uw_max_errors"] = per, order, flags, uw_len, uw_len
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_rec = torch.empty(n_jobs * F.DECIDE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def decide():
            t0 = time.perf_counter()
            e0.record(st)
            rv = f.L.fosphor_amd_decide(f.h, d_iq.data_ptr(), n, jobs.ctypes.data, n_jobs, uw.ctypes.data, uw_len, d_rec.data_ptr(),
                                        d_out.data_ptr(), n)
            e1.record(st)
            e1.synchronize()
            assert rv == 0, rv
            return (time.perf_counter() - t0) * 1e6, e0.elapsed_time(e1) * 1e3

        src = torch.empty(9 * n, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def copy():
            c0.record()
            dst.copy_(src)
            c1.record()
            c1.synchronize()
            return c0.elapsed_time(c1) * 1e3

        torch.cuda.synchronize()
        times = [decide() for rep in range(args.warmup + args.reps)][args.warmup:]
        copies = [copy() for rep in range(args.warmup + args.reps)][args.warmup:]
        more = [decide() for rep in range(args.reps)]				# again behind the copies: the spread over alternating runs
        rec = d_rec.cpu().numpy().view(F.DECIDE_RECORD_DTYPE)
        out = d_out.cpu().numpy()
        iq = d_iq.cpu().numpy()
        for i in (0, n_jobs - 1):						# the sanity check: the host's bits
            alone = jobs[i:i + 1].copy()
            alone["out_offset"] = 0
            want_rec, want = F.decide_host(iq, alone, uw)
            at = int(jobs["out_offset"][i])
            assert rec[i].tobytes() == want_rec[0].tobytes() and out[at:at + per].tobytes() == want[0].tobytes(), "not the host's bits"
        assert rec["uw_pos"][0] == word_at and rec["uw_errors"][0] == 0, rec[0]
        gpu = [tm[1] for tm in times + more]
        call_us, gpu_us, copy_us = float(np.median([tm[0] for tm in times + more])), float(np.median(gpu)), float(np.median(copies))
        row = dict(shape=name, n_jobs=n_jobs, n=per, order=order, uw_len=uw_len, bytes=9 * n, call_us=round(call_us, 1), gpu_us=round(gpu_us, 1),
                   gpu_us_min=round(min(gpu), 1), gpu_us_max=round(max(gpu), 1), copy_us=round(copy_us, 1), over_copy=round(gpu_us / copy_us, 2),
                   uw_pos=int(rec["uw_pos"][0]), evm_rms=F.decide_derive(rec[:1], uw_len)[0]["evm_rms"],
                   reps=2 * args.reps, stats=f.decide_stats(), device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        del d_iq, d_out, src, dst
    f.close()


if __name__ == "__main__":
    main()
