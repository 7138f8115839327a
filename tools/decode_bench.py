#!/usr/bin/env python3
"""Time fosphor_amd_decode against the bytes it has to move.

Shapes over QPSK symbol bytes in device memory that sit still (what fosphor_amd_decide leaves): terminated frames of the K = 7
(171, 133) code at rate 1/2 with CRC-16 and one coded bit in 50 inverted, so all four kernels run and every CRC holds:
  jobs64, jobs1024, jobs4096   that many jobs of --per steps each, back to back       (1024 by default)
  long                         one job of 65536 steps
Per shape:
  gpu_us     the call between two events on the instance's stream (table upload, four kernels)
  call_us    the whole call on the host clock (wait, table upload, launches, wait)
  nocrc_us   gpu_us of the same jobs with crc_width 0: the difference is the serial CRC of k_dcd_rec
  copy_us    a device-to-device copy of the bytes the pass cannot avoid, 1 per symbol read and 1 per 8 steps written, between two
             events on torch's stream
After warm-up each is repeated; the medians and the spread (min .. max) of gpu_us are reported.  The first and the last job of a
shape are compared bit for bit with fosphor_amd_decode_host.  One JSON line per shape.

  python tools/decode_bench.py [--per 1024] [--reps 9] [--warmup 3] [--shapes jobs64,jobs1024,jobs4096,long]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, POLYS, CRC = 7, (0o171, 0o133), (16, 0x1021, 0xffff, 0)


def crc16(bits):
    reg = CRC[2]
    for bit in bits:
        top = ((reg >> 15) & 1) ^ int(bit)
        reg = (reg << 1) & 0xffff
        if top:
            reg ^= CRC[1]
    return reg


def frame(rng, steps):
    """one QPSK symbol a step: info, CRC-16, six tail bits, encoded at rate 1/2, a coded bit in 50 inverted"""
    info = rng.integers(0, 2, steps - 16 - (K - 1))
    v = crc16(info)
    bits = np.concatenate([info, [(v >> (15 - i)) & 1 for i in range(16)], np.zeros(K - 1, np.int64)])
    u = np.concatenate([np.zeros(K - 1, np.int64), bits])
    streams = np.zeros((steps, 2), np.int64)
    for i, poly in enumerate(POLYS):
        for j in range(K):
            if (poly >> j) & 1:
                streams[:, i] ^= u[j:j + steps]
    coded = streams.reshape(-1)
    coded[rng.choice(2 * steps, 2 * steps // 50, replace=False)] ^= 1
    return (2 * coded[0::2] + coded[1::2]).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="jobs64,jobs1024,jobs4096,long")
    args = ap.parse_args()

    import torch
    from _pkg import gr_fosphor_amd
    F = gr_fosphor_amd.Fosphor
    f = F(n_bins=128, wf_rows=16)
    st = torch.cuda.ExternalStream(f.stream)
    shapes = {"jobs64": (64, args.per), "jobs1024": (1024, args.per), "jobs4096": (4096, args.per), "long": (1, F.DECODE_MAX_STEPS)}

    for name in args.shapes.split(","):
        n_jobs, per = shapes[name]
        n = n_jobs * per
        rng = np.random.default_rng(1)
        kinds = [frame(rng, per) for i in range(min(n_jobs, 16))]		# sixteen different frames, repeated
        sym = np.concatenate([kinds[i % len(kinds)] for i in range(n_jobs)])
        d_sym = torch.from_numpy(sym).cuda()
        own = F.decode_owned(per - (K - 1))
        jobs = np.zeros(n_jobs, F.DECODE_JOB_DTYPE)
        jobs["offset"] = np.arange(n_jobs, dtype=np.int64) * per
        jobs["out_offset"] = np.arange(n_jobs, dtype=np.int64) * own
        jobs["n"], jobs["order"], jobs["flags"], jobs["k"], jobs["n_poly"], jobs["period"] = per, 4, 1, K, 2, 1
        jobs["polys"], jobs["punct"] = POLYS + (0,), (1, 1, 0)
        jobs["crc_width"], jobs["crc_poly"], jobs["crc_init"] = CRC[:3]
        plain = jobs.copy()
        plain["crc_width"], plain["crc_poly"], plain["crc_init"] = 0, 0, 0
        d_out = torch.empty(n_jobs * own, dtype=torch.uint8, device="cuda")
        d_rec = torch.empty(n_jobs * F.DECODE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def decode(table=jobs):
            t0 = time.perf_counter()
            e0.record(st)
            rv = f.L.fosphor_amd_decode(f.h, d_sym.data_ptr(), n, table.ctypes.data, n_jobs, d_rec.data_ptr(), d_out.data_ptr(), n_jobs * own)
            e1.record(st)
            e1.synchronize()
            assert rv == 0, rv
            return (time.perf_counter() - t0) * 1e6, e0.elapsed_time(e1) * 1e3

        moved = n + n // 8
        src = torch.empty(moved, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def copy():
            c0.record()
            dst.copy_(src)
            c1.record()
            c1.synchronize()
            return c0.elapsed_time(c1) * 1e3

        torch.cuda.synchronize()
        nocrc = [decode(plain) for rep in range(args.warmup + args.reps)][args.warmup:]
        times = [decode() for rep in range(args.warmup + args.reps)][args.warmup:]
        copies = [copy() for rep in range(args.warmup + args.reps)][args.warmup:]
        more = [decode() for rep in range(args.reps)]				# again behind the copies: the spread over alternating runs
        rec = d_rec.cpu().numpy().view(F.DECODE_RECORD_DTYPE)
        out = d_out.cpu().numpy()
        for i in (0, n_jobs - 1):						# the sanity check: the host's bits
            alone = jobs[i:i + 1].copy()
            alone["out_offset"] = 0
            want_rec, want = F.decode_host(sym, alone)
            at = int(jobs["out_offset"][i])
            assert rec[i].tobytes() == want_rec[0].tobytes() and out[at:at + len(want[0])].tobytes() == want[0].tobytes(), "not the host's bits"
        assert not rec["status"].any() and (rec["metric"] == 2 * per // 50).all(), rec[0]
        gpu = [tm[1] for tm in times + more]
        call_us, gpu_us, copy_us = float(np.median([tm[0] for tm in times + more])), float(np.median(gpu)), float(np.median(copies))
        nocrc_us = float(np.median([tm[1] for tm in nocrc]))
        row = dict(shape=name, n_jobs=n_jobs, steps=per, k=K, crc_width=16, bytes=moved, call_us=round(call_us, 1), gpu_us=round(gpu_us, 1),
                   gpu_us_min=round(min(gpu), 1), gpu_us_max=round(max(gpu), 1), nocrc_us=round(nocrc_us, 1), copy_us=round(copy_us, 1),
                   over_copy=round(gpu_us / copy_us, 2), ns_per_step_of_a_wave=round(1e3 * nocrc_us / per, 2), metric=int(rec["metric"][0]),
                   reps=2 * args.reps, stats=f.decode_stats(), device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        del d_sym, d_out, src, dst
    f.close()


if __name__ == "__main__":
    main()
