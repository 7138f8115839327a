#!/usr/bin/env python3
"""Time fosphor_amd_soft beside fosphor_amd_decode on the same frames.

Terminated frames of the K = 7 (171, 133) code at rate 1/2 with CRC-16 as Gray QPSK symbols with white noise of 0.45 a part
(Es / N0 = 3.9 dB) in device memory (what fosphor_amd_carrier leaves), and their hard decisions as bytes (what
fosphor_amd_decide leaves): sixteen different frames, repeated.
  jobs64, jobs1024, jobs4096   that many jobs of --per steps each, back to back       (1024 by default)
  long                         one job of 65536 steps
Per shape and pass:
  gpu_us     the call between two events on the instance's stream (table upload, four kernels)
  call_us    the whole call on the host clock (wait, table upload, launches, wait)
  nocrc_us   gpu_us of the same jobs with crc_width 0
  ns_per_step_of_a_wave   nocrc_us / steps of a job: for the long shape that is k_*_acs and k_*_trace of one wave, step by step
After warm-up the two passes are repeated by turns; the medians and the spread (min .. max) of gpu_us are reported.  The first and
the last job of a shape are compared bit for bit with the host statements.  One JSON line per shape and pass.

  python tools/soft_bench.py [--per 1024] [--reps 9] [--warmup 3] [--shapes jobs64,jobs1024,jobs4096,long]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.decode_bench import CRC, K, POLYS, crc16		# noqa: E402

SIGMA = 0.45


def frame(rng, steps):
    """one Gray QPSK symbol a step: info, CRC-16, six tail bits, encoded at rate 1/2 -> (noisy symbols float32 [steps][2], hard bytes)"""
    info = rng.integers(0, 2, steps - 16 - (K - 1))
    v = crc16(info)
    bits = np.concatenate([info, [(v >> (15 - i)) & 1 for i in range(16)], np.zeros(K - 1, np.int64)])
    u = np.concatenate([np.zeros(K - 1, np.int64), bits])
    streams = np.zeros((steps, 2), np.int64)
    for i, poly in enumerate(POLYS):
        for j in range(K):
            if (poly >> j) & 1:
                streams[:, i] ^= u[j:j + steps]
    label = 2 * streams[:, 0] + streams[:, 1]
    q = np.array([0, 1, 3, 2])[label]						# the value whose Gray label it is
    z = np.exp(2j * np.pi * q / 4) + SIGMA * (rng.standard_normal(steps) + 1j * rng.standard_normal(steps))
    k = np.floor(np.angle(z) / (2 * np.pi) * 4 + 0.5).astype(np.int64) & 3
    return np.stack([z.real, z.imag], 1).astype(np.float32), (k ^ (k >> 1)).astype(np.uint8)


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
    shapes = {"jobs64": (64, args.per), "jobs1024": (1024, args.per), "jobs4096": (4096, args.per), "long": (1, F.SOFT_MAX_STEPS)}

    for name in args.shapes.split(","):
        n_jobs, per = shapes[name]
        n = n_jobs * per
        rng = np.random.default_rng(1)
        kinds = [frame(rng, per) for i in range(min(n_jobs, 16))]
        iq = np.concatenate([kinds[i % len(kinds)][0] for i in range(n_jobs)])
        sym = np.concatenate([kinds[i % len(kinds)][1] for i in range(n_jobs)])
        d_iq, d_sym = torch.from_numpy(iq).cuda(), torch.from_numpy(sym).cuda()
        own = F.decode_owned(per - (K - 1))
        tables = {}
        for pass_, dtype in (("decode", F.DECODE_JOB_DTYPE), ("soft", F.SOFT_JOB_DTYPE)):
            jobs = np.zeros(n_jobs, dtype)
            jobs["offset"] = np.arange(n_jobs, dtype=np.int64) * per
            jobs["out_offset"] = np.arange(n_jobs, dtype=np.int64) * own
            jobs["n"], jobs["order"], jobs["flags"], jobs["k"], jobs["n_poly"], jobs["period"] = per, 4, 1, K, 2, 1
            jobs["polys"], jobs["punct"] = POLYS + (0,), (1, 1, 0)
            jobs["crc_width"], jobs["crc_poly"], jobs["crc_init"] = CRC[:3]
            if pass_ == "soft":
                jobs["flags"], jobs["scale"] = 3, 16.0
            plain = jobs.copy()
            plain["crc_width"], plain["crc_poly"], plain["crc_init"] = 0, 0, 0
            tables[pass_] = (jobs, plain)
        d_out = torch.empty(n_jobs * own, dtype=torch.uint8, device="cuda")
        d_rec = torch.empty(n_jobs * 64, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def call(pass_, table):
            fn, src = (f.L.fosphor_amd_decode, d_sym) if pass_ == "decode" else (f.L.fosphor_amd_soft, d_iq)
            t0 = time.perf_counter()
            e0.record(st)
            rv = fn(f.h, src.data_ptr(), n, table.ctypes.data, n_jobs, d_rec.data_ptr(), d_out.data_ptr(), n_jobs * own)
            e1.record(st)
            e1.synchronize()
            assert rv == 0, rv
            return (time.perf_counter() - t0) * 1e6, e0.elapsed_time(e1) * 1e3

        torch.cuda.synchronize()
        times = {(p, c): [] for p in tables for c in (0, 1)}
        for rep in range(args.warmup + args.reps):				# by turns: decode, soft, each with and without its CRC
            for p in ("decode", "soft"):
                for c in (1, 0):
                    tm = call(p, tables[p][c])
                    if rep >= args.warmup:
                        times[(p, c)].append(tm)
        for p, dtype, host, src in (("decode", F.DECODE_RECORD_DTYPE, F.decode_host, sym), ("soft", F.SOFT_RECORD_DTYPE, F.soft_host, iq)):
            jobs = tables[p][0]
            call(p, jobs)
            rec = d_rec.cpu().numpy().view(dtype)
            out = d_out.cpu().numpy()
            for i in (0, n_jobs - 1):						# the sanity check: the host's bits
                alone = jobs[i:i + 1].copy()
                alone["out_offset"] = 0
                want_rec, want = host(src, alone)
                at = int(jobs["out_offset"][i])
                assert rec[i].tobytes() == want_rec[0].tobytes() and out[at:at + len(want[0])].tobytes() == want[0].tobytes(), "not the host's bits"
            gpu = [tm[1] for tm in times[(p, 0)]]
            nocrc = float(np.median([tm[1] for tm in times[(p, 1)]]))
            stats = f.decode_stats() if p == "decode" else f.soft_stats()
            row = dict(shape=name, fn=p, n_jobs=n_jobs, steps=per, k=K, crc_width=16, call_us=round(float(np.median([tm[0] for tm in times[(p, 0)]])), 1),
                       gpu_us=round(float(np.median(gpu)), 1), gpu_us_min=round(min(gpu), 1), gpu_us_max=round(max(gpu), 1), nocrc_us=round(nocrc, 1),
                       ns_per_step_of_a_wave=round(1e3 * nocrc / per, 2), crc_failures=int((rec["status"] != 0).sum()), metric=int(rec["metric"][0]),
                       reps=args.reps, stats=stats, device=torch.cuda.get_device_name(0))
            print(json.dumps(row), flush=True)
        del d_iq, d_sym, d_out
    f.close()


if __name__ == "__main__":
    main()
