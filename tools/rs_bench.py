#!/usr/bin/env python3
"""Time fosphor_amd_rs on CCSDS frames in device memory that sit still.

Shapes: 64, 1024 and 4096 jobs of the `ccsds` shape: I = 5, RS(255,223), scrambled (DESCRAMBLE_IN), 1275 bytes a job.
Error loads:
  clean    no byte wrong: k_rs_fix is not launched
  random   1 % of the bytes wrong, at random
  t        every codeword at exactly t = 16 errors
Per shape and load:
  gpu_us    the call between two events on the instance's stream (table upload, up to four kernels, two read-backs of the state words)
  call_us   the whole call on the host clock (wait, table upload, launches, wait)
  host_us   fosphor_amd_rs_host over the same jobs on one core, once
After warm-up each is repeated; the median and the spread (min .. max) are reported.  The first and the last job of a shape are
compared bit for bit with fosphor_amd_rs_host.  One JSON line per shape and load.

  python tools/rs_bench.py [--reps 9] [--warmup 3] [--shapes 64,1024,4096] [--loads clean,random,t]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CODE, DEPTH, T = 255, 5, 16
FRAME = N_CODE * DEPTH
KINDS = 16							# different frames, repeated over the jobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="64,1024,4096")
    ap.add_argument("--loads", default="clean,random,t")
    args = ap.parse_args()

    import torch
    from _pkg import gr_fosphor_amd
    F = gr_fosphor_amd.Fosphor
    f = F(n_bins=128, wf_rows=16)
    st = torch.cuda.ExternalStream(f.stream)
    code = dict(flags=F.RS_FLAGS["descramble_in"], scr_width=8, scr_taps=0x95, scr_init=0xff, **F.RS_CCSDS)
    n_data = DEPTH * (N_CODE - code["n_roots"])
    own = F.rs_owned(n_data)

    def table(n_jobs):
        jobs = np.zeros(n_jobs, F.RS_JOB_DTYPE)
        jobs["offset"] = np.arange(n_jobs, dtype=np.int64) * FRAME
        jobs["out_offset"] = np.arange(n_jobs, dtype=np.int64) * own
        jobs["n_code"], jobs["depth"] = N_CODE, DEPTH
        for k, v in code.items():
            jobs[k] = v
        return jobs

    rng = np.random.default_rng(1)
    kinds = table(KINDS)
    data = rng.integers(0, 256, KINDS * own).astype(np.uint8)
    clean = F.rs_encode(data, kinds)

    def loaded(load):
        frames = clean.copy()
        if load == "random":
            at = rng.choice(len(frames), len(frames) // 100, replace=False)
            frames[at] ^= rng.integers(1, 256, len(at)).astype(np.uint8)
        elif load == "t":
            for k in range(KINDS):
                for c in range(DEPTH):
                    pos = rng.choice(N_CODE, T, replace=False)
                    frames[k * FRAME + pos * DEPTH + c] ^= rng.integers(1, 256, T).astype(np.uint8)
        return frames

    for load in args.loads.split(","):
        kinds_frames = loaded(load)
        for n_jobs in (int(s) for s in args.shapes.split(",")):
            jobs = table(n_jobs)
            frames = np.concatenate([kinds_frames.reshape(KINDS, FRAME)[i % KINDS] for i in range(n_jobs)])
            d_in = torch.from_numpy(frames).cuda()
            d_out = torch.empty(n_jobs * own, dtype=torch.uint8, device="cuda")
            d_rec = torch.empty(n_jobs * F.RS_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def run():
                t0 = time.perf_counter()
                e0.record(st)
                rv = f.L.fosphor_amd_rs(f.h, d_in.data_ptr(), len(frames), jobs.ctypes.data, n_jobs, d_rec.data_ptr(), d_out.data_ptr(), n_jobs * own)
                e1.record(st)
                e1.synchronize()
                assert rv == 0, rv
                return (time.perf_counter() - t0) * 1e6, e0.elapsed_time(e1) * 1e3

            torch.cuda.synchronize()
            before = f.rs_stats()
            times = [run() for rep in range(args.warmup + args.reps)][args.warmup:]
            after = f.rs_stats()
            rec = d_rec.cpu().numpy().view(F.RS_RECORD_DTYPE)
            out = d_out.cpu().numpy()
            t0 = time.perf_counter()
            host_rec, host_views = F.rs_host(frames, jobs)
            host_us = (time.perf_counter() - t0) * 1e6
            for i in (0, n_jobs - 1):					# the sanity check: the host's bytes
                at = int(jobs["out_offset"][i])
                assert rec[i].tobytes() == host_rec[i].tobytes() and out[at:at + n_data].tobytes() == host_views[i].tobytes(), "not the host's bytes"
                assert out[at:at + n_data].tobytes() == data[(i % KINDS) * own:(i % KINDS) * own + n_data].tobytes(), "not the planted data"
            assert not rec["status"].any(), rec[0]
            gpu, call = [tm[1] for tm in times], [tm[0] for tm in times]
            calls = after["calls"] - before["calls"]
            row = dict(load=load, n_jobs=n_jobs, codewords=n_jobs * DEPTH, bytes_in=len(frames), call_us=round(float(np.median(call)), 1),
                       gpu_us=round(float(np.median(gpu)), 1), gpu_us_min=round(min(gpu), 1), gpu_us_max=round(max(gpu), 1),
                       host_us=round(host_us, 1), host_over_gpu=round(host_us / float(np.median(gpu)), 1),
                       ns_per_codeword=round(1e3 * float(np.median(gpu)) / (n_jobs * DEPTH), 2),
                       corrected_symbols=int(rec["corrected_symbols"].sum()), clean=int(rec["n_clean"].sum()),
                       launches_per_call={k: (after[k] - before[k]) / calls for k in ("k_syn", "k_fix", "k_out", "k_rec")},
                       reps=args.reps, device=torch.cuda.get_device_name(0))
            print(json.dumps(row), flush=True)
            del d_in, d_out, d_rec
    f.close()


if __name__ == "__main__":
    main()
