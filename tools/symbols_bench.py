#!/usr/bin/env python3
"""Time fosphor_amd_symbols against the bytes it has to move and against the same rules in torch.

Three shapes over random float32 IQ in device memory whose envelope swings at the symbol rate, every job under ESTIMATE:
  jobs     --jobs jobs of --per samples each at sps 4, back to back            (4096 x 4096 by default)
  long4    one job of 2^--long-log samples at sps 4                            (2^24 by default)
  long32   the same samples at sps 32: k_sym_pick reads y[g - 1 .. g + 2] straight from memory
Per shape:
  gpu_ms   the call between two events on the instance's stream (table upload, up to four kernels, the read-back of the counts)
  call_ms  the whole call on the host clock (wait, table upload, launches, wait)
  copy_ms  a device-to-device copy of the bytes the pass cannot avoid, 8 per input sample read and 8 per symbol written, between two
           events on torch's stream: the floor of a pass that reads its input once
  torch_ms rules 1 to 5 in float64 torch on the same device (|y|^2 folded by a reshaped sum, the line by a matrix product, the angle
           by torch.angle, four gathers and a weighted sum), on the host clock around a synchronize: an outside figure, not a parent
After warm-up each is repeated; the medians and the spread (min .. max) of gpu_ms are reported with the ratios gpu_ms / copy_ms
and gpu_ms / torch_ms.  The first and the last job of a shape are compared bit for bit with fosphor_amd_symbols_host.  One JSON
line per shape.

  python tools/symbols_bench.py [--jobs 4096] [--per 4096] [--long-log 24] [--reps 9] [--warmup 3] [--shapes jobs,long4,long32]
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
    ap.add_argument("--jobs", type=int, default=4096)
    ap.add_argument("--per", type=int, default=4096)
    ap.add_argument("--long-log", type=int, default=24)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="jobs,long4,long32")
    args = ap.parse_args()

    import torch
    from _pkg import gr_fosphor_amd
    F = gr_fosphor_amd.Fosphor
    f = F(n_bins=128, wf_rows=16)
    st = torch.cuda.ExternalStream(f.stream)
    shapes = {"jobs": (args.jobs, args.per, 4), "long4": (1, 1 << args.long_log, 4), "long32": (1, 1 << args.long_log, 32)}

    for name in args.shapes.split(","):
        n_jobs, per, sps = shapes[name]
        n = n_jobs * per
        torch.manual_seed(1)
        env = 1.0 + 0.5 * torch.cos(2.0 * np.pi * (torch.arange(n, device="cuda") % sps - 1.3) / sps)
        d_iq = (torch.randn((n, 2), device="cuda") * 0.1 + 1.0) * env[:, None].float()
        jobs = np.zeros(n_jobs, F.SYMBOLS_JOB_DTYPE)
        max_out = F.symbols_max_out(per, sps)
        jobs["offset"] = np.arange(n_jobs, dtype=np.int64) * per
        jobs["out_offset"] = np.arange(n_jobs, dtype=np.int64) * max_out
        jobs["n"], jobs["sps"] = per, sps
        cap = n_jobs * max_out
        d_out = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        d_rec = torch.empty(n_jobs * F.SYMBOLS_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def symbols():
            t0 = time.perf_counter()
            e0.record(st)
            rv = f.L.fosphor_amd_symbols(f.h, d_iq.data_ptr(), n, jobs.ctypes.data, n_jobs, d_rec.data_ptr(), d_out.data_ptr(), cap)
            e1.record(st)
            e1.synchronize()
            assert rv == 0, rv
            return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

        src = torch.empty(n + cap, dtype=torch.complex64, device="cuda")
        dst = torch.empty_like(src)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def copy():
            c0.record()
            dst.copy_(src)
            c1.record()
            c1.synchronize()
            return c0.elapsed_time(c1)

        tw = torch.from_numpy(F.symbols_twiddles(sps)).cuda()

        def torch_symbols():
            """the outside figure: rules 1 to 5 in float64, unordered sums, 256 jobs (or 2^22 samples of the long job's fold) a step"""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            R = per // sps
            z = d_iq.view(n_jobs, per, 2)
            A = torch.zeros((n_jobs, sps), dtype=torch.float64, device="cuda")
            step = max(1, (1 << 22) // per)
            for a in range(0, n_jobs, step):
                for lo in range(0, R * sps, sps << 20):
                    y = z[a:a + step, lo:min(lo + (sps << 20), R * sps)].double()
                    A[a:a + step] += (y * y).sum(-1).view(y.shape[0], -1, sps).sum(1)
            X = A.to(torch.complex128) @ tw
            e = torch.remainder(torch.angle(X.conj()) / (2.0 * np.pi), 1.0)
            base = e * sps
            i0 = torch.floor(base)
            mu = (base - i0)[:, None, None]
            first = torch.where(i0 >= 1, i0, torch.full_like(i0, sps)).long()
            n_sym = (per - 3 - sps) // sps + 1					# the symbols every job has
            c = (-(mu * (mu - 1) * (mu - 2)) / 6, ((mu + 1) * (mu - 1) * (mu - 2)) / 2, -((mu + 1) * mu * (mu - 2)) / 2, ((mu + 1) * mu * (mu - 1)) / 6)
            out = []
            for a in range(0, n_jobs, step):
                for lo in range(0, n_sym, 1 << 20):
                    g = first[a:a + step, None] + torch.arange(lo, min(lo + (1 << 20), n_sym), device="cuda")[None, :] * sps
                    rows = z[a:a + step]
                    s = sum(c[k][a:a + step] * torch.gather(rows, 1, (g + (k - 1))[:, :, None].expand(-1, -1, 2)).double() for k in range(4))
                    out.append(s.float())
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        torch.cuda.synchronize()
        times = [symbols() for rep in range(args.warmup + args.reps)][args.warmup:]
        copies = [copy() for rep in range(args.warmup + args.reps)][args.warmup:]
        more = [symbols() for rep in range(args.reps)]				# again behind the copies: the spread over alternating runs
        rec = d_rec.cpu().numpy().view(F.SYMBOLS_RECORD_DTYPE)
        out = d_out.cpu().numpy()
        iq = d_iq.cpu().numpy()
        for i in (0, n_jobs - 1):						# the sanity check: the host's bits
            alone = jobs[i:i + 1].copy()
            alone["out_offset"] = 0
            want_rec, want = F.symbols_host(iq, alone)
            at = int(jobs["out_offset"][i])
            got = out[at:at + int(rec["n_sym"][i])]
            assert rec[i].tobytes() == want_rec[0].tobytes() and got.tobytes() == want[0].tobytes(), "not the host's bits"
        torch_ms = float(np.median([torch_symbols() for rep in range(1 + 3)][1:]))
        gpu = [tm[1] for tm in times + more]
        call_ms, gpu_ms, copy_ms = float(np.median([tm[0] for tm in times + more])), float(np.median(gpu)), float(np.median(copies))
        symbols_written = int(rec["n_sym"].sum())
        nbytes = 8 * n + 8 * symbols_written
        row = dict(shape=name, n_jobs=n_jobs, n=per, sps=sps, symbols=symbols_written, bytes=nbytes, call_ms=round(call_ms, 4),
                   gpu_ms=round(gpu_ms, 4), gpu_ms_min=round(min(gpu), 4), gpu_ms_max=round(max(gpu), 4), copy_ms=round(copy_ms, 4),
                   torch_ms=round(torch_ms, 4), over_copy=round(gpu_ms / copy_ms, 3), over_torch=round(gpu_ms / torch_ms, 4),
                   bytes_per_s=round(nbytes / (gpu_ms * 1e-3), 0), tau=[round(float(rec["tau"][0]), 5), round(float(rec["tau"][-1]), 5)],
                   reps=2 * args.reps, stats=f.symbols_stats(), device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        del d_iq, d_out, src, dst
    f.close()


if __name__ == "__main__":
    main()
