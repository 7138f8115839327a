#!/usr/bin/env python3
"""Time fosphor_amd_correlate against the arithmetic it has to do, next to a plain torch expression for the same rho.

One call of 4096 jobs of 4096 samples each (16 Mi samples, 128 MiB of float32 IQ in device memory) against one template of T
samples, with one trace mode:
  correlate  fosphor_amd_correlate between two events on the instance's stream (table upload, the tile kernel, the combine kernel),
             and the whole call on the host clock (wait, table upload, launches, wait)
  torch      the same rho by a torch expression in float64 on the same device, between two events on torch's stream:
               w = x.unfold(1, T, 1); c = (w * t.conj()).sum(-1); E = (w.abs() ** 2).sum(-1); rho = |c|^2 / (E Et)
             over the first --torch-jobs jobs only (the unfolded products of all 4096 would not fit), scaled to the call
After warm-up the two are repeated alternately; the medians are reported.

Arithmetic: the kernel issues, per lag and template sample, 4 fp64 multiply-adds for c and 2 for E, and per lane and template
sample 2 for Et, shared by the lane's 4 lags: 6.5 per complex multiply-add.
  fma_per_s   6.5 * macs / gpu_ms
  peak_share  fma_per_s over the fp64 vector peak, FP64_FMA_PEAK below

The torch rho is also the sanity check: the peak lags must be equal, and the peak rho and every rho of a trace must agree to
1e-6 relative.  The device's rho is a float32 (6e-8 relative) and torch's sums are not pinned, so the two are not bit-identical.
--kernel-trace runs this script once more under rocprofv3 --kernel-trace --stats, in a process of its own, and adds the kernels'
average microseconds.  One JSON line.

  python tools/correlate_bench.py --tpl 128 --trace rho [--reps 9] [--warmup 2] [--kernel-trace]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_JOBS, PER = 4096, 4096
# fp64 vector peak of the MI355X in fused multiply-adds per second.  The microarchitecture notes this project works from list the
# FP32 vector peak, 157.3 TFLOPS at 256 CUs and 2.4 GHz (128 FLOP per clock and CU), and no fp64 vector figure; AMD's public
# MI355X data sheet lists FP64 vector at half of it, 78.6 TFLOPS = 39.3e12 multiply-adds per second.
FP64_FMA_PEAK = 78.6e12 / 2.0
FMA_PER_MAC = 6.5


def kernel_trace(argv):
    """this script once more under rocprofv3, in a fresh process -> {kernel: average us}"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "corr", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__)] + [a for a in argv if a != "--kernel-trace"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode:
            return {"error": r.stdout[-400:]}
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    if "k_correlate" in row.get("Name", ""):
                        name = "k_correlate_tile" if "tile" in row["Name"] else "k_correlate_combine"
                        out[name] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2))
        return out or {"error": "no k_correlate rows in the kernel stats"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tpl", type=int, required=True)
    ap.add_argument("--trace", choices=["none", "rho"], default="none")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-jobs", type=int, default=64)
    ap.add_argument("--kernel-trace", action="store_true")
    args = ap.parse_args()

    import torch
    from _pkg import gr_fosphor_amd
    F = gr_fosphor_amd.Fosphor
    f = F(n_bins=128, wf_rows=16)
    st = torch.cuda.ExternalStream(f.stream)
    T = args.tpl
    n = N_JOBS * PER
    torch.manual_seed(1)
    d_iq = torch.randn((N_JOBS, PER, 2), device="cuda")
    d_tpl = torch.randn((T, 2), device="cuda")
    x, t = torch.view_as_complex(d_iq), torch.view_as_complex(d_tpl)
    trace = F.CORRELATE_TRACES[args.trace]
    n_lags = PER - T + 1
    n_out = F.correlate_n_out(trace, PER, T)
    jobs = np.zeros(N_JOBS, F.CORRELATE_JOB_DTYPE)
    jobs["offset"] = np.arange(N_JOBS, dtype=np.int64) * PER
    jobs["out_offset"] = np.arange(N_JOBS, dtype=np.int64) * n_out
    jobs["n"], jobs["tpl_len"], jobs["trace"], jobs["threshold"] = PER, T, trace, 4.0 / T
    d_out = torch.empty(max(N_JOBS * n_out, 1), dtype=torch.float32, device="cuda")
    d_rec = torch.empty(N_JOBS * F.CORRELATE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0e, t1e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def correlate():
        t0 = time.perf_counter()
        e0.record(st)
        rv = f.L.fosphor_amd_correlate(f.h, d_iq.data_ptr(), n, d_tpl.data_ptr(), T, jobs.ctypes.data, N_JOBS, d_rec.data_ptr(),
                                       d_out.data_ptr(), N_JOBS * n_out)
        e1.record(st)
        e1.synchronize()
        assert rv == 0, rv
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    tj = min(args.torch_jobs, N_JOBS)
    xd, td = x[:tj].to(torch.complex128), t.to(torch.complex128)
    Et = (td.abs() ** 2).sum()

    def yardstick():
        t0e.record()
        w = xd.unfold(1, T, 1)
        c = (w * td.conj()).sum(-1)
        E = (w.real ** 2 + w.imag ** 2).sum(-1)
        rho = (c.real ** 2 + c.imag ** 2) / (E * Et)
        t1e.record()
        t1e.synchronize()
        return t0e.elapsed_time(t1e) * (N_JOBS / tj), rho

    torch.cuda.synchronize()
    times, torch_ms = [], []
    for rep in range(args.warmup + args.reps):				# alternating: both see the same state of the machine
        tm = correlate()
        ms, rho = yardstick()
        if rep >= args.warmup:
            times.append(tm)
            torch_ms.append(ms)
    records = d_rec.cpu().numpy().view(F.CORRELATE_RECORD_DTYPE)
    peak = rho.max(1)
    worst = float(((torch.from_numpy(records["peak_rho"][:tj].astype(np.float64)).cuda() - peak.values).abs() / peak.values).max())
    assert worst <= 1e-6 and np.array_equal(records["peak_lag"][:tj], peak.indices.cpu().numpy()), worst
    if trace:
        d = (d_out.view(N_JOBS, n_out)[:tj].double() - rho).abs() / (1e-3 + rho)
        worst = max(worst, float(d.max()))
        assert worst <= 1e-6, worst
    call_ms, gpu_ms = (float(np.median([tm[i] for tm in times])) for i in (0, 1))
    macs = N_JOBS * n_lags * T
    fma = FMA_PER_MAC * macs
    row = dict(tpl=T, trace=args.trace, n_jobs=N_JOBS, n=PER, n_lags=n_lags, macs=macs, call_ms=round(call_ms, 4),
               gpu_ms=round(gpu_ms, 4), fma_per_s=round(fma / (gpu_ms * 1e-3), 0), peak_share=round(fma / (gpu_ms * 1e-3) / FP64_FMA_PEAK, 4),
               torch_ms_scaled=round(float(np.median(torch_ms)), 3), torch_jobs=tj, worst_diff_to_torch=worst, reps=args.reps,
               stats=f.correlate_stats(), device=torch.cuda.get_device_name(0))
    f.close()
    if args.kernel_trace:
        row["kernel_us"] = kernel_trace(sys.argv[1:])
        tile = row["kernel_us"].get("k_correlate_tile")
        if tile:
            row["kernel_peak_share"] = round(fma / (tile["avg_us"] * 1e-6) / FP64_FMA_PEAK, 4)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
