#!/usr/bin/env python3
"""Time fosphor_amd_resample against the bytes it has to move and the arithmetic it has to do.

One call of --jobs jobs of --per samples each, back to back in one buffer of random float32 IQ in device memory, resampled by
--up / --down with a prototype of --branch taps a branch (fosphor_amd_resample_design); every job has its largest valid n_out and
the outputs lie back to back:
  gpu_ms   the call between two events on the instance's stream (table upload, one kernel)
  call_ms  the whole call on the host clock (wait, table upload, launch, wait)
After warm-up the call is repeated; the medians are reported.  There is no parent and no library routine to time beside it; the
yardsticks are what the pass cannot avoid:
  bytes      8 * (samples read once + outputs written) + 4 * taps: bytes_per_s = bytes / gpu_ms, hbm_share over HBM_PEAK
  fma        2 fp64 fused multiply-adds per output and branch tap: fma_per_s = 2 * macs / gpu_ms, fma_share over FP64_FMA_PEAK
  outputs_per_s
The first and the last job are compared bit for bit with fosphor_amd_resample_host.  --kernel-trace runs this script once more
under rocprofv3 --kernel-trace --stats, in a process of its own, and adds the kernel's average microseconds.  One JSON line.

  python tools/resample_bench.py --up 2 --down 3 --branch 16 [--jobs 4096] [--per 4096] [--reps 9] [--warmup 2] [--kernel-trace]
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

# fp64 vector peak in fused multiply-adds per second, as tools/correlate_bench.py takes it (AMD's public MI355X data sheet: 78.6
# TFLOPS FP64 vector), and the HBM3E peak of the same sheet, 8 TB/s
FP64_FMA_PEAK = 78.6e12 / 2.0
HBM_PEAK = 8.0e12


def kernel_trace(argv):
    """this script once more under rocprofv3, in a fresh process -> {kernel: average us}"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "resample", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__)] + [a for a in argv if a != "--kernel-trace"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode:
            return {"error": r.stdout[-400:]}
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    if "k_resample" in row.get("Name", ""):
                        name = "k_resample_tile" if "tile" in row["Name"] else "k_resample_direct"
                        out[name] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2))
        return out or {"error": "no k_resample rows in the kernel stats"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--up", type=int, required=True)
    ap.add_argument("--down", type=int, required=True)
    ap.add_argument("--branch", type=int, default=16)
    ap.add_argument("--jobs", type=int, default=4096)
    ap.add_argument("--per", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-trace", action="store_true")
    args = ap.parse_args()

    import torch
    from _pkg import gr_fosphor_amd
    F = gr_fosphor_amd.Fosphor
    f = F(n_bins=128, wf_rows=16)
    st = torch.cuda.ExternalStream(f.stream)
    U, D, Q, n_jobs, per = args.up, args.down, args.branch, args.jobs, args.per
    taps = F.resample_design(U, D, Q)
    n_out = F.resample_n_out(per, U, D, len(taps))
    n = n_jobs * per
    torch.manual_seed(1)
    d_iq = torch.randn((n, 2), device="cuda")
    d_taps = torch.from_numpy(taps).cuda()
    jobs = np.zeros(n_jobs, F.RESAMPLE_JOB_DTYPE)
    jobs["offset"] = np.arange(n_jobs, dtype=np.int64) * per
    jobs["out_offset"] = np.arange(n_jobs, dtype=np.int64) * n_out
    jobs["n"], jobs["n_out"], jobs["up"], jobs["down"], jobs["n_taps"] = per, n_out, U, D, len(taps)
    cap = n_jobs * n_out
    d_out = torch.empty((max(cap, 1), 2), dtype=torch.float32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def resample():
        t0 = time.perf_counter()
        e0.record(st)
        rv = f.L.fosphor_amd_resample(f.h, d_iq.data_ptr(), n, jobs.ctypes.data, n_jobs, d_taps.data_ptr(), len(taps), d_out.data_ptr(), cap)
        e1.record(st)
        e1.synchronize()
        assert rv == 0, rv
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    torch.cuda.synchronize()
    times = [resample() for rep in range(args.warmup + args.reps)][args.warmup:]
    iq = d_iq.cpu().numpy()
    out = d_out.cpu().numpy()
    for j in (jobs[0], jobs[-1]):						# the sanity check: the host's bits
        alone = j.copy()
        alone["out_offset"] = 0
        want = F.resample_host(iq, alone, taps)[0]
        assert out[int(j["out_offset"]):int(j["out_offset"]) + n_out].tobytes() == want.tobytes(), "not the host's bits"
    call_ms, gpu_ms = (float(np.median([tm[i] for tm in times])) for i in (0, 1))
    macs = n_jobs * n_out * Q
    nbytes = 8 * (n + cap) + 4 * len(taps)
    sec = gpu_ms * 1e-3
    row = dict(up=U, down=D, branch=Q, n_taps=len(taps), form=F.resample_form(U, D, len(taps)), n_jobs=n_jobs, n=per, n_out=n_out, macs=macs,
               bytes=nbytes, call_ms=round(call_ms, 4), gpu_ms=round(gpu_ms, 4), outputs_per_s=round(cap / sec, 0),
               fma_per_s=round(2 * macs / sec, 0), fma_share=round(2 * macs / sec / FP64_FMA_PEAK, 4), bytes_per_s=round(nbytes / sec, 0),
               hbm_share=round(nbytes / sec / HBM_PEAK, 4), reps=args.reps, stats=f.resample_stats(), device=torch.cuda.get_device_name(0))
    f.close()
    if args.kernel_trace:
        row["kernel_us"] = kernel_trace(sys.argv[1:])
        k = row["kernel_us"].get("k_resample_" + row["form"])
        if k:
            ksec = k["avg_us"] * 1e-6
            row["kernel_fma_share"] = round(2 * macs / ksec / FP64_FMA_PEAK, 4)
            row["kernel_hbm_share"] = round(nbytes / ksec / HBM_PEAK, 4)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
