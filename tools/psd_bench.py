#!/usr/bin/env python3
"""Time fosphor_amd_psd against the bytes it has to move and the arithmetic it has to do.

One call of --jobs jobs of --per samples each, back to back in one buffer of random float32 IQ in device memory, transformed in
segments of 2^--log samples, --hop apart (L / 2 by default: 50 % overlap), under a Hann window, every job with its trace; the traces
lie back to back:
  gpu_ms   the call between two events on the instance's stream (table upload, the tile kernel, the combine kernel)
  call_ms  the whole call on the host clock (wait, table upload, launches, wait)
After warm-up the call is repeated; the medians are reported.  There is no parent to time beside it; the yardsticks are what the
pass cannot avoid:
  bytes      8 per sample read once, 8 L per tile written and read again, 4 L per trace, 64 per record: bytes_per_s, hbm_share
  flops      10 fp64 operations per butterfly, L / 2 log2 L butterflies per segment, plus 2 per sample for the window and 3 per bin
             for |X|^2 and the sum: flops_per_s, fp64_share over FP64_PEAK
  torch_ms   torch.fft.fft in complex128 over the same windowed segments, |X|^2 and the mean: an outside figure, not a parent
The first and the last job are compared bit for bit with fosphor_amd_psd_host.  --kernel-trace runs this script once more under
rocprofv3 --kernel-trace --stats, in a process of its own, and adds the kernels' average microseconds.  One JSON line.

  python tools/psd_bench.py --log 8 [--hop 128] [--jobs 4096] [--per 4096] [--reps 9] [--warmup 2] [--kernel-trace]
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

# fp64 vector peak and HBM3E peak as tools/resample_bench.py takes them (AMD's public MI355X data sheet)
FP64_PEAK = 78.6e12
HBM_PEAK = 8.0e12


def kernel_trace(argv):
    """this script once more under rocprofv3, in a fresh process -> {kernel: calls, average us}"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "psd", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__)] + [a for a in argv if a != "--kernel-trace"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if r.returncode:
            return {"error": r.stdout[-400:]}
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    for name in ("k_psd_group", "k_psd_wave", "k_psd_combine"):
                        if name in row.get("Name", ""):
                            out[name] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2))
        return out or {"error": "no k_psd rows in the kernel stats"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, required=True)
    ap.add_argument("--hop", type=int, default=0)
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
    log, n_jobs, per = args.log, args.jobs, args.per
    L = 1 << log
    hop = args.hop or L // 2
    n_seg = F.psd_n_seg(per, log, hop)
    n = n_jobs * per
    torch.manual_seed(1)
    d_iq = torch.randn((n, 2), device="cuda")
    win = F.psd_window("hann", log)
    d_win = torch.from_numpy(win).cuda()
    jobs = np.zeros(n_jobs, F.PSD_JOB_DTYPE)
    jobs["offset"] = np.arange(n_jobs, dtype=np.int64) * per
    jobs["out_offset"] = np.arange(n_jobs, dtype=np.int64) * L
    jobs["n"], jobs["fft_len_log"], jobs["hop"], jobs["trace"], jobs["obw_fraction"], jobs["xdb_ratio"] = per, log, hop, 1, 0.99, 0.01
    cap = n_jobs * L
    d_out = torch.empty(cap, dtype=torch.float32, device="cuda")
    d_rec = torch.empty(n_jobs * 64, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def psd():
        t0 = time.perf_counter()
        e0.record(st)
        rv = f.L.fosphor_amd_psd(f.h, d_iq.data_ptr(), n, d_win.data_ptr(), L, jobs.ctypes.data, n_jobs, d_rec.data_ptr(), d_out.data_ptr(), cap)
        e1.record(st)
        e1.synchronize()
        assert rv == 0, rv
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    def torch_psd():
        """the outside figure: the same segments through torch.fft.fft in complex128, one job batch at a time"""
        z = d_iq.view(torch.complex64).reshape(n_jobs, per)
        w = d_win.double()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a in range(0, n_jobs, 256):
            rows = z[a:a + 256]
            seg = rows.as_strided((rows.shape[0], n_seg, L), (per, hop, 1)).to(torch.complex128) * w
            X = torch.fft.fft(seg, dim=2)
            (X.real * X.real + X.imag * X.imag).mean(1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    torch.cuda.synchronize()
    times = [psd() for rep in range(args.warmup + args.reps)][args.warmup:]
    iq = d_iq.cpu().numpy()
    out = d_out.cpu().numpy()
    rec = d_rec.cpu().numpy().view(F.PSD_RECORD_DTYPE)
    for i in (0, n_jobs - 1):							# the sanity check: the host's bits
        alone = jobs[i:i + 1].copy()
        alone["out_offset"] = 0
        want_rec, want = F.psd_host(iq, alone, win)
        assert out[i * L:(i + 1) * L].tobytes() == want[0].tobytes() and rec[i].tobytes() == want_rec[0].tobytes(), "not the host's bits"
    torch_ms = float(np.median([torch_psd() for rep in range(1 + 3)][1:]))
    call_ms, gpu_ms = (float(np.median([tm[i] for tm in times])) for i in (0, 1))
    tiles = n_jobs * -(-n_seg // F.PSD_TILE)
    segments = n_jobs * n_seg
    flops = segments * (10 * (L // 2) * log + 2 * L + 3 * L)
    nbytes = 8 * n + 2 * 8 * L * tiles + 4 * cap + 64 * n_jobs
    sec = gpu_ms * 1e-3
    row = dict(fft_len=L, hop=hop, form="group" if log > 7 else "wave", n_jobs=n_jobs, n=per, n_seg=n_seg, segments=segments, tiles=tiles,
               flops=flops, bytes=nbytes, call_ms=round(call_ms, 4), gpu_ms=round(gpu_ms, 4), torch_ms=round(torch_ms, 4),
               segments_per_s=round(segments / sec, 0), flops_per_s=round(flops / sec, 0), fp64_share=round(flops / sec / FP64_PEAK, 4),
               bytes_per_s=round(nbytes / sec, 0), hbm_share=round(nbytes / sec / HBM_PEAK, 4), reps=args.reps, stats=f.psd_stats(),
               device=torch.cuda.get_device_name(0))
    f.close()
    if args.kernel_trace:
        row["kernel_us"] = kernel_trace(sys.argv[1:])
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
