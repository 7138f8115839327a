#!/usr/bin/env python3
"""Times the frequency-mask scan (include/fosphor_amd_mask.h) and, beside it, the fosphor_amd_view PEAK pass over the same window
reduced to one pixel row 64 wide, which reads the same bytes, on the same instance; writes profiles/r10_mask.md.  Needs the GPU;
nothing here falls back.

    mask_bench.py --json T.json [--out profiles/r10_mask.md]

Geometries: (1024 points, 1024 waterfall rows) and (65536 points, 1024 rows, fp16 IQ).  The scan: the full window, every row, both
limits, 8 channels inside the window, rows and a 1024-entry event list wanted.  Call times are a host clock around the synchronising
calls: a warm-up, then `--reps` repetitions per figure and round with the two calls alternating, `--rounds` rounds.  Bytes are
computed from the shapes.  Kernel times need a rocprofv3 run of their own and are marked "not measured" here.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_READ = 8.0e12			# HBM3E read peak, bytes / s
GEOMETRIES = [("N1024", dict(fft_len_log=10, n_bins=128, wf_rows=1024, max_spectra=1024)),
              ("N65536", dict(fft_len_log=16, n_bins=512, wf_rows=1024, max_spectra=64, iq_fp16=True))]
CONFIGS = ["scan", "view_peak"]


class Bench:
    def __init__(self, kw):
        import numpy as np
        import torch
        from _pkg import gr_fosphor_amd as amd
        self.amd, self.torch = amd, torch
        f = self.f = amd.Fosphor(**kw)
        n = self.n = f.n
        rng = np.random.default_rng(10)
        per = min(f.max_spectra, 64)
        for call in range(2):			# noise and a tone: the timing does not depend on the values
            x = (rng.standard_normal((per * n, 2)) * 0.05).astype(np.float32)
            x[:, 0] += 0.1 * np.cos(2 * np.pi * 0.11 * np.arange(per * n)).astype(np.float32)
            d_x = torch.from_numpy(x.astype(np.float16) if f.iq_fp16 else x).cuda()
            assert f.process_device(d_x, 1, per) == 0 and f.finish() >= 0
        # limits that a few cells of every row break, and outputs allocated once: the timed calls are the library's alone
        self.upper = torch.full((n,), 1.0, dtype=torch.float32, device="cuda")
        self.lower = torch.full((n,), -3.0, dtype=torch.float32, device="cuda")
        self.cfg = amd._lib.MaskCfg(0, n, f.wf_rows, 1, 8)
        for c in range(8):
            self.cfg.channels[c].first, self.cfg.channels[c].last = c * (n // 8), (c + 1) * (n // 8) - 1
        self.d_res = torch.empty(4, dtype=torch.int32, device="cuda")
        self.d_rows = torch.empty(f.wf_rows * 6, dtype=torch.int32, device="cuda")
        self.d_ev = torch.empty(1024, dtype=torch.int32, device="cuda")
        self.d_pow = torch.empty((8, f.wf_rows), dtype=torch.float32, device="cuda")
        self.d_pix = torch.empty(64, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

    def call(self, cfg):
        f, L = self.f, self.f.L
        if cfg == "scan":
            rv = L.fosphor_amd_mask_scan(f.h, C.byref(self.cfg), self.upper.data_ptr(), self.lower.data_ptr(), self.d_res.data_ptr(),
                                         self.d_rows.data_ptr(), self.d_ev.data_ptr(), 1024, self.d_pow.data_ptr())
        else:
            v = self.amd._lib.View(0, self.n, 64, f.wf_rows, 1, 0)
            o = self.amd._lib.ViewOut()
            o.d_waterfall = self.d_pix.data_ptr()
            rv = L.fosphor_amd_view(f.h, C.byref(v), C.byref(o))
        if rv:
            raise RuntimeError("%s -> %d" % (cfg, rv))

    def timed(self, cfg):
        t0 = time.perf_counter()
        self.call(cfg)				# returns when the outputs are complete
        return time.perf_counter() - t0


def report(res, out_path):
    out = ["# Frequency-mask scan against the view's PEAK pass over the same bytes (MI355X)", "",
           "Written by `tools/mask_bench.py`.  Call times: host clock around the synchronising calls, %d repetitions per figure and"
           % next(iter(res.values()))["reps"],
           "round after a warm-up, the two calls alternating, %d rounds; the figure is the median of the round medians and the spread"
           % len(next(iter(res.values()))["rounds"]),
           "is the largest minus the smallest round median.  A call time holds the launches, the wait and, for the scan, its combine",
           "and event-list kernels.  Bytes are computed from the shapes: rows x columns x 4; bytes / time is over the call time, so it",
           "understates the scan kernel's own rate.  Kernel times (`rocprofv3 --kernel-trace --stats`): not measured.",
           "The scan: full window, every row, both limits, 8 channels inside the window, records and a 1024-entry event list.",
           "The view: PEAK over the same window and rows, reduced to one pixel row 64 wide.", ""]
    for name, geo in res.items():
        n, rws = geo["n"], geo["rows"]
        rd = 4 * n * rws
        med = {c: statistics.median(r[c] for r in geo["rounds"]) for c in CONFIGS}
        spread = {c: max(r[c] for r in geo["rounds"]) - min(r[c] for r in geo["rounds"]) for c in CONFIGS}
        out += ["## %s: N = %d, %d waterfall rows, form %s" % (name, n, rws, geo["form"]), "",
                "| call | call time, us | spread, us | bytes read, MiB | bytes / call time, TB/s | share of 8 TB/s |", "|---|---|---|---|---|---|"]
        for c in CONFIGS:
            out.append("| %s | %.1f | %.1f | %.2f | %.3f | %.1f %% |" % (c, med[c] * 1e6, spread[c] * 1e6, rd / 2 ** 20,
                                                                   rd / med[c] / 1e12, 100.0 * rd / med[c] / PEAK_READ))
        d = med["scan"] - med["view_peak"]
        out += ["", "The scan takes %.1f us %s than the view pass (spreads %.1f / %.1f us)."
                % (abs(d) * 1e6, "longer" if d > 0 else "less", spread["scan"] * 1e6, spread["view_peak"] * 1e6), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(out))
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_mask.md"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--report-only", action="store_true", help="write the report from an existing --json")
    args = ap.parse_args()
    if args.report_only:
        return report(json.load(open(args.json)), args.out)
    res = {}
    for name, kw in GEOMETRIES:
        b = Bench(kw)
        for cfg in CONFIGS * 5:
            b.call(cfg)
        before = b.f.mask_stats()
        rounds = []
        for _ in range(args.rounds):
            t = {cfg: [] for cfg in CONFIGS}
            for _ in range(args.reps):		# alternating: both calls see the same moments of the machine
                for cfg in CONFIGS:
                    t[cfg].append(b.timed(cfg))
            rounds.append({cfg: statistics.median(v) for cfg, v in t.items()})
        after = b.f.mask_stats()
        form = "SHARED" if after["form_shared"] > before["form_shared"] else "ROWS"
        res[name] = dict(n=b.n, rows=b.f.wf_rows, reps=args.reps, rounds=rounds, form=form)
        print(name, form, json.dumps(rounds))
        b.f.close()
    json.dump(res, open(args.json, "w"), indent=1)
    report(res, args.out)


if __name__ == "__main__":
    main()
