#!/usr/bin/env python3
"""Times views (include/fosphor_amd_view.h) against the only other way to a picture, the two full-resolution
fosphor_amd_colorize calls, on the same instance, and writes profiles/r08_view.md.  Needs the GPU; nothing here falls back.

Three steps, each a run of this file:
    view_bench.py time   --json T.json        host clock around the synchronising calls: warm-up, then `--reps` repetitions per
                                              figure and round with the configurations alternating, `--rounds` rounds
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python view_bench.py trace --json S.json
                                              a few calls of every configuration in a known order, for the kernel times
    view_bench.py report --json T.json --trace-json S.json --trace-dir DIR --out profiles/r08_view.md

Geometries: C5 (fft_len_log 16, 512 bins, 1024 waterfall rows, fp16 IQ) and C3 (fft_len_log 13, 512 bins, 1024 rows).
Configurations: the baseline; full-span views 1920 and 3840 pixels wide with both RGBA pictures (every waterfall row, PEAK); a 1 %
zoom (N / 100 columns around the centre, 1920 wide).  Bytes are computed from the shapes.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_READ = 8.0e12			# HBM3E read peak, bytes / s
GEOMETRIES = [("C5", dict(fft_len_log=16, n_bins=512, wf_rows=1024, max_spectra=64, iq_fp16=True)),
              ("C3", dict(fft_len_log=13, n_bins=512, wf_rows=1024, max_spectra=64))]
CONFIGS = ["baseline", "view1920", "view3840", "zoom1pct"]


def window(n, cfg):
    """(first_bin, n_cols, width) of a view configuration"""
    if cfg == "zoom1pct":
        cols = n // 100
        return n // 2 - cols // 2, cols, 1920
    return 0, n, int(cfg[4:])


def shape_bytes(n, bins, rows, cfg):
    """per kernel of one call, in launch order: (kernel, bytes read, bytes written)"""
    if cfg == "baseline":
        return [("k_colorize", 4 * rows * n, 4 * rows * n), ("k_colorize", 4 * bins * n, 4 * bins * n)]
    _, cols, width = window(n, cfg)
    return [("k_view", 4 * rows * cols, 4 * rows * width), ("k_view", 4 * bins * cols, 4 * bins * width)]


class Bench:
    def __init__(self, kw):
        import numpy as np
        import torch
        from _pkg import gr_fosphor_amd as amd
        self.amd, self.torch = amd, torch
        f = self.f = amd.Fosphor(**kw)
        n = self.n = f.n
        rng = np.random.default_rng(8)
        for call in range(3):			# noise and a tone: the timing does not depend on the values
            x = (rng.standard_normal((64 * n, 2)) * 0.05).astype(np.float32)
            x[:, 0] += 0.1 * np.cos(2 * np.pi * 0.11 * np.arange(64 * n)).astype(np.float32)
            d_x = torch.from_numpy(x.astype(np.float16) if f.iq_fp16 else x).cuda()
            assert f.process_device(d_x, 1, 64) == 0 and f.finish() >= 0
        # outputs allocated once: the timed calls are the library's alone
        self.full = [torch.empty((f.wf_rows, n), dtype=torch.int32, device="cuda"),
                     torch.empty((f.n_bins, n), dtype=torch.int32, device="cuda")]
        self.small = [torch.empty((f.wf_rows, 3840), dtype=torch.int32, device="cuda"),
                      torch.empty((f.n_bins, 3840), dtype=torch.int32, device="cuda")]

    def call(self, cfg):
        f, L = self.f, self.f.L
        if cfg == "baseline":
            rv = L.fosphor_amd_colorize(f.h, 0, None, 0, 1, 0.0, 0.0, f.wf_rows, self.full[0].data_ptr())
            rv |= L.fosphor_amd_colorize(f.h, 1, None, 0, 1, 0.0, 0.0, f.n_bins, self.full[1].data_ptr())
        else:
            first, cols, width = window(self.n, cfg)
            v = self.amd._lib.View(first, cols, width, f.wf_rows, f.wf_rows, 0)
            o = self.amd._lib.ViewOut()
            o.d_waterfall_rgba, o.d_histogram_rgba = self.small[0].data_ptr(), self.small[1].data_ptr()
            o.wf_color.use_defaults = o.histo_color.use_defaults = 1
            rv = L.fosphor_amd_view(f.h, C.byref(v), C.byref(o))
        if rv:
            raise RuntimeError("%s -> %d" % (cfg, rv))

    def timed(self, cfg):
        t0 = time.perf_counter()
        self.call(cfg)				# returns when the picture is complete
        return time.perf_counter() - t0


def mode_time(args):
    res = {}
    for name, kw in GEOMETRIES:
        b = Bench(kw)
        for cfg in CONFIGS * 5:
            b.call(cfg)
        rounds = []
        for _ in range(args.rounds):
            t = {cfg: [] for cfg in CONFIGS}
            for _ in range(args.reps):		# alternating: every configuration sees the same moments of the machine
                for cfg in CONFIGS:
                    t[cfg].append(b.timed(cfg))
            rounds.append({cfg: statistics.median(v) for cfg, v in t.items()})
        res[name] = dict(n=b.n, bins=b.f.n_bins, rows=b.f.wf_rows, reps=args.reps, rounds=rounds)
        print(name, json.dumps(rounds))
        b.f.close()
    json.dump(res, open(args.json, "w"), indent=1)


def mode_trace(args):
    seq = []
    for name, kw in GEOMETRIES:
        b = Bench(kw)
        for cfg in CONFIGS:
            for _ in range(args.trace_calls):
                b.call(cfg)
                seq.append((name, cfg))
        b.f.close()
    json.dump(seq, open(args.json, "w"))


def kernel_rows(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    rows = []
    for fn in files:
        for r in csv.DictReader(open(fn)):
            name = r["Kernel_Name"]
            kind = "k_view" if "k_view" in name else "k_colorize" if "k_colorize" in name else None
            if kind:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind))
    rows.sort()
    return rows


def mode_report(args):
    tim = json.load(open(args.json))
    seq = json.load(open(args.trace_json))
    rows = kernel_rows(args.trace_dir)
    if len(rows) != 2 * len(seq):
        raise SystemExit("trace has %d picture kernels, the sequence %d calls of 2" % (len(rows), len(seq)))
    kern = {}					# (geometry, config, kernel index in the call) -> [ns]
    for i, (name, cfg) in enumerate(seq):
        for j in range(2):
            start, end, kind = rows[2 * i + j]
            geo = tim[name]
            if kind != shape_bytes(geo["n"], geo["bins"], geo["rows"], cfg)[j][0]:
                raise SystemExit("trace order: call %d kernel %d is %s" % (i, j, kind))
            kern.setdefault((name, cfg, j), []).append(end - start)

    out = ["# Views against full-resolution colouring (MI355X)", "",
           "Written by `tools/view_bench.py`.  Call times: host clock around the synchronising calls, %d repetitions per figure and"
           % tim["C5"]["reps"],
           "round after a warm-up, the four configurations alternating, %d rounds; the figure is the median of the round medians and"
           % len(tim["C5"]["rounds"]),
           "the spread is the largest minus the smallest round median.  Kernel times: a separate `rocprofv3 --kernel-trace --stats`",
           "run, median of %d launches.  Bytes are computed from the shapes; the share is bytes read / time over the 8 TB/s read peak."
           % len(next(iter(kern.values()))),
           "The baseline is what the library offered before views: `fosphor_amd_colorize` of the waterfall and of the histogram at",
           "full resolution.  Views: both RGBA pictures, every waterfall row, PEAK; the 1 % zoom is N / 100 columns around the centre.", ""]
    verdicts = []
    for name, _ in GEOMETRIES:
        geo = tim[name]
        n, bins, rws = geo["n"], geo["bins"], geo["rows"]
        med = {c: statistics.median(r[c] for r in geo["rounds"]) for c in CONFIGS}
        spread = {c: max(r[c] for r in geo["rounds"]) - min(r[c] for r in geo["rounds"]) for c in CONFIGS}
        out += ["## %s: N = %d, %d bins, %d waterfall rows" % (name, n, bins, rws), "",
                "| configuration | call time, us | spread, us | bytes read, MiB | bytes written, MiB |", "|---|---|---|---|---|"]
        for c in CONFIGS:
            sb = shape_bytes(n, bins, rws, c)
            out.append("| %s | %.1f | %.1f | %.2f | %.2f |" % (c, med[c] * 1e6, spread[c] * 1e6, sum(x[1] for x in sb) / 2 ** 20,
                                                               sum(x[2] for x in sb) / 2 ** 20))
        out += ["", "| configuration | kernel | kernel time, us | bytes read, MiB | read rate, TB/s | share of 8 TB/s |", "|---|---|---|---|---|---|"]
        for c in CONFIGS:
            for j, (kind, rd, _) in enumerate(shape_bytes(n, bins, rws, c)):
                t = statistics.median(kern[(name, c, j)]) * 1e-9
                out.append("| %s | %s (%s) | %.1f | %.2f | %.2f | %.1f %% |" % (c, kind, ("waterfall", "histogram")[j], t * 1e6, rd / 2 ** 20,
                                                                          rd / t / 1e12, 100.0 * rd / t / PEAK_READ))
        out.append("")
        for c in ("view1920", "view3840"):
            ok = med[c] <= med["baseline"]
            verdicts.append("- %s %s: %.1f us against the baseline's %.1f us (spreads %.1f / %.1f us): %s"
                            % (name, c, med[c] * 1e6, med["baseline"] * 1e6, spread[c] * 1e6, spread["baseline"] * 1e6,
                               "no longer than the baseline" if ok else "LONGER than the baseline: FAILS"))
        gain, sp = med["view1920"] - med["zoom1pct"], max(spread["view1920"], spread["zoom1pct"])
        verdicts.append("- %s 1 %% zoom: %.1f us, %.1f us less than the full span at the same width (spread %.1f us): %s"
                        % (name, med["zoom1pct"] * 1e6, gain * 1e6, sp * 1e6,
                           "less by more than the spread" if gain >= sp and gain > 0 else "NOT less by the spread: FAILS"))
    out += ["## Acceptance", ""] + verdicts + [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(out))
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["time", "trace", "report"])
    ap.add_argument("--json", required=True)
    ap.add_argument("--trace-json")
    ap.add_argument("--trace-dir")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_view.md"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-calls", type=int, default=9)
    args = ap.parse_args()
    {"time": mode_time, "trace": mode_trace, "report": mode_report}[args.mode](args)


if __name__ == "__main__":
    main()
