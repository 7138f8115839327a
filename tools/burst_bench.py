#!/usr/bin/env python3
"""Times fosphor_amd_bursts (include/fosphor_amd_burst.h) against fosphor_amd_mask_scan over the same full window, on the same
instance, the two alternating; writes profiles/r11_burst.md.  Needs the GPU; nothing here falls back.

    burst_bench.py --json T.json [--out profiles/r11_burst.md]

Geometries: (1024 points, 1024 waterfall rows) and (65536 points, 1024 rows, fp16 IQ).  Fields, planted straight into the ring:
"sparse", 36 rectangular bursts on a quiet floor, and "dense", uniform noise against a threshold that leaves 0.3 of the cells on
(max_runs at its limit, 1 << 20; at 65536 points the full window holds some 14 million runs, which no max_runs admits, so the full
window is timed as the overflow it is and a 4096-column window beside it as the dense case that fits).  "bursts, count only" is the
same call with max_runs = 1: it ends after the count pass and the scan, which splits the call time into its two halves.
The mask scan: the same window and rows, an upper limit equal to the threshold, row records and a 1024-entry event list, no
channels.  Call times are a host clock around the synchronising calls: a warm-up, then `--reps` repetitions per figure and round,
`--rounds` rounds.  Kernel times need a rocprofv3 run of their own and are marked "not measured" here.
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMETRIES = [("N1024", dict(fft_len_log=10, n_bins=128, wf_rows=1024, max_spectra=1024)),
              ("N65536", dict(fft_len_log=16, n_bins=512, wf_rows=1024, max_spectra=64, iq_fp16=True))]
CONFIGS = ["mask_scan", "bursts", "bursts_count_only"]
THR = 0.7


def fields(rows, n):
    """(name, ys [rows][n] by j and shifted column, window) for each timed case"""
    import numpy as np
    rng = np.random.default_rng(11)
    sparse = (0.5 * rng.random((rows, n))).astype(np.float32)
    for k in range(36):				# 36 bursts of 8 .. 40 rows by 6 .. 30 columns
        j, i = int(rng.integers(0, rows - 40)), int(rng.integers(0, n - 30))
        sparse[j:j + int(rng.integers(8, 41)), i:i + int(rng.integers(6, 31))] = 2.0
    dense = rng.random((rows, n)).astype(np.float32)
    out = [("sparse", sparse, (0, n)), ("dense", dense, (0, n))]
    if n > 4096:
        out.append(("dense, 4096 columns", dense, (n // 2 - 2048, 4096)))
    return out


class Bench:
    def __init__(self, kw):
        import torch
        from _pkg import gr_fosphor_amd as amd
        self.amd, self.torch = amd, torch
        f = self.f = amd.Fosphor(**kw)
        self.n = f.n
        assert f.finish() >= 0
        self.upper = torch.full((self.n,), THR, dtype=torch.float32, device="cuda")
        self.d_res = torch.empty(8, dtype=torch.int32, device="cuda")
        self.d_rows = torch.empty(f.wf_rows * 6, dtype=torch.int32, device="cuda")
        self.d_ev = torch.empty(1024, dtype=torch.int32, device="cuda")
        self.d_out = torch.empty(1024 * 10, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def plant(self, ys, window):
        import numpy as np
        from gr_fosphor_amd.dist import wrap_device_array
        f, torch = self.f, self.torch
        b = f.buffers(False)
        wf = wrap_device_array(b.d_waterfall, (f.wf_rows, self.n), torch.float32)
        mem = np.empty((f.wf_rows, self.n), np.float32)
        mem[(b.waterfall_pos - 1 - np.arange(f.wf_rows)) % f.wf_rows] = ys[:, np.arange(self.n) ^ (self.n // 2)]
        wf.copy_(torch.from_numpy(mem))
        torch.cuda.synchronize()
        self.window = window
        self.mask_cfg = self.amd._lib.MaskCfg(window[0], window[1], f.wf_rows, 1, 0)
        mk = lambda max_runs: self.amd._lib.BurstCfg(window[0], window[1], f.wf_rows, THR, 0, 0, 1, 1, max_runs)
        self.burst_cfg = {"bursts": mk(1 << 20), "bursts_count_only": mk(1)}

    def call(self, cfg):
        f, L = self.f, self.f.L
        if cfg == "mask_scan":
            rv = L.fosphor_amd_mask_scan(f.h, C.byref(self.mask_cfg), self.upper.data_ptr(), None, self.d_res.data_ptr(),
                                         self.d_rows.data_ptr(), self.d_ev.data_ptr(), 1024, None)
        else:
            rv = L.fosphor_amd_bursts(f.h, C.byref(self.burst_cfg[cfg]), None, self.d_res.data_ptr(), self.d_out.data_ptr(), 1024)
        if rv:
            raise RuntimeError("%s -> %d" % (cfg, rv))

    def result(self):
        self.call("bursts")
        return dict(zip(("n_runs", "n_components", "n_found", "n_written", "overflow"), self.d_res.cpu().numpy()[:5].tolist()))

    def timed(self, cfg):
        t0 = time.perf_counter()
        self.call(cfg)				# returns when the outputs are complete
        return time.perf_counter() - t0


def kernel_resources():
    """registers / LDS / scratch of every kernel of fosphor_burst.hip, from the compiler"""
    src = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_burst.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-x", "hip", "--cuda-device-only",
                        "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    found, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k_burst_[a-z]+", m.group(1))
            cur = None if not k else k.group(0) + ("<true>" if "ILb1E" in m.group(1) else "<false>" if "ILb0E" in m.group(1) else "")
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            found.setdefault(cur, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    return found


def report(res, out_path):
    first = next(iter(res["cases"].values()))
    out = ["# Bursts (connected regions of the waterfall) against the mask scan over the same bytes (MI355X)", "",
           "Written by `tools/burst_bench.py`.  Call times: host clock around the synchronising calls, %d repetitions per figure and"
           % first["reps"],
           "round after a warm-up, the calls alternating, %d rounds; the figure is the median of the round medians and the spread"
           % len(first["rounds"]),
           "is the largest minus the smallest round median.  A call time holds every launch of the call and its waits: for the bursts",
           "that is the count pass, the per-row join, the scan, the host's read of the run count, and then the init, write, link,",
           "reduce and emit kernels.  \"count only\" is the same call with max_runs = 1, which ends after the host's read.",
           "Bytes are computed from the shapes: rows x columns x 4.  Kernel times (`rocprofv3 --kernel-trace --stats`): not measured.",
           "The mask scan: the same window and rows, an upper limit equal to the threshold, records and a 1024-entry event list.", ""]
    for name, case in res["cases"].items():
        med = {c: statistics.median(r[c] for r in case["rounds"]) for c in CONFIGS}
        spread = {c: max(r[c] for r in case["rounds"]) - min(r[c] for r in case["rounds"]) for c in CONFIGS}
        rd = 4 * case["n_cols"] * case["rows"]
        r = case["result"]
        out += ["## %s" % name, "",
                "N = %d, window %d columns, %d rows, %.2f MiB; n_runs %d, n_components %d, n_found %d, overflow %d." %
                (case["n"], case["n_cols"], case["rows"], rd / 2 ** 20, r["n_runs"], r["n_components"], r["n_found"], r["overflow"]), "",
                "| call | call time, us | spread, us | bytes / call time, TB/s |", "|---|---|---|---|"]
        for c in CONFIGS:
            out.append("| %s | %.1f | %.1f | %.3f |" % (c.replace("_", " "), med[c] * 1e6, spread[c] * 1e6, rd / med[c] / 1e12))
        out += ["", "bursts / mask scan = %.2f; count only / mask scan = %.2f; what follows the count takes %.1f us." %
                (med["bursts"] / med["mask_scan"], med["bursts_count_only"] / med["mask_scan"],
                 (med["bursts"] - med["bursts_count_only"]) * 1e6), ""]
    out += ["## Compiler resources (gfx950, -O3)", "", "| kernel | VGPRs | SGPRs | LDS, bytes | scratch, bytes / lane | waves / SIMD |",
            "|---|---|---|---|---|---|"]
    for k, v in sorted(res["resources"].items()):
        out.append("| %s | %d | %d | %d | %d | %d |" % (k, v.get("VGPRs", -1), v.get("TotalSGPRs", -1), v.get("LDS", -1),
                                                   v.get("ScratchSize", -1), v.get("Occupancy", -1)))
    out += ["", "## Reading", ""] + res.get("reading", ["not written"]) + [""]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(out))
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_burst.md"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--report-only", action="store_true", help="write the report from an existing --json (its \"reading\" list included)")
    args = ap.parse_args()
    if args.report_only:
        return report(json.load(open(args.json)), args.out)
    res = dict(cases={}, resources=kernel_resources())
    for gname, kw in GEOMETRIES:
        b = Bench(kw)
        for fname, ys, window in fields(b.f.wf_rows, b.n):
            b.plant(ys, window)
            for cfg in CONFIGS * 3:
                b.call(cfg)
            rounds = []
            for _ in range(args.rounds):
                t = {cfg: [] for cfg in CONFIGS}
                for _ in range(args.reps):		# alternating: every call sees the same moments of the machine
                    for cfg in CONFIGS:
                        t[cfg].append(b.timed(cfg))
                rounds.append({cfg: statistics.median(v) for cfg, v in t.items()})
            name = "%s, %s" % (gname, fname)
            res["cases"][name] = dict(n=b.n, rows=b.f.wf_rows, n_cols=window[1], reps=args.reps, rounds=rounds, result=b.result())
            print(name, json.dumps(res["cases"][name]["result"]), json.dumps(rounds), flush=True)
        b.f.close()
    json.dump(res, open(args.json, "w"), indent=1)
    report(res, args.out)


if __name__ == "__main__":
    main()
