#!/usr/bin/env python3
"""IQ formats side by side: sc16 (interleaved int16) against fp32 -- against fp16 at N = 65536 -- on the measured shapes.

    python3 tools/iq_format_bench.py [--rounds 3] [--steps 10] [--shapes C2,C3,C5,host,pinned]

One process; per shape the formats alternate for --rounds rounds (each round and format: a fresh instance -- one alive at a time --,
one warm-up step, then --steps timed steps);
which format goes first alternates from round to round, and the best round is reported.  One JSON line per (shape, format): GS/s of complex samples of the input stream (the unexpanded stream
where overlap_cc is fused into the read) and the IQ bytes per sample.  The sc16 input is int16 noise; the reference format gets the same
values widened (x * 2^-15, exact; at N = 65536 |x| <= 2048, where fp16 is exact too).  Every instance goes through the same calls, so the
hit counts after the timed runs must be identical: the tool checks the digests and fails otherwise.

Shapes: C2 (N 1024, 256 bins, process_device of 256 x 1024, relaxed input ordering as bench.py), C3 (N 8192, 512 bins, 28 x 4096,
overlap 2), C5 (N 65536, 512 bins, one 1024-spectrum frame), host (fosphor_process, calls of 1 Mi samples) and pinned
(upload_pinned / process_uploaded, calls of 1 Mi samples, two in flight)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "C2": dict(log2n=10, n_bins=256, n_batches=256, batch=1024, overlap=1, ref="fp32"),
    "C3": dict(log2n=13, n_bins=512, n_batches=28, batch=4096, overlap=2, ref="fp32"),
    "C5": dict(log2n=16, n_bins=512, n_batches=1, batch=1024, overlap=1, ref="fp16"),
    "host": dict(log2n=10, n_bins=128, n_batches=1, batch=1024, overlap=1, ref="fp32"),
    "pinned": dict(log2n=10, n_bins=128, n_batches=1, batch=1024, overlap=1, ref="fp32"),
}
BYTES = {"fp32": 8, "fp16": 4, "sc16": 4}


def make(amd, sh, fmt):
    total = sh["n_batches"] * sh["batch"]
    return amd.Fosphor(fft_len_log=sh["log2n"], n_bins=sh["n_bins"], wf_rows=1024, max_spectra=total,
                       max_batches=max(8, sh["n_batches"]), iq_format=fmt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shapes", default="C2,C3,C5,host,pinned")
    args = ap.parse_args()
    import torch
    from _pkg import gr_fosphor_amd as amd
    amd.load()
    torch.cuda.set_device(0)
    ok = True
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        n = 1 << sh["log2n"]
        total = sh["n_batches"] * sh["batch"]
        hop = n // sh["overlap"]
        n_samples = (total - 1) * hop + n
        g = torch.Generator(device="cuda").manual_seed(7)
        lim = 2048 if sh["ref"] == "fp16" else 32767
        x16 = torch.randint(-lim, lim + 1, (2 * n_samples,), dtype=torch.int16, device="cuda", generator=g)
        xr = x16.float() * 2.0 ** -15
        if sh["ref"] == "fp16":
            xr = xr.half()
        data = {"sc16": x16, sh["ref"]: xr}
        host = name in ("host", "pinned")
        if host:
            data = {k: (v.cpu().pin_memory() if name == "pinned" else v.cpu().numpy()) for k, v in data.items()}
        inst = {}

        def step(fmt):
            f, d = inst[fmt], data[fmt]
            if name == "host":
                rv = f.process(d)
            elif name == "pinned":
                rv = f.L.fosphor_amd_upload_pinned(f.h, d.data_ptr(), n_samples)
                if f.L.fosphor_amd_pending_uploads(f.h) == 2:
                    rv = rv or f.L.fosphor_amd_process_uploaded(f.h, None)
            elif sh["overlap"] > 1:
                rv = f.process_device_overlap(d, sh["n_batches"], sh["batch"], sh["overlap"])
            else:
                rv = f.process_device(d, sh["n_batches"], sh["batch"])
            if rv:
                raise RuntimeError("%s %s: %d" % (name, fmt, rv))

        def drain(fmt):
            f = inst[fmt]
            while name == "pinned" and f.L.fosphor_amd_pending_uploads(f.h):
                f.L.fosphor_amd_process_uploaded(f.h, None)
            f.finish()

        best = {fmt: 0.0 for fmt in data}
        dig = {}
        for rnd in range(args.rounds):
            for fmt in (list(data) if rnd % 2 == 0 else list(data)[::-1]):	# the order alternates from round to round
                # one instance alive at a time: two instances' streams share the process's hardware queues, and which of them
                # collide depends on the order they were made in (measured: the instance made first ran 14 % slower at C5)
                inst[fmt] = make(amd, sh, fmt)
                if not host:
                    inst[fmt].L.fosphor_amd_set_input_ordering(inst[fmt].h, 0)
                step(fmt)
                drain(fmt)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(fmt)
                drain(fmt)
                dt = time.perf_counter() - t0
                best[fmt] = max(best[fmt], args.steps * n_samples / dt / 1e9)
                dig[fmt] = hashlib.sha256(inst[fmt].hitcount.tobytes()).hexdigest()[:16]
                inst.pop(fmt).close()
        same = len(set(dig.values())) == 1
        ok = ok and same
        for fmt in data:
            print(json.dumps({"shape": name, "format": fmt, "GSps": round(best[fmt], 2), "iq_bytes_per_sample": BYTES[fmt],
                              "fft_len": n, "n_bins": sh["n_bins"], "batches": sh["n_batches"], "batch": sh["batch"],
                              "overlap": sh["overlap"], "samples_per_step": n_samples, "rounds": args.rounds, "steps": args.steps,
                              "hitcount_digest": dig[fmt], "digests_equal": same}), flush=True)
        del data, x16, xr
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
