#!/usr/bin/env python3
"""What the compact wire formats (include/fosphor_amd_wire.h) put on the wire for one frame, and what their kernels cost.

Default shape: the bench's C5 frame -- N = 65536, fp16 IQ, 512 bins, 1024 white-noise spectra (sigma 0.05, default power range)
cut into 8 time shards of 128 -- on 8 emulated ranks of ONE device; torch stands in for the collectives between the stages, as
in tests/test_gpu_wire.py.  Prints a markdown report: per rank, live rows and wire bytes from fosphor_amd_wire_stats and the
durations of k_wire_mask / k_wire_pack / k_wire_unpack from hipEvents (fosphor_amd_wire_kernel_times), for both forms.
The collectives themselves are not measured: nothing here runs between real devices."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=16)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--total", type=int, default=1024)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from _pkg import gr_fosphor_amd as amd
    from gr_fosphor_amd.dist import wrap_device_array

    n, per = 1 << a.log2n, a.total // a.world
    fp16 = a.log2n == 16
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(a.total * n * 2, device="cuda", generator=g) * 0.05
    x = x.half() if fp16 else x
    ranks = [amd.Fosphor(fft_len_log=a.log2n, n_bins=a.bins, wf_rows=64, max_spectra=per, max_batches=2,
                         iq_format="fp16" if fp16 else "fp32") for _ in range(a.world)]
    for f in ranks:
        f.profile(True)
    cells = a.bins * n
    print("# Compact wire: bytes per frame and kernel times\n")
    print("N = %d, %s IQ, %d bins, %d white-noise spectra (sigma 0.05), %d emulated shards of %d on one %s."
          % (n, "fp16" if fp16 else "fp32", a.bins, a.total, a.world, per, torch.cuda.get_device_name(0)))
    print("The uint32 wire is %.1f MiB per rank and frame.  Collectives emulated by torch copies: never run between real devices.\n"
          % (4 * cells / 2 ** 20))
    for form in ("sparse16", "packed16"):
        times = []
        for rep in range(a.reps):
            for r, f in enumerate(ranks):
                assert f.accumulate_device(x[r * per * n * 2:(r + 1) * per * n * 2], per, r * per, a.total) == 0
            torch.cuda.synchronize()
            hc = [wrap_device_array(f.partials().d_hc, (cells,), torch.int32) for f in ranks]
            if form == "sparse16":
                for r, f in enumerate(ranks):
                    assert f.wire_mask(a.total, a.world, r) == 0
                torch.cuda.synchronize()
                infos = [f.wire_info() for f in ranks]
                mv = [wrap_device_array(i.d_masks, (a.world, i.mask_words), torch.int32) for i in infos]
                own = torch.stack([mv[r][r] for r in range(a.world)])
                for v in mv:
                    v.copy_(own)
                torch.cuda.synchronize()
            packs = []
            for f in ranks:
                rv, w = f.wire_pack(a.total, form, a.world)
                assert rv == 0
                packs.append(w)
            torch.cuda.synchronize()
            words = [wrap_device_array(w.d_words, (w.n_words,), torch.int32) for w in packs]
            wsum = words[0].clone()
            for w in words[1:]:
                wsum += w
            for w in words:
                w.copy_(wsum)
            total = hc[0].clone()
            for h in hc[1:]:
                total += h
            torch.cuda.synchronize()
            for f in ranks:
                assert f.wire_unpack() == 0
            torch.cuda.synchronize()
            assert all(torch.equal(h, total) for h in hc), "the unpacked slots are not the uint32 sums"
            assert int(total.sum(dtype=torch.int64)) == a.total * n
            times.append([f.wire_kernel_times() for f in ranks])
            for f in ranks:
                f.finish()
                f.kernel_times()
        st = [f.wire_stats() for f in ranks]
        taken = {1: "packed16", 2: "sparse16"}[packs[0].form]
        print("## asked for %s, went out as %s\n" % (form, taken))
        print("| rank | live rows | of rows | wire bytes | MiB | of the uint32 wire | mask us | pack us | unpack us |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r, s in enumerate(st):
            t = times[-1][r]
            print("| %d | %d | %.4f | %d | %.2f | %.4f | %s | %.1f | %.1f |"
                  % (r, s["live_rows"], max(s["live_rows"], 0) / (cells // 64), s["wire_bytes"], s["wire_bytes"] / 2 ** 20,
                     s["wire_bytes"] / (4 * cells), "%.1f" % (1e3 * t["mask"]) if form == "sparse16" else "-", 1e3 * t["pack"], 1e3 * t["unpack"]))
        med = {k: float(np.median([1e3 * t[k] for rep in times[1:] or times for t in rep])) for k in ("mask", "pack", "unpack")}
        print("\nmedian over ranks and repetitions after the first: mask %s us, pack %.1f us, unpack %.1f us\n"
              % ("%.1f" % med["mask"] if form == "sparse16" else "-", med["pack"], med["unpack"]))
    for f in ranks:
        f.close()


if __name__ == "__main__":
    main()
