"""The emulated exchange of a time-sharded display frame, and the table of shard shapes the suite runs through it.

A frame of `total` spectra is cut into time shards (t_offset, n_local); every "rank" -- an instance of its own on the one GPU --
accumulates its shard from its part of the UNEXPANDED stream, the partial arrays are combined the way the all-reduce would (sum,
sum, max; torch stands in for the collective) and every rank merges.  The state of every rank must then be the state of ONE
display launch over the whole frame, which is what the oracle computes from the materialised (overlap_cc-expanded) frame.

CASES is data: tests/test_shard_cases_cpu.py checks it without a GPU (tiling, capacity, memory budget, stream lengths, and that the
512-bin inputs populate both bin-index planes); tests/test_gpu_shard_matrix.py runs it.
"""
import os

import numpy as np

from oracle_lib import Oracle, gaussian_iq, add_tone
from test_gpu_parity import assert_close, assert_hist_close, overlap_cc_reference
from test_gpu_iq_sc16 import sc16_iq, widen

# environment knobs a case may set; every one of them is cleared before a case's instances are made
KNOBS = ("FOSPHOR_AMD_SUB_LOG2", "FOSPHOR_AMD_FRAME_GROUP", "FOSPHOR_AMD_OVERLAP", "FOSPHOR_AMD_NO_SUM16", "FOSPHOR_AMD_TILE",
         "FOSPHOR_AMD_ALT", "FOSPHOR_AMD_K1_STREAMS")

DEVICE_BUDGET = 4 << 30		# bytes a case may need on the device ...
HOST_BUDGET = 4 << 30		# ... and on the host (stream, the oracle's expanded copy and its FFT output)

# Inputs.  At 512 bins the 9th bit of the bin index travels in a plane of its own (N = 8192) or in 9-bit packing (N = 65536): with
# the default power range (0 dB, 10 dB/div) Gaussian noise of sigma 0.05 leaves 0.05 % of the hits in bins >= 256, so that plane
# would carry next to nothing.  The ranges below were chosen on the CPU from the oracle's counts (fraction of hits in bins >= 256):
#   N = 8192  fp32, sigma 0.05 + tone 0.05:            (-40 dB, 5 dB/div) -> 0.69
#   N = 8192  sc16, sigma 3000 + tone 8000 (of 32768): (-32 dB, 5 dB/div) -> 0.50
#   N = 65536 fp16, sigma 0.05 + tone 0.05:            (-46 dB, 5 dB/div) -> 0.47
# tests/test_shard_cases_cpu.py asserts >= 1 % on either side for every such case.
_FP32 = {"sigma": 0.05, "amp": 0.05, "freq": 0.0313}
_SC16 = {"sigma": 3000.0, "amp": 8000.0, "freq": 0.123}

# launches: per rank (FFT pieces of accumulate, k2c chunk sums, k2b chunk reduces) of ONE frame (fosphor_amd_launch_stats deltas)
CASES = {
    # gcd chunks of 16 (1040, 3024) and 32 (2080) with the 32-bit reduce, a 2 x 1024 sum16 shard at an offset that is no multiple
    # of 1024, the first stored row (7168) in the middle of the last shard (local 1056), three ranks that store no row
    "a": dict(log2n=10, fmt="fp32", n_bins=256, wf_rows=1024, total=8192, overlap=1, frames=1,
              shards=[(0, 1040), (1040, 3024), (4064, 2048), (6112, 2080)], env={}, power=(0, 10), seed=7001, twin=False,
              launches=[(1, 0, 1), (1, 0, 1), (1, 1, 0), (1, 0, 1)]),
    # sub-launched shards with overlap: 4 pieces of 2 chunks (one count work-group per 2 chunks), first row (15360) at chunk 7 of
    # shard 1 = the second chunk of its last piece; two frames back to back
    "b": dict(log2n=10, fmt="fp32", n_bins=256, wf_rows=1024, total=16384, overlap=2, frames=2,
              shards=[(0, 8192), (8192, 8192)], env={"FOSPHOR_AMD_SUB_LOG2": "21", "FOSPHOR_AMD_FRAME_GROUP": "2"},
              power=(0, 10), seed=7002, twin=False, launches=[(4, 1, 0), (4, 1, 0)]),
    # the same pieces from 4-byte samples; first row (16128) in the middle of a chunk (local 7936)
    "c": dict(log2n=10, fmt="sc16", n_bins=256, wf_rows=256, total=16384, overlap=2, frames=1,
              shards=[(0, 8192), (8192, 8192)], env={"FOSPHOR_AMD_SUB_LOG2": "21", "FOSPHOR_AMD_FRAME_GROUP": "2"},
              power=(0, 10), seed=7003, twin=True, launches=[(4, 1, 0), (4, 1, 0)]),
    # N = 8192, one launch per shard; the second frame starts at ring position 512
    "d": dict(log2n=13, fmt="fp32", n_bins=512, wf_rows=1024, total=512, overlap=2, frames=2,
              shards=[(0, 256), (256, 256)], env={}, power=(-40, 5), seed=7004, twin=False,
              launches=[(1, 0, 0), (1, 0, 0)]),
    # N = 8192: a 48-spectrum shard (tiles of 8), a 1040-spectrum shard in chunks of 16 with the 32-bit reduce, the first row
    # (1024) in the middle of it (local 976) and off any tile of 64
    "e": dict(log2n=13, fmt="fp32", n_bins=512, wf_rows=1024, total=2048, overlap=4, frames=1,
              shards=[(0, 48), (48, 1040), (1088, 960)], env={}, power=(-40, 5), seed=7005, twin=False,
              launches=[(1, 0, 0), (1, 0, 1), (1, 0, 0)]),
    # N = 8192 sub-launched with overlap: 2 pieces of 2 chunks per shard; two frames
    "f": dict(log2n=13, fmt="fp32", n_bins=512, wf_rows=256, total=8192, overlap=2, frames=2,
              shards=[(0, 4096), (4096, 4096)], env={"FOSPHOR_AMD_SUB_LOG2": "24"}, power=(-40, 5), seed=7006, twin=False,
              launches=[(2, 1, 0), (2, 1, 0)]),
    "g": dict(log2n=13, fmt="sc16", n_bins=512, wf_rows=256, total=8192, overlap=2, frames=1,
              shards=[(0, 4096), (4096, 4096)], env={"FOSPHOR_AMD_SUB_LOG2": "24"}, power=(-32, 5), seed=7007, twin=True,
              launches=[(2, 1, 0), (2, 1, 0)]),
    # N = 65536 with overlap, unequal shards
    "h": dict(log2n=16, fmt="fp16", n_bins=512, wf_rows=64, total=64, overlap=2, frames=1,
              shards=[(0, 16), (16, 48)], env={}, power=(-46, 5), seed=7008, twin=False,
              launches=[(1, 0, 0), (1, 0, 0)]),
    # sub-launched pieces with the two-stream pipeline off (the count stream is the main stream)
    "i": dict(log2n=10, fmt="fp32", n_bins=256, wf_rows=1024, total=8192, overlap=1, frames=1,
              shards=[(0, 4096), (4096, 4096)], env={"FOSPHOR_AMD_SUB_LOG2": "21", "FOSPHOR_AMD_OVERLAP": "0"},
              power=(0, 10), seed=7009, twin=False, launches=[(2, 1, 0), (2, 1, 0)]),
    # Bin counts other than 128, 256 and 512 (BIN_COUNT_CASES below), two ranks each, small frames.
    # 16 bins, the minimum: the count kernel's row bitmask is half a word, its LDS histogram less than one pass of the work-group
    "j": dict(log2n=10, fmt="fp32", n_bins=16, wf_rows=64, total=64, overlap=1, frames=2,
              shards=[(0, 16), (16, 48)], env={}, power=(0, 20), seed=7010, twin=False, launches=[(1, 0, 0), (1, 0, 0)]),
    # N = 8192 at 48 bins (no multiple of 32; the plane of 9th bits is all zero, and still read and stored) ...
    "k": dict(log2n=13, fmt="fp32", n_bins=48, wf_rows=64, total=64, overlap=2, frames=1,
              shards=[(0, 16), (16, 48)], env={}, power=(0, 20), seed=7011, twin=False, launches=[(1, 0, 0), (1, 0, 0)]),
    # ... and at 272 (the 9th bit set in the last 16 rows only)
    "l": dict(log2n=13, fmt="fp32", n_bins=272, wf_rows=64, total=64, overlap=1, frames=1,
              shards=[(0, 48), (48, 16)], env={}, power=(-53, 10), seed=7012, twin=False, launches=[(1, 0, 0), (1, 0, 0)]),
    # N = 65536 at 496 bins, the largest count below 512: 9-bit packing
    "m": dict(log2n=16, fmt="fp16", n_bins=496, wf_rows=64, total=32, overlap=1, frames=1,
              shards=[(0, 16), (16, 16)], env={}, power=(-21, 10), seed=7013, twin=False, launches=[(1, 0, 0), (1, 0, 0)]),
}

# The cases above that are there for their bin count.  Their ranges were chosen on the CPU from the oracle's counts so that
# (tests/test_bin_counts_cpu.py asserts both) above 256 bins either side of row 256 holds at least 1 % of the hits, and the rows
# of 64 cells that hold a hit are strictly between 1 % and 50 % of all rows: tests/test_gpu_bin_counts.py sends these frames
# through the compact exchange in both forms, and the sparse form falls back to the packed one above one half.
#   "j" (0 dB, 20 dB/div):   0.33 / 0.32 of the rows live (frame 0 / 1)
#   "k" (0 dB, 20 dB/div):   0.26
#   "l" (-53 dB, 10 dB/div): 0.36, 0.23 of the hits in rows >= 256
#   "m" (-21 dB, 10 dB/div): 0.31, 0.34 of the hits in rows >= 256
BIN_COUNT_CASES = ("j", "k", "l", "m")

SAMPLE_BYTES = {"fp32": 8, "fp16": 4, "sc16": 4}
MAX_BATCHES = 2			# partial slots per instance (the default of 8 costs 1 GiB of counts at N = 65536, 512 bins)


def oracle_threads():
    return min(os.cpu_count() or 1, 16)


def stream_samples(case):
    n = 1 << case["log2n"]
    return (case["total"] - 1) * (n // case["overlap"]) + n


def rank_state_bytes(case, max_spectra):
    """Upper bound of what an instance of max_spectra spectra allocates on the device (fosphor_amd_init): hit-count slots and
    their export view, histogram, two waterfall rings, count slabs, four sets of 16-bit bin indices, the N = 65536 scratch
    spectrum, chunk partials."""
    n, nb = 1 << case["log2n"], case["n_bins"]
    cells = nb * n
    b = 4 * cells * (MAX_BATCHES + 2) + 2 * 4 * case["wf_rows"] * n + 2 * cells * (max_spectra // 1024)
    b += 4 * 2 * max_spectra * n + 8 * (max_spectra // 16 + 1) * n
    if case["log2n"] == 16:
        b += 8 * max_spectra * n
    return b


def case_bytes(case):
    """(device bytes, host bytes) a case needs, streams of both formats and both sets of ranks included for a twin case"""
    n, total = 1 << case["log2n"], case["total"]
    ns = stream_samples(case)
    twin = 2 if case["twin"] else 1
    dev = ns * SAMPLE_BYTES[case["fmt"]] + (ns * 8 if case["twin"] else 0)
    dev += twin * sum(rank_state_bytes(case, cnt) for _, cnt in case["shards"])
    dev += 3 * 4 * case["n_bins"] * n				# the stacked partial counts of the emulated all-reduce
    host = ns * SAMPLE_BYTES[case["fmt"]] + ns * 8 + 2 * total * n * 8	# stream, its fp32 form, expanded frame, the oracle's FFT output
    return dev, host


def make_stream(case, frame=0):
    """(host array handed to the device, float32 [samples][2] the oracle sees) of frame `frame` of a case"""
    ns = stream_samples(case)
    seed = case["seed"] + 100 * frame
    if case["fmt"] == "sc16":
        p = _SC16
        x = sc16_iq(ns, seed, sigma=p["sigma"], tone=(p["amp"], p["freq"] + 0.011 * frame))
        return x, widen(x).reshape(-1, 2)
    p = _FP32
    x = add_tone(gaussian_iq(ns, seed, p["sigma"]), p["amp"], p["freq"] + 0.011 * frame, t0=frame * ns)
    if case["fmt"] == "fp16":
        x = x.astype(np.float16)		# the oracle sees the values on the fp16 grid
        return x, x.astype(np.float32)
    return x, x


def make_oracle(case):
    o = Oracle(fft_len_log=case["log2n"], n_bins=case["n_bins"], wf_rows=case["wf_rows"])
    o.set_power_range(*case["power"])
    return o


def oracle_frame(o, case, x32):
    """one display launch over the whole materialised frame"""
    n = 1 << case["log2n"]
    expanded = x32 if case["overlap"] == 1 else overlap_cc_reference(x32, n, case["overlap"])
    expanded = expanded[:case["total"] * n]
    assert expanded.shape[0] == case["total"] * n
    assert o.process(expanded, strict=False, nthreads=oracle_threads()) == 0


def plane_fractions(o):
    """fraction of the oracle's hits in bins < 256 and in bins >= 256"""
    hc = o.hitcount			# [x][bin]
    tot = float(hc.sum())
    return hc[:, :256].sum() / tot, hc[:, 256:].sum() / tot


def make_ranks(amd, case, fmt=None):
    fmt = fmt or case["fmt"]
    ranks = []
    for _, cnt in case["shards"]:
        f = amd.Fosphor(fft_len_log=case["log2n"], n_bins=case["n_bins"], wf_rows=case["wf_rows"], max_spectra=cnt,
                        max_batches=MAX_BATCHES, iq_format=fmt)
        f.set_power_range(*case["power"])
        ranks.append(f)
    return ranks


def run_sharded_frame(amd, torch, ranks, d_stream, shards, total, overlap=1, sample_words=2):
    """One frame through the emulated exchange.  d_stream: device tensor of the unexpanded stream, sample_words elements per
    sample; rank r gets the (n_local - 1) * hop + N samples from sample t_offset * hop on.  Returns, per rank, what it launched
    (launch_stats deltas of the accumulate call) and the sum of its 32-bit partial counts before the exchange."""
    from gr_fosphor_amd.dist import wrap_device_array
    assert len(ranks) == len(shards)
    flat = d_stream.reshape(-1)
    launches, hc_sums, parts = [], [], []
    for fr, (off, cnt) in zip(ranks, shards):
        hop = fr.n // overlap
        lo, ln = off * hop, (cnt - 1) * hop + fr.n
        before = fr.launch_stats()
        assert fr.accumulate_device(flat[lo * sample_words:(lo + ln) * sample_words], cnt, off, total, overlap=overlap) == 0
        launches.append(tuple(a - b for a, b in zip(fr.launch_stats(), before)))
        assert fr.finish() >= 0
        parts.append(fr.partials())
    hc = [wrap_device_array(p.d_hc, (p.n_hc,), torch.int32) for p in parts]
    ls = [wrap_device_array(p.d_live_sum, (p.n_cols,), torch.float32) for p in parts]
    mx = [wrap_device_array(p.d_max, (p.n_cols,), torch.float32) for p in parts]
    hc_sums = [int(h.sum(dtype=torch.int64)) for h in hc]
    hc_sum = torch.stack(hc).sum(0, dtype=torch.int32)
    ls_sum = torch.stack(ls).sum(0)
    mx_max = torch.stack(mx).max(0).values
    for r in range(len(ranks)):
        hc[r].copy_(hc_sum); ls[r].copy_(ls_sum); mx[r].copy_(mx_max)
    torch.cuda.synchronize()
    for fr in ranks:
        assert fr.merge(total) == 0
    for fr in ranks:
        assert fr.finish() >= 0
    return {"launches": launches, "hc_sums": hc_sums}


def computed_rows(o, shard, total, wf_rows):
    """ring rows of the frame the oracle processed last that the rank of `shard` computed: spectra
    [max(t_offset, total - wf_rows), t_offset + n_local) of the frame; spectrum t sits wf_pos_before + t into the ring"""
    off, cnt = shard
    lo, hi = max(off, total - wf_rows), off + cnt
    return [(o.waterfall_pos - total + t) & (wf_rows - 1) for t in range(lo, hi)]


def assert_frame_state(rank, oracle, shard, total, wf_rows, what, others_boot=False):
    """`rank` after the merge of a frame against the oracle after its one launch over that frame.  others_boot: the rank's
    instance has seen this frame only, so every ring row it did not compute must still hold the boot value."""
    hc_gpu, hc_ref = rank.hitcount, oracle.hitcount.T
    assert np.array_equal(hc_gpu, hc_ref), "%s: hit counts differ in %d cells" % (what, (hc_gpu != hc_ref).sum())
    assert int(hc_gpu.sum(dtype=np.uint64)) == total * rank.n, what + ": hit counts do not add up to the frame"
    assert rank.waterfall_pos == oracle.waterfall_pos, what + ": ring position"
    sp_g, sp_o = rank.spectrum, oracle.spectrum
    assert_close(sp_g[0, :, 1], sp_o[0, :, 1], what + " live")
    assert_close(sp_g[1, :, 1], sp_o[1, :, 1], what + " max-hold")
    assert_hist_close(rank.histogram, oracle.histogram, what + " histogram")
    rows = computed_rows(oracle, shard, total, wf_rows)
    wf = rank.waterfall
    boot = np.float32(-rank.histo_offset)		# cl.c:406-433: the ring boots at the noise floor
    if rows:
        assert len(set(rows)) == len(rows)
        assert_close(wf[rows], oracle.waterfall[rows], what + " waterfall (the rank's %d rows)" % len(rows))
    else:
        assert np.all(wf == boot), "%s: a rank that stores no row changed %d ring words" % (what, (wf != boot).sum())
    if others_boot:
        rest = np.ones(wf_rows, dtype=bool)
        rest[rows] = False
        assert np.all(wf[rest] == boot), "%s: %d words changed in rows the rank did not compute" % (what, (wf[rest] != boot).sum())
