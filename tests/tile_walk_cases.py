"""FFT launches in which one wave or work-group takes SEVERAL tiles: data shared by tests/test_tile_walk_cases_cpu.py, which proves
without a GPU that every case strides, and tests/test_gpu_tile_walk.py, which runs the kernels against the oracle.

Every FFT-and-bin kernel is persistent: a wave (k1_fft_bin) or a work-group (k1v2_fft_bin, k1big_fft_bin, k1w_fft_bin) takes tile t,
then t + stride, ...  What crosses a tile boundary -- the prefetch of the next tile's first spectrum and its guard, the per-tile reset
of the live / max partials, k1_fft_bin's bin dwords flushed one spectrum late, k1w_fft_bin's held registers, the partial row index --
is exercised only by a launch with more tiles than the grid has units: 2048 waves, 1536, 4096 or (CU count) work-groups (launch_k1_as
in csrc/fosphor_kernels.hip).  The default tile rule avoids that for almost every call; the cases below are calls for which it
cannot, or that set FOSPHOR_AMD_TILE.

CASES states each walk by hand, for a 256-CU device (and WIDE_OTHER_CUS for the N = 8192 cases); expected_plan restates the launch
rules as they stood before fosphor_amd_plan_k1 existed.  Neither comes from the function under test."""
import functools

import numpy as np

from oracle_lib import gaussian_iq, add_tone
from test_gpu_iq_sc16 import sc16_iq, widen

# every knob that shapes an FFT launch or the pieces of a call; cleared before a case's instance is made (FOSPHOR_AMD_K1_BLOCKS, a
# debugging aid read once per process, is never set by a test)
KNOBS = ("FOSPHOR_AMD_K1", "FOSPHOR_AMD_TILE", "FOSPHOR_AMD_SUB_LOG2", "FOSPHOR_AMD_K1_STREAMS", "FOSPHOR_AMD_OVERLAP",
         "FOSPHOR_AMD_ALT", "FOSPHOR_AMD_PIPE3", "FOSPHOR_AMD_ROWMASK", "FOSPHOR_AMD_K1W_SHARE", "FOSPHOR_AMD_NO_SUM16")

_T4 = {"FOSPHOR_AMD_TILE": "4"}


def _case(log2n, n_bins, fmt, n_batches, batch, kernel, walk, wf_rows, overlap=1, offset=0, env=None, seed=0):
    return dict(log2n=log2n, n_bins=n_bins, fmt=fmt, n_batches=n_batches, batch=batch, kernel=kernel, walk=walk, wf_rows=wf_rows,
                overlap=overlap, offset=offset, env=env or {}, seed=seed)


def _walk(tile, tiles, units, most, n_most):
    """`tiles` tiles of `tile` spectra over `units` units: n_most of them take `most` tiles, the others one fewer"""
    return dict(tile=tile, tiles=tiles, units=units, max_tiles=most, min_tiles=most - 1, n_most=n_most)


# n_batches x batch spectra per call, batches <= 1088 (the pipeline's 16-bit count hand-off); overlap: process_device_overlap's ratio
# (hop = N / overlap); offset: samples in front of the first one handed over (sc16: one sample = a start at 4 mod 8 bytes).
# wf_rows: the ring holds every row of the walk's LAST pass (the highest-numbered tiles), see last_pass_spectra.
CASES = {
    # k1_fft_bin (N = 1024, <= 256 bins, even hop): 512 work-groups x 4 waves = 2048 waves
    "w_fp32_256":        _case(10, 256, "fp32", 10, 928, "k1_fft_bin", _walk(4, 2320, 2048, 2, 272), 2048, env=_T4, seed=9701),
    "w_sc16_128_x3":     _case(10, 128, "sc16", 16, 1056, "k1_fft_bin", _walk(4, 4224, 2048, 3, 128), 1024, env=_T4, seed=9702),
    # no knob: batch = 16 x odd and an odd number of batches, so that 16 is the largest tile that divides the batch AND the call
    # taken as one batch; 2065 tiles is within a few of the fewest (2049) with which the default configuration strides at all
    "w_default":         _case(10, 256, "fp32", 35, 944, "k1_fft_bin", _walk(16, 2065, 2048, 2, 17), 512, seed=9703),
    # k1v2_fft_bin: 1536 work-groups
    "v2_oddhop":         _case(10, 128, "fp32", 7, 1008, "k1v2_fft_bin", _walk(4, 1764, 1536, 2, 228), 1024, overlap=1024, seed=9704),
    "v2_sc16_unaligned": _case(10, 256, "sc16", 7, 1008, "k1v2_fft_bin", _walk(4, 1764, 1536, 2, 228), 1024, offset=1, seed=9705),
    # k1big_fft_bin<10>: 4096 work-groups
    "big_512":           _case(10, 512, "fp32", 17, 1008, "k1big_fft_bin", _walk(4, 4284, 4096, 2, 188), 1024, env=_T4, seed=9706),
    # k1w_fft_bin: one work-group per CU; overlap 2 reuses half a window from registers along a tile, overlap 1 is the no-reuse form
    "wide_ov2":          _case(13, 512, "fp32", 2, 1088, "k1w_fft_bin", _walk(8, 272, 256, 2, 16), 256, overlap=2, seed=9707),
    "wide_sc16_ov1":     _case(13, 512, "sc16", 2, 1088, "k1w_fft_bin", _walk(8, 272, 256, 2, 16), 256, seed=9708),
}
# the N = 8192 walks on a device of another size
WIDE_OTHER_CUS = 128
WIDE_OTHER_WALK = _walk(8, 272, 128, 3, 16)

FORMS = ("batches", "one_batch")	# the call as tabled / the same spectra as ONE batch of `total` spectra


def total(c):
    return c["n_batches"] * c["batch"]


def hop(c):
    return (1 << c["log2n"]) // c["overlap"]


def call_shape(c, form):
    """(n_batches, batch) of the call in that form"""
    return (c["n_batches"], c["batch"]) if form == "batches" else (1, total(c))


def iq_align(c):
    """byte address of the first sample handed over, modulo 16 (device allocations start on far larger boundaries)"""
    return (c["offset"] * (4 if c["fmt"] == "sc16" else 8)) % 16


def walk_on(c, n_cus):
    """the case's stated walk on a device of n_cus CUs (only the N = 8192 launches depend on it)"""
    if c["log2n"] == 13 and n_cus != 256:
        assert n_cus == WIDE_OTHER_CUS
        return WIDE_OTHER_WALK
    return c["walk"]


def last_pass_spectra(walk):
    """spectra of the tiles a unit reaches only in its last pass over the grid (the highest-numbered ones)"""
    return (walk["tiles"] - (walk["max_tiles"] - 1) * walk["units"]) * walk["tile"]


def sub_samples(log2n):
    """samples per piece of a device-resident call with no FOSPHOR_AMD_SUB_LOG2 set (fosphor_amd_init)"""
    return 1 << (30 if log2n == 13 else 26)


# ---- the launch rules, restated from pick_tile / fill_k1 (csrc/fosphor_api.cpp) and launch_k1_as (csrc/fosphor_kernels.hip) as they
# ---- stood before the hook: what fosphor_amd_plan_k1 must keep returning ----------------------------------------------------------
def expected_tile(log2n, n_bins, tile_knob, total, batch):
    v = tile_knob
    if (8 if log2n == 13 else 4) <= v <= (32 if log2n == 16 else 128) and not (v & (v - 1)) and batch % v == 0 and total % v == 0:
        return v
    if log2n == 16:
        return next((t for t in (32, 16, 8) if batch % t == 0 and total // t >= 32), 4)
    if log2n == 13:
        return next((t for t in (64, 32, 16, 8) if batch % t == 0 and total // t >= 256), 8)
    if n_bins > 256:
        return 16 if total // 16 >= 2048 else 8 if total // 8 >= 2048 else 4
    return next((t for t in (64, 32, 16, 8) if batch % t == 0 and total // t >= 1024), 4)


def expected_plan(log2n, n_bins, fmt, hop, align, tile_knob, k1_knob, n_cus, total, batch):
    tile = expected_tile(log2n, n_bins, tile_knob, total, batch)
    tiles = total // tile
    if log2n == 16:
        return dict(kernel="k1h_fused", tile=tile, tiles=tiles, units=32, max_tiles=0, min_tiles=0)
    if log2n == 13:
        kernel, cap = "k1w_fft_bin", n_cus or 256
    elif n_bins > 256:
        kernel, cap = "k1big_fft_bin", 4096
    elif k1_knob == 2 or hop % 2 or (fmt == "sc16" and align % 8):
        kernel, cap = "k1v2_fft_bin", 1536
    else:
        kernel, cap = "k1_fft_bin", 4 * min((tiles + 3) // 4, 512)
    units = min(tiles, cap)
    return dict(kernel=kernel, tile=tile, tiles=tiles, units=units, max_tiles=-(-tiles // units), min_tiles=tiles // units)


# the launches bench.py times (one piece of a step each): name -> arguments of expected_plan / plan_k1
BENCH_SHAPES = {
    "C2": dict(log2n=10, n_bins=256, fmt="fp32", hop=1024, align=0, tile_knob=0, k1_knob=1, n_cus=256, total=64 * 1024, batch=1024),
    "C3": dict(log2n=13, n_bins=512, fmt="fp32", hop=4096, align=0, tile_knob=0, k1_knob=1, n_cus=256, total=28 * 4096, batch=4096),
    "C5": dict(log2n=16, n_bins=512, fmt="fp16", hop=65536, align=0, tile_knob=0, k1_knob=1, n_cus=256, total=1024, batch=1024),
}


# ---- inputs: Gaussian noise and a tone ---------------------------------------------------------------------------------------
def n_samples(c):
    return (total(c) - 1) * hop(c) + (1 << c["log2n"])


@functools.lru_cache(maxsize=1)
def stream(cid):
    """(array handed to the library -- case["offset"] samples in front included --, float32 [samples][2] of exactly the values
    the library sees, from the first sample handed over on)"""
    c = CASES[cid]
    ns = n_samples(c) + c["offset"]
    if c["fmt"] == "sc16":
        x = sc16_iq(ns, c["seed"], sigma=3000.0, tone=(8000.0, 0.123))
        x32 = widen(x).reshape(-1, 2)
    else:
        x = add_tone(gaussian_iq(ns, c["seed"]), 0.05, 0.0313)
        x32 = x
    x32 = x32[c["offset"]:]
    x.setflags(write=False); x32.setflags(write=False)
    return x, x32


def oracle_call(o, c, form, x32, nthreads=8):
    """the oracle's statement of the call: one display launch per batch over the materialised (overlap_cc-expanded) windows"""
    n, h = 1 << c["log2n"], hop(c)
    n_batches, batch = call_shape(c, form)
    for k in range(n_batches):
        if c["overlap"] == 1:
            e = x32[k * batch * n:(k + 1) * batch * n]
        else:
            first = k * batch * h
            e = np.lib.stride_tricks.as_strided(x32[first:], shape=(batch, n, 2), strides=(h * 8, 8, 4), writeable=False)
        assert o.process(e, strict=False, nthreads=nthreads) == 0
