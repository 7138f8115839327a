"""Extreme and non-finite samples beside ordinary ones: data shared by tests/test_extreme_cases_cpu.py, which proves on the oracle
alone that the inputs reach what they claim, and tests/test_gpu_extremes.py, which runs the kernels against them.

Every FFT kernel carries its own copy of the epilogue that re-finds the samples bin_fast could not settle, calls bin_exact and patches
the result into its own index format (a byte of a dword of four spectra, 16-bit indices, the low bytes of an even / odd pair and a bit
of a byte of 9th bits, 9-bit packing per tile) and its own l2[] registers, which then feed the waterfall row, the live sum and the max.
The `else` branch of bin_exact (|X|^2 outside [1e-30, 1e30], zero, NaN, inf: full search, log-power from the double's exponent and
mantissa, "hypot overflows float -> bin 0, +inf") is what the spectra below reach, each beside ordinary spectra in the same launch.

A case is a sequence of BATCHES of 16 spectra.  Every spectrum is Gaussian noise (sigma 0.05) plus a tone; a special spectrum is then
altered by its class.  A class that a batch holds stands in it TWICE, at positions slot and slot + 9 (slots 0, 2, 4, 6): both halves of
an even / odd pair, two residues mod 4 and mod 8, every special spectrum the only one of its pair -- so it has an ordinary neighbour in
its pair, in its dword of four and in its byte of eight.  A row of the kernel table runs the sequence under each of its rotations
(every position moved up by `rot`, mod 16): rotations 0 and 2 put every class at every residue mod 4 (the byte of k1_fft_bin's
pack[m]), rotations 0, 2, 4, 6 at every residue mod 8 (the bit of k1w_fft_bin's hi9).  tests/test_extreme_cases_cpu.py asserts it.

With an overlap (hop < N) a spectrum shares samples with its neighbours: those rows lay the altered windows out so that no two meet
and ordinary spectra remain beside them (positions, HOP1_HEAD), and the CPU test has conditions of its own for them."""
import functools

import numpy as np

from oracle_lib import Oracle, gaussian_iq, add_tone
from window_cases import as_format

WF_ROWS = 64
BATCH = 16
SEED = 9800

# ---- classes: float32 [N][2] of an ordinary spectrum -> the special one -----------------------------------------------------------
TONE_INF_RE = 2.9e38		# re = im of the overflow tone's bin: finite, and hypot = 4.1e38 is above FLT_MAX = 3.4e38


def _scaled(f):
    # (in double: 1e-42 is itself a subnormal float)
    return lambda s, rng, n, copy, wsum: (s.astype(np.float64) * f).astype(np.float32)


def _zero(s, rng, n, copy, wsum):
    return np.zeros_like(s)


def tone_inf_bin(n, copy):
    return n // 8 + 3 if copy == 0 else 3 * n // 8 + 5


def _tone_inf(s, rng, n, copy, wsum):
    """a bin-centred tone of phase pi/4 alone (the noise is below its last bit): under a real window of tap sum wsum its bin holds
    re = im = TONE_INF_RE"""
    amp = TONE_INF_RE * np.sqrt(2.0) / wsum
    ph = 2.0 * np.pi * tone_inf_bin(n, copy) * np.arange(n, dtype=np.float64) / n + np.pi / 4.0
    return np.stack([amp * np.cos(ph), amp * np.sin(ph)], 1).astype(np.float32)


def _one_sample(value, where, comp):
    def f(s, rng, n, copy, wsum):
        s = s.copy()
        s[(n * where[0]) // where[1] + copy, comp] = value
        return s
    return f


def _signs(mag):
    """every component +mag or -mag"""
    return lambda s, rng, n, copy, wsum: (mag * (2.0 * rng.integers(0, 2, s.shape) - 1.0)).astype(np.float32)


def _sub16(s, rng, n, copy, wsum):
    """subnormal halves: k * 2^-24, 0 < |k| < 1024"""
    k = rng.integers(1, 1024, s.shape) * (2 * rng.integers(0, 2, s.shape) - 1)
    return (k * 2.0 ** -24).astype(np.float32)


CLASSES = {
    # fp32
    "big":      _scaled(1e30),			# |X|^2 ~ 1e60: above 1e30, the fast path's s32 overflows; finite log-power
    "small":    _scaled(1e-30),			# |X|^2 ~ 1e-60: the fast path's s32 underflows to 0
    "sub":      _scaled(1e-42),			# subnormal samples, subnormal FFT words
    "zero":     _zero,				# |X|^2 = 0: -inf rows, bin 0
    "tone_inf": _tone_inf,			# hypot overflows float with re and im finite: +inf, bin 0, in the tone's column
    "nan1":     _one_sample(np.nan, (1, 3), 0),	# one NaN sample: the whole spectrum NaN
    "inf1":     _one_sample(np.inf, (2, 3), 1),	# one inf sample: inf and (inf - inf) NaN words
    # fp16: what a half can hold (with zero, nan1, inf1)
    "max16":    _signs(65504.0),
    "sub16":    _sub16,
    # sc16: no non-finite value exists (with zero)
    "full":     _signs(1.0),			# +1.0 clips to 32767, -1.0 is -32768
    "lsb":      _signs(2.0 ** -15),
}

# ---- batches, in this order: name -> format -> [(class, slot)] ----------------------------------------------------------------------
# fp16 and sc16 have no `scaled` classes of fp32's reach and no overflow tone (the largest |X| a half or an int16 spectrum gives is
# N * 65504): their `scaled` batch holds the extremes of the format, their `column_inf` and `nan_columns` batches are ordinary, and
# sc16's `nan` batch is a mixed one of zero and full-scale spectra.
_SCALED = {"fp32": [("big", 0), ("small", 2), ("sub", 4)], "fp16": [("max16", 0), ("sub16", 2)], "sc16": [("full", 0), ("lsb", 2)]}
BATCHES = {
    # full search, log-power from exponent + mantissa; everything stays finite: live sum and max-hold compare as numbers
    "scaled":      _SCALED,
    # live -inf in every column, max-hold untouched
    "minus_inf":   {f: v + [("zero", 6)] for f, v in _SCALED.items()},
    # +inf and bin 0 in the tone's columns only, the top bin around them
    "column_inf":  {"fp32": [("tone_inf", 0)], "fp16": [], "sc16": []},
    # +inf + -inf = NaN in the tone's columns, -inf elsewhere
    "nan_columns": {"fp32": [("tone_inf", 2), ("zero", 4)], "fp16": [], "sc16": []},
    # ... and a NaN and an inf sample: NaN live everywhere, non-finite max-hold
    "nan":         {"fp32": [("tone_inf", 6), ("zero", 0), ("nan1", 2), ("inf1", 4)],
                    "fp16": [("zero", 0), ("nan1", 2), ("inf1", 4)], "sc16": [("zero", 0), ("full", 4)]},
    # display.cl:206-207,290-291 take the state back; the decay goes on as usual
    "recover":     {"fp32": [], "fp16": [], "sc16": []},
    "recover2":    {"fp32": [], "fp16": [], "sc16": []},
}
ORDER = tuple(BATCHES)
COPY_STEP = 9			# the second copy of a class: position slot + 9


def positions(name, fmt, rot, overlap=1):
    """[(class, copy, position in the batch)] of batch `name` under rotation rot.

    With an overlap (hop = N / overlap, 2 <= overlap <= 8) the altered window of N samples at position p is part of the spectra
    p - overlap + 1 .. p + overlap - 1 as well, so the windows must not meet and must leave spectra untouched: a batch holds
    16 / (2 overlap) classes, once each, 16 / that many positions apart, cyclically, from position 1 + rot on -- four at overlap 2
    (every class of the batch), ONE at overlap 8 (class `rot` of the batch's, in turn).  The same positions in every batch keep the
    windows of neighbouring batches apart too.  (hop 1 has a layout of its own: HOP1_HEAD.)"""
    if overlap == 1:
        return [(cls, copy, (slot + COPY_STEP * copy + rot) % BATCH) for cls, slot in BATCHES[name][fmt] for copy in (0, 1)]
    assert 2 <= overlap <= BATCH // 2
    classes = [cls for cls, _ in BATCHES[name][fmt]]
    room = BATCH // (2 * overlap)
    step = BATCH // room
    turn = rot if len(classes) > room else 0		# the batch's classes take turns where they do not all fit
    return [(classes[(i + turn) % len(classes)], 0, (1 + step * i + rot) % BATCH) for i in range(min(room, len(classes)))]


def special_positions(name, fmt, rot):
    return sorted(p for _, _, p in positions(name, fmt, rot))


# hop 1 (process_device_overlap at overlap N, the odd hop that selects k1v2_fft_bin): spectrum g is samples g .. g + N - 1, so a sample
# s < 112 is part of the spectra 0 .. s and of no other -- whatever is altered further in is part of every spectrum of the call.  The
# row therefore alters two samples at the head of the stream: a NaN at sample 2 + rot (spectra 0 .. 2 + rot are NaN) and a factor of
# 1e30 on sample 8 + rot (spectra 3 + rot .. 8 + rot: |X|^2 ~ 1e56 in every column, the top bin), and spectra 9 + rot .. 15 of the
# first batch and all six later batches are ordinary: NaN, huge and ordinary spectra in one launch, and the recovery inside it.
HOP1_HEAD = (("nan1", 2), ("big", 8))


def touched(log2n, fmt, overlap, rot, names=ORDER):
    """per spectrum of the stream: 2 = wholly a class's (hop 1: holds an altered sample), 1 = shares samples with such a window,
    0 = ordinary.  Asserts that no spectrum shares samples with two altered windows"""
    t = np.zeros(BATCH * len(names), np.int32)
    if overlap > BATCH:
        t[:HOP1_HEAD[-1][1] + rot + 1] = 2
        return t
    hits = np.zeros_like(t)
    for k, name in enumerate(names):
        for _, _, p in positions(name, fmt, rot, overlap):
            g = BATCH * k + p
            lo, hi = max(g - overlap + 1, 0), min(g + overlap, t.size)
            hits[lo:hi] += 1
            t[lo:hi] = np.maximum(t[lo:hi], 1)
            t[g] = 2
    assert hits.max() <= 1, "two altered windows meet in one spectrum"
    return t


# ---- streams -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def window_sum(log2n):
    return float(Oracle(fft_len_log=log2n, n_bins=128, wf_rows=WF_ROWS).window.astype(np.float64).sum())


def n_samples(log2n, overlap, n_spectra):
    n = 1 << log2n
    return (n_spectra - 1) * (n // overlap) + n


def ordinary_stream(log2n, overlap, names, seed=SEED):
    ns = n_samples(log2n, overlap, BATCH * len(names))
    return add_tone(gaussian_iq(ns, seed + log2n), 0.05, 0.0313)


def apply_classes(x32, log2n, overlap, placed, seed=SEED):
    """x32 with the spectrum at index g (samples g * hop .. g * hop + N) altered by its class, for (class, copy, g) in placed"""
    n = 1 << log2n
    hop = n // overlap
    x = x32.copy()
    for cls, copy, g in placed:
        rng = np.random.default_rng([seed, g, sorted(CLASSES).index(cls)])
        x[g * hop:g * hop + n] = CLASSES[cls](x[g * hop:g * hop + n], rng, n, copy, window_sum(log2n))
    return x


@functools.lru_cache(maxsize=2)
def stream(log2n, fmt, overlap=1, rot=0, names=ORDER, plain=False):
    """(array handed to the library, float32 [samples][2] of exactly those values for the oracle) of the batches `names` back to back,
    spectrum i of batch k at sample (16 k + i) * hop.  plain: the same stream with no spectrum altered"""
    x = ordinary_stream(log2n, overlap, names)
    if not plain and overlap > BATCH:
        assert overlap == 1 << log2n and fmt == "fp32"
        (_, s_nan), (_, s_big) = HOP1_HEAD
        x = x.copy()
        x[s_nan + rot, 0] = np.nan
        x[s_big + rot] *= np.float32(1e30)
    elif not plain:
        x = apply_classes(x, log2n, overlap, [(cls, copy, BATCH * k + p) for k, name in enumerate(names)
                                              for cls, copy, p in positions(name, fmt, rot, overlap)])
    with np.errstate(over="ignore", invalid="ignore"):
        x, xo = as_format(x, fmt)
    x.setflags(write=False); xo.setflags(write=False)
    return x, xo


def batch_of(xo, log2n, overlap, k):
    """float32 [16 * N][2]: the (overlap_cc-expanded) spectra of batch k of a stream, as the oracle takes them"""
    n = 1 << log2n
    hop = n // overlap
    if overlap == 1:
        return xo[k * BATCH * n:(k + 1) * BATCH * n]
    return np.concatenate([xo[(k * BATCH + i) * hop:(k * BATCH + i) * hop + n] for i in range(BATCH)])


def make_oracle(row):
    o = Oracle(fft_len_log=row["log2n"], n_bins=row["n_bins"], wf_rows=WF_ROWS)
    if row["power"]:
        o.set_power_range(*row["power"])
    return o


# ---- the kernel table -----------------------------------------------------------------------------------------------------------------
# entry: "device" = process_device, "overlap" = process_device_overlap (hop = N / overlap); host: the batches go through fosphor_process
# as well.  power: set_power_range (None: the default, 0 dB and 10 dB/div); at 512 bins the ranges put ordinary spectra's hits in both
# halves of the bin range (tests/shard_emul.py's, and at N = 1024 the same 9 dB further down: an eighth of the points).  rots: the
# rotations the row runs under (hop = N: by twos, see the top; with an overlap by ones, see positions; N = 65536: 0 and 2 put every
# class in every lane of k1h_fused's bng[4]).  fft: the window_cases.FFT_CASES entry that reaches the instantiation's FFT hook.
_R4, _R8 = (0, 2), (0, 2, 4, 6)
_OV = tuple(range(8))


def _row(log2n, n_bins, fmt, kernel, rots, entry="device", overlap=1, env=None, power=None, host=False, fft=None):
    return dict(log2n=log2n, n_bins=n_bins, fmt=fmt, kernel=kernel, plan=kernel.split("<")[0], rots=rots, entry=entry,
                overlap=overlap, env=env or {}, power=power, host=host, fft=fft)


ROWS = {
    "n1024_128":    _row(10, 128, "fp32", "k1_fft_bin<iq_fp32>", _R4, host=True, fft="n1024_v1"),
    "n1024_nb256":  _row(10, 256, "fp32", "k1_fft_bin<iq_fp32, NB256>", _R4),
    "n1024_hop1":   _row(10, 128, "fp32", "k1v2_fft_bin<iq_fp32> (odd hop)", (0, 1, 2, 3), entry="overlap", overlap=1024),
    "n1024_v2":     _row(10, 128, "fp32", "k1v2_fft_bin<iq_fp32> (FOSPHOR_AMD_K1=2)", _R4, env={"FOSPHOR_AMD_K1": "2"}, host=True,
                         fft="n1024_v2"),
    "n1024_k1big":  _row(10, 512, "fp32", "k1big_fft_bin<iq_fp32, 10>", _R4, power=(-31, 5), host=True, fft="n1024_k1big"),
    "n8192_ov1":    _row(13, 512, "fp32", "k1w_fft_bin<iq_fp32, 16> (no reuse)", _R8, power=(-40, 5), fft="n8192_k1w"),
    "n8192_ov2":    _row(13, 512, "fp32", "k1w_fft_bin<iq_fp32, 8>", _OV, entry="overlap", overlap=2, power=(-40, 5)),
    "n8192_ov8":    _row(13, 512, "fp32", "k1w_fft_bin<iq_fp32, 2>", _OV, entry="overlap", overlap=8, power=(-40, 5)),
    "n65536_fp32":  _row(16, 512, "fp32", "k1h_fused<iq_fp32>", _R4, power=(-46, 5), fft="n65536_fp32"),
    "n65536_fp16":  _row(16, 512, "fp16", "k1h_fused<iq_fp16>", _R4, power=(-46, 5), fft="n65536_fp16"),
    "n65536_sc16":  _row(16, 512, "sc16", "k1h_fused<iq_sc16>", _R4, power=(-46, 5), fft="n65536_sc16"),
}
MAX_SPECTRA = BATCH * len(ORDER)	# the smallest instance that holds the case in one call
FFT_BATCHES = ("scaled", "nan")	# the batches the FFT hook runs

# every knob a row may set; cleared before a row's instance is made
KNOBS = ("FOSPHOR_AMD_K1", "FOSPHOR_AMD_TILE", "FOSPHOR_AMD_SUB_LOG2", "FOSPHOR_AMD_K1_STREAMS", "FOSPHOR_AMD_OVERLAP",
         "FOSPHOR_AMD_ALT", "FOSPHOR_AMD_PIPE3", "FOSPHOR_AMD_ROWMASK", "FOSPHOR_AMD_K1W_SHARE", "FOSPHOR_AMD_NO_SUM16",
         "FOSPHOR_AMD_FRAME_GROUP")

# ---- sharded frames (tests/shard_emul.py's case form): two ranks of 16 spectra each ----------------------------------------------------
# frame 0, `nan`: the all-zero spectra on rank 0, the overflow tones on rank 1 -- one rank's -inf meets the other's +inf in the float
# sum of the exchange; frame 1, `column_inf`: the tones on rank 0, and a x 1e30 and a x 1e-30 spectrum on rank 1 (hits in bin
# n_bins - 1 and in bin 0).  (class, copy, spectrum of the frame)
SHARD_FRAMES = (
    [("zero", 0, 3), ("zero", 1, 12), ("tone_inf", 0, 20), ("tone_inf", 1, 29)],
    [("tone_inf", 0, 5), ("tone_inf", 1, 10), ("big", 0, 18), ("small", 0, 25)],
)
SHARD_CASES = {
    "n1024":  dict(log2n=10, fmt="fp32", n_bins=256, wf_rows=WF_ROWS, total=32, overlap=1, frames=2, shards=[(0, 16), (16, 16)],
                   env={}, power=(0, 10), seed=9811, twin=False),
    "n8192":  dict(log2n=13, fmt="fp32", n_bins=512, wf_rows=WF_ROWS, total=32, overlap=1, frames=2, shards=[(0, 16), (16, 16)],
                   env={}, power=(-40, 5), seed=9812, twin=False),
    # the row-mask hand-off is on (the default)
    "n65536": dict(log2n=16, fmt="fp32", n_bins=512, wf_rows=WF_ROWS, total=32, overlap=1, frames=2, shards=[(0, 16), (16, 16)],
                   env={}, power=(-46, 5), seed=9813, twin=False),
}


def shard_stream(case, frame):
    x = add_tone(gaussian_iq(case["total"] << case["log2n"], case["seed"] + 100 * frame), 0.05, 0.0313 + 0.011 * frame)
    x = apply_classes(x, case["log2n"], 1, SHARD_FRAMES[frame], seed=case["seed"])
    x.setflags(write=False)
    return x, x


# ---- tile walks: tests/tile_walk_cases.py's calls, with special spectra in the tiles of units that take a second tile ------------------
# At 7 x 16 spectra no launch has more tiles than units, so the long calls of tile_walk_cases.CASES serve: one per kernel, as tabled
# there (batches up to 1088 spectra).  The special spectra go one to a tile into the first-pass tiles T0, T0 + 1, ... where T0 is the
# first tile whose unit's NEXT tile (T0 + units) lies in the last batch of the call: a live / max partial that leaked from a unit's
# non-finite tile into the tile it takes next would then stand in the state the call leaves (a NaN in an earlier batch would be
# taken back by the batch after it, display.cl:206-207).  hop 1: the altered samples of WALK_HOP1_HEAD instead (spectra 0 .. 9 NaN,
# 10 .. 21 huge: the tiles 0 .. 5 of units that all take a second tile, in the last batch).
WALK_CASES = ("w_fp32_256", "v2_oddhop", "big_512", "wide_ov2")
WALK_CLASSES = ("zero", "tone_inf", "big", "small", "nan1")
WALK_HOP1_HEAD = (("nan1", 9), ("big", 21))


def walk_first_tile(c, plan):
    """T0 of the call c (a tile_walk_cases.CASES entry) under the launch plan (tile, tiles, units)"""
    total, batch = c["n_batches"] * c["batch"], c["batch"]
    return max(-(-(total - batch) // plan["tile"]) - plan["units"], 0)


def walk_placed(c, plan):
    """[(class, copy, spectrum of the call)]: class j in tile T0 + j, second spectrum of the tile (hop < N: the window's neighbours lie
    in the same tile of 8)"""
    t0 = walk_first_tile(c, plan)
    return [(cls, 0, (t0 + j) * plan["tile"] + 1) for j, cls in enumerate(WALK_CLASSES)]


def walk_stream(c, x32, plan):
    """the call's samples (tile_walk_cases.stream's float32 form) with the special spectra in"""
    if c["overlap"] > BATCH:
        (_, s_nan), (_, s_big) = WALK_HOP1_HEAD
        x = x32.copy()
        x[s_nan, 0] = np.nan
        x[s_big] *= np.float32(1e30)
        return x
    return apply_classes(x32, c["log2n"], c["overlap"], walk_placed(c, plan))
