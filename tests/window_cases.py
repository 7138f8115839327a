"""Caller-set FFT windows and mid-stream setting changes: data shared by tests/test_window_cases_cpu.py, which checks the inputs
and the oracle without a GPU, and tests/test_gpu_windows.py, which runs the kernels against them.

The default window (a periodic Hamming) is smooth, strictly positive and mirror-symmetric to 1.4e-6: a kernel that read the taps
backwards, half a turn off, or only the first 1024 of them would pass every test that runs under it.  WINDOWS are windows under
which such a kernel cannot pass; SCRAMBLES are the wrong windows a kernel or host bug would effectively apply, and
tests/test_window_cases_cpu.py asserts that the oracle's hit counts under a window differ from those under each of its scrambles in
at least MIN_CELLS cells -- a condition on the inputs, not a tolerance on the kernels.

FFT_CASES and PATH_CASES name the kernel instantiation each case reaches (launch_k1_as / launch_k1h in csrc/fosphor_kernels.hip,
the variant choice in fill_k1 of csrc/fosphor_api.cpp) and how it is reached."""
import functools

import numpy as np

from oracle_lib import gaussian_iq, add_tone
from test_gpu_iq_sc16 import sc16_iq, widen

MIN_CELLS = 1000
WF_ROWS = 64
RANDOM_SEED = 9100


# ---- windows: functions of n, float32 [n] ---------------------------------------------------------------------------------
def _ramp64(n):
    k = np.arange(n, dtype=np.float64)
    return (0.25 + 0.75 * k / n) * (1.0 + 0.25 * np.sin(2.0 * np.pi * 5.0 * k / n + 0.7))


def ramp(n):
    """smooth and visibly asymmetric"""
    return _ramp64(n).astype(np.float32)


def random(n):
    return (0.5 + np.random.default_rng(RANDOM_SEED + n).random(n)).astype(np.float32)


def signed_sparse(n):
    """ramp with the sign flipped on odd k, exact zeros on [n/4, n/4 + n/16), a gain of 8 on [3n/4, 3n/4 + 64): negative taps, zero
    taps and a discontinuity inside single threads' hoisted tap pairs (k and k + n/2)"""
    w = _ramp64(n)
    w[1::2] = -w[1::2]
    w[n // 4:n // 4 + n // 16] = 0.0
    w[3 * n // 4:3 * n // 4 + 64] *= 8.0
    return w.astype(np.float32)


def zero(n):
    return np.zeros(n, np.float32)


WINDOWS = {"ramp": ramp, "random": random, "signed_sparse": signed_sparse, "zero": zero}
FINITE = ("ramp", "random", "signed_sparse")		# the windows with a spectrum to compare


def default_window(n):
    """the library's default (fosphor.c:113-118: periodic Hamming x 1.855, float32 arithmetic); within an ulp or two of the
    oracle's own, which is what tests/test_window_cases_cpu.py holds it to -- it serves as a WRONG window here, nothing more"""
    k = np.arange(n, dtype=np.float32)
    return ((np.float32(0.54) - np.float32(0.46) * np.cos((np.float32(2.0) * np.float32(3.141592) * k) / np.float32(n)))
            * np.float32(1.855)).astype(np.float32)


# ---- scrambles: the window a bug would apply instead of w -----------------------------------------------------------------
def reversed_taps(w):
    n = w.size
    return w[(n - np.arange(n)) % n].copy()


def half_turn(w):
    n = w.size
    return w[(np.arange(n) + n // 2) % n].copy()


def first_1024_repeated(w):
    return w[np.arange(w.size) % 1024].copy()


SCRAMBLES = {"reversed": reversed_taps, "half_turn": half_turn, "first_1024_repeated": first_1024_repeated,
             "default": lambda w: default_window(w.size)}


def scrambles_of(n):
    """the scrambles that are scrambles at length n: the first 1024 taps repeated are the window itself at n = 1024"""
    return [s for s in SCRAMBLES if not (s == "first_1024_repeated" and n <= 1024)]


# ---- the discrimination input (CPU test): 16 spectra of noise and a tone, at the bin count of each length's cases ------------
DISCRIMINATION = {10: 128, 13: 512, 16: 512}		# log2n -> n_bins


def discrimination_input(log2n):
    return add_tone(gaussian_iq(16 << log2n, 9200 + log2n), 0.05, 0.0313)


# ---- samples in the three formats -------------------------------------------------------------------------------------------
def as_format(x32, fmt):
    """(array handed to the library, float32 [samples][2] of exactly those values for the oracle) from float32 [samples][2]"""
    if fmt == "fp16":
        x = x32.astype(np.float16)
        return x, x.astype(np.float32)
    if fmt == "sc16":
        x = np.clip(np.rint(x32.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16).reshape(-1)
        return x, widen(x).reshape(-1, 2)
    return x32, x32


# ---- 1. the FFT hook --------------------------------------------------------------------------------------------------------
FFT_SPECTRA = 8
FFT_CASES = {
    "n1024_v1":     dict(log2n=10, n_bins=128, fmt="fp32", env={}, kernel="k1_fft_bin<iq_fp32, fft_out>"),
    "n1024_v2":     dict(log2n=10, n_bins=128, fmt="fp32", env={"FOSPHOR_AMD_K1": "2"}, kernel="k1v2_fft_bin<iq_fp32, fft_out>"),
    "n1024_k1big":  dict(log2n=10, n_bins=512, fmt="fp32", env={}, kernel="k1big_fft_bin<iq_fp32, 10, fft_out>"),
    "n8192_k1w":    dict(log2n=13, n_bins=512, fmt="fp32", env={}, kernel="k1w_fft_bin<iq_fp32, 16>"),
    "n65536_fp32":  dict(log2n=16, n_bins=512, fmt="fp32", env={}, kernel="k1h_fused<iq_fp32, fft_out>"),
    "n65536_fp16":  dict(log2n=16, n_bins=512, fmt="fp16", env={}, kernel="k1h_fused<iq_fp16, fft_out>"),
    "n65536_sc16":  dict(log2n=16, n_bins=512, fmt="sc16", env={}, kernel="k1h_fused<iq_sc16, fft_out>"),
}
DFT_BOUND = {10: 1e-6, 13: 1e-6, 16: 2e-6}		# against numpy's fp64 FFT, relative to the largest value: the existing tests' bounds


@functools.lru_cache(maxsize=None)
def fft_input(log2n, fmt):
    """FFT_SPECTRA spectra of unit-variance noise (sc16: 2^-3 of full scale, so that nothing clips)"""
    x32 = gaussian_iq(FFT_SPECTRA << log2n, 9300 + log2n, sigma=1.0)
    if fmt == "sc16":
        x32 = x32 * np.float32(0.125)
    x, xo = as_format(x32, fmt)
    x.setflags(write=False); xo.setflags(write=False)
    return x, xo


# ---- 2. the whole path: three queued calls, a window and a power-range change, back to the default window -----------------
PAIRS = [("ramp", "signed_sparse"), ("random", "zero")]		# (window of call 0, window of call 1); call 2: the default window
POWER_RANGE_1 = (-10, 5)					# set with the second window

_T32 = {"FOSPHOR_AMD_TILE": "32"}


def _path(log2n, n_bins, fmt, entry, spectra, kernel, n_batches=1, overlap=1, env=None, offset=0):
    return dict(log2n=log2n, n_bins=n_bins, fmt=fmt, entry=entry, spectra=spectra, n_batches=n_batches, overlap=overlap,
                env=env or {}, offset=offset, kernel=kernel)


# entry: "host" = fosphor_process, "device" = process_device, "overlap" = process_device_overlap.  spectra: per batch, per call.
# offset: samples in front of the first one handed over (sc16: one sample = a start at 4 mod 8 bytes).
PATH_CASES = {
    "n1024_host":      _path(10, 128, "fp32", "host", (64, 64, 64), "k1_fft_bin<iq_fp32>"),
    "n1024_2x64":      _path(10, 128, "fp32", "device", (64, 64, 64), "k1_fft_bin<iq_fp32>", n_batches=2),
    "n1024_nb256":     _path(10, 256, "fp32", "device", (64, 64, 64), "k1_fft_bin<iq_fp32, NB256>"),
    "n1024_hop1":      _path(10, 128, "fp32", "overlap", (64, 64, 64), "k1v2_fft_bin<iq_fp32> (odd hop)", overlap=1024),
    "n1024_sc16_4mod8": _path(10, 128, "sc16", "device", (64, 64, 64), "k1v2_fft_bin<iq_sc16> (start at 4 mod 8 bytes)", offset=1),
    "n1024_k1big":     _path(10, 512, "fp32", "device", (64, 64, 64), "k1big_fft_bin<iq_fp32, 10>"),
    "n8192_ov1":       _path(13, 512, "fp32", "device", (32, 64, 64), "k1w_fft_bin<iq_fp32, 16> (no reuse)"),
    "n8192_host":      _path(13, 512, "fp32", "host", (16, 16, 16), "k1w_fft_bin<iq_fp32, 16> (no reuse)"),
    "n8192_sc16_ov4":  _path(13, 512, "sc16", "overlap", (32, 64, 64), "k1w_fft_bin<iq_sc16, 4>", overlap=4),
    "n65536_fp32":     _path(16, 512, "fp32", "device", (16, 32, 32), "k1h_fused<iq_fp32>"),
    "n65536_fp16":     _path(16, 512, "fp16", "device", (16, 32, 32), "k1h_fused<iq_fp16>"),
    "n65536_sc16":     _path(16, 512, "sc16", "device", (16, 32, 32), "k1h_fused<iq_sc16>"),
}
# hop N/2 .. N/16: rows reused from the previous spectrum (one instantiation each); N/32: none.  Tiles of 8 (what these short
# calls pick) and of 32 (FOSPHOR_AMD_TILE): the reuse runs along a tile
for _ov, _r in ((2, 8), (4, 4), (8, 2), (16, 1), (32, 16)):
    for _tile, _env in (("", {}), ("_tile32", _T32)):
        PATH_CASES["n8192_ov%d%s" % (_ov, _tile)] = _path(13, 512, "fp32", "overlap", (32, 64, 64),
                                                         "k1w_fft_bin<iq_fp32, %d>" % _r, overlap=_ov, env=_env)

MAX_SPECTRA = 128


def call_samples(case, call):
    n = 1 << case["log2n"]
    return (case["n_batches"] * case["spectra"][call] - 1) * (n // case["overlap"]) + n


@functools.lru_cache(maxsize=4)
def path_streams(cid):
    """per call of PATH_CASES[cid]: (array handed to the library -- case["offset"] samples in front included --, float32
    [samples][2] the oracle sees, from the first sample handed over on)"""
    c = PATH_CASES[cid]
    out, t0 = [], 0
    for call in range(3):
        ns = call_samples(c, call) + c["offset"]
        if c["fmt"] == "sc16":
            x = sc16_iq(ns, 9400 + 10 * c["log2n"] + call, sigma=3000.0, tone=(8000.0, 0.123 + 0.01 * call))
            x32 = widen(x).reshape(-1, 2)
        else:
            x, x32 = as_format(add_tone(gaussian_iq(ns, 9400 + 10 * c["log2n"] + call), 0.05, 0.0313 + 0.01 * call, t0=t0),
                               c["fmt"])
        t0 += ns
        x32 = x32[c["offset"]:]
        x.setflags(write=False); x32.setflags(write=False)
        out.append((x, x32))
    return out


def oracle_call(o, case, call, x32, nthreads=8):
    """the oracle's statement of one call: one display launch per batch over the materialised (overlap_cc-expanded) windows"""
    n = 1 << case["log2n"]
    hop, batch = n // case["overlap"], case["spectra"][call]
    for k in range(case["n_batches"]):
        if case["overlap"] == 1:
            e = x32[k * batch * n:(k + 1) * batch * n]
        else:
            e = np.concatenate([x32[(k * batch + i) * hop:(k * batch + i) * hop + n] for i in range(batch)])
        assert o.process(e, strict=False, nthreads=nthreads) == 0


# ---- 3. sharded frames (tests/shard_emul.py's case form): signed_sparse, then ramp --------------------------------------------
SHARD_CASES = {
    "n8192":  dict(log2n=13, fmt="fp32", n_bins=512, wf_rows=WF_ROWS, total=64, overlap=1, frames=2, shards=[(0, 48), (48, 16)],
                   env={}, power=(-40, 5), seed=9501, twin=False),
    "n65536": dict(log2n=16, fmt="fp16", n_bins=512, wf_rows=WF_ROWS, total=32, overlap=1, frames=2, shards=[(0, 16), (16, 16)],
                   env={}, power=(-46, 5), seed=9502, twin=False),
}
SHARD_WINDOWS = ("signed_sparse", "ramp")		# frame 0, frame 1

# ---- 4. table changes between relaxed calls ---------------------------------------------------------------------------------
# four calls of 4 batches x 16 spectra, cut into 2 pieces of 2 batches each; at N = 8192 an instance has one FFT stream unless
# FOSPHOR_AMD_K1_STREAMS says otherwise: with 2 the pieces alternate between them.  N = 65536: one fused kernel at a time, one stream
RELAXED_CASES = {
    "n8192_1stream":  dict(log2n=13, n_bins=512, fmt="fp32", env={"FOSPHOR_AMD_SUB_LOG2": "18"}),
    "n8192_2streams": dict(log2n=13, n_bins=512, fmt="fp32", env={"FOSPHOR_AMD_SUB_LOG2": "18", "FOSPHOR_AMD_K1_STREAMS": "2"}),
    "n65536":         dict(log2n=16, n_bins=512, fmt="fp16", env={"FOSPHOR_AMD_SUB_LOG2": "21"}),
}
RELAXED_BATCHES, RELAXED_BATCH = 4, 16
RELAXED_WINDOWS = {0: "ramp", 1: "signed_sparse", 3: None}	# set before call k (None: set_fft_window_default)
RELAXED_POWER = {2: (-10, 5)}

# every knob a case may set; cleared before a case's instance is made
KNOBS = ("FOSPHOR_AMD_K1", "FOSPHOR_AMD_TILE", "FOSPHOR_AMD_SUB_LOG2", "FOSPHOR_AMD_K1_STREAMS", "FOSPHOR_AMD_OVERLAP",
         "FOSPHOR_AMD_ALT", "FOSPHOR_AMD_PIPE3", "FOSPHOR_AMD_ROWMASK", "FOSPHOR_AMD_K1W_SHARE")
