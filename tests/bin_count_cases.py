"""Inputs of the bin-count tests: data shared by tests/test_bin_counts_cpu.py, which checks the inputs and the oracle without a
GPU, and tests/test_gpu_bin_counts.py, which runs the kernels against them.

n_bins is no passive size on the device: it selects the index format (8-bit, 16-bit, low bytes + a plane of 9th bits, 9-bit
packing), a kernel instantiation of its own at 256, the size of the count kernel's LDS histogram and of its row bitmask, and
every division by n_bins * 32 / n_bins * 64 in the merge kernels.  COUNTS are the counts on either side of each of these seams.

One stream per FFT length serves every count: band-stopped Gaussian noise plus a tone.  The power range spans 20 dB around the
noise, so that
  * the noise's own spread (|X|^2 is exponentially distributed: a long tail downwards) fills every row 0 .. n_bins - 1,
  * the tone's column and the noise's peaks lie above the last row (the upper clamp),
  * the columns inside the stop band hold window side lobes only and lie below row 0 (the lower clamp).
RANGES was chosen on the CPU from the oracle's waterfall; tests/test_bin_counts_cpu.py asserts what it is chosen for."""
import functools

import numpy as np

from oracle_lib import Oracle

COUNTS = [16, 48, 240, 256, 272, 496, 512]
# minimum, half a mask word | no multiple of 32 | either side of the index-format switch and of the n_bins == 256
# instantiation, the 9th bit in 16 rows only | the largest below 512 | the anchor against the existing tests

WF_ROWS = 64
MAX_SPECTRA = {10: 64, 13: 64, 16: 32}
FMT = {10: "fp32", 13: "fp32", 16: "fp16"}		# the float format of a length (fp16 at 65536 points, as the existing tests there)
SC16_COUNT = {10: 48, 13: 272, 16: 496}			# the one odd count per length that also runs from int16 samples

# calls of a whole-path case: (entry point, n_batches, batch, overlap).  Every length has a multi-batch call; 8192 points has
# the overlapped read; the last call of 1024 / 8192 points fills the 64-row ring exactly, the calls before it leave it at 48 / 64
CALLS = {
    10: [("host", 1, 48, 1), ("device", 2, 16, 1), ("device", 1, 64, 1)],
    13: [("device", 1, 32, 2), ("device", 2, 16, 1), ("device", 1, 64, 1)],
    16: [("device", 1, 16, 1), ("device", 2, 16, 1)],
}

SIGMA, TONE_AMP, TONE_FREQ = 0.05, 0.15, 0.0313
STOP_BAND = (0.30, 0.34)				# normalised frequency: 4 % of the columns (41 at 1024 points)
RANGES = {10: (-47, 2), 13: (-56, 2), 16: (-67, 2)}	# (db_ref, db_per_div): 20 dB that end about 4 dB above the noise's mean power


def call_samples(log2n, call):
    _, nbat, batch, overlap = call
    n = 1 << log2n
    return (nbat * batch - 1) * (n // overlap) + n


@functools.lru_cache(maxsize=None)
def base_stream(log2n):
    """float64 [samples][2] for all the calls of a length, one after the other: white complex Gaussian noise of unit variance per
    component with STOP_BAND removed over the whole stream (so that any window of it sees the same stop band), plus the tone"""
    ns = sum(call_samples(log2n, c) for c in CALLS[log2n])
    rng = np.random.default_rng(8800 + log2n)
    z = rng.standard_normal(ns) + 1j * rng.standard_normal(ns)
    Z = np.fft.fft(z)
    f = np.fft.fftfreq(ns)
    Z[(f >= STOP_BAND[0]) & (f < STOP_BAND[1])] = 0
    z = np.fft.ifft(Z)
    z = z + (TONE_AMP / SIGMA) * np.exp(2j * np.pi * TONE_FREQ * np.arange(ns))
    return np.stack([z.real, z.imag], 1)


@functools.lru_cache(maxsize=None)
def streams(log2n, fmt):
    """per call of CALLS[log2n]: (array handed to the library, float32 [samples][2] of the same values for the oracle)"""
    s = base_stream(log2n) * SIGMA
    if fmt == "sc16":
        x = np.clip(np.rint(s * 32768.0), -32768, 32767).astype(np.int16)
        x32 = x.astype(np.float32) * np.float32(2.0 ** -15)
    elif fmt == "fp16":
        x = s.astype(np.float16)
        x32 = x.astype(np.float32)
    else:
        x = s.astype(np.float32)
        x32 = x
    out, at = [], 0
    for c in CALLS[log2n]:
        k = call_samples(log2n, c)
        out.append((x[at:at + k], x32[at:at + k]))
        at += k
    for a, b in out:
        a.setflags(write=False); b.setflags(write=False)
    return out


def make_oracle(log2n, n_bins):
    o = Oracle(fft_len_log=log2n, n_bins=n_bins, wf_rows=WF_ROWS)
    o.set_power_range(*RANGES[log2n])
    return o


def oracle_call(o, log2n, call, x32, nthreads=8):
    """the oracle's statement of one call: one display launch per batch over the materialised (overlap_cc-expanded) windows"""
    _, nbat, batch, overlap = call
    n = 1 << log2n
    hop = n // overlap
    for k in range(nbat):
        if overlap == 1:
            e = x32[k * batch * n:(k + 1) * batch * n]
        else:
            e = np.concatenate([x32[(k * batch + i) * hop:(k * batch + i) * hop + n] for i in range(batch)])
        assert o.process(e, strict=False, nthreads=nthreads) == 0


def assert_covers(hc, n_bins, what, every_row=True):
    """The condition on the input, on the oracle's counts [x][bin] of one launch or summed over a case's launches: hits in row 0
    and in the last row, in every row between (every_row: a 16-spectrum launch at 1024 points is too short for that at 512 bins),
    and -- above 256 bins -- at least 1 % of them on either side of row 256: a case that never sets the 9th index bit proves
    nothing about it."""
    rows = hc.sum(axis=0, dtype=np.uint64)
    assert rows[0] > 0 and rows[n_bins - 1] > 0, what
    if every_row:
        assert np.all(rows > 0), "%s: rows %s hold no hit" % (what, np.flatnonzero(rows == 0)[:8])
    if n_bins > 256:
        tot = float(rows.sum())
        lo, hi = rows[:256].sum() / tot, rows[256:].sum() / tot
        assert lo >= 0.01 and hi >= 0.01, "%s: rows < 256 hold %.4f, rows >= 256 hold %.4f of the hits" % (what, lo, hi)


def assert_clamps(o, n_rows, what):
    """both clamps occur in the newest n_rows rows of the oracle's ring: powers that round below row 0 and above the last row"""
    rows = (o.waterfall_pos - n_rows + np.arange(n_rows)) & (o.wf_rows - 1)
    v = np.float32(o.histo_scale) * (o.waterfall[rows] + np.float32(o.histo_offset))
    assert (v < -0.5).any() and (v > o.n_bins - 0.5).any(), what
