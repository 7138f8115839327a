"""Signals that appear, move and vanish: the scenario table of the persistence (merge) tests, its input builders and the walker that
counts, on the ORACLE's state, the transitions a scenario is there to provoke.

A scenario is a list of calls on one instance.  A call names the entry point, n_batches, batch and a signal segment; the segments
are deterministic and built from a few primitives (below).  The levels are what matter: from one call to the next the occupied dB
bins move by more than the width of the occupied band (the noise levels are 50 dB apart, the band of white noise is ~35 dB wide at
the tails and ~15 dB where the bulk of the hits is), so rows empty out rather than wobble; signals vanish for long enough to decay
below the 0.01 fast-exit level (display.cl:237-238) and come back.

Constants.  e = (1 - hc/(batch t0r) - 1/t0d)^batch is what a cell keeps per batch (display.cl:241-247).  With no hits and
t0d = batch / 4 that is (1 - 4/batch)^batch <= e^-4 = 0.018: a cell at its plateau (<= 1) is below 0.01 after two silent batches,
whatever the batch.  Every scenario therefore sets t0d = batch / 4 of its usual batch (at least 4) and t0r = 2 (a cell that takes a
tenth of a column's hits plateaus at 0.05 t0d / (0.05 t0d + 1), well above 0.01).  Where few batches can be afforded (P2, P3, P7, P9)
t0d = batch / 8: e^-8 = 3.4e-4 takes every cell below 0.01 in ONE silent batch, and none is left near 0.01 at a compare point (at
batch / 4 the oracle showed 57 000 cells of P3 inside |h - 0.01| < 2e-4: the cells whose plateau is about 0.55).

Which form runs where.  tests/test_persistence_cases_cpu.py runs EVERY scenario through the oracle alone and asserts the walker's
floors and the band population there, within CPU_BUDGET samples in all.  `cpu: True` scenarios run in full.  The others run in a
REDUCED form (reduced() below): the same calls, batches, segments, seeds and constants on an oracle of fewer columns -- FFT length
2^cpu_log2n instead of 2^log2n.  What happens to a histogram cell depends on the hit counts of its column only, and a column's hit
counts on the level in its FFT output: the oracle's bin offset moves the level of white noise by 10 log10(N) dB with the FFT
length, so the reduced form raises db_ref by round(10 log10(N / N_reduced)) and the same dB bins are occupied (measured: MID noise
at (-40, 5) sits at bin 22.1 of 128 at N = 8192 and at 22.7 / 22.0 at N = 64 / 16 with the shifted range).  The floors on CELLS
are fractions and hold as they are; the floors on ROWS (100 at N = 65536, where a bin has 1024 rows) scale with the rows per bin:
ceil(100 N_reduced / 65536).  tests/test_gpu_persistence.py walks the full-size scenarios with the same walker and asserts the
unscaled floors on the oracle's state as well.
"""
import numpy as np

from oracle_lib import Oracle

SAMPLE_BYTES = {"fp32": 8, "fp16": 4, "sc16": 4}
DEVICE_BUDGET = 6 << 30		# bytes a scenario may need on the device (P7: 3 x 1040 spectra at N = 65536 take 3.3 GiB of bin indices and FFT scratch) ...
HOST_BUDGET = 6 << 30		# ... and on the host (P7: a call of 204 Mi samples; the largest call's stream, its fp32 form, the oracle's FFT output and state copies)
CPU_BUDGET = 64 << 20		# complex samples the oracle takes in the whole CPU module
GPU_BUDGET = 2 << 30		# ... and in the whole of tests/test_gpu_persistence.py
RANDOM_SAMPLES = 88 << 20	# what the random call sequences of the GPU module may put through the oracle (asserted there)
KNOBS = ("FOSPHOR_AMD_SUB_LOG2", "FOSPHOR_AMD_ROWMASK", "FOSPHOR_AMD_OVERLAP", "FOSPHOR_AMD_NO_SUM16", "FOSPHOR_AMD_FRAME_GROUP",
         "FOSPHOR_AMD_TILE", "FOSPHOR_AMD_ALT", "FOSPHOR_AMD_K1_STREAMS", "FOSPHOR_AMD_PIPE3")

# ---- signal primitives ------------------------------------------------------------------------------------------------------------
# Levels in units of full scale.  HI / LO noise are 50 dB apart; fp16 holds LO (3e-4 sigma: above its subnormals) and sc16 holds it
# as ~10 counts.
HI, MID, LO = 0.1, 0.006, 0.0003
A = ("noise", HI)
B = ("noise", LO)
M = ("noise", MID)
Z = ("silence",)


def _gauss(rng, n_samples, sigma):
    return rng.standard_normal((n_samples, 2), dtype=np.float32) * np.float32(sigma)


def build_segment(seg, n_samples, n, rng, t0=0, hop=None):
    """float32 [n_samples][2] of a segment (built in double where phases or an inverse FFT are involved):
      ("noise", sigma)                   white Gaussian noise
      ("tone", amp, freq, sigma)         a tone of `freq` cycles per sample over noise
      ("bintone", amp, k)                a tone exactly on FFT bin k, nothing else
      ("burst", sigma, c0, c1, floor)    noise confined to FFT outputs [c0, c1) of every N-sample window, over a noise floor
      ("silence",)                       exact zeros
      ("const", v)                       re = im = v
      ("clip",)                          the negative rail: -1.0 (sc16: every word -32768)
      ("seq", [(n_spectra, seg), ...])   segments one after the other, n_spectra hops (N samples without overlap) each; the last
                                         takes what is left"""
    kind = seg[0]
    if kind == "noise":
        return _gauss(rng, n_samples, seg[1])
    if kind in ("tone", "bintone"):
        amp, freq = (seg[1], seg[2]) if kind == "tone" else (seg[1], seg[2] / float(n))
        x = _gauss(rng, n_samples, seg[3]) if kind == "tone" else np.zeros((n_samples, 2), dtype=np.float32)
        ph = 2.0 * np.pi * freq * np.arange(t0, t0 + n_samples, dtype=np.float64)
        x[:, 0] += (amp * np.cos(ph)).astype(np.float32)
        x[:, 1] += (amp * np.sin(ph)).astype(np.float32)
        return x
    if kind == "burst":
        _, sigma, c0, c1, floor = seg
        n_win = (n_samples + n - 1) // n
        spec = np.zeros((n_win, n), dtype=np.complex128)
        g = rng.standard_normal((n_win, c1 - c0, 2)) * (sigma * np.sqrt(n))
        spec[:, c0:c1] = g[..., 0] + 1j * g[..., 1]
        t = np.fft.ifft(spec, axis=1).reshape(-1)[:n_samples]
        return np.stack([t.real, t.imag], axis=1).astype(np.float32) + _gauss(rng, n_samples, floor)
    if kind == "silence":
        return np.zeros((n_samples, 2), dtype=np.float32)
    if kind == "const":
        return np.full((n_samples, 2), seg[1], dtype=np.float32)
    if kind == "clip":
        return np.full((n_samples, 2), -1.0, dtype=np.float32)
    if kind == "seq":
        out, at = np.empty((n_samples, 2), dtype=np.float32), 0
        for i, (cnt, sub) in enumerate(seg[1]):
            ln = n_samples - at if i == len(seg[1]) - 1 else min(cnt * (hop or n), n_samples - at)
            out[at:at + ln] = build_segment(sub, ln, n, rng, t0 + at, hop)
            at += ln
        assert at == n_samples
        return out
    raise ValueError("unknown segment %r" % (seg,))


def to_format(x, fmt):
    """(array handed to the library, float32 [samples][2] the oracle sees) of float32 samples in units of full scale"""
    if fmt == "sc16":
        q = np.clip(np.rint(x * np.float32(32768.0)), -32768, 32767).astype(np.int16)
        return q.reshape(-1), q.astype(np.float32) * np.float32(2.0 ** -15)
    if fmt == "fp16":
        h = x.astype(np.float16)
        return h, h.astype(np.float32)
    return x, x


# ---- the table --------------------------------------------------------------------------------------------------------------------

def call(ep, nb, batch, seg, cmp=False):
    return dict(ep=ep, nb=nb, batch=batch, seg=seg, cmp=cmp)


def _pd(nb, batch, seg, cmp=False):
    return call("process_device", nb, batch, seg, cmp)


def _frame(batch, seg, cmp=False):
    return call("accumulate", 1, batch, seg, cmp)


def _degenerate(ep, sizes, kinds):
    """P9: a whole batch of each degenerate input at each size, each followed by noise and then silence again (16 spectra each)"""
    calls = []
    for kind in kinds:
        for b in sizes:
            calls.append(call(ep, 1, b, kind, True))
            calls.append(call(ep, 1, 16, M))
            calls.append(call(ep, 1, 16, Z, True))
    return calls


TONE_FS = ("bintone", 32767.0 / 32768.0, 37)
DEGENERATE_SC = [Z, ("const", 0.25), ("clip",), TONE_FS]

# forms: the merge_stats counters that must have grown at the end; every other form counter must be 0.  mem:
# how many of the long-batch launches read the table from memory (0 or "all").  smax: (least, exact) largest number of batches in
# one sparse launch.  FOSPHOR_AMD_SUB_LOG2 is raised where a call would otherwise be cut into sub-launches of 64 Mi samples (1 Gi at
# N = 8192), each with a merge launch of its own.  band: the largest population of |h - 0.01| < 2e-4 over the scenario's
# compare points, as the oracle gives it (printed and asserted by the CPU module or, for cpu: False, by the GPU module): 0
# everywhere -- under these constants a cell steps from its plateau to below 3 % of it in one silent batch.
SCENARIOS = {
    # dense <0>: launches of 1, 5, 8 and 13 batches (its 1-, 4+1-, 8- and 8+4+1-step loops)
    "P1": dict(log2n=10, fmt="fp32", n_bins=256, wf_rows=64, overlap=1, consts=(2.0, 16.0, 0.01), power=(0, 10), env={}, seed=8101,
               cpu=True, forms={"dense16"}, band=0,
               calls=[_pd(1, 64, A), _pd(5, 64, B, True), _pd(8, 64, A), _pd(13, 64, Z, True), _pd(1, 1024, B), _pd(5, 64, A, True),
                      _pd(8, 64, ("seq", [(128, B), (128, Z), (256, A)]), True), _pd(13, 64, ("seq", [(320, M), (512, Z)]), True),
                      call("process", 1, 64, A, True)]),
    # dense <3>, table in LDS: launches of 1..4 batches (four cells in flight) and of 5..7 (general loop, 4-step tail + single steps)
    "P2": dict(log2n=13, fmt="fp32", n_bins=512, wf_rows=64, overlap=2, consts=(2.0, 130.0, 0.01), power=(-40, 5), env={}, seed=8102,
               cpu=False, cpu_log2n=6, forms={"dense16_long4", "dense16_long"}, mem=0, band=0,
               calls=[call("process_device_overlap", 1, 1040, A), call("process_device_overlap", 3, 1040, B, True),
                      call("process_device_overlap", 5, 1040, ("seq", [(1040, A), (4160, B)]), True),
                      call("process_device_overlap", 2, 2048, Z, True),
                      call("process_device_overlap", 7, 1040, ("seq", [(1040, B), (4160, Z), (2080, A)]), True)]),
    # dense <3>, table in memory: 4112 spectra is the smallest batch whose 4113 table entries do not fit the 4097 of LDS
    "P3": dict(log2n=13, fmt="fp32", n_bins=512, wf_rows=64, overlap=1, consts=(2.0, 514.0, 0.01), power=(-40, 5), env={}, seed=8103,
               cpu=False, cpu_log2n=6, forms={"dense16_long4", "dense16_long"}, mem="all", band=0,
               calls=[_pd(2, 4112, A, True), _pd(5, 4112, ("seq", [(4112, B), (12336, Z), (4112, M)]), True),
                      _pd(2, 4112, ("seq", [(4112, A), (4112, Z)]), True)]),
    # <1> (frames of 2048 spectra: 32-bit sums, table) and <2> (16384 spectra: beyond the table)
    "P4": dict(log2n=10, fmt="fp32", n_bins=256, wf_rows=64, overlap=1, consts=(2.0, 256.0, 0.01), power=(0, 10), env={}, seed=8104,
               cpu=False, cpu_log2n=6, forms={"table32", "eval32"}, band=0,
               calls=[_frame(2048, A), _frame(2048, B), _frame(16384, B, True), _frame(2048, B, True), _frame(2048, A, True),
                      _frame(2048, Z, True), _frame(2048, Z, True), _frame(2048, A, True)]),
    # ... the frequency-sliced merge: 4 ranks, each holding the whole frame's partials and merging its quarter of the cells
    "P4s": dict(log2n=10, fmt="fp32", n_bins=256, wf_rows=64, overlap=1, consts=(2.0, 256.0, 0.01), power=(0, 10), env={}, seed=8114,
                cpu=True, world=4, forms={"table32"}, band=0,
                calls=[call("merge_sliced", 1, 2048, A), call("merge_sliced", 1, 2048, B), call("merge_sliced", 1, 2048, B, True),
                       call("merge_sliced", 1, 2048, B, True), call("merge_sliced", 1, 2048, A, True)]),
    # sparse <0, true>, pipelined branch (1 and 2 batches per launch)
    "P5": dict(log2n=16, fmt="fp16", n_bins=128, wf_rows=64, overlap=1, consts=(2.0, 4.0, 0.01), power=(0, 10), env={}, seed=8105,
               cpu=True, forms={"sparse16"}, smax=(1, 2), band=0,
               calls=[_pd(1, 16, A), _pd(2, 16, B), _pd(1, 16, B, True), _pd(1, 32, B, True), _pd(2, 16, ("seq", [(16, A), (16, Z)]), True),
                      _pd(1, 64, Z), _pd(2, 16, Z, True), _pd(1, 16, A, True),
                      _pd(2, 16, ("seq", [(16, ("burst", HI, 4096, 12288, LO)), (16, ("tone", HI, 0.123, LO))]), True),
                      _pd(1, 16, B), _pd(1, 16, B, True)]),
    # sparse <0, true>, general branch: 3..11 batches (bits carried by the list), 12..64 (one round of row masks), > 64 (two rounds)
    "P6": dict(log2n=16, fmt="fp16", n_bins=64, wf_rows=64, overlap=1, consts=(2.0, 4.0, 0.01), power=(0, 10),
               env={"FOSPHOR_AMD_SUB_LOG2": "27"}, seed=8106, cpu=False, cpu_log2n=10, forms={"sparse16"}, smax=(65, 66), band=0,
               calls=[_pd(3, 16, ("seq", [(16, A), (32, B)]), True),
                      _pd(11, 16, ("seq", [(16, B), (48, Z), (32, A), (48, B), (32, A)]), True),
                      _pd(12, 16, ("seq", [(64, B), (64, A), (64, Z)]), True),
                      _pd(66, 16, ("seq", [(48, A), (64, B), (48, Z), (16, A), (64, Z), (64, B), (64, A), (64, Z), (624, B)]), True),
                      _pd(2, 16, A, True)]),
    # sparse <3, true>: batches of 1040 spectra, 1 and 3 per launch
    "P7": dict(log2n=16, fmt="sc16", n_bins=128, wf_rows=64, overlap=1, consts=(2.0, 130.0, 0.01), power=(0, 10),
               env={"FOSPHOR_AMD_SUB_LOG2": "28"}, seed=8107,
               cpu=False, cpu_log2n=8, forms={"sparse16_long"}, mem="all", smax=(3, 3), band=0,
               calls=[_pd(1, 1040, A, True), _pd(3, 1040, ("seq", [(1040, B), (2080, Z)]), True), _pd(1, 1040, A, True)]),
    # path switches: sparse merges, a sharded frame whose signal sits in other rows (hot flags dropped), sparse merges again
    "P8": dict(log2n=16, fmt="fp16", n_bins=128, wf_rows=64, overlap=1, consts=(2.0, 4.0, 0.01), power=(0, 10), env={}, seed=8108,
               cpu=True, forms={"sparse16", "table32"}, smax=(1, 2), band=0,
               calls=[_pd(1, 16, A), _pd(1, 16, A, True), _frame(16, B, True), _pd(1, 16, Z, True), _pd(2, 16, Z, True), _frame(16, A, True),
                      _pd(1, 16, B, True), _frame(16, Z), _frame(16, Z, True), _pd(2, 16, ("seq", [(16, A), (16, B)]), True)]),
    # degenerate input: hc == batch.  (At N = 1024 a single batch above 1024 spectra is not counted as one chunk -- that needs 128
    # slabs in the launch -- so P9a's long batches go through the 32-bit table form; P9b's 8192 and P9c's 1040 take the 16-bit long
    # forms with the table in memory.)
    "P9a": dict(log2n=10, fmt="sc16", n_bins=256, wf_rows=64, overlap=1, consts=(2.0, 128.0, 0.01), power=(0, 10), env={}, seed=8109,
                cpu=False, cpu_log2n=6, forms={"dense16", "table32"}, degenerate=True, band=0,
                calls=_degenerate("process_device", (1024, 4096, 8192), DEGENERATE_SC)),
    "P9b": dict(log2n=13, fmt="sc16", n_bins=512, wf_rows=64, overlap=1, consts=(2.0, 128.0, 0.01), power=(-40, 5), env={}, seed=8110,
                cpu=False, cpu_log2n=6, forms={"dense16", "dense16_long4"}, mem="all", degenerate=True, band=0,
                calls=_degenerate("process_device", (1024, 8192), DEGENERATE_SC)),
    "P9c": dict(log2n=16, fmt="sc16", n_bins=128, wf_rows=64, overlap=1, consts=(2.0, 128.0, 0.01), power=(0, 10), env={}, seed=8111,
                cpu=False, cpu_log2n=8, forms={"sparse16", "sparse16_long"}, mem="all", smax=(1, 1), degenerate=True, band=0,
                calls=_degenerate("process_device", (1024, 1040), DEGENERATE_SC)),
    # the frame path with silence inside a frame: the -inf powers go through the weighted tile partials of the live sum
    "P10": dict(log2n=10, fmt="fp32", n_bins=256, wf_rows=64, overlap=1, consts=(2.0, 1024.0, 0.002), power=(0, 10), env={}, seed=8112,
                cpu=False, cpu_log2n=4, forms={"eval32"}, degenerate=True, band=0,
                calls=[_frame(65536, ("seq", [(32768, Z), (32768, M)]), True), _frame(65536, ("seq", [(49152, M), (16384, Z)]), True)]),
}


def n_of(s):
    return 1 << s["log2n"]


def call_spectra(c):
    return c["nb"] * c["batch"]


def call_stream_samples(s, c):
    n = n_of(s)
    return (call_spectra(c) - 1) * (n // s["overlap"]) + n


def oracle_samples(s):
    """complex samples the oracle takes for one run of the scenario"""
    return sum(call_spectra(c) for c in s["calls"]) * n_of(s)


def capacity(s):
    """(max_spectra, max_batches) the scenario's instance is made with: the tightest that accepts every call"""
    return max(call_spectra(c) for c in s["calls"]), max(max(c["nb"] for c in s["calls"]), 2)


def scenario_bytes(s):
    """(device bytes, host bytes) upper bounds, after shard_emul.case_bytes: per instance two sets of hit-count slots and the export
    view, histogram, two waterfall rings, count slabs, four sets of 16-bit bin indices, the N = 65536 scratch spectrum, chunk
    partials; the largest call's stream"""
    n, nb = n_of(s), s["n_bins"]
    max_spectra, max_batches = capacity(s)
    cells = nb * n
    inst = 4 * cells * (max_batches + 2) + 2 * 4 * s["wf_rows"] * n + 2 * cells * (max_spectra // 1024 + 1)
    inst += 4 * 2 * max_spectra * n + 8 * (max_spectra // 16 + 1) * n
    if s["log2n"] == 16:
        inst += 8 * max_spectra * n
    biggest = max(call_stream_samples(s, c) for c in s["calls"])
    dev = inst * s.get("world", 1) + biggest * SAMPLE_BYTES[s["fmt"]]
    # host: the call's stream as float32, one part of it being built, its fp16 / sc16 form, the overlap-expanded copy; the oracle's
    # FFT output of one batch (in and out); copies of the oracle's histogram and counts
    host = biggest * (8 + 8 + (SAMPLE_BYTES[s["fmt"]] if s["fmt"] != "fp32" else 0)) * (2 if s["overlap"] > 1 else 1)
    host += 2 * max(c["batch"] for c in s["calls"]) * n * 8 + 8 * 4 * cells
    return dev, host


def make_call_input(s, idx):
    """(array for the library, float32 [samples][2] of the unexpanded stream) of call idx"""
    c = s["calls"][idx]
    rng = np.random.default_rng(s["seed"] * 100 + idx)
    x = build_segment(c["seg"], call_stream_samples(s, c), n_of(s), rng, t0=idx * 4099, hop=n_of(s) // s["overlap"])
    return to_format(x, s["fmt"])


def reduced(s):
    """the form of a scenario the CPU module walks: s itself, or its calls on an oracle of 2^cpu_log2n columns (module docstring)"""
    if s["cpu"]:
        return s
    shift = int(round(10.0 * np.log10(float(1 << s["log2n"]) / (1 << s["cpu_log2n"]))))
    n_red = 1 << s["cpu_log2n"]
    return dict(s, log2n=s["cpu_log2n"], power=(s["power"][0] + shift, s["power"][1]), rows=s["log2n"] == 16,
                row_floor=-(-100 * n_red // 65536) if s["log2n"] == 16 else None)


def make_oracle(s):
    o = Oracle(fft_len_log=s["log2n"], n_bins=s["n_bins"], wf_rows=s["wf_rows"])
    o.set_power_range(*s["power"])
    o.set_constants(*s["consts"])
    return o


def expand(s, x32):
    n, ov = n_of(s), s["overlap"]
    if ov == 1:
        return x32
    hop = n // ov
    n_win = (x32.shape[0] - n) // hop + 1
    return np.concatenate([x32[i * hop:i * hop + n] for i in range(n_win)])


# ---- the walker -------------------------------------------------------------------------------------------------------------------

class Walk:
    """Feeds an oracle the calls of a scenario batch by batch and counts what happens to the histogram cells (and, at N = 65536, to
    the rows of 64 aligned columns of one bin that the sparse merge lists, flags and skips):
      a  was > 0.01 before the call, got no hit in the call, ends <= 0.01          (decays through the fast-exit level)
      b  was <= 0.01 and not 0 before the call, got no hit, keeps its bits         (stays frozen)
      c  was <= 0.01 and not 0 before the call and is hit in the call              (frozen, hit again)
      stale  (rows, per batch) the row is hot, has no hit in this batch and had hits in the previous batch of the instance: the
             sparse hand-off leaves the previous counts of such a row in memory
    `used` = cells (rows) that hold a hit anywhere in the scenario."""

    def __init__(self, s, threads):
        self.s, self.o, self.threads = s, make_oracle(s), threads
        self.n, self.nb = n_of(s), s["n_bins"]
        self.rows = s.get("rows", s["log2n"] == 16)
        self.row_floor = s.get("row_floor") or 100
        self.cell = dict(a=0, b=0, c=0)
        self.row = dict(a=0, b=0, c=0, stale=0)
        self.used = np.zeros((self.nb, self.n), dtype=bool)
        self.prev_row_hit = None
        self.full = []			# batches (size, segment kind, max count, every column sums to the batch)
        self.bands = []			# population of |h - 0.01| < 2e-4 at the compare points
        self.samples = 0
        self.alive_rows = None

    def _rows(self, m):
        return m.reshape(self.nb, self.n // 64, 64)

    def call(self, idx, x32):
        """the oracle through call idx, whose unexpanded stream is x32"""
        s, o, c = self.s, self.o, self.s["calls"][idx]
        ex = expand(s, x32)
        per = c["batch"] * self.n
        assert ex.shape[0] == c["nb"] * per
        h0 = o.histogram
        hit = np.zeros((self.nb, self.n), dtype=bool)
        h = h0
        for k in range(c["nb"]):
            assert o.process(ex[k * per:(k + 1) * per], strict=False, nthreads=self.threads) == 0
            self.samples += per
            hc = o.hitcount.T
            self.full.append((c["batch"], c["seg"][0], int(hc.max()), bool(np.all(hc.sum(0, dtype=np.int64) == c["batch"]))))
            hb = hc > 0
            hit |= hb
            if self.rows:
                row_hit = self._rows(hb).any(2)
                if self.prev_row_hit is not None:
                    hot = self._rows(h > 0.01).any(2)
                    self.row["stale"] += int((hot & ~row_hit & self.prev_row_hit).sum())
                self.prev_row_hit = row_hit
                if k < c["nb"] - 1:
                    h = o.histogram
        h1 = o.histogram
        self.used |= hit
        frozen0 = (h0 <= 0.01) & (h0 != 0)
        same = h1.view(np.uint32) == h0.view(np.uint32)
        self.cell["a"] += int(((h0 > 0.01) & ~hit & (h1 <= 0.01)).sum())
        self.cell["b"] += int((frozen0 & ~hit & same).sum())
        self.cell["c"] += int((frozen0 & hit).sum())
        if self.rows:
            r_hot0, r_hot1 = self._rows(h0 > 0.01).any(2), self._rows(h1 > 0.01).any(2)
            r_frozen0 = ~r_hot0 & self._rows(h0 != 0).any(2)
            r_hit, r_same = self._rows(hit).any(2), self._rows(same).all(2)
            self.alive_rows = int((r_hot0 | r_hit).sum())	# what a sparse launch over this call lists when its hot flags are valid
            self.row["a"] += int((r_hot0 & ~r_hit & ~r_hot1).sum())
            self.row["b"] += int((r_frozen0 & ~r_hit & r_same).sum())
            self.row["c"] += int((r_frozen0 & r_hit).sum())
        if c["cmp"]:
            self.bands.append(int((np.abs(h1 - 0.01) < 2e-4).sum()))

    def report(self, sid):
        used = int(self.used.sum())
        line = "%s: %d cells used; cells a/b/c %d/%d/%d" % (sid, used, self.cell["a"], self.cell["b"], self.cell["c"])
        if self.rows:
            line += "; rows a/b/c/stale %d/%d/%d/%d" % (self.row["a"], self.row["b"], self.row["c"], self.row["stale"])
        line += "; band |h - 0.01| < 2e-4 at the compare points: %s (max %d)" % (self.bands, max(self.bands or [0]))
        return line

    def assert_floors(self, sid):
        """the conditions on the INPUTS: the scenario does what it is there for"""
        s = self.s
        if s.get("degenerate"):
            # every spectrum of a silent, constant or clipped batch is the same spectrum: each kind must fill ONE bin of a column
            for b, kind in sorted({(c["batch"], c["seg"][0]) for c in s["calls"]
                                   if c["seg"][0] in ("silence", "const", "clip") and c["batch"] > 16}):
                assert any(sz == b and kd == kind and mx == b for sz, kd, mx, _ in self.full), \
                    "%s: no cell with hc == batch in the %s batch of %d" % (sid, kind, b)
            assert all(ok for _, _, _, ok in self.full), "%s: a column's counts do not sum to the batch" % sid
            return
        floor = int(self.used.sum()) // 100 + 1
        for k in "abc":
            assert self.cell[k] >= floor, "%s: transition %s in %d cells, floor %d (1 %% of the used cells)" % (sid, k, self.cell[k], floor)
        if self.rows:
            for k in ("a", "b", "c", "stale"):
                assert self.row[k] >= self.row_floor, "%s: row transition %s %d times, floor %d" % (sid, k, self.row[k], self.row_floor)
        assert all(ok for _, _, _, ok in self.full), "%s: a column's counts do not sum to the batch" % sid
