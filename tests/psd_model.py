"""numpy statement of rules 1-5 of include/fosphor_amd_psd.h and the input sets the CPU and GPU tests share.

A case is (iq, win, jobs): iq float32 [n][2] as it lies in memory, win the float32 buffer of windows, and jobs a JOB_DTYPE array whose
traces are placed with GUARD floats before, between and behind them (place()).  The twiddles and the windows are read through
fosphor_amd_psd_twiddles and fosphor_amd_psd_window: they are data of the contract, not recomputed here.  The FFT is vectorised per
stage over all segments of all jobs of one length; every operation is one IEEE double operation that numpy rounds once, in the
order of the header's parentheses.  The ordered sums are cumsum from an explicit 0.0 or Python loops, never np.sum.  A NaN float
is 0x7fc00000, a NaN double of the record 0x7ff8000000000000 (rule 4)."""
import numpy as np

from _pkg import gr_fosphor_amd
from measure_model import EXTRACT_DTYPE			# noqa: F401  (the chain's extract jobs)

JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("win_offset", "<i8"), ("n", "<i4"), ("fft_len_log", "<i4"),
                      ("hop", "<i4"), ("pre", "<i4"), ("trace", "<i4"), ("obw_fraction", "<f4"), ("xdb_ratio", "<f4"),
                      ("reserved", "<i4")])
RECORD_DTYPE = np.dtype([("n_seg", "<i4"), ("fft_len", "<i4"), ("peak_bin", "<i4"), ("peak_power", "<f4"), ("obw_lo", "<i4"),
                         ("obw_hi", "<i4"), ("xdb_lo", "<i4"), ("xdb_hi", "<i4"), ("total", "<f8"), ("m1", "<f8"), ("m2", "<f8"),
                         ("win_energy", "<f8")])
STATS = ("calls", "k_group", "k_wave", "k_combine", "jobs", "segments")
MAX_JOBS, MIN_LOG, MAX_LOG, TILE, BLOCKS = 4096, 6, 10, 32, 64
WAVE_MAX_LOG = 7						# L <= 128 is the WAVE form
LOGS = (6, 7, 8, 9, 10)
NONE, SQUARE, FOURTH, MAGSQ = 0, 1, 2, 3
PRES = {"none": NONE, "square": SQUARE, "fourth": FOURTH, "magsq": MAGSQ}
T_NONE, T_POWER = 0, 1
TRACES = {"none": T_NONE, "power": T_POWER}
RECT, HANN, BH = 0, 1, 2
WINDOWS = {"rect": RECT, "hann": HANN, "blackman_harris": BH}
GUARD = 3						# sentinel floats before, between and behind the jobs' traces
QNAN = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]
QNAN64 = np.frombuffer(np.uint64(0x7ff8000000000000).tobytes(), np.float64)[0]

_TW = []


def twiddles():
    """the table of rule 3 through fosphor_amd_psd_twiddles: (re, im) float64 [512] each"""
    if not _TW:
        gr_fosphor_amd.load()
        t = gr_fosphor_amd.Fosphor.psd_twiddles()
        _TW.extend([np.ascontiguousarray(t.real), np.ascontiguousarray(t.imag)])
    return _TW


def window(kind, log):
    gr_fosphor_amd.load()
    return gr_fosphor_amd.Fosphor.psd_window(kind, log)


def quiet(v):
    v = np.array(v, np.float32)
    v[np.isnan(v)] = QNAN
    return v


def quiet64(v):
    v = np.array(v, np.float64)
    v[np.isnan(v)] = QNAN64
    return v


def ordered_sum(terms):
    """the sum over axis 0 in ascending order from 0.0 (cumsum adds one row after the other)"""
    terms = np.asarray(terms, np.float64)
    return np.cumsum(np.concatenate([np.zeros((1,) + terms.shape[1:]), terms]), axis=0)[-1]


def n_seg(n, log, hop):
    L = 1 << log
    return 0 if n < L else (n - L) // hop + 1


def job_n_seg(job):
    return n_seg(int(job["n"]), int(job["fft_len_log"]), int(job["hop"]))


def n_out(job):
    return (1 << int(job["fft_len_log"])) if int(job["trace"]) == T_POWER and job_n_seg(job) > 0 else 0


def bitrev(log):
    i = np.arange(1 << log)
    r = np.zeros_like(i)
    for b in range(log):
        r |= ((i >> b) & 1) << (log - 1 - b)
    return r


def pre_of(pre, re, im, w):
    """rule 2: float32 re, im [S][L] and w [S][L] -> x as (float64 re, float64 im)"""
    re, im, w = re.astype(np.float64), im.astype(np.float64), w.astype(np.float64)
    pre = np.broadcast_to(np.asarray(pre).reshape(-1, 1), re.shape)
    with np.errstate(all="ignore"):
        sr, si = (re * re) - (im * im), (re * im) + (re * im)
        fr, fi = (sr * sr) - (si * si), (sr * si) + (sr * si)
        mr = (re * re) + (im * im)
        zr = np.where(pre == NONE, re, np.where(pre == SQUARE, sr, np.where(pre == FOURTH, fr, mr)))
        zi = np.where(pre == NONE, im, np.where(pre == SQUARE, si, np.where(pre == FOURTH, fi, 0.0)))
        return w * zr, w * zi


def fft(xr, xi):
    """rule 3 over [S][L] float64 -> (Xr, Xi)"""
    S, L = xr.shape
    log = L.bit_length() - 1
    twr, twi = twiddles()
    br = bitrev(log)
    ar, ai = np.ascontiguousarray(xr[:, br]), np.ascontiguousarray(xi[:, br])
    with np.errstate(all="ignore"):
        for t in range(1, log + 1):
            h = 1 << (t - 1)
            wr, wi = twr[np.arange(h) * (512 // h)], twi[np.arange(h) * (512 // h)]
            ar, ai = ar.reshape(S, L // (2 * h), 2, h), ai.reshape(S, L // (2 * h), 2, h)
            ur, ui, vr, vi = ar[:, :, 0], ai[:, :, 0], ar[:, :, 1], ai[:, :, 1]
            tr = (wr * vr) - (wi * vi)
            ti = (wr * vi) + (wi * vr)
            ar = np.stack([ur + tr, ur - tr], 2).reshape(S, L)
            ai = np.stack([ui + ti, ui - ti], 2).reshape(S, L)
    return ar, ai


def two_level(terms):
    """rule 5's order over [L] float64 -> (cum [L], the sum)"""
    L = len(terms)
    per = L // BLOCKS
    with np.errstate(all="ignore"):
        run = np.cumsum(np.concatenate([np.zeros((BLOCKS, 1)), terms.reshape(BLOCKS, per)], 1), 1)[:, 1:]
        base = np.cumsum(np.concatenate([[0.0], run[:, -1]]))		# base[0] = 0.0, base[k] = base[k - 1] + B[k - 1]
        return (base[:BLOCKS, None] + run).reshape(L), base[BLOCKS]


def record_of(P32, job, nseg, U):
    """rule 5 -> a RECORD_DTYPE array [1]"""
    L = 1 << int(job["fft_len_log"])
    r = np.zeros(1, RECORD_DTYPE)
    r["n_seg"], r["fft_len"], r["win_energy"] = nseg, L, quiet64(U)
    for k in ("peak_bin", "obw_lo", "obw_hi", "xdb_lo", "xdb_hi"):
        r[k] = -1
    if nseg == 0:
        return r
    P = P32.astype(np.float64)
    d = (np.arange(L) - L // 2).astype(np.float64)
    with np.errstate(all="ignore"):
        cum, total = two_level(P)
        m1, m2 = two_level(d * P)[1], two_level((d * d) * P)[1]
        r["total"], r["m1"], r["m2"] = quiet64(total), quiet64(m1), quiet64(m2)
        ok = ~np.isnan(P32)
        if ok.any():
            i = int(np.flatnonzero(P32 == P32[ok].max())[0])
            r["peak_bin"], r["peak_power"] = i, P32[i]
            level = np.float32(P32[i]) * np.float32(job["xdb_ratio"])
            at = np.flatnonzero(P32 >= level)
            if len(at):
                r["xdb_lo"], r["xdb_hi"] = at[0], at[-1]
        if np.isfinite(total) and total > 0.0:
            t = (np.float64(1.0) - np.float64(np.float32(job["obw_fraction"]))) * np.float64(0.5)
            lo_thr = total * t
            hi_thr = total - lo_thr
            lo, hi = np.flatnonzero(cum > lo_thr), np.flatnonzero(cum >= hi_thr)
            r["obw_lo"], r["obw_hi"] = (lo[0] if len(lo) else -1), (hi[0] if len(hi) else -1)
    return r


def buffers(case):
    return np.ascontiguousarray(case[0], np.float32).reshape(-1, 2), np.ascontiguousarray(case[1], np.float32).reshape(-1)


def powers(iq, win, start, woff, pre, L):
    """rules 2 and 3 and |X|^2 of the segments that begin at iq[start[s]] under the window at win[woff[s]] -> float64 [S][L]"""
    p = np.zeros((len(start), L))
    for a in range(0, len(start), 8192):					# bounded memory
        sl = slice(a, a + 8192)
        at = start[sl, None] + np.arange(L)
        xr, xi = pre_of(pre[sl], iq[at, 0], iq[at, 1], win[woff[sl, None] + np.arange(L)])
        Xr, Xi = fft(xr, xi)
        with np.errstate(all="ignore"):
            p[sl] = (Xr * Xr) + (Xi * Xi)
    return p


def result_of(job, S, win):
    """the end of rule 4 and rule 5: a job's S[b] (None without a segment) -> (a RECORD_DTYPE array [1], P32 or None)"""
    L = 1 << int(job["fft_len_log"])
    w = win[int(job["win_offset"]):int(job["win_offset"]) + L].astype(np.float64)
    with np.errstate(all="ignore"):
        U = ordered_sum(w * w)
    nseg = job_n_seg(job)
    P32 = None
    if nseg > 0:
        den = np.float64(nseg) * U
        with np.errstate(all="ignore"):
            S = np.roll(S, L // 2)						# P32[i] is bin (i + L / 2) mod L
            P32 = np.zeros(L, np.float32) if den == 0.0 else quiet((S / den).astype(np.float32))
    return record_of(P32, job, nseg, U), P32


def psd(case):
    """(records RECORD_DTYPE [n_jobs], [trace floats per job, float32 [0] or [L]], [P32 per job or None])"""
    iq, win = buffers(case)
    jobs = case[2]
    S_of = [None] * len(jobs)
    for log in LOGS:
        L = 1 << log
        idx = [i for i, j in enumerate(jobs) if int(j["fft_len_log"]) == log and job_n_seg(j) > 0]
        if not idx:
            continue
        counts = [job_n_seg(jobs[i]) for i in idx]
        start = np.concatenate([int(jobs[i]["offset"]) + np.arange(c, dtype=np.int64) * int(jobs[i]["hop"]) for i, c in zip(idx, counts)])
        woff = np.concatenate([np.full(c, int(jobs[i]["win_offset"]), np.int64) for i, c in zip(idx, counts)])
        pre = np.concatenate([np.full(c, int(jobs[i]["pre"])) for i, c in zip(idx, counts)])
        p = powers(iq, win, start, woff, pre, L)
        at = 0
        for i, c in zip(idx, counts):
            mine = p[at:at + c]
            at += c
            with np.errstate(all="ignore"):
                T = np.stack([ordered_sum(mine[s:s + TILE]) for s in range(0, c, TILE)])
                S_of[i] = ordered_sum(T)
    records, traces, P32s = [], [], []
    for i, j in enumerate(jobs):
        record, P32 = result_of(j, S_of[i], win)
        records.append(record)
        traces.append(P32 if P32 is not None and int(j["trace"]) == T_POWER else np.zeros(0, np.float32))
        P32s.append(P32)
    return np.concatenate(records), traces, P32s


def capacity(jobs):
    """floats of the output buffer of a case: the last trace float and GUARD behind it"""
    return max([int(j["out_offset"]) + n_out(j) for j in jobs] + [0]) + GUARD


_IMAGES = {}


def image(case, fill, key=None):
    """(records, the whole output buffer as the model leaves it: uint32 [capacity], `fill` wherever no job writes); with a key the
    result is computed once for all the tests of a session"""
    if key is not None and (key, fill) in _IMAGES:
        return _IMAGES[(key, fill)]
    jobs = case[2]
    records, traces, _ = psd(case)
    out = np.full(capacity(jobs), fill, np.uint32)
    for j, v in zip(jobs, traces):
        out[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v.view(np.uint32)
    if key is not None:
        _IMAGES[(key, fill)] = (records, out)
    return records, out


# ---- the builders ---------------------------------------------------------------------------------------------------------------

class Bank:
    """the window buffer of a case: at(log, kind, shift) is the offset of that window, placed on first use at an offset that is
    `shift` modulo 4"""

    def __init__(self):
        self.parts, self.size, self.where = [], 0, {}

    def at(self, log, kind, shift=0):
        key = (log, kind, shift)
        if key not in self.where:
            gap = (shift - self.size) % 4
            self.parts += [np.full(gap, 7.0, np.float32), window(kind, log)]		# a gap's floats belong to no window
            self.where[key] = self.size + gap
            self.size += gap + (1 << log)
        return self.where[key]

    def buffer(self):
        return np.concatenate(self.parts + [np.full(GUARD, 7.0, np.float32)])


def make_jobs(rows):
    """rows of (offset, out_offset, win_offset, n, fft_len_log, hop, pre, trace, obw_fraction, xdb_ratio)"""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    for j, r in zip(jobs, rows):
        (j["offset"], j["out_offset"], j["win_offset"], j["n"], j["fft_len_log"], j["hop"], j["pre"], j["trace"], j["obw_fraction"],
         j["xdb_ratio"]) = r
    return jobs


def place(rows):
    """rows of (offset, win_offset, n, log, hop, pre, trace, obw_fraction, xdb_ratio) -> jobs whose traces follow each other with
    GUARD or GUARD + 1 floats between them, so that odd and even out_offsets both occur; a job without a trace has out_offset 0"""
    out, at = [], GUARD
    for i, (off, woff, n, log, hop, pre, trace, obw, xdb) in enumerate(rows):
        out.append((off, at if trace else 0, woff, n, log, hop, pre, trace, obw, xdb))
        if trace:
            at += (1 << log if n_seg(n, log, hop) > 0 else 0) + GUARD + (i & 1)
    return make_jobs(out)


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * np.exp(rng.uniform(-1.0, 1.0, (n, 1)))).astype(np.float32)


def tone(n, cycles_per_sample, amp=1.0, phase=0.0):
    ph = 2.0 * np.pi * (cycles_per_sample * np.arange(n) + phase)
    return np.stack([amp * np.cos(ph), amp * np.sin(ph)], 1).astype(np.float32)


def loads_case():
    """every L with n = L - 1, L, L + hop - 1 and L + hop at hop 37; offset and win_offset walk 0 .. 3 in both parities against
    each other; the three windows; the traces alternate; the last job of each L ends on the buffer's last sample"""
    bank, rows, i = Bank(), [], 0
    total = 1024 + 37 + 3
    for log in LOGS:
        L = 1 << log
        for n in (L - 1, L, L + 36, L + 37):
            off = total - n if n == L + 37 else i % 4
            rows.append((off, bank.at(log, i % 3, (i // 4 + i) % 4), n, log, 37, NONE, (i + 1) % 2, 0.99, 1e-2))
            i += 1
    return noise(total, 10), bank.buffer(), place(rows)


SEG_COUNTS = (0, 1, 2, 31, 32, 33, 65, 3 * 32 + 5)


def tiles_case():
    """n_seg of SEG_COUNTS in both forms, the hops 1, 37, L / 2 and L among them"""
    bank, rows, i = Bank(), [], 0
    for log, hops in ((6, (1, 37, 32, 64)), (7, (1, 64)), (8, (1, 37, 128)), (10, (37,))):
        L = 1 << log
        for hop in hops:
            for c in SEG_COUNTS:
                if L * c > 40000 and hop > 64:
                    continue
                n = L - 1 - (i % 3) if c == 0 else L + (c - 1) * hop + (i % hop if hop > 1 else 0)
                rows.append((i % 4, bank.at(log, HANN, i % 4), n, log, hop, NONE, T_POWER if i % 4 else T_NONE, 0.99, 1e-3))
                i += 1
    rows.append((1, bank.at(9, BH, 1), 512 + 256 * 32, 9, 256, NONE, T_POWER, 0.99, 1e-3))		# 33 segments of 512 at L / 2
    rows.append((2, bank.at(10, RECT, 2), 1024 + 1024, 10, 1024, NONE, T_POWER, 0.99, 1e-3))	# 2 segments of 1024 at hop L
    longest = max(r[0] + r[2] for r in rows)
    return noise(longest, 20), bank.buffer(), place(rows)


def wave_tiles_case(tiles):
    """WAVE-form jobs whose tiles add up to 1, 3, 4 or 5: the last work-group of four tiles is partly filled"""
    bank = Bank()
    segs = {1: (5,), 3: (65,), 4: (33, 40), 5: (33, 0, 65)}[tiles]
    rows = [(i, bank.at(6 + (i & 1), HANN, (tiles + i) % 4), (64 << (i & 1)) + (c - 1) * 3 if c else 10, 6 + (i & 1), 3, NONE, T_POWER, 0.99, 0.1)
            for i, c in enumerate(segs)]
    return noise(128 + 64 * 3 + 8, 30 + tiles), bank.buffer(), place(rows)


def mixed_case():
    """one call with both forms, jobs without segments in between, all four pre modes, TRACE_NONE beside TRACE_POWER, the
    fractions 1.0, 0.99 and 0.5 and the ratios 1.0 and 1e-3; the input ranges overlap"""
    rng = np.random.default_rng(77)
    bank, rows = Bank(), []
    total = 6000
    iq = noise(total, 40) * np.float32(0.05) + tone(total, 0.11, 0.7) + tone(total, -0.2, 0.2)
    for i in range(41):
        log = LOGS[i % 5]
        L = 1 << log
        hop = (1, 37, L // 2, L)[(i // 5) % 4]
        n = int(rng.integers(0, L)) if i % 7 == 3 else int(rng.integers(L, min(total, L + 70 * hop)))
        rows.append((int(rng.integers(0, total - n + 1)), bank.at(log, i % 3, i % 4), n, log, hop, i % 4, T_NONE if i % 3 == 1 else T_POWER,
                     (1.0, 0.99, 0.5)[i % 3], (1.0, 1e-3)[i % 2]))
    return iq.astype(np.float32), bank.buffer(), place(rows)


IMPULSE_LOG = 10


def impulses_case():
    """x = delta[n] + delta[n - L / 2] under a rectangular window: X[b] = 1 + (-1)^b exactly, so P32 is 2^-8 (L = 1024) on
    every even trace index and 0 on every odd one.  The peak is a tie of L / 2 bins and the smallest index, 0, wins.  total =
    512 P, and with obw_fraction 0.5 lo_thr = total / 4 is met exactly by cum[254] = cum[255] and first exceeded at index 256, the
    first index of block 16 of rule 5: obw_lo = 256, where `>` and `>=` part; hi_thr = 3 total / 4 is met exactly at index 766.
    A single impulse gives a flat spectrum, a tie of all bins.  Then two bins alone: the same with x = 1 + (-1)^n (X is L at bins
    0 and L / 2) must give peak_bin 0 if the two are equal as floats, else the larger: the model decides, the device follows."""
    bank, rows = Bank(), []
    L = 1 << IMPULSE_LOG
    iq = np.zeros((5 * L + 8, 2), np.float32)
    iq[0, 0] = iq[L // 2, 0] = 1.0						# job 0: one segment
    iq[L, 0] = 1.0								# job 1: a single impulse
    iq[2 * L:3 * L:2, 0] = 2.0							# job 2: 1 + (-1)^n
    iq[3 * L + 3, 0] = iq[3 * L + 3 + 32, 0] = 1.0				# job 3: L = 64 from an odd offset
    for off, log, obw in ((0, IMPULSE_LOG, 0.5), (L, IMPULSE_LOG, 1.0), (2 * L, IMPULSE_LOG, 0.99), (3 * L + 3, 6, 0.5)):
        rows.append((off, bank.at(log, RECT, 1), 1 << log, log, 1 << log, NONE, T_POWER, obw, 1.0))
    return iq, bank.buffer(), place(rows)


def tones_case():
    """a tone on bin k under a rectangular window, every L: peak_bin = k + L / 2 (mod L) = obw_lo = obw_hi.  With SQUARE the line
    moves to 2 k, with FOURTH to 4 k.  At L = 1024 the trace indices 16 m and 16 m + 15 are the first and the last of a block of
    rule 5: the cumulative sum crosses both thresholds at that seam.  MAGSQ of a two-level envelope of period P: the peak is DC, the
    mean of |y|^2, and the largest bin beside it the line at +-L / P.  -> (case, the peak's bin per job, [(job, P)] of MAGSQ)"""
    bank, rows, parts, at, want, lines = Bank(), [], [], 0, [], []
    for log in LOGS:
        L = 1 << log
        for k, pre in ((5, NONE), (-7, NONE), (5, SQUARE), (3, FOURTH)):
            parts.append(tone(2 * L, k / L, 0.5))
            rows.append((at, bank.at(log, RECT, 0), 2 * L, log, L // 2, pre, T_POWER, 0.99, 1e-3))
            want.append((k * (1, 2, 4)[pre]) % L)
            at += 2 * L
    L = 1024
    for i in (16 * 40, 16 * 40 + 15, 16 * 3, 1023):
        k = i - L // 2
        parts.append(tone(L, k / L, 1.0))
        rows.append((at, bank.at(10, RECT, 0), L, 10, L, NONE, T_NONE, 0.99, 0.5))
        want.append(k % L)
        at += L
    for log, period in ((6, 8), (9, 4)):
        L = 1 << log
        env = np.where(np.arange(2 * L) % period < period // 2, 1.0, 0.25)
        parts.append(tone(2 * L, 0.123, 1.0) * env[:, None].astype(np.float32))
        rows.append((at, bank.at(log, RECT, 0), 2 * L, log, L, MAGSQ, T_POWER, 0.99, 1e-3))
        want.append(0)
        lines.append((len(rows) - 1, period))
        at += 2 * L
    return (np.concatenate(parts), bank.buffer(), place(rows)), want, lines


def silence_case():
    """silence: total == 0, every index -1 but the peak's (P32 is +0.0 everywhere, the largest number at index 0), a trace of
    +0.0f; and an all-zero window over noise: den == 0, the same"""
    bank = Bank()
    iq = noise(3000, 50)
    iq[100:2400] = 0.0
    rows = [(100, bank.at(6, HANN), 700, 6, 16, NONE, T_POWER, 0.99, 1e-3), (101, bank.at(8, BH, 1), 2000, 8, 128, SQUARE, T_POWER, 0.5, 1.0),
            (100, bank.at(10, RECT, 2), 2300, 10, 37, MAGSQ, T_NONE, 1.0, 1e-3)]
    zero_at = bank.size + GUARD
    buf = np.concatenate([bank.buffer(), np.zeros(256 + 2, np.float32)])
    rows += [(0, zero_at, 100, 6, 7, NONE, T_POWER, 0.99, 1e-3), (2, zero_at + 1, 700, 8, 100, FOURTH, T_POWER, 0.99, 1e-3)]
    return iq, buf, place(rows)


def nonfinite_case():
    """one NaN and one inf sample in one segment each of multi-tile jobs: the canonical NaNs appear, jobs beside them are not
    touched; +-3e38 with FOURTH overflows to inf and propagates; subnormal samples, and samples whose P32 is subnormal"""
    bank = Bank()
    iq = noise(9000, 60)
    iq[1500, 1] = np.nan							# in segments of jobs 0, 1
    iq[2600] = (np.inf, 1.0)							# in segments of jobs 0, 1, 2
    iq[5000:5200] = np.clip(noise(200, 61), -8.0, 8.0) * np.float32(3e38 / 8.0)
    iq[5003] = (3e38, -3e38)
    iq[6000:7100] = (noise(1100, 62) * np.float32(1e-41)).astype(np.float32)	# subnormal samples: P32 underflows to +0
    iq[7200:8300] = noise(1100, 63) * np.float32(1e-21)				# |y|^2 near 1e-42: P32 is subnormal
    rows = [(0, bank.at(6, HANN, 2), 64 + 69 * 50, 6, 50, NONE, T_POWER, 0.99, 1e-3),		# 70 segments, three tiles
            (1000, bank.at(8, BH, 1), 256 + 40 * 64, 8, 64, SQUARE, T_POWER, 0.99, 1e-3),	# 41 segments, two tiles
            (2590, bank.at(7, RECT, 2), 128 + 33 * 4, 7, 4, MAGSQ, T_NONE, 0.5, 1.0),
            (3000, bank.at(6, HANN, 2), 64 + 69 * 20, 6, 20, NONE, T_POWER, 0.99, 1e-3),		# beside them: finite
            (3000, bank.at(8, BH, 1), 256 + 40 * 32, 8, 32, FOURTH, T_POWER, 0.99, 1e-3),
            (5000, bank.at(6, RECT, 3), 200, 6, 8, FOURTH, T_POWER, 0.99, 1e-3),
            (5000, bank.at(7, HANN, 3), 200, 7, 8, NONE, T_POWER, 0.99, 1e-3),
            (5000, bank.at(6, RECT, 3), 200, 6, 8, SQUARE, T_POWER, 0.99, 1e-3),
            (6000, bank.at(6, HANN, 2), 1100, 6, 32, NONE, T_POWER, 0.99, 1e-3),
            (6001, bank.at(10, BH, 2), 1099, 10, 1, MAGSQ, T_POWER, 0.99, 1e-3),
            (6000, bank.at(8, RECT, 1), 1100, 8, 100, SQUARE, T_POWER, 0.5, 0.1),
            (7200, bank.at(6, HANN, 2), 1100, 6, 32, NONE, T_POWER, 0.99, 1e-3),
            (7201, bank.at(8, RECT, 1), 1099, 8, 37, NONE, T_POWER, 0.5, 0.5)]
    return iq, bank.buffer(), place(rows)


def full_table_case():
    """MAX_JOBS jobs of L = 64 and n = 64 .. 96 at hop 1 (1 .. 33 segments, one tile or two) in shuffled order, every 11th with
    n < L: the deepest search of the prefix"""
    rng = np.random.default_rng(4096)
    bank, rows = Bank(), []
    total = 5000
    order = rng.permutation(MAX_JOBS)
    for i in order:
        n = int(i) % 64 if i % 11 == 0 else 64 + (int(i) // 4) % 33
        rows.append((int(rng.integers(0, total - n + 1)), bank.at(6, int(i) % 3, int(i) % 4), n, 6, 1, int(i) % 4, int(i) % 2, 0.99, 1e-2))
    return noise(total, 90), bank.buffer(), place(rows)


def cases():
    """name -> (iq, win, jobs): every set the CPU and GPU tests share"""
    out = {"loads": loads_case(), "tiles": tiles_case(), "mixed": mixed_case(), "impulses": impulses_case(), "tones": tones_case()[0],
           "silence": silence_case(), "nonfinite": nonfinite_case(), "full_table": full_table_case()}
    for k in (1, 3, 4, 5):
        out["wave_tiles%d" % k] = wave_tiles_case(k)
    return out


# ---- the chain: extract -> psd ---------------------------------------------------------------------------------------------------

CHAIN_LOG = 6


def chain_jobs(F, ejobs, win_offset=0):
    """the psd jobs over what correlate_model.chain_case()'s extract job writes: the plain spectrum, and the fourth power, whose
    line for the QPSK preamble at the extraction's own centre is at DC"""
    plain = F.psd_jobs(ejobs, CHAIN_LOG, win_offset=win_offset, trace="power", xdb=-20.0)
    fourth = F.psd_jobs(ejobs, CHAIN_LOG, win_offset=win_offset, pre="fourth", trace="power", xdb=-3.0)
    fourth["out_offset"] += (1 << CHAIN_LOG) + GUARD
    return np.concatenate([plain, fourth])
