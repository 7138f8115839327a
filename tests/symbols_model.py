"""numpy statement of rules 1-6 of include/fosphor_amd_symbols.h and the input sets the CPU and GPU tests share.

A case is (iq, jobs): iq float32 [n][2] as it lies in memory and jobs a JOB_DTYPE array whose reserved output ranges are placed
with GUARD complex samples before, between and behind them (place()).  The twiddles are read through fosphor_amd_symbols_twiddles:
they are data of the contract, not recomputed here; the angle is demod_model.atan2_turns, the numpy statement of the pinned
fosphor_amd_atan2_turns.  Every operation is one IEEE double operation that numpy rounds once, in the order of the header's
parentheses.  The ordered sums are cumsum from an explicit 0.0, never np.sum; a block or a tile that a job ends in is filled up with
+0.0, which leaves a running sum that began at +0.0 as it is (it is never -0.0, and NaN + 0.0 is NaN).  A NaN float is 0x7fc00000,
a NaN double of the record 0x7ff8000000000000."""
import numpy as np

import demod_model as dm
from _pkg import gr_fosphor_amd
from measure_model import EXTRACT_DTYPE			# noqa: F401  (the chain's extract jobs)

JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("sps", "<i4"), ("mode", "<i4"), ("tau", "<f4"),
                      ("reserved", "<i4", (2,))])
RECORD_DTYPE = np.dtype([("n_sym", "<i4"), ("first", "<i4"), ("tau", "<f4"), ("status", "<i4"), ("mu", "<f8"), ("x_re", "<f8"),
                         ("x_im", "<f8"), ("a0", "<f8"), ("m2", "<f8"), ("m4", "<f8"), ("z2_re", "<f8"), ("z2_im", "<f8"),
                         ("z4_re", "<f8"), ("z4_im", "<f8")])
STATS = ("calls", "k_fold", "k_time", "k_pick", "k_record", "jobs_estimate", "jobs_fixed", "samples", "symbols")
MAX_JOBS, MIN_SPS, MAX_SPS, BLOCK, TILE, STAGE_SPS = 4096, 2, 64, 64, 4096, 8
ESTIMATE, FIXED = 0, 1
MODES = {"estimate": ESTIMATE, "fixed": FIXED}
OK, NO_TIMING = 0, 1
STATUS = {"ok": OK, "no_timing": NO_TIMING}
RECORD_WORDS = RECORD_DTYPE.itemsize // 4
GUARD = 3						# sentinel complex samples before, between and behind the jobs' reserved ranges
QNAN = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]
QNAN64 = np.frombuffer(np.uint64(0x7ff8000000000000).tobytes(), np.float64)[0]

_TW = {}


def twiddles(sps):
    """the table of rule 2 through fosphor_amd_symbols_twiddles: (re, im) float64 [sps] each"""
    if sps not in _TW:
        gr_fosphor_amd.load()
        t = gr_fosphor_amd.Fosphor.symbols_twiddles(sps)
        _TW[sps] = (np.ascontiguousarray(t.real), np.ascontiguousarray(t.imag))
    return _TW[sps]


def quiet(v):
    v = np.array(v, np.float32)
    v[np.isnan(v)] = QNAN
    return v


def quiet64(v):
    v = np.array(v, np.float64)
    v[np.isnan(v)] = QNAN64
    return v


def max_out(n, sps):
    return 0 if n < 4 else (n - 4) // sps + 1


def job_max_out(job):
    return max_out(int(job["n"]), int(job["sps"]))


def ordered_sum(terms, axis=0):
    """the sum over one axis in ascending order from 0.0 (cumsum adds one element after the other)"""
    terms = np.moveaxis(np.asarray(terms, np.float64), axis, 0)
    with np.errstate(all="ignore"):
        return np.cumsum(np.concatenate([np.zeros((1,) + terms.shape[1:]), terms]), axis=0)[-1]


def _fill(terms, to):
    pad = -len(terms) % to
    return np.concatenate([terms, np.zeros((pad,) + terms.shape[1:])]) if pad else terms


def three_level(terms):
    """the order of rules 1 and 6 over axis 0 of [N][K] float64 -> [K]: blocks of 64, tiles of 64 blocks, the job"""
    terms = np.asarray(terms, np.float64)
    K = terms.shape[1]
    if len(terms) == 0:
        return np.zeros(K)
    blocks = ordered_sum(_fill(terms, BLOCK).reshape(-1, BLOCK, K), axis=1)
    tiles = ordered_sum(_fill(blocks, BLOCK).reshape(-1, BLOCK, K), axis=1)
    return ordered_sum(tiles, axis=0)


def line(y, sps):
    """rules 1 and 2 over float32 y [n][2] -> (Xr, Xi, a0) as float64 scalars"""
    R = len(y) // sps
    re, im = y[:R * sps, 0].astype(np.float64), y[:R * sps, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        return line_of(three_level(((re * re) + (im * im)).reshape(R, sps)), sps)


def line_of(A, sps):
    """rule 2 over the folded sums A [sps] -> (Xr, Xi, a0)"""
    twr, twi = twiddles(sps)
    with np.errstate(all="ignore"):
        return ordered_sum(A * twr), ordered_sum(A * twi), ordered_sum(A)


def phase(xr, xi):
    """rule 3 -> e as a float64, or None: no timing"""
    a = dm.atan2_turns(-np.float64(xi), np.float64(xr))
    if np.isnan(a):
        return None
    e = np.float64(a)
    if e < 0.0:
        e = e + np.float64(1.0)
    if not e < 1.0:
        e = np.float64(0.0)
    return e + np.float64(0.0)


def place_of(e, n, sps):
    """rule 4 -> (first, mu, n_sym)"""
    base = np.float64(e) * np.float64(sps)
    i0 = int(np.floor(base))
    mu = base - np.float64(i0)
    first = i0 if i0 >= 1 else sps
    return first, mu, (0 if n - 3 - first < 0 else (n - 3 - first) // sps + 1)


def coefficients(mu):
    """rule 5 -> (c_1, c0, c1, c2)"""
    mu = np.float64(mu)
    u, b, c = mu + 1.0, mu - 1.0, mu - 2.0
    return -(((mu * b) * c) / 6.0), ((u * b) * c) / 2.0, -(((u * mu) * c) / 2.0), ((u * mu) * b) / 6.0


def interpolate(y, first, mu, n_sym, sps):
    """rule 5 over float32 y [n][2] -> float32 [n_sym][2]"""
    g = first + np.arange(n_sym, dtype=np.int64) * sps
    c = coefficients(mu)
    y = y.astype(np.float64)
    with np.errstate(all="ignore"):
        s = (((c[0] * y[g - 1]) + (c[1] * y[g])) + (c[2] * y[g + 1])) + (c[3] * y[g + 2])
        return quiet(s.astype(np.float32))


def moments(s32):
    """rule 6 over float32 [n_sym][2] -> float64 [6]: m2, m4, z2 re, z2 im, z4 re, z4 im"""
    sr, si = s32[:, 0].astype(np.float64), s32[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        w = (sr * sr) + (si * si)
        ar, ai = (sr * sr) - (si * si), (sr * si) + (sr * si)
        return three_level(np.stack([w, w * w, ar, ai, (ar * ar) - (ai * ai), (ar * ai) + (ar * ai)], 1))


MOMENTS = ("m2", "m4", "z2_re", "z2_im", "z4_re", "z4_im")


def timing_of(job, xyz):
    """rules 3 and 4 of a job whose line is xyz = (Xr, Xi, a0), None under FIXED -> a RECORD_DTYPE array [1] that lacks only the
    moments; status NO_TIMING where there is no phase"""
    r = np.zeros(1, RECORD_DTYPE)
    e = np.float64(np.float32(job["tau"]))
    if int(job["mode"]) == ESTIMATE:
        r["x_re"], r["x_im"], r["a0"] = quiet64(xyz[0]), quiet64(xyz[1]), quiet64(xyz[2])
        e = phase(xyz[0], xyz[1])
        if e is None:
            r["status"], r["tau"] = NO_TIMING, QNAN
            return r
    first, mu, n_sym = place_of(e, int(job["n"]), int(job["sps"]))
    r["n_sym"], r["first"], r["tau"], r["mu"] = n_sym, first, np.float32(e), mu
    return r


def symbols_job(iq, job):
    """-> (a RECORD_DTYPE array [1], the job's symbols float32 [n_sym][2])"""
    n, sps = int(job["n"]), int(job["sps"])
    y = iq[int(job["offset"]):int(job["offset"]) + n]
    r = timing_of(job, line(y, sps) if int(job["mode"]) == ESTIMATE else None)
    if r["status"][0] == NO_TIMING:
        return r, np.zeros((0, 2), np.float32)
    out = interpolate(y, int(r["first"][0]), r["mu"][0], int(r["n_sym"][0]), sps)
    for k, v in zip(MOMENTS, moments(out)):
        r[k] = quiet64(v)
    return r, out


def buffer(case):
    return np.ascontiguousarray(case[0], np.float32).reshape(-1, 2)


def symbols(case):
    """(records RECORD_DTYPE [n_jobs], [symbols per job, float32 [n_sym][2]])"""
    iq = buffer(case)
    both = [symbols_job(iq, j) for j in case[1]]
    return np.concatenate([b[0] for b in both]), [b[1] for b in both]


def capacity(jobs):
    """complex samples of the output buffer of a case: the last reserved sample and GUARD behind it"""
    return max([int(j["out_offset"]) + job_max_out(j) for j in jobs] + [0]) + GUARD


_IMAGES = {}


def image(case, fill, key=None):
    """(records, the whole output buffer as the model leaves it: uint32 [capacity][2], `fill` wherever no job writes -- the
    reserved samples behind a job's n_sym included); with a key the result is computed once for all the tests of a session"""
    if key is not None and (key, fill) in _IMAGES:
        return _IMAGES[(key, fill)]
    jobs = case[1]
    records, outs = symbols(case)
    out = np.full((capacity(jobs), 2), fill, np.uint32)
    for j, v in zip(jobs, outs):
        out[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v.view(np.uint32)
    if key is not None:
        _IMAGES[(key, fill)] = (records, out)
    return records, out


# ---- the builders ---------------------------------------------------------------------------------------------------------------

def make_jobs(rows):
    """rows of (offset, out_offset, n, sps, mode, tau)"""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    for j, r in zip(jobs, rows):
        j["offset"], j["out_offset"], j["n"], j["sps"], j["mode"], j["tau"] = r
    return jobs


def place(rows):
    """rows of (offset, n, sps, mode, tau) -> jobs whose reserved ranges follow each other with GUARD or GUARD + 1 samples between
    them, so that odd and even out_offsets both occur"""
    out, at = [], GUARD
    for i, (off, n, sps, mode, tau) in enumerate(rows):
        out.append((off, at, n, sps, mode, tau))
        at += max_out(n, sps) + GUARD + (i & 1)
    return make_jobs(out)


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * np.exp(rng.uniform(-1.0, 1.0, (n, 1)))).astype(np.float32)


def pulses(n, sps, delay, seed, depth=0.5):
    """noise whose envelope swings with the period sps and peaks `delay` samples behind sample 0: an input with a line"""
    env = 1.0 + depth * np.cos(2.0 * np.pi * (np.arange(n) - delay) / sps)
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0.0, 2.0 * np.pi, n)
    return (np.stack([np.cos(ph), np.sin(ph)], 1) * env[:, None]).astype(np.float32)


SPS = (2, 3, 4, 5, 8, 16, 63, 64)


def n_for(n_sym, first, sps, extra=0):
    """the n that gives n_sym symbols from `first` on, plus `extra` < sps samples that change nothing"""
    return 3 + first + (n_sym - 1) * sps + extra if n_sym > 0 else 2 + first


def loads_case():
    """every sps of SPS under FIXED and (from 3 on) under ESTIMATE; offsets 0 .. 3, so both parities against both parities of
    out_offset; a few symbols and a few hundred; the last job ends on the buffer's last sample"""
    rows, i = [], 0
    total = 64 * 300 + 7
    for sps in SPS:
        for mode in (FIXED, ESTIMATE):
            if mode == ESTIMATE and sps < 3:
                continue
            for n in (5 * sps + 3 + i % 3, 290 * sps + 5):
                tau = ((i * 7) % 16) / 16.0 if mode == FIXED else 0.0
                rows.append((i % 4, n, sps, mode, tau))
                i += 1
    rows.append((total - 1000, 1000, 5, ESTIMATE, 0.0))
    rows.append((total - 999, 999, 4, FIXED, 0.3))
    return pulses(total, 5, 1.7, 10), place(rows)


FOLD_COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 5)


def fold_case():
    """ESTIMATE at sps 3 with n / sps of FOLD_COUNTS and n not a multiple of sps; n / sps = 65 at sps 64; 4097 at sps 5 and at
    sps 16 (a piece of 12 and of 4 blocks); the offsets of both parities"""
    rows = [(i % 4, 3 * c + 1 + (i & 1), 3, ESTIMATE, 0.0) for i, c in enumerate(FOLD_COUNTS)]
    rows += [(1, 64 * 65 + 63, 64, ESTIMATE, 0.0), (2, 64 * 64, 64, ESTIMATE, 0.0), (3, 5 * 4097 + 4, 5, ESTIMATE, 0.0),
             (0, 16 * 4097 + 1, 16, ESTIMATE, 0.0), (1, 63 * 129 + 62, 63, ESTIMATE, 0.0), (2, 33 * 70, 33, ESTIMATE, 0.0)]
    longest = max(r[0] + r[1] for r in rows)
    return pulses(longest, 3, 0.8, 20) + noise(longest, 21) * np.float32(0.01), place(rows)


PICK_COUNTS = (0, 1, 63, 64, 65, 4096, 4097)


def pick_case():
    """FIXED, so that n_sym does not hang on an estimate: n_sym of PICK_COUNTS with the span staged (sps 4, first 2) and read
    directly (sps 16, first 9); n = 3, 4 and sps + 3; the pair of n at which g + 2 == n - 1 holds and just fails"""
    rows, i = [], 0
    for sps, tau, first in ((4, 0.5, 2), (16, 0.5625, 9), (3, 0.5, 1), (9, 0.5, 4)):
        for c in PICK_COUNTS:
            if sps in (3, 9) and c > 65:
                continue
            rows.append((i % 4, n_for(c, first, sps, extra=i % sps if c else 0), sps, FIXED, tau))
            i += 1
        for n in (3, 4, sps + 3, n_for(70, first, sps), n_for(70, first, sps) - 1):
            rows.append((i % 4, n, sps, FIXED, tau))
            i += 1
    longest = max(r[0] + r[1] for r in rows)
    return noise(longest, 30), place(rows)


def phase_fixed_case():
    """FIXED: tau = 0, where i0 = 0 and symbol 0 is dropped; a tau whose base is a whole number, where mu = 0 and the symbols are
    input samples; tau = 0.99999994, the largest; a tau of -0.0"""
    rows, i = [], 0
    for sps in (2, 4, 5, 16, 64):
        for tau in (0.0, 1.0 / sps, 0.5, 0.99999994, -0.0, 0.3):
            rows.append((i % 4, 40 * sps + i % 5, sps, FIXED, tau))
            i += 1
    longest = max(r[0] + r[1] for r in rows)
    return noise(longest, 40), place(rows)


def phase_estimate_case():
    """ESTIMATE at sps 4, where the table is exact and X is a difference of two sums.  Jobs of one symbol: A[k] = |y[k]|^2.
      0  a constant envelope: X = 0, a = -0, e = 0
      1  A0 > A2, A1 == A3: Xi = +0, a = -0
      2  A2 > A0, A1 == A3: a = -0.5, e = 0.5
      3  A2 >> A0, A1 a little above A3: a rounds to +0.5
      4  A0 = 2^40, A3 - A1 = 2^-52: a = -2^-92 / 2 pi, e + 1.0 rounds to 1.0 and goes to 0
      5  a small negative a that stays: e just below 1
    and the same six from an odd offset; a NaN sample and an inf sample in a long job
    (NO_TIMING, nothing written), each beside a job that does not see it; a NaN in the samples behind the last whole symbol,
    which the fold does not read and the interpolation does"""
    one = np.zeros((6, 4, 2), np.float32)
    one[0, :, 0] = 1.5
    one[1, :, 0] = (2.0, 1.0, 0.5, 1.0)
    one[2, :, 0] = (0.5, 1.0, 2.0, 1.0)
    one[3, :, 0] = (2.0 ** -20, 1.0 + 2.0 ** -12, 2.0 ** 20, 1.0)
    one[4, :, 0] = (2.0 ** 20, 1.0, 0.0, 1.0)
    one[4, 3, 1] = 2.0 ** -26
    one[5, :, 0] = (2.0, 1.0, 0.0, 1.001)
    parts, rows, at = [], [], 0
    for rep in range(2):
        for k in range(6):
            parts.append(np.concatenate([np.zeros((rep, 2), np.float32), one[k], np.float32(0.25) * noise(3, 50 + k)]))
            rows.append((at + rep, 7 - rep, 4, ESTIMATE, 0.0))
            at += len(parts[-1])
    y = pulses(3000, 4, 1.3, 51)
    y[700, 1] = np.nan
    y[1900, 0] = np.inf
    y[2999, 0] = np.nan
    parts.append(y)
    rows += [(at + 1, 1000, 4, ESTIMATE, 0.0), (at + 100, 500, 4, ESTIMATE, 0.0), (at + 1500, 1000, 3, ESTIMATE, 0.0),
             (at + 1000, 800, 5, ESTIMATE, 0.0), (at + 2000, 1000, 7, ESTIMATE, 0.0), (at + 600, 300, 4, FIXED, 0.4)]
    return np.concatenate(parts), place(rows)


def numbers_case():
    """subnormal samples; samples of 1e30 (the fourth moments reach 1e240); +-3e38 alternating so that the interpolated float
    overflows to inf and the moments to inf and NaN; under both modes"""
    iq = noise(4000, 60)
    iq[0:1000] = (noise(1000, 61) * np.float32(1e-41)).astype(np.float32)
    iq[1000:2000] = noise(1000, 62) * np.float32(1e30)
    iq[2000:3000, 0] = np.float32(3e38) * np.where((np.arange(1000) // 2) % 2, 1.0, -1.0).astype(np.float32)
    iq[2000:3000, 1] = np.float32(-3e38)
    rows = []
    for lo in (0, 1000, 2000):
        rows += [(lo + 1, 998, 4, ESTIMATE, 0.0), (lo, 1000, 4, FIXED, 0.375), (lo + 2, 900, 5, FIXED, 0.5), (lo, 999, 3, ESTIMATE, 0.0)]
    return iq, place(rows)


def mixed_case(count=41, seed=77, total=9000):
    """one call with both modes, every sps of SPS and jobs without a symbol in between; the input ranges overlap"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(count):
        sps = SPS[i % len(SPS)]
        mode = FIXED if sps == 2 or i % 3 == 0 else ESTIMATE
        n = int(rng.integers(0, 4)) if i % 7 == 3 else int(rng.integers(sps + 3, min(total, 150 * sps)))
        rows.append((int(rng.integers(0, total - n + 1)), n, sps, mode, float(np.float32(rng.uniform(0.0, 0.999))) if mode == FIXED else 0.0))
    return pulses(total, 4, 2.2, seed + 1), place(rows)


def full_table_case(modes=(ESTIMATE, FIXED)):
    """MAX_JOBS jobs in shuffled order, the modes and sps mixed, every 11th with n = 0: the deepest search of both prefixes"""
    rng = np.random.default_rng(4096 + len(modes) + modes[0])
    rows, total = [], 5000
    for i in rng.permutation(MAX_JOBS):
        i = int(i)
        mode = modes[i % len(modes)]
        sps = SPS[i % len(SPS)] if mode == FIXED else SPS[1 + i % (len(SPS) - 1)]
        n = 0 if i % 11 == 0 else sps + 3 + (i // 4) % (3 * sps + 40)
        rows.append((int(rng.integers(0, total - n + 1)), n, sps, mode, ((i * 13) % 64) / 64.0 if mode == FIXED else 0.0))
    return pulses(total, 4, 0.6, 90), place(rows)


def cases():
    """name -> (iq, jobs): every set the CPU and GPU tests share"""
    return {"loads": loads_case(), "fold": fold_case(), "pick": pick_case(), "phase_fixed": phase_fixed_case(),
            "phase_estimate": phase_estimate_case(), "numbers": numbers_case(), "mixed": mixed_case(),
            "full_table": full_table_case(), "only_fixed": full_table_case((FIXED,)), "only_estimate": full_table_case((ESTIMATE,))}


def expected_stats(jobs, records):
    """the stats delta of one call over jobs whose records are known"""
    est = jobs["mode"] == ESTIMATE
    fold = any(int(j["n"]) // int(j["sps"]) > 0 for j in jobs[est])
    pick = any(job_max_out(j) > 0 for j in jobs)
    return dict(calls=1, k_fold=int(fold), k_time=1, k_pick=int(pick), k_record=1, jobs_estimate=int(est.sum()),
                jobs_fixed=int((~est).sum()), samples=int(jobs["n"].sum()), symbols=int(records["n_sym"].sum()))


# ---- linear modulation for the tests of function ------------------------------------------------------------------------------

def raised_cosine(t, beta):
    """the raised-cosine pulse at t symbols"""
    t = np.asarray(t, np.float64)
    den = 1.0 - (2.0 * beta * t) ** 2
    safe = np.where(np.abs(den) < 1e-9, 1.0, den)
    p = np.sinc(t) * np.cos(np.pi * beta * t) / safe
    return np.where(np.abs(den) < 1e-9, np.pi / 4.0 * np.sinc(1.0 / (2.0 * beta)), p)


def modulate(sym, sps, delay, beta, lead=8, span=12):
    """complex128 samples of the symbols `sym` through a raised-cosine pulse of +-span symbols; symbol j sits (lead + j + delay) sps
    samples behind sample 0"""
    n = (len(sym) + 2 * lead) * sps
    m = np.arange(n)[:, None]
    y = np.zeros(n, np.complex128)
    for lo in range(0, len(sym), 64):
        j = np.arange(lo, min(lo + 64, len(sym)))[None, :]
        t = m / sps - (lead + j + delay)
        y += (np.where(np.abs(t) <= span, raised_cosine(t, beta), 0.0) * sym[None, lo:lo + 64]).sum(1)
    return y
