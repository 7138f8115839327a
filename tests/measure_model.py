"""numpy statement of include/fosphor_amd_measure.h, the bound on its sums, and the input sets the CPU and GPU tests share.

A case is (iq, jobs): iq float32 [n][2] as it lies in memory, jobs a JOB_DTYPE array.  The power p is float32 arithmetic as rule 1
writes it; the integers follow from it; every sum is math.fsum over its terms, each formed in float64 from the float32 values as
rule 3 forms them (where a term is not finite fsum has no meaning and the plain float64 sum stands in: rule 3 asks for IEEE
propagation there, not for a value)."""
import math

import numpy as np

JOB_DTYPE = np.dtype([("offset", "<i8"), ("n", "<i4"), ("threshold", "<f4")])
RECORD_DTYPE = np.dtype([("n_above", "<i4"), ("first_above", "<i4"), ("last_above", "<i4"), ("n_edges", "<i4"),
                         ("peak_index", "<i4"), ("peak_power", "<f4"), ("s_re", "<f8"), ("s_im", "<f8"), ("s_p", "<f8"),
                         ("s_p2", "<f8"), ("s_zz_re", "<f8"), ("s_zz_im", "<f8"), ("r1_re", "<f8"), ("r1_im", "<f8"),
                         ("n", "<i4"), ("form", "<i4")])
EXTRACT_DTYPE = np.dtype([("first", "<i8"), ("out_offset", "<i8"), ("n_out", "<i4"), ("decim", "<i4"), ("phase_inc", "<u4"),
                          ("phase0", "<u4"), ("taps_offset", "<i4"), ("n_taps", "<i4")])
INTS = ("n_above", "first_above", "last_above", "n_edges", "peak_index", "peak_power", "n", "form")
SUMS = ("s_re", "s_im", "s_p", "s_p2", "s_zz_re", "s_zz_im", "r1_re", "r1_im")
STATS = ("calls", "k_wave", "k_split", "k_combine", "jobs_wave", "jobs_split", "samples")
MAX_JOBS, WAVE_MAX, CHUNK = 4096, 4096, 8192
FORM_WAVE, FORM_SPLIT = 0, 1
GUARD = 2						# sentinel records before and behind the jobs' records (GPU tests)


def form(n):
    return FORM_WAVE if n <= WAVE_MAX else FORM_SPLIT


def power(y):
    """rule 1: float32 (re * re) + (im * im), three rounded operations"""
    y = np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        return (y[:, 0] * y[:, 0]) + (y[:, 1] * y[:, 1])


def terms(y):
    """field -> the float64 terms of its sum (rule 3)"""
    y = np.asarray(y, np.float32)
    re, im, p = y[:, 0].astype(np.float64), y[:, 1].astype(np.float64), power(y).astype(np.float64)
    with np.errstate(all="ignore"):
        return {"s_re": re, "s_im": im, "s_p": p, "s_p2": p * p, "s_zz_re": re * re - im * im, "s_zz_im": (2.0 * re) * im,
                "r1_re": re[1:] * re[:-1] + im[1:] * im[:-1], "r1_im": im[1:] * re[:-1] - re[1:] * im[:-1]}


def job_samples(iq, job):
    return np.asarray(iq, np.float32).reshape(-1, 2)[int(job["offset"]):int(job["offset"]) + int(job["n"])]


def measure_job(iq, job):
    y = job_samples(iq, job)
    n = len(y)
    r = np.zeros((), RECORD_DTYPE)
    r["n"], r["form"] = n, form(n)
    p = power(y)
    with np.errstate(all="ignore"):
        above = p >= np.float32(job["threshold"])
    idx = np.flatnonzero(above)
    r["n_above"] = len(idx)
    r["first_above"], r["last_above"] = (idx[0], idx[-1]) if len(idx) else (-1, -1)
    r["n_edges"] = int(np.count_nonzero(above & ~np.concatenate([[False], above[:-1]])))
    ok = ~np.isnan(p)
    if ok.any():
        r["peak_power"] = p[ok].max()
        r["peak_index"] = np.flatnonzero(ok & (p == r["peak_power"]))[0]
    else:
        r["peak_index"], r["peak_power"] = -1, 0.0
    for k, t in terms(y).items():
        with np.errstate(all="ignore"):
            r[k] = math.fsum(t) if np.isfinite(t).all() else t.sum()
    return r


def measure(iq, jobs):
    return np.array([measure_job(iq, j) for j in np.atleast_1d(jobs)], RECORD_DTYPE)


def job_tolerance(iq, job):
    """field -> n * 2^-52 * sum|term| (rule 3: (n - 1) * 2^-53 for n additions in any order, 2^-53 per term's own rounding, doubled)"""
    y = job_samples(iq, job)
    with np.errstate(all="ignore"):
        return {k: len(y) * 2.0 ** -52 * float(np.abs(t).sum()) for k, t in terms(y).items()}


def tolerance(case):
    """one dict per job of the case"""
    iq, jobs = case
    return [job_tolerance(iq, j) for j in jobs]


def assert_records(got, want, tols, tag=""):
    """got against the model's records: integers, peak, n and form equal; sums inside the tolerance, or not finite where the
    model's are not"""
    assert len(got) == len(want), tag
    for i, (g, w, tol) in enumerate(zip(got, want, tols)):
        for k in INTS:
            assert g[k] == w[k], (tag, i, k, g[k], w[k])
        for k in SUMS:
            if np.isfinite(w[k]):
                assert abs(float(g[k]) - float(w[k])) <= tol[k], (tag, i, k, float(g[k]), float(w[k]), tol[k])
            else:
                assert not np.isfinite(g[k]), (tag, i, k, float(g[k]), float(w[k]))


# ---- the input sets -------------------------------------------------------------------------------------------------------------

def make_jobs(rows):
    """rows of (offset, n, threshold)"""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    for j, r in zip(jobs, rows):
        j["offset"], j["n"], j["threshold"] = r
    return jobs


def bursty(n, seed):
    """Gaussian samples under an envelope that steps between 0.1 and 1 in runs of 1 .. 40 samples: a threshold of 0.3 sees many
    runs, most samples near it on neither side"""
    rng = np.random.default_rng(seed)
    runs = rng.integers(1, 41, n // 8 + 2)
    env = np.repeat(np.where(np.arange(len(runs)) % 2 == 0, 0.1, 1.0), runs)[:n]
    return (rng.standard_normal((n, 2)) * env[:, None]).astype(np.float32)


def wave_n_case():
    """the lengths at the seams of a wave's loop, at offsets 0, 1, 2, 3, ...; the last job ends on the buffer's last sample"""
    ns = (0, 1, 2, 63, 64, 65, 127, 128, 129, WAVE_MAX - 1, WAVE_MAX)
    total = WAVE_MAX + 16
    rows = [(i, n, 0.3) for i, n in enumerate(ns)] + [(total - 129, 129, 0.3), (total - 1, 1, 0.3), (total, 0, 0.3)]
    return bursty(total, 1), make_jobs(rows)


def wave_offset_case():
    """the 16-byte boundary: even and odd lengths from offsets 0, 1, 2, 3; the buffer ends with the last job"""
    rows = [(off, n, 0.3) for off in (0, 1, 2, 3) for n in (300, 301)]
    total = 3 + 301
    return bursty(total, 2), make_jobs(rows + [(total - 300, 300, 0.3), (total - 301, 301, 0.3)])


def wave_count_case(count):
    """four jobs per work-group: 1, 3, 4, 5 jobs"""
    return bursty(700, 10 + count), make_jobs([(7 * i + (i & 1), 200 + 31 * i, 0.3) for i in range(count)])


def split_n_case():
    """the lengths at the seams of the SPLIT form, each at an even and an odd offset"""
    ns = (WAVE_MAX + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 3 * CHUNK + 5)
    total = 3 * CHUNK + 5 + 3
    rows = [(off, n, 0.3) for n in ns for off in (2, 3)]
    rows[-1] = (total - ns[-1], ns[-1], 0.3)				# odd offset, ends on the buffer's last sample
    assert rows[-1][0] % 2 == 1
    return bursty(total, 3), make_jobs(rows)


def planted_case():
    """quiet noise (p around 2e-4) with, relative to each job's sample 0: a run above the threshold over the boundary of chunks 0
    and 1 that holds the maximum twice, at CHUNK - 1 and CHUNK (the smaller index wins across chunks); a rising edge exactly at a
    chunk's first sample, 2 * CHUNK; the same maximum twice more in chunk 2, the second as a run of one; one sample above, last of all.  The jobs: the whole
    at an even and an odd offset, and WAVE jobs over the first run where the maximum is attained twice, lanes apart."""
    rng = np.random.default_rng(4)
    n = 3 * CHUNK + 5
    base = (rng.standard_normal((n, 2)) * 0.01).astype(np.float32)
    big, top = np.float32([0.75, -0.5]), np.float32([1.5, 0.25])
    base[CHUNK - 3:CHUNK + 3] = big
    base[CHUNK - 1] = base[CHUNK] = top
    base[2 * CHUNK:2 * CHUNK + 70] = big
    base[2 * CHUNK + 40] = base[2 * CHUNK + 105] = top				# the second one stands alone, 65 samples on
    base[n - 1] = big
    even = n + 3 + ((n + 3) & 1)					# the second copy's offset; the first lies at 1
    iq = np.zeros((even + n, 2), np.float32)
    iq[1:1 + n] = base
    iq[even:even + n] = base
    rows = [(1, n, 0.5), (even, n, 0.5),
            (1 + 2 * CHUNK - 10, 200, 0.5), (even + 2 * CHUNK, 70, 0.5),	# WAVE: edge inside, and above from sample 0 on
            (1 + CHUNK - 100, 200, 0.5)]					# WAVE: the maximum twice, in neighbouring lanes
    rows.append((even + 2 * CHUNK, 300, 0.5))				# WAVE: the maximum twice, other lanes and rounds of the loop apart
    return iq, make_jobs(rows)


def mixed_case(count=257):
    """257 jobs of both forms whose input ranges overlap, with thresholds of +inf, below zero, and exactly a sample's p"""
    rng = np.random.default_rng(257)
    total = 2 * CHUNK + 4000
    iq = bursty(total, 5)
    p = power(iq)
    rows = []
    for i in range(count):
        n = int(rng.integers(WAVE_MAX + 1, 2 * CHUNK + 3000)) if i % 16 == 5 else int(rng.integers(0, 700))
        n = WAVE_MAX if i == 7 else n
        off = int(rng.integers(0, total - n + 1))
        thr = (np.inf, -1.0, 0.3, float(p[off + n // 2]) if n else 0.0)[i % 4]
        rows.append((off, n, thr))
    return iq, make_jobs(rows)


def equal_case():
    """thresholds exactly equal to a sample's p, to the float32 below it and to the one above"""
    iq = bursty(9000, 6)
    p = power(iq)
    rows = []
    for off, n, at in ((0, 500, 17), (3, 8999 - 3, 8500)):
        q = p[off + at]
        rows += [(off, n, q), (off, n, np.nextafter(q, np.float32(0))), (off, n, np.nextafter(q, np.float32(np.inf)))]
    return iq, make_jobs(rows)


def nonfinite_case():
    """NaN and Inf planted in a WAVE and in a SPLIT job: a NaN p is not above and is no peak; an infinite p is both"""
    iq = bursty(CHUNK + 4500, 7)
    iq[100, 0] = np.nan
    iq[101, 1] = np.inf
    iq[CHUNK + 20] = (-np.inf, 1.0)
    iq[CHUNK + 4000, 1] = np.nan
    rows = [(0, 50, 0.3), (90, 20, 0.3), (100, 1, 0.3), (60, 300, np.inf), (CHUNK - 100, 4500, 0.3), (0, CHUNK + 4500, 0.3)]
    return iq, make_jobs(rows)


def cases():
    """name -> (iq, jobs): every set the CPU and GPU tests share, but the chain"""
    out = {"wave_n": wave_n_case(), "wave_offsets": wave_offset_case(), "split_n": split_n_case(), "planted": planted_case(),
           "mixed257": mixed_case(), "equal": equal_case(), "nonfinite": nonfinite_case()}
    for count in (1, 3, 4, 5):
        out["wave_jobs_%d" % count] = wave_count_case(count)
    return out


# ---- the chain: extract -> measure -> derive ------------------------------------------------------------------------------------

CHAIN_DECIM, CHAIN_TAPS = 8, 65
CHAIN_THRESHOLD = 1e-3					# on p: 24 dB below the tone, inside the noise burst's spread, far above the quiet
CHAIN_CENTRE, CHAIN_DELTA = 0.2, 0.003			# cycles per input sample: the mixer's frequency, the tone's distance from it


def chain_case():
    """A small sc16 stream: quiet noise, a tone burst over samples 4000 .. 20000 and a noise burst over 24000 .. 36000.
    -> (raw int16 [n][2], extract jobs, planted): job 0 lies inside the tone burst, job 1 inside the noise burst, job 2 spans the
    whole tone burst with quiet on both sides.  planted is the tone's frequency in cycles per OUTPUT sample,
    (f_tone - phase_inc / 2^32) * D: a symmetric real low-pass moves no frequency."""
    rng = np.random.default_rng(99)
    n = 40000
    x = 1e-3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    t = np.arange(4000, 20000)
    x[t] += 0.5 * np.exp(2j * np.pi * (CHAIN_CENTRE + CHAIN_DELTA) * t)
    x[24000:36000] += 0.1 * (rng.standard_normal(12000) + 1j * rng.standard_normal(12000))
    raw = np.round(np.stack([x.real, x.imag], 1) * 32768.0).astype(np.int16)
    inc = int(round(CHAIN_CENTRE * 2.0 ** 32))
    jobs = np.zeros(3, EXTRACT_DTYPE)
    at = 1							# an odd offset into d_out
    for j, (first, last) in zip(jobs, ((4100, 19900), (24100, 35900), (2000, 22000))):
        j["first"], j["decim"], j["phase_inc"], j["phase0"], j["taps_offset"], j["n_taps"] = first, CHAIN_DECIM, inc, 0, 0, CHAIN_TAPS
        j["n_out"] = (last - first - CHAIN_TAPS) // CHAIN_DECIM + 1
        j["out_offset"] = at
        at += int(j["n_out"]) + 3
    planted = (CHAIN_CENTRE + CHAIN_DELTA - inc / 2.0 ** 32) * CHAIN_DECIM
    return raw, jobs, planted
