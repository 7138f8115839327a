"""numpy statement of include/fosphor_amd_extract.h: the contract in float64, the design formula, a float32 emulation of a plain
implementation (used on the CPU only, to confirm the tolerance of the GPU tests), and the input sets those tests share.

A case is (fmt, raw, jobs, taps): raw the samples as they lie in memory (float32 [n][2], int16 [n][2] or float16 [n][2]), jobs a
JOB_DTYPE array, taps float32.  Output offsets leave GUARD untouched entries before, between and behind the jobs' ranges."""
import numpy as np

FP32, FP16, SC16 = 0, 1, 2
RAW_DTYPE = {FP32: np.float32, FP16: np.float16, SC16: np.int16}
JOB_DTYPE = np.dtype([("first", "<i8"), ("out_offset", "<i8"), ("n_out", "<i4"), ("decim", "<i4"), ("phase_inc", "<u4"),
                      ("phase0", "<u4"), ("taps_offset", "<i4"), ("n_taps", "<i4")])
STATS = ("calls", "k_tile", "k_wave", "jobs_tile", "jobs_wave", "samples")
MAX_JOBS, MAX_DECIM, MAX_TAPS = 4096, 1024, 8192
TILE_OUT, TILE_LDS, WAVE_OUT = 256, 6656, 4
GUARD = 3
M32 = np.uint64(0xffffffff)


def form(decim, n_taps):
    row = (TILE_OUT + (n_taps - 1) // decim + 1) | 1
    return "tile" if decim * row <= TILE_LDS else "wave"


def widen(raw, fmt):
    """the samples as complex128, exactly"""
    raw = np.asarray(raw, RAW_DTYPE[fmt])
    v = raw.astype(np.float64)
    if fmt == SC16:
        v = v * 2.0 ** -15
    return v[:, 0] + 1j * v[:, 1]


def phases(job, n):
    """phi(n), uint64 values below 2^32"""
    return (np.uint64(job["phase0"]) + (np.asarray(n, np.uint64) & M32) * np.uint64(job["phase_inc"])) & M32


def job_indices(job):
    """n = m * D + k, [n_out][T]"""
    return np.arange(int(job["n_out"]), dtype=np.int64)[:, None] * int(job["decim"]) + np.arange(int(job["n_taps"]), dtype=np.int64)


def extract_job(x, job, taps):
    """y[m] of one job in float64"""
    if job["n_out"] == 0:
        return np.zeros(0, np.complex128)
    n = job_indices(job)
    h = np.asarray(taps, np.float32)[int(job["taps_offset"]):int(job["taps_offset"]) + int(job["n_taps"])].astype(np.float64)
    lo = np.exp(-2j * np.pi * (phases(job, n).astype(np.float64) / 2.0 ** 32))
    return (x[int(job["first"]) + n] * lo) @ h


def extract(raw, fmt, jobs, taps):
    x = widen(raw, fmt)
    return [extract_job(x, j, taps) for j in jobs]


def extract_naive(x, job, taps):
    """the contract as three loops, sharing nothing with extract_job but the phase's integer arithmetic written out again"""
    out = []
    for m in range(int(job["n_out"])):
        acc = 0j
        for k in range(int(job["n_taps"])):
            n = m * int(job["decim"]) + k
            phi = (int(job["phase0"]) + n * int(job["phase_inc"])) % (1 << 32)
            ang = -2.0 * np.pi * phi / 2.0 ** 32
            acc += float(taps[int(job["taps_offset"]) + k]) * x[int(job["first"]) + n] * complex(np.cos(ang), np.sin(ang))
        out.append(acc)
    return np.array(out, np.complex128)


def bound(x, job, taps):
    """(T + 16) * 2^-24 * sum|h| * max|x| over the job's input span, per component"""
    if job["n_out"] == 0:
        return 0.0
    t, d = int(job["n_taps"]), int(job["decim"])
    h = np.asarray(taps, np.float32)[int(job["taps_offset"]):int(job["taps_offset"]) + t].astype(np.float64)
    span = x[int(job["first"]):int(job["first"]) + (int(job["n_out"]) - 1) * d + t]
    return (t + 16) * 2.0 ** -24 * np.abs(h).sum() * np.abs(span).max()


def extract_job_f32(x, job, taps):
    """a plain float32 implementation: the mixer's sine and cosine rounded to float32, the complex product in float32 with one
    fused multiply-add per component, and a sequential fmaf sum over k.  (A fused multiply-add is formed in float64 and rounded
    once more: the product of two float32 is exact there.)"""
    if job["n_out"] == 0:
        return np.zeros(0, np.complex128)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    n = job_indices(job)
    h = np.asarray(taps, np.float32)[int(job["taps_offset"]):int(job["taps_offset"]) + int(job["n_taps"])].astype(np.float64)
    ang = 2.0 * np.pi * (phases(job, n).astype(np.float64) / 2.0 ** 32)
    c, s = f32(np.cos(ang)), f32(np.sin(ang))
    xs = x[int(job["first"]) + n]
    vr = f32(xs.real * c + f32(xs.imag * s))
    vi = f32(xs.imag * c - f32(xs.real * s))
    re = np.zeros(n.shape[0])
    im = np.zeros(n.shape[0])
    for k in range(n.shape[1]):
        re = f32(h[k] * vr[:, k] + re)
        im = f32(h[k] * vi[:, k] + im)
    return re + 1j * im


def design(decim, n_taps, guard):
    """the formula of fosphor_amd_extract_design, float64 (not rounded to float32)"""
    fc = guard / (2.0 * decim)
    k = np.arange(n_taps, dtype=np.float64)
    t = k - 0.5 * (n_taps - 1)
    safe = np.where(t == 0.0, 1.0, t)
    s = np.where(t == 0.0, 2.0 * fc, np.sin(2.0 * np.pi * fc * safe) / (np.pi * safe))
    w = np.ones(1) if n_taps == 1 else 0.54 - 0.46 * np.cos(2.0 * np.pi * k / (n_taps - 1))
    g = s * w
    half = (n_taps + 1) // 2
    g[n_taps - half:] = g[:half][::-1]
    return g / g.sum()


# ---- the input sets -------------------------------------------------------------------------------------------------------------

def make_jobs(rows):
    """rows of (first, n_out, decim, phase_inc, phase0, taps_offset, n_taps); out_offset is given in that order, GUARD apart"""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    at = GUARD
    for j, r in zip(jobs, rows):
        j["first"], j["n_out"], j["decim"], j["phase_inc"], j["phase0"], j["taps_offset"], j["n_taps"] = r
        j["out_offset"] = at
        at += int(j["n_out"]) + GUARD
    return jobs


def capacity(jobs):
    return int((jobs["out_offset"] + jobs["n_out"]).max()) + GUARD


def need(n_out, d, t):
    return (n_out - 1) * d + t if n_out else 0


def stream(fmt, n, seed):
    """n samples; sc16 with full-scale and -32768 entries, fp16 with subnormals"""
    rng = np.random.default_rng(seed)
    if fmt == FP32:
        return rng.standard_normal((n, 2)).astype(np.float32)
    if fmt == SC16:
        raw = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
        raw[::97] = (-32768, 32767)
        return raw
    raw = rng.standard_normal((n, 2)).astype(np.float16)
    raw[::89] = (np.float16(6e-8), np.float16(-3e-6))		# subnormals of float16
    return raw


def lowpass(rng, t):
    """taps of both signs, sum|h| near 1"""
    h = rng.standard_normal(t)
    return (h / np.abs(h).sum()).astype(np.float32)


def representable(n, seed):
    """int16 values that float16 holds exactly as i * 2^-15: an 11-bit integer times a power of two (the small ones are float16
    subnormals), -32768 included"""
    rng = np.random.default_rng(seed)
    m = rng.integers(-1024, 1024, (n, 2))
    s = rng.integers(0, 6, (n, 2))
    raw = (m << s).astype(np.int16)
    raw[0] = (-32768, 1)
    return raw


def same_values(raw_sc16, fmt):
    v = raw_sc16.astype(np.float64) * 2.0 ** -15
    out = v.astype(RAW_DTYPE[fmt]) if fmt != SC16 else raw_sc16
    assert np.array_equal(out.astype(np.float64) * (2.0 ** -15 if fmt == SC16 else 1.0), v)
    return out


def one_tap_set(rng, shapes):
    """taps of the (decim, n_taps) shapes side by side -> (taps, {shape: offset})"""
    at, parts, where = 0, [], {}
    for d, t in shapes:
        if (d, t) not in where:
            where[(d, t)] = at
            parts.append(lowpass(rng, t))
            at += t
    return np.concatenate(parts), where


def simple_case(fmt, seed, shapes, first=0, exact_end=True):
    """one job per (decim, n_taps, n_out) shape, all from sample `first`; the stream ends with the longest job's last sample"""
    rng = np.random.default_rng(seed)
    taps, where = one_tap_set(rng, [(d, t) for d, t, _ in shapes])
    rows = [(first, n_out, d, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), where[(d, t)], t) for d, t, n_out in shapes]
    n = first + max(need(n_out, d, t) for d, t, n_out in shapes) + (0 if exact_end else 7)
    return fmt, stream(fmt, max(n, 1), seed + 1), make_jobs(rows), taps


def mixer_case():
    """D = 1, T = 1: the phase alone, wrapping many times over 4096 samples"""
    taps = np.array([0.75], np.float32)
    rows = [(0, 4096, 1, inc, 0xfffffff0, 0, 1) for inc in (1, 0x7fffffff, 0x80000000, 0xffffffff)]
    return FP32, stream(FP32, 4096, 11), make_jobs(rows), taps


def tile_edge():
    """(largest TILE decimation, smallest WAVE decimation) with T = 8 D + 1"""
    d = max(d for d in range(1, MAX_DECIM + 1) if form(d, 8 * d + 1) == "tile")
    assert form(d + 1, 8 * d + 9) == "wave"
    return d, d + 1


def many_jobs_case():
    """257 jobs, mixed D, T and forms, overlapping inputs, outputs out of order, some with n_out = 0"""
    rng = np.random.default_rng(257)
    shapes = [(1, 5), (2, 17), (3, 25), (4, 3), (7, 57), (16, 129), (32, 257), (40, 64), (64, 513)]
    taps, where = one_tap_set(rng, shapes)
    n = 40000
    rows = []
    for i in range(257):
        d, t = shapes[i % len(shapes)]
        n_out = 0 if i % 11 == 0 else int(rng.integers(1, 24 if form(d, t) == "wave" else 300))
        first = int(rng.integers(0, n - need(n_out, d, t) + 1))
        rows.append((first, n_out, d, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), where[(d, t)], t))
    jobs = make_jobs(rows)
    jobs = jobs[rng.permutation(len(jobs))]
    return SC16, stream(SC16, n, 258), jobs, taps


def split_case(d, t, fmt=SC16):
    """a job of 64 outputs, and the same as two jobs of 32, the second with first and phase0 advanced"""
    rng = np.random.default_rng(64 + d)
    taps = lowpass(rng, t)
    inc, ph = 0x1234567b, 0xdeadbeef
    rows = [(3, 64, d, inc, ph, 0, t), (3, 32, d, inc, ph, 0, t),
            (3 + 32 * d, 32, d, inc, (ph + 32 * d * inc) % (1 << 32), 0, t)]
    return fmt, stream(fmt, 3 + need(64, d, t), 65), make_jobs(rows), taps


def cases():
    """name -> (fmt, raw, jobs, taps): every set the GPU tests run, but the end-to-end chain"""
    big, small = tile_edge()
    out = {
        "mixer": mixer_case(),
        "d1_t33_d4_t3": simple_case(SC16, 1, [(1, 33, 600), (4, 3, 600)]),
        "d16_t129": simple_case(FP32, 2, [(16, 129, 300)]),
        "odd_d": simple_case(FP16, 3, [(3, 25, 520), (5, 41, 300)]),
        "form_edge": simple_case(SC16, 4, [(big, 8 * big + 1, 260), (small, 8 * small + 1, 9)]),
        "d1024_t8192": simple_case(FP32, 5, [(1024, 8192, 3)]),
        "n_out_seams": simple_case(SC16, 6, [(2, 17, n) for n in (0, 1, TILE_OUT - 1, TILE_OUT, TILE_OUT + 1, 2 * TILE_OUT + 1)] +
                                   [(32, 257, n) for n in (0, 1, WAVE_OUT - 1, WAVE_OUT, WAVE_OUT + 1, 2 * WAVE_OUT + 1)]),
        "many": many_jobs_case(),
        "split_tile": split_case(4, 33),
        "split_wave": split_case(48, 385),
    }
    for fmt, name in ((FP32, "fp32"), (FP16, "fp16"), (SC16, "sc16")):
        for first in (0, 1, 2, 3, 5):
            out["first%d_%s" % (first, name)] = simple_case(fmt, 20 + first, [(2, 9, 300), (32, 70, 6)], first=first)
    return out
