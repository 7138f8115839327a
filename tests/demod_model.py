"""numpy statement of rules 1-3 of include/fosphor_amd_demod.h and the input sets the CPU and GPU tests share.

A case is (iq, jobs): iq float32 [n][2] as it lies in memory, jobs a JOB_DTYPE array whose outputs are placed with GUARD floats
before, between and behind them (place()).  Everything here is IEEE arithmetic that numpy performs one rounded operation at a
time: float32 for the power, float64 for the angle and the integrate-and-dump sum, one conversion to float32 at the end.  The
device and fosphor_amd_demod_host must reproduce it to the bit; a NaN is the one quiet NaN 0x7fc00000 (rule 3)."""
import numpy as np

JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("mode", "<i4"), ("avg", "<i4"), ("reserved", "<i4")])
STATS = ("calls", "k_direct", "k_avg", "jobs_direct", "jobs_avg", "samples", "outputs")
MAX_JOBS, MAX_AVG, TILE = 4096, 256, 2048
POWER, PHASE, FM = 0, 1, 2
MODES = {"power": POWER, "phase": PHASE, "fm": FM}
GUARD = 3						# sentinel floats before, between and behind the jobs' outputs
QNAN = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]

TAN_PI_8 = 0.41421356237309503
INV_2PI = 0.15915494309189535
COEFF = [(1.0 if k % 2 == 0 else -1.0) / (2 * k + 1) for k in range(12)]		# s_k / (2k + 1), each one rounded division


def atan2_turns(y, x):
    """rule 2, operation for operation, in float64; the result in float32"""
    y, x = np.broadcast_arrays(np.asarray(y, np.float64), np.asarray(x, np.float64))
    with np.errstate(all="ignore"):
        nan = np.isnan(y) | np.isnan(x)
        ax, ay = np.abs(x), np.abs(y)
        swap = ay > ax
        mn, mx = np.where(swap, ax, ay), np.where(swap, ay, ax)
        t = np.where(mx == 0.0, 0.0, np.where(np.isinf(mn), 1.0, mn / mx))
        big = t > TAN_PI_8
        u = np.where(big, (t - 1.0) / (t + 1.0), t)
        z = u * u
        q = np.full(z.shape, 1.0 / 25.0)
        for k in range(11, -1, -1):
            q = q * z
            q = q + COEFF[k]
        a = (u * q) * INV_2PI
        a = np.where(big, 0.125 + a, a)
        a = np.where(swap, 0.25 - a, a)
        a = np.where(np.signbit(x), 0.5 - a, a)
        a = np.where(np.signbit(y), -a, a)
        out = a.astype(np.float32)
    out[nan] = QNAN
    return out


def quiet(v):
    v = np.array(v, np.float32)
    v[np.isnan(v)] = QNAN
    return v


def n_trace(mode, n):
    return max(n - 1, 0) if mode == FM else n


def n_out(mode, n, avg):
    return n_trace(mode, n) // avg


def trace(y, mode):
    """rule 1: the whole trace of the samples y, float32 [n_trace]"""
    y = np.asarray(y, np.float32).reshape(-1, 2)
    re, im = y[:, 0], y[:, 1]
    with np.errstate(all="ignore"):
        if mode == POWER:
            return quiet((re * re) + (im * im))
        if mode == PHASE:
            return atan2_turns(im.astype(np.float64), re.astype(np.float64))
        re0, im0, re1, im1 = (a.astype(np.float64) for a in (re[:-1], im[:-1], re[1:], im[1:]))
        if len(y) < 2:
            return np.zeros(0, np.float32)
        return atan2_turns(im1 * re0 - re1 * im0, re1 * re0 + im1 * im0)


def dump(v, L):
    """rule 3: integrate and dump"""
    if L == 1:
        return v
    k = len(v) // L
    rows = v[:k * L].reshape(k, L).astype(np.float64)
    S = np.zeros(k, np.float64)
    with np.errstate(all="ignore"):
        for i in range(L):
            S = S + rows[:, i]
        return quiet((S / np.float64(L)).astype(np.float32))


def job_samples(iq, job):
    return np.asarray(iq, np.float32).reshape(-1, 2)[int(job["offset"]):int(job["offset"]) + int(job["n"])]


def demod_job(iq, job):
    return dump(trace(job_samples(iq, job), int(job["mode"])), int(job["avg"]))


def demod(iq, jobs):
    """one float32 array per job"""
    return [demod_job(iq, j) for j in np.atleast_1d(jobs)]


def capacity(jobs):
    """floats of the output buffer of a case: the last output and GUARD behind it"""
    return max([int(j["out_offset"]) + n_out(int(j["mode"]), int(j["n"]), int(j["avg"])) for j in jobs] + [0]) + GUARD


def image(iq, jobs, fill):
    """the whole output buffer of a case as the model leaves it: uint32 [capacity], `fill` wherever no job writes"""
    out = np.full(capacity(jobs), fill, np.uint32)
    for j, v in zip(jobs, demod(iq, jobs)):
        out[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v.view(np.uint32)
    return out


# ---- the builders ---------------------------------------------------------------------------------------------------------------

def make_jobs(rows):
    """rows of (offset, out_offset, n, mode, avg)"""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    for j, r in zip(jobs, rows):
        j["offset"], j["out_offset"], j["n"], j["mode"], j["avg"] = r
    return jobs


def place(rows):
    """rows of (offset, n, mode, avg) -> jobs whose outputs follow each other with GUARD or GUARD + 1 floats between them, so that
    odd and even out_offsets both occur whatever the lengths are"""
    out, at = [], GUARD
    for i, (off, n, mode, avg) in enumerate(rows):
        out.append((off, at, n, mode, avg))
        at += n_out(mode, n, avg) + GUARD + (i & 1)
    return make_jobs(out)


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * np.exp(rng.uniform(-3.0, 3.0, (n, 1)))).astype(np.float32)


NS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 3 * TILE + 5)
LS = (1, 2, 3, 7, 64, 255, 256)


def lengths_case(mode):
    """every n of NS with every L of LS from input offsets 0, 1, 2, 3 in turn; the longest job of every L once more so that it
    ends on the buffer's last sample.  n = 4097 and 3 * TILE + 5 have trace values in two and four DIRECT tiles, and in AVG tiles
    of 2048 (L = 2, 64, 256), 2046 (L = 3), 2044 (L = 7) and 2040 (L = 255) trace values: in FM the last value of a tile reads
    y[m + 1] from what the next work-group loads as its first sample."""
    total = NS[-1] + 3
    rows, i = [], 0
    for n in NS:
        for L in LS:
            rows.append((i % 4, n, mode, L))
            i += 1
    for k, L in enumerate(LS):
        n = NS[-1] - (k & 1)
        rows.append((total - n, n, mode, L))
    return noise(total, 10 + mode), place(rows)


def fm_edges_case():
    """FM with n = 0, 1 (no trace value), n = L (L - 1 trace values: no output for L > 1) and n = L + 1 (one output)"""
    rows = [(0, 0, FM, 1), (1, 1, FM, 1)]
    for i, L in enumerate(LS):
        rows += [(i % 4, 1, FM, L), (i % 4 + 1, L, FM, L), (i % 4 + 2, L + 1, FM, L), (i % 4 + 3, 2 * L, FM, L)]
    return noise(2 * MAX_AVG + 8, 20), place(rows)


SEAM_T = np.float32(TAN_PI_8)
SEAMS_T = (np.nextafter(SEAM_T, np.float32(0)), SEAM_T, np.nextafter(SEAM_T, np.float32(1)))


def seam_pairs():
    """(y, x) pairs, every value a float32: the header's seam table, every octant, t at the float32 neighbours of tan(pi / 8) on
    both sides in all eight reflections, signed zeros, infinities, NaN, and quotients that leave a subnormal float32"""
    inf, nan = np.inf, np.nan
    out = [(0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (1.0, 1.0), (1.0, -1.0), (0.0, 0.0),
           (inf, inf), (inf, 1.0), (1.0, -inf)]
    signs = [(sy, sx) for sy in (1.0, -1.0) for sx in (1.0, -1.0)]
    for sy, sx in signs:
        out += [(sy * 1.0, sx * 3.0), (sy * 3.0, sx * 1.0), (sy * 0.5, sx * 0.5)]			# the eight octants, the diagonals
        for t in SEAMS_T:
            out += [(sy * float(t), sx * 1.0), (sy * 1.0, sx * float(t))]
        out += [(sy * 0.0, sx * 0.0), (sy * 0.0, sx * 1.0), (sy * 1.0, sx * 0.0)]
        out += [(sy * inf, sx * inf), (sy * inf, sx * 1.0), (sy * 1.0, sx * inf), (sy * inf, sx * 0.0), (sy * 0.0, sx * inf)]
        out += [(sy * 1e-20, sx * 1e20), (sy * 1e20, sx * 1e-20), (sy * 1e-30, sx * 1e-30), (sy * 3e38, sx * 3e38)]
    out += [(nan, 1.0), (1.0, nan), (nan, nan), (nan, inf), (0.0, nan)]
    a = np.array(out, np.float32).astype(np.float64)
    return a[:, 0], a[:, 1]


def seams_case():
    """the seam pairs as PHASE samples (re = x, im = y), and as FM pairs: each between two samples (1, 0), so that z is the seam
    sample, then its conjugate; power over them for good measure.  L = 1 and L = 2"""
    y, x = seam_pairs()
    n = len(y)
    iq = np.zeros((3 * n + 1, 2), np.float32)
    iq[:n, 0], iq[:n, 1] = x, y
    iq[n::2] = (1.0, 0.0)
    iq[n + 1::2, 0], iq[n + 1::2, 1] = x, y
    rows = [(0, n, PHASE, 1), (n, 2 * n + 1, FM, 1), (0, 3 * n + 1, POWER, 1), (0, n, PHASE, 2), (n, 2 * n + 1, FM, 2),
            (1, n - 1, PHASE, 3), (n + 1, 2 * n, FM, 3)]
    return iq, place(rows)


def nonfinite_case():
    """NaN and inf samples inside jobs of every mode and both forms: the outputs they reach are NaN or inf, the neighbours finite"""
    iq = noise(3000, 30)
    iq[100, 0] = np.nan
    iq[200] = (np.inf, 1.0)
    iq[300] = (-np.inf, np.inf)
    iq[2500, 1] = np.nan
    iq[2600] = (0.0, 0.0)
    rows = [(0, 3000, mode, L) for mode in (POWER, PHASE, FM) for L in (1, 4)] + [(97, 8, FM, 1), (100, 1, PHASE, 1)]
    return iq, place(rows)


def mixed_case(count=257):
    """257 jobs of mixed modes and L whose input ranges overlap"""
    rng = np.random.default_rng(257)
    total = 2 * TILE + 900
    rows = []
    for i in range(count):
        n = int(rng.integers(TILE + 1, total)) if i % 16 == 5 else int(rng.integers(0, 700))
        L = (1, 1, 2, 3, 7, 16, 64, 255, 256)[int(rng.integers(0, 9))]
        rows.append((int(rng.integers(0, total - n + 1)), n, i % 3, L))
    return noise(total, 40), place(rows)


def cut_case():
    """rule 3: every (mode, L) of the cut rule as three jobs -- the whole, and the two it is cut into at c * L trace values, where c
    is chosen inside a tile, on a tile's edge and in the last tile.  -> (iq, jobs, [(whole, first, second, c)] job indices)"""
    n, off = 2 * TILE + 777, 3
    rows, triples = [], []
    for mode in (POWER, PHASE, FM):
        for L in (1, 3, 64):
            for c in (1, 5, TILE // L, TILE // L + 1, n_out(mode, n, L) - 1):
                triples.append((len(rows), len(rows) + 1, len(rows) + 2, c))
                fm = int(mode == FM)
                rows += [(off, n, mode, L), (off, c * L + fm, mode, L), (off + c * L, n - c * L, mode, L)]
    return noise(n + off, 50), place(rows), triples


def tone(n, f, phase=0.1):
    """float32 roundings of the unit phasor exp(2 pi i (f m + phase))"""
    z = np.exp(2j * np.pi * (f * np.arange(n) + phase))
    return np.stack([z.real, z.imag], 1).astype(np.float32)


def cases():
    """name -> (iq, jobs): every set the CPU and GPU tests share, but the cut rule and the chain"""
    return {"n_power": lengths_case(POWER), "n_phase": lengths_case(PHASE), "n_fm": lengths_case(FM), "fm_edges": fm_edges_case(),
            "seams": seams_case(), "nonfinite": nonfinite_case(), "mixed257": mixed_case()}
