"""numpy statement of rules 1-7 of include/fosphor_amd_carrier.h and the input sets the CPU and GPU tests share.

A case is (iq, jobs): iq float32 [n][2] as it lies in memory, one complex sample per symbol, and jobs a JOB_DTYPE array whose
outputs are placed with GUARD complex samples before, between and behind them (place()).  The angle is demod_model.atan2_turns,
the numpy statement of the pinned fosphor_amd_atan2_turns; the rotation is cossin_turns below, the numpy statement of the pinned
fosphor_amd_cossin_turns.  Every operation is one IEEE double operation that numpy rounds once, in the order of the header's
parentheses.  The ordered sums are symbols_model.three_level: cumsum from an explicit 0.0, never np.sum; a block or a tile that the
terms end in is filled up with +0.0, which leaves a running sum that began at +0.0 as it is.  A NaN float is 0x7fc00000, a NaN double
of the record 0x7ff8000000000000."""
import math

import numpy as np

import demod_model as dm
from symbols_model import QNAN, QNAN64, noise, quiet, quiet64, three_level		# noqa: F401

JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("order", "<i4"), ("mode", "<i4"), ("lag", "<i4"),
                      ("freq", "<f8"), ("phase", "<f8")])
RECORD_DTYPE = np.dtype([("n", "<i4"), ("order", "<i4"), ("lag_used", "<i4"), ("status", "<i4"), ("freq", "<f8"), ("phase", "<f8"),
                         ("r1_re", "<f8"), ("r1_im", "<f8"), ("rl_re", "<f8"), ("rl_im", "<f8"), ("z_re", "<f8"), ("z_im", "<f8"),
                         ("m2", "<f8"), ("mm", "<f8")])
STATS = ("calls", "k_lag", "k_freq", "k_sum", "k_phase", "k_turn", "jobs_freq", "jobs_phase", "symbols")
MAX_JOBS, MAX_LAG, BLOCK, TILE = 4096, 64, 64, 4096
ESTIMATE, FREQ_FIXED, PHASE_FIXED = 0, 1, 2
MODES = {"estimate": 0, "freq_fixed": 1, "phase_fixed": 2, "fixed": 3}
OK, NO_CARRIER = 0, 1
STATUS = {"ok": OK, "no_carrier": NO_CARRIER}
ORDERS = (2, 4, 8)
RECORD_WORDS = RECORD_DTYPE.itemsize // 4
GUARD = 3						# sentinel complex samples before, between and behind the jobs' outputs

TWO_PI = 6.283185307179586
SIN_COEFF = [(1.0 if k % 2 == 0 else -1.0) / float(math.factorial(2 * k + 1)) for k in range(9)]	# s_k / (2k + 1)!, one rounded division
COS_COEFF = [(1.0 if k % 2 == 0 else -1.0) / float(math.factorial(2 * k)) for k in range(9)]	# s_k / (2k)!


def cossin_turns(t):
    """rule 4, operation for operation, in float64 -> (cos, sin) of t turns"""
    t = np.asarray(t, np.float64)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(t)
        t = np.where(bad, 0.0, t)
        r = t - np.floor(t)
        r = np.where(r < 1.0, r, 0.0)
        q = np.floor((r * 4.0) + 0.5)
        d = r - (q * 0.25)
        x = d * TWO_PI
        z = x * x
        S = np.full(z.shape, SIN_COEFF[8])
        C = np.full(z.shape, COS_COEFF[8])
        for k in range(7, -1, -1):
            S = S * z
            S = S + SIN_COEFF[k]
            C = C * z
            C = C + COS_COEFF[k]
        S = x * S
        quad = q.astype(np.int64) & 3
        c = np.choose(quad, [C, -S, -C, S])
        s = np.choose(quad, [S, C, -S, -C])
    return np.where(bad, QNAN64, c), np.where(bad, QNAN64, s)


def square(re, im):
    """the SQUARE rule of fosphor_amd_psd.h"""
    return (re * re) - (im * im), (re * im) + (re * im)


def power(y, order):
    """rule 1 over float32 y [n][2] -> (pr, pi, w, |s|^M) as float64 [n]"""
    re, im = y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        w = (re * re) + (im * im)
        wm = w
        pr, pi = re, im
        m = 2
        while m <= order:
            pr, pi = square(pr, pi)
            if m >= 4:
                wm = wm * wm
            m *= 2
    return pr, pi, w, wm


def lag_used(n, lag):
    return lag if n >= 2 * lag else 1


def lag_sum(pr, pi, d):
    """rule 2 for one lag -> (Rr, Ri)"""
    n = len(pr)
    if n <= d:
        return np.float64(0.0), np.float64(0.0)
    ar, ai, br, bi = pr[d:], pi[d:], pr[:n - d], pi[:n - d]
    with np.errstate(all="ignore"):
        R = three_level(np.stack([(ar * br) + (ai * bi), (ai * br) - (ar * bi)], 1))
    return R[0], R[1]


def frequency(R, Le):
    """rule 3 from the lag sums (R1r, R1i, RLr, RLi) -> g, or None: no carrier"""
    a1 = dm.atan2_turns(R[1], R[0])
    if np.isnan(a1):
        return None
    if Le <= 1:
        return np.float64(a1)
    aL = dm.atan2_turns(R[3], R[2])
    if np.isnan(aL):
        return None
    with np.errstate(all="ignore"):
        k = np.floor(((np.float64(Le) * np.float64(a1)) - np.float64(aL)) + 0.5)
        return (np.float64(aL) + k) / np.float64(Le)


def phase_sums(pr, pi, w, wm, g, j0=0):
    """rule 5 -> (Zr, Zi, m2, mm); j0: the job's index of the first symbol, a multiple of TILE (the sums of the tiles from there on)"""
    j = np.arange(j0, j0 + len(pr), dtype=np.float64)
    with np.errstate(all="ignore"):
        c, sn = cossin_turns(np.float64(g) * j)
        return three_level(np.stack([(pr * c) + (pi * sn), (pi * c) - (pr * sn), w, wm], 1))


def derotate(y, theta, f, j0=0):
    """rule 6 over float32 y [n][2], the symbols j0, j0 + 1, .. of a job -> float32 [n][2]"""
    sr, si = y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)
    j = np.arange(j0, j0 + len(y), dtype=np.float64)
    with np.errstate(all="ignore"):
        c, sn = cossin_turns(np.float64(theta) + (np.float64(f) * j))
        return quiet(np.stack([((sr * c) + (si * sn)).astype(np.float32), ((si * c) - (sr * sn)).astype(np.float32)], 1))


def carrier_job(iq, job):
    """-> (a RECORD_DTYPE array [1], the job's derotated symbols float32 [n][2], or [0][2] without a carrier)"""
    n, M, mode, L = int(job["n"]), int(job["order"]), int(job["mode"]), int(job["lag"])
    y = iq[int(job["offset"]):int(job["offset"]) + n]
    none = np.zeros((0, 2), np.float32)
    pr, pi, w, wm = power(y, M)
    r = np.zeros(1, RECORD_DTYPE)
    r["n"], r["order"] = n, M
    if mode & FREQ_FIXED:
        g = np.float64(job["freq"]) * np.float64(M)
    else:
        Le = lag_used(n, L)
        R = lag_sum(pr, pi, 1) + (lag_sum(pr, pi, Le) if Le > 1 else (np.float64(0.0), np.float64(0.0)))
        r["lag_used"] = Le
        r["r1_re"], r["r1_im"], r["rl_re"], r["rl_im"] = (quiet64(v) for v in R)
        g = frequency(R, Le)
        if g is None:
            r["status"], r["freq"], r["phase"] = NO_CARRIER, QNAN64, QNAN64
            return r, none
    f = g / np.float64(M)
    Z = phase_sums(pr, pi, w, wm, g)
    r["z_re"], r["z_im"], r["m2"], r["mm"] = (quiet64(v) for v in Z)
    if mode & PHASE_FIXED:
        theta = np.float64(job["phase"])
    else:
        thM = dm.atan2_turns(Z[1], Z[0])
        if np.isnan(thM):
            r["status"], r["freq"], r["phase"] = NO_CARRIER, QNAN64, QNAN64
            return r, none
        theta = np.float64(thM) / np.float64(M)
    r["freq"], r["phase"] = f, theta
    return r, derotate(y, theta, f)


def buffer(case):
    return np.ascontiguousarray(case[0], np.float32).reshape(-1, 2)


def carrier(case):
    """(records RECORD_DTYPE [n_jobs], [derotated symbols per job, float32 [n][2] or [0][2]])"""
    iq = buffer(case)
    both = [carrier_job(iq, j) for j in case[1]]
    return np.concatenate([b[0] for b in both]), [b[1] for b in both]


def capacity(jobs):
    """complex samples of the output buffer of a case: the last output and GUARD behind it"""
    return max([int(j["out_offset"]) + int(j["n"]) for j in jobs] + [0]) + GUARD


_IMAGES = {}


def image(case, fill, key=None):
    """(records, the whole output buffer as the model leaves it: uint32 [capacity][2], `fill` wherever no job writes -- the outputs
    of a job without a carrier included); with a key the result is computed once for all the tests of a session"""
    if key is not None and (key, fill) in _IMAGES:
        return _IMAGES[(key, fill)]
    jobs = case[1]
    records, outs = carrier(case)
    out = np.full((capacity(jobs), 2), fill, np.uint32)
    for j, v in zip(jobs, outs):
        out[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v.view(np.uint32)
    if key is not None:
        _IMAGES[(key, fill)] = (records, out)
    return records, out


def expected_stats(jobs):
    """the stats delta of one call over jobs"""
    est_f, est_p = (jobs["mode"] & FREQ_FIXED) == 0, (jobs["mode"] & PHASE_FIXED) == 0
    some = bool((jobs["n"] > 0).any())
    return dict(calls=1, k_lag=int((est_f & (jobs["n"] >= 2)).any()), k_freq=int(est_f.any()), k_sum=int(some), k_phase=1,
                k_turn=int(some), jobs_freq=int(est_f.sum()), jobs_phase=int(est_p.sum()), symbols=int(jobs["n"].sum()))


# ---- the builders ---------------------------------------------------------------------------------------------------------------

def make_jobs(rows):
    """rows of (offset, out_offset, n, order, mode, lag, freq, phase)"""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    for j, r in zip(jobs, rows):
        j["offset"], j["out_offset"], j["n"], j["order"], j["mode"], j["lag"], j["freq"], j["phase"] = r
    return jobs


def place(rows):
    """rows of (offset, n, order, mode, lag, freq, phase) -> jobs whose outputs follow each other with GUARD or GUARD + 1 samples
    between them, so that odd and even out_offsets both occur"""
    out, at = [], GUARD
    for i, row in enumerate(rows):
        out.append((row[0], at) + tuple(row[1:]))
        at += row[1] + GUARD + (i & 1)
    return make_jobs(out)


def psk(n, order, f0, theta0, seed, snr_db=None, amp=1.0):
    """float32 [n][2]: n random symbols of a PSK of `order` points, turning by f0 turns per symbol from theta0 turns on, in complex
    noise of the given SNR"""
    rng = np.random.default_rng(seed)
    ph = rng.integers(0, order, n) / order + theta0 + f0 * np.arange(n)
    z = amp * np.exp(2j * np.pi * ph)
    if snr_db is not None:
        sigma = amp * 10.0 ** (-snr_db / 20.0) / np.sqrt(2.0)
        z = z + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return np.stack([z.real, z.imag], 1).astype(np.float32)


def three_bursts(n, seed, snr_db=30.0):
    """a BPSK, a QPSK and an 8PSK burst of n symbols one behind the other -> (iq, {order: offset of its burst})"""
    parts = [psk(n, M, 0.3 / M * (1 - 0.5 * i), 0.2 / M, seed + i, snr_db) for i, M in enumerate(ORDERS)]
    return np.concatenate(parts), {M: i * n for i, M in enumerate(ORDERS)}


def loads_case():
    """offsets 0 .. 3 against odd and even out_offsets at every order; a few symbols and a few hundred; the last job ends on the
    buffer's last sample"""
    iq, at = three_bursts(700, 10)
    rows, i = [], 0
    for M in ORDERS:
        for n in (37, 300, 301, 600):
            for off in range(4):
                rows.append((at[M] + off, n + (i % 3), M, ESTIMATE, 16, 0.0, 0.0))
                i += 1
    rows.append((len(iq) - 500, 500, 8, ESTIMATE, 8, 0.0, 0.0))
    rows.append((len(iq) - 499, 499, 8, ESTIMATE, 1, 0.0, 0.0))
    return iq, place(rows)


TILE_COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 5)


def tiles_case():
    """n of TILE_COUNTS at every order, L = 16, the offsets of both parities"""
    iq, at = three_bursts(2 * 4096 + 9, 20)
    rows = [(at[M] + (i + k) % 4, n, M, ESTIMATE, 16, 0.0, 0.0) for k, M in enumerate(ORDERS) for i, n in enumerate(TILE_COUNTS)]
    return iq, place(rows)


LAGS = (1, 2, 16, 63, 64)


def lag_case():
    """every L of LAGS with n = 2 L - 1 and n = 2 L, where lag_used switches, and with n - L on 64 and 65 (a block seam), 256 and
    257 (a pass of k_car_lag), 4096 and 4097 (a tile seam): the last terms of a block, a pass and a tile read the next one's
    symbols"""
    iq, at = three_bursts(4096 + 64 + 9, 30)
    rows, i = [], 0
    for L in LAGS:
        for n in (2 * L - 1, 2 * L, 64 + L, 65 + L, 256 + L, 257 + L, 4096 + L, 4097 + L):
            M = ORDERS[i % 3]
            rows.append((at[M] + i % 4, n, M, ESTIMATE, L, 0.0, 0.0))
            i += 1
    return iq, place(rows)


def modes_case():
    """all four combinations of the mode bits at every order; fixed frequencies of +-0.5, 0 and the burst's own; fixed phases of
    +-0.5 and others"""
    iq, at = three_bursts(700, 40)
    rows, i = [], 0
    for M in ORDERS:
        for mode in (ESTIMATE, FREQ_FIXED, PHASE_FIXED, FREQ_FIXED | PHASE_FIXED):
            for freq, phase in ((0.5, 0.5), (-0.5, -0.5), (0.0, 0.0), (0.3 / M, 0.125), (-0.0123, -0.25)):
                rows.append((at[M] + i % 4, 300 + 67 * (i % 5), M, mode, 16, freq if mode & FREQ_FIXED else 0.0,
                             phase if mode & PHASE_FIXED else 0.0))
                i += 1
    return iq, place(rows)


def numbers_case():
    """all-zero symbols (R = 0 and Z = 0: f = 0, theta = 0); a NaN symbol (NO_CARRIER, nothing written) beside jobs that do not see
    it; an inf symbol; subnormal symbols; symbols of 3e38, whose eighth power overflows a double; bursts whose g is near +-0.5 with
    L = 64, where k of rule 3 is at its extremes; under every mode"""
    zeros = np.zeros((300, 2), np.float32)
    sick = psk(1000, 4, 0.01, 0.05, 50, 30.0)
    sick[400, 1] = np.nan
    sick[800, 0] = np.inf
    tiny = (psk(300, 4, 0.02, 0.1, 51, 30.0).astype(np.float64) * 1e-41).astype(np.float32)
    huge = psk(300, 4, 0.02, 0.1, 52, 30.0) * np.float32(3e38)
    edge = [psk(300, M, s * 0.4999 / M, 0.03, 53 + i, 40.0) for i, (M, s) in enumerate((M, s) for M in ORDERS for s in (1, -1))]
    parts = [zeros, sick, tiny, huge] + edge
    starts = np.cumsum([0] + [len(p) for p in parts])
    rows = []
    for mode in (ESTIMATE, FREQ_FIXED, PHASE_FIXED, FREQ_FIXED | PHASE_FIXED):
        fr, ph = (0.01 if mode & FREQ_FIXED else 0.0), (0.05 if mode & PHASE_FIXED else 0.0)
        rows += [(starts[0] + 1, 299, 4, mode, 16, fr, ph),
                 (starts[1], 400, 4, mode, 16, fr, ph), (starts[1] + 300, 200, 4, mode, 16, fr, ph),
                 (starts[1] + 401, 399, 2, mode, 16, fr, ph), (starts[1] + 700, 300, 8, mode, 4, fr, ph),
                 (starts[1] + 399, 2, 4, mode, 1, fr, ph), (starts[1] + 400, 1, 4, mode, 1, fr, ph)]
        for M in ORDERS:
            rows += [(starts[2] + 1, 299, M, mode, 16, fr, ph), (starts[3], 300, M, mode, 16, fr, ph)]
    for i, (M, s) in enumerate((M, s) for M in ORDERS for s in (1, -1)):
        rows += [(starts[4 + i], 300, M, ESTIMATE, 64, 0.0, 0.0), (starts[4 + i] + 1, 299, M, PHASE_FIXED, 63, 0.0, 0.25)]
    return np.concatenate(parts), place([tuple(int(v) if k < 5 else v for k, v in enumerate(r)) for r in rows])


def mixed_case(count=41, seed=77):
    """one call with every mode, order and a spread of lags, jobs without a symbol in between; the input ranges overlap"""
    rng = np.random.default_rng(seed)
    iq, at = three_bursts(3000, seed + 1, 25.0)
    rows = []
    for i in range(count):
        M = ORDERS[i % 3]
        mode = (ESTIMATE, ESTIMATE, FREQ_FIXED, PHASE_FIXED, FREQ_FIXED | PHASE_FIXED)[i % 5]
        n = int(rng.integers(0, 3)) if i % 7 == 3 else int(rng.integers(3, 2900))
        rows.append((at[M] + int(rng.integers(0, 3000 - n + 1)), n, M, mode, int(rng.integers(1, MAX_LAG + 1)),
                     float(rng.uniform(-0.5, 0.5)) if mode & FREQ_FIXED else 0.0, float(rng.uniform(-0.5, 0.5)) if mode & PHASE_FIXED else 0.0))
    return iq, place(rows)


def full_table_case(modes=(ESTIMATE, FREQ_FIXED, PHASE_FIXED, FREQ_FIXED | PHASE_FIXED)):
    """MAX_JOBS jobs in shuffled order, the orders, lags and modes mixed, n <= 130, every 11th with n = 0: the deepest search of
    both prefixes"""
    rng = np.random.default_rng(4096 + len(modes) + modes[0])
    iq, at = three_bursts(1500, 90, 25.0)
    rows = []
    for i in rng.permutation(MAX_JOBS):
        i = int(i)
        M, mode = ORDERS[i % 3], modes[i % len(modes)]
        n = 0 if i % 11 == 0 else 1 + (i // 4) % 130
        rows.append((at[M] + int(rng.integers(0, 1500 - n + 1)), n, M, mode, 1 + (i * 7) % MAX_LAG,
                     ((i * 13) % 65 - 32) / 64.0 if mode & FREQ_FIXED else 0.0, ((i * 29) % 65 - 32) / 64.0 if mode & PHASE_FIXED else 0.0))
    return iq, place(rows)


def cases():
    """name -> (iq, jobs): every set the CPU and GPU tests share"""
    return {"loads": loads_case(), "tiles": tiles_case(), "lag": lag_case(), "modes": modes_case(), "numbers": numbers_case(),
            "mixed": mixed_case(), "full_table": full_table_case(), "only_fixed": full_table_case((FREQ_FIXED | PHASE_FIXED,))}
