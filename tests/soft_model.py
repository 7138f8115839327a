"""numpy statement of rules S1-S3 of include/fosphor_amd_soft.h over rules 2-7 of include/fosphor_amd_decode.h, and the input sets
the CPU and GPU tests share.

A case is (iq, jobs): iq float32 [n][2] as it lies in memory, one complex sample per symbol (what fosphor_amd_carrier writes), and
jobs a JOB_DTYPE array whose owned bytes are placed with GUARD or 2 GUARD bytes before, between and behind them (place()).  The
points are carrier_model.cossin_turns, the numpy statement of the pinned fosphor_amd_cossin_turns; every floating-point operation
is one IEEE double operation that numpy rounds once, in the order of the header's parentheses; everything behind the soft values is
integer work, written from the rules alone: the trellis as arrays over the S states, the jobs of one shape decoded together.  The
encoder, the puncture patterns, the CRCs and rules 2, 6 and 7 are decode_model's."""
import numpy as np

import carrier_model as cm
import decode_model as dm

JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("order", "<i2"), ("flags", "<i2"), ("steps", "<i4"),
                      ("k", "u1"), ("n_poly", "u1"), ("period", "u1"), ("crc_width", "u1"), ("polys", "<u2", (3,)),
                      ("punct", "<u2", (3,)), ("crc_poly", "<u4"), ("crc_init", "<u4"), ("crc_xorout", "<u4"), ("rot", "<i4"),
                      ("scale", "<f4")])
RECORD_DTYPE = np.dtype([("n_steps", "<i4"), ("n_bits", "<i4"), ("n_coded", "<i4"), ("status", "<i4"), ("end_state", "<i4"),
                         ("metric", "<i4"), ("best_state", "<i4"), ("best_metric", "<i4"), ("crc_calc", "<u4"), ("crc_recv", "<u4"),
                         ("k", "<i4"), ("flags", "<i4"), ("erasures", "<i4"), ("saturated", "<i4"), ("abs_sum", "<i8")])
STATS = ("calls", "k_bits", "k_acs", "k_trace", "k_rec", "jobs_crc", "steps")
MAX_JOBS, MAX_STEPS, MAX_CALL_STEPS, BLOCK, GROUP, MAX_VALUE, INF = 4096, 65536, 1 << 22, 64, 256, 127, 1 << 25
TERMINATED, GRAY = 1, 2
FLAGS = {"terminated": TERMINATED, "gray": GRAY}
OK, CRC_FAIL, SHORT = dm.OK, dm.CRC_FAIL, dm.SHORT
STATUS = dm.STATUS
ORDERS = dm.ORDERS
RECORD_WORDS = RECORD_DTYPE.itemsize // 4
GUARD = dm.GUARD

# every constraint length at two and at three streams: (k, polys)
CODES2 = {3: dm.K3, 4: (4, (0o15, 0o17, 0)), 5: dm.K5, 6: (6, (0o53, 0o75, 0)), 7: dm.K7}
CODES3 = {3: (3, (0o5, 0o7, 0o7)), 4: dm.K4_THIRD, 5: (5, (0o25, 0o33, 0o37)), 6: (6, (0o47, 0o53, 0o75)), 7: dm.K7_THIRD}
# rates 1/2, 2/3, 3/4 and 7/8 of a two-stream code, and the same masks with a third stream that is sent once a period
PUNCT2 = (dm.P_NONE, dm.P_23, dm.P_34, dm.P_78)
PUNCT3 = (dm.P3_NONE, (2, (0b11, 0b01, 0b10)), (3, (0b011, 0b101, 0b100)), (7, (0b1010001, 0b0101111, 0b0010000)))

shape, owned, job_owned, capacity, unpack, crc_of = dm.shape, dm.owned, dm.job_owned, dm.capacity, dm.unpack, dm.crc_of


def labels(M, gray):
    q = np.arange(M)
    return q ^ (q >> 1) if gray else q


def points(M, rot):
    """rule S1 -> (C_q, S_q), float64 [M] each"""
    q = np.arange(M)
    return cm.cossin_turns(((q + int(rot)) & (M - 1)).astype(np.float64) / np.float64(M))


def soft_values(y, M, rot, gray, scale, variant=0):
    """rules S1 and S2 over float32 y [n][2] -> (v int64 [n][b], a part is a NaN: bool [n]).  variant: 0, or a contraction of the
    correlation (contracted_values(), finite symbols only)"""
    b = dm.bits_of(M)
    sr, si = y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)
    nan = np.isnan(sr) | np.isnan(si)
    C, S = points(M, rot)
    lab = labels(M, gray)
    v = np.zeros((len(y), b), np.int64)
    with np.errstate(all="ignore"):
        corr = (sr[:, None] * C[None, :]) + (si[:, None] * S[None, :])
        for i in range(b):
            bit = (lab >> (b - 1 - i)) & 1
            # the largest, a NaN never: fmax hands on the other operand; -inf where the set holds nothing larger
            zero = np.fmax.reduce(np.where(bit[None, :] == 0, corr, -np.inf), axis=1, initial=-np.inf)
            one = np.fmax.reduce(np.where(bit[None, :] == 1, corr, -np.inf), axis=1, initial=-np.inf)
            x = ((zero - one) * np.float64(np.float32(scale))) + 0.5
            v[:, i] = np.where(np.isnan(x), 0.0, np.clip(np.floor(x), -MAX_VALUE, MAX_VALUE)).astype(np.int64)
    v[nan] = 0
    if variant:
        for m in np.flatnonzero(~nan):
            v[m] = contracted_values(y[m], M, rot, gray, scale, variant)
    return v, nan


def step_values(iq, job, T, variant=0):
    """rules 2 and S2 -> (v int64 [T][3], 0 where a stream's bit was not sent; sent bool [T][3]; erasures)"""
    M, b, n_poly = int(job["order"]), dm.bits_of(job["order"]), int(job["n_poly"])
    at, n = int(job["offset"]), int(job["n"])
    v, nan = soft_values(iq[at:at + n], M, job["rot"], int(job["flags"]) & GRAY, job["scale"], variant)
    coded = v.reshape(-1)
    sent = dm.sent_of(T, n_poly, int(job["period"]), job["punct"])
    flat = sent.reshape(-1)
    q = np.cumsum(flat) - flat
    out = np.where(flat, coded[np.minimum(q, max(len(coded) - 1, 0))] if len(coded) else 0, 0).reshape(T, 3)
    n_coded = int(flat.sum())
    return out, sent, int(nan[:(n_coded + b - 1) // b].sum())


def expected(k, polys, n_poly):
    """rule 3 -> (p [2][S], e [2][3][S]: what predecessor x sends into state s', stream by stream)"""
    S = 1 << (k - 1)
    s = np.arange(S)
    u = s >> (k - 2)
    p = np.stack([((s << 1) | x) & (S - 1) for x in (0, 1)])
    e = np.zeros((2, 3, S), np.int64)
    for x in (0, 1):
        R = (u << (k - 1)) | p[x]
        for i in range(n_poly):
            e[x, i] = dm.parity(int(polys[i]) & R)
    return p, e


def viterbi(v, k, polys, n_poly, terminated):
    """rules 3-5 with the costs of rule S3 over v int64 [J][T][3] -> (ends int [J][4], the decoded inputs u_t uint8 [J][T])"""
    J, T = v.shape[:2]
    S = 1 << (k - 1)
    if T == 0:
        return np.zeros((J, 4), np.int64), np.zeros((J, 0), np.uint8)
    p, e = expected(k, polys, n_poly)
    for_one, for_zero = np.maximum(v, 0), np.maximum(-v, 0)			# what expecting a 1, a 0 costs: [J][T][3]
    metric = np.full((J, S), INF, np.int64)
    metric[:, 0] = 0
    dec = np.zeros((T, J, S), bool)
    for t in range(T):
        cost = [sum(np.where(e[x, i][None, :] == 1, for_one[:, t, i][:, None], for_zero[:, t, i][:, None]) for i in range(3)) for x in (0, 1)]
        c0 = metric[:, p[0]] + cost[0]
        c1 = metric[:, p[1]] + cost[1]
        one = c1 < c0							# ties go to x = 0
        metric = np.where(one, c1, c0)
        dec[t] = one
    key = metric * 64 + np.arange(S)
    best = key.argmin(1)						# the least metric, then the smallest state
    best_metric = metric[np.arange(J), best]
    end = np.zeros(J, np.int64) if terminated else best
    ends = np.stack([end, metric[np.arange(J), end], best, best_metric], 1).astype(np.int64)
    state, rows = end.copy(), np.arange(J)
    u = np.zeros((J, T), np.uint8)
    for t in range(T - 1, -1, -1):
        u[:, t] = state >> (k - 2)
        state = ((state << 1) | dec[t, rows, state]) & (S - 1)
    return ends, u


def buffer(case):
    return np.ascontiguousarray(case[0], np.float32).reshape(-1, 2)


def decode(case, variant=0):
    """(records RECORD_DTYPE [n_jobs], [the owned bytes per job, uint8]); variant: soft_values()'s"""
    iq, jobs = buffer(case), case[1]
    records, outs = np.zeros(len(jobs), RECORD_DTYPE), [None] * len(jobs)
    groups = {}
    for i, j in enumerate(jobs):
        T = shape(j)[0]
        groups.setdefault((T, int(j["k"]), tuple(int(v) for v in j["polys"]), int(j["n_poly"]), int(j["flags"]) & TERMINATED), []).append(i)
    for (T, k, polys, n_poly, term), members in groups.items():
        steps = [step_values(iq, jobs[i], T, variant) for i in members]
        ends, u = viterbi(np.stack([s[0] for s in steps]) if T else np.zeros((len(members), 0, 3), np.int64), k, polys, n_poly, term)
        for row, i in enumerate(members):
            j, r = jobs[i], records[i]
            _, n_bits, n_coded = shape(j)
            v, sent, erasures = steps[row]
            bits = u[row, :n_bits]
            r["n_steps"], r["n_bits"], r["n_coded"], r["k"], r["flags"] = T, n_bits, n_coded, k, j["flags"]
            r["end_state"], r["metric"], r["best_state"], r["best_metric"] = ends[row]
            r["crc_calc"], r["crc_recv"], r["status"] = dm.check_crc(bits, crc_of(j))
            r["erasures"], r["saturated"], r["abs_sum"] = erasures, int(((np.abs(v) == MAX_VALUE) & sent).sum()), int(np.abs(v)[sent].sum())
            outs[i] = dm.pack(bits)
    return records, outs


_IMAGES = {}


def image(case, fill, key=None):
    """(records, the whole output buffer as the model leaves it: uint8 [capacity], the byte `fill` wherever no job owns it); with a
    key the result is computed once for all the tests of a session"""
    if key is not None and (key, fill) in _IMAGES:
        return _IMAGES[(key, fill)]
    jobs = case[1]
    records, outs = decode(case)
    out = np.full(capacity(jobs), fill, np.uint8)
    for j, v in zip(jobs, outs):
        out[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v
    if key is not None:
        _IMAGES[(key, fill)] = (records, out)
    return records, out


def expected_stats(jobs):
    """the stats delta of one call over jobs"""
    steps = [shape(j)[0] for j in jobs]
    some = int(any(steps))
    return dict(calls=1, k_bits=some, k_acs=some, k_trace=some, k_rec=1, jobs_crc=int((jobs["crc_width"] > 0).sum()), steps=int(sum(steps)))


# ---- the modulator --------------------------------------------------------------------------------------------------------------

def modulate(sym, M, rot=0, gray=False, amp=1.0):
    """the bytes of decode_model.to_symbols (labels) as points: the inverse of rule S1, in float64 by numpy's cos and sin -> complex"""
    sym = np.asarray(sym, np.int64) & (M - 1)
    q = np.argsort(labels(M, gray))[sym]					# the value whose label it is
    return amp * np.exp(2j * np.pi * ((q + int(rot)) & (M - 1)) / M)


def pairs(z):
    """complex -> float32 [n][2]"""
    z = np.asarray(z, np.complex128)
    return np.stack([z.real, z.imag], 1).astype(np.float32)


def noise(rng, n, sigma):
    """complex white noise of standard deviation sigma a part"""
    return sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


# ---- the builders ---------------------------------------------------------------------------------------------------------------

def make_job(offset, out_offset, n, order, code, punct, crc=dm.CRC_NONE, steps=0, flags=0, rot=0, scale=32.0):
    j = np.zeros(1, JOB_DTYPE)
    k, polys = code
    j["offset"], j["out_offset"], j["n"], j["order"], j["steps"], j["flags"] = offset, out_offset, n, order, steps, flags
    j["k"], j["n_poly"], j["period"], j["crc_width"] = k, 3 if polys[2] else 2, punct[0], crc[0]
    j["polys"], j["punct"] = polys, punct[1]
    j["crc_poly"], j["crc_init"], j["crc_xorout"] = crc[1:]
    j["rot"], j["scale"] = rot, scale
    return j


def place(jobs):
    """the jobs with their owned bytes following each other, GUARD or 2 GUARD bytes between them"""
    jobs = np.concatenate(jobs) if len(jobs) else np.zeros(0, JOB_DTYPE)
    at = GUARD
    for i, j in enumerate(jobs):
        j["out_offset"] = at
        at += job_owned(j) + GUARD * (1 + (i & 1))
    return jobs


def noisy_frame(rng, n_info, code, punct, order, crc, terminated, rot, gray, sigma, amp=1.0):
    """an encoded frame as noisy symbols -> (iq float32 [n][2], T, info)"""
    info = rng.integers(0, 2, n_info)
    sym, T = dm.frame(info, code, punct, order, crc, terminated)
    z = modulate(sym, order, rot, gray, amp) + noise(rng, len(sym), sigma)
    return pairs(z), T, info


SEAM_STEPS = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
SEAM_CODES = ((dm.K7, dm.P_NONE), (dm.K3, dm.P_34), (dm.K5, dm.P_23), (dm.K7_THIRD, dm.P3_NONE), (dm.K7, dm.P_78), (dm.K4_THIRD, dm.P3_16),
              (dm.K7, dm.P_34), (CODES2[6], dm.P_16), (CODES3[5], PUNCT3[2]))


def seams_case():
    """T of SEAM_STEPS: across the 64-step block of k_sft_acs and k_sft_trace and the 256-step work-group of k_sft_bits, twice each,
    and jobs with T = 0 and with n = 0 among them.  The codes, puncture patterns, orders, labelings, rotations, CRC widths and
    TERMINATED take turns; noisy frames at about 3 dB so that soft values of every size occur and paths compete; the symbols of a
    job begin at odd and even samples; steps is 0 where the fewest symbols for T hold no step more, else T"""
    rng = np.random.default_rng(2424)
    parts, jobs, at, i = [], [], 0, 0
    for T in SEAM_STEPS:
        for rep in range(2):
            code, punct = SEAM_CODES[i % len(SEAM_CODES)]
            order = ORDERS[(i + rep) % 3]
            crc = dm.CRCS[i % 5]
            term = (i // 2 + rep) & 1
            gray, rot = (i >> 1) & 1, (3 * i + rep) % order
            n_info = max(T - (code[0] - 1 if term else 0) - crc[0], 0)
            info = rng.integers(0, 2, n_info)
            bits = dm.with_crc(info, crc) if n_info else np.zeros(0, np.uint8)
            if term:
                bits = np.concatenate([bits, np.zeros(code[0] - 1, np.uint8)])
            bits = np.concatenate([bits, rng.integers(0, 2, max(T - len(bits), 0)).astype(np.uint8)])[:T]	# a T below the tail and the CRC: any bits
            n_poly = 3 if code[1][2] else 2
            coded = dm.puncture(dm.encode(bits, code[0], code[1], n_poly), n_poly, punct[0], punct[1])
            sym = dm.to_symbols(coded, order)
            n = dm.symbols_for(T, order, punct)
            assert len(sym) == n
            z = modulate(sym, order, rot, gray, 0.8 + 0.1 * (i % 5)) + noise(rng, n, 0.5)
            lead = 1 + i % 2						# samples that belong to no job, so that offsets are odd and even
            parts += [pairs(noise(rng, lead, 1.0)), pairs(z)]
            fits = dm.steps_that_fit(n, order, punct[0], punct[1]) == T
            jobs.append(make_job(at + lead, 0, n, order, code, punct, crc, 0 if fits else T, term | (GRAY if gray else 0), rot, 20.0 + 7 * (i % 4)))
            at += lead + n
            i += 1
            if i % 5 == 0:						# no step: no symbol, or fewer than a step needs
                jobs.append(make_job(at, 0, 0, 4, dm.K7, dm.P_NONE, dm.CRC16 if i % 10 else dm.CRC_NONE, 0, TERMINATED if i % 3 else 0, 0, 1.0))
                jobs.append(make_job(max(at - 1, 0), 0, 1, 2, dm.K5, dm.P_NONE, dm.CRC_NONE, 0, GRAY, 1, 3.0))	# one BPSK symbol, two bits a step
    return np.concatenate(parts), place(jobs)


def nan_case():
    """NaN, infinite and zero parts among live symbols, every order and labeling: erasures, NaN correlations, ties"""
    rng = np.random.default_rng(2525)
    parts, jobs, at = [], [], 0
    odd = np.array([[np.nan, 1.0], [1.0, np.nan], [np.nan, np.nan], [np.inf, 1.0], [1.0, -np.inf], [np.inf, np.inf], [-np.inf, np.nan],
                    [0.0, 0.0], [-0.0, 0.0], [np.inf, 0.0], [0.0, -np.inf], [3e38, 3e38], [1e-45, 0.0]], np.float32)
    for i, order in enumerate(ORDERS):
        for gray in (0, 1):
            code, punct = ((dm.K7, dm.P_34), (dm.K5, dm.P_NONE), (dm.K7_THIRD, dm.P3_NONE))[i]
            iq, T, info = noisy_frame(rng, 150, code, punct, order, dm.CRC16, True, i + gray, gray, 0.3)
            where = rng.choice(len(iq), 3 * len(odd), replace=False)
            iq[where] = np.tile(odd, (3, 1))
            parts.append(iq)
            jobs.append(make_job(at, 0, len(iq), order, code, punct, dm.CRC16, T, TERMINATED | (GRAY if gray else 0), i + gray, 40.0))
            at += len(iq)
    whole = np.full((40, 2), np.nan, np.float32)				# every symbol a NaN: all ties, zeros come out
    parts.append(whole)
    jobs.append(make_job(at, 0, 40, 4, dm.K7, dm.P_NONE, dm.CRC8, 0, 0, 2, 1.0))
    return np.concatenate(parts), place(jobs)


def max_steps_case():
    """one job of MAX_STEPS: K = 7 at rate 1/2, QPSK, Gray, CRC-16, TERMINATED, a noisy frame at about 4 dB"""
    rng = np.random.default_rng(2626)
    iq, T, info = noisy_frame(rng, MAX_STEPS - 6 - 16, dm.K7, dm.P_NONE, 4, dm.CRC16, True, 3, True, 0.45)
    assert T == MAX_STEPS
    return iq, place([make_job(0, 0, len(iq), 4, dm.K7, dm.P_NONE, dm.CRC16, 0, TERMINATED | GRAY, 3, 32.0)])


FULL_CODES = ((dm.K7, dm.P_34, 4, dm.CRC8), (dm.K5, dm.P_NONE, 2, dm.CRC_NONE), (dm.K7_THIRD, dm.P3_NONE, 8, dm.CRC16))


def full_table_case():
    """MAX_JOBS jobs in shuffled order over noise, three codes, n <= 40, every 11th with n = 0: the deepest search of the prefix"""
    rng = np.random.default_rng(4096)
    iq = pairs(noise(rng, 300, 1.0))
    jobs = []
    for i in rng.permutation(MAX_JOBS):
        i = int(i)
        code, punct, order, crc = FULL_CODES[i % 3]
        n = 0 if i % 11 == 0 else 1 + (i // 3) % 40
        jobs.append(make_job(int(rng.integers(0, 260)), 0, n, order, code, punct, crc, 0, ((i // 5) & 1) | (GRAY if i & 8 else 0), i % order, 10.0 + i % 50))
    return iq, place(jobs)


# ---- one crafted symbol a job: the edges of rule S2, and symbols that tell a contracted correlation -----------------------------

F32_MAX = float(np.finfo(np.float32).max)


def value_job(at, order=2, rot=0, gray=0, scale=1.0):
    """one step over the crafted symbol iq[at] whose bits it consumes exactly, so that the record carries the symbol's soft values
    out -> (symbols of the job, the job).  BPSK: K = 3 (7, 5) at rate 1/2, and a second symbol (0, 0) that is worth nothing:
    abs_sum is |v| and the decoded bit is 1 exactly when v < 0 (input 1 sends 11).  QPSK: the same code, one symbol.  8-PSK: K = 4
    at rate 1/3, one symbol.  There abs_sum is the sum of the |v|, metric what the cheaper input pays, and the decoded bit says
    which it was"""
    code, n = {2: (dm.K3, 2), 4: (dm.K3, 1), 8: (dm.K4_THIRD, 1)}[order]
    return n, make_job(at, 0, n, order, code, dm.P3_NONE if order == 8 else dm.P_NONE, dm.CRC_NONE, 1, GRAY if gray else 0, rot, scale)


# BPSK at rot 0: the points are (1, +0) and (-1, -0), L = 2 sr exactly, x = 2 sr scale + 0.5.  (sr, scale, the v of rule S2)
EDGE_VALUES = ((0.25, 1.0, 1), (0.75, 1.0, 2), (-0.25, 1.0, 0), (-0.75, 1.0, -1), (1.25, 1.0, 3), (-1.25, 1.0, -2),	# x at an integer: L at a half
               (0.24999999, 1.0, 0), (0.75, 0.99999994, 1), (63.25, 1.0, 127), (63.0, 1.0, 126), (63.5, 1.0, 127), (1e30, 1.0, 127),
               (-63.5, 1.0, -127), (-63.25, 1.0, -126), (-63.75, 1.0, -127), (-64.0, 1.0, -127), (-1e30, 1e30, -127),
               (3e38, 3e38, 127), (np.inf, 1.0, 127), (-np.inf, 1.0, -127), (1e-30, 1e-30, 0), (0.0, 1e6, 0), (-0.0, 1e6, 0))
# what a flush of float32 subnormals to zero would change: a subnormal symbol under the largest scale (L = 2e-38, x = 7.3; flushed,
# v = 0) and a subnormal scale under a large symbol (L = 6e38, x = 1.1; flushed, the scale is 0 and v = 0)
EDGE_SUBNORMAL = ((1e-38, F32_MAX, 7), (3e38, 1e-39, 1))
# a NaN part: v = 0 and one erasure, whatever the other part is
EDGE_NAN = ((np.nan, 0.0), (1.0, np.nan), (np.nan, np.nan), (np.inf, np.nan), (np.nan, -np.inf))
# an infinite imaginary part meets the zero of the points' sines: both correlations are NaN, none is the largest,
# L = -inf - -inf is a NaN: v = 0, and no erasure
EDGE_INF = ((1.0, np.inf), (-1.0, -np.inf), (np.inf, np.inf))
# 4- and 8-PSK: symbols on the axes and the diagonals, where two correlations tie or L = 0 ((1, 1) lies on a decision boundary of
# QPSK at rot 0 and on a point of 8-PSK, (0, 1) on a point of both), and one symbol off them all; two scales, the second puts
# L = 1 on a half
EDGE_PSK_SYMBOLS = ((1.0, 1.0), (0.0, 1.0), (-1.0, 1.0), (-1.0, 0.0), (-1.0, -1.0), (0.0, -1.0), (1.0, -1.0), (1.0, 0.0), (0.5, 0.25))
EDGE_PSK_SCALES = (10.0, 63.5)
EDGE_ODD = (np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 3e38, 1e-45, np.nan)
EDGE_ODD_SCALES = (1e-3, 1.0, 3e38)


def edge_rows():
    """the one-symbol jobs of the "edges" case, in its order: (sr, si, order, rot, gray, scale, the expected v of bit 0 or None,
    the expected erasures or None)"""
    rows = [(sr, 0.0, 2, 0, 0, scale, want, 0) for sr, scale, want in EDGE_VALUES + EDGE_SUBNORMAL]
    rows += [(sr, si, 2, 0, 0, 32.0, 0, 1) for sr, si in EDGE_NAN]
    rows += [(sr, si, 2, 0, 0, 32.0, 0, 0) for sr, si in EDGE_INF]
    for order in (4, 8):
        for gray in (0, 1):
            for rot in (0, order - 1):
                for scale in EDGE_PSK_SCALES:
                    rows += [(sr, si, order, rot, gray, scale, None, 0) for sr, si in EDGE_PSK_SYMBOLS]
    return rows


def edge_odd_jobs(at):
    """36 jobs over the same 600 symbols at iq[at]: every order, labeling, rot = 0 and M - 1, three scales"""
    return [make_job(at, 0, 600, order, dm.K5, dm.P_NONE, dm.CRC8, 0, gray * GRAY, rot, scale)
            for order in ORDERS for gray in (0, 1) for rot in (0, order - 1) for scale in EDGE_ODD_SCALES]


def edges_case():
    """the numerical edges of rule S2, a job a crafted value (scale is a job field): halves that round upwards, 126 / 127 and
    -126 / -127, x < -127, infinity minus infinity, NaN correlations beside live ones, +-0, scales from 1e-3 to 3e38, float32
    subnormals that must survive the widening to double, 4- and 8-PSK symbols on decision boundaries and on points at rot = 0 and
    M - 1 under both labelings; then 36 jobs over 600 symbols drawn from +-inf, +-0, +-1, 3e38, 1e-45 and NaN"""
    rows = edge_rows()
    parts, jobs, at = [], [], 0
    for sr, si, order, rot, gray, scale, _, _ in rows:
        n, job = value_job(at, order, rot, gray, scale)
        parts.append(np.array([[sr, si], [0.0, 0.0]][:n], np.float32))
        jobs.append(job)
        at += n
    rng = np.random.default_rng(5)
    odd = np.array(EDGE_ODD, np.float32)
    parts.append(np.stack([rng.choice(odd, 600), rng.choice(odd, 600)], 1))
    jobs += edge_odd_jobs(at)
    return np.concatenate(parts), place(jobs)


# the correlation of rule S2 and the two ways a compiler may contract it
S2, FMA_RE, FMA_IM = 0, 1, 2
CONTRACT_DRAWS, CONTRACT_NEAR, CONTRACT_MAX_JOBS = 100000, 1e-9, 128
_CONTRACT = {}


def corr_variants(sr, si, c, s):
    """(sr c) + (si s) over doubles in exact rational arithmetic, each IEEE operation rounded once (int / int rounds correctly)
    -> [rule S2: three roundings, fma(sr, c, round(si s)), fma(si, s, round(sr c))]"""
    from fractions import Fraction
    a, b = Fraction(sr) * Fraction(c), Fraction(si) * Fraction(s)
    ra, rb = Fraction(float(a)), Fraction(float(b))
    return [float(ra + rb), float(a + rb), float(ra + b)]


def contracted_values(y, M, rot, gray, scale, variant):
    """soft_values() of one finite symbol y = (sr, si) with the correlations of corr_variants()[variant] -> v [b]"""
    b = dm.bits_of(M)
    C, S = points(M, rot)
    corr = np.array([corr_variants(float(y[0]), float(y[1]), float(C[q]), float(S[q]))[variant] for q in range(M)])
    lab = labels(M, gray)
    v = []
    for i in range(b):
        bit = (lab >> (b - 1 - i)) & 1
        x = ((corr[bit == 0].max() - corr[bit == 1].max()) * np.float64(np.float32(scale))) + 0.5
        v.append(int(np.clip(np.floor(x), -MAX_VALUE, MAX_VALUE)))
    return v


def _scale_between(lo, hi, seed):
    """a float32 scale with a half-integer n - 0.5, 1 <= n <= 126, between lo scale and hi scale, 0 < lo < hi: floor(x) of rule S2
    steps there, for either sign of L.  Four n are tried, from a start that `seed` picks, and four neighbouring scales each"""
    for n in [1 + (seed + 37 * t) % 126 for t in range(4)]:
        scale = np.float32((n - 0.5) / hi)
        for _ in range(4):
            if np.floor(lo * np.float64(scale) + 0.5) != np.floor(hi * np.float64(scale) + 0.5):
                return scale
            scale = np.nextafter(scale, np.float32(np.inf))
    return None


def contract_search():
    """-> (iq float32 [n][2], [(rot, gray, scale)]): 8-PSK symbols on which the quantised values of rule S2 differ from those of a
    correlation contracted either way.  Seeded, CONTRACT_DRAWS draws, at most CONTRACT_MAX_JOBS kept; once a session.

    Such a symbol lies within about 1e-9 (relative) of the boundary between two neighbouring points, one on an axis, whose
    correlation is exact, and one on a diagonal, whose correlation is rounded three times by rule S2 and twice by a fused
    multiply-add.  L is then the exact difference of the two, a few million ulps of them, and where both contractions move the
    diagonal's correlation by an ulp to the same side, a float32 scale puts a half-integer of L scale between rule S2's L and
    theirs.  Draw u, set w = float32(u tan(3 pi / 8)); (u, w) lies at 3/16 of a turn, and swapping and negating the parts gives the
    other seven boundaries, which take turns with the labelings and rot = 0 and 5."""
    if "search" in _CONTRACT:
        return _CONTRACT["search"]
    rng = np.random.default_rng(2727)
    u = rng.uniform(0.25, 4.0, CONTRACT_DRAWS).astype(np.float32)
    w = (u.astype(np.float64) * np.tan(3 * np.pi / 8)).astype(np.float32)
    i = np.arange(CONTRACT_DRAWS)
    swap, neg_re, neg_im = (i & 1).astype(bool), (i & 2).astype(bool), (i & 4).astype(bool)
    re, im = np.where(swap, w, u), np.where(swap, u, w)
    y = np.stack([np.where(neg_re, -re, re), np.where(neg_im, -im, im)], 1).astype(np.float32)
    gray, rot = (i >> 3) & 1, np.where((i >> 4) & 1, 5, 0)
    found_y, found = [], []
    for r in (0, 5):
        C, S = points(8, r)
        sel = np.flatnonzero(rot == r)
        sr, si = y[sel, 0].astype(np.float64), y[sel, 1].astype(np.float64)
        corr = (sr[:, None] * C[None, :]) + (si[:, None] * S[None, :])
        top = np.argsort(corr, 1)[:, -2:]						# the second largest, the largest
        c2, c1 = corr[np.arange(len(sel)), top[:, 0]], corr[np.arange(len(sel)), top[:, 1]]
        near = np.flatnonzero((c1 - c2 > 0) & (c1 - c2 < CONTRACT_NEAR * c1))
        for m in near:
            d = [a - b for a, b in zip(corr_variants(sr[m], si[m], C[top[m, 1]], S[top[m, 1]]),
                                       corr_variants(sr[m], si[m], C[top[m, 0]], S[top[m, 0]]))]
            if min(d) <= 0 or d[FMA_RE] == d[S2] or d[FMA_IM] == d[S2] or (d[FMA_RE] > d[S2]) != (d[FMA_IM] > d[S2]):
                continue								# both contractions have to move L, to the same side
            lo, hi = sorted((d[S2], min(d[1:]) if d[FMA_RE] > d[S2] else max(d[1:])))
            k = int(sel[m])
            scale = _scale_between(lo, hi, k)
            if scale is None:
                continue
            v = [contracted_values(y[k], 8, r, gray[k], scale, variant) for variant in (S2, FMA_RE, FMA_IM)]
            if v[FMA_RE] != v[S2] and v[FMA_IM] != v[S2]:
                found_y.append(y[k])
                found.append((k, r, int(gray[k]), float(scale)))
    order = np.argsort([f[0] for f in found])[:CONTRACT_MAX_JOBS]			# in the order drawn
    _CONTRACT["search"] = (np.array([found_y[o] for o in order], np.float32).reshape(-1, 2), [found[o][1:] for o in order])
    return _CONTRACT["search"]


def contract_case():
    """one 8-PSK symbol a job, each a job on which rule S2's record differs from the record with the correlation contracted either
    way, fma(sr, C_q, round(si S_q)) or fma(si, S_q, round(sr C_q)) (contract_search(), contract_records()): what a build without
    -ffp-contract=off, a pragma or a compiler that fuses the correlation gives away.  The contraction of the last operation,
    (L scale) + 0.5, is not covered: with these L the product is exact, and an input that separates it needs a product within
    2^-54 below -0.5"""
    y, found = contract_search()
    jobs = [value_job(i, 8, rot, gray, scale)[1] for i, (rot, gray, scale) in enumerate(found)]
    return y, place(jobs)


def contract_records():
    """the records of contract_case() under [rule S2, either contraction]; once a session"""
    if "records" not in _CONTRACT:
        _CONTRACT["records"] = [decode(contract_case(), variant)[0] for variant in (S2, FMA_RE, FMA_IM)]
    return _CONTRACT["records"]


# ---- a call at MAX_CALL_STEPS -----------------------------------------------------------------------------------------------------

LIMIT_JOBS = MAX_CALL_STEPS // MAX_STEPS
_LIMIT = []


def call_limit_case():
    """64 jobs of MAX_STEPS, exactly MAX_CALL_STEPS, in shuffled order with place()'s guards; two shapes, so that the model decodes
    the jobs of a shape together: K = 7 at rate 1/2, QPSK, Gray, CRC-16, TERMINATED at scale 32, and K = 7 at rate 1/3, 8-PSK,
    CRC-32 at scale 1e6, which saturates nearly every value: abs_sum and metric are the largest a job can produce.  Noisy frames at
    the level of max_steps_case().  Not in cases(): the model takes its time for it.  Once a session"""
    if _LIMIT:
        return _LIMIT[0]
    rng = np.random.default_rng(2828)
    parts, jobs, at = [], [], 0
    for i in rng.permutation(LIMIT_JOBS):
        if i & 1:
            iq, T, _ = noisy_frame(rng, MAX_STEPS - 32, dm.K7_THIRD, dm.P3_NONE, 8, dm.CRC32, False, int(i) % 8, (i >> 1) & 1, 0.45)
            job = make_job(at, 0, len(iq), 8, dm.K7_THIRD, dm.P3_NONE, dm.CRC32, 0, GRAY if (i >> 1) & 1 else 0, int(i) % 8, 1e6)
        else:
            iq, T, _ = noisy_frame(rng, MAX_STEPS - 6 - 16, dm.K7, dm.P_NONE, 4, dm.CRC16, True, int(i) % 4, True, 0.45)
            job = make_job(at, 0, len(iq), 4, dm.K7, dm.P_NONE, dm.CRC16, 0, TERMINATED | GRAY, int(i) % 4, 32.0)
        assert T == MAX_STEPS
        parts.append(iq)
        jobs.append(job)
        at += len(iq)
    _LIMIT.append((np.concatenate(parts), place(jobs)))
    return _LIMIT[0]


def one_step_more(case):
    """the case with one more job of one step behind its table: a step past MAX_CALL_STEPS"""
    iq, jobs = case
    return iq, place([jobs.copy(), value_job(0, 4)[1]])


def cases():
    """name -> (iq, jobs): every set the CPU and GPU tests share"""
    return {"seams": seams_case(), "nan": nan_case(), "max_steps": max_steps_case(), "full_table": full_table_case(),
            "edges": edges_case(), "contract": contract_case()}
