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


def soft_values(y, M, rot, gray, scale):
    """rules S1 and S2 over float32 y [n][2] -> (v int64 [n][b], a part is a NaN: bool [n])"""
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
    return v, nan


def step_values(iq, job, T):
    """rules 2 and S2 -> (v int64 [T][3], 0 where a stream's bit was not sent; sent bool [T][3]; erasures)"""
    M, b, n_poly = int(job["order"]), dm.bits_of(job["order"]), int(job["n_poly"])
    at, n = int(job["offset"]), int(job["n"])
    v, nan = soft_values(iq[at:at + n], M, job["rot"], int(job["flags"]) & GRAY, job["scale"])
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


def decode(case):
    """(records RECORD_DTYPE [n_jobs], [the owned bytes per job, uint8])"""
    iq, jobs = buffer(case), case[1]
    records, outs = np.zeros(len(jobs), RECORD_DTYPE), [None] * len(jobs)
    groups = {}
    for i, j in enumerate(jobs):
        T = shape(j)[0]
        groups.setdefault((T, int(j["k"]), tuple(int(v) for v in j["polys"]), int(j["n_poly"]), int(j["flags"]) & TERMINATED), []).append(i)
    for (T, k, polys, n_poly, term), members in groups.items():
        steps = [step_values(iq, jobs[i], T) for i in members]
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


def cases():
    """name -> (iq, jobs): every set the CPU and GPU tests share"""
    return {"seams": seams_case(), "nan": nan_case(), "max_steps": max_steps_case(), "full_table": full_table_case()}
