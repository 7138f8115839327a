"""numpy statement of rules 1-7 of include/fosphor_amd_decode.h, an encoder, and the input sets the CPU and GPU tests share.

A case is (sym, jobs): sym uint8 [n_bytes], one symbol a byte as fosphor_amd_decide leaves them, and jobs a JOB_DTYPE array whose
owned bytes are placed with GUARD or 2 GUARD bytes before, between and behind them (place()).  Everything is integer work, written
from the header's rules alone: the trellis as arrays over the S states, the jobs of one shape (steps, code, puncture pattern)
decoded together, one more array axis.  The decoder keeps every survivor decision and traces the whole frame back."""
import numpy as np

JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("order", "<i4"), ("steps", "<i4"), ("flags", "<i4"),
                      ("k", "u1"), ("n_poly", "u1"), ("period", "u1"), ("crc_width", "u1"), ("polys", "<u2", (3,)),
                      ("punct", "<u2", (3,)), ("crc_poly", "<u4"), ("crc_init", "<u4"), ("crc_xorout", "<u4"), ("reserved", "<u4")])
RECORD_DTYPE = np.dtype([("n_steps", "<i4"), ("n_bits", "<i4"), ("n_coded", "<i4"), ("status", "<i4"), ("end_state", "<i4"),
                         ("metric", "<i4"), ("best_state", "<i4"), ("best_metric", "<i4"), ("crc_calc", "<u4"), ("crc_recv", "<u4"),
                         ("k", "<i4"), ("flags", "<i4"), ("reserved", "<i4", (4,))])
STATS = ("calls", "k_bits", "k_acs", "k_trace", "k_rec", "jobs_crc", "steps")
MAX_JOBS, MAX_STEPS, MAX_CALL_STEPS, BLOCK, INF = 4096, 65536, 1 << 22, 64, 1 << 24
TERMINATED = 1
FLAGS = {"terminated": TERMINATED}
OK, CRC_FAIL, SHORT = 0, 1, 2
STATUS = {"ok": OK, "crc_fail": CRC_FAIL, "short": SHORT}
ORDERS = (2, 4, 8)
RECORD_WORDS = RECORD_DTYPE.itemsize // 4
GUARD = 8						# sentinel bytes before, between (or twice as many) and behind the jobs' owned bytes

# codes: (k, polys); puncture patterns of a two-stream code: (period, masks); CRCs: (width, poly, init, xorout)
K3, K4_THIRD, K5, K7, K7_THIRD = (3, (0o7, 0o5, 0)), (4, (0o13, 0o15, 0o17)), (5, (0o23, 0o35, 0)), (7, (0o171, 0o133, 0)), (7, (0o171, 0o133, 0o165))
P_NONE, P_23, P_34, P_78, P_16 = (1, (1, 1, 0)), (2, (0b11, 0b01, 0)), (3, (0b011, 0b101, 0)), (7, (0b1010001, 0b0101111, 0)), (16, (0xffff, 0x5a5a, 0))
P3_NONE, P3_16 = (1, (1, 1, 1)), (16, (0xf0f0, 0x0ff0, 0x8001))		# three streams; the second sends nothing in steps 1 .. 3 of 16
CRC_NONE, CRC8, CRC16, CRC24, CRC32 = (0, 0, 0, 0), (8, 0x07, 0, 0), (16, 0x1021, 0xffff, 0), (24, 0x864cfb, 0xb704ce, 0), (32, 0x04c11db7, 0xffffffff, 0)
CRCS = (CRC_NONE, CRC8, CRC16, CRC24, CRC32)


def bits_of(order):
    return {2: 1, 4: 2, 8: 3}[int(order)]


def popcount(v):
    return bin(int(v)).count("1")


def kept(T, period, punct):
    """rule 2"""
    below = (1 << (T % period)) - 1
    return (T // period) * sum(popcount(m) for m in punct) + sum(popcount(int(m) & below) for m in punct)


def steps_that_fit(n, order, period, punct):
    """rule 2: the largest T with kept(T) <= n b"""
    coded, W = int(n) * bits_of(order), sum(popcount(m) for m in punct)
    T = (coded // W) * period
    while kept(T + 1, period, punct) <= coded:
        T += 1
    return T


def shape(job):
    """(T, n_bits, n_coded) of a job"""
    period, punct = int(job["period"]), [int(m) for m in job["punct"]]
    T = int(job["steps"]) or steps_that_fit(job["n"], job["order"], period, punct)
    n_bits = max(T - (int(job["k"]) - 1), 0) if int(job["flags"]) & TERMINATED else T
    return T, n_bits, kept(T, period, punct)


def owned(n_bits):
    return 8 * ((int(n_bits) + 63) // 64)


def job_owned(job):
    return owned(shape(job)[1])


def sent_of(T, n_poly, period, punct):
    """bool [T][3]: stream i's bit of step t was sent"""
    phase = np.arange(T) % period
    return np.stack([((int(punct[i]) >> phase) & 1).astype(bool) if i < n_poly else np.zeros(T, bool) for i in range(3)], 1)


def codes_of(sym, job, T):
    """rules 1 and 2 -> the code bytes of the job's steps, uint8 [T]: received bits in bits 0 .. 2, erased flags in bits 4 .. 6"""
    b, n_poly = bits_of(job["order"]), int(job["n_poly"])
    at, n = int(job["offset"]), int(job["n"])
    coded = ((sym[at:at + n, None].astype(np.int64) >> (b - 1 - np.arange(b))) & 1).reshape(-1)
    sent = sent_of(T, n_poly, int(job["period"]), job["punct"])
    q = np.cumsum(sent.reshape(-1)) - sent.reshape(-1)			# kept bits before this one, step by step, stream by stream
    recv = np.where(sent.reshape(-1), coded[np.minimum(q, max(len(coded) - 1, 0))] if len(coded) else 0, 0).reshape(T, 3)
    erased = np.stack([~sent[:, i] if i < n_poly else np.zeros(T, bool) for i in range(3)], 1)
    return ((recv << np.arange(3)).sum(1) | ((erased.astype(np.int64) << (4 + np.arange(3))).sum(1))).astype(np.uint8)


def parity(v):
    v = np.asarray(v, np.int64)
    out = np.zeros_like(v)
    for i in range(8):
        out ^= (v >> i) & 1
    return out


def trellis(k, polys, n_poly):
    """rule 3 -> (p [2][S], cost [2][128][S]: the branch cost of predecessor x into state s' under code byte c)"""
    S = 1 << (k - 1)
    s = np.arange(S)
    u = s >> (k - 2)
    p = np.stack([((s << 1) | x) & (S - 1) for x in (0, 1)])
    c = np.arange(128)
    cost = np.zeros((2, 128, S), np.int32)
    for x in (0, 1):
        R = (u << (k - 1)) | p[x]
        for i in range(n_poly):
            e = parity(int(polys[i]) & R)					# [S]
            counts = ((c >> (4 + i)) & 1) == 0				# sent
            cost[x] += (counts[:, None] & (((c >> i) & 1)[:, None] != e[None, :])).astype(np.int32)
    return p, cost


def viterbi(codes, k, polys, n_poly, terminated):
    """rules 3-5 over codes uint8 [J][T] of J jobs of one shape -> (ends int [J][4], the decoded inputs u_t uint8 [J][T])"""
    J, T = codes.shape
    S = 1 << (k - 1)
    if T == 0:
        return np.zeros((J, 4), np.int64), np.zeros((J, 0), np.uint8)
    p, cost = trellis(k, polys, n_poly)
    metric = np.full((J, S), INF, np.int32)
    metric[:, 0] = 0
    dec = np.zeros((T, J, S), bool)
    for t in range(T):
        c = codes[:, t]
        c0 = metric[:, p[0]] + cost[0][c]
        c1 = metric[:, p[1]] + cost[1][c]
        one = c1 < c0							# ties go to x = 0
        metric = np.where(one, c1, c0)
        dec[t] = one
    key = metric.astype(np.int64) * 64 + np.arange(S)
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


def crc_bits(bits, crc):
    """rule 7's register over bits -> crc_calc"""
    w, poly, init, xorout = crc
    mask, reg = (1 << w) - 1, init
    for bit in bits:
        top = ((reg >> (w - 1)) & 1) ^ int(bit)
        reg = (reg << 1) & mask
        if top:
            reg ^= poly
    return reg ^ xorout


def check_crc(bits, crc):
    """rule 7 -> (crc_calc, crc_recv, status)"""
    w = crc[0]
    if w == 0:
        return 0, 0, OK
    if len(bits) < w:
        return 0, 0, SHORT
    calc = crc_bits(bits[:len(bits) - w], crc)
    recv = 0
    for bit in bits[len(bits) - w:]:
        recv = (recv << 1) | int(bit)
    return calc, recv, OK if calc == recv else CRC_FAIL


def pack(bits):
    """rule 6 -> the job's owned bytes"""
    out = np.zeros(owned(len(bits)), np.uint8)
    packed = np.packbits(np.asarray(bits, np.uint8))			# MSB first
    out[:len(packed)] = packed
    return out


def crc_of(job):
    return tuple(int(job[f]) for f in ("crc_width", "crc_poly", "crc_init", "crc_xorout"))


def decode(case):
    """(records RECORD_DTYPE [n_jobs], [the owned bytes per job, uint8])"""
    sym, jobs = np.ascontiguousarray(case[0], np.uint8).reshape(-1), case[1]
    records, outs = np.zeros(len(jobs), RECORD_DTYPE), [None] * len(jobs)
    groups = {}
    for i, j in enumerate(jobs):
        T = shape(j)[0]
        groups.setdefault((T, int(j["k"]), tuple(int(v) for v in j["polys"]), int(j["n_poly"]), int(j["flags"]) & TERMINATED), []).append(i)
    for (T, k, polys, n_poly, term), members in groups.items():
        codes = np.stack([codes_of(sym, jobs[i], T) for i in members]) if T else np.zeros((len(members), 0), np.uint8)
        ends, u = viterbi(codes, k, polys, n_poly, term)
        for row, i in enumerate(members):
            j, r = jobs[i], records[i]
            _, n_bits, n_coded = shape(j)
            bits = u[row, :n_bits]
            r["n_steps"], r["n_bits"], r["n_coded"], r["k"], r["flags"] = T, n_bits, n_coded, k, j["flags"]
            r["end_state"], r["metric"], r["best_state"], r["best_metric"] = ends[row]
            r["crc_calc"], r["crc_recv"], r["status"] = check_crc(bits, crc_of(j))
            outs[i] = pack(bits)
    return records, outs


def unpack(out, n_bits):
    return np.unpackbits(np.asarray(out, np.uint8))[:n_bits]


def capacity(jobs):
    """bytes of the output buffer of a case: the last owned byte and GUARD behind it"""
    return max([int(j["out_offset"]) + job_owned(j) for j in jobs] + [0]) + GUARD


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


# ---- the encoder ----------------------------------------------------------------------------------------------------------------

def encode(bits, k, polys, n_poly):
    """rule 3 from state 0 -> the streams' bits uint8 [len(bits)][n_poly]"""
    u = np.concatenate([np.zeros(k - 1, np.int64), np.asarray(bits, np.int64)])
    T = len(bits)
    out = np.zeros((T, n_poly), np.int64)
    for i in range(n_poly):
        for j in range(k):							# bit j of R is u[t - (k - 1 - j)]
            if (int(polys[i]) >> j) & 1:
                out[:, i] ^= u[j:j + T]
    return out.astype(np.uint8)


def puncture(streams, n_poly, period, punct):
    """rule 2 -> the kept bits in the order sent"""
    sent = sent_of(len(streams), n_poly, period, punct)[:, :n_poly]
    return streams[sent]


def to_symbols(coded, order, junk=None):
    """rule 1 -> one byte a symbol, the last filled up with 0 bits; junk: a generator that sets bits above b"""
    b = bits_of(order)
    coded = np.concatenate([np.asarray(coded, np.int64), np.zeros(-len(coded) % b, np.int64)]).reshape(-1, b)
    sym = (coded << (b - 1 - np.arange(b))).sum(1)
    if junk is not None:
        sym = sym | (junk.integers(0, 256, len(sym)) & ~(order - 1) & 0xff)
    return sym.astype(np.uint8)


def with_crc(info, crc):
    """the info bits and their CRC behind them, MSB first"""
    if crc[0] == 0:
        return np.asarray(info, np.uint8)
    v = crc_bits(info, crc)
    return np.concatenate([np.asarray(info, np.uint8), [(v >> (crc[0] - 1 - i)) & 1 for i in range(crc[0])]]).astype(np.uint8)


def frame(info, code, punct, order, crc=CRC_NONE, terminated=True, flips=(), junk=None):
    """the symbols of a frame: info bits, their CRC, the tail, encoded, punctured, `flips` coded bits inverted -> (sym, T)"""
    k, polys = code
    n_poly = 3 if polys[2] else 2
    bits = with_crc(info, crc)
    if terminated:
        bits = np.concatenate([bits, np.zeros(k - 1, np.uint8)])
    coded = puncture(encode(bits, k, polys, n_poly), n_poly, punct[0], punct[1]).copy()
    for f in flips:
        coded[f] ^= 1
    return to_symbols(coded, order, junk), len(bits)


# ---- the builders ---------------------------------------------------------------------------------------------------------------

def make_job(offset, out_offset, n, order, code, punct, crc=CRC_NONE, steps=0, flags=0):
    j = np.zeros(1, JOB_DTYPE)
    k, polys = code
    j["offset"], j["out_offset"], j["n"], j["order"], j["steps"], j["flags"] = offset, out_offset, n, order, steps, flags
    j["k"], j["n_poly"], j["period"], j["crc_width"] = k, 3 if polys[2] else 2, punct[0], crc[0]
    j["polys"], j["punct"] = polys, punct[1]
    j["crc_poly"], j["crc_init"], j["crc_xorout"] = crc[1:]
    return j


def place(jobs):
    """the jobs with their owned bytes following each other, GUARD or 2 GUARD bytes between them"""
    jobs = np.concatenate(jobs) if len(jobs) else np.zeros(0, JOB_DTYPE)
    at = GUARD
    for i, j in enumerate(jobs):
        j["out_offset"] = at
        at += job_owned(j) + GUARD * (1 + (i & 1))
    return jobs


def symbols_for(T, order, punct):
    """the fewest symbols that hold T steps"""
    b = bits_of(order)
    return (kept(T, punct[0], punct[1]) + b - 1) // b


SEAM_STEPS = (0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)
SEAM_CODES = ((K3, P_NONE), (K3, P_34), (K5, P_23), (K5, P_78), (K7, P_NONE), (K7, P_34), (K7, P_16), (K4_THIRD, P3_NONE), (K7_THIRD, P3_16),
              (K7_THIRD, P3_NONE), (K7, P_78), (K5, P_16))


def seams_case():
    """T of SEAM_STEPS and k - 2, k - 1, k at k = 3, 5 and 7 (and 4 at rate 1/3), over random bytes: every second coded bit an
    error, ties abound, bits above b set.  The codes, puncture patterns, orders, CRC widths and TERMINATED take turns; the input
    offsets run through 0 .. 3 mod 4; steps is 0 where the fewest symbols for T hold no step more, else T"""
    rng = np.random.default_rng(2323)
    sym = rng.integers(0, 256, 16384).astype(np.uint8)
    jobs, i = [], 0
    for code in (K3, K5, K7, K4_THIRD, K7_THIRD):
        k = code[0]
        for T in SEAM_STEPS + (k - 2, k - 1, k):
            for rep in range(2):
                punct = [pc[1] for pc in SEAM_CODES if pc[0] is code][(i + rep) % sum(pc[0] is code for pc in SEAM_CODES)]
                order = ORDERS[(i + rep) % 3]
                n = symbols_for(T, order, punct)
                fits = steps_that_fit(n, order, punct[0], punct[1]) == T
                offset = int(rng.integers(0, 64)) * 4 + i % 4
                jobs.append(make_job(offset, 0, n, order, code, punct, CRCS[i % 5], 0 if fits else T, (i // 2 + rep) & 1))
                i += 1
    # a job that ends on the buffer's last byte
    jobs.append(make_job(len(sym) - 301, 0, 301, 8, K7, P_34, CRC16, 0, TERMINATED))
    return sym, place(jobs)


def codes_case():
    """every code and puncture pattern of SEAM_CODES at every order, 700 steps, with and without TERMINATED, over random bytes"""
    rng = np.random.default_rng(2424)
    sym = rng.integers(0, 256, 4096).astype(np.uint8)
    jobs = []
    for i, (code, punct) in enumerate(SEAM_CODES):
        for m, order in enumerate(ORDERS):
            T = 700 + i + m
            jobs.append(make_job(17 * i + m, 0, symbols_for(T, order, punct) + m, order, code, punct, CRCS[(i + m) % 5], T if m else 0, (i + m) & 1))
    return sym, place(jobs)


def frames_case():
    """encoded frames with a few channel errors: every CRC width, held and (one info bit changed behind the CRC's back) failing; 8PSK,
    whose three bits a symbol straddle the steps; a frame too short for its CRC"""
    rng = np.random.default_rng(2525)
    parts, jobs, at = [], [], 0
    for i, crc in enumerate(CRCS):
        for spoil in (False, True):
            for order, (code, punct) in ((8, (K7, P_34)), (4, (K7, P_NONE)), (2, (K5, P_23)), (8, (K7_THIRD, P3_NONE))):
                info = rng.integers(0, 2, 150 + 7 * i)
                bits = with_crc(info, crc)
                if spoil:
                    bits[3] ^= 1
                sym, T = frame(bits, code, punct, order, CRC_NONE, True, flips=(20, 90, 91 + 40 * i), junk=rng)
                parts.append(sym)
                jobs.append(make_job(at, 0, len(sym), order, code, punct, crc, 0 if order != 8 else T, TERMINATED))
                at += len(sym)
    sym, T = frame(rng.integers(0, 2, 10), K3, P_NONE, 4, CRC_NONE, True)
    parts.append(sym)
    jobs.append(make_job(at, 0, len(sym), 4, K3, P_NONE, CRC16, 0, TERMINATED))		# 10 bits, CRC-16: SHORT
    return np.concatenate(parts), place(jobs)


def max_steps_case():
    """one job of MAX_STEPS: K = 7 at rate 1/2, QPSK, CRC-16, TERMINATED, an encoded frame with a coded bit in 50 inverted"""
    rng = np.random.default_rng(2626)
    info = rng.integers(0, 2, MAX_STEPS - 6 - 16)
    flips = rng.choice(2 * MAX_STEPS, 2 * MAX_STEPS // 50, replace=False)
    sym, T = frame(info, K7, P_NONE, 4, CRC16, True, flips=flips)
    assert T == MAX_STEPS
    return sym, place([make_job(0, 0, len(sym), 4, K7, P_NONE, CRC16, 0, TERMINATED)])


FULL_CODES = ((K7, P_34, 4, CRC8), (K5, P_NONE, 2, CRC_NONE), (K7_THIRD, P3_NONE, 8, CRC16))


def full_table_case():
    """MAX_JOBS jobs in shuffled order, three codes, n <= 40, every 11th with n = 0: the deepest search of the prefix"""
    rng = np.random.default_rng(4096)
    sym = rng.integers(0, 256, 300).astype(np.uint8)
    jobs = []
    for i in rng.permutation(MAX_JOBS):
        i = int(i)
        code, punct, order, crc = FULL_CODES[i % 3]
        n = 0 if i % 11 == 0 else 1 + (i // 3) % 40
        jobs.append(make_job(int(rng.integers(0, 260)), 0, n, order, code, punct, crc, 0, (i // 5) & 1))
    return sym, place(jobs)


LIMIT_JOBS = MAX_CALL_STEPS // MAX_STEPS
_LIMIT = []


def call_limit_case():
    """64 jobs of MAX_STEPS, exactly MAX_CALL_STEPS, in shuffled order with place()'s guards; two shapes, so that the model decodes
    the jobs of a shape together: K = 7 at rate 1/2, QPSK, CRC-16, TERMINATED, and K = 5 punctured 3/4, 8PSK, CRC-32, not
    terminated; encoded frames with a coded bit in 50 inverted, as max_steps_case().  Not in cases(): the model takes its time for
    it.  Once a session"""
    if _LIMIT:
        return _LIMIT[0]
    rng = np.random.default_rng(2828)
    parts, jobs, at = [], [], 0
    for i in rng.permutation(LIMIT_JOBS):
        if i & 1:
            code, punct, order, crc, term, n_info = K5, P_34, 8, CRC32, False, MAX_STEPS - 32
        else:
            code, punct, order, crc, term, n_info = K7, P_NONE, 4, CRC16, True, MAX_STEPS - 6 - 16
        n_coded = kept(MAX_STEPS, punct[0], punct[1])
        sym, T = frame(rng.integers(0, 2, n_info), code, punct, order, crc, term, flips=rng.choice(n_coded, n_coded // 50, replace=False))
        assert T == MAX_STEPS
        parts.append(sym)
        jobs.append(make_job(at, 0, len(sym), order, code, punct, crc, T, TERMINATED if term else 0))
        at += len(sym)
    _LIMIT.append((np.concatenate(parts), place(jobs)))
    return _LIMIT[0]


def one_step_more(case):
    """the case with one more job of one step behind its table: a step past MAX_CALL_STEPS"""
    sym, jobs = case
    return sym, place([jobs.copy(), make_job(0, 0, 1, 4, K3, P_NONE, CRC_NONE, 1, 0)])


def cases():
    """name -> (sym, jobs): every set the CPU and GPU tests share"""
    return {"seams": seams_case(), "codes": codes_case(), "frames": frames_case(), "max_steps": max_steps_case(),
            "full_table": full_table_case()}
