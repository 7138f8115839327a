"""numpy / Python statement of rules 1 - 6 of include/fosphor_amd_rs.h, and the input sets the CPU and GPU tests share.

Independent of the library's route: the field is a pair of log / antilog tables (the library multiplies by shift and XOR), the
linear complexity L and the connection polynomial come from the Newton identities S_j = Lambda_1 S_(j-1) + ... + Lambda_L S_(j-L)
solved by Gaussian elimination over GF(2^8) for L = 1 upwards (the library runs Berlekamp-Massey), the uniqueness of Lambda is
checked through the rank, and the error values are the solution of the Vandermonde system S_j = sum Y X^(fcr + j) by elimination
(the library uses Forney's formula).  The encoder divides by g(x) as a polynomial."""
import functools

import numpy as np

MAX_JOBS, MAX_ROOTS, MAX_DEPTH, MAX_CALL_CODEWORDS = 4096, 32, 16, 65536
IN, OUT = 1, 2
FLAGS = {"descramble_in": IN, "descramble_out": OUT}
OK, FAIL, FAILED = 0, 1, 255
STATUS = {"ok": OK, "fail": FAIL}
STATS = ("calls", "k_syn", "k_fix", "k_out", "k_rec", "codewords", "clean", "failed")
GUARD = 16
JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("flags", "<i4"), ("gf_poly", "<u2"), ("fcr", "u1"),
                      ("prim", "u1"), ("n_roots", "u1"), ("n_code", "u1"), ("depth", "u1"), ("scr_width", "u1"),
                      ("scr_taps", "<u4"), ("scr_init", "<u4"), ("reserved", "<u4", (7,))])
RECORD_DTYPE = np.dtype([("n_codewords", "<i4"), ("n_data", "<i4"), ("status", "<i4"), ("n_failed", "<i4"),
                         ("n_clean", "<i4"), ("corrected_symbols", "<i4"), ("corrected_bits", "<i4"), ("max_errors", "<i4"),
                         ("failed_mask", "<u4"), ("errors", "u1", (16,)), ("n_code", "<u2"), ("n_roots", "<u2"),
                         ("reserved", "<u4", (2,))])
RECORD_WORDS = RECORD_DTYPE.itemsize // 4

# (gf_poly, fcr, prim, n_roots)
CCSDS = (0x187, 112, 11, 32)
DVB = (0x11d, 0, 1, 16)
QR10 = (0x11d, 0, 1, 10)
# (scr_width, scr_taps, scr_init)
NO_SCR = (0, 0, 0)
CCSDS_SCR = (8, 0x95, 0xff)			# ff 48 0e c0 9a 0d 70 bc ...
DVB_SCR = (15, 0x6000, 0x4a80)			# 1 + x^14 + x^15 from 100101010000000
WIDE_SCR = (32, 0x80200003, 0xdeadbeef)


# ---- the field -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def field(poly):
    """(exp [510], log [256]) of GF(2^8) modulo poly, alpha = 2"""
    exp, log = np.zeros(510, np.int64), np.zeros(256, np.int64)
    x = 1
    for i in range(255):
        exp[i], log[x] = x, i
        x <<= 1
        if x & 0x100:
            x ^= poly
    assert x == 1 and len(set(exp[:255])) == 255, "not primitive"
    exp[255:] = exp[:255]
    return exp, log


def primitive(poly):
    x = 1
    for i in range(1, 256):
        x <<= 1
        if x & 0x100:
            x ^= poly
        if x == 1:
            return i == 255
    return False


def mul(a, b, poly):
    exp, log = field(poly)
    return int(exp[log[a] + log[b]]) if a and b else 0


def inv(a, poly):
    exp, log = field(poly)
    return int(exp[(255 - log[a]) % 255])


def alpha(e, poly):
    return int(field(poly)[0][e % 255])


def poly_eval(coefs_low_first, x, poly):
    v = 0
    for c in reversed(coefs_low_first):
        v = mul(v, x, poly) ^ int(c)
    return v


def solve(rows, rhs, poly):
    """Gaussian elimination over the field: rows [m][n], rhs [m] -> (rank, consistent, a solution with the free unknowns 0)"""
    m, n = len(rows), len(rows[0]) if rows else 0
    a = [list(map(int, r)) + [int(b)] for r, b in zip(rows, rhs)]
    pivots, row = [], 0
    for col in range(n):
        at = next((i for i in range(row, m) if a[i][col]), None)
        if at is None:
            continue
        a[row], a[at] = a[at], a[row]
        scale = inv(a[row][col], poly)
        a[row] = [mul(v, scale, poly) for v in a[row]]
        for i in range(m):
            if i != row and a[i][col]:
                f = a[i][col]
                a[i] = [v ^ mul(f, w, poly) for v, w in zip(a[i], a[row])]
        pivots.append(col)
        row += 1
    consistent = all(not r[n] for r in a[row:])
    x = [0] * n
    for i, col in enumerate(pivots):
        x[col] = a[i][n]
    return row, consistent, x


# ---- rules 1 - 3 -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def scramble(w, taps, init, n):
    """rule 1: n bytes of the sequence"""
    reg, mask, out = init, (1 << w) - 1, np.zeros(n, np.uint8)
    for p in range(n):
        byte = 0
        for i in range(8):
            byte = (byte << 1) | ((reg >> (w - 1)) & 1)
            reg = ((reg << 1) | (bin(reg & taps).count("1") & 1)) & mask
        out[p] = byte
    return out


def root_exps(code):
    poly, fcr, prim, n_roots = code
    return [(prim * (fcr + j)) % 255 for j in range(n_roots)]


@functools.lru_cache(None)
def generator(code):
    """rule 3: g(x), highest coefficient first"""
    poly = code[0]
    g = [1]
    for e in root_exps(code):
        r = alpha(e, poly)
        g = [a ^ mul(b, r, poly) for a, b in zip(g + [0], [0] + g)]
    return g


def parity(data, code):
    """the remainder of data(x) x^n_roots by g(x), highest coefficient first: the n_roots parity bytes"""
    poly, n_roots, g = code[0], code[3], generator(code)
    rem = [int(v) for v in data] + [0] * n_roots
    for i in range(len(data)):
        f = rem[i]
        if f:
            for k in range(1, n_roots + 1):
                rem[i + k] ^= mul(f, g[k], poly)
    return rem[len(data):]


def syndromes(r, code):
    poly = code[0]
    exp, log = field(poly)
    r = np.asarray(r, np.int64)
    n = len(r)
    nz = np.flatnonzero(r)
    out = []
    for e in root_exps(code):
        terms = exp[(log[r[nz]] + e * (n - 1 - nz)) % 255] if len(nz) else np.zeros(0, np.int64)
        out.append(int(np.bitwise_xor.reduce(terms)) if len(terms) else 0)
    return out


def decide(r, code):
    """rule 4 over one codeword -> (errors or FAILED, [(position, value)])"""
    poly, fcr, prim, n_roots = code
    n, t = len(r), n_roots // 2
    S = syndromes(r, code)
    if not any(S):
        return 0, []
    lam = None
    for L in range(1, t + 1):				# the shortest recurrence that holds for all L <= j < n_roots
        rows = [[S[j - k] for k in range(1, L + 1)] for j in range(L, n_roots)]
        rank, consistent, x = solve(rows, [S[j] for j in range(L, n_roots)], poly)
        if consistent:
            assert rank == L, "2 L <= n_roots: Lambda is unique"
            lam = [1] + x
            break
    if lam is None:
        return FAILED, []
    L = len(lam) - 1
    found = []
    for i in range(n):
        e = (prim * (n - 1 - i)) % 255
        if poly_eval(lam, alpha(-e, poly), poly) == 0:
            found.append((i, alpha(e, poly)))
    if len(found) != L:
        return FAILED, []
    exp, log = field(poly)
    rows = [[int(exp[(log[X] * (fcr + j)) % 255]) for _, X in found] for j in range(L)]
    rank, consistent, Y = solve(rows, S[:L], poly)
    assert rank == L and consistent and all(Y)
    return L, [(i, y) for (i, _), y in zip(found, Y)]


def code_of(j):
    return int(j["gf_poly"]), int(j["fcr"]), int(j["prim"]), int(j["n_roots"])


def scr_of(j):
    return int(j["scr_width"]), int(j["scr_taps"]), int(j["scr_init"])


def n_data_of(j):
    return int(j["depth"]) * (int(j["n_code"]) - int(j["n_roots"]))


def owned(n_data):
    return 8 * ((int(n_data) + 7) // 8)


def job_owned(j):
    return owned(n_data_of(j))


def decode_job(buf, j):
    """rules 1 - 6 over one job -> (record, data bytes)"""
    I, n, flags = int(j["depth"]), int(j["n_code"]), int(j["flags"])
    code = code_of(j)
    frame = np.array(buf[int(j["offset"]):int(j["offset"]) + I * n], np.uint8)
    seq = scramble(*scr_of(j), I * n) if flags else None
    if flags & IN:
        frame ^= seq
    r = np.zeros(1, RECORD_DTYPE)[0]
    r["n_codewords"], r["n_data"], r["n_code"], r["n_roots"] = I, n_data_of(j), n, code[3]
    for c in range(I):
        count, fixes = decide(frame[c::I], code)
        r["errors"][c] = count
        if count == FAILED:
            r["n_failed"] += 1
            r["failed_mask"] |= 1 << c
            continue
        r["n_clean"] += count == 0
        r["corrected_symbols"] += count
        r["max_errors"] = max(r["max_errors"], count)
        for i, y in fixes:
            r["corrected_bits"] += bin(y).count("1")
            frame[i * I + c] ^= y
    r["status"] = FAIL if r["n_failed"] else OK
    data = frame[:n_data_of(j)].copy()
    if flags & OUT:
        data ^= seq[:len(data)]
    return r, data


def decode(case):
    """-> (records, [data bytes per job])"""
    buf, jobs = case
    got = [decode_job(buf, j) for j in jobs]
    return np.array([g[0] for g in got], RECORD_DTYPE), [g[1] for g in got]


def encode_frame(data, j):
    """the way back: data bytes in the order of rule 5 -> the frame"""
    I, n, flags = int(j["depth"]), int(j["n_code"]), int(j["flags"])
    code = code_of(j)
    k = n - code[3]
    data = np.array(data, np.uint8)
    assert len(data) == I * k
    seq = scramble(*scr_of(j), I * n) if flags else None
    if flags & OUT:
        data = data ^ seq[:len(data)]
    frame = np.zeros(I * n, np.uint8)
    frame[:I * k] = data
    for c in range(I):
        frame[I * k + c::I] = parity(data[c::I], code)
    if flags & IN:
        frame ^= seq
    return frame


def capacity(jobs):
    return max([int(j["out_offset"]) + job_owned(j) for j in jobs] + [0]) + GUARD


_IMAGES = {}


def image(case, sentinel, key=None):
    """(records, the whole output buffer: the owned bytes as rule 5 writes them, `sentinel` everywhere else); cached under key"""
    if key is not None and key in _IMAGES:
        return _IMAGES[key]
    buf, jobs = case
    records, datas = decode(case)
    out = np.full(capacity(jobs), sentinel, np.uint8)
    for j, d in zip(jobs, datas):
        at = int(j["out_offset"])
        out[at:at + job_owned(j)] = 0
        out[at:at + len(d)] = d
    if key is not None:
        _IMAGES[key] = (records, out)
    return records, out


def expected_stats(records):
    cw, clean, failed = int(records["n_codewords"].sum()), int(records["n_clean"].sum()), int(records["n_failed"].sum())
    return dict(calls=1, k_syn=1, k_fix=int(clean != cw), k_out=1, k_rec=1, codewords=cw, clean=clean, failed=failed)


# ---- the jobs and the named cases ---------------------------------------------------------------------------------------------------

def make_job(offset, out_offset, n_code, depth, code, scr=NO_SCR, flags=0):
    j = np.zeros(1, JOB_DTYPE)
    j["offset"], j["out_offset"], j["flags"], j["n_code"], j["depth"] = offset, out_offset, flags, n_code, depth
    j["gf_poly"], j["fcr"], j["prim"], j["n_roots"] = code
    j["scr_width"], j["scr_taps"], j["scr_init"] = scr
    return j


def place(jobs, gap=GUARD):
    """the jobs' owned bytes one behind the other, GUARD bytes before, between and behind them"""
    jobs = np.concatenate(jobs) if isinstance(jobs, (list, tuple)) else jobs.copy()
    at = GUARD
    for j in jobs:
        j["out_offset"] = at
        at += job_owned(j) + gap
    return jobs


def plant(rng, frame_clean, j, mode):
    """channel errors on the clean, scrambled frame of job j -> (frame, errors per codeword).  mode: per codeword (cycled) a
    count, "t", "t+1", "t+2", "all", "first", "last", "parity", "ff" """
    I, n, n_roots = int(j["depth"]), int(j["n_code"]), int(j["n_roots"])
    t = n_roots // 2
    frame = frame_clean.copy()
    counts = []
    for c in range(I):
        what = mode[c % len(mode)]
        if what == "all":
            pos, val = np.arange(n), rng.integers(1, 256, n)
        elif what in ("first", "last", "ff"):
            pos = np.array([0 if what == "first" else (n - 1 if what == "last" else int(rng.integers(0, n)))])
            val = np.array([0xff if what == "ff" else int(rng.integers(1, 256))])
        elif what == "parity":
            pos = n - n_roots + rng.choice(n_roots, min(t, n_roots), replace=False)
            val = rng.integers(1, 256, len(pos))
        else:
            count = {"t": t, "t+1": t + 1, "t+2": t + 2}.get(what, what)
            count = min(int(count), n)
            pos, val = rng.choice(n, count, replace=False), rng.integers(1, 256, count)
        frame[pos * I + c] ^= val.astype(np.uint8)
        counts.append(len(pos))
    return frame, counts


PLANTED = {}			# case name -> per job (data bytes, errors planted per codeword)


def build(name, specs, seed, tail=0, shuffle=False):
    """specs: (n_code, depth, code, scr, flags, mode, offset mod 8) per job -> (input buffer, jobs); the jobs' frames lie one behind
    the other with gaps that give each its offset mod 8; `tail` bytes of noise behind the last"""
    rng = np.random.default_rng(seed)
    parts, jobs, planted, at = [], [], [], 0
    for n_code, depth, code, scr, flags, mode, mod in specs:
        pad = (mod - at) % 8
        parts.append(rng.integers(0, 256, pad).astype(np.uint8))
        at += pad
        j = make_job(at, 0, n_code, depth, code, scr, flags)
        data = rng.integers(0, 256, n_data_of(j[0])).astype(np.uint8)
        frame, counts = plant(rng, encode_frame(data, j[0]), j[0], mode)
        parts.append(frame)
        at += len(frame)
        jobs.append(j)
        planted.append((data, counts))
    parts.append(rng.integers(0, 256, tail).astype(np.uint8))
    jobs = place(jobs)
    if shuffle:
        order = rng.permutation(len(jobs))
        places = jobs["out_offset"].copy()
        jobs, planted = jobs[order], [planted[i] for i in order]
        jobs["out_offset"] = places[order]
    PLANTED[name] = planted
    return np.concatenate(parts), jobs


SEAM_CODES = (9, 63, 64, 65, 127, 128, 129, 254, 255)		# 9 stands for n_roots + 1
SEAM_ROOTS = (2, 3, 4, 10, 16, 31, 32)
SEAM_DEPTHS = (1, 2, 3, 5, 8, 16)
SEAM_MODES = (0, 1, "t", "t+1", "all", "first", "last", "parity", "ff")
FIELDS = ((0x11d, 0, 1), (0x187, 112, 11), (0x11d, 1, 1), (0x12b, 254, 7))
TURNS = ((NO_SCR, 0), (CCSDS_SCR, IN), (DVB_SCR, OUT), (WIDE_SCR, IN), (CCSDS_SCR, OUT), (DVB_SCR, 0))


def seam_specs():
    specs, i = [], 0
    for n_roots in SEAM_ROOTS:
        for n_code in SEAM_CODES:
            field3 = FIELDS[i % len(FIELDS)]
            scr, flags = TURNS[i % len(TURNS)]
            depth = SEAM_DEPTHS[(i + i // len(SEAM_DEPTHS)) % len(SEAM_DEPTHS)]
            mode = tuple(SEAM_MODES[(i + c) % len(SEAM_MODES)] for c in range(len(SEAM_MODES)))
            specs.append((n_roots + 1 if n_code == 9 else n_code, depth, field3 + (n_roots,), scr, flags, mode, i % 8))
            i += 1
    return specs


def over_t_specs():
    specs = []
    for n_roots, n_code in ((2, 20), (2, 255), (4, 24), (4, 200), (32, 255), (32, 80)):
        for extra in ("t+1", "t+2"):
            specs.append((n_code, 8, (0x11d, 1, 1, n_roots), NO_SCR, 0, (extra, "t", extra, extra, 1, extra, extra, 0), len(specs) % 8))
    return specs


def small_specs(count, seed):
    rng = np.random.default_rng(seed)
    specs = []
    for i in range(count):
        n_roots = int(rng.integers(2, 5))
        scr, flags = TURNS[int(rng.integers(0, len(TURNS)))]
        mode = (0,) if i % 11 == 0 else tuple(int(v) for v in rng.integers(0, n_roots // 2 + 2, 2))
        specs.append((int(rng.integers(n_roots + 1, 16)), int(rng.integers(1, 3)), FIELDS[i % 2] + (n_roots,), scr, flags, mode, i % 8))
    return specs


@functools.lru_cache(None)
def cases():
    t = 16
    return {
        "seams": build("seams", seam_specs(), 1),
        "over_t": build("over_t", over_t_specs(), 2, tail=5),
        "ccsds": build("ccsds", [(255, 5, CCSDS, CCSDS_SCR, IN, mode, 3) for mode in ((0,), (2, 3, 0, 1, 4), (t,), (t, t + 1, 1, 0, t))], 3),
        "dvb": build("dvb", [(204, 1, DVB, DVB_SCR, OUT, (m,), i) for i, m in enumerate((0, 1, 8, 9, "parity", "ff", 2, "all"))], 4),
        "full_table": build("full_table", small_specs(MAX_JOBS, 5), 5, shuffle=True),
        "all_clean": build("all_clean", [(255, 5, CCSDS, CCSDS_SCR, IN, (0,), 1), (204, 1, DVB, DVB_SCR, OUT, (0,), 0),
                                         (12, 3, (0x11d, 0, 1, 4), NO_SCR, 0, (0,), 5)], 6),
    }


def call_limit_case():
    """MAX_JOBS frames of MAX_DEPTH codewords of (4, 2) over one shared input: exactly MAX_CALL_CODEWORDS"""
    rng = np.random.default_rng(7)
    j = make_job(0, 0, 4, MAX_DEPTH, (0x11d, 0, 1, 2))
    data = rng.integers(0, 256, n_data_of(j[0])).astype(np.uint8)
    frame = encode_frame(data, j[0])
    frame[5] ^= 0x40					# one error in codeword 5
    jobs = place([j] * MAX_JOBS, gap=0)
    return frame, jobs, data
