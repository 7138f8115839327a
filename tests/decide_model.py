"""numpy statement of rules 1-5 of include/fosphor_amd_decide.h and the input sets the CPU and GPU tests share.

A case is (iq, jobs, uw): iq float32 [n][2] as it lies in memory, one complex sample per symbol, jobs a JOB_DTYPE array whose owned
bytes are placed with GUARD or 2 GUARD bytes before, between and behind them (place()), and uw the call's table of unique-word
symbols, uint8.  The angle is demod_model.atan2_turns and the decided point carrier_model.cossin_turns, the numpy statements of the
two pinned inlines.  Every floating-point operation is one IEEE double operation that numpy rounds once, in the order of the header's
parentheses; the ordered sums are symbols_model.three_level.  The decisions and the terms of rule 2 depend on the symbol and on M
alone, so they are computed once per buffer and M and the jobs cut their ranges out of them.  A NaN double of the record is
0x7ff8000000000000."""
import numpy as np

import carrier_model as cm
import demod_model as dm
from symbols_model import QNAN64, quiet64, three_level		# noqa: F401

JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("n", "<i4"), ("order", "<i4"), ("flags", "<i4"), ("uw_offset", "<i4"),
                      ("uw_len", "<i4"), ("uw_first", "<i4"), ("uw_count", "<i4"), ("uw_max_errors", "<i4"), ("reserved", "<i4", (4,))])
RECORD_DTYPE = np.dtype([("n", "<i4"), ("order", "<i4"), ("flags", "<i4"), ("status", "<i4"), ("uw_pos", "<i4"), ("uw_rot", "<i4"),
                         ("uw_errors", "<i4"), ("erasures", "<i4"), ("a", "<f8"), ("b", "<f8"), ("m2", "<f8"), ("hist", "<i4", (8,)),
                         ("reserved", "<i4", (2,))])
STATS = ("calls", "k_hard", "k_uw", "k_job", "k_out", "jobs_uw", "symbols")
MAX_JOBS, MAX_UW, MAX_UW_TABLE, BLOCK, TILE, UW_GROUP = 4096, 64, 65536, 64, 4096, 256
DIFF, GRAY, UW = 1, 2, 4
FLAGS = {"diff": DIFF, "gray": GRAY, "uw": UW}
OK, NO_UW = 0, 1
STATUS = {"ok": OK, "no_uw": NO_UW}
ORDERS = (2, 4, 8)
RECORD_WORDS = RECORD_DTYPE.itemsize // 4
GUARD = 4						# sentinel bytes before, between (or twice as many) and behind the jobs' owned bytes

psk = cm.psk


def planted(n, order, seed):
    """the indices that carrier_model.psk(n, order, .., seed) draws first"""
    return np.random.default_rng(seed).integers(0, order, n)


def owned(n):
    return 4 * ((int(n) + 3) // 4)


def decisions(y, M):
    """rule 1 over float32 y [n][2] -> (k int64 [n], erased bool [n])"""
    t = dm.atan2_turns(y[:, 1].astype(np.float64), y[:, 0].astype(np.float64))
    erased = np.isnan(t)
    with np.errstate(all="ignore"):
        k = np.floor((np.where(erased, 0.0, t).astype(np.float64) * np.float64(M)) + 0.5).astype(np.int64) & (M - 1)
    return k, erased


def terms(y, k, M):
    """rule 2 -> the terms of a, b and m2, float64 [n][3]"""
    sr, si = y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        c, sn = cm.cossin_turns(k.astype(np.float64) / np.float64(M))
        return np.stack([(sr * c) + (si * sn), (si * c) - (sr * sn), (sr * sr) + (si * si)], 1)


def difference(k, M, flags):
    """rule 3"""
    if not flags & DIFF or len(k) == 0:
        return k.copy()
    return np.concatenate([k[:1], (k[1:] - k[:-1]) & (M - 1)])


def candidates(job):
    """rule 4 -> (the first candidate position, how many)"""
    if not int(job["flags"]) & UW:
        return 0, 0
    last = int(job["n"]) - int(job["uw_len"])
    if int(job["uw_count"]) > 0:
        last = min(last, int(job["uw_first"]) + int(job["uw_count"]) - 1)
    first = max(int(job["uw_first"]), 1 if int(job["flags"]) & DIFF else 0)
    return first, max(last - first + 1, 0)


def find_word(d, u, M, flags, first, count):
    """rule 4 -> (uw_pos, uw_rot, matches) of the winner; count >= 1"""
    win = np.lib.stride_tricks.sliding_window_view(d, len(u))[first:first + count]
    e = (win - u[None, :]) & (M - 1)
    rots = 1 if flags & DIFF else M
    matches = np.stack([(e == r).sum(1) for r in range(rots)], 1)		# [count][rots]
    p, r = np.argwhere(matches == matches.max())[0]				# row-major: the smallest p, then the smallest r
    return first + int(p), int(r), int(matches[p, r])


_PER_BUFFER = {}


def per_buffer(iq, M):
    """(k, erased, terms) of every sample of iq at order M, computed once per buffer"""
    key = (id(iq), M)
    if key not in _PER_BUFFER or _PER_BUFFER[key][0] is not iq:
        k, erased = decisions(iq, M)
        _PER_BUFFER[key] = (iq, k, erased, terms(iq, k, M))
    return _PER_BUFFER[key][1:]


def decide_job(iq, job, uw):
    """-> (a RECORD_DTYPE array [1], the job's owned bytes uint8 [4 ceil(n / 4)], its q before Gray mapping)"""
    n, M, flags = int(job["n"]), int(job["order"]), int(job["flags"])
    at = int(job["offset"])
    k_all, erased_all, terms_all = per_buffer(iq, M)
    k, erased = k_all[at:at + n], erased_all[at:at + n]
    r = np.zeros(1, RECORD_DTYPE)
    r["n"], r["order"], r["flags"], r["uw_pos"] = n, M, flags, -1
    r["erasures"] = int(erased.sum())
    r["hist"][0] = np.bincount(k, minlength=8)
    r["a"], r["b"], r["m2"] = (quiet64(v) for v in three_level(terms_all[at:at + n]))
    d = difference(k, M, flags)
    if flags & UW:
        L = int(job["uw_len"])
        u = np.asarray(uw, np.int64)[int(job["uw_offset"]):int(job["uw_offset"]) + L]
        first, count = candidates(job)
        r["uw_errors"] = L
        if count:
            pos, rot, matches = find_word(d, u, M, flags, first, count)
            r["uw_pos"], r["uw_rot"], r["uw_errors"] = pos, rot, L - matches
        if not count or r["uw_errors"][0] > int(job["uw_max_errors"]):
            r["status"] = NO_UW
    q = (d - int(r["uw_rot"][0])) & (M - 1)
    v = q ^ (q >> 1) if flags & GRAY else q
    out = np.zeros(owned(n), np.uint8)
    out[:n] = v
    return r, out, q


def buffer(case):
    return np.ascontiguousarray(case[0], np.float32).reshape(-1, 2)


def table(case):
    return np.ascontiguousarray(case[2], np.uint8).reshape(-1)


def decide(case):
    """(records RECORD_DTYPE [n_jobs], [the owned bytes per job, uint8])"""
    iq = case[0] if case[0].dtype == np.float32 and case[0].ndim == 2 else buffer(case)
    both = [decide_job(iq, j, case[2]) for j in case[1]]
    return np.concatenate([b[0] for b in both]), [b[1] for b in both]


def capacity(jobs):
    """bytes of the output buffer of a case: the last owned byte and GUARD behind it"""
    return max([int(j["out_offset"]) + owned(j["n"]) for j in jobs] + [0]) + GUARD


_IMAGES = {}


def image(case, fill, key=None):
    """(records, the whole output buffer as the model leaves it: uint8 [capacity], the byte `fill` wherever no job owns it); with a
    key the result is computed once for all the tests of a session"""
    if key is not None and (key, fill) in _IMAGES:
        return _IMAGES[(key, fill)]
    jobs = case[1]
    records, outs = decide(case)
    out = np.full(capacity(jobs), fill, np.uint8)
    for j, v in zip(jobs, outs):
        out[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v
    if key is not None:
        _IMAGES[(key, fill)] = (records, out)
    return records, out


def expected_stats(jobs):
    """the stats delta of one call over jobs"""
    some = bool((jobs["n"] > 0).any())
    return dict(calls=1, k_hard=int(some), k_uw=int(any(candidates(j)[1] for j in jobs)), k_job=1, k_out=int(some),
                jobs_uw=int(((jobs["flags"] & UW) != 0).sum()), symbols=int(jobs["n"].sum()))


# ---- the builders ---------------------------------------------------------------------------------------------------------------

FIELDS = ("offset", "out_offset", "n", "order", "flags", "uw_offset", "uw_len", "uw_first", "uw_count", "uw_max_errors")


def make_jobs(rows):
    """rows of (offset, out_offset, n, order, flags, uw_offset, uw_len, uw_first, uw_count, uw_max_errors); a short row ends in 0s"""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    for j, r in zip(jobs, rows):
        for name, v in zip(FIELDS, r):
            j[name] = v
    return jobs


def place(rows):
    """rows of (offset, n, order, flags[, uw_offset, uw_len, uw_first, uw_count, uw_max_errors]) -> jobs whose owned bytes follow
    each other with GUARD or 2 GUARD bytes between them"""
    out, at = [], GUARD
    for i, row in enumerate(rows):
        out.append((row[0], at) + tuple(row[1:]))
        at += owned(row[1]) + GUARD * (1 + (i & 1))
    return make_jobs(out)


def three_bursts(n, seed, snr_db=30.0, turn=1):
    """a BPSK, a QPSK and an 8PSK burst of n symbols one behind the other, each turned by turn / M turns
    -> (iq, {order: offset of its burst}, {order: its planted indices})"""
    parts = [psk(n, M, 0.0, turn / M + 0.01 / M, seed + i, snr_db) for i, M in enumerate(ORDERS)]
    return np.concatenate(parts), {M: i * n for i, M in enumerate(ORDERS)}, {M: planted(n, M, seed + i) for i, M in enumerate(ORDERS)}


TILE_COUNTS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 5)
ALL_FLAGS = (0, DIFF, GRAY, DIFF | GRAY)


def tiles_case():
    """n of TILE_COUNTS at every order: the four-symbol store with each remainder and both tile seams; the flags without UW take
    turns, and the counts across a tile seam come with DIFF once more"""
    iq, at, _ = three_bursts(2 * 4096 + 9, 20)
    rows = [(at[M] + (i + k) % 4, n, M, ALL_FLAGS[(i + k) % 4]) for k, M in enumerate(ORDERS) for i, n in enumerate(TILE_COUNTS)]
    rows += [(at[M] + k, n, M, DIFF | (GRAY if k else 0)) for k, M in enumerate(ORDERS) for n in (4097, 2 * 4096 + 5)]
    return iq, place(rows), np.zeros(0, np.uint8)


def offsets_case():
    """input offsets 0 .. 3 at every order and a few symbol counts; the last job ends on the buffer's last sample"""
    iq, at, _ = three_bursts(700, 10)
    rows, i = [], 0
    for M in ORDERS:
        for n in (37, 300, 301, 600):
            for off in range(4):
                rows.append((at[M] + off, n + (i % 3), M, ALL_FLAGS[i % 4]))
                i += 1
    rows.append((len(iq) - 499, 499, 8, DIFF))
    return iq, place(rows), np.zeros(0, np.uint8)


def word_of(idx, M, flags, p, L):
    """the L symbols that rule 4 finds at position p of a burst with the planted indices idx: the indices, or their differences"""
    d = difference(np.asarray(idx, np.int64), M, flags)
    return d[p:p + L].astype(np.uint8)


def windows_case():
    """the windows of rule 4, over bursts turned by 1 / M turns (uw_rot = 1 without DIFF); the words are cut from the planted
    indices, so every one is found without an error unless the row says otherwise:
      a window that starts at 0, and at 1 under DIFF (uw_first = 0 there too);
      one that ends on the last position that fits (uw_count = 0 and a count that ends there);
      words at 250, 255 and 256 of a window over all of 700 symbols: the 256-position seam of k_dec_uw;
      a word at 4080 and one at 4096 of a window from 4000 on, 200 positions: the tile seam of the decisions;
      uw_len 1, 63 and 64; a window of one position;
      no candidate: a window behind the last position that fits, a job shorter than its word, n = 0, n = 1 under DIFF with a
      word of one symbol (NO_UW);
      uw_max_errors exceeded: a word that is not in the burst, 0 errors allowed, and a word with 3 symbols changed, 2 allowed"""
    n = 4500
    iq, at, idx = three_bursts(n, 60)
    words, rows = [], []

    def add(M, flags, p, L, first, count, max_errors=0, n_job=n, off=0, spoil=0, cut=True):
        w = word_of(idx[M][off:off + n_job], M, flags, p, L) if cut else (np.arange(L) * 3 % M).astype(np.uint8)
        w = np.concatenate([w, np.zeros(L - len(w), np.uint8)])				# a job shorter than its word
        for s in range(spoil):
            w[5 * s] = (w[5 * s] + 1) % M
        rows.append((at[M] + off, n_job, M, flags | UW, sum(len(x) for x in words), L, first, count, max_errors))
        words.append(w)

    for k, M in enumerate(ORDERS):
        for flags in (0, DIFF, GRAY, DIFF | GRAY):
            start = 1 if flags & DIFF else 0
            add(M, flags, start, 32, 0, 1 + start)						# starts at 0 (1 under DIFF)
            add(M, flags, 700 - 32, 32, 0, 0, n_job=700, off=k + 1)				# ends on the last position, to the end
            add(M, flags, 700 - 32, 32, 600, 700 - 32 - 600 + 1, n_job=700, off=k)		# ... by a count that ends there
            add(M, flags, 700 - 32, 32, 600, 1000, n_job=700, off=k)				# ... by a count that ends behind it
        for p in (250, 255, 256):
            add(M, (0, DIFF, GRAY)[k], p, 40, 0, 0, n_job=700)
        add(M, DIFF | GRAY, 4080, 32, 4000, 200)
        add(M, 0, 4096, 32, 4000, 200)
        add(M, DIFF, 4095, 64, 3900, 0)
        for L in (1, 63, 64):
            add(M, (DIFF, 0, DIFF | GRAY)[k], 300, L, 200, 300, n_job=900, off=3)
        add(M, 0, 77, 16, 77, 1, n_job=300)							# a window of one position
        add(M, DIFF, 0, 32, 700 - 31, 0, n_job=700)						# no candidate: behind the last that fits
        add(M, 0, 0, 20, 0, 0, n_job=19)							# ... shorter than its word
        add(M, GRAY, 0, 1, 0, 0, n_job=0)							# ... no symbol
        add(M, DIFF, 0, 1, 0, 0, n_job=1)							# ... d[0] is no difference
        add(M, 0, 0, 48, 0, 0, n_job=600, cut=False)						# a word that is not there
        add(M, DIFF, 100, 48, 0, 0, max_errors=2, n_job=600, spoil=3)				# 3 errors, 2 allowed
        add(M, DIFF, 100, 48, 0, 0, max_errors=3, n_job=600, spoil=3)				# 3 errors, 3 allowed
    return iq, place(rows), np.concatenate(words)


def numbers_case():
    """all-zero symbols (k = 0, no erasure); NaN symbols (erasures) and an inf symbol; subnormals; symbols of 3e38, whose m2
    overflows a float but not a double; with and without a word"""
    zeros = np.zeros((300, 2), np.float32)
    sick = psk(1000, 4, 0.0, 0.26, 50, 30.0)
    sick[400, 1] = np.nan
    sick[401] = np.nan
    sick[650, 0] = np.nan
    sick[800, 0] = np.inf
    sick[801] = (-np.inf, np.inf)
    tiny = (psk(300, 4, 0.0, 0.26, 51, 30.0).astype(np.float64) * 1e-41).astype(np.float32)
    huge = psk(300, 4, 0.0, 0.26, 52, 30.0) * np.float32(3e38)
    parts = [zeros, sick, tiny, huge]
    starts = np.cumsum([0] + [len(p) for p in parts])
    word = word_of(planted(1000, 4, 50), 4, 0, 380, 40)				# lies over the NaN symbols
    rows = []
    for flags in ALL_FLAGS:
        rows += [(starts[0] + 1, 299, 4, flags), (starts[0], 300, 8, flags | UW, 0, 8, 0, 0, 8),
                 (starts[1], 1000, 4, flags | UW, 0, 40, 0, 0, 4), (starts[1] + 399, 5, 4, flags), (starts[1] + 1, 999, 8, flags),
                 (starts[1] + 2, 998, 2, flags), (starts[1] + 799, 4, 4, flags)]
        for M in ORDERS:
            rows += [(starts[2] + 1, 299, M, flags), (starts[3], 300, M, flags)]
    return np.concatenate(parts), place([tuple(int(v) for v in r) for r in rows]), word


def mixed_case(count=41, seed=77, with_uw=True):
    """one call with every flag and order, jobs with and without a word and without a symbol in between; the input ranges overlap"""
    rng = np.random.default_rng(seed)
    iq, at, idx = three_bursts(3000, seed + 1, 25.0, turn=3)
    rows, words = [], []
    for i in range(count):
        M = ORDERS[i % 3]
        flags = ALL_FLAGS[(i // 2) % 4]
        n = int(rng.integers(0, 3)) if i % 7 == 3 else int(rng.integers(3, 2900))
        off = int(rng.integers(0, 3000 - n + 1))
        if with_uw and i % 2 == 0 and n > 80:
            L = int(rng.integers(1, MAX_UW + 1))
            p = int(rng.integers(1, n - L + 1))
            rows.append((at[M] + off, n, M, flags | UW, sum(len(x) for x in words), L, int(rng.integers(0, p + 1)), 0, int(rng.integers(0, 3))))
            words.append(word_of(idx[M][off:off + n], M, flags, p, L))
        else:
            rows.append((at[M] + off, n, M, flags))
    return iq, place(rows), np.concatenate(words) if words else np.zeros(0, np.uint8)


def full_table_case():
    """MAX_JOBS jobs in shuffled order, the orders and flags mixed, every third with a word, n <= 130, every 11th with n = 0: the
    deepest search of both prefixes"""
    rng = np.random.default_rng(4096)
    iq, at, idx = three_bursts(1500, 90, 25.0, turn=1)
    uw = np.concatenate([word_of(idx[M], M, f, 40, 24) for M in ORDERS for f in (0, DIFF)])
    rows = []
    for i in rng.permutation(MAX_JOBS):
        i = int(i)
        M, flags = ORDERS[i % 3], ALL_FLAGS[(i // 3) % 4]
        n = 0 if i % 11 == 0 else 1 + (i // 4) % 130
        off = int(rng.integers(0, 100))
        if i % 3 == 0:
            rows.append((at[M] + off, n, M, flags | UW, 24 * (2 * ORDERS.index(M) + (flags & DIFF)), 24, i % 5, (i // 5) % 3 * 20, i % 4))
        else:
            rows.append((at[M] + off, n, M, flags))
    return iq, place(rows), uw


def cases():
    """name -> (iq, jobs, uw): every set the CPU and GPU tests share"""
    return {"tiles": tiles_case(), "offsets": offsets_case(), "windows": windows_case(), "numbers": numbers_case(),
            "mixed": mixed_case(), "without_word": mixed_case(seed=78, with_uw=False), "full_table": full_table_case()}
