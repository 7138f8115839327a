"""numpy statement of rules 1-2 of include/fosphor_amd_resample.h and the input sets the CPU and GPU tests share.

A case is (iq, taps, jobs): iq float32 [n][2] and taps float32 [n_taps_total] as they lie in memory, and jobs a JOB_DTYPE array
whose outputs are placed with GUARD complex samples before, between and behind them (place()).  The sums are vectorised over the
outputs with a Python loop over the branch index q, ascending: that is the pinned order.  Every operation is one IEEE double
operation that numpy rounds once (a product, then an addition); the products are exact, so the device's fused multiply-adds and
fosphor_amd_resample_host's a * b + s give the same bits.  A NaN float is 0x7fc00000 (rule 2)."""
import numpy as np

from measure_model import EXTRACT_DTYPE

JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("phase0", "<i8"), ("n", "<i4"), ("n_out", "<i4"), ("up", "<i4"),
                      ("down", "<i4"), ("taps_offset", "<i4"), ("n_taps", "<i4")])
STATS = ("calls", "k_tile", "k_direct", "jobs_tile", "jobs_direct", "outputs", "macs")
MAX_JOBS, MAX_UP, MAX_DOWN, MAX_BRANCH = 4096, 256, 256, 64
TILE, TILE_LDS, DIRECT_OUT = 512, 40960, 256		# FOSPHOR_AMD_RESAMPLE_TILE, _TILE_LDS, _DIRECT_OUT
GUARD = 3						# sentinel complex samples before, between and behind the jobs' outputs
MAX_MACS = 2 ** 23
QNAN = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]


def quiet(v):
    v = np.array(v, np.float32)
    v[np.isnan(v)] = QNAN
    return v


def form(up, down, n_taps):
    """rule 4: "tile" or "direct" from (U, D, T) alone, as the header's #defines say it"""
    span = ((TILE - 1) * down + up - 1) // up + n_taps // up
    return "tile" if 8 * (span + 1) + 4 * ((n_taps + 3) & ~3) <= TILE_LDS else "direct"


def max_n_out(n, up, down, n_taps, phase0=0):
    """rule 1: the largest valid n_out"""
    q = n_taps // up
    if n < q or phase0 > (n - q) * up:
        return 0
    return ((n - q) * up - phase0) // down + 1


def need(up, down, q, phase0, n_out):
    """the fewest input samples with which n_out outputs are valid"""
    if n_out == 0:
        return 0
    return q + -(-(phase0 + (n_out - 1) * down) // up)


def resample_job(iq, taps, job):
    """rules 1 and 2 for one job -> float32 [n_out][2]"""
    U, D, T = int(job["up"]), int(job["down"]), int(job["n_taps"])
    Q, n_out = T // U, int(job["n_out"])
    x = np.asarray(iq, np.float32).reshape(-1, 2)[int(job["offset"]):int(job["offset"]) + int(job["n"])]
    h = np.asarray(taps, np.float32)[int(job["taps_offset"]):int(job["taps_offset"]) + T].astype(np.float64)
    xr, xi = x[:, 0].astype(np.float64), x[:, 1].astype(np.float64)
    p = int(job["phase0"]) + np.arange(n_out, dtype=np.int64) * D
    b = -((-p) // U)
    s = b * U - p
    assert n_out == 0 or (s.min() >= 0 and s.max() < U and b.max() + Q <= len(x)), "the job is not valid"
    re, im = np.zeros(n_out), np.zeros(n_out)
    with np.errstate(all="ignore"):
        for q in range(Q):
            hq = h[s + q * U]
            re = re + hq * xr[b + q]
            im = im + hq * xi[b + q]
        return quiet(np.stack([re, im], 1).astype(np.float32))


def resample(case):
    """[float32 [n_out][2] per job]"""
    iq, taps, jobs = case
    return [resample_job(iq, taps, j) for j in jobs]


def macs(jobs):
    return sum(int(j["n_out"]) * (int(j["n_taps"]) // int(j["up"])) for j in jobs)


def capacity(jobs):
    """complex samples of the output buffer of a case: the last output and GUARD behind it"""
    return max([int(j["out_offset"]) + int(j["n_out"]) for j in jobs] + [0]) + GUARD


def image(case, fill):
    """the whole output buffer as the model leaves it: uint32 [2 * capacity], `fill` wherever no job writes"""
    jobs = case[2]
    out = np.full(2 * capacity(jobs), fill, np.uint32)
    for j, v in zip(jobs, resample(case)):
        out[2 * int(j["out_offset"]):2 * (int(j["out_offset"]) + len(v))] = v.reshape(-1).view(np.uint32)
    return out


def outputs_of(buf, job):
    """the floats of a job in a whole output buffer (uint32 or float32 [2 * capacity])"""
    return buf[2 * int(job["out_offset"]):2 * (int(job["out_offset"]) + int(job["n_out"]))]


def expected_stats(jobs):
    """the stats delta of one call"""
    forms = [form(int(j["up"]), int(j["down"]), int(j["n_taps"])) for j in jobs]
    live = {f for f, j in zip(forms, jobs) if j["n_out"] > 0}
    return dict(calls=1, k_tile=int("tile" in live), k_direct=int("direct" in live), jobs_tile=forms.count("tile"),
                jobs_direct=forms.count("direct"), outputs=int(jobs["n_out"].astype(np.int64).sum()), macs=macs(jobs))


# ---- the builders ---------------------------------------------------------------------------------------------------------------

FIELDS = ("offset", "out_offset", "phase0", "n", "n_out", "up", "down", "taps_offset", "n_taps")


def make_jobs(rows):
    """rows of (offset, out_offset, phase0, n, n_out, up, down, taps_offset, n_taps)"""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    for j, r in zip(jobs, rows):
        for k, v in zip(FIELDS, r):
            j[k] = v
    return jobs


def place(rows):
    """rows of (offset, phase0, n, n_out, up, down, taps_offset, n_taps) -> jobs whose outputs follow each other with GUARD or
    GUARD + 1 samples between them, so that odd and even out_offsets both occur whatever the lengths are"""
    out, at = [], GUARD
    for i, (off, ph, n, n_out, up, down, toff, T) in enumerate(rows):
        out.append((off, at, ph, n, n_out, up, down, toff, T))
        at += n_out + GUARD + (i & 1)
    return make_jobs(out)


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * np.exp(rng.uniform(-1.0, 1.0, (n, 1)))).astype(np.float32)


def some_taps(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


RATIOS = ((1, 1), (1, 4), (4, 1), (3, 2), (2, 3), (7, 5), (256, 1), (1, 256), (255, 256))
QS = (1, 2, 63, 64)
COUNTS = (0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


def ratios_case():
    """every (U, D) of RATIOS with every Q of QS; the output counts walk COUNTS, offset and taps_offset 0 .. 3 in both parities
    against each other, phase0 walks 0 (branch 0 at output 0), 1 and U + 3 (a later branch; with U = 1 there is one branch only)"""
    rows, i = [], 0
    for U, D in RATIOS:
        for Q in QS:
            n_out, ph = COUNTS[(i + i // 9) % 9], (0, 1, U + 3)[i % 3]
            rows.append((i % 4, ph, need(U, D, Q, ph, n_out) + (i % 2), n_out, U, D, (i // 4 + i) % 4, Q * U))
            i += 1
    total = max(r[0] + r[2] for r in rows)
    return noise(total, 10), some_taps(MAX_BRANCH * MAX_UP + 3, 11), place(rows)


COUNT_FORMS = ((3, 2, 4), (1, 16, 5))			# (U, D, Q): a TILE and a DIRECT form


def counts_case():
    """every n_out of COUNTS in both forms; phase0 = 0, 1, 2 in turn; the longest job of each form ends on the buffer's last
    sample; a job with phase0 = (n - Q) U exactly: one output, from the last Q samples"""
    total = need(1, 16, 5, 2, COUNTS[-1]) + 3
    rows, i = [], 0
    for U, D, Q in COUNT_FORMS:
        for n_out in COUNTS:
            ph = i % 3
            n = need(U, D, Q, ph, n_out)
            rows.append((total - n if n_out == COUNTS[-1] else i % 4, ph, n, n_out, U, D, (i + 1) % 4, Q * U))
            i += 1
        rows.append((5, (100 - Q) * U, 100, 1, U, D, 0, Q * U))
    return noise(total, 20), some_taps(64, 21), place(rows)


def seam_of(up, down=None, q=None):
    """the largest D (q given) or Q (down given) at which (up, ., .) is still in the TILE form; the next one is DIRECT"""
    if down is None:
        return max(d for d in range(1, MAX_DOWN) if form(up, d, q * up) == "tile")
    return max(k for k in range(1, MAX_BRANCH) if form(up, down, k * up) == "tile")


SEAM_PHASE0 = 77


def seam_case():
    """jobs just on either side of the TILE / DIRECT seam, computed from the header's macros: through D (U = 1, Q = 8), through T
    (U = 256, D = 1 and U = 255, D = 256).  The first two jobs are the SAME job in both forms: (U, D, phase0) = (256, 1, 77) and one
    prototype of Q taps a branch, once as it is (TILE) and once with a (Q + 1)-th tap of 0.0 behind every branch (DIRECT); a
    product with that tap adds +0 or -0 to a sum that is never -0, so the outputs are the same bits."""
    d_tile = seam_of(1, q=8)
    q_tile, q2_tile = seam_of(256, down=1), seam_of(255, down=256)
    h = some_taps(q_tile * 256, 31)
    taps = np.concatenate([h, h, np.zeros(256, np.float32), some_taps(MAX_BRANCH * 255 + 5, 32)])
    n_out = TILE + 5
    n_same = need(256, 1, q_tile + 1, SEAM_PHASE0, n_out)
    rows = [(1, SEAM_PHASE0, n_same, n_out, 256, 1, 0, q_tile * 256), (1, SEAM_PHASE0, n_same, n_out, 256, 1, len(h), (q_tile + 1) * 256)]
    other = 2 * len(h) + 256
    for i, (U, D, Q) in enumerate(((1, d_tile, 8), (1, d_tile + 1, 8), (255, 256, q2_tile), (255, 256, q2_tile + 1))):
        rows.append((i, i, need(U, D, Q, i, n_out), n_out, U, D, other + i, Q * U))
    total = max(r[0] + r[2] for r in rows)
    return noise(total, 30), taps, place(rows)


def nonfinite_case():
    """NaN and inf samples, float32 subnormals in samples and taps, and zero taps beside an inf sample (0 * inf is a NaN), in
    both forms: the outputs whose window holds a NaN, or an inf under a zero tap, are the one quiet NaN, the others finite or
    infinite as IEEE says"""
    iq = noise(9000, 60)
    iq[291, 0] = np.nan						# inside a window of the D = 16 jobs too
    iq[900] = (np.inf, 1.0)
    iq[1500] = (-np.inf, np.inf)
    iq[2000:2040] *= np.float32(1e-42)				# subnormal samples
    iq[2100:2110] = 0.0
    iq[2105, 1] = -0.0
    taps = some_taps(64, 61)
    taps[5] = taps[17] = 0.0
    taps[6] = -0.0
    taps[30:34] = np.float32(3e-45), np.float32(-1e-40), np.float32(1e-38), np.float32(1e-39)
    rows = []
    for U, D, Q in COUNT_FORMS + ((1, 1, 1), (2, 3, 16)):
        n_out = max_n_out(2500, U, D, Q * U)
        rows.append((0, 0, 2500, n_out, U, D, 0, Q * U))
        rows.append((1, 1, 2300, max_n_out(2300, U, D, Q * U, 1), U, D, 28, Q * U))
    return iq, taps, place(rows)


def mixed_case(count=257):
    """257 jobs of both forms whose input ranges overlap, some of them several tiles long"""
    rng = np.random.default_rng(257)
    total = 40000
    pool = ((1, 1, 1), (1, 1, 17), (3, 2, 4), (2, 3, 8), (7, 5, 3), (4, 1, 12), (1, 4, 9), (5, 1, 2), (1, 16, 5), (1, 40, 3), (16, 1, 64),
            (160, 147, 4), (256, 255, 60), (1, 12, 64))
    rows = []
    for i in range(count):
        U, D, Q = pool[int(rng.integers(0, len(pool)))]
        n_out = int(rng.integers(TILE + 1, 3 * TILE)) if i % 16 == 5 else int(rng.integers(0, 400))
        if i % 16 == 5 and need(U, D, Q, 0, n_out) > total // 2:
            U, D, Q = (3, 2, 4) if i % 32 == 5 else (1, 16, 5)
        ph = int(rng.integers(0, 3 * U))
        n = need(U, D, Q, ph, n_out) + int(rng.integers(0, 3))
        rows.append((int(rng.integers(0, total - n + 1)), ph, n, n_out, U, D, int(rng.integers(0, 4)), Q * U))
    return noise(total, 70), some_taps(MAX_BRANCH * MAX_UP + 3, 71), place(rows)


def cases():
    """name -> (iq, taps, jobs): every set the CPU and GPU tests share, but the cut rule and the chain"""
    return {"ratios": ratios_case(), "counts": counts_case(), "seam": seam_case(), "nonfinite": nonfinite_case(),
            "mixed257": mixed_case()}


CUT_FORMS = ((3, 2, 4), (7, 5, 3), (1, 16, 5), (256, 1, 2))


def cut_case():
    """rule 3: every (U, D, Q) of CUT_FORMS as three jobs -- the whole, and the two it is cut into at output c, where c is chosen
    inside a tile, on both sides of a tile's and of a DIRECT work-group's edge and in the last tile.
    -> (case, [(whole, first, second, c)] job indices)"""
    L, off = 2 * TILE + 77, 3
    rows, triples = [], []
    for U, D, Q in CUT_FORMS:
        ph = U + 2
        n = need(U, D, Q, ph, L) + 1
        for c in (1, 5, 255, 256, 257, TILE - 1, TILE, TILE + 1, L - 1):
            triples.append((len(rows), len(rows) + 1, len(rows) + 2, c))
            rows += [(off, ph, n, L, U, D, 1, Q * U), (off, ph, n, c, U, D, 1, Q * U), (off, ph + c * D, n, L - c, U, D, 1, Q * U)]
    total = max(r[0] + r[2] for r in rows)
    return (noise(total, 80), some_taps(513, 81), place(rows)), triples


def assert_cut(outs, triples):
    """the cut rule over the outputs (uint32 views or float arrays, two per sample) of cut_case()"""
    for w, a, b, c in triples:
        whole, first, second = outs[w], outs[a], outs[b]
        assert len(first) == 2 * c and len(first) + len(second) == len(whole) and len(second) >= 2
        assert whole[:2 * c].tobytes() == first.tobytes() and whole[2 * c:].tobytes() == second.tobytes(), (w, c)


# ---- the chain: extract -> resample -> correlate ----------------------------------------------------------------------------------

CHAIN_DECIM, CHAIN_TAPS, CHAIN_CENTRE = 8, 65, 0.2		# the extract job: as in correlate_model
CHAIN_UP, CHAIN_DOWN, CHAIN_BRANCH = 2, 3, 12			# the resampler: 2 / 3, T = 24
CHAIN_RAW_PER_TPL = CHAIN_DECIM * CHAIN_DOWN // CHAIN_UP	# 12 raw samples a template sample: 3 / 2 extract samples
CHAIN_HOLD, CHAIN_SYMBOLS = 4, 64				# the preamble: 64 QPSK symbols, each held for 4 template samples
CHAIN_T = CHAIN_HOLD * CHAIN_SYMBOLS
CHAIN_FIRST, CHAIN_LAST, CHAIN_LAG = 2000, 30000, 700
CHAIN_TPL_OFFSET = 3


def chain_case():
    """A small sc16 stream: noise of 0.02 a component and, at 0.25, a preamble of CHAIN_SYMBOLS QPSK symbols on the carrier
    CHAIN_CENTRE, each template sample held for CHAIN_RAW_PER_TPL = 12 raw samples: 3 / 2 samples of the extract job's output,
    which is at 1 / CHAIN_DECIM of the raw rate.  The resampler by 2 / 3 brings that to one sample per template sample.
    Extract output j is centred on raw sample first + 8 j + 32 (its 65 taps: a delay of 4 whole extract samples).  Resampler
    output m is centred (3 m + 23 / 2) / 2 extract samples behind its input 0, 12 m + 46 raw samples: T = Q U is even for an even
    U, so the delay 23 / 6 output samples cannot be a whole number of them -- the tap counts make both delays a whole number of
    RAW samples instead, and the preamble is planted where that puts it.  Template sample i is centred on raw sample
    m0 + 12 i + 11 / 2, so with m0 = first + 12 lag + 32 + 46 - 11 / 2 + 1 / 2 (an integer) the template lies at output lag
    CHAIN_LAG, half a raw sample -- a twenty-fourth of an output sample -- late.
    -> (raw int16 [n][2], extract jobs [1], tpl float32 [CHAIN_TPL_OFFSET + T][2], planted lag)"""
    rng = np.random.default_rng(4321)
    n = 32000
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    sym = np.exp(0.5j * np.pi * (rng.integers(0, 4, CHAIN_SYMBOLS) + 0.5))
    p = np.repeat(sym, CHAIN_HOLD)
    inc = int(round(CHAIN_CENTRE * 2.0 ** 32))
    delay = (CHAIN_TAPS - 1) // 2 + CHAIN_DECIM * (CHAIN_BRANCH * CHAIN_UP - 1) // (2 * CHAIN_UP)	# 32 + 46 raw samples
    assert (CHAIN_DECIM * (CHAIN_BRANCH * CHAIN_UP - 1)) % (2 * CHAIN_UP) == 0
    m0 = CHAIN_FIRST + CHAIN_LAG * CHAIN_RAW_PER_TPL + delay - (CHAIN_RAW_PER_TPL - 1) // 2
    m = np.arange(m0, m0 + CHAIN_T * CHAIN_RAW_PER_TPL)
    x[m] += 0.25 * np.repeat(p, CHAIN_RAW_PER_TPL) * np.exp(2j * np.pi * (inc / 2.0 ** 32) * m)
    raw = np.round(np.stack([x.real, x.imag], 1) * 32768.0).astype(np.int16)
    jobs = np.zeros(1, EXTRACT_DTYPE)
    j = jobs[0]
    j["first"], j["decim"], j["phase_inc"], j["phase0"], j["taps_offset"], j["n_taps"] = CHAIN_FIRST, CHAIN_DECIM, inc, 0, 0, CHAIN_TAPS
    j["n_out"] = (CHAIN_LAST - CHAIN_FIRST - CHAIN_TAPS) // CHAIN_DECIM + 1
    j["out_offset"] = 1						# an odd offset into d_out
    tpl = np.zeros((CHAIN_TPL_OFFSET + CHAIN_T, 2), np.float32)
    tpl[CHAIN_TPL_OFFSET:, 0], tpl[CHAIN_TPL_OFFSET:, 1] = p.real, p.imag
    return raw, jobs, tpl, CHAIN_LAG


def chain_margin(rho, lag):
    """(the peak, the largest rho more than T / 4 lags away from it): the condition on the chain's input is peak >= 2 * far"""
    k = np.arange(len(rho))
    return float(rho[lag]), float(rho[np.abs(k - lag) > CHAIN_T // 4].max())
