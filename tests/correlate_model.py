"""numpy statement of rules 1-3 of include/fosphor_amd_correlate.h and the input sets the CPU and GPU tests share.

A case is (iq, tpl, jobs): iq and tpl float32 [n][2] as they lie in memory -- tpl is None where the templates are taken from iq
itself -- and jobs a JOB_DTYPE array whose traces are placed with GUARD floats before, between and behind them (place()).  The sums
are vectorised over the lags with a Python loop over the template index i, ascending: that is the pinned order.  Every operation is
one IEEE double operation that numpy rounds once (a product, then an addition); the products are exact, so the device's fused
multiply-adds and fosphor_amd_correlate_host's a * b + s give the same bits.  A NaN float is 0x7fc00000, a NaN double of the record
0x7ff8000000000000 (rule 2).  Sigma n_lags * T of a case stays at or below 2^24 (macs())."""
import numpy as np

from measure_model import EXTRACT_DTYPE

JOB_DTYPE = np.dtype([("offset", "<i8"), ("out_offset", "<i8"), ("tpl_offset", "<i8"), ("n", "<i4"), ("tpl_len", "<i4"),
                      ("trace", "<i4"), ("threshold", "<f4")])
RECORD_DTYPE = np.dtype([("n_lags", "<i4"), ("n_above", "<i4"), ("first_above", "<i4"), ("last_above", "<i4"), ("n_edges", "<i4"),
                         ("peak_lag", "<i4"), ("peak_rho", "<f4"), ("tpl_len", "<i4"), ("peak_c_re", "<f8"), ("peak_c_im", "<f8"),
                         ("peak_energy", "<f8"), ("tpl_energy", "<f8")])
STATS = ("calls", "k_tile", "k_combine", "jobs", "lags", "macs")
MAX_JOBS, MAX_TPL, TILE = 4096, 1024, 1024
NONE, RHO, C = 0, 1, 2
TRACES = {"none": NONE, "rho": RHO, "c": C}
GUARD = 3						# sentinel floats before, between and behind the jobs' traces
MAX_MACS = 2 ** 24
QNAN = np.frombuffer(np.uint32(0x7fc00000).tobytes(), np.float32)[0]
QNAN64 = np.frombuffer(np.uint64(0x7ff8000000000000).tobytes(), np.float64)[0]


def quiet(v):
    v = np.array(v, np.float32)
    v[np.isnan(v)] = QNAN
    return v


def quiet64(v):
    v = np.array(v, np.float64)
    v[np.isnan(v)] = QNAN64
    return v


def n_lags(n, T):
    return max(n - T + 1, 0)


def n_out(trace, n, T):
    return n_lags(n, T) * trace


def sums(y, t):
    """rule 1: (cre, cim, E) per lag in float64 and Et, from y float32 [n][2] and t float32 [T][2]"""
    y, t = np.asarray(y, np.float32).reshape(-1, 2), np.asarray(t, np.float32).reshape(-1, 2)
    T, L = len(t), n_lags(len(y), len(t))
    yr, yi = y[:, 0].astype(np.float64), y[:, 1].astype(np.float64)
    tr, ti = t[:, 0].astype(np.float64), t[:, 1].astype(np.float64)
    cre, cim, E, Et = np.zeros(L), np.zeros(L), np.zeros(L), np.float64(0.0)
    with np.errstate(all="ignore"):
        for i in range(T):
            a, b = yr[i:i + L], yi[i:i + L]
            cre = cre + a * tr[i]
            cre = cre + b * ti[i]
            cim = cim + b * tr[i]
            cim = cim - a * ti[i]
            E = E + a * a
            E = E + b * b
            Et = Et + tr[i] * tr[i]
            Et = Et + ti[i] * ti[i]
    return cre, cim, E, Et


def rho_of(cre, cim, E, Et):
    """rule 2: float32 per lag"""
    with np.errstate(all="ignore"):
        num = (cre * cre) + (cim * cim)
        den = E * Et
        return quiet(np.where(den == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den)).astype(np.float32))


def buffers(case):
    """(iq, tpl) of a case, float32 [n][2]: the templates of a case without tpl lie in iq"""
    iq = np.ascontiguousarray(case[0], np.float32).reshape(-1, 2)
    return iq, iq if case[1] is None else np.ascontiguousarray(case[1], np.float32).reshape(-1, 2)


def correlate_job(iq, tpl, job):
    """-> (record as a RECORD_DTYPE scalar array [1], the trace floats float32 [n_out], rho32 per lag)"""
    y = iq[int(job["offset"]):int(job["offset"]) + int(job["n"])]
    t = tpl[int(job["tpl_offset"]):int(job["tpl_offset"]) + int(job["tpl_len"])]
    cre, cim, E, Et = sums(y, t)
    rho = rho_of(cre, cim, E, Et)
    r = np.zeros(1, RECORD_DTYPE)
    r["n_lags"], r["tpl_len"], r["tpl_energy"] = len(rho), len(t), quiet64(Et)
    above = rho >= np.float32(job["threshold"])			# a NaN is not above
    r["n_above"] = above.sum()
    at = np.flatnonzero(above)
    r["first_above"], r["last_above"] = (at[0], at[-1]) if len(at) else (-1, -1)
    r["n_edges"] = (int(above[0]) + int((above[1:] & ~above[:-1]).sum())) if len(above) else 0
    ok = ~np.isnan(rho)
    r["peak_lag"] = -1
    if ok.any():
        k = int(np.flatnonzero(rho == rho[ok].max())[0])		# the smallest lag of the largest non-NaN rho
        r["peak_lag"], r["peak_rho"] = k, rho[k]
        r["peak_c_re"], r["peak_c_im"], r["peak_energy"] = quiet64(cre[k]), quiet64(cim[k]), quiet64(E[k])
    trace = int(job["trace"])
    if trace == RHO:
        out = rho
    elif trace == C:
        with np.errstate(all="ignore"):
            out = quiet(np.stack([cre, cim], 1).astype(np.float32).reshape(-1))
    else:
        out = np.zeros(0, np.float32)
    return r, out, rho


def correlate(case):
    """(records RECORD_DTYPE [n_jobs], [trace floats per job])"""
    iq, tpl = buffers(case)
    got = [correlate_job(iq, tpl, j) for j in case[2]]
    return np.concatenate([g[0] for g in got]), [g[1] for g in got]


def macs(jobs):
    return sum(n_lags(int(j["n"]), int(j["tpl_len"])) * int(j["tpl_len"]) for j in jobs)


def capacity(jobs):
    """floats of the output buffer of a case: the last trace float and GUARD behind it"""
    return max([int(j["out_offset"]) + n_out(int(j["trace"]), int(j["n"]), int(j["tpl_len"])) for j in jobs] + [0]) + GUARD


def image(case, fill):
    """(records, the whole output buffer as the model leaves it: uint32 [capacity], `fill` wherever no job writes)"""
    jobs = case[2]
    records, traces = correlate(case)
    out = np.full(capacity(jobs), fill, np.uint32)
    for j, v in zip(jobs, traces):
        out[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v.view(np.uint32)
    return records, out


# ---- the builders ---------------------------------------------------------------------------------------------------------------

def make_jobs(rows):
    """rows of (offset, out_offset, tpl_offset, n, tpl_len, trace, threshold)"""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    for j, r in zip(jobs, rows):
        j["offset"], j["out_offset"], j["tpl_offset"], j["n"], j["tpl_len"], j["trace"], j["threshold"] = r
    return jobs


def place(rows):
    """rows of (offset, tpl_offset, n, tpl_len, trace, threshold) -> jobs whose traces follow each other with GUARD or GUARD + 1
    floats between them, so that odd and even out_offsets both occur whatever the lengths are; a job without a trace has
    out_offset 0"""
    out, at = [], GUARD
    for i, (off, toff, n, T, trace, thr) in enumerate(rows):
        out.append((off, at if trace else 0, toff, n, T, trace, thr))
        if trace:
            at += n_out(trace, n, T) + GUARD + (i & 1)
    return make_jobs(out)


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2)) * np.exp(rng.uniform(-1.0, 1.0, (n, 1)))).astype(np.float32)


TS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)


def tpl_lengths_case():
    """every T of TS with n = 0, T - 1 (no lag), T (one lag) and n_lags = 255, 256, 257; offset and tpl_offset walk 0 .. 3 in
    both parities against each other; the traces walk none, rho, c; thresholds around what noise gives (1 / T)"""
    rows, i = [], 0
    for T in TS:
        for n in (0, T - 1, T, T + 254, T + 255, T + 256):
            rows.append((i % 4, (i // 4 + i) % 4, n, T, i % 3, 1.0 / T))
            i += 1
    return noise(TS[-1] + 256 + 3, 10), noise(TS[-1] + 3, 11), place(rows)


def lag_counts_case():
    """n_lags = 1023 .. 1025, 2 TILE + 1 and 3 TILE + 5 with an even and an odd T; the longest job of each T ends on the buffer's
    last sample"""
    counts = (1023, 1024, 1025, 2 * TILE + 1, 3 * TILE + 5)
    total = counts[-1] + 257 - 1 + 2
    rows, i = [], 0
    for T in (64, 257):
        for L in counts:
            n = L + T - 1
            off = total - n if L == counts[-1] else i % 4
            rows.append((off, (i + 1) % 4, n, T, (RHO, C, NONE)[i % 3], 2.0 / T))
            i += 1
    return noise(total, 20), noise(257 + 3, 21), place(rows)


TIE_T, TIE_AT = 48, 100


def tie_case():
    """the template is iq[TIE_AT .. TIE_AT + T) itself, and the same T samples lie once more TILE + 37 lags later: two
    bit-identical windows in different tiles.  cre == E == Et there and cim == 0, so rho is the same float at both lags and
    the larger of all; the smaller lag wins.  A second job begins 60 samples in, so that the windows fall into tiles 0 and 1 at
    other lanes; the last sees only the second of them."""
    iq = noise(3 * TILE, 30)
    second = TIE_AT + TILE + 37
    iq[second:second + TIE_T] = iq[TIE_AT:TIE_AT + TIE_T]
    rows = [(0, TIE_AT, 3 * TILE, TIE_T, RHO, 0.5), (60, TIE_AT, 2 * TILE, TIE_T, NONE, 0.5), (1, TIE_AT, 3 * TILE - 1, TIE_T, C, 0.5),
            (TIE_AT + 7, TIE_AT, TILE + 200, TIE_T, RHO, 0.5)]
    return iq, None, place(rows)


def edges_pattern():
    """which of 3 TILE + 5 lags are above, for T = 1: runs over both seams, a single lag on each side of a seam, the first and
    the last lag, a tile that ends above while the next begins below, and the other way round"""
    on = np.zeros(3 * TILE + 5, bool)
    on[0] = True
    on[5:9] = True
    on[TILE - 1:TILE + 1] = True				# lags TILE - 1 and TILE: one edge across the seam
    on[2 * TILE - 1] = True					# a tile ends above, the next begins below
    on[3 * TILE] = True						# a tile ends below, the next begins above
    on[3 * TILE + 2:] = True					# up to the last lag
    rng = np.random.default_rng(41)
    on[TILE + 50:2 * TILE - 50] = rng.random(TILE - 100) < 0.3
    return on


def edges_case():
    """T = 1 with the template (1, 0): rho is 1 (within an ulp) where the sample is not zero and 0 where it is (den == 0).  The
    threshold 0.5 makes `above` the pattern of edges_pattern().  Also T = 2 over the same samples, and thresholds of 0, below 0
    and +inf: everything, everything and nothing is above."""
    on = edges_pattern()
    iq = noise(len(on), 40)
    iq[~on] = 0.0
    tpl = np.array([(1.0, 0.0), (0.6, -0.8), (0.0, 2.0)], np.float32)
    n = len(on)
    rows = [(0, 0, n, 1, RHO, 0.5), (0, 0, n, 1, NONE, 0.5), (1, 1, n - 1, 1, C, 0.5), (0, 1, n, 2, RHO, 0.5),
            (0, 0, n, 1, NONE, 0.0), (0, 0, n, 1, NONE, -1.0), (0, 0, n, 1, RHO, np.inf), (TILE - 1, 2, 2, 1, RHO, 0.5)]
    return iq, tpl, place(rows)


def silence_case():
    """silence against a template (den == 0: rho = 0), noise against an all-zero template (Et == 0: rho = 0), both at once; the
    peak of an all-zero rho is lag 0 with rho 0"""
    iq = noise(TILE + 300, 50)
    iq[100:700] = 0.0
    tpl = noise(40, 51)
    tpl[8:24] = 0.0
    rows = [(100, 0, 600, 8, RHO, 0.0), (100, 8, 600, 16, RHO, 0.0), (0, 8, TILE + 300, 16, C, 0.5), (90, 0, 620, 8, RHO, 0.1),
            (0, 9, TILE + 300, 3, NONE, -0.0), (100, 24, 600, 7, C, 1e-3)]
    return iq, tpl, place(rows)


def nonfinite_case():
    """NaN and inf samples in the signal: the lags whose window holds one are NaN, the others finite, and the peak is the largest
    of the others.  A template with a NaN, and one with an inf beside zeros in the signal: every rho is NaN, there is no peak, and
    tpl_energy is the one NaN or inf."""
    iq = noise(2 * TILE + 100, 60)
    iq[300, 0] = np.nan
    iq[900] = (np.inf, 1.0)
    iq[TILE + 20] = (-np.inf, np.inf)
    iq[2000:2030] = 0.0
    tpl = noise(64, 61)
    tpl[40, 1] = np.nan
    tpl[50, 0] = np.inf
    rows = [(0, 0, 2 * TILE + 100, 16, RHO, 0.1), (0, 0, 2 * TILE + 100, 16, C, 0.1), (1, 1, 2 * TILE, 33, NONE, 0.05),
            (0, 32, 500, 16, RHO, 0.1), (0, 44, 500, 12, C, 0.1), (2000, 48, 30, 4, RHO, 0.1), (290, 0, 20, 16, RHO, 0.1),
            (0, 36, 3, 8, NONE, 0.1)]
    return iq, tpl, place(rows)


def mixed_case(count=257):
    """257 jobs of all three traces whose input ranges overlap, some of them several tiles long"""
    rng = np.random.default_rng(257)
    total = 2 * TILE + 900
    tpl = noise(300, 71)
    rows = []
    for i in range(count):
        T = (1, 2, 3, 7, 16, 64, 65, 128, 255)[int(rng.integers(0, 9))]
        n = int(rng.integers(TILE + 1, total)) if i % 16 == 5 else int(rng.integers(0, 500))
        T = min(T, 65) if i % 16 == 5 else T
        rows.append((int(rng.integers(0, total - n + 1)), int(rng.integers(0, 300 - T + 1)), n, T, i % 3, 1.5 / T))
    return noise(total, 70), tpl, place(rows)


def cases():
    """name -> (iq, tpl, jobs): every set the CPU and GPU tests share, but the cut rule and the chain"""
    return {"tpl_lengths": tpl_lengths_case(), "lag_counts": lag_counts_case(), "tie": tie_case(), "edges": edges_case(),
            "silence": silence_case(), "nonfinite": nonfinite_case(), "mixed257": mixed_case()}


CUT_FORMS = ((1, RHO), (64, C), (257, RHO), (33, C))


def cut_case():
    """rule 4: every (T, trace) of CUT_FORMS as three jobs -- the whole, and the two it is cut into at lag c, where c is chosen
    inside a tile, on both sides of a tile's edge and in the last tile.  -> (case, [(whole, first, second, c)] job indices)"""
    L, off = 2 * TILE + 77, 3
    rows, triples = [], []
    for T, trace in CUT_FORMS:
        n = L + T - 1
        for c in (1, 5, TILE - 1, TILE, TILE + 1, L - 1):
            triples.append((len(rows), len(rows) + 1, len(rows) + 2, c))
            rows += [(off, 1, n, T, trace, 1.0 / T), (off, 1, c + T - 1, T, trace, 1.0 / T), (off + c, 1, n - c, T, trace, 1.0 / T)]
    return (noise(L + 257 - 1 + off, 80), noise(258, 81), place(rows)), triples


def assert_cut(records, traces, jobs, triples):
    """the cut rule over the records and the traces (uint32 views or float arrays) of cut_case()"""
    for w, a, b, c in triples:
        whole, first, second = traces[w], traces[a], traces[b]
        per = int(jobs["trace"][w])
        assert len(first) == c * per and len(first) + len(second) == len(whole) and len(second) >= per
        assert whole[:c * per].tobytes() == first.tobytes() and whole[c * per:].tobytes() == second.tobytes(), (w, c)
        rw, ra, rb = records[w], records[a], records[b]
        assert ra["n_lags"] == c and ra["n_lags"] + rb["n_lags"] == rw["n_lags"]
        assert rw["n_above"] == ra["n_above"] + rb["n_above"]
        assert rw["first_above"] == (ra["first_above"] if ra["n_above"] else rb["first_above"] + c if rb["n_above"] else -1)
        assert rw["last_above"] == (rb["last_above"] + c if rb["n_above"] else ra["last_above"])
        seam = ra["last_above"] == c - 1 and rb["first_above"] == 0
        assert rw["n_edges"] == ra["n_edges"] + rb["n_edges"] - int(seam), (w, c)
        assert rw["tpl_energy"].tobytes() == ra["tpl_energy"].tobytes() == rb["tpl_energy"].tobytes()
        win = ra if ra["peak_rho"] >= rb["peak_rho"] else rb
        assert rw["peak_rho"].tobytes() == win["peak_rho"].tobytes() and rw["peak_lag"] == win["peak_lag"] + (c if win is rb else 0)
        for k in ("peak_c_re", "peak_c_im", "peak_energy"):
            assert rw[k].tobytes() == win[k].tobytes(), (w, c, k)


# ---- the chain: extract -> correlate ---------------------------------------------------------------------------------------------

CHAIN_DECIM, CHAIN_TAPS, CHAIN_CENTRE = 8, 65, 0.2
CHAIN_HOLD, CHAIN_SYMBOLS = 4, 64				# the preamble: 64 QPSK symbols, each held for 4 output samples
CHAIN_T = CHAIN_HOLD * CHAIN_SYMBOLS
CHAIN_FIRST, CHAIN_LAST, CHAIN_LAG = 2000, 30000, 1500
CHAIN_TPL_OFFSET = 3


def chain_case():
    """A small sc16 stream: noise of 0.02 a component and, at 0.25, a preamble of CHAIN_SYMBOLS QPSK symbols on the carrier
    CHAIN_CENTRE, each symbol held for CHAIN_HOLD * CHAIN_DECIM input samples.  One extract job brings samples CHAIN_FIRST ..
    CHAIN_LAST to baseband at 1 / CHAIN_DECIM of the rate.  Output sample j is centred on input sample first + j D + (taps - 1) / 2
    and template sample i on m0 + i D + (D - 1) / 2, so with m0 = first + lag D + (taps - 1) / 2 - (D - 1) / 2 + 1 / 2 (an integer)
    the template lies at output lag CHAIN_LAG, half an input sample -- a sixteenth of an output sample -- late.
    -> (raw int16 [n][2], extract jobs [1], tpl float32 [CHAIN_TPL_OFFSET + T][2], planted lag)"""
    rng = np.random.default_rng(1234)
    n = 32000
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    sym = np.exp(0.5j * np.pi * (rng.integers(0, 4, CHAIN_SYMBOLS) + 0.5))
    p = np.repeat(sym, CHAIN_HOLD)
    inc = int(round(CHAIN_CENTRE * 2.0 ** 32))
    m0 = CHAIN_FIRST + CHAIN_LAG * CHAIN_DECIM + (CHAIN_TAPS - 1) // 2 - (CHAIN_DECIM - 1) // 2
    m = np.arange(m0, m0 + CHAIN_T * CHAIN_DECIM)
    x[m] += 0.25 * np.repeat(p, CHAIN_DECIM) * np.exp(2j * np.pi * (inc / 2.0 ** 32) * m)
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
