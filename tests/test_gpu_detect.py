"""Detection on the device (include/fosphor_amd_detect.h) against its numpy statement (tests/detect_model.py).

Inputs are planted straight into the instance's buffers (gr_fosphor_amd.dist.wrap_device_array over fosphor_amd_get_buffers_nohc),
so every seam of the kernels is hit on purpose, and every planted test ends by checking that the buffers are bit-identical: the
passes only read.  Geometries: 1024 points with 128 bins, and 65536 points with 512 bins and max_spectra = 16.

Seams.  k_percentiles: a wave owns 64 adjacent columns and loads 32 bins ahead (both geometries are multiples of both).  k_bands:
FOSPHOR_AMD_DETECT_LANES = 1024 lanes, lane t owns the window's columns [t * chunk, (t + 1) * chunk), chunk = ceil(n_cols / 1024);
waves of 64 lanes meet every 64 * chunk columns.  One percentile form exists, so there is no form to select.
"""
import ctypes as C
import errno
import os

import numpy as np
import pytest

import detect_model as dm
from oracle_lib import Oracle, gaussian_iq, add_tone

pytestmark = pytest.mark.gpu

GEOMETRIES = [(10, 128), (16, 512)]
Q4 = [0.1, 0.5, 0.9, 1.0]
SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Planted:
    """an instance and torch views of its histogram [n_bins][N] and spectrum [2][N][2] buffers"""

    def __init__(self, amd, log, bins):
        import torch
        from gr_fosphor_amd.dist import wrap_device_array
        if log == 10:
            self.f = amd.Fosphor(n_bins=bins, wf_rows=16)
        else:
            self.f = amd.Fosphor(fft_len_log=log, n_bins=bins, wf_rows=16, max_spectra=16)
        self.n, self.bins, self.lib = self.f.n, bins, amd._lib
        assert self.f.finish() >= 0			# a new instance fills its buffers at its first wait (the boot): before anything is planted
        b = self.f.buffers(False)
        assert (b.fft_len, b.n_bins) == (self.n, bins)
        self.hist = wrap_device_array(b.d_histogram, (bins, self.n), torch.float32)
        self.spec = wrap_device_array(b.d_spectrum, (2, self.n, 2), torch.float32)
        self.table = dm.bin_y(bins, b.histo_scale, b.histo_offset)
        self.saved = None

    def plant(self, hist=None, live=None, maxhold=None):
        import torch
        if hist is not None:
            self.hist.copy_(torch.from_numpy(np.ascontiguousarray(hist, dtype=np.float32)))
        for row, y in ((0, live), (1, maxhold)):
            if y is not None:
                self.spec[row, :, 1].copy_(torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)))
        torch.cuda.synchronize()
        self.saved = (self.hist.view(torch.int32).clone(), self.spec.view(torch.int32).clone())

    def assert_untouched(self):
        import torch
        torch.cuda.synchronize()
        assert torch.equal(self.hist.view(torch.int32), self.saved[0]), "the histogram was written"
        assert torch.equal(self.spec.view(torch.int32), self.saved[1]), "the spectrum lines were written"

    def detect_raw(self, cfg, max_bands, alloc=None):
        """fosphor_amd_detect through the C ABI into sentinel-filled buffers -> (rv, result dict, all `alloc` band entries)"""
        import torch
        lib = self.f.L
        alloc = max_bands if alloc is None else alloc
        d_res = torch.full((5,), SENTINEL, dtype=torch.int32, device="cuda")
        d_bands = torch.full((max(alloc, 1) * 5,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()			# the fills run on torch's stream, the pass on the instance's
        rv = lib.fosphor_amd_detect(self.f.h, C.byref(cfg) if cfg is not None else None, d_res.data_ptr(), d_bands.data_ptr(), max_bands)
        raw = d_res.cpu().numpy()
        res = dict(n_found=int(raw[0]), n_written=int(raw[1]), floor_bin=int(raw[2]),
                   floor_y=raw[3:4].view(np.float32)[0], threshold_y=raw[4:5].view(np.float32)[0])
        return rv, res, d_bands.cpu().numpy().view(dm.BAND_DTYPE), raw


def same_f32(a, b):
    return np.array_equal(np.asarray(a, np.float32).reshape(-1).view(np.uint32), np.asarray(b, np.float32).reshape(-1).view(np.uint32))


def assert_result(got, want, tag=""):
    for k in ("n_found", "n_written", "floor_bin"):
        assert got[k] == want[k], (tag, k, got[k], want[k])
    for k in ("floor_y", "threshold_y"):
        assert same_f32(got[k], want[k]), (tag, k, got[k], want[k])


# ---- percentiles --------------------------------------------------------------------------------------------------------

def percentile_histogram(n, bins):
    """Random non-negative cells of mixed magnitude, 1e-3 .. 1e3, and the special columns (memory columns):
    0: all mass in bin 0; N/2: all mass in the last bin; 5, 6, 7, N-1, N/2+64: empty; 9: ten ones (c_b == q * T exactly at
    q = 0.5 and 1.0: T = 10, c_4 = 5); 70: small integers 1, 2, 3, ... (c_b == q * T at q = 1.0).
    With seed 7 a sum in another order -- the pairwise order of a parallel scan over the bins, c[d:] += c[:-d] for d = 1, 2, 4, ... --
    gives 4 different bins of the 4 x 1024 at (1024, 128) and 2668 of the 4 x 65536 at (65536, 512) for q = Q4, and four partial
    sums of n_bins / 4 bins combined, as four lanes sharing a column would form them, give 2179 at (65536, 512) (counted on the CPU
    with the model when this test was written), so the order of the sum is under test."""
    rng = np.random.default_rng(7)
    h = np.power(10.0, rng.uniform(-3.0, 3.0, (bins, n))).astype(np.float32)
    h[:, 0] = 0; h[0, 0] = 3.5
    h[:, n // 2] = 0; h[bins - 1, n // 2] = 0.25
    for x in (5, 6, 7, n - 1, n // 2 + 64):
        h[:, x] = 0
    h[:, 9] = 0; h[:10, 9] = 1
    h[:, 70] = np.arange(1, bins + 1)
    return h


@pytest.fixture(scope="module", params=GEOMETRIES, ids=lambda g: "N%d_bins%d" % (1 << g[0], g[1]))
def pct(request, amd):
    log, bins = request.param
    s = Planted(amd, log, bins)
    h = percentile_histogram(s.n, bins)
    s.plant(hist=h)
    s.want = dm.percentile_bins(h, Q4)
    yield s
    s.f.close()


def run_percentiles(s, q, want_y=True, want_bin=True):
    import torch
    qa = np.asarray(q, np.float32)
    d_y = torch.full((len(q), s.n), SENTINEL, dtype=torch.int32, device="cuda")
    d_bin = torch.full((len(q), s.n), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()				# the fills run on torch's stream, the pass on the instance's
    rv = s.f.L.fosphor_amd_percentiles(s.f.h, qa.ctypes.data, len(q), d_y.data_ptr() if want_y else None, d_bin.data_ptr() if want_bin else None)
    return rv, d_y.cpu().numpy().view(np.float32), d_bin.cpu().numpy()


def test_percentiles_exact(pct):
    s, n, bins = pct, pct.n, pct.bins
    want = s.want
    # the model sees the special columns as planned
    assert np.all(want[:, n // 2] == 0) and np.all(want[:, 0] == bins - 1)		# memory 0 -> shifted N/2, memory N/2 -> shifted 0
    for x in (5, 6, 7, n - 1, n // 2 + 64):
        assert np.all(want[:, x ^ (n // 2)] == -1)
    assert want[:, 9 ^ (n // 2)].tolist() == [0, 4, 8, 9]
    assert (want >= 0).sum() == 4 * (n - 5)
    before = s.f.detect_stats()

    rv, y, b = run_percentiles(s, Q4)
    assert rv == 0
    assert np.array_equal(b, want)
    assert same_f32(y, dm.percentile_y(want, s.table))
    assert np.isnan(y[:, 5 ^ (n // 2)]).all()
    rv, y, b = run_percentiles(s, [0.5])						# one q alone
    assert rv == 0 and np.array_equal(b, want[1:2]) and same_f32(y, dm.percentile_y(want[1:2], s.table))
    rv, y, b = run_percentiles(s, [1.0, 0.1, 0.5], want_y=False)			# three, in any order; d_y NULL
    assert rv == 0 and np.array_equal(b, want[[3, 0, 1]]) and np.all(y.view(np.int32) == SENTINEL)
    rv, y, b = run_percentiles(s, [0.9, 0.1], want_bin=False)				# two; d_bin NULL
    assert rv == 0 and same_f32(y, dm.percentile_y(want[[2, 0]], s.table)) and np.all(b == SENTINEL)
    py, pb = s.f.percentiles(Q4, bins=True)						# the Python class
    assert np.array_equal(pb, want) and same_f32(py, dm.percentile_y(want, s.table))
    assert same_f32(s.f.percentiles(0.5), dm.percentile_y(want[1:2], s.table))
    after = s.f.detect_stats()
    assert after["percentiles"] - before["percentiles"] == 6 and after["floor"] == before["floor"] and after["bands"] == before["bands"]
    s.assert_untouched()


def test_percentile_argument_errors(pct):
    s = pct
    nan = float("nan")
    for q in ([], [0.1] * 5, [0.0], [0.5, 0.0], [1.0000001], [0.5, 2.0], [-0.5], [nan], [0.5, 0.9, nan]):
        rv, y, b = run_percentiles(s, q if q else [0.5][:0])
        assert rv == -errno.EINVAL, q
        assert np.all(y.view(np.int32) == SENTINEL) and np.all(b == SENTINEL), q
    rv, y, b = run_percentiles(s, [0.5], want_y=False, want_bin=False)		# both outputs NULL
    assert rv == -errno.EINVAL
    import torch
    d = torch.full((s.n,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert s.f.L.fosphor_amd_percentiles(s.f.h, None, 1, d.data_ptr(), d.data_ptr()) == -errno.EINVAL
    assert bool((d == SENTINEL).all())
    with pytest.raises(RuntimeError):
        s.f.percentiles([0.0])
    with pytest.raises(RuntimeError):
        s.f.percentiles([0.1] * 5)
    s.assert_untouched()


# ---- bands ---------------------------------------------------------------------------------------------------------------

MAX_GAP, MIN_COLS = 2, 3

# patterns for max_gap = 2, min_cols = 3, threshold 0; each is laid between columns that are below.  h / l: above / below with a
# value of its own; N: NaN; digits: that value exactly (ties)
PATTERNS = ["hhlllhhh",		# a run of min_cols - 1 (dropped), a gap of max_gap + 1 (open), a run of min_cols (kept)
            "hhllhh",		# a gap of exactly max_gap (closed)
            "hlh",		# reaches min_cols only through closing
            "hNhNNh",		# NaN columns inside a band
            "h55l5h",		# equal maxima: the lowest column; one of them behind a closed gap
            "NN7N7NN",		# NaN around and between equal maxima
            "hhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhhh"]	# longer than a chunk and a wave's reach


def lay(y, at, pattern, rng):
    for j, ch in enumerate(pattern):
        y[at + j] = (1.0 + rng.random() if ch == "h" else -1.0 - rng.random() if ch == "l" else np.nan if ch == "N" else float(ch))


def planted_trace(n, seed):
    """Below everywhere (values of their own), then: a band at each edge of the buffer; a band [64k - 2, 64k + 1] across every
    multiple of 64 -- every lane seam of the whole-buffer call at 65536 columns (chunk 64), every wave seam at 1024 (chunk 1), the
    multiples of 1024 and the DC column N/2, where memory columns wrap; and the patterns above, once clear of the seams and, at
    65536 columns, once more with each of their columns in turn on a lane seam."""
    rng = np.random.default_rng(seed)
    y = (-1.0 - rng.random(n)).astype(np.float32)
    lay(y, 0, "hhh", rng)
    lay(y, n - 4, "hhhh", rng)
    straddle = {}
    if n > 1024:									# seams 64 * k given to the patterns instead
        k = 3
        for p in PATTERNS:
            for j in range(min(len(p), 8)):
                straddle[k] = (p, j)
                k += 2
    for k in range(1, n // 64):
        if k in straddle:
            p, j = straddle[k]
            lay(y, 64 * k - j, p, rng)							# column j of the pattern on the seam
        else:
            lay(y, 64 * k - 2, "hhhh", rng)
    at = 24
    for p in PATTERNS[:-1]:								# clear of the seams: 64 * k + 24 ..
        lay(y, at, p, rng)
        at += 64
    if n == 1024:
        y[64 * 9 + 2: 64 * 10 - 2] = 1.5						# the long pattern, across 60 lanes
    return y


@pytest.fixture(scope="module", params=GEOMETRIES, ids=lambda g: "N%d_bins%d" % (1 << g[0], g[1]))
def traces(request, amd):
    log, bins = request.param
    s = Planted(amd, log, bins)
    s.live, s.maxhold = planted_trace(s.n, 11), planted_trace(s.n, 12)[::-1].copy()	# two different traces
    h = np.zeros((bins, s.n), np.float32)
    s.plant(hist=h, live=s.live, maxhold=s.maxhold)
    yield s
    s.f.close()


def absolute_cfg(s, trace, first_bin, n_cols, thr=0.0, max_gap=MAX_GAP, min_cols=MIN_COLS):
    return s.lib.DetectCfg(trace, first_bin, n_cols, 0, 0.0, 0.0, thr, max_gap, min_cols)


@pytest.mark.parametrize("trace", [0, 1], ids=["live", "maxhold"])
def test_detect_exact(traces, trace):
    s, n = traces, traces.n
    y = s.live if trace == 0 else s.maxhold
    # the whole buffer; a window that cuts through a band at both ends (and moves every seam: another chunk, an odd origin);
    # a window of fewer columns than lanes
    windows = [(0, n), (63, n - 63 - (n - 64 * (n // 64 - 2))), (n // 2 - 301, 777)]
    assert y[63] > 0 and y[62] > 0 and y[windows[1][0] + windows[1][1] - 1] > 0 and y[windows[1][0] + windows[1][1]] > 0
    for first_bin, n_cols in windows:
        for max_gap, min_cols in [(MAX_GAP, MIN_COLS), (0, 1)]:
            tag = "N=%d trace=%d window=(%d, %d) max_gap=%d min_cols=%d" % (n, trace, first_bin, n_cols, max_gap, min_cols)
            want_res, want = dm.detect(y, first_bin, n_cols, max_gap, min_cols, 65536, threshold_y=0.0)
            rv, res, bands, _ = s.detect_raw(absolute_cfg(s, trace, first_bin, n_cols, 0.0, max_gap, min_cols), 65536, alloc=want_res["n_found"] + 2)
            assert rv == 0, tag
            assert_result(res, want_res, tag)
            worst = dm.assert_bands_equal(bands[:res["n_written"]], want, tag=tag)
            assert np.all(bands["first"][res["n_written"]:] == SENTINEL), tag
            print("%s: %d bands, worst |power_y error| %.3g" % (tag, res["n_found"], worst))
            assert want_res["n_found"] >= (10 if n_cols < 1024 else n_cols // 64 - 40), tag	# the planted bands are there
    # the Python class gives the same
    res, bands = s.f.detect(trace=("live", "maxhold")[trace], floor="absolute", threshold_y=0.0, max_gap=MAX_GAP, min_cols=MIN_COLS, max_bands=4096)
    want_res, want = dm.detect(y, 0, n, MAX_GAP, MIN_COLS, 4096, threshold_y=0.0)
    assert_result(res, want_res)
    dm.assert_bands_equal(bands, want)
    s.assert_untouched()


@pytest.mark.parametrize("density", [0.03, 0.5, 0.97])
def test_detect_random_traces(traces, density):
    """random masks with NaN columns and tied maxima over the whole buffer: every seam sees every situation"""
    s, n = traces, traces.n
    rng = np.random.default_rng(int(density * 100))
    y = (rng.standard_normal(n) * 0.5 + np.where(rng.random(n) < density, 1.0, -1.0)).astype(np.float32)
    y[rng.integers(0, n, n // 40)] = np.nan
    y[rng.integers(0, n, n // 30)] = np.float32(1.25)
    s.plant(live=y)
    for max_gap, min_cols, first_bin, n_cols in [(0, 1, 0, n), (1, 2, 0, n), (3, 4, 1, n - 2), (2, 1, n // 2 - 100, 333)]:
        tag = "N=%d density=%g max_gap=%d min_cols=%d window=(%d, %d)" % (n, density, max_gap, min_cols, first_bin, n_cols)
        want_res, want = dm.detect(y, first_bin, n_cols, max_gap, min_cols, 65536, threshold_y=0.0)
        rv, res, bands, _ = s.detect_raw(absolute_cfg(s, 0, first_bin, n_cols, 0.0, max_gap, min_cols), 65536, alloc=want_res["n_found"] + 1)
        assert rv == 0, tag
        assert_result(res, want_res, tag)
        dm.assert_bands_equal(bands[:res["n_written"]], want, tag=tag)
    s.assert_untouched()
    s.plant(live=s.live)


def test_detect_fixed_cases_and_overflow(traces):
    """the CPU list's cases one by one in a window at the start of the buffer, then max_bands = 3 with 10 bands present"""
    s, n = traces, traces.n
    for name, y, thr, max_gap, min_cols, max_bands, n_found, expect in dm.band_cases():
        full = np.full(n, 9.0, np.float32)						# above outside the window: only the window counts
        full[:y.size] = y
        s.plant(maxhold=full)
        rv, res, bands, _ = s.detect_raw(absolute_cfg(s, 1, 0, y.size, thr, max_gap, min_cols), max_bands, alloc=max_bands + 2)
        assert rv == 0 and (res["n_found"], res["n_written"]) == (n_found, len(expect)), name
        assert [(int(b["first"]), int(b["last"]), int(b["peak_col"])) for b in bands[:len(expect)]] == expect, name
        dm.assert_bands_equal(bands[:len(expect)], dm.bands(y, thr, max_gap, min_cols, max_bands)[1], tag=name)
        assert np.all(bands["first"][len(expect):] == SENTINEL), name
        assert same_f32(res["threshold_y"], thr) and res["floor_bin"] == -1 and np.isnan(res["floor_y"]), name
    y = np.full(n, -1.0, np.float32)
    starts = [0, 60, 64 * 7 - 1, n // 2 - 1, n // 2 + 200, n // 2 + 206, n - 300, n - 200, n - 100, n - 2]
    for k, c in enumerate(starts):
        y[c:c + 2] = 1.0 + k
    assert dm.bands(y, 0.0, 0, 1)[0] == 10
    s.plant(maxhold=y)
    rv, res, bands, _ = s.detect_raw(absolute_cfg(s, 1, 0, n, 0.0, 0, 1), 3, alloc=12)
    assert rv == 0 and (res["n_found"], res["n_written"]) == (10, 3)
    dm.assert_bands_equal(bands[:3], dm.bands(y, 0.0, 0, 1, 3)[1])
    assert np.all(bands.view(np.int32).reshape(-1)[15:] == SENTINEL)			# entry 3 onward untouched
    s.assert_untouched()
    s.plant(maxhold=s.maxhold)


# ---- floor ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log,bins", GEOMETRIES)
def test_floor_is_the_lower_median(amd, log, bins):
    s = Planted(amd, log, bins)
    n = s.n
    lib = amd._lib
    rng = np.random.default_rng(3)
    # in shifted column order: each valid column's mass in one bin, so every q gives that bin
    col_bin = rng.integers(bins // 4, bins // 2, n)
    col_bin[rng.integers(0, n, n // 8)] = bins - 1
    col_bin[0], col_bin[1] = 0, bins - 1
    empty = np.zeros(n, bool)
    empty[rng.integers(0, n, n // 5)] = True
    empty[n // 2 - 40:n // 2 + 40:3] = True
    h = np.zeros((bins, n), np.float32)
    i = np.flatnonzero(~empty)
    h[col_bin[i], i ^ (n // 2)] = 2.5						# shifted i is memory column i ^ (N/2)
    y = (s.table[0] - 1.0 - rng.random(n)).astype(np.float32)			# below every bin's y
    tone = s.table[bins - 1] + np.float32(1.0)					# above every threshold of the cases
    y[100:110] = tone; y[n // 2 - 3:n // 2 + 3] = tone + 1; y[n - 50:n - 45] = tone
    s.plant(hist=h, live=y)
    fbins = dm.percentile_bins(h, [0.5])[0]
    assert np.array_equal(fbins, np.where(empty, -1, col_bin))
    before = s.f.detect_stats()
    seen = set()
    margin = np.float32(0.37)
    windows = [(0, n), (0, n - 1), (3, 500), (3, 501), (n // 2 - 40, 81), (n // 2 - 38, 75), (n - 7, 7), (1, 1)]
    for first_bin, n_cols in windows:
        m = int((fbins[first_bin:first_bin + n_cols] >= 0).sum())
        seen.add(m % 2 if m else -1)
        want_res, want = dm.detect(y, first_bin, n_cols, 1, 2, 1024, floor_bins=fbins, table=s.table, margin_y=margin)
        cfg = lib.DetectCfg(0, first_bin, n_cols, 1, 0.5, margin, 123.0, 1, 2)
        rv, res, bands, _ = s.detect_raw(cfg, 1024)
        tag = "N=%d window=(%d, %d), %d valid columns" % (n, first_bin, n_cols, m)
        assert rv == 0, tag
        assert_result(res, want_res, tag)
        if m:
            assert same_f32(res["threshold_y"], s.table[res["floor_bin"]] + margin), tag
        dm.assert_bands_equal(bands[:res["n_written"]], want, tag=tag)
    assert seen >= {0, 1}, "an even and an odd number of valid columns"
    assert dm.detect(y, 0, n, 1, 2, 1024, floor_bins=fbins, table=s.table, margin_y=margin)[0]["n_found"] == 3
    after = s.f.detect_stats()
    assert [after[k] - before[k] for k in s.f.DETECT_STATS] == [len(windows)] * 3
    # a window of empty columns only, then a histogram of empty columns only
    e0 = n // 2 - 40
    assert fbins[e0] < 0
    for first_bin, n_cols, hist in [(e0, 1, None), (0, n, np.zeros((bins, n), np.float32))]:
        if hist is not None:
            s.plant(hist=hist)
        rv, res, bands, _ = s.detect_raw(lib.DetectCfg(0, first_bin, n_cols, 1, 0.5, margin, 0.0, 0, 1), 16)
        assert rv == 0 and (res["n_found"], res["n_written"], res["floor_bin"]) == (0, 0, -1)
        assert np.isnan(res["floor_y"]) and np.isnan(res["threshold_y"])
        assert np.all(bands["first"] == SENTINEL)
    s.assert_untouched()
    s.f.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------

E2E_TONES = (412, 612)		# shifted columns: -100 and +100 bins from DC, 200 columns apart


def e2e_input(call):
    """64 spectra of Gaussian noise (sigma 0.05 per component) and two tones on bin centres"""
    x = gaussian_iq(64 * 1024, 500 + call)
    for col in E2E_TONES:
        x = add_tone(x, 0.2, (col - 512) / 1024.0, phase0=0.3 * col, t0=call * 64 * 1024)
    return x


def test_end_to_end_two_tones(amd):
    """N = 1024, 128 bins, fp32: 4 calls of 64 spectra, then detect(live, floor_q 0.5, margin 15 dB, max_gap 2, min_cols 1).
    alpha is 0.05: with the reference's 0.002 the live line is an average over about 500 spectra that starts from the bottom of the
    power range, and after 256 spectra it has covered a third of the way to the spectrum, below the histogram's floor everywhere.
    Checked on the CPU with the oracle when this test was written (and again below, on every run): the model finds exactly the two
    bands, (411, 413) and (611, 613), peaks on the tones' columns; the tones stand 40.2 dB over the median live y; no column's live
    y is within 0.05 y of the threshold (the nearest is 0.62 y away; GPU floats are within 1e-4 of the oracle's); and the oracle's
    floor bin 59 is the median by a margin: 0.062 of the columns lie below it and 0.277 above, far from the 0.5 +- 0.02 of a tie."""
    import torch
    f = amd.Fosphor(n_bins=128, alpha=0.05)
    o = Oracle(n_bins=128)
    o.set_constants(16.0, 1024.0, 0.05)						# t0r, t0d: the defaults of both
    for call in range(4):
        x = e2e_input(call)
        d_x = torch.from_numpy(x).cuda()
        assert f.process_device(d_x, 1, 64) == 0
        assert f.finish() >= 0
        assert o.process(x) == 0
    table = dm.bin_y(128, o.histo_scale, o.histo_offset)
    assert same_f32(table, dm.bin_y(128, f.histo_scale, f.histo_offset))
    live = o.spectrum[0, :, 1]
    fbins = dm.percentile_bins(o.histogram, [0.5])[0]
    want_res, want = dm.detect(live, 0, 1024, 2, 1, 1024, floor_bins=fbins, table=table, margin_y=np.float32(15.0 / 20.0))
    # the margins the docstring states
    assert want_res["n_found"] == 2 and tuple(want["peak_col"]) == E2E_TONES
    assert np.all(np.abs(20.0 * (live[list(E2E_TONES)] - np.median(live)) - 40.0) < 1.0)
    assert np.min(np.abs(live - want_res["threshold_y"])) > 0.05
    valid = fbins[fbins >= 0]
    below, above = np.mean(valid < want_res["floor_bin"]), np.mean(valid > want_res["floor_bin"])
    assert below < 0.48 and above < 0.48 and valid.size == 1024

    res, bands = f.detect(trace="live", floor="percentile", floor_q=0.5, margin_db=15, max_gap=2, min_cols=1)
    print("floor bin %d (oracle %d), threshold %.4f (oracle %.4f), bands %s" % (res["floor_bin"], want_res["floor_bin"], res["threshold_y"],
                                                                                 want_res["threshold_y"], bands.tolist()))
    assert res["n_found"] == 2 and res["n_written"] == 2
    assert tuple(bands["peak_col"]) == E2E_TONES
    assert abs(res["floor_bin"] - want_res["floor_bin"]) <= 1
    assert np.array_equal(bands["first"], want["first"]) and np.array_equal(bands["last"], want["last"])
    assert np.allclose(bands["peak_y"], want["peak_y"], rtol=0, atol=1e-3) and np.allclose(bands["power_y"], want["power_y"], rtol=0, atol=1e-3)
    f.close()


# ---- argument errors -----------------------------------------------------------------------------------------------------

def test_detect_argument_errors(traces):
    import torch
    s, n = traces, traces.n
    lib = s.lib
    nan = float("nan")
    good = dict(trace=0, first_bin=10, n_cols=500, floor_mode=1, floor_q=0.5, margin_y=0.5, threshold_y=0.0, max_gap=1, min_cols=1)
    bad = [dict(trace=2), dict(trace=-1), dict(floor_mode=2), dict(floor_mode=-1),
           dict(first_bin=-1), dict(first_bin=n), dict(n_cols=0), dict(n_cols=n - 9), dict(first_bin=0, n_cols=n + 1),
           dict(min_cols=0), dict(min_cols=-4), dict(max_gap=-1),
           dict(floor_q=0.0), dict(floor_q=1.5), dict(floor_q=nan), dict(floor_q=-0.1)]
    for change in bad:
        kw = dict(good, **change)
        rv, res, bands, raw = s.detect_raw(lib.DetectCfg(*[kw[k] for k, _ in lib.DetectCfg._fields_]), 8)
        assert rv == -errno.EINVAL, change
        assert np.all(raw == SENTINEL) and np.all(bands["first"] == SENTINEL), change
    cfg = lib.DetectCfg(*[good[k] for k, _ in lib.DetectCfg._fields_])
    for max_bands in (0, -1, 65537):
        rv, res, bands, raw = s.detect_raw(cfg, max_bands, alloc=8)
        assert rv == -errno.EINVAL and np.all(raw == SENTINEL) and np.all(bands["first"] == SENTINEL), max_bands
    rv, res, bands, raw = s.detect_raw(None, 8)
    assert rv == -errno.EINVAL and np.all(raw == SENTINEL)
    d = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert s.f.L.fosphor_amd_detect(s.f.h, C.byref(cfg), None, d.data_ptr(), 8) == -errno.EINVAL
    assert s.f.L.fosphor_amd_detect(s.f.h, C.byref(cfg), d.data_ptr(), None, 8) == -errno.EINVAL
    assert bool((d == SENTINEL).all())
    rv, res, bands, raw = s.detect_raw(cfg, 8)						# and the good one is good
    assert rv == 0 and res["n_written"] <= 8
    with pytest.raises(ValueError):
        s.f.detect(trace="average")
    with pytest.raises(ValueError):
        s.f.detect(floor="median")
    with pytest.raises(RuntimeError):
        s.f.detect(min_cols=0)
    with pytest.raises(RuntimeError):
        s.f.detect(max_bands=0)
    with pytest.raises(RuntimeError):
        s.f.detect(first_bin=5, n_cols=n)
    s.assert_untouched()
