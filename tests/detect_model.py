"""numpy statement of include/fosphor_amd_detect.h: percentile traces of the persistence histogram, the noise floor, the mask / gap /
band rules and the per-band numbers.  Written from the definitions, not from the kernels; tests/test_detect_cpu.py and
tests/test_gpu_detect.py compare the library against it."""
import numpy as np

F32 = np.float32
BAND_DTYPE = np.dtype([("first", "<i4"), ("last", "<i4"), ("peak_col", "<i4"), ("peak_y", "<f4"), ("power_y", "<f4")])


def bin_y(n_bins, histo_scale, histo_offset):
    """y of each bin: (float)b / histo_scale - histo_offset, every step in float32"""
    return (np.arange(n_bins, dtype=F32) / F32(histo_scale) - F32(histo_offset)).astype(F32)


def shift(a):
    """memory column order -> fft-shifted order along the last axis: shifted i is memory i ^ (N/2)"""
    n = a.shape[-1]
    return a[..., np.arange(n) ^ (n // 2)]


def percentile_bins(hist, q):
    """hist: float32 [n_bins][N] in memory column order; q: percentiles in ]0, 1].  int32 [n_q][N] in shifted order.
    The prefix sum is sequential in float32 (np.cumsum accumulates in order); the threshold is the float32 product q * T."""
    hist = np.asarray(hist, dtype=F32)
    c = np.cumsum(hist, axis=0, dtype=F32)
    total = c[-1]
    some = total > 0
    out = np.empty((len(q), hist.shape[1]), np.int32)
    for k, qk in enumerate(q):
        thr = F32(qk) * total					# float32 * float32 array: rounded once
        assert thr.dtype == F32
        b = np.argmax(c >= thr[None, :], axis=0)		# the first True
        out[k] = np.where(some, b, -1)
    return shift(out)


def percentile_y(bins, table):
    return np.where(bins >= 0, table[np.maximum(bins, 0)], F32(np.nan)).astype(F32)


def floor_bin(bins):
    """lower median of the bins that are >= 0: element (m - 1) // 2 of them sorted; -1 when there is none"""
    v = np.sort(bins[bins >= 0])
    return int(v[(v.size - 1) // 2]) if v.size else -1


def closed_mask(y, threshold_y, max_gap):
    above = np.asarray(y, dtype=F32) > F32(threshold_y)		# NaN on either side: False
    m = above.copy()
    idx = np.flatnonzero(above)
    for a, b in zip(idx[:-1], idx[1:]):				# consecutive above columns: the run between them has one on both sides
        if 0 < b - a - 1 <= max_gap:
            m[a + 1:b] = True
    return m


def bands(y, threshold_y, max_gap, min_cols, max_bands=None, first_bin=0):
    """(n_found, structured array of the first max_bands bands); columns are first_bin + the index into y"""
    y = np.asarray(y, dtype=F32)
    m = closed_mask(y, threshold_y, max_gap)
    edges = np.diff(np.concatenate(([0], m.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(edges == 1), np.flatnonzero(edges == -1) - 1
    keep = ends - starts + 1 >= min_cols
    starts, ends = starts[keep], ends[keep]
    n_found = int(starts.size)
    n_out = n_found if max_bands is None else min(n_found, max_bands)
    out = np.zeros(n_out, BAND_DTYPE)
    for k in range(n_out):
        s, e = int(starts[k]), int(ends[k])
        seg = y[s:e + 1]
        ok = ~np.isnan(seg)
        peak = np.max(seg[ok])
        col = s + int(np.flatnonzero(ok & (seg == peak))[0])	# the lowest column attaining the maximum
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            terms = np.power(10.0, 2.0 * seg.astype(np.float64))
            power = 0.5 * np.log10(np.sum(terms[np.isfinite(terms)]))
        out[k] = (first_bin + s, first_bin + e, first_bin + col, y[col], F32(power))
    return n_found, out


def detect(trace_y, first_bin, n_cols, max_gap, min_cols, max_bands, threshold_y=None, floor_bins=None, table=None, margin_y=0.0):
    """The whole of fosphor_amd_detect on host arrays.  trace_y: [N] shifted.  ABSOLUTE: threshold_y.  PERCENTILE: floor_bins, the
    [N] shifted floor_q bins of percentile_bins, table and margin_y.  Returns (result dict, bands)."""
    if floor_bins is not None:
        fb = floor_bin(floor_bins[first_bin:first_bin + n_cols])
        fy = table[fb] if fb >= 0 else F32(np.nan)
        thr = F32(fy) + F32(margin_y)
    else:
        fb, fy, thr = -1, F32(np.nan), F32(threshold_y)
    n_found, b = bands(trace_y[first_bin:first_bin + n_cols], thr, max_gap, min_cols, max_bands, first_bin)
    return dict(n_found=n_found, n_written=len(b), floor_bin=fb, floor_y=F32(fy), threshold_y=F32(thr)), b


def assert_bands_equal(got, want, power_tol=5e-5, tag=""):
    """every integer and peak_y exactly, power_y within power_tol (equal infinities pass)"""
    assert len(got) == len(want), (tag, len(got), len(want))
    for k in ("first", "last", "peak_col"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k][:8], want[k][:8])
    assert np.array_equal(got["peak_y"].view(np.uint32), want["peak_y"].view(np.uint32)), (tag, "peak_y")
    g, w = got["power_y"].astype(np.float64), want["power_y"].astype(np.float64)
    same = (g == w)
    with np.errstate(invalid="ignore"):
        err = np.where(same, 0.0, np.abs(g - w))
    assert np.all(err <= power_tol), (tag, "power_y", float(np.nanmax(err)) if err.size else 0.0)
    return float(err.max()) if err.size else 0.0


def band_cases():
    """The fixed cases of the band rules: (name, trace, threshold, max_gap, min_cols, max_bands, n_found, [(first, last, peak_col)])
    with the expected bands worked out by hand.  H is above the threshold 0, L below, N is NaN."""
    H, L, N = 1.0, -1.0, np.nan
    f = lambda *v: np.array(v, dtype=F32)
    return [
        ("nothing above", f(L, L, L, L, L), 0.0, 2, 1, 8, 0, []),
        ("nothing above, all NaN", f(N, N, N), 0.0, 2, 1, 8, 0, []),
        ("everything above", f(H, 2, H, H), 0.0, 0, 1, 8, 1, [(0, 3, 1)]),
        ("one column, above", f(H), 0.0, 3, 1, 8, 1, [(0, 0, 0)]),
        ("bands at column 0 and n-1", f(H, L, L, L, 3), 0.0, 2, 1, 8, 2, [(0, 0, 0), (4, 4, 4)]),
        ("gap of max_gap is closed", f(L, H, H, L, L, 2, L), 0.0, 2, 1, 8, 1, [(1, 5, 5)]),
        ("gap of max_gap + 1 is not", f(L, H, H, L, L, L, 2, L), 0.0, 2, 1, 8, 2, [(1, 2, 1), (6, 6, 6)]),
        ("max_gap 0 closes nothing", f(H, L, H), 0.0, 0, 1, 8, 2, [(0, 0, 0), (2, 2, 2)]),
        ("gaps touching both edges stay", f(L, L, H, H, L, L), 0.0, 2, 1, 8, 1, [(2, 3, 2)]),
        ("gap at the left edge only", f(L, H, L, H), 0.0, 5, 1, 8, 1, [(1, 3, 1)]),
        ("run of min_cols - 1 dropped, min_cols kept", f(H, H, L, L, L, L, H, 2, H), 0.0, 0, 3, 8, 1, [(6, 8, 7)]),
        ("min_cols reached only through closing", f(L, H, L, 2, L, L), 0.0, 1, 3, 8, 1, [(1, 3, 3)]),
        ("... and not without", f(L, H, L, 2, L, L), 0.0, 0, 2, 8, 0, []),
        ("NaN inside a band is a gap", f(L, H, N, 3, N, N, H, L), 0.0, 2, 1, 8, 1, [(1, 6, 3)]),
        ("NaN splits when gaps stay open", f(H, N, 2), 0.0, 0, 1, 8, 2, [(0, 0, 0), (2, 2, 2)]),
        ("equal maxima: the lowest column", f(L, 2, 5, 5, 3, 5, L), 0.0, 0, 1, 8, 1, [(1, 5, 2)]),
        ("equal maxima across a closed gap", f(4, L, 4), 0.0, 1, 1, 8, 1, [(0, 2, 0)]),
        ("a column equal to the threshold is not above", f(0, H, 0), 0.0, 0, 1, 8, 1, [(1, 1, 1)]),
        ("max_bands below n_found", f(H, L, H, L, H, L, H, L, H), 0.0, 0, 1, 3, 5, [(0, 0, 0), (2, 2, 2), (4, 4, 4)]),
        ("NaN threshold", f(H, H, H), np.nan, 0, 1, 8, 0, []),
    ]
