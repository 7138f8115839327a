"""numpy statement of include/fosphor_amd_mask.h: the row rule, the trigger and the event list, channel power in fp64, limit lines
from a trace and from points.  Written from the definitions, not from the kernels; tests/test_mask_cpu.py and
tests/test_gpu_mask.py compare the library against it."""
import numpy as np

F32 = np.float32
ROW_DTYPE = np.dtype([("n_over", "<i4"), ("n_under", "<i4"), ("first_col", "<i4"), ("last_col", "<i4"),
                      ("peak_col", "<i4"), ("peak_over", "<f4")])
RESULT_DTYPE = np.dtype([("n_triggered", "<i4"), ("n_written", "<i4"), ("newest", "<i4"), ("oldest", "<i4")])
CHANNEL_DTYPE = np.dtype([("first", "<i4"), ("last", "<i4")])
CFG_DTYPE = np.dtype([("first_bin", "<i4"), ("n_cols", "<i4"), ("rows", "<i4"), ("min_cols", "<i4"), ("n_channels", "<i4"),
                      ("channels", CHANNEL_DTYPE, (8,))])


def shift(a):
    """memory column order -> fft-shifted order along the last axis: shifted i is memory i ^ (N/2)"""
    n = a.shape[-1]
    return a[..., np.arange(n) ^ (n // 2)]


def newest_first(wf, pos):
    """the ring [wf_rows][N] in memory order -> rows by source index j (0 = newest: ring row (pos - 1 - j) mod wf_rows), shifted"""
    rows = wf.shape[0]
    return shift(wf[(pos - 1 - np.arange(rows)) % rows])


def row_rule(y, upper=None, lower=None, first_bin=0):
    """one record for a row y[n] against limits [n] (None: never violated); columns are first_bin + the index into y"""
    y = np.asarray(y, dtype=F32)
    with np.errstate(invalid="ignore"):
        over = y > np.asarray(upper, F32) if upper is not None else np.zeros(y.size, bool)	# a NaN on either side: False
        under = y < np.asarray(lower, F32) if lower is not None else np.zeros(y.size, bool)
    out = np.zeros((), ROW_DTYPE)
    out["n_over"], out["n_under"] = int(over.sum()), int(under.sum())
    viol = np.flatnonzero(over | under)
    out["first_col"] = first_bin + int(viol[0]) if viol.size else -1
    out["last_col"] = first_bin + int(viol[-1]) if viol.size else -1
    if over.any():
        idx = np.flatnonzero(over)
        with np.errstate(over="ignore", invalid="ignore"):
            ex = (y[idx] - np.asarray(upper, F32)[idx]).astype(F32)			# one float32 subtraction
        assert not np.isnan(ex).any()
        best = ex.max()
        out["peak_col"] = first_bin + int(idx[np.flatnonzero(ex == best)[0]])		# the lowest column of equal excesses
        out["peak_over"] = best
    else:
        out["peak_col"], out["peak_over"] = -1, np.nan
    return out


def rows_rule(ys, upper, lower, first_bin, n_cols):
    """records for ys[rows][N] (shifted, j order) over the window; upper / lower [N] shifted or None"""
    sl = slice(first_bin, first_bin + n_cols)
    out = np.zeros(ys.shape[0], ROW_DTYPE)
    for j in range(ys.shape[0]):
        out[j] = row_rule(ys[j, sl], None if upper is None else upper[sl], None if lower is None else lower[sl], first_bin)
    return out


def events(rows, min_cols, max_events):
    """(result record, the first max_events triggered j in ascending order)"""
    trig = np.flatnonzero(rows["n_over"] + rows["n_under"] >= min_cols).astype(np.int32)
    res = np.zeros((), RESULT_DTYPE)
    res["n_triggered"] = trig.size
    res["n_written"] = min(trig.size, max_events)
    res["newest"] = trig[0] if trig.size else -1
    res["oldest"] = trig[-1] if trig.size else -1
    return res, trig[:max_events]


def channel_power(ys, channels):
    """float32 [n_channels][rows]: 0.5 * log10 of the fp64 sum of the finite 10^(2 y) over the columns first .. last"""
    out = np.zeros((len(channels), ys.shape[0]), F32)
    for c, (a, b) in enumerate(channels):
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            t = np.power(10.0, 2.0 * ys[:, a:b + 1].astype(np.float64))
            t = np.where(np.isfinite(t), t, 0.0)
            out[c] = (0.5 * np.log10(t.sum(axis=1))).astype(F32)
    return out


def power_error(got, want):
    """worst |got - want|, equal infinities counting as 0; inf where one side alone is not finite"""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        err = np.where(g == w, 0.0, np.abs(g - w))
    err = np.where(np.isnan(err), np.inf, err)
    return float(err.max()) if err.size else 0.0


def from_trace(trace_y, margin_y, spread):
    """out[i] = fmax over [i - spread, i + spread] (clipped) of trace_y, + margin_y, in float32"""
    y = np.asarray(trace_y, F32)
    n = y.size
    pad = np.full(n + 2 * spread, np.nan, F32)
    pad[spread:spread + n] = y
    m = np.full(n, np.nan, F32)
    for k in range(2 * spread + 1):
        m = np.fmax(m, pad[k:k + n])
    return (m + F32(margin_y)).astype(F32)


def from_points(n, col, y):
    """the piecewise-linear limit line of fosphor_amd_mask_from_points, the expression in double as the header writes it"""
    col = np.asarray(col, np.float64)
    y = np.asarray(y, F32)
    out = np.zeros(n, F32)
    for i in range(n):
        x = np.float64(i)
        if x <= col[0]:
            out[i] = y[0]
        elif x >= col[-1]:
            out[i] = y[-1]
        else:
            k = int(np.searchsorted(col, x, side="right")) - 1			# col[k] <= x < col[k + 1]
            c0, c1, y0, y1 = col[k], col[k + 1], np.float64(y[k]), np.float64(y[k + 1])
            with np.errstate(all="ignore"):
                out[i] = F32(y0 + (y1 - y0) * ((x - c0) / (c1 - c0)))
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def assert_rows_equal(got, want, tag=""):
    """every integer exactly, peak_over bit for bit (every NaN is the same NaN to this check)"""
    assert len(got) == len(want), (tag, len(got), len(want))
    for k in ("n_over", "n_under", "first_col", "last_col", "peak_col"):
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (tag, k, "row", int(bad[0]), int(got[k][bad[0]]), int(want[k][bad[0]]))
    g, w = got["peak_over"], want["peak_over"]
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), (tag, "peak_over NaN")
    assert np.array_equal(g[~nan].view(np.uint32), w[~nan].view(np.uint32)), (tag, "peak_over")


def row_cases():
    """The fixed cases of the row rule: (name, y, upper, lower, (n_over, n_under, first_col, last_col, peak_col, peak_over)) with
    the expectation worked out by hand; limits None = NULL."""
    N, I = np.nan, np.inf
    f = lambda *v: np.array(v, dtype=F32)
    return [
        ("no violation", f(0, 1, 2, 1), f(3, 3, 3, 3), f(-1, -1, -1, -1), (0, 0, -1, -1, -1, N)),
        ("only column 0", f(5, 1, 1, 1), f(3, 3, 3, 3), f(-1, -1, -1, -1), (1, 0, 0, 0, 0, 2.0)),
        ("only column n-1", f(1, 1, 1, -4), f(3, 3, 3, 3), f(-1, -1, -1, -1), (0, 1, 3, 3, -1, N)),
        ("over / under mix", f(-2, 4, 0, 7, -3), f(3, 3, 3, 3, 3), f(-1, -1, -1, -1, -1), (2, 2, 0, 4, 3, 4.0)),
        ("tie of the excess", f(0, 5, 5, 6, 0), f(3, 3, 3, 4, 3), None, (3, 0, 1, 3, 1, 2.0)),
        ("+inf excess", f(0, 4, I, I), f(3, 3, 3, 3), None, (3, 0, 1, 3, 2, I)),
        ("+inf y against a +inf limit", f(I, 4), f(I, 3), None, (1, 0, 1, 1, 1, 1.0)),
        ("NaN y", f(N, 9, N), f(3, 3, 3), f(5, 5, 5), (1, 0, 1, 1, 1, 6.0)),
        ("NaN limit", f(9, 9, -9), f(N, 3, 3), f(-1, -1, N), (1, 0, 1, 1, 1, 6.0)),
        ("-inf against a lower limit", f(-I, 0, -I), None, f(-5, -5, -I), (0, 1, 0, 0, -1, N)),
        ("equal to the limits", f(3, -1, 3), f(3, 3, 3), f(-1, -1, 3), (0, 0, -1, -1, -1, N)),
        ("both limits NULL", f(9, -9, N), None, None, (0, 0, -1, -1, -1, N)),
    ]
