"""CPU statement of a view (include/fosphor_amd_view.h) in plain numpy: the span rule, the fft-shift, the ring order, both
detectors and a float32 restatement of the palette lookup.  AVERAGE is computed in float64.

The sources are the arrays the Fosphor properties return:
    waterfall [wf_rows][N]   unshifted columns, ring in rows
    histogram [n_bins][N]    unshifted columns, row 0 = lowest dB bin
    spectrum  [2][N][2]      live then max-hold vertices (x, y), already shifted
"""
import numpy as np

PEAK, AVERAGE = 0, 1


# ---- pixel-to-cell mapping ---------------------------------------------------

def span(n_src, n_out, p):
    """[lo, hi) of n_src that output index p of n_out covers (Python integers: no overflow)"""
    lo = (p * n_src) // n_out
    hi = max(lo + 1, ((p + 1) * n_src) // n_out)
    return lo, hi


def spans(n_src, n_out):
    """lo[n_out], hi[n_out] as int64 arrays"""
    p = np.arange(n_out, dtype=np.int64)
    lo = (p * n_src) // n_out
    hi = np.maximum(lo + 1, ((p + 1) * n_src) // n_out)
    return lo, hi


# ---- source coordinates ------------------------------------------------------

def window_columns(n, first_bin, n_cols):
    """memory columns of the shifted columns first_bin .. first_bin + n_cols - 1"""
    return (first_bin + np.arange(n_cols)) ^ (n // 2)


def ring_rows(wf_rows, pos, count):
    """ring rows of the `count` newest waterfall rows, newest first"""
    return (pos - 1 - np.arange(count)) % wf_rows


# ---- detectors ---------------------------------------------------------------

def reduce_axis(a, n_out, axis, op):
    """op.reduce over the spans of `axis` -> n_out entries along it.  ufunc.reduceat over the lower ends is the span rule: spans
    that tile end where the next begins, and a lower end that repeats (n_src < n_out) yields that one cell again."""
    lo, hi = spans(a.shape[axis], n_out)
    assert np.all(hi[:-1] == np.maximum(lo[1:], lo[:-1] + 1)) and hi[-1] == a.shape[axis]
    return op.reduceat(a, lo, axis=axis)


def reduce_naive(a, out_rows, out_cols, detector):
    """the same by explicit loops (small arrays: the check of reduce_block)"""
    out = np.empty((out_rows, out_cols), np.float32 if detector == PEAK else np.float64)
    for r in range(out_rows):
        rl, rh = span(a.shape[0], out_rows, r)
        for c in range(out_cols):
            cl, ch = span(a.shape[1], out_cols, c)
            blk = a[rl:rh, cl:ch].reshape(-1)
            out[r, c] = np.fmax.reduce(blk) if detector == PEAK else np.add.reduce(blk.astype(np.float64)) / blk.size
    return out


def reduce_block(a, out_rows, out_cols, detector):
    """a: float32 [src_rows][src_cols] in source order -> [out_rows][out_cols].
    PEAK: float32, np.fmax.reduce over each block (NaN ignored unless the whole block is NaN).
    AVERAGE: (mean, mean of |cell|, cell count) in float64."""
    a = np.asarray(a, np.float32)
    with np.errstate(all="ignore"):
        if detector == PEAK:
            return reduce_axis(reduce_axis(a, out_cols, 1, np.fmax), out_rows, 0, np.fmax)
        rl, rh = spans(a.shape[0], out_rows)
        cl, ch = spans(a.shape[1], out_cols)
        count = np.outer(rh - rl, ch - cl).astype(np.float64)
        a64 = a.astype(np.float64)
        total = reduce_axis(reduce_axis(a64, out_cols, 1, np.add), out_rows, 0, np.add)
        total_abs = reduce_axis(reduce_axis(np.abs(a64), out_cols, 1, np.add), out_rows, 0, np.add)
        return total / count, total_abs / count, count


def view(waterfall, histogram, spectrum, pos, first_bin, n_cols, width, wf_src_rows, wf_out_rows, detector,
         what=("waterfall", "histogram", "live", "max")):
    """dict of the float pictures `what` of a view; entries as reduce_block returns them"""
    n = histogram.shape[1]
    cols = window_columns(n, first_bin, n_cols)
    out = {}
    if "waterfall" in what:
        rows = ring_rows(waterfall.shape[0], pos, wf_src_rows)
        out["waterfall"] = reduce_block(waterfall[rows][:, cols], wf_out_rows, width, detector)
    if "histogram" in what:
        out["histogram"] = reduce_block(histogram[::-1][:, cols], histogram.shape[0], width, detector)
    for name, line in (("live", spectrum[0, :, 1]), ("max", spectrum[1, :, 1])):
        if name in what:
            res = reduce_block(line[None, first_bin:first_bin + n_cols], 1, width, detector)
            out[name] = res[0] if detector == PEAK else tuple(x[0] for x in res)
    return out


def average_bound(mean, mean_abs, count):
    """|float32 result - mean| allowed for a span of `count` cells: count * 2^-24 * mean(|x|) for summing count float32 values in
    any order + 2^-23 * |mean| for the reciprocal multiply and the final rounding"""
    return count * 2.0 ** -24 * mean_abs + 2.0 ** -23 * np.abs(mean)


# ---- palette lookup ----------------------------------------------------------

def lookup(t, pal, scale, offset):
    """uint32 RGBA of float32 intensities: fosphor_amd_colorize's lookup, every operation in float32"""
    f32 = np.float32
    t = np.asarray(t, f32)
    pal = np.asarray(pal, np.uint32)
    n = pal.size
    with np.errstate(all="ignore"):
        m = (t + f32(offset)) * f32(scale)
        u = m * f32(n) - f32(0.5)
        u = np.where(np.isnan(u), f32(-1.0), u).astype(f32)
        u = np.minimum(np.maximum(u, f32(-1.0)), f32(n))
        fl = np.floor(u)
        f = u - fl
        i0 = np.clip(fl.astype(np.int64), 0, n - 1)
        i1 = np.clip(fl.astype(np.int64) + 1, 0, n - 1)
        a, b = pal[i0], pal[i1]
        out = np.zeros(t.shape, np.uint32)
        for ch in range(4):
            c0 = ((a >> np.uint32(8 * ch)) & np.uint32(0xff)).astype(f32)
            c1 = ((b >> np.uint32(8 * ch)) & np.uint32(0xff)).astype(f32)
            c = c0 + f * (c1 - c0)
            assert c.dtype == f32
            out |= ((c + f32(0.5)).astype(np.uint32) & np.uint32(0xff)) << np.uint32(8 * ch)
    return out
