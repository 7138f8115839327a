"""Views (include/fosphor_amd_view.h), the part that needs no GPU: the exported span rule, the window a struct fosphor_render
selects, and the numpy statement of a view (tests/view_ref.py) tied to the existing colour-map checker."""
import ctypes as C
import errno
import os

import numpy as np
import pytest

import view_ref
from oracle_lib import ORACLE_SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cmap_palettes.npz"))


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


@pytest.fixture(scope="module")
def oracle(oracle_built):
    """loaded as tests/test_cmap.py loads it"""
    L = C.CDLL(ORACLE_SO)
    L.fosphor_oracle_colorize.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                          C.c_float, C.c_float, C.c_int, C.c_void_p]
    return L


SIZES = [1, 2, 3, 7, 13, 64, 97, 100, 333, 640, 1000, 1021, 1024, 1920, 8192, 65521, 65536]
GRID = [(s, o) for s in SIZES for o in SIZES if s * o <= 1024 * 8192] + [(65536, 1), (65536, 1920), (65536, 3840), (65536, 65536),
                                                                         (1, 65536), (100, 65536), (65521, 65536)]


@pytest.mark.parametrize("n_src,n_out", GRID)
def test_span_rule(amd, n_src, n_out):
    L = amd.load()
    lo_ref, hi_ref = view_ref.spans(n_src, n_out)
    lo, hi = C.c_int(), C.c_int()
    ps = range(n_out) if n_out <= 4096 else list(range(0, n_out, 37)) + [n_out - 2, n_out - 1]
    for p in ps:
        assert L.fosphor_amd_view_span(n_src, n_out, p, C.byref(lo), C.byref(hi)) == 0
        assert (lo.value, hi.value) == (lo_ref[p], hi_ref[p]) == view_ref.span(n_src, n_out, p), p
    assert np.all(hi_ref > lo_ref) and lo_ref[0] == 0 and hi_ref[-1] == n_src
    if n_src >= n_out:						# the spans tile [0, n_src)
        assert np.array_equal(hi_ref[:-1], lo_ref[1:])
    else:							# one cell per pixel, nearest, repeated
        assert np.all(hi_ref - lo_ref == 1) and np.all(np.diff(lo_ref) >= 0) and np.all(np.diff(lo_ref) <= 1)
        assert len(np.unique(lo_ref)) == n_src


def test_span_argument_errors(amd):
    L = amd.load()
    lo, hi = C.c_int(-7), C.c_int(-7)
    for n_src, n_out, p in [(0, 4, 0), (4, 0, 0), (-1, 4, 0), (4, 4, -1), (4, 4, 4), (65536, 1, 1)]:
        assert L.fosphor_amd_view_span(n_src, n_out, p, C.byref(lo), C.byref(hi)) == -errno.EINVAL
    assert L.fosphor_amd_view_span(4, 4, 0, None, C.byref(hi)) == -errno.EINVAL
    assert L.fosphor_amd_view_span(4, 4, 0, C.byref(lo), None) == -errno.EINVAL
    assert (lo.value, hi.value) == (-7, -7)


def render(amd, center=None, span=None, wf_span=None):
    r = amd._lib.Render()
    amd.load().fosphor_render_defaults(C.byref(r))
    if center is not None:
        r.freq_center = center
    if span is not None:
        r.freq_span = span
    if wf_span is not None:
        r.wf_span = wf_span
    return r


def from_render(amd, n, wf_rows, r, width, wf_out_rows):
    v = amd._lib.View()
    rv = amd.load().fosphor_amd_view_from_render(n, wf_rows, C.byref(r), width, wf_out_rows, C.byref(v))
    return rv, v


@pytest.mark.parametrize("log", [10, 13, 16])
def test_view_from_render_defaults_give_the_whole_buffer(amd, log):
    n = 1 << log
    r = render(amd)
    assert (r.freq_center, r.freq_span, r.wf_span) == (0.5, 1.0, 1.0)
    rv, v = from_render(amd, n, 1024, r, 1920, 512)
    assert rv == 0
    assert (v.first_bin, v.n_cols, v.wf_src_rows) == (0, n, 1024)
    assert (v.width, v.wf_out_rows, v.detector) == (1920, 512, view_ref.PEAK)


ZOOMS = [(0.5, 0.2, 1.0),		# the demo's zoom (main.c: zoom_center 0.5, zoom_width 0.2)
         (0.5, 1.0, 1.0), (0.5, 0.5, 0.5), (0.25, 0.5, 0.25), (0.75, 0.5, 1.0),	# touching the left / the right edge
         (0.1, 0.2, 0.3), (0.9, 0.2, 0.01), (0.05, 0.2, 1.0), (0.97, 0.2, 1.0),	# hanging over an edge: clamped
         (0.3333, 0.1234, 0.777), (0.5, 1e-6, 1e-6), (0.999, 0.001, 0.5), (0.6180339, 0.0314159, 0.2718)]


@pytest.mark.parametrize("log", [10, 13, 16])
@pytest.mark.parametrize("center,span,wf_span", ZOOMS)
def test_view_from_render_zooms(amd, log, center, span, wf_span):
    n, wf_rows = 1 << log, 1024 if log == 10 else 512
    r = render(amd, center, span, wf_span)
    fc, fs, ws = float(r.freq_center), float(r.freq_span), float(r.wf_span)	# the float fields, widened to double
    first = int(min(max(np.floor(0.5 + n * (fc - fs / 2)), 0), n - 1))
    cols = int(min(max(round(n * fs), 1), n - first))				# round(): to nearest, ties to even, as lrint
    rows = int(min(max(round(wf_rows * ws), 1), wf_rows))
    rv, v = from_render(amd, n, wf_rows, r, 640, 300)
    assert rv == 0
    assert (v.first_bin, v.n_cols, v.wf_src_rows) == (first, cols, rows)
    assert (v.width, v.wf_out_rows, v.detector) == (640, 300, view_ref.PEAK)
    assert 0 <= v.first_bin < n and 1 <= v.n_cols <= n - v.first_bin and 1 <= v.wf_src_rows <= wf_rows


def test_view_from_render_demo_zoom_values(amd):
    """the demo's second render at 1024 points: 0.2 of the span around the centre"""
    rv, v = from_render(amd, 1024, 1024, render(amd, 0.5, 0.2), 640, 300)
    assert rv == 0 and (v.first_bin, v.n_cols, v.wf_src_rows) == (410, 205, 1024)
    rv, v = from_render(amd, 65536, 1024, render(amd, 0.25, 0.5), 640, 300)
    assert rv == 0 and (v.first_bin, v.n_cols) == (0, 32768)
    rv, v = from_render(amd, 65536, 1024, render(amd, 0.75, 0.5), 640, 300)
    assert rv == 0 and (v.first_bin, v.n_cols) == (32768, 32768)


def test_view_from_render_argument_errors(amd):
    L = amd.load()
    bad = [render(amd, span=0.0), render(amd, span=-0.5), render(amd, span=1.5), render(amd, span=float("nan")),
           render(amd, center=0.0), render(amd, center=1.0), render(amd, center=-0.1), render(amd, center=float("nan")),
           render(amd, wf_span=0.0), render(amd, wf_span=1.01), render(amd, wf_span=float("nan"))]
    for r in bad:
        assert from_render(amd, 1024, 1024, r, 640, 300)[0] == -errno.EINVAL
    ok = render(amd)
    for n, wf_rows, width, out_rows in [(0, 1024, 640, 300), (-1024, 1024, 640, 300), (1024, 0, 640, 1), (1024, 1024, 0, 300),
                                        (1024, 1024, 65537, 300), (1024, 1024, 640, 0), (1024, 1024, 640, 1025)]:
        assert from_render(amd, n, wf_rows, ok, width, out_rows)[0] == -errno.EINVAL
    v = amd._lib.View()
    assert L.fosphor_amd_view_from_render(1024, 1024, None, 640, 300, C.byref(v)) == -errno.EINVAL
    assert L.fosphor_amd_view_from_render(1024, 1024, C.byref(ok), 640, 300, None) == -errno.EINVAL
    assert from_render(amd, 1024, 1024, ok, 65536, 1024)[0] == 0


def test_view_entry_refuses_null_without_a_device(amd):
    L = amd.load()
    v, o = amd._lib.View(0, 1024, 1024, 1, 1, 0), amd._lib.ViewOut()
    assert L.fosphor_amd_view(None, C.byref(v), C.byref(o)) == -errno.EINVAL
    assert L.fosphor_amd_view_stats(None, None) == -errno.EINVAL


def random_state(rng, rows, n):
    a = (rng.standard_normal((rows, n)) * 2.0 - 1.0).astype(np.float32)		# well outside the palette's [0, 1] on both sides
    k = rng.integers(0, a.size, 200)
    a.reshape(-1)[k[:50]] = np.nan
    a.reshape(-1)[k[50:100]] = np.inf
    a.reshape(-1)[k[100:150]] = -np.inf
    a.reshape(-1)[k[150:]] = 0.0
    return a


@pytest.mark.parametrize("n,wf_rows,bins,pos", [(1024, 64, 128, 17), (8192, 16, 32, 0)])
def test_reference_identity_view_is_the_oracle_picture(oracle, n, wf_rows, bins, pos):
    """identity view (first_bin 0, n_cols = width = N, every row, PEAK) + view_ref.lookup == fosphor_oracle_colorize, both images"""
    rng = np.random.default_rng(n + pos)
    wf, hist = random_state(rng, wf_rows, n), random_state(rng, bins, n)
    spec = rng.standard_normal((2, n, 2)).astype(np.float32)
    got = view_ref.view(wf, hist, spec, pos, 0, n, n, wf_rows, wf_rows, view_ref.PEAK)
    assert np.array_equal(got["live"], spec[0, :, 1]) and np.array_equal(got["max"], spec[1, :, 1])
    for image, src, key, rows, opos in ((0, wf, "waterfall", wf_rows, pos), (1, hist, "histogram", bins, 0)):
        for pal, scale, offset in ((GOLD["waterfall_256"], 0.2, 1.99), (GOLD["histogram_256"], 1.1, 0.0), (GOLD["prog_1000"], 0.37, 2.5),
                                   (GOLD["waterfall_64"], 3.0, -0.01)):
            want = np.zeros((rows, n), np.uint32)
            assert oracle.fosphor_oracle_colorize(image, src.ctypes.data, rows, n, opos, pal.ctypes.data, pal.size, scale, offset,
                                                  rows, want.ctypes.data) == 0
            assert np.array_equal(view_ref.lookup(got[key], pal, scale, offset), want), (key, pal.size)
        assert np.isnan(got[key]).sum() == np.isnan(src).sum()


@pytest.mark.parametrize("detector", [view_ref.PEAK, view_ref.AVERAGE])
def test_reference_block_reduction_equals_explicit_loops(detector):
    rng = np.random.default_rng(5)
    for rows, cols, out_rows, out_cols in [(7, 50, 3, 11), (5, 13, 5, 13), (4, 9, 9, 31), (16, 64, 1, 1), (1, 1, 3, 5), (9, 100, 4, 100)]:
        a = random_state(rng, rows, cols) if detector == view_ref.PEAK else rng.standard_normal((rows, cols)).astype(np.float32)
        if detector == view_ref.PEAK:
            a[0, :3] = np.nan					# a block of NaN only stays NaN
        want = view_ref.reduce_naive(a, out_rows, out_cols, detector)
        got = view_ref.reduce_block(a, out_rows, out_cols, detector)
        if detector == view_ref.PEAK:
            assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
        else:
            mean, mean_abs, count = got
            assert np.allclose(mean, want, rtol=1e-13, atol=1e-15)
            assert np.all(mean_abs >= np.abs(mean) - 1e-15) and count.sum() >= rows * cols


def test_reference_window_and_ring_order():
    assert list(view_ref.window_columns(16, 6, 5)) == [14, 15, 0, 1, 2]	# shifted 6..10 of 16: across DC
    assert list(view_ref.ring_rows(8, 2, 4)) == [1, 0, 7, 6]			# newest first, wrapping
