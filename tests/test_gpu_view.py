"""Views on the device (include/fosphor_amd_view.h) against their numpy statement (tests/view_ref.py).

Every case goes through the C ABI or the Python class; the state is read back with the waterfall / histogram / spectrum /
waterfall_pos properties and reduced on the CPU.  Geometries (sizes chosen so that every row count the cases ask for exists and a
readback stays small): 1024 points with 128 and 256 bins and the default 1024 waterfall rows; 8192 points, 512 bins, 512 rows;
65536 points, 512 bins, fp16 input, 512 rows (waterfall 128 MiB, histogram 128 MiB).  Every ring is filled past its end, so
waterfall_pos != 0 and the newest rows wrap.
"""
import ctypes as C
import errno
import os

import numpy as np
import pytest

import view_ref
from oracle_lib import gaussian_iq, add_tone

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cmap_palettes.npz"))
PEAK, AVERAGE = view_ref.PEAK, view_ref.AVERAGE
FLOATS = ("waterfall", "histogram", "live", "max")


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class State:
    """an instance and the host copy of what a view of it reads"""

    def __init__(self, f):
        f.draw()
        self.f = f
        self.wf, self.hist, self.spec, self.pos = f.waterfall, f.histogram, f.spectrum, f.waterfall_pos
        self.n, self.bins, self.wf_rows = f.n, f.n_bins, f.wf_rows
        # the reference's colouring defaults, as tests/test_cmap.py derives them
        self.wf_color = (GOLD["waterfall_256"], np.float32(f.histo_scale / f.n_bins), np.float32(f.histo_offset))
        self.histo_color = (GOLD["histogram_256"], np.float32(1.1), np.float32(0.0))

    def ref(self, first_bin, n_cols, width, src_rows, out_rows, detector, what=FLOATS):
        return view_ref.view(self.wf, self.hist, self.spec, self.pos, first_bin, n_cols, width, src_rows, out_rows, detector, what)

    def arrays(self):
        return [self.f.waterfall, self.f.histogram, self.f.spectrum, np.array([self.f.waterfall_pos])]


def make_state(amd, log, bins):
    import torch
    n = 1 << log
    if log == 10:
        f = amd.Fosphor(n_bins=bins)
        x = add_tone(add_tone(gaussian_iq(1024 * 1024, 61), 0.2, 0.17), 0.1, -0.31)
        assert f.process(x[:768 * 1024]) == 0
        assert f.process(x[256 * 1024:768 * 1024]) == 0		# wrapped: pos = 256
        want_pos = 256
    else:
        f = amd.Fosphor(fft_len_log=log, n_bins=bins, wf_rows=512, max_spectra=64, iq_fp16=(log == 16))
        for call in range(9):						# 576 spectra into 512 rows: pos = 64
            x = add_tone(gaussian_iq(64 * n, 70 + call), 0.05 + 0.01 * call, 0.0313 * (call - 4), t0=call * 64 * n)
            if log == 16:
                x = x.astype(np.float16)
            d_x = torch.from_numpy(x).cuda()
            assert f.process_device(d_x, 1, 64) == 0
            assert f.finish() >= 0					# d_x is read until here
        want_pos = 64
    s = State(f)
    assert s.pos == want_pos
    assert all(np.isfinite(a).all() for a in (s.wf, s.hist, s.spec))
    return s


def make_special_state(amd):
    """inf / NaN spectra and an all-zero spectrum (-inf dB), as test_colorize_special_values_and_errors feeds them"""
    f = amd.Fosphor()
    x = gaussian_iq(16 * 1024, 5)
    x[3] = np.inf; x[2048 + 10] = np.nan; x[4096:6144] = 0.0
    assert f.process(x) == 0
    s = State(f)
    assert np.isnan(s.wf).any() and np.isinf(s.wf).any()
    return s


def rgba32(t):
    return t.cpu().numpy().view(np.uint32).reshape(t.shape[:-1])


def check_view(s, first_bin, n_cols, width, src_rows, out_rows, detector, finite=True, what=FLOATS):
    """one view, floats and RGBA together, against view_ref; returns the device results as numpy arrays"""
    tag = "N=%d bins=%d view=(%d, %d -> %d; %d -> %d rows) det=%d" % (s.n, s.bins, first_bin, n_cols, width, src_rows, out_rows, detector)
    outputs = [k for k in s.f.VIEW_OUTPUTS if k.split("_")[0] in what]
    got = s.f.view(first_bin, n_cols, width, src_rows, out_rows, detector=("peak", "average")[detector], outputs=outputs)
    got = {k: (rgba32(v) if k.endswith("_rgba") else v.cpu().numpy()) for k, v in got.items()}
    want = s.ref(first_bin, n_cols, width, src_rows, out_rows, detector, what)
    for k in what:
        g = got[k]
        assert g.dtype == np.float32
        if detector == PEAK:
            assert g.shape == want[k].shape, (tag, k)
            assert np.array_equal(np.isnan(g), np.isnan(want[k])), (tag, k, "NaN positions")
            assert np.array_equal(g, want[k], equal_nan=True), (tag, k)
        else:
            mean, mean_abs, count = want[k]
            assert g.shape == mean.shape, (tag, k)
            if finite:
                assert np.isfinite(mean).all() and np.isfinite(g).all(), (tag, k)
                err, bound = np.abs(g.astype(np.float64) - mean), view_ref.average_bound(mean, mean_abs, count)
                worst = np.argmax(err - bound)
                print("%s %s: AVERAGE worst |err| %.3g at bound %.3g (k = %d)" % (tag, k, err.flat[worst], bound.flat[worst], count.flat[worst]))
                assert np.all(err <= bound), (tag, k, err.flat[worst], bound.flat[worst])	# no cell is excused
            else:
                assert np.array_equal(np.isnan(g), np.isnan(mean)), (tag, k, "NaN pixels")
                assert np.array_equal(np.isposinf(g), np.isposinf(mean)) and np.array_equal(np.isneginf(g), np.isneginf(mean)), (tag, k)
    for k, (pal, scale, offset) in (("waterfall", s.wf_color), ("histogram", s.histo_color)):
        if k in what:
            # PEAK: the float picture is the reference's, so this is the reference's colouring; AVERAGE: the lookup of the call's own floats
            assert np.array_equal(got[k + "_rgba"], view_ref.lookup(got[k], pal, scale, offset)), (tag, k + "_rgba")
    return got


def window_views(n):
    """(first_bin, n_cols, width): the frequency cases of every geometry"""
    h = n // 2
    return [(0, n, n),					# identity
            (0, n, 1024), (0, n, 1000), (0, n, 333), (0, n, 1),	# full span
            (0, n, 64),					# spans of 16 cells and more at every length
            (h - 301, 777, 200), (h - 1, 3, 2), (h - 333, 666, 666),	# across N/2 at an odd first_bin
            (5, 400, 400), (7, h - 7, 97), (h, h, 500), (h + 9, 300, 97), (n - 1, 1, 1),	# one side only
            (h - 37, 100, 640), (h + 3, 1, 64), (3, 2, 1000)]	# magnification, a single column


def time_views(rows):
    """(wf_src_rows, wf_out_rows): 1, a non-dividing count and every row, to 1, 300 and every row"""
    return [(a, b) for a in (1, 301, rows) for b in (1, 300, rows)]


@pytest.mark.parametrize("log,bins", [(10, 128), (10, 256), (13, 512), (16, 512)])
def test_views_equal_reference(amd, log, bins):
    s = make_state(amd, log, bins)
    n, rows = s.n, s.wf_rows
    before = s.f.view_stats()
    assert before == dict.fromkeys(s.f.VIEW_FORMS, 0)
    for det in (PEAK, AVERAGE):
        for first_bin, n_cols, width in window_views(n):
            check_view(s, first_bin, n_cols, width, rows, rows, det)
        for src_rows, out_rows in time_views(rows):
            check_view(s, 0, n, 333, src_rows, out_rows, det, what=("waterfall",))
            check_view(s, n // 2 - 301, 777, 200, src_rows, out_rows, det, what=("waterfall",))
        check_view(s, n // 2 - 37, 100, 640, 301, 300, det, what=("waterfall",))	# magnified in frequency, reduced in time
        check_view(s, 0, n, 1, rows, 1, det, what=("waterfall",))			# everything into one pixel
    st = s.f.view_stats()
    assert all(st[k] > 0 for k in s.f.VIEW_FORMS), st				# the cases above ran every form
    s.f.close()


def test_views_of_non_finite_state(amd):
    s = make_special_state(amd)
    n = s.n
    for det in (PEAK, AVERAGE):
        for first_bin, n_cols, width in [(0, n, n), (0, n, 333), (0, n, 1), (n // 2 - 301, 777, 200), (n // 2 - 37, 100, 640)]:
            for src_rows, out_rows in [(32, 32), (32, 5), (1024, 300), (16, 1)]:
                check_view(s, first_bin, n_cols, width, src_rows, out_rows, det, finite=False)
    s.f.close()


@pytest.mark.parametrize("log,bins", [(10, 128), (13, 512)])
def test_identity_view_equals_colorize(amd, log, bins):
    s = make_state(amd, log, bins)
    f = s.f
    v = f.view(outputs=("waterfall_rgba", "histogram_rgba"))
    assert np.array_equal(rgba32(v["waterfall_rgba"]), rgba32(f.colorize(0)))
    assert np.array_equal(rgba32(v["histogram_rgba"]), rgba32(f.colorize(1)))
    assert len(np.unique(rgba32(v["histogram_rgba"]))) > 20			# a real picture, not a constant
    v = f.view(outputs=("waterfall_rgba", "histogram_rgba"), wf_palette=GOLD["prog_1000"], wf_scale=0.37, wf_offset=2.5,
               histo_palette=GOLD["waterfall_64"], histo_scale=3.0, histo_offset=-0.01)
    assert np.array_equal(rgba32(v["waterfall_rgba"]), rgba32(f.colorize(0, palette=GOLD["prog_1000"], scale=0.37, offset=2.5)))
    assert np.array_equal(rgba32(v["histogram_rgba"]), rgba32(f.colorize(1, palette=GOLD["waterfall_64"], scale=3.0, offset=-0.01)))
    # fewer rows: the newest 300
    v = f.view(wf_src_rows=300, outputs=("waterfall_rgba",))
    assert np.array_equal(rgba32(v["waterfall_rgba"]), rgba32(f.colorize(0, rows=300)))
    f.close()


def test_view_from_render_is_the_zoomed_second_view(amd):
    """the demo's second render (main.c: 0.2 of the span around the centre), at display size"""
    s = make_state(amd, 10, 128)
    r = amd._lib.Render()
    s.f.L.fosphor_render_defaults(C.byref(r))
    r.freq_center, r.freq_span, r.wf_span = 0.5, 0.2, 0.5
    got = s.f.view_from_render(r, 640, 300)
    want = s.ref(410, 205, 640, 512, 300, PEAK)
    for k in FLOATS:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert got["waterfall_rgba"].shape == (300, 640, 4) and got["histogram_rgba"].shape == (128, 640, 4)
    s.f.close()


@pytest.mark.parametrize("detector", ["peak", "average"])
def test_each_output_alone_equals_all_together(amd, detector):
    s = make_state(amd, 10, 128)
    f = s.f
    for args in [(211, 777, 200, 301, 300), (0, 1024, 1, 1024, 1), (475, 100, 640, 7, 7)]:
        kw = dict(detector=detector, wf_palette=GOLD["prog_1000"], histo_scale=0.9, histo_offset=0.05)
        full = {k: v.cpu().numpy() for k, v in f.view(*args, **kw).items()}
        assert sorted(full) == sorted(f.VIEW_OUTPUTS)
        for k in f.VIEW_OUTPUTS:
            alone = f.view(*args, outputs=(k,), **kw)
            assert list(alone) == [k]
            assert np.array_equal(alone[k].cpu().numpy(), full[k], equal_nan=True), (args, k)
        half = f.view(*args, rgba=False, **kw)
        assert sorted(half) == sorted(FLOATS)
        half = f.view(*args, floats=False, **kw)
        assert sorted(half) == ["histogram_rgba", "waterfall_rgba"]
    f.close()


def test_views_only_read(amd):
    a, b = make_state(amd, 10, 128), make_state(amd, 10, 128)		# b is never viewed
    before = a.arrays()
    for det in ("peak", "average"):
        for first_bin, n_cols, width in window_views(a.n):
            a.f.view(first_bin, n_cols, width, 301, 300, detector=det)
    for x, y in zip(before, a.arrays()):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    x = add_tone(gaussian_iq(64 * 1024, 99), 0.1, 0.05)
    assert a.f.process(x) == 0 and b.f.process(x) == 0
    a.f.draw(); b.f.draw()
    for u, w in zip(a.arrays(), b.arrays()):
        assert np.array_equal(u.view(np.uint32) if u.dtype == np.float32 else u, w.view(np.uint32) if w.dtype == np.float32 else w)
    assert np.array_equal(a.f.hitcount, b.f.hitcount)
    a.f.close(); b.f.close()


def test_view_errors_write_nothing(amd):
    import torch
    s = make_state(amd, 10, 128)
    f, L, lib = s.f, s.f.L, amd._lib
    n, rows = s.n, s.wf_rows
    sentinel = 0x5a5a5a5a
    bufs = {k: torch.full((rows * n,), sentinel, dtype=torch.int32, device="cuda") for k in f.VIEW_OUTPUTS}

    def out(names=f.VIEW_OUTPUTS):
        o = lib.ViewOut()
        for k in names:
            setattr(o, "d_" + k, bufs[k].data_ptr())
        o.wf_color.use_defaults = o.histo_color.use_defaults = 1
        return o

    def call(v, o):
        return L.fosphor_amd_view(f.h, C.byref(lib.View(*v)) if v is not None else None, C.byref(o) if o is not None else None)

    good = (100, 500, 64, 300, 30, PEAK)
    bad = [(-1, 500, 64, 300, 30, PEAK), (n, 1, 64, 300, 30, PEAK),			# first_bin
           (100, 0, 64, 300, 30, PEAK), (100, n - 99, 64, 300, 30, PEAK), (0, n + 1, 64, 300, 30, PEAK),	# n_cols
           (100, 500, 0, 300, 30, PEAK), (100, 500, 65537, 300, 30, PEAK), (100, 500, -3, 300, 30, PEAK),	# width
           (100, 500, 64, 0, 30, PEAK), (100, 500, 64, rows + 1, 30, PEAK),		# wf_src_rows
           (100, 500, 64, 300, 0, PEAK), (100, 500, 64, 300, rows + 1, PEAK),		# wf_out_rows
           (100, 500, 64, 300, 30, 2), (100, 500, 64, 300, 30, -1)]			# detector
    for v in bad:
        assert call(v, out()) == -errno.EINVAL, v
        assert call(v, out(("live",))) == -errno.EINVAL, v			# every field is checked whatever is produced
    assert call(good, lib.ViewOut()) == -errno.EINVAL				# nothing to produce
    assert call(good, None) == -errno.EINVAL and call(None, out()) == -errno.EINVAL
    assert L.fosphor_amd_view(None, C.byref(lib.View(*good)), C.byref(out())) == -errno.EINVAL
    for pal_n in (1, 4097, 5000, 0, -1):						# palette entry counts
        pal = np.zeros(5000, np.uint32)
        for which in ("wf_color", "histo_color"):
            o = out()
            getattr(o, which).palette, getattr(o, which).n = pal.ctypes.data, pal_n
            assert call(good, o) == -errno.EINVAL, (which, pal_n)
    o = out(FLOATS)									# a bad palette beside a picture that is not asked for is not read
    o.wf_color.palette, o.wf_color.n = 1, 1
    torch.cuda.synchronize()
    for k in bufs:
        assert bool((bufs[k] == sentinel).all()), k
    assert call(good, o) == 0
    assert not bool((bufs["waterfall"][:30 * 64] == sentinel).any())
    assert bool((bufs["waterfall"][30 * 64:] == sentinel).all()) and bool((bufs["waterfall_rgba"] == sentinel).all())
    with pytest.raises(RuntimeError):
        f.view(first_bin=n)
    with pytest.raises(RuntimeError):
        f.view(width=65537)
    with pytest.raises(ValueError):
        f.view(detector="median")
    with pytest.raises(ValueError):
        f.view(outputs=("hitcount",))
    r = lib.Render()
    L.fosphor_render_defaults(C.byref(r))
    r.freq_span = 0.0
    with pytest.raises(RuntimeError):
        f.view_from_render(r, 640, 300)
    f.close()
