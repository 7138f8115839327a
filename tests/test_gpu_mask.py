"""The frequency mask on the device (include/fosphor_amd_mask.h) against its numpy statement (tests/mask_model.py).

Inputs are planted straight into the waterfall ring and the spectrum lines (gr_fosphor_amd.dist.wrap_device_array over
fosphor_amd_get_buffers_nohc, re-queried after every wait: the waterfall is one of two rings), outputs go into sentinel-filled
buffers, and every planted test ends by checking that the ring and the spectrum are bit-identical (the pass only reads) and that
nothing beyond the specified extents was written.

Geometries: (1024 points, wf_rows 16); (1024 points, wf_rows 256) for the event list and the ring position; (65536 points, 512 bins,
wf_rows 16, max_spectra 16), a 4 MiB ring; and (1024 points, wf_rows 8192), a 32 MiB ring, the smallest at which a work-group takes
more than one row (see below).

Seams of k_mask_scan, all counted from a = first column of the call & ~3: a lane owns the aligned group of 4 columns a + 4k (one
16-byte load; the groups the window cuts at its head and tail load column by column), a wave 256 columns, a work-group a strip of
FOSPHOR_AMD_MASK_STRIP = 1024 columns, and in the SHARED form (more than one strip: only at 65536 points) the strips are the shares
of a row that k_mask_combine merges.  Memory columns wrap at shifted column N/2.  Along time a work-group takes rpg = rows * strips /
1024 consecutive rows (1 .. 32) and loads them 4 at a time: rpg is 1 at the three small geometries, and 7 / 8 with 8191 / 8192 rows
of 1024 points.  k_mask_events: lane t of 1024 owns the rows [t * chunk, (t + 1) * chunk), chunk = ceil(rows / 1024); waves meet
every 64 lanes (rows 63 | 64 at chunk 1).

The ring position moves in steps of 16 only (the library takes spectra in multiples of 16), so the positions under test are 0, 16,
wf_rows - 16 and mid-ring, at wf_rows 256.
"""
import ctypes as C
import errno
import os

import numpy as np
import pytest

import mask_model as mm
from oracle_lib import Oracle, gaussian_iq, add_tone

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a5a5a5a
STRIP = 1024


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Ring:
    """an instance, torch views of its waterfall ring [wf_rows][N] and spectrum [2][N][2], and what was planted"""

    def __init__(self, amd, log, wf_rows):
        if log == 10:
            self.f = amd.Fosphor(n_bins=128, wf_rows=wf_rows)
        else:
            self.f = amd.Fosphor(fft_len_log=log, n_bins=512, wf_rows=wf_rows, max_spectra=16)
        self.n, self.wf_rows, self.lib = self.f.n, wf_rows, amd._lib
        assert self.f.finish() >= 0			# a new instance fills its buffers at its first wait (the boot): before anything is planted
        self.saved = None

    def views(self):
        import torch
        from gr_fosphor_amd.dist import wrap_device_array
        b = self.f.buffers(False)
        assert (b.fft_len, b.wf_rows) == (self.n, self.wf_rows)
        self.pos = b.waterfall_pos
        self.wf = wrap_device_array(b.d_waterfall, (self.wf_rows, self.n), torch.float32)
        self.spec = wrap_device_array(b.d_spectrum, (2, self.n, 2), torch.float32)

    def plant(self, ys=None, live=None, maxhold=None):
        """ys: [wf_rows][N] by source index j (0 = newest) and shifted column"""
        import torch
        assert self.f.finish() >= 0
        self.views()
        if ys is not None:
            mem = np.empty((self.wf_rows, self.n), np.float32)
            mem[(self.pos - 1 - np.arange(self.wf_rows)) % self.wf_rows] = mm.shift(np.asarray(ys, np.float32))
            assert mm.same_bits(mm.newest_first(mem, self.pos), np.asarray(ys, np.float32))
            self.wf.copy_(torch.from_numpy(mem))
        for row, y in ((0, live), (1, maxhold)):
            if y is not None:
                self.spec[row, :, 1].copy_(torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)))
        torch.cuda.synchronize()
        self.saved = (self.wf.view(torch.int32).clone(), self.spec.view(torch.int32).clone(), self.pos)

    def assert_untouched(self):
        import torch
        torch.cuda.synchronize()
        self.views()
        assert self.pos == self.saved[2], "the ring position moved"
        assert torch.equal(self.wf.view(torch.int32), self.saved[0]), "the waterfall was written"
        assert torch.equal(self.spec.view(torch.int32), self.saved[1]), "the spectrum lines were written"

    def scan(self, first_bin, n_cols, rows, min_cols=1, upper=None, lower=None, channels=(), max_events=0, alloc_events=None,
             want_rows=True, want_events=None, want_power=None, want_result=True, null_cfg=False, n_channels=None):
        """fosphor_amd_mask_scan through the C ABI into sentinel-filled buffers with guard entries behind the specified extents"""
        import torch
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        d_up, d_lo = dev(upper), dev(lower)
        cfg = self.lib.MaskCfg(first_bin, n_cols, rows, min_cols, len(channels) if n_channels is None else n_channels)
        for k, (a, b) in enumerate(channels):
            cfg.channels[k].first, cfg.channels[k].last = a, b
        nr = max(rows, 1)
        want_events = (max_events != 0) if want_events is None else want_events
        want_power = (len(channels) > 0) if want_power is None else want_power
        alloc_events = max(max_events, 1) + 2 if alloc_events is None else alloc_events
        d_res = torch.full((4 + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        d_rows = torch.full(((nr + 1) * 6,), SENTINEL, dtype=torch.int32, device="cuda")
        d_ev = torch.full((alloc_events,), SENTINEL, dtype=torch.int32, device="cuda")
        d_pow = torch.full(((max(len(channels), 1) + 1) * nr,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()			# the fills and the uploads run on torch's stream, the pass on the instance's
        ptr = lambda t, on: t.data_ptr() if (on and t is not None) else None
        rv = self.f.L.fosphor_amd_mask_scan(self.f.h, None if null_cfg else C.byref(cfg), ptr(d_up, True), ptr(d_lo, True),
                                            ptr(d_res, want_result), ptr(d_rows, want_rows), ptr(d_ev, want_events), max_events,
                                            ptr(d_pow, want_power))
        raw = dict(res=d_res.cpu().numpy(), rows=d_rows.cpu().numpy(), ev=d_ev.cpu().numpy(), pow=d_pow.cpu().numpy())
        out = dict(rv=rv, raw=raw, result=raw["res"][:4].copy().view(mm.RESULT_DTYPE)[0],
                   rows=raw["rows"][:nr * 6].copy().view(mm.ROW_DTYPE), events=raw["ev"],
                   power=raw["pow"][:len(channels) * nr].copy().view(np.float32).reshape(len(channels), nr))
        # nothing behind the specified extents
        assert np.all(raw["res"][4:] == SENTINEL) and np.all(raw["rows"][nr * 6:] == SENTINEL)
        assert np.all(raw["pow"][len(channels) * nr:] == SENTINEL)
        if rv == 0:
            assert np.all(raw["ev"][int(out["result"]["n_written"]):] == SENTINEL)
        return out

    def assert_nothing_written(self, out, tag=""):
        for k, v in out["raw"].items():
            assert np.all(v == SENTINEL), (tag, k)


def assert_result(got, want, tag=""):
    for k in mm.RESULT_DTYPE.names:
        assert int(got[k]) == int(want[k]), (tag, k, int(got[k]), int(want[k]))


def planted_rows(n, wf_rows, seed, extra_cols=()):
    """ys [wf_rows][N] (j order, shifted) and limits [N]: quiet cells between the limits, then on every row a random sprinkle of
    over / under / NaN / +-inf / equal-to-limit cells and of tied excesses, and on row j % 4 == 1 a violation on both sides of every
    seam column in `extra_cols` (and of N/2, 256 k and 1024 k)"""
    rng = np.random.default_rng(seed)
    up = (1.0 + 0.2 * rng.random(n)).astype(np.float32)
    lo = (-1.0 - 0.2 * rng.random(n)).astype(np.float32)
    up[rng.integers(0, n, max(n // 200, 2))] = np.nan			# a NaN limit is violated by nothing
    lo[rng.integers(0, n, max(n // 200, 2))] = np.nan
    ys = (rng.random((wf_rows, n)) - 0.5).astype(np.float32)
    seams = sorted(set([c for c in list(extra_cols) + [n // 2] + list(range(256, n, 256)) if 0 < c < n]))
    for j in range(wf_rows):
        k = rng.integers(0, n, 12)
        ys[j, k[0]], ys[j, k[1]], ys[j, k[2]] = np.nan, np.inf, -np.inf
        ys[j, k[3]], ys[j, k[4]] = up[k[3]], lo[k[4]]				# equality violates neither side
        ys[j, k[5:8]] = up[k[5:8]] + np.float32(0.5) * rng.integers(1, 3)	# over, small set of excesses: ties in the data
        ys[j, k[8:10]] = lo[k[8:10]] - np.float32(rng.random() + 0.1)
        if j % 4 == 1:
            for c in seams:
                ys[j, c - 1] = up[c - 1] + np.float32(1.5) if np.isfinite(up[c - 1]) else np.float32(9.0)
                ys[j, c] = lo[c] - np.float32(1.5) if np.isfinite(lo[c]) else np.float32(-9.0)
        if j % 4 == 3:
            ys[j] = np.clip(ys[j], -0.5, 0.5)					# a row without a violation
            ys[j, np.isnan(ys[j])] = 0.0
    return ys, up, lo


def windows_of(n):
    """(first_bin, n_cols): the whole width; a single column; first_bin odd with n_cols no multiple of 4; ending at N/2 - 1;
    starting at N/2; straddling N/2 by one column each side; the last column; a head and tail cut inside a 16-byte group with the
    strips moved off the multiples of 1024"""
    h = n // 2
    return [(0, n), (h + 37, 1), (5, n - 5 - 6), (h - 301, 301), (h, 207), (h - 1, 2), (n - 1, 1), (n - 3, 3), (259, min(n - 259 - 2, 1500))]


def check_rows(s, ys, up, lo, first_bin, n_cols, rows, mode, tag, plant_edges=True):
    upper, lower = (up if mode != "lower" else None), (lo if mode != "upper" else None)
    want = mm.rows_rule(ys[:rows], upper, lower, first_bin, n_cols)
    o = s.scan(first_bin, n_cols, rows, upper=upper, lower=lower)
    assert o["rv"] == 0, tag
    mm.assert_rows_equal(o["rows"], want, tag)
    assert_result(o["result"], mm.events(want, 1, 0)[0], tag)
    return want


GEOS = {"N1024_rows16": (10, 16), "N65536_rows16": (16, 16)}


@pytest.fixture(scope="module", params=list(GEOS), ids=list(GEOS))
def ring(request, amd):
    log, wf_rows = GEOS[request.param]
    s = Ring(amd, log, wf_rows)
    n = s.n
    seam_cols = []
    for first_bin, n_cols in windows_of(n):				# every window's first and last column, and its own strip seams
        a = first_bin & ~3
        seam_cols += [first_bin + 1, first_bin + n_cols - 1] + [c for c in range(a + 256, first_bin + n_cols, 256)]
    s.ys, s.up, s.lo = planted_rows(n, wf_rows, 5, seam_cols)
    for first_bin, n_cols in windows_of(n):				# violations at the first and last column of every window, row 1
        s.ys[1, first_bin] = np.float32(7.0)
        s.ys[1, first_bin + n_cols - 1] = np.float32(-7.0)
        for a in (s.up, s.lo):
            a[first_bin] = np.nan_to_num(a[first_bin], nan=0.25)
            a[first_bin + n_cols - 1] = np.nan_to_num(a[first_bin + n_cols - 1], nan=-0.25)
    s.plant(ys=s.ys)
    yield s
    s.f.close()


@pytest.mark.parametrize("mode", ["both", "upper", "lower"])
def test_row_records_exact(ring, mode):
    """1. integers and peak_over bit for bit against the model, every window of windows_of(), violations on both sides of every
    seam the docstring of this file names (row 1 carries them at the windows' edges, at N/2 and at every multiple of 256 counted
    from each window's aligned origin, which are the wave, work-group and share seams; the random cells fall on the 16-byte groups)"""
    s, n = ring, ring.n
    for first_bin, n_cols in windows_of(n):
        tag = "N=%d window=(%d, %d) %s" % (n, first_bin, n_cols, mode)
        want = check_rows(s, s.ys, s.up, s.lo, first_bin, n_cols, s.wf_rows, mode, tag)
        if mode == "both":
            assert want["first_col"][1] == first_bin and want["last_col"][1] == first_bin + n_cols - 1, tag
        if n_cols == n:
            assert (want["n_over"] + want["n_under"] > 0).sum() >= s.wf_rows // 2, tag		# the planted violations are there
    # the Python class gives the same
    import torch
    d_up, d_lo = torch.from_numpy(s.up).cuda(), torch.from_numpy(s.lo).cuda()
    res, rows, events, power = s.f.mask_scan(upper=d_up if mode != "lower" else None, lower=d_lo if mode != "upper" else None,
                                             first_bin=5, n_cols=n - 11, max_events=64)
    want = mm.rows_rule(s.ys, s.up if mode != "lower" else None, s.lo if mode != "upper" else None, 5, n - 11)
    mm.assert_rows_equal(rows, want)
    wres, wev = mm.events(want, 1, 64)
    assert res == {k: int(wres[k]) for k in mm.RESULT_DTYPE.names} and np.array_equal(events, wev) and power.shape == (0, s.wf_rows)
    s.assert_untouched()


def test_every_form_ran(ring):
    """3. a shape per counted form, proven by mask_stats before and after, results equal to the model in each"""
    s, n = ring, ring.n
    shared = n > STRIP
    for first_bin, n_cols, rows, form in [(0, n, 3, "form_shared" if shared else "form_rows"),
                                          (n // 2 - 100, 200, 3, "form_rows"),		# one strip at either width
                                          (3, 1021, s.wf_rows, "form_rows"),			# [0, 1024): still one strip
                                          (3, 1022, s.wf_rows, "form_shared" if shared else None)]:
        if form is None:
            continue
        before = s.f.mask_stats()
        check_rows(s, s.ys, s.up, s.lo, first_bin, n_cols, rows, "both", "form %s (%d, %d)" % (form, first_bin, n_cols))
        after = s.f.mask_stats()
        other = "form_rows" if form == "form_shared" else "form_shared"
        assert after[form] - before[form] == 1 and after[other] == before[other] and after["scans"] - before["scans"] == 1, (form, before, after)
        assert after["from_trace"] == before["from_trace"]
    if shared:
        before = s.f.mask_stats()
        o = s.scan(0, n, 3, upper=s.up, channels=[(10, 20)])		# the 65536-point geometry with rows = 3: the shared-row form
        assert o["rv"] == 0 and s.f.mask_stats()["form_shared"] - before["form_shared"] == 1
    s.assert_untouched()


def channel_sets(n):
    h = n // 2
    return [[(h + 3, h + 3)],
            [(7, 7), (0, n - 1), (100, 400), (300, 500), (h - 1, h), (h - 130, h + 140), (n - 1, n - 1), (n - 260, n - 2)]]


@pytest.mark.parametrize("masked", [True, False], ids=["with_mask", "power_only"])
def test_channel_power(ring, masked):
    """5. 1 and 8 channels: one column, the whole width, overlapping, inside and outside the mask window, straddling N/2; rows with
    -inf and NaN cells and an all -inf channel; within 5e-5 absolute of the model, equal infinities passing.  Both limits NULL is a
    pure power pass: every record all-zero / -1 / NaN, nothing triggers."""
    s, n = ring, ring.n
    ys = s.ys.copy()
    ys[2, 100:401] = -np.inf							# an all -inf channel on row 2: (100, 400)
    ys[5, 7] = np.nan								# a channel of one NaN column
    s.plant(ys=ys)
    worst = 0.0
    windows = [(0, n), (50, 500), (n // 2 - 64, 300)] if masked else [(0, n)]
    for chans in channel_sets(n):
        for first_bin, n_cols in windows:
            for rows in (s.wf_rows, 3):
                tag = "N=%d %d channels window=(%d, %d) rows=%d masked=%s" % (n, len(chans), first_bin, n_cols, rows, masked)
                before = s.f.mask_stats()
                o = s.scan(first_bin, n_cols, rows, upper=s.up if masked else None, lower=s.lo if masked else None, channels=chans,
                           max_events=4)
                assert o["rv"] == 0, tag
                want = mm.channel_power(ys[:rows], chans)
                err = mm.power_error(o["power"], want)
                worst = max(worst, err)
                assert err <= 5e-5, (tag, err)
                if masked:
                    wrows = mm.rows_rule(ys[:rows], s.up, s.lo, first_bin, n_cols)
                    inside = [first_bin <= a and b < first_bin + n_cols for a, b in chans]
                    launches = 1 + (not all(inside))
                else:
                    wrows = mm.rows_rule(ys[:rows], None, None, 0, n)
                    assert np.all(wrows["n_over"] == 0) and np.all(wrows["peak_col"] == -1) and np.isnan(wrows["peak_over"]).all()
                    launches = 1
                mm.assert_rows_equal(o["rows"], wrows, tag)
                assert_result(o["result"], mm.events(wrows, 1, 4)[0], tag)
                after = s.f.mask_stats()
                assert after["form_rows"] + after["form_shared"] - before["form_rows"] - before["form_shared"] == launches, tag
    assert np.isneginf(mm.channel_power(ys[2:3], [(100, 400)])[0, 0]) and np.isneginf(mm.channel_power(ys[5:6], [(7, 7)])[0, 0])
    print("N=%d masked=%s: worst |power error| %.3g" % (n, masked, worst))
    s.assert_untouched()
    s.plant(ys=s.ys)


def test_mask_from_trace(ring):
    """6. bit for bit against the model: spread 0, 1, 64, 1024; NaN vertices, among them a run longer than 2 * spread + 1 (NaN out);
    live and max-hold; both edges of the width"""
    import torch
    s, n = ring, ring.n
    rng = np.random.default_rng(21)
    traces = []
    for k in range(2):
        y = (rng.standard_normal(n) + 0.01).astype(np.float32)
        y[rng.integers(0, n, n // 50)] = np.nan
        y[0], y[n - 1] = 3.0 + k, 4.0 + k					# the greatest values sit on the edges
        y[300:300 + 140] = np.nan						# longer than 2 * 64 + 1
        if n > 4096:
            y[9000:9000 + 2100] = np.nan					# longer than 2 * 1024 + 1
        y[5], y[6] = -np.inf, np.inf
        traces.append(y)
    s.plant(live=traces[0], maxhold=traces[1])
    before = s.f.mask_stats()
    calls = 0
    for trace in (0, 1):
        for spread, margin in [(0, 0.3), (1, 0.0), (64, -0.125), (1024, 0.3)]:
            want = mm.from_trace(traces[trace], margin, spread)
            d = torch.full((n + 2,), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            rv = s.f.L.fosphor_amd_mask_from_trace(s.f.h, trace, margin, spread, d.data_ptr())
            calls += 1
            got = d.cpu().numpy()
            tag = "N=%d trace=%d spread=%d" % (n, trace, spread)
            assert rv == 0 and np.all(got[n:] == SENTINEL), tag
            g = got[:n].view(np.float32)
            assert np.array_equal(np.isnan(g), np.isnan(want)), tag
            assert np.array_equal(g[~np.isnan(g)].view(np.uint32), want[~np.isnan(want)].view(np.uint32)), tag
            if spread == 64:
                assert np.isnan(want[300 + 64:300 + 140 - 64]).all() and not np.isnan(want[300 + 63])
            if spread == 0:
                assert same_nan_bits(g, traces[trace] + np.float32(margin))
    out = s.f.mask_from_trace("live", margin_db=6.0, spread_cols=2)		# the Python class
    assert mm.same_bits(np.nan_to_num(out.cpu().numpy(), nan=-77.0), np.nan_to_num(mm.from_trace(traces[0], np.float32(6.0 / 20.0), 2), nan=-77.0))
    after = s.f.mask_stats()
    assert after["from_trace"] - before["from_trace"] == calls + 1 and after["scans"] == before["scans"]
    # argument errors write nothing
    d = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for trace, spread in [(2, 0), (-1, 0), (0, -1), (0, 1025)]:
        assert s.f.L.fosphor_amd_mask_from_trace(s.f.h, trace, 0.0, spread, d.data_ptr()) == -errno.EINVAL
    assert s.f.L.fosphor_amd_mask_from_trace(s.f.h, 0, 0.0, 0, None) == -errno.EINVAL
    assert bool((d == SENTINEL).all())
    with pytest.raises(ValueError):
        s.f.mask_from_trace("average")
    s.assert_untouched()


def same_nan_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


def test_einval_writes_nothing(ring):
    """7. every listed cause, against sentinel-filled outputs"""
    s, n = ring, ring.n
    good = dict(first_bin=10, n_cols=500, rows=4, min_cols=1, upper=s.up, lower=s.lo, channels=[(3, 9)], max_events=8)
    bad = [dict(first_bin=-1), dict(first_bin=n), dict(n_cols=0), dict(n_cols=n - 9), dict(first_bin=0, n_cols=n + 1),
           dict(rows=0), dict(rows=-2), dict(rows=s.wf_rows + 1), dict(min_cols=0), dict(min_cols=-3),
           dict(n_channels=-1), dict(n_channels=9),
           dict(channels=[(9, 3)]), dict(channels=[(-1, 3)]), dict(channels=[(3, n)]), dict(channels=[(0, 5), (n, n)]),
           dict(max_events=-1, want_events=True), dict(max_events=65537), dict(max_events=0, want_events=True),
           dict(max_events=8, want_events=False),
           dict(null_cfg=True), dict(want_result=False),
           dict(want_power=False), dict(channels=[], want_power=True),
           dict(upper=None, lower=None, channels=[], max_events=8)]			# nothing to do
    for change in bad:
        o = s.scan(**dict(good, **change))
        assert o["rv"] == -errno.EINVAL, change
        s.assert_nothing_written(o, change)
    o = s.scan(**good)								# and the good one is good
    assert o["rv"] == 0 and int(o["result"]["n_written"]) <= 8
    import torch
    with pytest.raises(RuntimeError):
        s.f.mask_scan(upper=torch.zeros(n, device="cuda"), min_cols=0)
    with pytest.raises(RuntimeError):
        s.f.mask_scan()
    with pytest.raises(ValueError):
        s.f.mask_scan(upper=torch.zeros(n - 1, device="cuda"))
    s.assert_untouched()


# ---- the ring position and the event list: wf_rows 256 ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def ring256(amd):
    s = Ring(amd, 10, 256)
    s.ys, s.up, s.lo = planted_rows(s.n, 256, 6)
    yield s
    s.f.close()


def test_ring_order(ring256):
    """2. the same planted rows give the same records wherever the ring stands: waterfall_pos 0, 16, mid-ring and wf_rows - 16 (the
    position moves in steps of 16 spectra), moved by processing that many spectra and planting again; rows = 1, wf_rows - 1, wf_rows"""
    import torch
    s, n = ring256, ring256.n
    seen = []
    first = None
    for advance in (0, 16, 112, 112):						# positions 0, 16, 128, 240
        if advance:
            d_x = torch.from_numpy(gaussian_iq(advance * n, 40 + advance)).cuda()
            assert s.f.process_device(d_x, 1, advance) == 0
        s.plant(ys=s.ys)
        seen.append(s.pos)
        for rows in (1, 255, 256):
            want = check_rows(s, s.ys, s.up, s.lo, 3, n - 7, rows, "both", "pos=%d rows=%d" % (s.pos, rows))
            if rows == 256:
                first = want if first is None else first
                mm.assert_rows_equal(want, first)
        s.assert_untouched()
    assert seen == [0, 16, 128, 240]


def test_trigger_and_event_list(ring256):
    """4. min_cols 1, 2 and a value no row reaches; triggered rows at j = 0, 63, 64, 255; every row; none; max_events below
    n_triggered; d_rows NULL with events wanted, and the reverse"""
    s, n = ring256, ring256.n
    up = np.full(n, 1.0, np.float32)
    quiet = np.zeros((256, n), np.float32)
    ys = quiet.copy()
    for j, k in ((0, 1), (63, 2), (64, 3), (255, 2), (100, 1)):			# k columns over on row j
        ys[j, 40:40 + k] = 2.0
    s.plant(ys=ys)
    for min_cols, expect in ((1, [0, 63, 64, 100, 255]), (2, [63, 64, 255]), (3, [64]), (4, [])):
        wrows = mm.rows_rule(ys, up, None, 0, n)
        wres, wev = mm.events(wrows, min_cols, 16)
        assert wev.tolist() == expect
        o = s.scan(0, n, 256, min_cols=min_cols, upper=up, max_events=16)
        assert o["rv"] == 0
        assert_result(o["result"], wres, "min_cols=%d" % min_cols)
        assert o["events"][:len(expect)].tolist() == expect
        mm.assert_rows_equal(o["rows"], wrows)
        if not expect:
            assert int(o["result"]["newest"]) == -1 and int(o["result"]["oldest"]) == -1 and np.all(o["events"] == SENTINEL)
    # max_events smaller than n_triggered: the first max_events in ascending order, the rest of the buffer still sentinel
    o = s.scan(0, n, 256, upper=up, max_events=2, alloc_events=8)
    assert o["rv"] == 0 and (int(o["result"]["n_triggered"]), int(o["result"]["n_written"])) == (5, 2)
    assert o["events"][:2].tolist() == [0, 63] and np.all(o["events"][2:] == SENTINEL)
    assert (int(o["result"]["newest"]), int(o["result"]["oldest"])) == (0, 255)
    # fewer rows than the ring holds: j = 255 is not scanned
    o = s.scan(0, n, 255, upper=up, max_events=16)
    assert o["rv"] == 0 and o["events"][:4].tolist() == [0, 63, 64, 100] and int(o["result"]["oldest"]) == 100
    # d_rows NULL with events wanted, and the reverse
    o = s.scan(0, n, 256, upper=up, max_events=16, want_rows=False)
    assert o["rv"] == 0 and o["events"][:5].tolist() == [0, 63, 64, 100, 255] and np.all(o["raw"]["rows"] == SENTINEL)
    o = s.scan(0, n, 256, upper=up, max_events=0)
    assert o["rv"] == 0 and int(o["result"]["n_triggered"]) == 5 and int(o["result"]["n_written"]) == 0 and np.all(o["events"] == SENTINEL)
    mm.assert_rows_equal(o["rows"], mm.rows_rule(ys, up, None, 0, n))
    s.assert_untouched()
    # every row triggered, under a lower limit this time
    s.plant(ys=np.full((256, n), -3.0, np.float32))
    o = s.scan(17, 100, 256, min_cols=100, lower=np.full(n, -1.0, np.float32), max_events=256)
    assert o["rv"] == 0 and (int(o["result"]["n_triggered"]), int(o["result"]["n_written"])) == (256, 256)
    assert np.array_equal(o["events"][:256], np.arange(256)) and (int(o["result"]["newest"]), int(o["result"]["oldest"])) == (0, 255)
    assert np.all(o["rows"]["n_under"] == 100) and np.all(o["rows"]["first_col"] == 17) and np.all(o["rows"]["last_col"] == 116)
    s.assert_untouched()


# ---- several rows per work-group: wf_rows 8192 ---------------------------------------------------------------------------------

def test_several_rows_per_work_group(amd):
    """1024 points, 8191 and 8192 rows: rpg = 7 and 8, so a work-group loads its rows 4 at a time with a tail of 3 and of 0, and
    the last work-group of 8191 rows has a single row; the event list gives a lane 8 rows.  Records exact, powers within 5e-5."""
    s = Ring(amd, 10, 8192)
    n = s.n
    rng = np.random.default_rng(9)
    up = (1.0 + 0.2 * rng.random(n)).astype(np.float32)
    lo = (-1.0 - 0.2 * rng.random(n)).astype(np.float32)
    ys = (rng.random((8192, n)) - 0.5).astype(np.float32)
    hit = rng.random(8192) < 0.3							# a third of the rows violate, each in its own columns
    for j in np.flatnonzero(hit):
        k = rng.integers(0, n, 4)
        ys[j, k[:2]] = up[k[:2]] + np.float32(0.5)					# a tied excess where the limits are equal bits
        ys[j, k[2]] = lo[k[2]] - np.float32(0.25)
        ys[j, k[3]] = np.nan
    ys[[0, 6, 7, 8, 8183, 8184, 8189, 8190, 8191], 5] = 9.0				# both sides of the first and last row groups
    s.plant(ys=ys)
    chans = [(0, n - 1), (500, 520)]
    for rows in (8191, 8192):
        before = s.f.mask_stats()
        o = s.scan(2, n - 3, rows, upper=up, lower=lo, channels=chans, max_events=65536, alloc_events=8200)
        assert o["rv"] == 0
        want = mm.rows_rule(ys[:rows], up, lo, 2, n - 3)
        mm.assert_rows_equal(o["rows"], want, "rows=%d" % rows)
        wres, wev = mm.events(want, 1, 65536)
        assert_result(o["result"], wres)
        assert np.array_equal(o["events"][:wev.size], wev) and wev.size > 2000
        err = mm.power_error(o["power"], mm.channel_power(ys[:rows], chans))
        print("rows=%d: worst |power error| %.3g" % (rows, err))
        assert err <= 5e-5
        after = s.f.mask_stats()
        assert after["form_rows"] - before["form_rows"] == 2 and after["form_shared"] == before["form_shared"]	# (0, n - 1) is outside the window
    s.assert_untouched()
    s.f.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------

E2E_TONE = 100 / 1024.0		# a bin centre: shifted column 612


def e2e_input(n_spec, seed, burst=None):
    """Gaussian IQ of sigma 0.05, and a tone of amplitude 0.5 added to the whole spectra burst[0] .. burst[1] - 1 only"""
    x = gaussian_iq(n_spec * 1024, seed)
    if burst:
        a, b = burst
        x[a * 1024:b * 1024] = add_tone(x[a * 1024:b * 1024], 0.5, E2E_TONE, phase0=0.3, t0=a * 1024)
    return x


def test_end_to_end_burst(amd):
    """8. 1024 points, wf_rows 64: 48 spectra with a tone in spectra 20 .. 23, upper = a constant line at y = 1.8, min_cols 1.
    Checked on the CPU with the oracle when this test was written, and again below on every run: no noise cell exceeds y = 0.94
    (bound asserted: 1.5), the tone's peak is y = 2.71 in each of its four rows (bound asserted: 2.1), its side lobes stay below
    0.9.  The records are compared with the model applied to the device's own waterfall, bit for bit; the oracle's floats agree to
    1e-4 only and decide no comparison.  With a mask learnt from the max-hold of noise (6 dB, spread 2) the oracle puts the
    greatest noise cell 0.19 below the line and the burst 1.6 above it."""
    import torch
    x = e2e_input(48, 900, (20, 24))
    o = Oracle(n_bins=128, wf_rows=64)
    assert o.process(x) == 0 and o.waterfall_pos == 48
    oy = mm.newest_first(o.waterfall, 48)
    assert np.delete(oy[:48], [24, 25, 26, 27], axis=0).max() < 1.5 and np.all(oy[24:28].max(axis=1) > 2.1)

    f = amd.Fosphor(n_bins=128, wf_rows=64)
    n = f.n
    up = np.full(n, 1.8, np.float32)
    d_up = torch.from_numpy(up).cuda()

    def scan_and_check(expect):
        res, rows, events, _ = f.mask_scan(upper=d_up, min_cols=1, max_events=64)
        ys = mm.newest_first(f.waterfall, f.waterfall_pos)
        want = mm.rows_rule(ys, up, None, 0, n)
        mm.assert_rows_equal(rows, want)
        wres, wev = mm.events(want, 1, 64)
        assert res == {k: int(wres[k]) for k in mm.RESULT_DTYPE.names} and np.array_equal(events, wev)
        assert events.tolist() == expect, (events.tolist(), expect)
        return rows

    assert f.process_device(torch.from_numpy(x).cuda(), 1, 48) == 0
    rows = scan_and_check([24, 25, 26, 27])
    assert f.waterfall_pos == 48 and np.all(rows["peak_col"][24:28] == 612)
    assert f.process_device(torch.from_numpy(e2e_input(32, 901)).cuda(), 1, 32) == 0		# the ring wraps
    scan_and_check([56, 57, 58, 59])
    assert f.waterfall_pos == 16
    assert f.process_device(torch.from_numpy(e2e_input(64, 902)).cuda(), 1, 64) == 0		# every row rewritten: the other ring
    scan_and_check([])
    f.close()

    # learn the mask from noise, arm it, feed the burst
    f = amd.Fosphor(n_bins=128, wf_rows=64)
    assert f.process_device(torch.from_numpy(e2e_input(48, 903)).cuda(), 1, 48) == 0
    d_learnt = f.mask_from_trace("maxhold", margin_db=6, spread_cols=2)
    learnt = d_learnt.cpu().numpy()
    assert mm.same_bits(learnt, mm.from_trace(f.spectrum[1, :, 1], np.float32(6 / 20.0), 2))
    res, rows, events, _ = f.mask_scan(upper=d_learnt, rows=48, max_events=64)
    assert res["n_triggered"] == 0 and events.size == 0
    assert f.process_device(torch.from_numpy(e2e_input(16, 904, (4, 8))).cuda(), 1, 16) == 0
    res, rows, events, _ = f.mask_scan(upper=d_learnt, max_events=64)			# the burst: spectra 4 .. 7 of 16, j = 11 .. 8
    mm.assert_rows_equal(rows, mm.rows_rule(mm.newest_first(f.waterfall, f.waterfall_pos), learnt, None, 0, n))
    assert events.tolist() == [8, 9, 10, 11] and np.all(rows["peak_col"][8:12] == 612)
    f.close()
