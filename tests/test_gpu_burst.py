"""Bursts on the device (include/fosphor_amd_burst.h) against the numpy statement (tests/burst_model.py), by the method of
tests/test_gpu_mask.py: ys are planted straight into the waterfall ring, outputs go into sentinel-filled buffers with guard entries
behind the specified extents, and every planted test ends by checking that the ring and the spectrum are bit-identical.

Geometries: (1024 points, wf_rows 16); (1024 points, wf_rows 256) for the ring position (0, 16, 240 and mid-ring: it moves in steps
of 16 spectra); (65536 points, 512 bins, wf_rows 16, max_spectra 16), a 4 MiB ring, for every multi-strip seam.  The run kernel
gives a work-group one strip of one row at every shape, so there is no several-rows-per-work-group geometry to test.

Seams of the kernels, all counted from a = first column of the call & ~3:
  k_burst_runs    a lane owns the aligned group of 4 columns a + 4k (one 16-byte load; the groups the window cuts at its head and
                  tail load column by column), a wave 256 columns, a work-group a strip of FOSPHOR_AMD_BURST_STRIP = 1024 columns;
                  more than one strip only at 65536 points.  Memory columns wrap at shifted column N/2.  The nearest on cell before
                  and after a cell is looked for in the lane, the wave, the work-group and the row's other strips in turn; a run is
                  summed inside a wave and joined across waves and strips by atomics.
  k_burst_rows    one lane per strip, up to 64.
  k_burst_scan    lane t of 1024 owns the rows [t * chunk, (t + 1) * chunk), chunk = ceil(rows / 1024) = 1 here.
  k_burst_link / k_burst_reduce  one lane per run, work-groups of 256 runs.
  k_burst_emit    lane t of 1024 owns ceil(n_runs / 1024) consecutive runs: more than one from 1025 runs on (the random fields, the
                  checkerboards).
energy_y is compared within 5e-5 absolute, the tolerance of the mask and detect tests for the same quantity; everything else with
equality."""
import ctypes as C
import errno
import os

import numpy as np
import pytest

import burst_model as bm
import mask_model as mm
from oracle_lib import gaussian_iq, add_tone

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a5a5a5a
TOL = 5e-5
REC = bm.BURST_DTYPE.itemsize // 4


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Ring:
    """an instance, torch views of its waterfall ring [wf_rows][N] and spectrum, and what was planted"""

    def __init__(self, amd, log, wf_rows):
        if log == 10:
            self.f = amd.Fosphor(n_bins=128, wf_rows=wf_rows)
        else:
            self.f = amd.Fosphor(fft_len_log=log, n_bins=512, wf_rows=wf_rows, max_spectra=16)
        self.n, self.wf_rows, self.lib = self.f.n, wf_rows, amd._lib
        assert self.f.finish() >= 0			# a new instance fills its buffers at its first wait: before anything is planted
        self.saved = None

    def views(self):
        import torch
        from gr_fosphor_amd.dist import wrap_device_array
        b = self.f.buffers(False)
        assert (b.fft_len, b.wf_rows) == (self.n, self.wf_rows)
        self.pos = b.waterfall_pos
        self.wf = wrap_device_array(b.d_waterfall, (self.wf_rows, self.n), torch.float32)
        self.spec = wrap_device_array(b.d_spectrum, (2, self.n, 2), torch.float32)

    def plant(self, ys):
        """ys: [wf_rows][N] by source index j (0 = newest) and shifted column"""
        import torch
        assert self.f.finish() >= 0
        self.views()
        ys = np.asarray(ys, np.float32)
        mem = np.empty((self.wf_rows, self.n), np.float32)
        mem[(self.pos - 1 - np.arange(self.wf_rows)) % self.wf_rows] = mm.shift(ys)
        assert mm.same_bits(mm.newest_first(mem, self.pos), ys)
        self.wf.copy_(torch.from_numpy(mem))
        torch.cuda.synchronize()
        self.ys = ys
        self.saved = (self.wf.view(torch.int32).clone(), self.spec.view(torch.int32).clone(), self.pos)

    def assert_untouched(self):
        import torch
        torch.cuda.synchronize()
        self.views()
        assert self.pos == self.saved[2], "the ring position moved"
        assert torch.equal(self.wf.view(torch.int32), self.saved[0]), "the waterfall was written"
        assert torch.equal(self.spec.view(torch.int32), self.saved[1]), "the spectrum lines were written"

    def call(self, thr, first_bin=0, n_cols=None, rows=None, max_gap_cols=0, max_gap_rows=0, min_rows=1, min_cols=1,
             max_bursts=4096, max_runs=1 << 20, null=()):
        """fosphor_amd_bursts through the C ABI into sentinel-filled buffers with guard entries behind the specified extents.
        thr: a scalar (cfg->threshold_y, d_threshold NULL) or an array [N]"""
        import torch
        n_cols = self.n - first_bin if n_cols is None else n_cols
        rows = self.wf_rows if rows is None else rows
        scalar = np.ndim(thr) == 0
        d_thr = None if scalar else torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float32)).cuda()
        cfg = self.lib.BurstCfg(first_bin, n_cols, rows, float(thr) if scalar else 0.0, max_gap_cols, max_gap_rows, min_rows,
                                min_cols, max_runs)
        cap = min(max(max_bursts, 1), 65536)
        d_res = torch.full((5 + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        d_out = torch.full(((cap + 2) * REC,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()			# the fills and the upload run on torch's stream, the pass on the instance's
        rv = self.f.L.fosphor_amd_bursts(None if "self" in null else self.f.h, None if "cfg" in null else C.byref(cfg),
                                         None if d_thr is None else d_thr.data_ptr(), None if "res" in null else d_res.data_ptr(),
                                         None if "out" in null else d_out.data_ptr(), max_bursts)
        raw_res, raw_out = d_res.cpu().numpy(), d_out.cpu().numpy()
        assert np.all(raw_res[5:] == SENTINEL), "behind the result"
        if rv != 0:
            return rv, raw_res, raw_out
        res = dict(zip(bm.RESULT_NAMES, raw_res[:5].tolist()))
        nw = res["n_written"]
        assert 0 <= nw <= cap and np.all(raw_out[nw * REC:] == SENTINEL), "entries behind n_written are not written"
        return rv, res, raw_out[:nw * REC].copy().view(bm.BURST_DTYPE)

    def check(self, thr, tag="", **kw):
        """the device against the model on what was planted; returns (result, records)"""
        first_bin = kw.get("first_bin", 0)
        n_cols = kw.get("n_cols") or self.n - first_bin
        rows = kw.get("rows") or self.wf_rows
        win = slice(first_bin, first_bin + n_cols)
        mkw = {k: v for k, v in kw.items() if k not in ("n_cols", "rows")}
        mkw.setdefault("max_bursts", 4096)
        want_res, want = bm.bursts(self.ys[:rows, win], thr if np.ndim(thr) == 0 else np.asarray(thr, np.float32)[win], **mkw)
        before = self.f.burst_stats()
        rv, res, got = self.call(thr, **kw)
        assert rv == 0, tag
        bm.assert_result_equal(res, want_res, tag)
        bm.assert_bursts_equal(got, want, TOL, tag)
        after = self.f.burst_stats()
        full = 0 if (want_res["overflow"] or want_res["n_runs"] == 0) else 1
        delta = {k: after[k] - before[k] for k in after}
        assert delta == dict(calls=1, overflows=want_res["overflow"], k_count=1, k_rows=1, k_scan=1, k_init=full, k_write=full,
                             k_link=full, k_reduce=full, k_emit=full), (tag, delta)
        return res, got


def windows_of(n):
    """(first_bin, n_cols): the whole width; first_bin odd with an odd n_cols; straddling N/2; a head and tail cut inside a 16-byte
    group with the strips moved off the multiples of 1024"""
    h = n // 2
    return [(0, n), (5, n - 5 - 6), (h - 301, 603), (259, min(n - 259 - 2, 2301))]


def seams_of(n, first_bin, n_cols):
    """columns c inside the window at which a lane group, a wave, a strip or the memory wrap begins"""
    a = first_bin & ~3
    cols = [a + 4, a + 8, n // 2] + list(range(a + 256, first_bin + n_cols, 256))
    return sorted(set(c for c in cols if first_bin + 4 <= c <= first_bin + n_cols - 4))


GEOS = {"N1024_rows16": (10, 16), "N65536_rows16": (16, 16)}


@pytest.fixture(scope="module", params=list(GEOS), ids=list(GEOS))
def ring(request, amd):
    log, wf_rows = GEOS[request.param]
    s = Ring(amd, log, wf_rows)
    yield s
    s.f.close()


@pytest.fixture(scope="module")
def ring256(amd):
    s = Ring(amd, 10, 256)
    yield s
    s.f.close()


def test_degenerate_fields(ring):
    """nothing on: every count 0.  Everything on: one burst of rows x n_cols cells with all four flags, its runs joined across every
    lane, wave, work-group and strip seam."""
    s, n, rows = ring, ring.n, ring.wf_rows
    rng = np.random.default_rng(1)
    s.plant(rng.random((rows, n)).astype(np.float32))
    for first_bin, n_cols in windows_of(n):
        res, got = s.check(2.0, "nothing on", first_bin=first_bin, n_cols=n_cols)
        assert res == dict(n_runs=0, n_components=0, n_found=0, n_written=0, overflow=0)
        res, got = s.check(-1.0, "everything on", first_bin=first_bin, n_cols=n_cols)
        assert res == dict(n_runs=rows, n_components=1, n_found=1, n_written=1, overflow=0)
        assert got["n_cells"][0] == rows * n_cols and got["flags"][0] == 15
        assert (got["first_col"][0], got["last_col"][0], got["newest"][0], got["oldest"][0]) == (first_bin, first_bin + n_cols - 1, 0, rows - 1)
        res, got = s.check(-1.0, "one row", first_bin=first_bin, n_cols=n_cols, rows=1)
        assert got["n_cells"][0] == n_cols and got["flags"][0] == 15
    # through the Python class: a float, an array, a device tensor
    import torch
    thr = np.full(n, -1.0, np.float32)
    for t in (-1.0, thr, torch.from_numpy(thr).cuda()):
        res, recs = s.f.bursts(t, first_bin=5, n_cols=n - 11)
        assert res["n_found"] == 1 and recs["n_cells"][0] == rows * (n - 11) and recs.dtype == bm.BURST_DTYPE
    s.assert_untouched()


def shapes_field(rows, n, base):
    """on cells of the four union-find shapes, each `rows` tall, from column `base` on; returns the bool field"""
    on = np.zeros((rows, n), bool)
    R = rows
    c = base						# two vertical bars that join only in the oldest row
    on[:, c] = on[:, c + 2] = True
    on[R - 1, c:c + 3] = True
    c = base + 6					# a comb of 64 teeth on a bottom bar
    for t in range(64):
        on[:R - 1, c + 2 * t] = True
    on[R - 1, c:c + 127] = True
    c = base + 136					# a serpentine: its root, the run of row 0, is one end; the other is the oldest row
    for j in range(0, R, 2):
        on[j, c:c + 40] = True
    for j in range(1, R, 2):
        on[j, c + 39 if (j // 2) % 2 == 0 else c] = True
    c = base + 180					# two components that interleave without touching
    on[0, c:c + 41] = True
    for t in range(0, 41, 4):
        on[1:R - 2, c + t] = True
    on[R - 1, c:c + 41] = True
    for t in range(2, 41, 4):
        on[2:R - 1, c + t] = True
    return on


def field_from(on, seed):
    """ys for a bool field: on cells 2 + noise (a unique peak), the others below the threshold 1"""
    rng = np.random.default_rng(seed)
    return np.where(on, 2.0 + rng.random(on.shape), 0.5 * rng.random(on.shape)).astype(np.float32)


def test_union_find_shapes(ring):
    """the four shapes across the wave seams, the strip seam and N/2, at 16 rows"""
    s, n, rows = ring, ring.n, ring.wf_rows
    bases = [3, n // 2 - 100] + ([1024 - 90, 2048 - 150] if n > 1024 else [])
    on = np.zeros((rows, n), bool)
    for b in bases:
        on |= shapes_field(rows, n, b)
    s.plant(field_from(on, 2))
    res, got = s.check(1.0, "shapes")
    assert res["n_components"] == 5 * len(bases)
    for kw in (dict(max_gap_cols=1), dict(max_gap_rows=1), dict(first_bin=7, n_cols=n - 16, max_gap_cols=3, max_gap_rows=2)):
        s.check(1.0, "shapes %s" % kw, **kw)
    s.assert_untouched()


def test_union_find_shapes_where_the_ring_wraps(ring256, amd):
    """256 rows, ring positions 0, 16, 128 and 240 (so j wraps the ring's end inside every shape): the same planted field gives the
    same records"""
    import torch
    s, n = ring256, ring256.n
    on = shapes_field(256, n, 3) | shapes_field(256, n, n // 2 - 100)
    ys = field_from(on, 3)
    seen, first = [], None
    for advance in (0, 16, 112, 112):
        if advance:
            d_x = torch.from_numpy(gaussian_iq(advance * n, 40 + advance)).cuda()
            assert s.f.process_device(d_x, 1, advance) == 0
        s.plant(ys)
        seen.append(s.pos)
        res, got = s.check(1.0, "pos=%d" % s.pos)
        assert res["n_components"] == 10 and res["n_runs"] > 1024
        first = got if first is None else first
        bm.assert_bursts_equal(got, first, TOL)
        for rows in (1, 255):
            s.check(1.0, "pos=%d rows=%d" % (s.pos, rows), rows=rows, max_gap_rows=1)
        s.assert_untouched()
    assert seen == [0, 16, 128, 240]


def test_connectivity(ring):
    """checkerboard: every cell its own component, n_runs half the cells; with max_gap_cols = 1 the rows become runs and it is one
    component.  A diagonal staircase is not linked; one with a column of overlap is."""
    s, n, rows = ring, ring.n, ring.wf_rows
    jj, ii = np.meshgrid(np.arange(rows), np.arange(n), indexing="ij")
    s.plant(field_from((jj + ii) % 2 == 0, 4))
    first_bin, n_cols = (0, n) if n == 1024 else (1021, 2052)		# the model's time, not the device's, bounds the large one
    res, got = s.check(1.0, "checkerboard", first_bin=first_bin, n_cols=n_cols, max_bursts=65536)
    assert res["n_runs"] == res["n_components"] == res["n_found"] == rows * n_cols // 2 and np.all(got["n_cells"] == 1)
    res, got = s.check(1.0, "checkerboard, gap 1", first_bin=first_bin, n_cols=n_cols, max_gap_cols=1)
    assert (res["n_runs"], res["n_components"]) == (rows, 1) and got["n_cells"][0] == rows * (n_cols - 1)
    rv, res, got = s.call(1.0, max_gap_cols=1)				# the whole width on the device alone
    assert rv == 0 and (res["n_runs"], res["n_components"]) == (rows, 1) and got["n_cells"][0] == rows * (n - 1)
    on = np.zeros((rows, n), bool)
    for c in (40, n // 2 - 7, 1024 - 9 if n > 1024 else 250):
        for j in range(rows):
            on[j, c + j] = True						# diagonal: corners touch, nothing is linked
            on[j, c + 100 + 2 * j:c + 100 + 2 * j + 3] = True		# one column of overlap: linked
    s.plant(field_from(on, 5))
    res, got = s.check(1.0, "staircases")
    assert res["n_components"] == 3 * (rows + 1) and sorted(got["n_cells"].tolist())[-3:] == [3 * rows] * 3
    s.assert_untouched()


def test_gaps_and_seams(ring):
    """runs and gaps across every seam of every window: at each seam column c a run c - 3 .. c + 2, and on cells at c - 2 and c + 1
    (a gap of 2 across the seam) seen with max_gap_cols 1, 2 and 3; row gaps of exactly max_gap_rows and one more; a gap at the
    window's edge, which is not closed because the on cell beyond it is outside"""
    s, n, rows = ring, ring.n, ring.wf_rows
    for first_bin, n_cols in windows_of(n):
        on = np.zeros((rows, n), bool)
        last = first_bin + n_cols - 1
        for c in seams_of(n, first_bin, n_cols):
            on[1, c - 3:c + 3] = True
            on[3, [c - 2, c + 1]] = True
            on[5, [c - 3, c + 1]] = True					# a gap of 3
            on[8, c - 1:c + 1] = True						# rows 8 and 11: a row gap of 2; rows 11 and 15: of 3
            on[11, c - 1:c + 1] = True
            on[15, c - 1:c + 1] = True
        if first_bin > 0:
            on[7, [first_bin - 1, first_bin + 2]] = True			# the gap first_bin .. first_bin + 1 touches the edge
        if last < n - 1:
            on[7, [last - 2, last + 1]] = True
        on[9, [first_bin, first_bin + 3, last - 3, last]] = True		# gaps just inside the edges are closed
        s.plant(field_from(on, 6))
        for gc, gr in ((0, 0), (1, 1), (2, 2), (3, 3), (2, 7)):
            res, got = s.check(1.0, "window=(%d, %d) gaps=(%d, %d)" % (first_bin, n_cols, gc, gr), first_bin=first_bin, n_cols=n_cols,
                               max_gap_cols=gc, max_gap_rows=gr)
            assert res["n_found"] > 0
    # one very long gap across every strip: closed by max_gap_cols >= its length only
    on = np.zeros((rows, n), bool)
    on[2, [10, n - 10]] = True
    on[4, [10, n // 2 + 3]] = True
    s.plant(field_from(on, 7))
    for gc in (n // 2 - 8, n // 2 - 9, n - 21, n - 22, 1 << 30):
        s.check(1.0, "long gap %d" % gc, max_gap_cols=gc)
    s.assert_untouched()


def test_values(ring):
    """equality with the threshold, NaN and +-inf cells, a NaN and a +inf threshold column, peak ties within a row and across rows,
    -0 against +0, and a burst whose closed-gap cells are -inf and NaN"""
    s, n, rows = ring, ring.n, ring.wf_rows
    N, I = np.nan, np.inf
    rng = np.random.default_rng(8)
    thr = (1.0 + 0.1 * rng.random(n)).astype(np.float32)
    ys = (0.5 * rng.random((rows, n))).astype(np.float32)
    h = n // 2
    ys[0, 20:24] = thr[20:24]						# equality is not on
    ys[0, 30:34] = [N, I, -I, 3.0]
    thr[40], thr[41] = N, I
    ys[1, 38:44] = [3.0, 3.0, 9.0, I, 3.0, 3.0]				# columns 40 and 41 are never on
    ys[2:5, h - 2:h + 2] = 4.0						# a tie in every cell: the peak is (2, h - 2)
    ys[3, h + 1] = 5.0
    ys[4, h - 1] = 5.0							# a tie across rows: (3, h + 1)
    ys[6, 255:258] = [3.0, -I, 3.0]					# closed gaps of -inf and NaN, across the wave seam
    ys[7, 254:259] = [3.0, N, N, -I, 3.0]
    ys[9, 500:504] = [3.0, N, I, 3.0]					# a NaN inside a run that has +inf as its peak; the energy skips both
    thr[600:604] = -1.0
    ys[:, 600:604] = N							# a threshold below 0 here, and no other row is on under it
    ys[10, 600:604] = [-0.0, 0.0, -0.0, -0.5]				# -0 and +0 tie: the smallest column
    s.plant(ys)
    for kw in (dict(), dict(max_gap_cols=1), dict(max_gap_cols=3, max_gap_rows=1), dict(first_bin=31, n_cols=n - 40, max_gap_cols=3)):
        s.check(thr, "values %s" % kw, **kw)
    res, got = s.check(thr, "values", max_gap_cols=3)
    by = {(int(b["newest"]), int(b["first_col"])): b for b in got}
    assert (by[(2, h - 2)]["peak_row"], by[(2, h - 2)]["peak_col"]) == (3, h + 1)
    b = by[(6, 254)]
    assert (b["n_cells"], b["oldest"], b["peak_y"]) == (8, 7, 3.0) and abs(b["energy_y"] - 0.5 * np.log10(4e6)) < TOL
    assert by[(9, 500)]["peak_y"] == I and (by[(9, 500)]["peak_col"], by[(9, 500)]["n_cells"]) == (502, 4)
    assert abs(by[(9, 500)]["energy_y"] - 0.5 * np.log10(2e6)) < TOL
    assert (by[(10, 600)]["peak_col"], by[(10, 600)]["peak_y"], by[(10, 600)]["n_cells"]) == (600, 0.0, 4)
    s.assert_untouched()


def test_filters_and_overflow(ring):
    s, n, rows = ring, ring.n, ring.wf_rows
    on = np.zeros((rows, n), bool)
    on[2:7, 100:109] = True						# 5 rows x 9 columns
    on[3:5, n // 2 - 2:n // 2 + 2] = True				# 2 x 4
    on[10, 7] = True
    on[12, n - 300:n - 100] = True
    s.plant(field_from(on, 9))
    for min_rows, min_cols, expect in ((5, 9, 1), (6, 9, 0), (5, 10, 0), (2, 4, 2), (1, 1, 4), (1, 200, 1), (1, 201, 0)):
        res, got = s.check(1.0, "filters", min_rows=min_rows, min_cols=min_cols)
        assert (res["n_components"], res["n_found"]) == (4, expect)
    # max_bursts one below n_found: guards intact (Ring.call checks them), order ascending
    full_res, full = s.check(1.0)
    res, got = s.check(1.0, "max_bursts", max_bursts=3)
    assert (res["n_found"], res["n_written"]) == (4, 3) and np.all(np.diff(got["newest"]) >= 0)
    bm.assert_bursts_equal(got, full[:3], TOL)
    # max_runs at and one below n_runs
    assert full_res["n_runs"] == 5 + 2 + 1 + 1
    s.check(1.0, "max_runs fits", max_runs=9)
    res, got = s.check(1.0, "max_runs overflows", max_runs=8)
    assert res == dict(n_runs=9, n_components=0, n_found=0, n_written=0, overflow=1) and got.size == 0
    with pytest.raises(RuntimeError):
        s.f.bursts(1.0, max_gap_rows=8)
    s.assert_untouched()


@pytest.mark.parametrize("density,gap", [(0.3, 0), (0.3, 2), (0.6, 0), (0.6, 2)])
def test_random_fields(ring, density, gap):
    """the full ring, uniform ys against a threshold that leaves `density` of the cells on, NaN and +-inf cells, a NaN threshold
    column; 0.6 is above the site-percolation threshold: large, tortuous components"""
    s, n, rows = ring, ring.n, ring.wf_rows
    rng = np.random.default_rng(int(density * 10) + gap)
    ys = rng.random((rows, n)).astype(np.float32)
    k = rng.integers(0, rows * n, 60)
    ys.reshape(-1)[k[:20]], ys.reshape(-1)[k[20:40]], ys.reshape(-1)[k[40:]] = np.nan, np.inf, -np.inf
    thr = np.full(n, 1.0 - density, np.float32)
    thr[rng.integers(0, n, 4)] = np.nan
    s.plant(ys)
    res, got = s.check(thr, "random %g gap %d" % (density, gap), max_gap_cols=gap, max_gap_rows=gap, max_bursts=65536)
    assert res["n_runs"] > 8 * rows and res["n_components"] >= 1
    s.check(thr, "random, window", first_bin=n // 2 - 333, n_cols=777, max_gap_cols=gap, max_gap_rows=gap, min_rows=2, min_cols=2)
    s.assert_untouched()


def test_einval_writes_nothing(ring):
    """every listed cause, against sentinel-filled outputs; no call reaches the device"""
    s, n = ring, ring.n
    s.plant(np.zeros((s.wf_rows, n), np.float32))
    good = dict(first_bin=10, n_cols=500, rows=4, max_gap_cols=1, max_gap_rows=7, min_rows=1, min_cols=1, max_bursts=8, max_runs=64)
    bad = [dict(first_bin=-1), dict(first_bin=n), dict(n_cols=0), dict(n_cols=n - 9), dict(first_bin=0, n_cols=n + 1),
           dict(rows=0), dict(rows=-2), dict(rows=s.wf_rows + 1),
           dict(max_gap_cols=-1), dict(max_gap_rows=-1), dict(max_gap_rows=8), dict(min_rows=0), dict(min_cols=0),
           dict(max_runs=0), dict(max_runs=(1 << 20) + 1), dict(max_bursts=0), dict(max_bursts=-1), dict(max_bursts=65537),
           dict(null=("self",)), dict(null=("cfg",)), dict(null=("res",)), dict(null=("out",))]
    before = s.f.burst_stats()
    for change in bad:
        rv, raw_res, raw_out = s.call(1.0, **dict(good, **change))
        assert rv == -errno.EINVAL, change
        assert np.all(raw_res == SENTINEL) and np.all(raw_out == SENTINEL), change
    assert s.f.burst_stats() == before
    rv, res, got = s.call(1.0, **good)
    assert rv == 0 and res["n_runs"] == 0
    assert s.f.burst_stats()["calls"] == before["calls"] + 1
    s.assert_untouched()


TONE = 100 / 1024.0		# a bin centre: shifted column 612


def test_whole_path(amd):
    """1024 points, 256 rows: 128 spectra of noise, then noise plus a tone for 3 calls of 16 spectra, then 16 of noise.  The threshold
    is the live trace of the quiet state plus 20 dB (y + 1: mask_from_trace("live")); the device's records equal the model applied to
    the read-back waterfall, and exactly one burst with min_rows = 32 holds the tone's column: 48 rows, j = 16 .. 63.
    alpha is 0.05, as in the detect test: the live line is then an average over about 20 spectra and has settled on the noise after
    128 (with the Python class's alpha = 0 it never leaves the bottom of the power range).  Gaussian IQ of sigma 0.05 gives |X| an
    rms of 2.26, y = 0.35; of the 200 000 noise cells the greatest is expected near y = 0.9 (the mask test met 0.94), the line
    stands at 1.2 to 1.35, and the tone, on a bin centre, peaks at y = 2.71 with side lobes below 0.9."""
    import torch
    f = amd.Fosphor(n_bins=128, wf_rows=256, alpha=0.05)
    n = f.n
    feed = lambda x, count: f.process_device(torch.from_numpy(x).cuda(), 1, count)
    assert feed(gaussian_iq(128 * n, 700), 128) == 0
    d_thr = f.mask_from_trace("live", margin_db=20.0, spread_cols=0)
    thr = d_thr.cpu().numpy()
    t0 = 128
    for call in range(3):
        x = gaussian_iq(16 * n, 701 + call)
        x = add_tone(x, 0.5, TONE, phase0=0.3, t0=t0 * n)
        assert feed(x, 16) == 0
        t0 += 16
    assert feed(gaussian_iq(16 * n, 710), 16) == 0
    print("threshold y: min %.3f max %.3f; waterfall max %.3f" % (thr.min(), thr.max(), f.waterfall.max()))
    assert f.waterfall_pos == 192 and 1.0 < thr.min() and thr.max() < 1.6
    ys = mm.newest_first(f.waterfall, f.waterfall_pos)
    for kw in (dict(), dict(min_rows=32), dict(max_gap_cols=2, max_gap_rows=1, min_rows=32)):
        want_res, want = bm.bursts(ys, thr, max_bursts=1024, **kw)
        res, got = f.bursts(d_thr, **kw)
        bm.assert_result_equal(res, want_res, kw)
        bm.assert_bursts_equal(got, want, TOL, kw)
    res, got = f.bursts(d_thr, min_rows=32)
    hit = got[(got["first_col"] <= 612) & (got["last_col"] >= 612)]
    assert len(hit) == 1 and (hit["newest"][0], hit["oldest"][0], hit["peak_col"][0]) == (16, 63, 612), got
    assert hit["flags"][0] == 0 and res["n_found"] == 1
    st = f.burst_stats()
    assert st["calls"] == 4 and st["k_emit"] == 4 and st["overflows"] == 0
    f.close()
