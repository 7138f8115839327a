"""The read-only passes over the waterfall ring (gr-fosphor_amd/csrc/fosphor_ring.h) on one instance and one window: mask_scan,
bursts, view and detect against numpy over the host copy of the ring.  The counterpart of tests/test_gpu_job_tables.py: the
single-module tests hold each pass's own seams; what is new here is that the four read the same window of the same ring, at the
smallest shapes at which the shared read can go wrong.

  n1024     N = 1024, wf_rows 8, window [509, 519): one strip (the ROWS form), head and tail groups both cut, astride the N/2 wrap
  n8192     N = 8192, wf_rows 4, window [4093, 6147): three strips (the SHARED form), head cut to 3 of 4 columns, tail cut, the first
            strip begins one group before the wrap
  n1024_pos the window of n1024 on a ring of 64 rows after 80 spectra: the ring has wrapped and stands at row 16.  Spectra come in
            multiples of 16, so a ring of 8 or 4 rows always stands at row 0 after a call; this shape is here for a position that is
            not 0, and asserts it.

Noise of sigma 0.05 with a tone of amplitude 0.5 in the window; the flat threshold T lies halfway between the median and the maximum
of the window's cells on the host copy, so some cells clear it and most do not (asserted).  Everything is compared exactly."""
import os

import numpy as np
import pytest

import mask_model as mm
from oracle_lib import add_tone, gaussian_iq

pytestmark = pytest.mark.gpu

SHAPES = {
    # fft_len_log, wf_rows, n_bins, max_spectra, spectra processed, first_bin, n_cols, the tone's bin (shifted column bin + N/2)
    "n1024": (10, 8, 128, 1024, 32, 509, 10, 2),
    "n8192": (13, 4, 512, 16, 16, 4093, 2054, 1000),
    "n1024_pos": (10, 64, 128, 1024, 80, 509, 10, 2),
}


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Case:
    pass


@pytest.fixture(scope="module", params=list(SHAPES))
def case(request, amd):
    import torch
    log, wf_rows, n_bins, max_spectra, spectra, first_bin, n_cols, tone_bin = SHAPES[request.param]
    c = Case()
    c.f = amd.Fosphor(fft_len_log=log, n_bins=n_bins, wf_rows=wf_rows, max_spectra=max_spectra)
    c.n, c.rows, c.first_bin, c.n_cols = c.f.n, wf_rows, first_bin, n_cols
    x = add_tone(gaussian_iq(spectra * c.n, 1800 + log), 0.5, tone_bin / c.n, phase0=0.3)
    assert c.f.process_device(torch.from_numpy(x).cuda(), 1, spectra) == 0
    b = c.f.buffers(False)
    assert spectra > wf_rows and b.wf_rows == wf_rows and b.waterfall_pos == spectra % wf_rows	# the ring has wrapped
    if request.param == "n1024_pos":
        assert b.waterfall_pos == 16
    c.W = mm.newest_first(c.f.waterfall, b.waterfall_pos)		# [rows][N]: row 0 the newest, shifted columns; left unchanged
    c.win = c.W[:, first_bin:first_bin + n_cols]
    c.T = float(np.float32((np.median(c.win) + c.win.max()) / 2))
    over = int((c.win > np.float32(c.T)).sum())
    assert 0 < over < c.win.size // 2, over
    c.d_T = torch.full((c.n,), c.T, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    yield c
    c.f.close()


def mask_check(c):
    res, recs, _, _ = c.f.mask_scan(upper=c.d_T, first_bin=c.first_bin, n_cols=c.n_cols, rows=c.rows, max_events=0)
    over = c.win > np.float32(c.T)
    excess = np.where(over, c.win - np.float32(c.T), np.float32(-1))
    some = over.any(axis=1)
    cols = c.first_bin + np.arange(c.n_cols)
    assert np.array_equal(recs["n_over"], over.sum(axis=1)) and not recs["n_under"].any()
    assert np.array_equal(recs["first_col"], np.where(some, cols[over.argmax(axis=1)], -1))
    assert np.array_equal(recs["last_col"], np.where(some, cols[c.n_cols - 1 - over[:, ::-1].argmax(axis=1)], -1))
    assert np.array_equal(recs["peak_col"], np.where(some, cols[excess.argmax(axis=1)], -1))	# argmax: the lowest column of equals
    assert res["n_triggered"] == int(some.sum())
    return recs


def burst_check(c, n_over):
    res, recs = c.f.bursts(c.T, first_bin=c.first_bin, n_cols=c.n_cols, rows=c.rows, max_gap_cols=0, max_gap_rows=0, min_rows=1,
                           min_cols=1, max_bursts=65536)
    assert res["overflow"] == 0 and res["n_written"] == res["n_found"] == len(recs) > 0
    assert int(recs["n_cells"].sum()) == int(n_over.sum())
    assert recs["peak_y"].max().tobytes() == c.win.max().tobytes()


def view_check(c):
    out = c.f.view(c.first_bin, c.n_cols, width=c.n_cols, wf_src_rows=c.rows, wf_out_rows=c.rows, detector="peak",
                   outputs=["waterfall"])["waterfall"].cpu().numpy()
    assert out.shape == c.win.shape and np.array_equal(out.view(np.uint32), np.ascontiguousarray(c.win).view(np.uint32))


def detect_check(c):
    res, bands = c.f.detect(trace="live", floor="absolute", threshold_y=c.T, max_gap=0, min_cols=1, first_bin=c.first_bin,
                            n_cols=c.n_cols, max_bands=65536)
    above = c.f.spectrum[0, c.first_bin:c.first_bin + c.n_cols, 1] > np.float32(c.T)
    edge = np.diff(np.concatenate(([0], above.astype(np.int8), [0])))
    first, last = c.first_bin + np.flatnonzero(edge == 1), c.first_bin + np.flatnonzero(edge == -1) - 1
    assert res["n_found"] == res["n_written"] == first.size
    assert np.array_equal(bands["first"], first) and np.array_equal(bands["last"], last)


def test_mask_and_bursts_read_the_window(case):
    recs = mask_check(case)
    burst_check(case, recs["n_over"])


def test_view_reads_the_window(case):
    view_check(case)


def test_detect_reads_the_window(case):
    detect_check(case)


def test_bad_windows_are_refused_and_the_instance_lives(case):
    c = case
    bad = [(-1, 10), (c.n, 1), (c.first_bin, 0), (c.first_bin, c.n - c.first_bin + 1)]
    calls = [
        lambda fb, nc: c.f.mask_scan(upper=c.d_T, first_bin=fb, n_cols=nc, rows=c.rows, max_events=0),
        lambda fb, nc: c.f.bursts(c.T, first_bin=fb, n_cols=nc, rows=c.rows),
        lambda fb, nc: c.f.view(fb, nc, width=10, wf_src_rows=c.rows, wf_out_rows=c.rows, outputs=["waterfall"]),
        lambda fb, nc: c.f.detect(trace="live", floor="absolute", threshold_y=c.T, first_bin=fb, n_cols=nc),
    ]
    for call in calls:
        for fb, nc in bad:
            with pytest.raises(RuntimeError, match="EINVAL"):
                call(fb, nc)
    recs = mask_check(c)
    burst_check(c, recs["n_over"])
    view_check(c)
    detect_check(c)
