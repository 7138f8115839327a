"""CPU: the inputs of the bin-count tests (tests/bin_count_cases.py) and the oracle at bin counts it had never been run at.

The GPU module holds the device to the oracle at 16, 48, 240, 256, 272, 496 and 512 bins; here the oracle itself is held to a plain
numpy statement at the same counts -- the power range's scale and offset, the hit counts recomputed from the power rows, the
conservation of hits -- and the product's host-side threshold table to the oracle's binning.  The conditions on the inputs (row 0,
the last row, every row between, both sides of row 256, both clamps) are asserted here, on the CPU, for every case the GPU runs."""
import numpy as np
import pytest

import bin_count_cases as bc
import shard_emul as se
import wire_cases as wc
from oracle_lib import hitcount_from_rows, oracle_bins

CASES = [(log2n, nb, bc.FMT[log2n]) for log2n in (10, 13, 16) for nb in bc.COUNTS] + \
        [(log2n, nb, "sc16") for log2n, nb in sorted(bc.SC16_COUNT.items())]


def test_case_tables_are_consistent():
    assert bc.COUNTS == sorted(bc.COUNTS) and all(16 <= nb <= 512 and nb % 16 == 0 for nb in bc.COUNTS)
    for log2n, calls in bc.CALLS.items():
        assert 2 <= len(calls) <= 3 and any(nbat == 2 for _, nbat, _, _ in calls)
        for kind, nbat, batch, overlap in calls:
            assert kind in ("host", "device") and 16 <= nbat * batch <= bc.MAX_SPECTRA[log2n] and batch % 16 == 0
            assert 16 <= batch <= 64 and (overlap == 1 or kind == "device")
        assert bc.SC16_COUNT[log2n] in bc.COUNTS and bc.SC16_COUNT[log2n] % 32
    assert [c for c in bc.CALLS[13] if c[3] == 2]
    # the streams: one slice per call, of the call's length, read-only (shared among the cases)
    for log2n in (10, 13):
        for (x, x32), call in zip(bc.streams(log2n, bc.FMT[log2n]), bc.CALLS[log2n]):
            assert x.shape == x32.shape == (bc.call_samples(log2n, call), 2) and not x32.flags.writeable


@pytest.mark.parametrize("log2n,n_bins,fmt", CASES)
def test_oracle_equals_numpy_statement_and_inputs_cover_the_rows(oracle_built, log2n, n_bins, fmt):
    n = 1 << log2n
    o = bc.make_oracle(log2n, n_bins)
    # fosphor.c:131-152 / cl.c:1087: the range [db_ref - 10 db_per_div, db_ref] over the n_bins rows, 0 dB = a full-scale tone
    db_ref, db_div = bc.RANGES[log2n]
    assert o.histo_scale == np.float32(n_bins * 20.0 / (10 * db_div))
    assert abs(o.histo_offset - -(np.log10(n) + (db_ref - 10 * db_div) / 20.0)) < 1e-6
    total = np.zeros((n, n_bins), np.uint64)
    pos = 0
    for k, (call, (_, x32)) in enumerate(zip(bc.CALLS[log2n], bc.streams(log2n, fmt))):
        _, nbat, batch, _ = call
        what = "N %d, %d bins, %s, call %d" % (n, n_bins, fmt, k)
        bc.oracle_call(o, log2n, call, x32)
        pos = (pos + nbat * batch) % bc.WF_ROWS
        assert o.waterfall_pos == pos
        hc = o.hitcount				# of the call's last batch
        assert hc.shape == (n, n_bins) and np.all(hc.sum(axis=1) == batch), what + ": a column's hits do not add up to the batch"
        # the counts restated: round-half-away of scale * (pwr + offset), clamped to [0, n_bins - 1], from the batch's power rows
        rows = (pos - batch + np.arange(batch)) & (bc.WF_ROWS - 1)
        want = hitcount_from_rows(o.waterfall[rows], o.histo_scale, o.histo_offset, n_bins)
        assert np.array_equal(hc, want), what + ": %d cells differ from the numpy statement" % (hc != want).sum()
        bc.assert_covers(hc, n_bins, what, every_row=False)
        bc.assert_clamps(o, batch, what)
        total += hc
    bc.assert_covers(total, n_bins, "N %d, %d bins, %s, all calls" % (n, n_bins, fmt))
    hist = o.histogram
    assert hist.shape == (n_bins, n) and np.isfinite(hist).all() and hist.min() >= 0.0 and hist.max() <= 1.0
    assert (hist[0] > 0).any() and (hist[n_bins - 1] > 0).any()


@pytest.mark.parametrize("cid", se.BIN_COUNT_CASES)
def test_sharded_bin_count_frames_stay_sparse(oracle_built, cid):
    """what shard_emul.BIN_COUNT_CASES' ranges were chosen for: the rows of 64 cells that hold a hit are a real subset, strictly
    between 1 % and 50 % of all rows, in every frame (above one half the sparse wire form falls back to the packed one and the
    GPU test of it would prove nothing); above 256 bins both sides of row 256 hold at least 1 % of the hits"""
    c = se.CASES[cid]
    o = se.make_oracle(c)
    for frame in range(c["frames"]):
        _, x32 = se.make_stream(c, frame)
        se.oracle_frame(o, c, x32)
        want = wc.oracle_counts(o)
        frac = wc.live_rows(want) / (want.size // 64)
        print("case %s frame %d: %.3f of the rows live" % (cid, frame, frac))
        assert 0.01 < frac < 0.5
        if c["n_bins"] > 256:
            lo, hi = se.plane_fractions(o)
            assert lo >= 0.01 and hi >= 0.01


def test_the_stop_band_is_quiet_and_the_tone_is_loud(oracle_built):
    """the lower clamp comes from whole columns (the stop band: row 0 only), the upper one from the tone's column (the last row only)"""
    for log2n in (10, 13):
        n, nb = 1 << log2n, 272
        o = bc.make_oracle(log2n, nb)
        call, (_, x32) = bc.CALLS[log2n][-1], bc.streams(log2n, bc.FMT[log2n])[-1]
        bc.oracle_call(o, log2n, call, x32)
        hc = o.hitcount				# [x][bin], x the FFT's own (unshifted) index
        quiet = int(0.5 * (bc.STOP_BAND[0] + bc.STOP_BAND[1]) * n)
        loud = int(round(bc.TONE_FREQ * n))
        assert hc[quiet, 0] == call[2] and hc[loud, nb - 1] == call[2]


@pytest.mark.parametrize("n_bins", [16, 48, 240, 272, 496, 512])
def test_threshold_table_reproduces_oracle_bins(oracle_built, n_bins):
    """tests/test_boundary_cpu.py's check of the table the device compares against (count(s >= thr[b]) == oracle bin), at the
    counts and the 20 dB range of these cases: random samples over 24 decades and three floats around every threshold"""
    from _pkg import gr_fosphor_amd
    L = gr_fosphor_amd.load()
    rng = np.random.default_rng(3)
    o = bc.make_oracle(10, n_bins)
    thr = np.empty(n_bins + 1, np.float64)
    assert L.fosphor_amd_host_thresholds(n_bins, o.histo_scale, o.histo_offset, thr.ctypes.data) == 0
    assert thr[0] == -1.0 and np.all(np.diff(thr[1:]) >= 0)
    mag = np.exp(rng.uniform(np.log(1e-12), np.log(1e12), 200000))
    ph = rng.uniform(0, 2 * np.pi, mag.size)
    v = np.stack([mag * np.cos(ph), mag * np.sin(ph)], 1).astype(np.float32)
    edge = []
    for b in range(1, n_bins):
        if thr[b] < thr[n_bins]:
            h = np.float32(np.sqrt(thr[b]))
            edge += [np.nextafter(h, np.float32(0)), h, np.nextafter(h, np.float32(np.inf))]
    edge = np.array(edge, np.float32)
    v = np.concatenate([v, np.stack([edge, np.zeros_like(edge)], 1)])
    want, _ = oracle_bins(v, o.histo_scale, o.histo_offset, n_bins)
    s = v[:, 0].astype(np.float64) ** 2 + v[:, 1].astype(np.float64) ** 2
    got = np.searchsorted(thr[1:n_bins], s, side="right")
    got = np.where(s >= thr[n_bins], 0, got)
    assert np.array_equal(got, want), "%d samples" % (got != want).sum()
    assert want.min() == 0 and want.max() == n_bins - 1 and np.unique(want).size == n_bins
