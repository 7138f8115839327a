"""No GPU: the inputs of tests/test_gpu_extremes.py (tests/extreme_cases.py) reach what they claim, on the oracle alone -- its FFT
(Oracle.fft), its pinned bin pipeline (oracle_bins) and its state after every batch, for every length, bin count and format of the
kernel table, at hop = N (the rows with an overlap have conditions of their own, below).
A condition that fails here means the input is wrong, not the assertion.

  * classes: |X|^2 (in double) below 1e-30 and above 1e30 with a finite log-power, exactly 0, NaN, each in the batch that names it;
    cells of +inf power and bin 0 whose re and im are both finite; no non-finite FFT word outside the spectra that hold a NaN or an
    inf sample (no intermediate overflowed);
  * bins: the x 1e30 spectra's hits in bin n_bins - 1 (>= 256 at 512 bins), the x 1e-30 and zero spectra's in bin 0; with the special
    spectra replaced by the ordinary ones under them, the oracle's hit counts differ in at least (special spectra) x N cells;
  * state: after `scaled` everything finite; after `minus_inf` live -inf everywhere and max-hold finite; after `column_inf` live
    +inf in the tones' columns only; after `nan_columns` NaN in exactly those; after `nan` NaN everywhere; after `recover` finite;
  * positions: every class at every residue mod 4 (N = 1024) / mod 8 (N = 8192) over the rotations of a row, the only special
    spectrum of its even / odd pair;
  * the fp16 and sc16 arrays hold exactly the values handed to the oracle;
  * the rows with an overlap: no two altered windows share a spectrum, and every batch that holds a class holds wholly special AND
    ordinary spectra, checked on the oracle's FFT; hop 1: NaN, huge and ordinary spectra in the first batch, recovery after it;
  * the tile-walk calls: the special tiles' units take a second tile, in the call's last batch."""
import numpy as np
import pytest

import extreme_cases as ec
import window_cases as wc
from oracle_lib import Oracle, canon_bits, oracle_bins
from test_gpu_iq_sc16 import widen

# one entry per (length, bin count, format, power range) of the kernel table
GEOMETRIES = sorted({(r["log2n"], r["n_bins"], r["fmt"], r["power"]) for r in ec.ROWS.values()}, key=str)

# what a format's classes claim; the rest of the conditions follow from the batch tables
NONFINITE_SAMPLE = ("nan1", "inf1")


def _sq(f):
    f = f.astype(np.float64)
    return f[..., 0] ** 2 + f[..., 1] ** 2


@pytest.mark.parametrize("log2n,n_bins,fmt,power", GEOMETRIES, ids=["n%d_%d_%s" % (1 << g[0], g[1], g[2]) for g in GEOMETRIES])
def test_inputs_reach_what_they_claim(oracle_built, log2n, n_bins, fmt, power):
    row = dict(log2n=log2n, n_bins=n_bins, fmt=fmt, power=power)
    n, top = 1 << log2n, n_bins - 1
    _, xo = ec.stream(log2n, fmt)
    _, xp = ec.stream(log2n, fmt, plain=True)
    o, plain = ec.make_oracle(row), ec.make_oracle(row)
    w = o.window
    seen = set()
    for k, name in enumerate(ec.ORDER):
        what = "N = %d, %d bins, %s, batch %s" % (n, n_bins, fmt, name)
        b = ec.batch_of(xo, log2n, 1, k)
        assert o.process(b, strict=False, nthreads=8) == 0 and plain.process(ec.batch_of(xp, log2n, 1, k), strict=False, nthreads=8) == 0
        f = Oracle.fft(b, w, fft_len_log=log2n)
        bins, pwr = oracle_bins(f, o.histo_scale, o.histo_offset, n_bins)
        bins, pwr, s = bins.reshape(ec.BATCH, n), pwr.reshape(ec.BATCH, n), _sq(f)
        placed = ec.positions(name, fmt, 0)
        special = np.zeros(ec.BATCH, bool)
        special[[p for _, _, p in placed]] = True
        tone_cols = []
        # ---- classes and bins, per special spectrum
        for cls, copy, p in placed:
            seen.add(cls)
            fin_words = np.isfinite(f[p]).all()
            assert fin_words == (cls not in NONFINITE_SAMPLE), "%s: %s at %d, non-finite FFT words" % (what, cls, p)
            if cls == "big":
                assert np.all(s[p] > 1e30) and np.all(np.isfinite(pwr[p])) and np.all(bins[p] == top), what
                assert n_bins < 512 or top >= 256			# the 9th bit of the index is set
            elif cls in ("small", "sub"):
                assert np.all((s[p] < 1e-30) & (s[p] > 0)) and np.all(np.isfinite(pwr[p])) and np.all(bins[p] == 0), what
                if cls == "sub":		# subnormal samples give subnormal FFT words
                    assert np.all(np.abs(b.reshape(ec.BATCH, n, 2)[p]) < 2.0 ** -126)
                    assert ((np.abs(f[p]) < 2.0 ** -126) & (f[p] != 0)).sum() > n
            elif cls == "zero":
                assert not s[p].any() and np.all(np.isneginf(pwr[p])) and np.all(bins[p] == 0), what
            elif cls == "tone_inf":
                col = ec.tone_inf_bin(n, copy)
                tone_cols.append(col)
                over = np.isposinf(pwr[p])
                assert np.array_equal(np.flatnonzero(over), [col]), "%s: +inf power in columns %s" % (what, np.flatnonzero(over))
                assert np.all(np.isfinite(f[p, col])) and bins[p, col] == 0, what		# hypot overflows float, re and im finite
                assert s[p, col] > float(np.finfo(np.float32).max) ** 2
                assert bins[p, col - 1] == top and bins[p, col + 1] == top, what		# the top bin in its neighbours
                assert not np.isnan(pwr[p]).any()
            elif cls in NONFINITE_SAMPLE:
                assert np.all(np.isnan(s[p])) and np.all(bins[p] == 0), what
            elif cls == "max16":
                assert np.all(np.isfinite(pwr[p])) and np.all(bins[p] == top), what
            elif cls == "full":			# |X|^2 ~ 2 N: the upper half of this range, half of it in the top bin
                assert np.all(np.isfinite(pwr[p])) and (bins[p] >= n_bins // 2).mean() > 0.9 and (bins[p] == top).mean() > 0.5, what
            elif cls in ("sub16", "lsb"):
                assert np.all(np.isfinite(pwr[p])) and np.all(bins[p] == 0), what
            else:
                raise AssertionError(cls)
        # ---- the ordinary spectra stay ordinary: finite, and off both ends of the bin range for the most part
        assert np.all(np.isfinite(f[~special])) and np.all(np.isfinite(pwr[~special])), what
        mid = (bins[~special] > 0) & (bins[~special] < top)
        assert mid.mean() > 0.9, what
        # ---- the special spectra's hits are what distinguishes the batch
        hc = o.hitcount
        assert int(hc.sum(dtype=np.uint64)) == ec.BATCH * n
        differ = int((hc != plain.hitcount).sum())
        print("%s: %d special spectra, %d cells differ from the ordinary batch's counts" % (what, special.sum(), differ))
        assert differ >= special.sum() * n, what
        # ---- state
        live, mx = o.spectrum[0, :, 1], o.spectrum[1, :, 1]
        classes = {cls for cls, _, _ in placed}
        if name == "scaled":
            assert np.all(np.isfinite(live)) and np.all(np.isfinite(mx)) and np.all(np.isfinite(o.waterfall)), what
        elif name == "minus_inf":
            assert np.all(np.isneginf(live)) and np.all(np.isfinite(mx)), what
        elif name == "column_inf" and tone_cols:
            shifted = sorted((c + n // 2) % n for c in tone_cols)		# the vertices are fft-shifted
            assert np.array_equal(np.flatnonzero(np.isposinf(live)), shifted) and not np.isnan(live).any(), what
            assert np.array_equal(np.flatnonzero(~np.isfinite(mx)), shifted), what
        elif name == "nan_columns" and tone_cols:
            shifted = sorted((c + n // 2) % n for c in tone_cols)
            assert np.array_equal(np.flatnonzero(np.isnan(live)), shifted), what
            assert np.all(np.isneginf(np.delete(live, shifted))), what
        elif name == "nan":
            if classes & set(NONFINITE_SAMPLE):
                assert np.all(np.isnan(live)) and not np.isfinite(mx).any(), what
            else:
                assert np.all(np.isneginf(live)), what			# sc16: zero beside full scale
        else:
            assert not placed
        if not placed:
            assert np.all(np.isfinite(live)) and np.all(np.isfinite(o.waterfall[ec.BATCH * k % ec.WF_ROWS:][:ec.BATCH])), what
            if name.startswith("recover"):
                assert np.all(np.isfinite(mx)), what
    assert seen == {cls for v in ec.BATCHES.values() for cls, _ in v[fmt]}
    if fmt == "fp32":
        assert {"big", "small", "sub", "zero", "tone_inf", "nan1", "inf1"} <= seen
    # ordinary spectra (the last batch) put hits in both halves of a 512-bin range
    if n_bins == 512:
        lo, hi = o.hitcount[:, :256].sum() / (ec.BATCH * n), o.hitcount[:, 256:].sum() / (ec.BATCH * n)
        print("N = %d, %s: %.2f / %.2f of the ordinary hits below / from bin 256 on" % (n, fmt, lo, hi))
        assert lo >= 0.1 and hi >= 0.1


def test_every_class_stands_at_every_residue():
    for rid, row in ec.ROWS.items():
        if row["overlap"] > 1:			# (test_overlap_rows_cover_the_residues)
            continue
        mod = {10: 4, 13: 8, 16: 4}[row["log2n"]]
        at = {}
        for rot in row["rots"]:
            assert rot % 2 == 0 and 0 <= rot < ec.BATCH
            for name in ec.ORDER:
                placed = ec.positions(name, row["fmt"], rot)
                pos = [p for _, _, p in placed]
                assert len(set(p // 2 for p in pos)) == len(pos) <= 8, (rid, name)	# one special spectrum per even / odd pair:
                for cls, _, p in placed:						# ordinary neighbours in pair, dword and byte
                    at.setdefault(cls, set()).add(p)
                    for group in (2, 4, 8):
                        assert any(q // group == p // group and q not in pos for q in range(ec.BATCH)), (rid, name, cls, group)
        assert at, rid
        for cls, ps in at.items():
            assert {p % 2 for p in ps} == {0, 1}, (rid, cls)
            if mod:
                assert {p % mod for p in ps} == set(range(mod)), "%s: %s stands at residues %s mod %d" % (rid, cls, sorted(ps), mod)


_OVERLAP = [(rid, rot) for rid, r in ec.ROWS.items() if r["overlap"] > 1 for rot in r["rots"]]


@pytest.mark.parametrize("rid,rot", _OVERLAP, ids=["%s-rot%d" % p for p in _OVERLAP])
def test_overlap_rows_hold_special_and_ordinary_spectra(oracle_built, rid, rot):
    """With an overlap the altered windows must not meet, and every batch that holds a class must hold a spectrum that is wholly that
    class's AND ordinary spectra; on the oracle's FFT the former are special (non-finite words, or nine hits in ten in bin 0 or the
    top bin), the latter finite with nine hits in ten off both ends.  hop 1: NaN, huge and ordinary spectra in the first batch."""
    r = ec.ROWS[rid]
    log2n, fmt, ov = r["log2n"], r["fmt"], r["overlap"]
    n, top = 1 << log2n, r["n_bins"] - 1
    t = ec.touched(log2n, fmt, ov, rot)			# (asserts that no two windows meet)
    _, xo = ec.stream(log2n, fmt, ov, rot)
    o = ec.make_oracle(r)
    for k, name in enumerate(ec.ORDER):
        what = "%s rotation %d batch %s" % (rid, rot, name)
        tk = t[ec.BATCH * k:ec.BATCH * (k + 1)]
        holds = bool(ec.BATCHES[name][fmt]) if ov <= ec.BATCH else k == 0
        assert (tk == 2).any() == holds, what
        assert (tk == 0).any(), what + ": no ordinary spectrum"
        if ov <= ec.BATCH and holds:
            assert (tk == 2).sum() == len(ec.positions(name, fmt, rot, ov)) and (tk == 0).sum() >= (4 if ov == 2 else 1), what
        f = Oracle.fft(ec.batch_of(xo, log2n, ov, k), o.window, fft_len_log=log2n)
        bins, pwr = oracle_bins(f, o.histo_scale, o.histo_offset, r["n_bins"])
        bins, pwr = bins.reshape(ec.BATCH, n), pwr.reshape(ec.BATCH, n)
        for i in range(ec.BATCH):
            ends = ((bins[i] == 0) | (bins[i] == top)).mean()
            if tk[i] == 2:
                assert not np.isfinite(f[i]).all() or ends > 0.9, "%s: spectrum %d is not special" % (what, i)
            elif tk[i] == 0:
                assert np.isfinite(f[i]).all() and np.isfinite(pwr[i]).all() and ends < 0.1, "%s: spectrum %d is not ordinary" % (what, i)
    if ov > ec.BATCH:
        (_, s_nan), (_, s_big) = ec.HOP1_HEAD
        f = Oracle.fft(ec.batch_of(xo, log2n, ov, 0), o.window, fft_len_log=log2n)
        assert np.isnan(f[:s_nan + rot + 1]).any(axis=-1).all() and np.all(np.isfinite(f[s_nan + rot + 1:]))
        assert np.all(_sq(f[s_nan + rot + 1:s_big + rot + 1]) > 1e30)
        # the stream ends recovered on the oracle
        for k in range(len(ec.ORDER)):
            assert o.process(ec.batch_of(xo, log2n, ov, k), strict=False, nthreads=8) == 0
            assert np.all(np.isfinite(o.spectrum[0, :, 1])) == (k > 0)


def test_overlap_rows_cover_the_residues():
    """overlap 2: every class of a batch at every position residue mod 8 over the row's rotations; overlap 8: the one wholly special
    spectrum of a batch at every residue mod 8, every class of the batch in its turn"""
    for rid, r in ec.ROWS.items():
        if not 1 < r["overlap"] <= ec.BATCH:
            continue
        for name in ec.ORDER:
            placed = [x for rot in r["rots"] for x in ec.positions(name, r["fmt"], rot, r["overlap"])]
            classes = {cls for cls, _ in ec.BATCHES[name][r["fmt"]]}
            assert {cls for cls, _, _ in placed} == classes, (rid, name)
            if r["overlap"] == 2:
                for cls in classes:
                    assert {p % 8 for c, _, p in placed if c == cls} == set(range(8)), (rid, name, cls)
            elif classes:
                assert {p % 8 for _, _, p in placed} == set(range(8)), (rid, name)


@pytest.mark.parametrize("cid", ec.WALK_CASES)
def test_walk_cases_put_special_tiles_in_front_of_the_last_batch(oracle_built, cid):
    """tile-walk calls (tile_walk_cases' launch rules restated for 256 CUs, and 128 at N = 8192): the units of the special tiles take a
    second tile, and that tile lies in the call's last batch"""
    import tile_walk_cases as tw
    c = tw.CASES[cid]
    total = tw.total(c)
    for n_cus in (256, 128) if c["log2n"] == 13 else (256,):
        p = tw.expected_plan(c["log2n"], c["n_bins"], c["fmt"], tw.hop(c), tw.iq_align(c), int(c["env"].get("FOSPHOR_AMD_TILE", 0)),
                             int(c["env"].get("FOSPHOR_AMD_K1", 1)), n_cus, total, c["batch"])
        assert p["kernel"] == c["kernel"] and p["max_tiles"] >= 2
        if c["overlap"] > ec.BATCH:
            tiles = range(ec.WALK_HOP1_HEAD[-1][1] // p["tile"] + 1)
        else:
            placed = ec.walk_placed(c, p)
            assert [cls for cls, _, _ in placed] == list(ec.WALK_CLASSES)
            tiles = [g // p["tile"] for _, _, g in placed]
            assert len(set(tiles)) == len(tiles)
            for _, _, g in placed:		# the window and what shares samples with it stay inside its tile
                assert (g - c["overlap"] + 1) // p["tile"] == g // p["tile"] == (g + c["overlap"] - 1) // p["tile"] or c["overlap"] == 1
                assert c["overlap"] <= 2
        for t in tiles:
            assert t < p["units"] and t + p["units"] < p["tiles"], (cid, t)			# its unit takes a second tile ...
            assert (t + p["units"]) * p["tile"] >= total - c["batch"], (cid, t)		# ... in the last batch
            assert t * p["tile"] < total - c["batch"]


def test_input_arrays_hold_what_the_oracle_is_fed():
    for log2n, fmt in sorted({(r["log2n"], r["fmt"]) for r in ec.ROWS.values()}):
        x, xo = ec.stream(log2n, fmt)
        assert xo.dtype == np.float32 and xo.shape == (ec.n_samples(log2n, 1, ec.MAX_SPECTRA), 2)
        if fmt == "sc16":
            assert x.dtype == np.int16 and x.min() == -32768 and x.max() == 32767
            assert np.array_equal(xo.astype(np.float64).reshape(-1), x.astype(np.float64) * 2.0 ** -15)
            assert np.array_equal(canon_bits(xo), canon_bits(widen(x).reshape(-1, 2)))
            assert np.all(np.isfinite(xo))
        elif fmt == "fp16":
            assert x.dtype == np.float16 and np.array_equal(xo.astype(np.float16).view(np.uint16), x.view(np.uint16))
            assert np.array_equal(canon_bits(xo), canon_bits(x.astype(np.float32)))
            fin = np.isfinite(x)
            assert np.isnan(x).sum() == 2 and np.isinf(x).sum() == 2			# one NaN and one inf half per copy
            assert np.abs(x[fin]).max() == 65504 and ((np.abs(x[fin]) < 2.0 ** -14) & (x[fin] != 0)).sum() > 4 << log2n
        else:
            assert x is xo or np.array_equal(canon_bits(x), canon_bits(xo))
            assert np.isnan(x).sum() == 2 and np.isinf(x).sum() == 2
    for c in ec.SHARD_CASES.values():
        for frame in range(c["frames"]):
            x, x32 = ec.shard_stream(c, frame)
            assert x.dtype == np.float32 and x.shape == (c["total"] << c["log2n"], 2) and np.all(np.isfinite(x))


def test_tables_are_consistent():
    assert ec.ORDER[:3] == ("scaled", "minus_inf", "column_inf") and ec.ORDER[-3:] == ("nan", "recover", "recover2")
    assert len(ec.ORDER) <= 8 and ec.MAX_SPECTRA == ec.BATCH * len(ec.ORDER) and ec.WF_ROWS == 64
    assert set(ec.FFT_BATCHES) <= set(ec.ORDER)
    kernels = {r["kernel"] for r in ec.ROWS.values()}
    assert {"k1_fft_bin<iq_fp32>", "k1_fft_bin<iq_fp32, NB256>", "k1big_fft_bin<iq_fp32, 10>"} <= kernels
    assert sum(k.startswith("k1v2_fft_bin") for k in kernels) == 2
    assert {"k1w_fft_bin<iq_fp32, 16> (no reuse)", "k1w_fft_bin<iq_fp32, 8>", "k1w_fft_bin<iq_fp32, 2>"} <= kernels
    assert {"k1h_fused<iq_%s>" % f for f in ("fp32", "fp16", "sc16")} <= kernels
    for rid, r in ec.ROWS.items():
        n = 1 << r["log2n"]
        assert n % r["overlap"] == 0 and (r["overlap"] == 1) == (r["entry"] == "device"), rid
        assert r["fmt"] == "fp32" or r["log2n"] == 16, rid
        assert set(r["env"]) <= set(ec.KNOBS), rid
        assert not r["host"] or (r["log2n"] == 10 and r["overlap"] == 1), rid
        if r["fft"]:
            fc = wc.FFT_CASES[r["fft"]]
            assert (fc["log2n"], fc["n_bins"], fc["fmt"], fc["env"]) == (r["log2n"], r["n_bins"], r["fmt"], r["env"]), rid
    # every instantiation of the FFT hook is some row's
    assert {r["fft"] for r in ec.ROWS.values() if r["fft"]} == set(wc.FFT_CASES)
    assert any(r["host"] for r in ec.ROWS.values() if r["log2n"] == 10)
    for cid, c in ec.SHARD_CASES.items():
        assert sum(cnt for _, cnt in c["shards"]) == c["total"] and all(cnt % 16 == 0 and off % 16 == 0 for off, cnt in c["shards"])
        (_, first), = [s for s in c["shards"] if s[0] == 0]
        zero = {g < first for cls, _, g in ec.SHARD_FRAMES[0] if cls == "zero"}
        tone = {g < first for cls, _, g in ec.SHARD_FRAMES[0] if cls == "tone_inf"}
        assert zero == {True} and tone == {False}, cid		# the all-zero and the overflow-tone spectra on different ranks
        assert {cls for cls, _, _ in ec.SHARD_FRAMES[1]} == {"tone_inf", "big", "small"}


@pytest.mark.parametrize("cid", list(ec.SHARD_CASES))
def test_sharded_frames_on_the_oracle(oracle_built, cid):
    """frame 0: the float sum of the ranks' live partials is NaN in the tones' columns (+inf on one rank, -inf on the other), -inf
    elsewhere; frame 1: +inf in the tones' columns, hits in bin 0 and in bin n_bins - 1 in every column"""
    import shard_emul as se
    c = ec.SHARD_CASES[cid]
    n = 1 << c["log2n"]
    o = se.make_oracle(c)
    cols = sorted((ec.tone_inf_bin(n, copy) + n // 2) % n for copy in (0, 1))
    for frame in range(c["frames"]):
        _, x32 = ec.shard_stream(c, frame)
        se.oracle_frame(o, c, x32)
        live = o.spectrum[0, :, 1]
        if frame == 0:
            assert np.array_equal(np.flatnonzero(np.isnan(live)), cols) and np.all(np.isneginf(np.delete(live, cols)))
        else:
            assert np.array_equal(np.flatnonzero(np.isposinf(live)), cols) and not np.isnan(live).any()
            hc = o.hitcount
            assert np.all(hc[:, 0] >= 1) and np.all(hc[:, c["n_bins"] - 1] >= 1)
