"""No GPU: the inputs of tests/test_gpu_windows.py (tests/window_cases.py) are what they are chosen for, on the oracle alone.

  * every window but `zero` is told from each of its scrambles -- the taps reversed, half a turn off, the first 1024 repeated, the
    default window -- by the oracle's hit counts of 16 spectra in at least window_cases.MIN_CELLS cells, at all three lengths: a
    device that applied a scramble could not pass a comparison of counts.  The counts are printed (pytest -s); DESIGN.md section
    2.4 records them;
  * under `zero` every row written is -inf and every hit lands in bin 0;
  * the sc16 and fp16 samples of the cases widen exactly to the float32 the oracle is fed;
  * the case tables are consistent with the library's entry-point rules."""
import numpy as np
import pytest

import window_cases as wc
from oracle_lib import Oracle, canon_bits
from test_gpu_iq_sc16 import widen


def _counts(log2n, window):
    o = Oracle(fft_len_log=log2n, n_bins=wc.DISCRIMINATION[log2n], wf_rows=wc.WF_ROWS)
    o.set_window(window)
    assert o.process(wc.discrimination_input(log2n), strict=False, nthreads=8) == 0
    return o.hitcount


@pytest.mark.parametrize("log2n", [10, 13, 16])
@pytest.mark.parametrize("name", wc.FINITE)
def test_windows_are_told_from_their_scrambles(oracle_built, name, log2n):
    n = 1 << log2n
    w = wc.WINDOWS[name](n)
    assert w.dtype == np.float32 and w.shape == (n,) and np.all(np.isfinite(w))
    want = _counts(log2n, w)
    assert int(want.sum(dtype=np.uint64)) == 16 * n
    for s in wc.scrambles_of(n):
        ws = wc.SCRAMBLES[s](w)
        assert ws.dtype == np.float32 and ws.shape == (n,)
        differ = int((_counts(log2n, ws) != want).sum())
        print("N = %5d, %d bins: %-13s against %-19s %8d cells differ" % (n, wc.DISCRIMINATION[log2n], name, s, differ))
        assert differ >= wc.MIN_CELLS, "%s against its %s scramble at N = %d: only %d cells differ" % (name, s, n, differ)


def test_windows_are_what_they_say():
    for n in (1024, 8192, 65536):
        r, s = wc.ramp(n), wc.signed_sparse(n)
        assert r.min() > 0.15 and np.abs(r - wc.reversed_taps(r)).max() > 0.5			# positive, asymmetric
        assert np.array_equal(s[n // 4:n // 4 + n // 16], np.zeros(n // 16, np.float32))
        live = np.ones(n, bool); live[n // 4:n // 4 + n // 16] = False
        k = np.arange(n)
        assert np.all(s[live & (k % 2 == 1)] < 0) and np.all(s[live & (k % 2 == 0)] > 0)
        gain = np.ones(n); gain[3 * n // 4:3 * n // 4 + 64] = 8.0
        assert np.allclose(np.abs(s[live]), (r * gain)[live], rtol=1e-6)
        # a thread's hoisted pair (k, k + n/2): pairs with a zero and a live tap, with the step of 8 between neighbours
        assert (s[:n // 2] == 0).sum() == n // 16 and np.all(s[n // 2:] != 0)
        q = wc.random(n)
        assert q.min() >= 0.5 and q.max() < 1.5 and np.array_equal(q, wc.random(n))
        assert not wc.zero(n).any()
    w = wc.ramp(1024)
    assert np.array_equal(wc.first_1024_repeated(w), w) and "first_1024_repeated" not in wc.scrambles_of(1024)
    assert "first_1024_repeated" in wc.scrambles_of(8192)
    assert wc.reversed_taps(w)[0] == w[0] and wc.reversed_taps(w)[1] == w[1023] and wc.half_turn(w)[0] == w[512]


@pytest.mark.parametrize("log2n", [10, 13, 16])
def test_default_window_restatement(oracle_built, log2n):
    """window_cases.default_window against the oracle's own default: the same expression up to the host's cosf"""
    o = Oracle(fft_len_log=log2n, n_bins=128, wf_rows=wc.WF_ROWS)
    assert np.abs(wc.default_window(1 << log2n) - o.window).max() <= 5e-7
    # the property that makes the default a poor test window: mirror-symmetric to 12 ulps of its largest taps (1.43e-6)
    assert np.abs(o.window - wc.reversed_taps(o.window)).max() <= 12 * 2.0 ** -23


@pytest.mark.parametrize("log2n", [10, 13, 16])
def test_zero_window_on_the_oracle(oracle_built, log2n):
    n, nb = 1 << log2n, wc.DISCRIMINATION[log2n]
    o = Oracle(fft_len_log=log2n, n_bins=nb, wf_rows=wc.WF_ROWS)
    o.set_window(wc.zero(n))
    assert o.process(wc.discrimination_input(log2n), strict=False, nthreads=8) == 0
    wf = o.waterfall
    assert np.all(np.isneginf(wf[:16])) and np.all(wf[16:] == np.float32(-o.histo_offset))
    hc = o.hitcount
    assert np.all(hc[:, 0] == 16) and not hc[:, 1:].any()
    assert not np.all(np.isfinite(o.spectrum[0, :, 1]))
    # ... and the live spectrum leaves the non-finite state with the next call (display.cl:206-207)
    o.set_window(wc.ramp(n))
    assert o.process(wc.discrimination_input(log2n), strict=False, nthreads=8) == 0
    assert np.all(np.isfinite(o.spectrum[0, :, 1])) and np.all(np.isfinite(o.waterfall[16:32]))


def test_widened_inputs_are_exact():
    """sc16: i * 2^-15 is exact in float32 and is what the oracle is fed, bit for bit; fp16: the float32 the oracle is fed converts
    back to the same fp16 bits"""
    for cid, c in wc.PATH_CASES.items():
        if c["fmt"] == "fp32" or c["log2n"] == 16:
            continue
        for x, x32 in wc.path_streams(cid):
            assert x.dtype == np.int16 and x32.dtype == np.float32
            assert np.array_equal(x32.astype(np.float64).reshape(-1), x.astype(np.float64)[2 * c["offset"]:] * 2.0 ** -15)
            assert np.array_equal(canon_bits(x32), canon_bits(widen(x).reshape(-1, 2)[c["offset"]:]))
        assert x.min() == -32768 and x.max() == 32767
    for log2n in (10, 13, 16):
        for fmt in ("sc16", "fp16"):
            if fmt == "fp16" and log2n != 16:
                continue
            x, xo = wc.fft_input(log2n, fmt)
            assert xo.dtype == np.float32 and np.all(np.isfinite(xo))
            if fmt == "sc16":
                assert x.dtype == np.int16 and np.abs(x.astype(np.int32)).max() < 32767	# nothing clipped
                assert np.array_equal(xo.astype(np.float64).reshape(-1), x.astype(np.float64) * 2.0 ** -15)
                assert np.array_equal(canon_bits(xo), canon_bits(widen(x).reshape(-1, 2)))
            else:
                assert x.dtype == np.float16 and np.array_equal(xo.astype(np.float16).view(np.uint16), x.view(np.uint16))
                assert np.array_equal(xo.astype(np.float64), x.astype(np.float64))
    # the 65536-point streams, one call each (the largest arrays): the same two statements
    for cid in ("n65536_fp16", "n65536_sc16"):
        x, x32 = wc.path_streams(cid)[0]
        if x.dtype == np.int16:
            assert np.array_equal(x32.astype(np.float64).reshape(-1), x.astype(np.float64) * 2.0 ** -15)
        else:
            assert x.dtype == np.float16 and np.array_equal(x32.astype(np.float16).view(np.uint16), x.view(np.uint16))


def test_case_tables_are_consistent():
    """every case obeys the entry points' rules (batches of a multiple of 16 spectra within the instance's capacity, an overlap that
    divides N, sc16 starts at a multiple of 4 bytes), and the tables reach what the issue lists"""
    assert {c["log2n"] for c in wc.FFT_CASES.values()} == {10, 13, 16}
    assert {c["fmt"] for c in wc.FFT_CASES.values() if c["log2n"] == 16} == {"fp32", "fp16", "sc16"}
    for cid, c in wc.PATH_CASES.items():
        n = 1 << c["log2n"]
        assert c["entry"] in ("host", "device", "overlap") and len(c["spectra"]) == 3, cid
        assert n % c["overlap"] == 0 and (c["overlap"] == 1) == (c["entry"] != "overlap"), cid
        assert c["fmt"] in ("fp32", "sc16") or c["log2n"] == 16, cid
        assert c["offset"] == 0 or c["fmt"] == "sc16", cid
        for call, b in enumerate(c["spectra"]):
            assert b % 16 == 0 and c["n_batches"] * b <= wc.MAX_SPECTRA, cid
            if c["env"].get("FOSPHOR_AMD_TILE"):
                assert b % int(c["env"]["FOSPHOR_AMD_TILE"]) == 0, cid
            assert wc.call_samples(c, call) == (c["n_batches"] * b - 1) * (n // c["overlap"]) + n
        assert set(c["env"]) <= set(wc.KNOBS), cid
        # the ring of WF_ROWS rows wraps within the three calls (but for the 16-spectrum host calls at N = 8192)
        assert sum(c["n_batches"] * b for b in c["spectra"]) > wc.WF_ROWS or cid == "n8192_host", cid
    k = {c["kernel"] for c in wc.PATH_CASES.values()}
    assert {"k1w_fft_bin<iq_fp32, %d>" % r for r in (8, 4, 2, 1, 16)} <= k
    assert {"k1h_fused<iq_%s>" % f for f in ("fp32", "fp16", "sc16")} <= k
    assert {"k1_fft_bin<iq_fp32>", "k1_fft_bin<iq_fp32, NB256>", "k1big_fft_bin<iq_fp32, 10>"} <= k
    assert sum("k1v2" in s for s in k) == 2
    for a, b in wc.PAIRS:
        assert a in wc.WINDOWS and b in wc.WINDOWS
    for c in wc.RELAXED_CASES.values():
        per_batch = wc.RELAXED_BATCH << c["log2n"]
        pieces = wc.RELAXED_BATCHES * per_batch // (1 << int(c["env"]["FOSPHOR_AMD_SUB_LOG2"]))
        assert pieces >= 2 and 14 <= int(c["env"]["FOSPHOR_AMD_SUB_LOG2"]) <= 34
    for c in wc.SHARD_CASES.values():
        assert sum(cnt for _, cnt in c["shards"]) == c["total"] and all(cnt % 16 == 0 and off % 16 == 0 for off, cnt in c["shards"])
