"""GPU: caller-set FFT windows and mid-stream setting changes on every FFT kernel and entry point (the windows, scrambles and case
tables of tests/window_cases.py).

Until here the long lengths and most kernel variants ran under the default window alone -- a periodic Hamming, smooth, positive and
mirror-symmetric to 1.4e-6, under which taps read backwards, half a turn off or from the first 1024 only go unseen.  Here an
asymmetric ramp, a random window, one with negative and zero taps and a step, and the all-zero window go through
  1. the FFT hook of every instantiation, bit for bit against the oracle's FFT (and against numpy's fp64 DFT),
  2. the whole path of every entry point and kernel: three queued calls with a window and a power-range change and the return to the
     default window between them, the state against the oracle's at the end and, separately, after every call,
  3. sharded frames (accumulate_device on two ranks, the emulated exchange, merge),
  4. table changes between relaxed calls whose FFT pieces alternate between streams, at N = 8192 and N = 65536,
  5. the zero window: -inf rows, every hit in bin 0, and the recovery under the next window.
The comparisons and bars are test_gpu_parity's (compare_state: FFT words and counts exact, waterfall / live / max-hold rtol 1e-4
atol 1e-6, the histogram through assert_hist_close) and tests/shard_emul.py's; nothing here has a tolerance of its own.
tests/test_window_cases_cpu.py asserts that the oracle's counts tell every window from each of its scrambles."""
import functools
import types

import numpy as np
import pytest

import shard_emul as se
import window_cases as wc
from oracle_lib import Oracle, canon_bits, gaussian_iq, add_tone
from test_gpu_parity import amd, torch_cuda, compare_state, assert_close	# noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _set_env(monkeypatch, env):
    for k in wc.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _window(name, n):
    return wc.WINDOWS[name](n)


def _snapshot(o):
    """the oracle's state as compare_state reads it, frozen"""
    return types.SimpleNamespace(waterfall_pos=o.waterfall_pos, hitcount=o.hitcount, waterfall=o.waterfall, spectrum=o.spectrum,
                                 histogram=o.histogram)


# ---- 1. the FFT hook ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(wc.FFT_CASES))
def test_fft_hook_under_caller_set_windows(amd, torch_cuda, oracle_built, monkeypatch, cid):
    """All four windows, one after the other on one instance (each upload replaces the one before), then the default again."""
    torch = torch_cuda
    c = wc.FFT_CASES[cid]
    _set_env(monkeypatch, c["env"])
    n, ns = 1 << c["log2n"], wc.FFT_SPECTRA
    f = amd.Fosphor(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=wc.WF_ROWS, max_spectra=16, iq_format=c["fmt"])
    x, xo = wc.fft_input(c["log2n"], c["fmt"])
    d_in = torch.tensor(x).cuda()
    d_out = torch.empty((ns, n, 2), dtype=torch.float32, device="cuda")
    z = xo.astype(np.float64).reshape(ns, n, 2)
    z = z[..., 0] + 1j * z[..., 1]
    default = Oracle(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=wc.WF_ROWS).window
    for name in list(wc.WINDOWS) + ["default"]:
        if name == "default":
            w = default
            f.set_fft_window_default()
        else:
            w = _window(name, n)
            f.set_fft_window(w)
        assert f.fft_device(d_in, d_out, ns) == 0
        got = d_out.cpu().numpy()
        want = Oracle.fft(xo, w, fft_len_log=c["log2n"])
        differ = int((canon_bits(got) != canon_bits(want)).sum())
        assert differ == 0, "%s (%s), window %s: %d words differ from the oracle's FFT" % (cid, c["kernel"], name, differ)
        if name == "zero":
            assert not got.any()
            continue
        ref = np.fft.fft(z * w.astype(np.float64), axis=-1)
        g = got[..., 0].astype(np.float64) + 1j * got[..., 1]
        err = np.max(np.abs(g - ref)) / np.max(np.abs(ref))
        print("%s window %s: %.3g of the largest value off numpy's fp64 DFT" % (cid, name, err))
        assert err < wc.DFT_BOUND[c["log2n"]], "%s, window %s: %.3g off numpy's fp64 DFT" % (cid, name, err)
    f.close()


# ---- 2. the whole path ---------------------------------------------------------------------------------------------------------
def _settings(call, pair, n):
    """(window, power range) set in front of call `call`; None: the default window / no change.  Call 0: window A; call 1: window B
    and a power range; call 2: back to the default window"""
    if call == 2:
        return None, None
    return _window(pair[call], n), (wc.POWER_RANGE_1 if call == 1 else None)


def _apply_device(f, window, power):
    if window is None:
        f.set_fft_window_default()
    else:
        f.set_fft_window(window)
    if power:
        f.set_power_range(*power)


def _apply_oracle(o, window, power):
    if window is None:
        o.set_window_default()
    else:
        o.set_window(window)
    if power:
        o.set_power_range(*power)


@functools.lru_cache(maxsize=1)
def _oracle_states(cid, pair):
    """the oracle's state after each of the three calls (computed once for both forms of the test below)"""
    c = wc.PATH_CASES[cid]
    n = 1 << c["log2n"]
    o = Oracle(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=wc.WF_ROWS)
    out = []
    for call, (_, x32) in enumerate(wc.path_streams(cid)):
        _apply_oracle(o, *_settings(call, pair, n))
        wc.oracle_call(o, c, call, x32)
        out.append(_snapshot(o))
    return out


# (the first decorator varies fastest: the two forms of a case follow each other and share _oracle_states' one entry)
@pytest.mark.parametrize("every_call", [False, True], ids=["queued", "every_call"])
@pytest.mark.parametrize("pair", wc.PAIRS, ids=["%s-%s" % p for p in wc.PAIRS])
@pytest.mark.parametrize("cid", list(wc.PATH_CASES))
def test_whole_path_under_changing_settings(amd, torch_cuda, oracle_built, monkeypatch, every_call, pair, cid):
    """Call 0 under window A; set_fft_window(B) and set_power_range(-10, 5), call 1; set_fft_window_default(), call 2 -- no finish()
    between them.  queued: the state after the last call (the three calls and their table uploads in flight together);
    every_call: the state after each (reading it waits)."""
    torch = torch_cuda
    c = wc.PATH_CASES[cid]
    _set_env(monkeypatch, c["env"])
    n = 1 << c["log2n"]
    f = amd.Fosphor(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=wc.WF_ROWS, max_spectra=wc.MAX_SPECTRA, max_batches=2,
                    iq_format=c["fmt"])
    states = _oracle_states(cid, pair)
    keep = []
    words = 2 if c["fmt"] == "sc16" else 1		# array elements per sample in front of the first one handed over
    for call, (x, _) in enumerate(wc.path_streams(cid)):
        what = "%s (%s), windows %s, call %d" % (cid, c["kernel"], pair, call)
        _apply_device(f, *_settings(call, pair, n))
        batch = c["spectra"][call]
        if c["entry"] == "host":
            assert f.process(x) == 0, what
        else:
            keep.append(torch.tensor(x).cuda())
            torch.cuda.synchronize()
            d = keep[-1][words * c["offset"]:]
            if c["offset"]:
                assert d.data_ptr() % 8 == 4
            if c["entry"] == "overlap":
                assert f.process_device_overlap(d, c["n_batches"], batch, c["overlap"]) == 0, what
            else:
                assert f.process_device(d, c["n_batches"], batch) == 0, what
        if every_call or call == 2:
            o = states[call]
            assert (f.histo_scale, f.histo_offset) == _histo(c, call), what
            assert int(f.hitcount.sum(dtype=np.uint64)) == batch * n, what + ": the counts do not add up to the batch"
            compare_state(f, o, what)
            if call < 2 and pair[call] == "zero":
                kept = min(c["n_batches"] * batch, wc.WF_ROWS)
                rows = (o.waterfall_pos - kept + np.arange(kept)) & (wc.WF_ROWS - 1)
                assert np.all(np.isneginf(f.waterfall[rows])), what + ": rows under the zero window"
    f.close()


@functools.lru_cache(maxsize=None)
def _histo_of(log2n, n_bins, power):
    o = Oracle(fft_len_log=log2n, n_bins=n_bins, wf_rows=wc.WF_ROWS)
    if power is not None:
        o.set_power_range(*power)
    return o.histo_scale, o.histo_offset


def _histo(c, call):
    """(histo_scale, histo_offset) in force at call `call`"""
    return _histo_of(c["log2n"], c["n_bins"], None if call == 0 else wc.POWER_RANGE_1)


# ---- 3. sharded frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(wc.SHARD_CASES))
def test_sharded_frames_under_caller_set_windows(amd, torch_cuda, oracle_built, monkeypatch, cid):
    """A frame under signed_sparse, then one after set_fft_window(ramp): two ranks accumulate a shard each, tests/shard_emul.py's
    exchange, merge; every rank against the oracle fed the whole frames."""
    torch = torch_cuda
    c = wc.SHARD_CASES[cid]
    for k in se.KNOBS:
        monkeypatch.delenv(k, raising=False)
    n = 1 << c["log2n"]
    o = se.make_oracle(c)
    ranks = se.make_ranks(amd, c)
    keep = []
    for frame, name in enumerate(wc.SHARD_WINDOWS):
        w = _window(name, n)
        o.set_window(w)
        for f in ranks:
            f.set_fft_window(w)
        x, x32 = se.make_stream(c, frame)
        se.oracle_frame(o, c, x32)
        keep.append(torch.from_numpy(x).cuda())
        res = se.run_sharded_frame(amd, torch, ranks, keep[-1], c["shards"], c["total"], overlap=c["overlap"])
        assert res["hc_sums"] == [cnt * n for _, cnt in c["shards"]]
        for r, (f, shard) in enumerate(zip(ranks, c["shards"])):
            se.assert_frame_state(f, o, shard, c["total"], c["wf_rows"], "%s frame %d (%s) rank %d" % (cid, frame, name, r),
                                  others_boot=(frame == 0))
    for f in ranks:
        f.close()


# ---- 4. table changes between relaxed calls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(wc.RELAXED_CASES))
def test_table_change_between_relaxed_calls_long(amd, torch_cuda, oracle_built, monkeypatch, cid):
    """test_gpu_parity.test_table_change_between_relaxed_calls at the long lengths: relaxed input ordering, every call cut into two
    pieces (on alternating FFT streams where the instance has two), four calls without synchronisation, a window in front of calls
    0 and 1, a power range in front of call 2, the default window in front of call 3.  A change must not reach the earlier call's
    spectra and must apply to all of the later call's: the state equals the oracle's after the same sequence."""
    torch = torch_cuda
    c = wc.RELAXED_CASES[cid]
    _set_env(monkeypatch, c["env"])
    n, nbat, b = 1 << c["log2n"], wc.RELAXED_BATCHES, wc.RELAXED_BATCH
    f = amd.Fosphor(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=wc.WF_ROWS, max_spectra=nbat * b, max_batches=nbat,
                    iq_format=c["fmt"])
    assert f.set_input_ordering(False) == 0
    o = Oracle(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=wc.WF_ROWS)
    keep = []
    for call in range(4):
        x, x32 = wc.as_format(add_tone(gaussian_iq(nbat * b * n, 9600 + call), 0.05, 0.0313 + 0.02 * call), c["fmt"])
        keep.append(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        if call in wc.RELAXED_WINDOWS:
            name = wc.RELAXED_WINDOWS[call]
            if name is None:
                f.set_fft_window_default(); o.set_window_default()
            else:
                f.set_fft_window(_window(name, n)); o.set_window(_window(name, n))
        if call in wc.RELAXED_POWER:
            f.set_power_range(*wc.RELAXED_POWER[call]); o.set_power_range(*wc.RELAXED_POWER[call])
        assert f.process_device(keep[-1], nbat, b) == 0			# no synchronisation between the calls
        for k in range(nbat):
            assert o.process(x32[k * b * n:(k + 1) * b * n], strict=False, nthreads=8) == 0
    assert f.finish() >= 0
    assert f.histo_scale == o.histo_scale and f.histo_offset == o.histo_offset
    compare_state(f, o, "%s: tables changed between relaxed calls" % cid)
    f.close()


# ---- 5. the zero window ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2n,fmt", [(10, "fp32"), (13, "fp32"), (16, "fp16")])
def test_zero_window_and_recovery(amd, torch_cuda, oracle_built, log2n, fmt):
    """Under the all-zero window every row written is -inf and every hit lands in bin 0 (log10(hypot(0, 0)), display.cl:136); the
    live spectrum is then not finite, and leaves that state with the next call, under ramp (display.cl:206-207, as the reference
    fixtures document): the state equals the oracle's."""
    torch = torch_cuda
    n, nb, ns = 1 << log2n, wc.DISCRIMINATION[log2n], 16
    f = amd.Fosphor(fft_len_log=log2n, n_bins=nb, wf_rows=wc.WF_ROWS, max_spectra=ns, iq_format=fmt)
    o = Oracle(fft_len_log=log2n, n_bins=nb, wf_rows=wc.WF_ROWS)
    x, x32 = wc.as_format(wc.discrimination_input(log2n), fmt)
    d = torch.from_numpy(x).cuda()
    f.set_fft_window(wc.zero(n)); o.set_window(wc.zero(n))
    assert f.process_device(d, 1, ns) == 0 and o.process(x32, strict=False, nthreads=8) == 0
    wf = f.waterfall
    assert np.all(np.isneginf(wf[:ns])) and np.all(wf[ns:] == np.float32(-f.histo_offset))
    hc = f.hitcount
    assert np.all(hc[0] == ns) and not hc[1:].any()
    assert not np.all(np.isfinite(f.spectrum[0, :, 1]))
    compare_state(f, o, "N = %d, zero window" % n)
    f.set_fft_window(wc.ramp(n)); o.set_window(wc.ramp(n))
    assert f.process_device(d, 1, ns) == 0 and o.process(x32, strict=False, nthreads=8) == 0
    assert np.all(np.isfinite(f.spectrum[0, :, 1])) and np.all(np.isfinite(f.waterfall[ns:2 * ns]))
    assert int(f.hitcount[1:].sum(dtype=np.uint64)) > ns * n // 2		# the hits have left bin 0
    compare_state(f, o, "N = %d, ramp after the zero window" % n)
    f.close()
