"""Interleaved int16 (sc16) IQ: FOSPHOR_AMD_IQ_SC16 at fft_len_log 10, 13 and 16.

The sample value is i * 2^-15 and the widening is exact, so an sc16 instance must leave every buffer BIT-IDENTICAL to an fp32
instance of the same geometry fed x.astype(float32) * 2**-15 through the same calls (hit counts, histogram, waterfall and its ring
position, live / max-hold spectrum).  At N = 65536 the reference format is fp16 (exact for |i| <= 2048)."""
import errno

import numpy as np
import pytest

from oracle_lib import Oracle, canon_bits

pytestmark = pytest.mark.gpu

SCALE = np.float32(2.0 ** -15)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    return torch


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    gr_fosphor_amd.load()
    return gr_fosphor_amd


def sc16_iq(n_samples, seed, sigma=3000.0, tone=None):
    """int16 pairs [n_samples * 2]: clipped Gaussian noise (+ an optional tone), with the extremes planted near the start."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, sigma, 2 * n_samples)
    if tone is not None:
        amp, freq = tone
        t = np.arange(n_samples)
        v[0::2] += amp * np.cos(2 * np.pi * freq * t)
        v[1::2] += amp * np.sin(2 * np.pi * freq * t)
    x = np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    x[:8] = [-32768, 32767, 0, 1, -1, -32768, 32767, -1]
    return x


def widen(x):
    return x.astype(np.float32) * SCALE


def state(f):
    return {"hitcount": f.hitcount, "histogram": canon_bits(f.histogram), "waterfall": canon_bits(f.waterfall),
            "spectrum": canon_bits(f.spectrum), "waterfall_pos": f.waterfall_pos}


def assert_same_state(a, b, what):
    sa, sb = state(a), state(b)
    for k in sa:
        assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), "%s: %s differs (%s words)" % (
            what, k, np.sum(np.asarray(sa[k]) != np.asarray(sb[k])))


# ---- the FFT hook: bit-exact against the oracle's FFT of the widened input --------------------------------------------------
@pytest.mark.parametrize("log2n", [10, 13, 16])
def test_fft_hook_bit_exact(amd, torch_cuda, oracle_built, log2n):
    torch = torch_cuda
    n, ns = 1 << log2n, 8
    f = amd.Fosphor(fft_len_log=log2n, n_bins=512 if log2n == 16 else 128, wf_rows=64, max_spectra=16, iq_format="sc16")
    x = sc16_iq(ns * n, 11 + log2n).reshape(ns, n, 2)
    x[1] = 0						# an all-zero spectrum
    t = np.arange(n)
    x[2, :, 0] = np.clip(np.rint(32767 * np.cos(2 * np.pi * 37 * t / n)), -32768, 32767)	# full-scale tone
    x[2, :, 1] = np.clip(np.rint(32767 * np.sin(2 * np.pi * 37 * t / n)), -32768, 32767)
    x[3] = -32768
    x[4, ::2] = 32767
    d_in = torch.from_numpy(x.reshape(-1)).cuda()
    d_out = torch.empty((ns, n, 2), dtype=torch.float32, device="cuda")
    assert f.fft_device(d_in, d_out, ns) == 0
    o = Oracle(fft_len_log=log2n, n_bins=512 if log2n == 16 else 128, wf_rows=64)
    want = Oracle.fft(widen(x), o.window, fft_len_log=log2n)
    got = d_out.cpu().numpy()
    assert np.array_equal(canon_bits(got), canon_bits(want)), "%d words differ" % (canon_bits(got) != canon_bits(want)).sum()
    f.close()


# ---- the whole path against an fp32 instance ------------------------------------------------------------------------------
N1024 = [  # (n_bins, overlap, batch, n_batches, calls, window)
    (128, 1, 64, 1, 3, False),		# variant 1, state carried over three calls
    (256, 1, 128, 4, 2, False),		# NB256, multi-batch launches
    (512, 1, 64, 2, 2, False),		# k1big (16-bit bin indices)
    (128, 1024, 64, 1, 2, False),	# hop 1: odd, variant 2
    (128, 2, 64, 3, 2, True),		# overlap 2, a loaded window
]


def _run_pair(amd, torch, log2n, n_bins, overlap, batch, n_batches, calls, window, seed, offset=0, sigma=3000.0):
    n = 1 << log2n
    hop = n // overlap
    total = n_batches * batch
    need = (total - 1) * hop + n
    fs = amd.Fosphor(fft_len_log=log2n, n_bins=n_bins, wf_rows=256, max_spectra=total, max_batches=max(n_batches, 8),
                     iq_format="sc16")
    ff = amd.Fosphor(fft_len_log=log2n, n_bins=n_bins, wf_rows=256, max_spectra=total, max_batches=max(n_batches, 8))
    if window:
        w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)
        fs.set_fft_window(w)
        ff.set_fft_window(w)
    for c in range(calls):
        x = sc16_iq(need + offset, seed + c, sigma=sigma, tone=(8000.0, 0.123))
        ds = torch.from_numpy(x).cuda()[2 * offset:]
        df = torch.from_numpy(widen(x)).cuda()[2 * offset:]
        if overlap == 1:
            assert fs.process_device(ds, n_batches, batch) == 0
            assert ff.process_device(df, n_batches, batch) == 0
        else:
            assert fs.process_device_overlap(ds, n_batches, batch, overlap) == 0
            assert ff.process_device_overlap(df, n_batches, batch, overlap) == 0
    fs.finish()
    ff.finish()
    return fs, ff


@pytest.mark.parametrize("case", N1024, ids=["v1_b128", "nb256_multibatch", "k1big_b512", "v2_odd_hop", "overlap2_window"])
def test_n1024_bit_identical_to_fp32(amd, torch_cuda, case):
    fs, ff = _run_pair(amd, torch_cuda, 10, *case, seed=100)
    assert_same_state(fs, ff, "N=1024 %s" % (case,))
    fs.close(); ff.close()


def test_n1024_4_byte_aligned_start(amd, torch_cuda):
    """A start that is 4- but not 8-byte aligned takes the 4-byte-per-lane kernel: same results."""
    fs, ff = _run_pair(amd, torch_cuda, 10, 128, 1, 64, 2, 2, False, seed=140, offset=1)
    assert_same_state(fs, ff, "N=1024, start at 4 mod 8")
    fs.close(); ff.close()


@pytest.mark.parametrize("overlap", [2, 4, 8, 16, 32])
def test_n8192_bit_identical_to_fp32(amd, torch_cuda, overlap):
    fs, ff = _run_pair(amd, torch_cuda, 13, 512, overlap, 64, 2, 2, False, seed=200 + overlap)
    assert_same_state(fs, ff, "N=8192 overlap %d" % overlap)
    fs.close(); ff.close()


def test_n8192_space_sharing_shape_bit_identical(amd, torch_cuda):
    """14 batches of 1024, overlap 2, calls back to back: the FFT launch may run on 224 CUs beside the previous launch's tail."""
    fs, ff = _run_pair(amd, torch_cuda, 13, 512, 2, 1024, 14, 2, False, seed=300)
    assert_same_state(fs, ff, "N=8192 14 x 1024")
    fs.close(); ff.close()


def test_n65536_equals_fp16_and_oracle_counts(amd, torch_cuda, oracle_built):
    torch = torch_cuda
    n, ns = 65536, 16
    # |i| <= 2048: i * 2^-15 is exact in fp16 as well
    x = np.clip(sc16_iq(ns * n, 400, sigma=600.0), -2048, 2048).astype(np.int16)
    fs = amd.Fosphor(fft_len_log=16, n_bins=512, wf_rows=64, max_spectra=ns, iq_format="sc16")
    fh = amd.Fosphor(fft_len_log=16, n_bins=512, wf_rows=64, max_spectra=ns, iq_fp16=True)
    for c in range(2):
        assert fs.process_device(torch.from_numpy(x).cuda(), 1, ns) == 0
        assert fh.process_device(torch.from_numpy(widen(x).astype(np.float16)).cuda(), 1, ns) == 0
    fs.finish(); fh.finish()
    assert_same_state(fs, fh, "N=65536 sc16 vs fp16")
    fs.close(); fh.close()
    # the full int16 range: counts equal to the oracle's
    x = sc16_iq(ns * n, 401, sigma=12000.0, tone=(20000.0, 0.01))
    fs = amd.Fosphor(fft_len_log=16, n_bins=512, wf_rows=64, max_spectra=ns, iq_format="sc16")
    assert fs.process_device(torch.from_numpy(x).cuda(), 1, ns) == 0
    fs.finish()
    o = Oracle(fft_len_log=16, n_bins=512, wf_rows=64)
    assert o.process(widen(x).reshape(-1, 2), strict=False, nthreads=8) == 0
    assert np.array_equal(fs.hitcount, o.hitcount.T)
    fs.close()


# ---- host entry points ----------------------------------------------------------------------------------------------------
def test_host_entry_points_equal_process_device(amd, torch_cuda):
    torch = torch_cuda
    n, batch = 1024, 64
    x = sc16_iq(batch * n, 500, tone=(9000.0, 0.2))
    ref = amd.Fosphor(iq_format="sc16")
    assert ref.process_device(torch.from_numpy(x).cuda(), 1, batch) == 0
    ref.finish()

    f = amd.Fosphor(iq_format="sc16")
    assert f.process(x) == 0
    assert f.process(x[: 2 * 1000]) == -errno.EINVAL		# not a multiple of 16 spectra
    assert f.process(np.zeros((0,), np.int16)) == -errno.EINVAL
    f.finish()
    assert_same_state(f, ref, "fosphor_process (flat int16)")
    f.close()

    f = amd.Fosphor(iq_format="sc16")
    assert f.process(x.reshape(-1, 2)) == 0			# (n, 2) form
    f.finish()
    assert_same_state(f, ref, "fosphor_process ((n, 2) int16)")
    f.close()

    pinned = torch.from_numpy(x).pin_memory()
    f = amd.Fosphor(iq_format="sc16")
    assert f.L.fosphor_amd_process_pinned(f.h, pinned.data_ptr(), 2 * 1000) == -errno.EINVAL
    assert f.L.fosphor_amd_process_pinned(f.h, pinned.data_ptr(), batch * n) == 0
    f.finish()
    assert_same_state(f, ref, "process_pinned")
    f.close()

    f = amd.Fosphor(iq_format="sc16")
    assert f.L.fosphor_amd_upload_pinned(f.h, pinned.data_ptr(), batch * n) == 0
    assert f.L.fosphor_amd_process_uploaded(f.h, None) == 0
    f.finish()
    assert_same_state(f, ref, "upload_pinned / process_uploaded")
    f.close()
    ref.close()


def test_device_argument_errors(amd, torch_cuda):
    torch = torch_cuda
    f = amd.Fosphor(iq_format="sc16", max_spectra=64)
    d = torch.zeros(2 * 65 * 1024 + 4, dtype=torch.int16, device="cuda")
    assert f.process_device(d, 1, 8) == -errno.EINVAL			# batch % 16
    assert f.process_device(d, 2, 64) == -errno.EINVAL			# over capacity
    assert f.process_device_overlap(d, 1, 64, 3) == -errno.EINVAL	# overlap must divide N
    assert f.process_device(d[1:], 1, 64) == -errno.EINVAL		# 2-byte aligned: misaligned sc16 pointer
    assert f.process_device_overlap(d[1:], 1, 64, 2) == -errno.EINVAL
    assert f.accumulate_device(d[1:], 64, 0, 64) == -errno.EINVAL
    out = torch.empty((4, 1024, 2), dtype=torch.float32, device="cuda")
    assert f.fft_device(d[1:], out, 4) == -errno.EINVAL
    import ctypes as C
    ms = C.c_float()
    assert f.L.fosphor_amd_traffic_twin(f.h, d.data_ptr(), 1, 64, 1, C.byref(ms)) == -errno.EINVAL
    assert f.process_device(d[2:], 1, 64) == 0				# 4-byte aligned is fine
    f.finish()
    with pytest.raises(ValueError):
        f.process_device(torch.zeros(2 * 64 * 1024, dtype=torch.float32, device="cuda"), 1, 64)
    with pytest.raises(ValueError):
        f.accumulate_device(torch.zeros(2 * 64 * 1024, dtype=torch.float32, device="cuda"), 64, 0, 64)
    f.close()


def test_python_dtype_checks_and_unknown_format(amd, torch_cuda):
    f = amd.Fosphor(iq_format="sc16")
    with pytest.raises(TypeError):
        f.process(np.zeros(2 * 16 * 1024, np.float32))
    with pytest.raises(TypeError):
        f.process(np.zeros(2 * 16 * 1024, np.int32))
    with pytest.raises(TypeError):
        f.process(list(range(32)))
    with pytest.raises(TypeError):
        f.process(np.zeros((16 * 1024, 3), np.int16))
    f.close()
    with pytest.raises(RuntimeError):
        amd.Fosphor(iq_format=3)
    with pytest.raises(RuntimeError):
        amd.Fosphor(fft_len_log=13, iq_format="fp16")	# the fp16-only-at-16 rule stays
    with pytest.raises(ValueError):
        amd.Fosphor(iq_format="s16")
    g = amd.Fosphor(iq_fp16=True, fft_len_log=16, n_bins=512, wf_rows=64, max_spectra=16)
    assert g.iq_fp16 and g.iq_format == 1
    g.close()


# ---- the multi-GPU split with sc16 shards ---------------------------------------------------------------------------------
def test_sharded_sc16_equals_single_instance(amd, torch_cuda):
    """Two emulated ranks accumulate halves of one 2048-spectrum batch from slices of ONE int16 tensor; the partials are
    combined as the all-reduce would; one merge each: every buffer equals a single sc16 instance's (rank 1: the waterfall too)."""
    torch = torch_cuda
    from gr_fosphor_amd.dist import shard_range, wrap_device_array
    total, n = 2048, 1024
    x = sc16_iq(total * n, 600, tone=(7000.0, 0.31))
    d = torch.from_numpy(x).cuda()
    single = amd.Fosphor(max_spectra=total, iq_format="sc16")
    assert single.process_device(d, 1, total) == 0
    single.finish()
    ranks = [amd.Fosphor(max_spectra=total, iq_format="sc16") for _ in range(2)]
    parts = []
    for r, fr in enumerate(ranks):
        off, cnt = shard_range(total, r, 2)
        assert fr.accumulate_device(d[2 * off * n:2 * (off + cnt) * n], cnt, off, total) == 0
        fr.finish()
        parts.append(fr.partials())
    hc = [wrap_device_array(p.d_hc, (p.n_hc,), torch.int32) for p in parts]
    ls = [wrap_device_array(p.d_live_sum, (p.n_cols,), torch.float32) for p in parts]
    mx = [wrap_device_array(p.d_max, (p.n_cols,), torch.float32) for p in parts]
    hc_sum, ls_sum, mx_max = hc[0] + hc[1], ls[0] + ls[1], torch.maximum(mx[0], mx[1])
    for r in range(2):
        hc[r].copy_(hc_sum); ls[r].copy_(ls_sum); mx[r].copy_(mx_max)
    torch.cuda.synchronize()
    for fr in ranks:
        assert fr.merge(total) == 0
        fr.finish()
        assert np.array_equal(fr.hitcount, single.hitcount)
        assert fr.waterfall_pos == single.waterfall_pos
    # a sharded frame equals the single launch up to the float sums' order; compare to an fp32 pair run the same way
    ref = [amd.Fosphor(max_spectra=total) for _ in range(2)]
    dfl = torch.from_numpy(widen(x)).cuda()
    parts = []
    for r, fr in enumerate(ref):
        off, cnt = shard_range(total, r, 2)
        assert fr.accumulate_device(dfl[2 * off * n:2 * (off + cnt) * n], cnt, off, total) == 0
        fr.finish()
        parts.append(fr.partials())
    hc = [wrap_device_array(p.d_hc, (p.n_hc,), torch.int32) for p in parts]
    ls = [wrap_device_array(p.d_live_sum, (p.n_cols,), torch.float32) for p in parts]
    mx = [wrap_device_array(p.d_max, (p.n_cols,), torch.float32) for p in parts]
    hc_sum, ls_sum, mx_max = hc[0] + hc[1], ls[0] + ls[1], torch.maximum(mx[0], mx[1])
    for r in range(2):
        hc[r].copy_(hc_sum); ls[r].copy_(ls_sum); mx[r].copy_(mx_max)
    torch.cuda.synchronize()
    for fr in ref:
        assert fr.merge(total) == 0
        fr.finish()
    for a, b in zip(ranks, ref):
        assert_same_state(a, b, "sharded sc16 vs sharded fp32")
    for fr in ranks + ref + [single]:
        fr.close()
