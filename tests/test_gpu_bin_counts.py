"""GPU: bin counts other than 128, 256 and 512 at every FFT length (the cases and inputs of tests/bin_count_cases.py).

fosphor_init accepts any multiple of 16 from 16 to 512 at all three lengths, and the count is no passive size: it selects the index
format, a kernel instantiation of its own at 256, the size of the count kernel's LDS histogram and row bitmask, and the divisions
of the merge kernels.  Here 16, 48, 240, 256, 272, 496 and 512 bins go through FFT -> bin -> count -> merge at 1024, 8192 and 65536
points against the oracle, with test_gpu_parity's comparison and bars (compare_state: counts exact, floats in its tolerances) and
nothing of their own; the indices alone by test_bin_exact's method; sharded frames through the compact exchange in both forms
(tests/shard_emul.py BIN_COUNT_CASES; tests/test_gpu_shard_matrix.py runs the same cases through the plain sum); and the readers
of histogram rows -- percentiles, the view's histogram picture, the colour map -- against the models their own tests use.
tests/test_bin_counts_cpu.py holds the oracle to a numpy statement at these counts and asserts the conditions on the inputs."""
import numpy as np
import pytest

import bin_count_cases as bc
import detect_model as dm
import shard_emul as se
import wire_cases as wc
from oracle_lib import oracle_bins
from test_cmap import GOLD, oracle, oracle_colorize				# noqa: F401  (oracle: fixture)
from test_gpu_detect import Planted, Q4, percentile_histogram, run_percentiles, same_f32
from test_gpu_parity import amd, torch_cuda, _bin_inputs, assert_close, compare_state	# noqa: F401  (fixtures)
from test_gpu_view import AVERAGE, PEAK, State, check_view
from test_gpu_wire import FORMS, _accumulate, emulated_compact_exchange

pytestmark = pytest.mark.gpu

WHOLE = [(log2n, nb, bc.FMT[log2n]) for log2n in (10, 13, 16) for nb in bc.COUNTS] + \
        [(log2n, nb, "sc16") for log2n, nb in sorted(bc.SC16_COUNT.items())]


@pytest.mark.parametrize("log2n,n_bins,fmt", WHOLE)
def test_whole_path_vs_oracle(amd, torch_cuda, oracle_built, log2n, n_bins, fmt):
    """Two or three calls per case (bin_count_cases.CALLS: the host path, a multi-batch call, the overlapped read at 8192 points),
    so that the merge runs on a non-empty histogram and the 64-row ring advances and wraps; after every call the whole state
    against the oracle's.  The condition on the input -- hits in row 0, in the last row and, above 256 bins, on both sides of
    row 256 -- is asserted on the oracle's counts before the device's are looked at."""
    torch = torch_cuda
    n = 1 << log2n
    f = amd.Fosphor(fft_len_log=log2n, n_bins=n_bins, wf_rows=bc.WF_ROWS, max_spectra=bc.MAX_SPECTRA[log2n], max_batches=2,
                    iq_format=fmt)
    o = bc.make_oracle(log2n, n_bins)
    f.set_power_range(*bc.RANGES[log2n])
    assert f.histo_scale == o.histo_scale and f.histo_offset == o.histo_offset
    keep = []
    for k, (call, (x, x32)) in enumerate(zip(bc.CALLS[log2n], bc.streams(log2n, fmt))):
        kind, nbat, batch, overlap = call
        what = "N %d, %d bins, %s, call %d %s" % (n, n_bins, fmt, k, call)
        bc.oracle_call(o, log2n, call, x32)
        bc.assert_covers(o.hitcount, n_bins, what, every_row=False)
        if kind == "host":
            assert f.process(x) == 0
        else:
            keep.append(torch.tensor(x).cuda())
            if overlap > 1:
                assert f.process_device_overlap(keep[-1], nbat, batch, overlap) == 0
            else:
                assert f.process_device(keep[-1], nbat, batch) == 0
        assert f.finish() >= 0
        assert int(f.hitcount.sum(dtype=np.uint64)) == batch * n, what + ": the counts do not add up to the batch"
        compare_state(f, o, what)
    f.close()


@pytest.mark.parametrize("log2n", [10, 13])
@pytest.mark.parametrize("n_bins", [272, 496])
def test_indices_alone(amd, torch_cuda, oracle_built, monkeypatch, log2n, n_bins):
    """test_gpu_parity.test_bin_exact's method and inputs (every float around every bin edge, 60 decades of magnitudes, the specials)
    at counts strictly between 256 and 512, on a 1024-point and on an 8192-point instance: the indices the FFT kernels' epilogue
    forms, 16 bits each through this entry point at both lengths, bit-equal to the oracle's with the fast and with the exact form.
    (How the 8192- and 65536-point kernels then split them into low bytes and a plane of 9th bits is seen by the whole path.)"""
    torch = torch_cuda
    f = amd.Fosphor(fft_len_log=log2n, n_bins=n_bins, wf_rows=bc.WF_ROWS, max_spectra=bc.MAX_SPECTRA[log2n])
    o = bc.make_oracle(log2n, n_bins)
    f.set_power_range(*bc.RANGES[log2n])
    assert f.histo_scale == o.histo_scale and f.histo_offset == o.histo_offset
    v = _bin_inputs(o, n_bins)
    d = torch.from_numpy(v).cuda()
    d_bin = torch.empty(v.shape[0], dtype=torch.int16, device="cuda")
    d_pwr = torch.empty(v.shape[0], dtype=torch.float32, device="cuda")
    want_bin, want_pwr = oracle_bins(v, o.histo_scale, o.histo_offset, n_bins)
    assert want_bin.min() == 0 and want_bin.max() == n_bins - 1 and np.unique(want_bin).size == n_bins
    for force in ("0", "1"):
        monkeypatch.setenv("FOSPHOR_AMD_FORCE_EXACT_BIN", force)
        assert f.bin_device(d, d_bin, d_pwr, v.shape[0]) == 0
        got = d_bin.cpu().numpy().astype(np.int32)
        bad = got != want_bin
        assert not bad.any(), "force=%s: %d bins differ, e.g. %r -> gpu %d oracle %d" % (
            force, bad.sum(), v[np.argmax(bad)], got[np.argmax(bad)], want_bin[np.argmax(bad)])
        assert_close(d_pwr.cpu().numpy(), want_pwr, "pwr (force=%s)" % force)
    f.close()


@pytest.mark.parametrize("form", ["packed16", "sparse16"])
@pytest.mark.parametrize("cid", se.BIN_COUNT_CASES)
def test_sharded_frames_through_the_compact_exchange(amd, torch_cuda, oracle_built, monkeypatch, cid, form):
    """The bin-count cases of the shard table, two ranks, through mask -> all-gather -> pack -> all-reduce -> unpack in both wire
    forms (tests/test_gpu_wire.py's emulated exchange): every rank's slot holds the oracle's counts of the whole frame, the wire
    words are the numpy statement's, the sparse form really ran, and after the merge every rank holds the state of one launch."""
    from gr_fosphor_amd.dist import wire_pack_numpy, wire_mask_numpy, wire_union_rows, wrap_device_array
    torch = torch_cuda
    c = se.CASES[cid]
    for k in se.KNOBS:
        monkeypatch.delenv(k, raising=False)
    n, nb, total = 1 << c["log2n"], c["n_bins"], c["total"]
    o = se.make_oracle(c)
    ranks = se.make_ranks(amd, c)
    keep = []
    for frame in range(c["frames"]):
        x, x32 = se.make_stream(c, frame)
        se.oracle_frame(o, c, x32)
        want = wc.oracle_counts(o)
        if nb > 256:
            lo, hi = se.plane_fractions(o)
            assert lo >= 0.01 and hi >= 0.01, "case %s: rows < 256 hold %.4f, rows >= 256 hold %.4f of the hits" % (cid, lo, hi)
        keep.append(torch.from_numpy(x).cuda())
        _accumulate(torch, ranks, keep[-1], c)
        st0 = [f.wire_stats() for f in ranks]
        res = emulated_compact_exchange(torch, ranks, total, form)
        d_want = torch.from_numpy(want.view(np.int32)).cuda()
        for r, f in enumerate(ranks):
            p = f.partials()
            assert p.n_hc == nb * n
            assert torch.equal(wrap_device_array(p.d_hc, (p.n_hc,), torch.int32), d_want), \
                "case %s frame %d rank %d: slot after the unpack" % (cid, frame, r)
        if form == "sparse16":
            # the presence mask has one bit per row of 64 cells of the whole [bin][x] array: n_bins * N / 64 rows, a whole number
            # of 32-bit words at every count the library accepts (n_bins * N / 2048), however n_bins / 32 rounds
            for f in ranks:
                i = f.wire_info()
                assert i.rows == nb * n // 64 and i.mask_words == -(-i.rows // 32) == nb * n // 2048 and i.world == len(ranks)
            live = wc.live_rows(want)
            rows, fall_back = wire_union_rows(wire_mask_numpy(want))
            assert not fall_back and 0.01 < live / (want.size // 64) < 0.5
            for f, a, p in zip(ranks, st0, res["packs"]):
                b = f.wire_stats()
                assert b["sparse16"] == a["sparse16"] + 1 and b["fell_back"] == a["fell_back"], "the sparse form did not run"
                assert p.form == FORMS["sparse16"] and p.live_rows == b["live_rows"] == live and p.n_words == 32 * live
            assert np.array_equal(np.bitwise_or.reduce(res["masks"], axis=0), wire_mask_numpy(want))
            assert np.array_equal(res["summed"], wire_pack_numpy(want, rows))
        else:
            assert all(p.form == FORMS["packed16"] and p.n_words == nb * n // 2 for p in res["packs"])
            assert np.array_equal(res["summed"], wire_pack_numpy(want))
        for f in ranks:
            assert f.merge(total) == 0
        for f in ranks:
            assert f.finish() >= 0
        for r, (f, shard) in enumerate(zip(ranks, c["shards"])):
            se.assert_frame_state(f, o, shard, total, c["wf_rows"], "case %s frame %d rank %d (%s)" % (cid, frame, r, form),
                                  others_boot=(frame == 0))
    for f in ranks:
        f.close()


@pytest.mark.parametrize("log2n,n_bins", [(10, 48), (13, 272)])
def test_readers_of_histogram_rows(amd, torch_cuda, oracle, log2n, n_bins):
    """A histogram planted as tests/test_gpu_detect.py plants it, at a count that is no multiple of the 32 rows the percentile
    kernel loads ahead: the percentile bins and levels against detect_model, the view's histogram picture against view_ref (the
    identity, exact, and a zoomed average within view_ref's bound), the colour-mapped histogram against the oracle's lookup."""
    s = Planted(amd, log2n, n_bins)
    n = s.n
    h = percentile_histogram(n, n_bins)
    s.plant(hist=h)
    want = dm.percentile_bins(h, Q4)
    assert want[:, n // 2].tolist() == [0] * 4 and want[:, 0].tolist() == [n_bins - 1] * 4 and want.max() == n_bins - 1
    rv, y, b = run_percentiles(s, Q4)
    assert rv == 0
    assert np.array_equal(b, want), "%d percentile bins differ" % (b != want).sum()
    assert same_f32(y, dm.percentile_y(want, s.table))
    s.assert_untouched()
    # a picture: values in [0, 1.1] and beyond, every row different
    pic = np.sqrt(h / np.float32(900.0)).astype(np.float32)
    assert pic.max() > 1.0 and pic.min() == 0.0
    s.plant(hist=pic)
    st = State(s.f)
    assert np.array_equal(st.hist, pic)
    check_view(st, 0, n, n, s.f.wf_rows, s.f.wf_rows, PEAK, what=("histogram",))
    check_view(st, n // 2 - 301, 777, 200, s.f.wf_rows, s.f.wf_rows, AVERAGE, what=("histogram",))
    img = s.f.colorize(1).cpu().numpy().view(np.uint32).reshape(n_bins, n)
    assert np.array_equal(img, oracle_colorize(oracle, 1, pic, 0, GOLD["histogram_256"], 1.1, 0.0, n_bins))
    assert len(np.unique(img)) > 20
    s.assert_untouched()
    s.f.close()
