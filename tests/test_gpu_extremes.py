"""GPU: extreme and non-finite samples beside ordinary ones on every FFT kernel and hand-off (the batches, classes and kernel table
of tests/extreme_cases.py).

Every FFT kernel patches the samples its fast path could not settle back into its own index format and its own log-power registers;
until here only k1_fft_bin<iq_fp32>, one batch per launch, met a spectrum that takes bin_exact's full-search branch beside ordinary
ones (fixture c9_nonfinite_b16x2), and the zero window makes EVERY sample -inf / bin 0, so a patch of the wrong byte, lane, spectrum
or 9th bit passes under it.  Here spectra scaled by 1e30, 1e-30 and 1e-42, all-zero spectra, a tone whose bin overflows hypot with
finite parts, a NaN and an inf sample stand beside ordinary spectra, at every residue of the position in the batch, and go through
  1. the FFT hook of every instantiation: the words bit for bit the oracle's, subnormal ones included;
  2. every row of the kernel table one batch per call, the state against the oracle's after every batch (N = 1024: through
     fosphor_process as well);
  3. the same batches in ONE call: live sum and max-hold go non-finite in batch f and are taken back in batch f + 1 inside one launch
     (update_column, display.cl:206-207,290-291).  The hit counts a call exposes are its last batch's: they and form 2's are both held
     to the oracle's after the last batch, bit for bit;
  4. tests/tile_walk_cases.py's long calls, one per kernel, with the special spectra in tiles of units that take a SECOND tile, that
     tile in the call's last batch: a non-finite live / max partial must not reach the tile the same unit takes next;
  5. sharded frames on two emulated ranks: one rank's -inf meets the other's +inf in the float sum of the exchange.
Which parameter reaches which instantiation: extreme_cases.ROWS[rid]["kernel"] (test_batches_vs_oracle[rid-...]) and
window_cases.FFT_CASES[cid]["kernel"] (test_fft_hook_on_extreme_spectra[cid]); where a knob or a hop selects the kernel, the choice is
asserted through plan_k1.
The comparisons and bars are test_gpu_parity's (compare_state: ring position and counts exact, waterfall / live / max-hold rtol 1e-4
atol 1e-6 with inf and NaN matched by position, the histogram through assert_hist_close) and tests/shard_emul.py's; nothing here has
a tolerance of its own.  tests/test_extreme_cases_cpu.py proves on the oracle that the inputs reach what they claim."""
import numpy as np
import pytest

import extreme_cases as ec
import shard_emul as se
import tile_walk_cases as tw
import window_cases as wc
from oracle_lib import Oracle, canon_bits
from test_gpu_parity import amd, torch_cuda, compare_state	# noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _set_env(monkeypatch, env):
    for k in ec.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _samples(x, fmt, lo, hi):
    """samples [lo, hi) of an array as_format made"""
    return x[2 * lo:2 * hi] if fmt == "sc16" else x[lo:hi]


# ---- 1. the FFT hook ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(wc.FFT_CASES))
def test_fft_hook_on_extreme_spectra(amd, torch_cuda, oracle_built, monkeypatch, cid):
    """The `scaled` batch (a flushed subnormal in a packed-FMA pass of the long plans would show here) and the `nan` batch."""
    torch = torch_cuda
    c = wc.FFT_CASES[cid]
    _set_env(monkeypatch, c["env"])
    n = 1 << c["log2n"]
    f = amd.Fosphor(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=ec.WF_ROWS, max_spectra=ec.BATCH, iq_format=c["fmt"])
    w = Oracle(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=ec.WF_ROWS).window
    x, xo = ec.stream(c["log2n"], c["fmt"])
    d_out = torch.empty((ec.BATCH, n, 2), dtype=torch.float32, device="cuda")
    for name in ec.FFT_BATCHES:
        k = ec.ORDER.index(name)
        d_in = torch.tensor(_samples(x, c["fmt"], k * ec.BATCH * n, (k + 1) * ec.BATCH * n)).cuda()
        assert f.fft_device(d_in, d_out, ec.BATCH) == 0
        got = d_out.cpu().numpy()
        want = Oracle.fft(ec.batch_of(xo, c["log2n"], 1, k), w, fft_len_log=c["log2n"])
        differ = int((canon_bits(got) != canon_bits(want)).sum())
        assert differ == 0, "%s (%s), batch %s: %d words differ from the oracle's FFT" % (cid, c["kernel"], name, differ)
        if name == "scaled" and c["fmt"] == "fp32":
            assert ((np.abs(got) < 2.0 ** -126) & (got != 0)).sum() > n		# the subnormal words are there
    f.close()


# ---- 2. and 3. the whole path: one batch per call, all batches in one call --------------------------------------------------------------
FORMS = ("per_call", "one_call", "host")
_PATH = [(rid, rot, form) for rid, r in ec.ROWS.items() for rot in r["rots"] for form in FORMS if form != "host" or r["host"]]


@pytest.mark.parametrize("rid,rot,form", _PATH, ids=["%s-rot%d-%s" % p for p in _PATH])
def test_batches_vs_oracle(amd, torch_cuda, oracle_built, monkeypatch, rid, rot, form):
    """per_call: process_device / process_device_overlap once per batch, the state after each against the oracle's; host: the same
    through fosphor_process; one_call: process_device(d, n_batches, 16) over all batches, the state at the end."""
    torch = torch_cuda
    r = ec.ROWS[rid]
    _set_env(monkeypatch, r["env"])
    log2n, fmt, ov = r["log2n"], r["fmt"], r["overlap"]
    n, nb = 1 << log2n, len(ec.ORDER)
    hop = n // ov
    one = form == "one_call"
    f = amd.Fosphor(fft_len_log=log2n, n_bins=r["n_bins"], wf_rows=ec.WF_ROWS, max_spectra=ec.MAX_SPECTRA if one else ec.BATCH,
                    max_batches=nb if one else 2, iq_format=fmt)
    o = ec.make_oracle(r)
    if r["power"]:
        f.set_power_range(*r["power"])
    assert (f.histo_scale, f.histo_offset) == (o.histo_scale, o.histo_offset)
    x, xo = ec.stream(log2n, fmt, ov, rot)
    d = None
    if form != "host":
        d = torch.tensor(x).cuda()
        torch.cuda.synchronize()
    n_cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count

    def plan(ptr, total):
        p = amd.plan_k1(log2n, r["n_bins"], fmt, hop, ptr % 16, total, ec.BATCH, k1_knob=int(r["env"].get("FOSPHOR_AMD_K1", 1)), n_cus=n_cus)
        assert p["kernel"] == r["plan"], "%s: the launch would take %s" % (rid, p)

    def call(dk, n_batches):
        if r["entry"] == "overlap":
            return f.process_device_overlap(dk, n_batches, ec.BATCH, ov)
        return f.process_device(dk, n_batches, ec.BATCH)

    if one:
        plan(d.data_ptr(), ec.MAX_SPECTRA)
        assert call(d, nb) == 0
    for k, name in enumerate(ec.ORDER):
        what = "%s (%s), rotation %d, %s, batch %d (%s)" % (rid, r["kernel"], rot, form, k, name)
        assert o.process(ec.batch_of(xo, log2n, ov, k), strict=False, nthreads=8) == 0
        if one:
            continue
        lo = k * ec.BATCH * hop
        hi = lo + (ec.BATCH - 1) * hop + n
        if form == "host":
            assert f.process(np.ascontiguousarray(_samples(x, fmt, lo, hi))) == 0, what
        else:
            dk = _samples(d, fmt, lo, hi)
            plan(dk.data_ptr(), ec.BATCH)
            assert call(dk, 1) == 0, what
        assert int(f.hitcount.sum(dtype=np.uint64)) == ec.BATCH * n, what + ": the counts do not add up to the batch"
        compare_state(f, o, what)
    if one:
        what = "%s (%s), rotation %d, all %d batches in one call" % (rid, r["kernel"], rot, nb)
        assert f.finish() >= 0
        assert int(f.hitcount.sum(dtype=np.uint64)) == ec.BATCH * n, what + ": the counts do not add up to the last batch"
        compare_state(f, o, what)
    # the sequence ends recovered: nothing non-finite is left in the live trace (with an overlap the last altered window reaches
    # into `recover`, and `recover2` takes the trace back)
    assert np.all(np.isfinite(f.spectrum[0, :, 1])), rid
    f.close()


# ---- 4. tile walks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ec.WALK_CASES)
def test_non_finite_tiles_in_front_of_a_units_next_tile(amd, torch_cuda, oracle_built, monkeypatch, cid):
    """The call of tile_walk_cases.CASES[cid] as tabled there, with an all-zero spectrum, an overflow tone, a x 1e30, a x 1e-30 and a
    NaN spectrum one to a tile (hop 1: a NaN and a x 1e30 sample at the head) in first-pass tiles whose units take their next tile in
    the LAST batch: a partial that leaked across the tile boundary would stand in the live / max-hold the call leaves."""
    torch = torch_cuda
    c = tw.CASES[cid]
    n, total = 1 << c["log2n"], tw.total(c)
    what = "%s (%s), %d x %d spectra" % (cid, c["kernel"], c["n_batches"], c["batch"])
    for k in tw.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    n_cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    p = amd.plan_k1(c["log2n"], c["n_bins"], c["fmt"], tw.hop(c), 0, total, c["batch"], tile_knob=int(c["env"].get("FOSPHOR_AMD_TILE", 0)),
                    k1_knob=int(c["env"].get("FOSPHOR_AMD_K1", 1)), n_cus=n_cus)
    assert p["kernel"] == c["kernel"] and p["max_tiles"] >= 2 and p["tiles"] * p["tile"] == total, "%s: %s" % (what, p)
    tiles = (range(ec.WALK_HOP1_HEAD[-1][1] // p["tile"] + 1) if c["overlap"] > ec.BATCH
             else [g // p["tile"] for _, _, g in ec.walk_placed(c, p)])
    for t in tiles:		# the special tiles' units take a second tile, in the last batch
        assert t + p["units"] < p["tiles"] and (t + p["units"]) * p["tile"] >= total - c["batch"] > t * p["tile"], what
    x = ec.walk_stream(c, tw.stream(cid)[1], p)
    f = amd.Fosphor(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=c["wf_rows"], max_spectra=total, max_batches=c["n_batches"],
                    iq_format=c["fmt"])
    o = Oracle(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=c["wf_rows"])
    tw.oracle_call(o, c, "batches", x, nthreads=16)
    assert np.all(np.isfinite(o.spectrum[0, :, 1]))		# the special batch is long taken back: a leak is all that could be non-finite
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    assert d.data_ptr() % 16 == 0
    assert f.finish() >= 0
    if c["overlap"] > 1:
        assert f.process_device_overlap(d, c["n_batches"], c["batch"], c["overlap"]) == 0, what
    else:
        assert f.process_device(d, c["n_batches"], c["batch"]) == 0, what
    assert f.finish() >= 0
    assert int(f.hitcount.sum(dtype=np.uint64)) == c["batch"] * n, what
    compare_state(f, o, what)
    f.close()


# ---- 5. sharded frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(ec.SHARD_CASES))
def test_sharded_frames_with_non_finite_partials(amd, torch_cuda, oracle_built, monkeypatch, cid):
    """Frame 0: the all-zero spectra on rank 0, the overflow tones on rank 1 (-inf + +inf = NaN in the tones' columns of the summed
    live partials, +inf in the max); frame 1: the tones on rank 0, a x 1e30 and a x 1e-30 spectrum on rank 1.  Two ranks accumulate a
    shard each, tests/shard_emul.py's exchange, merge; every rank against ONE oracle launch over the whole frame."""
    torch = torch_cuda
    c = ec.SHARD_CASES[cid]
    for k in se.KNOBS:
        monkeypatch.delenv(k, raising=False)
    n = 1 << c["log2n"]
    o = se.make_oracle(c)
    ranks = se.make_ranks(amd, c)
    keep = []
    for frame in range(c["frames"]):
        x, x32 = ec.shard_stream(c, frame)
        se.oracle_frame(o, c, x32)
        keep.append(torch.from_numpy(x).cuda())
        res = se.run_sharded_frame(amd, torch, ranks, keep[-1], c["shards"], c["total"], overlap=c["overlap"])
        assert res["hc_sums"] == [cnt * n for _, cnt in c["shards"]]
        live = o.spectrum[0, :, 1]
        assert (np.isnan(live).sum() == 2) if frame == 0 else (np.isposinf(live).sum() == 2)
        for rk, (f, shard) in enumerate(zip(ranks, c["shards"])):
            se.assert_frame_state(f, o, shard, c["total"], c["wf_rows"], "%s frame %d rank %d" % (cid, frame, rk),
                                  others_boot=(frame == 0))
            if frame == 1:
                hc = f.hitcount
                assert np.all(hc[0] >= 1) and np.all(hc[c["n_bins"] - 1] >= 1)		# hits in bin 0 and in the top bin
    for f in ranks:
        f.close()
