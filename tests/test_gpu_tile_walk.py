"""GPU: the FFT kernels where one wave or work-group takes several tiles (the cases of tests/tile_walk_cases.py).

Every FFT-and-bin kernel is persistent -- a unit takes tile t, then t + stride, ... -- and what it carries across a tile boundary
(the prefetch of the next tile's first spectrum and its guard, the per-tile reset of the live / max partials, k1_fft_bin's bin
dwords flushed one spectrum late, k1w_fft_bin's held registers, the partial row index) runs only when a launch has more tiles than
its grid has units.  The default tile rule gives almost every call one tile per unit, so the rest of the suite enters the second
iteration of those loops in two multi-minute tests of the N = 8192 kernel and, for the N = 1024 kernels, nowhere.

Each case runs twice, on fresh instances over the same samples:
  batches    the call as tabled (batches up to 1088 spectra: the pipeline's 16-bit count hand-off), against the oracle fed the same
             batches one at a time;
  one_batch  the same spectra as ONE batch of `total` spectra: the hit counts a call exposes are its last batch's, so here they cover
             every tile of the walk, bit for bit.
Before either, the test asks fosphor_amd_plan_k1 -- the function the launch takes its tile, kernel and grid from -- with the
device's CU count and the sample pointer's alignment, and asserts the walk it is about to test: some unit takes two tiles or more,
some unit fewer.  tests/test_tile_walk_cases_cpu.py proves the same without a GPU, against walks stated by hand.
The comparisons and bars are test_gpu_parity's (compare_state: ring position and counts exact, waterfall / live / max-hold rtol 1e-4
atol 1e-6, the histogram through assert_hist_close); nothing here has a tolerance of its own."""
import functools
import types

import numpy as np
import pytest

import tile_walk_cases as tw
from oracle_lib import Oracle
from test_gpu_parity import amd, torch_cuda, compare_state	# noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _set_env(monkeypatch, env):
    for k in tw.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=1)
def _oracle_state(cid, form):
    """the oracle's state after the call (compare_state reads it; frozen)"""
    c = tw.CASES[cid]
    o = Oracle(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=c["wf_rows"])
    tw.oracle_call(o, c, form, tw.stream(cid)[1], nthreads=16)
    return types.SimpleNamespace(waterfall_pos=o.waterfall_pos, hitcount=o.hitcount, waterfall=o.waterfall, spectrum=o.spectrum,
                                 histogram=o.histogram)


# (the first decorator varies fastest: the two forms of a case follow each other and share tile_walk_cases.stream's one entry)
@pytest.mark.parametrize("form", tw.FORMS)
@pytest.mark.parametrize("cid", list(tw.CASES))
def test_units_that_take_several_tiles_vs_oracle(amd, torch_cuda, oracle_built, monkeypatch, cid, form):
    torch = torch_cuda
    c = tw.CASES[cid]
    n, total = 1 << c["log2n"], tw.total(c)
    n_batches, batch = tw.call_shape(c, form)
    what = "%s (%s), %d x %d spectra" % (cid, c["kernel"], n_batches, batch)
    _set_env(monkeypatch, c["env"])
    f = amd.Fosphor(fft_len_log=c["log2n"], n_bins=c["n_bins"], wf_rows=c["wf_rows"], max_spectra=total, max_batches=n_batches,
                    iq_format=c["fmt"])
    x, _ = tw.stream(cid)
    keep = torch.tensor(x).cuda()
    torch.cuda.synchronize()
    d = keep[(2 if c["fmt"] == "sc16" else 1) * c["offset"]:]
    assert d.data_ptr() % 16 == tw.iq_align(c), what

    # the walk this launch will take, from the function it takes it from
    n_cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    p = amd.plan_k1(c["log2n"], c["n_bins"], c["fmt"], tw.hop(c), d.data_ptr() % 16, total, batch,
                    tile_knob=int(c["env"].get("FOSPHOR_AMD_TILE", 0)), k1_knob=int(c["env"].get("FOSPHOR_AMD_K1", 1)), n_cus=n_cus)
    print("%s on %d CUs: %s" % (what, n_cus, p))
    assert p["kernel"] == c["kernel"], what
    assert p["max_tiles"] >= 2 and p["min_tiles"] < p["max_tiles"], "%s: no unit takes a second tile, or all take as many: %s" % (what, p)
    assert p["tiles"] * p["tile"] == total, what
    assert amd.load().fosphor_amd_plan_piece_batches(c["log2n"], 1, n_batches, batch, tw.sub_samples(c["log2n"])) == n_batches, what
    # the rows of the walk's last pass (the highest-numbered tiles) are rows of the ring when the call is over
    last_pass = (p["tiles"] - (p["max_tiles"] - 1) * p["units"]) * p["tile"]
    assert 0 < last_pass <= c["wf_rows"] <= total, what

    assert f.finish() >= 0			# an N = 8192 launch that finds the chip idle takes the full-chip form (what the hook describes)
    if c["overlap"] > 1:
        assert f.process_device_overlap(d, n_batches, batch, c["overlap"]) == 0, what
    else:
        assert f.process_device(d, n_batches, batch) == 0, what
    assert f.finish() >= 0
    assert f.waterfall_pos == total % c["wf_rows"], what		# ... with the last wf_rows spectra of the call in it
    hc = f.hitcount
    assert int(hc.sum(dtype=np.uint64)) == batch * n, what + ": the counts do not add up to the (last) batch"
    compare_state(f, _oracle_state(cid, form), what)
    f.close()
