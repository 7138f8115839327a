"""fosphor_amd_plan_k1 without a GPU: every case of tests/tile_walk_cases.py makes its kernel walk several tiles per wave or
work-group, in both forms tests/test_gpu_tile_walk.py runs it in -- proven through the one host function the library's tile choice,
kernel choice and grid sizes come from, against walks stated by hand in the case table and against a restatement of the launch rules
as they stood before the hook.  None of the expectations comes from the function under test."""
import ctypes as C
import errno
import itertools

import pytest

import tile_walk_cases as tw
from test_boundary_cpu import amd		# noqa: F401  (the fixture: builds the library when it is missing)


def _hook(amd, c, form, n_cus):
    n_batches, batch = tw.call_shape(c, form)
    return amd.plan_k1(c["log2n"], c["n_bins"], c["fmt"], tw.hop(c), tw.iq_align(c), n_batches * batch, batch,
                       tile_knob=int(c["env"].get("FOSPHOR_AMD_TILE", 0)), k1_knob=int(c["env"].get("FOSPHOR_AMD_K1", 1)), n_cus=n_cus)


def _cus(cid):
    return [256, tw.WIDE_OTHER_CUS] if tw.CASES[cid]["log2n"] == 13 else [256]


@pytest.mark.parametrize("form", tw.FORMS)
@pytest.mark.parametrize("cid,n_cus", [(cid, n) for cid in tw.CASES for n in _cus(cid)])
def test_every_case_strides_as_stated(amd, cid, n_cus, form):
    """The named kernel runs; some unit takes the stated maximum of tiles (at least 2) and some unit fewer, so the
    `tile + stride < ntiles` guard of the prefetch is taken both ways; the call is one piece."""
    c = tw.CASES[cid]
    want = tw.walk_on(c, n_cus)
    p = _hook(amd, c, form, n_cus)
    assert p["kernel"] == c["kernel"], (cid, form, p)
    for k in ("tile", "tiles", "units", "max_tiles", "min_tiles"):
        assert p[k] == want[k], (cid, form, k, p)
    assert p["max_tiles"] >= 2 and p["min_tiles"] < p["max_tiles"], (cid, form, p)
    # unit u takes tiles u, u + units, ...: the units that take the maximum, counted
    assert sum(1 for u in range(p["units"]) if len(range(u, p["tiles"], p["units"])) == p["max_tiles"]) == want["n_most"]
    assert p["tiles"] * p["tile"] == tw.total(c)
    n_batches, batch = tw.call_shape(c, form)
    streams = 1
    assert amd.load().fosphor_amd_plan_piece_batches(c["log2n"], streams, n_batches, batch, tw.sub_samples(c["log2n"])) == n_batches
    assert n_batches * batch << c["log2n"] <= tw.sub_samples(c["log2n"])


def test_case_table_is_well_formed():
    for cid, c in tw.CASES.items():
        assert c["batch"] <= 1088 and c["batch"] % 16 == 0, cid		# the 16-bit count hand-off; every entry point's multiple
        assert set(c["env"]) <= set(tw.KNOBS) and "FOSPHOR_AMD_K1_BLOCKS" not in c["env"], cid
        assert c["wf_rows"] & (c["wf_rows"] - 1) == 0, cid
        for n_cus in _cus(cid):
            # the ring still holds every row of the walk's last pass when the call is over
            assert tw.last_pass_spectra(tw.walk_on(c, n_cus)) <= c["wf_rows"], cid
        assert tw.n_samples(c) <= 34 << 20, cid				# a second or two of oracle per case
    assert {c["kernel"] for c in tw.CASES.values()} == {"k1_fft_bin", "k1v2_fft_bin", "k1big_fft_bin", "k1w_fft_bin"}
    # both ways into the two-wave kernel, the three-pass walk, the default tile rule, both forms of the N = 8192 kernel
    assert tw.CASES["v2_oddhop"]["overlap"] == 1024 and tw.iq_align(tw.CASES["v2_sc16_unaligned"]) == 4
    assert tw.CASES["w_sc16_128_x3"]["walk"]["max_tiles"] == 3 and not tw.CASES["w_default"]["env"]
    assert tw.CASES["wide_ov2"]["overlap"] == 2 and tw.CASES["wide_sc16_ov1"]["overlap"] == 1


def test_a_case_that_does_not_stride_is_caught(amd):
    """The check above bites: the same cases with one batch fewer or a longer tile fit the grid, and the hook says so."""
    c = dict(tw.CASES["w_fp32_256"], n_batches=8)		# 1856 tiles of 4 for 2048 waves
    p = _hook(amd, c, "batches", 256)
    assert (p["tiles"], p["units"], p["max_tiles"], p["min_tiles"]) == (1856, 1856, 1, 1)
    c = dict(tw.CASES["w_default"], n_batches=48, batch=688)	# 16 x 43: tile 16 as tabled, but tile 32 as one batch of 33024
    assert _hook(amd, c, "batches", 256)["max_tiles"] == 2 and _hook(amd, c, "one_batch", 256)["max_tiles"] == 1
    c = dict(tw.CASES["wide_ov2"], n_batches=1)
    assert _hook(amd, c, "batches", 256)["max_tiles"] == 1
    assert _hook(amd, tw.CASES["wide_ov2"], "batches", 304)["max_tiles"] == 1		# 272 tiles on a 304-CU device


def _plan(amd, **s):
    return amd.plan_k1(s["log2n"], s["n_bins"], s["fmt"], s["hop"], s["align"], s["total"], s["batch"], tile_knob=s["tile_knob"],
                       k1_knob=s["k1_knob"], n_cus=s["n_cus"])


def test_bench_shapes_keep_their_launches(amd):
    """The launches bench.py times: kernel, tile and grid as before the hook (printed: pytest -s shows both)."""
    want = {"C2": dict(kernel="k1_fft_bin", tile=64, tiles=1024, units=1024, max_tiles=1, min_tiles=1),
            "C3": dict(kernel="k1w_fft_bin", tile=64, tiles=1792, units=256, max_tiles=7, min_tiles=7),
            "C5": dict(kernel="k1h_fused", tile=32, tiles=32, units=32, max_tiles=0, min_tiles=0)}
    for name, s in tw.BENCH_SHAPES.items():
        p = _plan(amd, **s)
        print("%s: rules before the hook %s\n%s: fosphor_amd_plan_k1    %s" % (name, tw.expected_plan(**s), name, p))
        assert p == tw.expected_plan(**s) == want[name], name


def test_hook_equals_the_launch_rules_it_replaced(amd):
    """A sweep over geometry, format, hop, alignment, knobs, device size and call shape: the hook returns what pick_tile, fill_k1 and
    launch_k1_as computed, each on its own, before they shared one function."""
    calls = [(1, 16), (1, 64), (3, 48), (2, 1088), (7, 1008), (10, 928), (16, 1056), (35, 944), (48, 688), (64, 1024), (17, 1008),
             (1, 4096), (28, 4096), (1, 9280), (1, 33040), (4, 8192), (1, 65536), (33, 1024)]
    n = 0
    for log2n, n_bins, tile_knob, n_cus, (nb, batch) in itertools.product((10, 13, 16), (48, 128, 256, 272, 512),
                                                                         (0, 4, 8, 16, 32, 64, 128, 3, 256), (0, 128, 256, 304), calls):
        for fmt in ("fp32", "sc16", "fp16") if log2n == 16 else ("fp32", "sc16"):
            for overlap, align, k1_knob in ((1, 0, 1), (2, 8, 1), (1 << log2n, 0, 1), (1, 4, 1), (1, 12, 2)):
                s = dict(log2n=log2n, n_bins=n_bins, fmt=fmt, hop=(1 << log2n) // overlap, align=align, tile_knob=tile_knob,
                         k1_knob=k1_knob, n_cus=n_cus, total=nb * batch, batch=batch)
                assert _plan(amd, **s) == tw.expected_plan(**s), s
                n += 1
    assert n > 10000


def test_hook_refuses_nonsense(amd):
    from gr_fosphor_amd._lib import K1Plan
    f, p = amd.load().fosphor_amd_plan_k1, K1Plan()
    good = [10, 256, 0, 1024, 0, 0, 1, 256, 1024, 64]
    assert f(*good, C.byref(p)) == 0 and f(*good, None) == -errno.EINVAL
    for i, v in ((0, 11), (0, 0), (1, 0), (1, 1024), (2, 3), (2, 1), (3, 0), (4, -1), (7, -1), (8, 32), (8, 1000), (9, 0), (9, 6)):
        bad = list(good)
        bad[i] = v
        assert f(*bad, C.byref(p)) == -errno.EINVAL, (i, v)
    assert f(13, 512, 0, 8192, 0, 0, 1, 256, 1032, 1032, C.byref(p)) == -errno.EINVAL	# N = 8192: batches of whole 16s
    with pytest.raises(ValueError):
        amd.plan_k1(10, 256, "fp32", 1024, 0, 1000, 64)
