"""Detection (include/fosphor_amd_detect.h), the parts that need no GPU: the header against its Python mirrors, the host statement
of the band rules against the numpy model (tests/detect_model.py), the bin table, and the compiled kernels' resources."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import detect_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fosphor_amd_detect.h")
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_detect.hip")


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


def bands_host(amd, y, thr, max_gap, min_cols, max_bands):
    """fosphor_amd_detect_bands_host -> (return value, n_found, structured array with guard entries behind max_bands)"""
    L = amd.load()
    y = np.ascontiguousarray(y, dtype=np.float32)
    out = np.zeros(max(max_bands, 0) + 2, dm.BAND_DTYPE)
    out["first"] = -77
    n_found = C.c_int(-5)
    rv = L.fosphor_amd_detect_bands_host(y.ctypes.data, y.size, thr, max_gap, min_cols, out.ctypes.data, max_bands, C.byref(n_found))
    return rv, n_found.value, out


def test_header_constants_match_python(amd):
    text = open(HEADER).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(FOSPHOR_AMD_\w+)\s+(-?\d+)", text)}
    F = amd.Fosphor
    assert F.TRACES == {"live": defs["FOSPHOR_AMD_TRACE_LIVE"], "maxhold": defs["FOSPHOR_AMD_TRACE_MAXHOLD"]} == {"live": 0, "maxhold": 1}
    assert F.FLOOR_MODES == {"absolute": defs["FOSPHOR_AMD_FLOOR_ABSOLUTE"], "percentile": defs["FOSPHOR_AMD_FLOOR_PERCENTILE"]}
    assert F.FLOOR_MODES == {"absolute": 0, "percentile": 1}
    assert F.DETECT_MAX_Q == defs["FOSPHOR_AMD_DETECT_MAX_Q"] == 4
    assert F.DETECT_LANES == defs["FOSPHOR_AMD_DETECT_LANES"] == 1024
    assert defs["FOSPHOR_AMD_DETECT_MAX_BANDS"] == 65536
    m = re.search(r"enum\s*\{([^}]*FOSPHOR_AMD_DETECT_STATS[^}]*)\}", text)
    names = [s.strip() for s in m.group(1).split(",") if s.strip()]
    assert names == ["FOSPHOR_AMD_DETECT_" + k.upper() for k in F.DETECT_STATS] + ["FOSPHOR_AMD_DETECT_STATS"]
    lib = amd._lib
    assert [n for n, _ in lib.DetectCfg._fields_] == re.findall(r"^\s+(?:int|float)\s+(\w+);", text.split("struct fosphor_amd_detect_cfg")[1].split("};")[0], re.M)
    assert [n for n, _ in lib.DetectResult._fields_] == ["n_found", "n_written", "floor_bin", "floor_y", "threshold_y"]
    assert C.sizeof(lib.DetectCfg) == 36 and C.sizeof(lib.DetectResult) == 20
    assert C.sizeof(lib.Band) == F.BAND_DTYPE.itemsize == dm.BAND_DTYPE.itemsize == 20
    assert F.BAND_DTYPE == dm.BAND_DTYPE and [n for n, _ in lib.Band._fields_] == list(dm.BAND_DTYPE.names)


@pytest.mark.parametrize("n_bins,scale,offset", [(128, 16.0, 1.5), (512, 51.2, 3.3), (256, 25.6 / 3.0, -0.7), (16, 1.6, 0.0)])
def test_bin_y_table(amd, n_bins, scale, offset):
    out = np.full(n_bins + 1, -9.0, np.float32)
    assert amd.load().fosphor_amd_detect_bin_y(n_bins, scale, offset, out.ctypes.data) == 0
    assert np.array_equal(out[:n_bins].view(np.uint32), dm.bin_y(n_bins, scale, offset).view(np.uint32))
    assert out[n_bins] == -9.0
    assert amd.load().fosphor_amd_detect_bin_y(n_bins, scale, offset, None) == -errno.EINVAL
    assert amd.load().fosphor_amd_detect_bin_y(0, scale, offset, out.ctypes.data) == -errno.EINVAL


@pytest.mark.parametrize("case", dm.band_cases(), ids=lambda c: c[0])
def test_band_rules_fixed_cases(amd, case):
    name, y, thr, max_gap, min_cols, max_bands, n_found, expect = case
    want_found, want = dm.bands(y, thr, max_gap, min_cols, max_bands)
    assert want_found == n_found, "the model against the hand-made expectation"
    assert [(int(b["first"]), int(b["last"]), int(b["peak_col"])) for b in want] == expect
    rv, found, out = bands_host(amd, y, thr, max_gap, min_cols, max_bands)
    assert rv == len(expect) and found == n_found
    dm.assert_bands_equal(out[:rv], want, tag=name)
    assert np.all(out["first"][rv:] == -77), "entries behind the written ones are untouched"


def test_band_rules_random_cases(amd):
    rng = np.random.default_rng(2024)
    worst, total = 0.0, 0
    for it in range(200):
        n = 257
        max_gap, min_cols = int(rng.integers(0, 4)), int(rng.integers(1, 5))
        density = rng.choice([0.1, 0.5, 0.9])
        y = (rng.standard_normal(n) * 0.5 + np.where(rng.random(n) < density, 1.0, -1.0)).astype(np.float32)
        y[rng.integers(0, n, 6)] = np.nan
        y[rng.integers(0, n, 8)] = np.float32(1.25)			# ties among the maxima
        max_bands = int(rng.choice([3, 300]))
        want_found, want = dm.bands(y, 0.0, max_gap, min_cols, max_bands)
        rv, found, out = bands_host(amd, y, 0.0, max_gap, min_cols, max_bands)
        assert (rv, found) == (len(want), want_found), it
        worst = max(worst, dm.assert_bands_equal(out[:rv], want, tag="random %d" % it))
        total += want_found
    print("random band cases: %d bands, worst |power_y error| %.3g" % (total, worst))
    assert total > 2000							# the cases are not empty


def test_bands_host_argument_errors(amd):
    y = np.ones(4, np.float32)
    for args in [(0, 1, 4), (-1, 1, 4), (2, 0, 4), (2, 1, 0)]:
        rv, found, out = bands_host(amd, y, 0.0, *args)
        assert (rv == -errno.EINVAL) == (args != (0, 1, 4)), args
        if rv < 0:
            assert found == -5 and np.all(out["first"] == -77)
    L = amd.load()
    out, nf = np.zeros(4, dm.BAND_DTYPE), C.c_int()
    assert L.fosphor_amd_detect_bands_host(None, 4, 0.0, 0, 1, out.ctypes.data, 4, C.byref(nf)) == -errno.EINVAL
    assert L.fosphor_amd_detect_bands_host(y.ctypes.data, 0, 0.0, 0, 1, out.ctypes.data, 4, C.byref(nf)) == -errno.EINVAL
    assert L.fosphor_amd_detect_bands_host(y.ctypes.data, 4, 0.0, 0, 1, None, 4, C.byref(nf)) == -errno.EINVAL
    assert L.fosphor_amd_detect_bands_host(y.ctypes.data, 4, 0.0, 0, 1, out.ctypes.data, 4, None) == -errno.EINVAL


def test_device_entries_refuse_null_without_a_device(amd):
    L = amd.load()
    q = (C.c_float * 1)(0.5)
    assert L.fosphor_amd_percentiles(None, q, 1, 1, 1) == -errno.EINVAL
    assert L.fosphor_amd_detect(None, C.byref(amd._lib.DetectCfg()), 1, 1, 1) == -errno.EINVAL
    assert L.fosphor_amd_detect_stats(None, None) == -errno.EINVAL


def test_model_percentiles_by_hand():
    """the model against columns worked out by hand: N = 4, 4 bins; memory columns 0 .. 3 come out at 2, 3, 0, 1"""
    h = np.array([[0, 4, 0, 1],
                  [0, 0, 0, 1],
                  [0, 0, 0, 1],
                  [0, 0, 7, 1]], np.float32)
    b = dm.percentile_bins(h, [0.25, 0.5, 1.0])
    assert b.tolist() == [[3, 0, -1, 0], [3, 1, -1, 0], [3, 3, -1, 0]]		# c_b == q * T exactly at 0.25 and 0.5: the >= rule
    t = dm.bin_y(4, 2.0, 1.0)
    assert t.tolist() == [-1.0, -0.5, 0.0, 0.5]
    y = dm.percentile_y(b, t)
    assert np.isnan(y[:, 2]).all() and y[0].tolist()[:2] == [0.5, -1.0]
    assert dm.floor_bin(np.array([5, -1, 3, 9, -1, 7])) == 5 and dm.floor_bin(np.array([5, 3, 9])) == 5		# lower median, even / odd
    assert dm.floor_bin(np.array([-1, -1])) == -1


def test_detect_kernels_do_not_spill():
    """-Rpass-analysis=kernel-resource-usage: every kernel of fosphor_detect.hip has 0 bytes of scratch and at most 128 VGPRs"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-x", "hip", "--cuda-device-only",
                        "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        for key in ("ScratchSize", "VGPRs"):
            m = re.search(r"remark:\s+%s( \[bytes/lane\])?: (\d+)" % key, line)
            if m and cur:
                found.setdefault(cur, {})[key] = int(m.group(2))
    ours = {k: v for k, v in found.items() if re.search(r"k_percentiles|k_floor|k_bands", k)}
    assert len(ours) == 6 and sum("k_percentiles" in k for k in ours) == 4, sorted(found)
    for name, res in ours.items():
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 0) <= 128, (name, res)
