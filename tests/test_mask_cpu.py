"""The frequency mask (include/fosphor_amd_mask.h), the parts that need no GPU: the header against its Python mirrors, the host
statement of the row rule and the limit line through points against the numpy model (tests/mask_model.py), and the compiled
kernels' resources."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import mask_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fosphor_amd_mask.h")
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_mask.hip")


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


def row_host(amd, y, upper, lower):
    """fosphor_amd_mask_row_host -> (return value, record)"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    up = None if upper is None else np.ascontiguousarray(upper, dtype=np.float32)
    lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float32)
    out = np.zeros(2, mm.ROW_DTYPE)
    out["n_over"] = -77
    rv = amd.load().fosphor_amd_mask_row_host(y.ctypes.data, None if up is None else up.ctypes.data,
                                              None if lo is None else lo.ctypes.data, y.size,
                                              C.cast(out.ctypes.data, C.POINTER(amd._lib.MaskRow)))
    assert out["n_over"][1] == -77, "the entry behind the record is untouched"
    return rv, out[:1]


def test_header_matches_python(amd):
    text = open(HEADER).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(FOSPHOR_AMD_\w+)\s+(-?\d+)", text)}
    F, lib = amd.Fosphor, amd._lib
    assert F.MASK_MAX_EVENTS == defs["FOSPHOR_AMD_MASK_MAX_EVENTS"] == 65536
    assert F.MASK_STRIP == defs["FOSPHOR_AMD_MASK_STRIP"] == 1024
    assert defs["FOSPHOR_AMD_MASK_MAX_SPREAD"] == 1024
    assert F.MASK_MAX_CHANNELS == 8 and re.search(r"#define\s+FOSPHOR_MAX_CHANNELS\s+8", open(os.path.join(ROOT, "include", "fosphor.h")).read())
    m = re.search(r"enum\s*\{([^}]*FOSPHOR_AMD_MASK_STATS[^}]*)\}", text)
    names = [s.strip() for s in m.group(1).split(",") if s.strip()]
    assert names == ["FOSPHOR_AMD_MASK_" + k.upper() for k in F.MASK_STATS] + ["FOSPHOR_AMD_MASK_STATS"]

    def fields(struct):
        body = re.split(r"struct %s\b[^{;()]*\{" % struct, text)[1].split("};")[0]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                out += [re.sub(r"\[.*\]", "", w.strip().split()[-1]) for w in decl.split(",")]
        return out
    assert [n for n, _ in lib.MaskChannel._fields_] == fields("fosphor_amd_mask_channel") == list(mm.CHANNEL_DTYPE.names)
    assert [n for n, _ in lib.MaskCfg._fields_] == fields("fosphor_amd_mask_cfg") == list(mm.CFG_DTYPE.names)
    assert [n for n, _ in lib.MaskRow._fields_] == fields("fosphor_amd_mask_row") == list(mm.ROW_DTYPE.names)
    assert [n for n, _ in lib.MaskResult._fields_] == fields("fosphor_amd_mask_result") == list(mm.RESULT_DTYPE.names)
    assert C.sizeof(lib.MaskChannel) == mm.CHANNEL_DTYPE.itemsize == 8
    assert C.sizeof(lib.MaskCfg) == mm.CFG_DTYPE.itemsize == 84
    assert C.sizeof(lib.MaskRow) == mm.ROW_DTYPE.itemsize == F.MASK_ROW_DTYPE.itemsize == 24 and F.MASK_ROW_DTYPE == mm.ROW_DTYPE
    assert C.sizeof(lib.MaskResult) == mm.RESULT_DTYPE.itemsize == 16


@pytest.mark.parametrize("case", mm.row_cases(), ids=lambda c: c[0])
def test_row_rule_fixed_cases(amd, case):
    name, y, upper, lower, expect = case
    want = mm.row_rule(y, upper, lower)
    got_model = tuple(want[k].item() for k in mm.ROW_DTYPE.names)
    assert got_model[:5] == expect[:5], "the model against the hand-made expectation"
    assert got_model[5] == expect[5] or (np.isnan(got_model[5]) and np.isnan(expect[5]))
    rv, out = row_host(amd, y, upper, lower)
    assert rv == 0
    mm.assert_rows_equal(out, want.reshape(1), tag=name)


def random_row(rng, n):
    """a row and its limits with NaN, +-inf and cells equal to a limit"""
    y = rng.standard_normal(n).astype(np.float32)
    up = (0.8 + 0.3 * rng.standard_normal(n)).astype(np.float32)
    lo = (-0.8 + 0.3 * rng.standard_normal(n)).astype(np.float32)
    for a in (y, up, lo):
        k = rng.integers(0, n, 4)
        a[k[0]], a[k[1]], a[k[2]] = np.nan, np.inf, -np.inf
    eq = rng.integers(0, n, 6)
    y[eq[:3]] = up[eq[:3]]						# equality violates neither side
    y[eq[3:]] = lo[eq[3:]]
    q = rng.integers(0, n, 4)						# tied excesses: exact in float32
    y[q], up[q] = np.float32(2.5), np.float32(1.25)
    return y, up, lo


def test_row_rule_random_rows(amd):
    rng = np.random.default_rng(1234)
    seen_over = seen_under = seen_inf = 0
    for it in range(3000):
        n = int(rng.choice([1, 2, 3, 5, 64, 257]))
        y, up, lo = random_row(rng, n)
        mode = it % 4
        upper, lower = (up if mode != 1 else None), (lo if mode != 0 else None)
        if mode == 3:
            upper = lower = None
        want = mm.row_rule(y, upper, lower)
        rv, out = row_host(amd, y, upper, lower)
        assert rv == 0
        mm.assert_rows_equal(out, want.reshape(1), tag="random %d" % it)
        seen_over += int(want["n_over"] > 0)
        seen_under += int(want["n_under"] > 0)
        seen_inf += int(np.isinf(want["peak_over"]))
    assert seen_over > 800 and seen_under > 800 and seen_inf > 50		# the cases are not empty


def test_row_host_argument_errors(amd):
    L = amd.load()
    y = np.ones(4, np.float32)
    out = amd._lib.MaskRow()
    assert L.fosphor_amd_mask_row_host(None, y.ctypes.data, y.ctypes.data, 4, C.byref(out)) == -errno.EINVAL
    assert L.fosphor_amd_mask_row_host(y.ctypes.data, y.ctypes.data, y.ctypes.data, 0, C.byref(out)) == -errno.EINVAL
    assert L.fosphor_amd_mask_row_host(y.ctypes.data, y.ctypes.data, y.ctypes.data, 4, None) == -errno.EINVAL


def points_host(amd, n, col, y, n_pts=None):
    col = np.ascontiguousarray(col, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float32)
    out = np.full(max(n, 0) + 1, -9.0, np.float32)
    rv = amd.load().fosphor_amd_mask_from_points(n, col.ctypes.data, y.ctypes.data, col.size if n_pts is None else n_pts, out.ctypes.data)
    assert out[-1] == -9.0
    return rv, out[:-1]


@pytest.mark.parametrize("name,n,col,y", [
    ("a single point", 16, [5.0], [1.5]),
    ("two points inside", 64, [10.0, 50.0], [0.0, 2.0]),
    ("points outside 0 .. n-1", 32, [-7.5, 12.25, 100.0], [3.0, -1.0, 0.7]),
    ("every point left of the buffer", 8, [-9.0, -2.0], [1.0, 2.0]),
    ("every point right of the buffer", 8, [8.0, 20.0], [1.0, 2.0]),
    ("fractional columns, thirds", 1024, [0.0, 100.0 / 3.0, 511.7, 512.0, 1023.0], [0.1, 1.0 / 3.0, 2.7, -0.3, 0.9]),
    ("a step of one column", 16, [3.0, 4.0, 9.0], [0.0, 5.0, 5.0]),
    ("infinite y", 16, [2.0, 6.0, 10.0], [0.0, np.inf, 1.0]),
])
def test_from_points_bit_for_bit(amd, name, n, col, y):
    want = mm.from_points(n, col, y)
    rv, out = points_host(amd, n, col, y)
    assert rv == 0
    assert mm.same_bits(out, want), name
    f32 = np.asarray(y, np.float32)
    assert out[0] == f32[0] or col[0] < 0 or np.isnan(out[0])


def test_from_points_random_bit_for_bit(amd):
    rng = np.random.default_rng(77)
    for it in range(50):
        n = int(rng.choice([7, 100, 1024]))
        k = int(rng.integers(1, 9))
        col = np.sort(rng.uniform(-0.2 * n, 1.2 * n, k))
        if np.any(np.diff(col) <= 0):
            continue
        y = rng.uniform(-3, 3, k).astype(np.float32)
        rv, out = points_host(amd, n, col, y)
        assert rv == 0 and mm.same_bits(out, mm.from_points(n, col, y)), it


def test_from_points_argument_errors(amd):
    L = amd.load()
    col, y = np.array([1.0, 2.0]), np.array([0.0, 1.0], np.float32)
    out = np.full(8, -9.0, np.float32)
    for n, c, yy, k, o in [(0, col, y, 2, out), (-1, col, y, 2, out), (8, col, y, 0, out), (8, col, y, -1, out),
                           (8, None, y, 2, out), (8, col, None, 2, out), (8, col, y, 2, None),
                           (8, np.array([2.0, 1.0]), y, 2, out), (8, np.array([1.0, 1.0]), y, 2, out),
                           (8, np.array([1.0, np.nan]), y, 2, out), (8, np.array([np.nan]), y, 1, out)]:
        rv = L.fosphor_amd_mask_from_points(n, None if c is None else c.ctypes.data, None if yy is None else yy.ctypes.data, k,
                                            None if o is None else o.ctypes.data)
        assert rv == -errno.EINVAL, (n, c, k)
        assert np.all(out == -9.0)
    assert L.fosphor_amd_mask_from_points(8, col.ctypes.data, y.ctypes.data, 2, out.ctypes.data) == 0


def test_device_entries_refuse_null_without_a_device(amd):
    L = amd.load()
    assert L.fosphor_amd_mask_scan(None, C.byref(amd._lib.MaskCfg()), 1, 1, 1, 1, 1, 1, None) == -errno.EINVAL
    assert L.fosphor_amd_mask_from_trace(None, 0, 0.0, 0, 1) == -errno.EINVAL
    assert L.fosphor_amd_mask_stats(None, None) == -errno.EINVAL


def test_model_by_hand():
    """the model's ring order, event list, channel power and trace line against values worked out by hand"""
    wf = np.arange(16, dtype=np.float32).reshape(4, 4)			# ring rows 0 .. 3, memory columns 0 .. 3
    ys = mm.newest_first(wf, 1)						# pos 1: the newest row is ring row 0, then 3, 2, 1
    assert ys[:, 0].tolist() == [2.0, 14.0, 10.0, 6.0]			# shifted column 0 is memory column 2
    rows = mm.rows_rule(ys, np.full(4, 9.5, np.float32), None, 1, 2)	# window: shifted columns 1, 2 = memory 3, 0
    assert rows["n_over"].tolist() == [0, 2, 1, 0] and rows["first_col"].tolist() == [-1, 1, 1, -1]
    assert rows["peak_col"].tolist() == [-1, 1, 1, -1] and rows["peak_over"][1] == 5.5
    res, ev = mm.events(rows, 1, 1)
    assert (int(res["n_triggered"]), int(res["n_written"]), int(res["newest"]), int(res["oldest"])) == (2, 1, 1, 2) and ev.tolist() == [1]
    res, ev = mm.events(rows, 3, 8)
    assert (int(res["n_triggered"]), int(res["newest"]), int(res["oldest"])) == (0, -1, -1) and ev.size == 0
    p = mm.channel_power(np.array([[0.0, 0.5, -np.inf, np.nan], [-np.inf, -np.inf, np.nan, 1.0]], np.float32), [(0, 1), (0, 2), (3, 3)])
    assert np.allclose(p[0], [0.5 * np.log10(11.0), -np.inf]) and np.isneginf(p[1, 1]) and np.isneginf(p[2, 0]) and p[2, 1] == 1.0
    t = mm.from_trace(np.array([1, np.nan, np.nan, np.nan, 5, 2], np.float32), 0.5, 1)
    assert t[0] == 1.5 and t[1] == 1.5 and np.isnan(t[2]) and t[3] == 5.5 and t[5] == 5.5
    assert mm.from_points(4, [1.0, 3.0], [0.0, 1.0]).tolist() == [0.0, 0.0, 0.5, 1.0]


def test_mask_kernels_do_not_spill():
    """-Rpass-analysis=kernel-resource-usage: every kernel of fosphor_mask.hip has 0 bytes of scratch and at most 128 VGPRs"""
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
    ours = {k: v for k, v in found.items() if re.search(r"k_mask_(scan|combine|events|trace)", k)}
    assert len(ours) == 4, sorted(found)
    for name, res in ours.items():
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 0) <= 128, (name, res)
