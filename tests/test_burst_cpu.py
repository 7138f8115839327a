"""Bursts in time and frequency (include/fosphor_amd_burst.h), the parts that need no GPU: the run-based model against a pixel flood
fill that shares no code with it (tests/burst_model.py), the library's host function against the model, its -EINVAL table and its
two overflows, the header against its Python mirrors, and the compiled kernels' resources."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import burst_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fosphor_amd_burst.h")
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_burst.hip")
EINVAL = -errno.EINVAL


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


def random_field(rows, n, density, seed):
    """ys uniform in [0, 1) against a threshold that leaves `density` of the cells on; a sprinkle of NaN and +-inf cells, of cells
    equal to the threshold and of tied peaks; a NaN threshold column (never on) and a +inf one"""
    rng = np.random.default_rng(seed)
    ys = rng.random((rows, n)).astype(np.float32)
    thr = np.full(n, 1.0 - density, np.float32)
    thr[rng.integers(0, n, 3)] += np.float32(0.05)
    k = rng.integers(0, rows * n, 24)
    flat = ys.reshape(-1)
    flat[k[0:4]], flat[k[4:8]], flat[k[8:12]] = np.nan, np.inf, -np.inf
    flat[k[12:16]] = thr[k[12:16] % n]					# equality is not on
    flat[k[16:24]] = np.float32(0.96875)					# ties of the peak, exact in float32
    thr[int(rng.integers(1, n - 1))] = np.nan
    thr[int(rng.integers(1, n - 1))] = np.inf
    return ys, thr


FIELDS = [(d, gc, gr) for d in (0.3, 0.5, 0.6) for gc in (0, 1, 3) for gr in (0, 1, 2)]


def host(amd, ys, thr, first_bin=0, max_gap_cols=0, max_gap_rows=0, min_rows=1, min_cols=1, max_bursts=65536, max_runs=1 << 20,
         threshold_y=0.0, cfg_rows=None, cfg_cols=None, null=()):
    """fosphor_amd_bursts_host -> (return value, result dict, written records, everything behind them)"""
    ys = np.ascontiguousarray(ys, dtype=np.float32)
    rows, n = ys.shape
    t = None if thr is None else np.ascontiguousarray(thr, dtype=np.float32)
    cfg = amd._lib.BurstCfg(first_bin, n if cfg_cols is None else cfg_cols, rows if cfg_rows is None else cfg_rows, threshold_y,
                            max_gap_cols, max_gap_rows, min_rows, min_cols, max_runs)
    res = amd._lib.BurstResult(-7, -7, -7, -7, -7)
    out = np.zeros(min(max(max_bursts, 1), 70000) + 2, bm.BURST_DTYPE)
    out["n_cells"] = -77
    rv = amd.load().fosphor_amd_bursts_host(None if "ys" in null else ys.ctypes.data, rows, n, None if t is None else t.ctypes.data,
                                            None if "cfg" in null else C.byref(cfg), None if "res" in null else C.byref(res),
                                            None if "out" in null else out.ctypes.data, max_bursts)
    r = {k: getattr(res, k) for k in bm.RESULT_NAMES}
    nw = r["n_written"] if rv == 0 else 0
    assert np.all(out["n_cells"][nw:] == -77), "entries behind n_written are not written"
    return rv, r, out[:nw]


@pytest.mark.parametrize("density,gap_cols,gap_rows", FIELDS)
def test_model_against_flood_fill(density, gap_cols, gap_rows):
    """random 24 x 96 fields: the run-based statement and the pixel flood fill give identical components and identical records
    (energy_y too: both sum in fp64, in different orders, and round to float32 -- 1e-6 covers the last bit)"""
    ys, thr = random_field(24, 96, density, int(density * 100) + 10 * gap_cols + gap_rows)
    res, recs = bm.bursts(ys, thr, max_gap_cols=gap_cols, max_gap_rows=gap_rows)
    fres, frecs = bm.flood_bursts(ys, thr, max_gap_cols=gap_cols, max_gap_rows=gap_rows)
    bm.assert_result_equal(res, fres)
    bm.assert_bursts_equal(recs, frecs, 1e-6)
    assert res["n_components"] == len(recs) > 0 and res["n_runs"] >= res["n_components"]
    if density == 0.6 and gap_rows:
        assert recs["n_cells"].max() > 24 * 96 // 4, "above the percolation threshold a component spans the field"
    # with filters, an offset and a short output
    kw = dict(first_bin=5, max_gap_cols=gap_cols, max_gap_rows=gap_rows, min_rows=2, min_cols=3, max_bursts=4)
    res, recs = bm.bursts(ys, thr, **kw)
    fres, frecs = bm.flood_bursts(ys, thr, **kw)
    bm.assert_result_equal(res, fres)
    bm.assert_bursts_equal(recs, frecs, 1e-6)


@pytest.mark.parametrize("density,gap_cols,gap_rows", FIELDS)
def test_host_function_against_model(amd, density, gap_cols, gap_rows):
    """the same fields: integers, peak and flags exact, energy_y within 1e-6"""
    ys, thr = random_field(24, 96, density, int(density * 100) + 10 * gap_cols + gap_rows)
    for kw in (dict(), dict(first_bin=5, min_rows=2, min_cols=3, max_bursts=4), dict(min_rows=24), dict(min_cols=97)):
        kw = dict(kw, max_gap_cols=gap_cols, max_gap_rows=gap_rows)
        want_res, want = bm.bursts(ys, thr, **kw)
        rv, res, got = host(amd, ys, thr, **kw)
        assert rv == 0
        bm.assert_result_equal(res, want_res, kw)
        bm.assert_bursts_equal(got, want, 1e-6, kw)
    # a scalar threshold: thr NULL, cfg->threshold_y
    want_res, want = bm.bursts(ys, np.float32(0.7), max_gap_cols=gap_cols, max_gap_rows=gap_rows)
    rv, res, got = host(amd, ys, None, threshold_y=0.7, max_gap_cols=gap_cols, max_gap_rows=gap_rows)
    assert rv == 0
    bm.assert_result_equal(res, want_res)
    bm.assert_bursts_equal(got, want, 1e-6)


def test_model_by_hand(amd):
    """a field small enough to work out on paper, through both models and the host function"""
    N, I = np.nan, np.inf
    ys = np.array([[5, 0, 5, 0, 0, 5, 0, 0],		# j = 0: runs (0, 0) (2, 2) (5, 5); with max_gap_cols 1: (0, 2) (5, 5)
                   [0, 0, 7, 0, 0, 0, 0, 0],		# j = 1: (2, 2)
                   [0, 0, 0, 0, 0, 0, 0, 0],		# j = 2: nothing
                   [0, N, 7, -I, 9, 0, 0, 5]], np.float32)	# j = 3: (2, 2) (4, 4) (7, 7); with max_gap_cols 1: (2, 4) (7, 7)
    res, recs = bm.bursts(ys, 1.0)
    assert res == dict(n_runs=7, n_components=6, n_found=6, n_written=6, overflow=0)
    assert recs[["newest", "oldest", "first_col", "last_col", "n_cells"]].tolist() == \
        [(0, 0, 0, 0, 1), (0, 1, 2, 2, 2), (0, 0, 5, 5, 1), (3, 3, 2, 2, 1), (3, 3, 4, 4, 1), (3, 3, 7, 7, 1)]
    assert recs["flags"].tolist() == [bm.ON | bm.FIRST_COL, bm.ON, bm.ON, bm.CUT, bm.CUT, bm.CUT | bm.LAST_COL]
    assert (recs["peak_row"][1], recs["peak_col"][1], recs["peak_y"][1]) == (1, 2, 7.0)
    assert abs(recs["energy_y"][1] - 0.5 * np.log10(1e10 + 1e14)) < 1e-6
    # gaps of one column closed, rows two apart joined: (0, 2) of j = 0, (2, 2) of j = 1 and (2, 4) of j = 3 are one component
    res, recs = bm.bursts(ys, 1.0, max_gap_cols=1, max_gap_rows=1)
    assert res == dict(n_runs=5, n_components=3, n_found=3, n_written=3, overflow=0)
    assert recs[["newest", "oldest", "first_col", "last_col", "n_cells"]].tolist() == [(0, 3, 0, 4, 7), (0, 0, 5, 5, 1), (3, 3, 7, 7, 1)]
    assert (recs["peak_row"][0], recs["peak_col"][0], recs["peak_y"][0]) == (3, 4, 9.0)		# the closed -inf cell adds nothing
    assert abs(recs["energy_y"][0] - 0.5 * np.log10(2e10 + 1.0 + 2e14 + 1e18)) < 1e-6
    # a peak tie across rows goes to the smallest j, within a row to the smallest column
    ys2 = np.array([[0, 3, 3, 0], [0, 3, 4, 0], [0, 4, 4, 0]], np.float32)
    _, r2 = bm.bursts(ys2, 1.0)
    assert (r2["peak_row"][0], r2["peak_col"][0]) == (1, 2)
    for kw in (dict(), dict(max_gap_cols=1, max_gap_rows=1), dict(max_gap_cols=1, max_gap_rows=1, first_bin=100)):
        for field in (ys, ys2):
            want_res, want = bm.bursts(field, 1.0, **kw)
            fres, frecs = bm.flood_bursts(field, 1.0, **kw)
            bm.assert_result_equal(want_res, fres)
            bm.assert_bursts_equal(frecs, want, 1e-6)
            rv, res, got = host(amd, field, None, threshold_y=1.0, **kw)
            assert rv == 0
            bm.assert_result_equal(res, want_res)
            bm.assert_bursts_equal(got, want, 1e-6)


def test_host_overflows(amd):
    ys, thr = random_field(24, 96, 0.5, 3)
    full_res, full = bm.bursts(ys, thr)
    n_found, n_runs = full_res["n_found"], full_res["n_runs"]
    assert n_found > 8 and n_runs > n_found
    # max_bursts one below n_found: the first n_found - 1 in ascending root order, nothing behind them, no error
    rv, res, got = host(amd, ys, thr, max_bursts=n_found - 1)
    assert rv == 0 and (res["n_found"], res["n_written"], res["overflow"]) == (n_found, n_found - 1, 0)
    bm.assert_bursts_equal(got, full[:n_found - 1], 1e-6)
    assert np.all(np.diff(got["newest"]) >= 0)					# a root lies in its component's newest row
    # max_runs at n_runs is fine, one below overflows: n_runs exact, the other counts 0, out untouched
    rv, res, got = host(amd, ys, thr, max_runs=n_runs)
    assert rv == 0 and res == full_res
    rv, res, got = host(amd, ys, thr, max_runs=n_runs - 1)
    assert rv == 0 and res == dict(n_runs=n_runs, n_components=0, n_found=0, n_written=0, overflow=1) and got.size == 0
    assert bm.bursts(ys, thr, max_runs=n_runs - 1)[0] == res


def test_host_einval_table(amd):
    ys, thr = random_field(8, 32, 0.3, 4)
    good = dict(first_bin=3, max_gap_cols=1, max_gap_rows=7, min_rows=1, min_cols=1, max_bursts=65536, max_runs=1 << 20)
    bad = [dict(first_bin=-1), dict(first_bin=65536), dict(first_bin=65536 - 31),		# a window outside the buffer
           dict(cfg_rows=7), dict(cfg_rows=0), dict(cfg_cols=31), dict(cfg_cols=0),
           dict(max_gap_cols=-1), dict(max_gap_rows=-1), dict(max_gap_rows=8),
           dict(min_rows=0), dict(min_cols=0), dict(min_rows=-3),
           dict(max_runs=0), dict(max_runs=(1 << 20) + 1), dict(max_bursts=0), dict(max_bursts=65537), dict(max_bursts=-1),
           dict(null=("ys",)), dict(null=("cfg",)), dict(null=("res",)), dict(null=("out",))]
    for change in bad:
        rv, res, got = host(amd, ys, thr, **dict(good, **change))
        assert rv == EINVAL, change
        assert all(v == -7 for v in res.values()), change				# nothing is written
    rv, res, got = host(amd, ys, thr, **good)
    assert rv == 0 and res["n_found"] > 0
    rv, res, got = host(amd, ys, thr, **dict(good, first_bin=65536 - 32))		# the last window that fits
    assert rv == 0 and got["last_col"].max() <= 65535


def test_device_entries_refuse_null_without_a_device(amd):
    L = amd.load()
    assert L.fosphor_amd_bursts(None, C.byref(amd._lib.BurstCfg()), None, 1, 1, 1) == EINVAL
    assert L.fosphor_amd_burst_stats(None, None) == EINVAL


def test_header_matches_python(amd):
    text = open(HEADER).read()
    F, lib = amd.Fosphor, amd._lib
    assert re.search(r"#define\s+FOSPHOR_AMD_BURST_MAX_RUNS\s+\(1 << 20\)", text) and F.BURST_MAX_RUNS == 1 << 20
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(FOSPHOR_AMD_\w+)\s+(\d+)u?\b", text)}
    assert F.BURST_MAX_BURSTS == defs["FOSPHOR_AMD_BURST_MAX_BURSTS"] == 65536
    assert F.BURST_STRIP == defs["FOSPHOR_AMD_BURST_STRIP"] == 1024
    assert defs["FOSPHOR_AMD_BURST_MAX_ROWS"] == 65536 and defs["FOSPHOR_AMD_BURST_MAX_GAP_ROWS"] == 7
    assert F.BURST_FLAGS == {"on": defs["FOSPHOR_AMD_BURST_ON"], "cut": defs["FOSPHOR_AMD_BURST_CUT"],
                             "first_col": defs["FOSPHOR_AMD_BURST_FIRST_COL"], "last_col": defs["FOSPHOR_AMD_BURST_LAST_COL"]}
    assert F.BURST_FLAGS == dict(on=bm.ON, cut=bm.CUT, first_col=bm.FIRST_COL, last_col=bm.LAST_COL)
    m = re.search(r"enum\s*\{([^}]*FOSPHOR_AMD_BURST_STATS[^}]*)\}", text)
    names = [s.strip() for s in m.group(1).split(",") if s.strip()]
    assert names == ["FOSPHOR_AMD_BURST_" + k.upper() for k in F.BURST_STATS] + ["FOSPHOR_AMD_BURST_STATS"]
    assert lib.SIGNATURES["fosphor_amd_burst_stats"][1][1]._type_._length_ == len(F.BURST_STATS)

    def fields(struct):
        body = re.split(r"struct %s\b[^{;()]*\{" % struct, text)[1].split("};")[0]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                out += [w.strip().split()[-1] for w in decl.split(",")]
        return out
    assert [n for n, _ in lib.BurstCfg._fields_] == fields("fosphor_amd_burst_cfg") == list(bm.CFG_DTYPE.names)
    assert [n for n, _ in lib.Burst._fields_] == fields("fosphor_amd_burst") == list(bm.BURST_DTYPE.names) == list(F.BURST_DTYPE.names)
    assert [n for n, _ in lib.BurstResult._fields_] == fields("fosphor_amd_burst_result") == list(bm.RESULT_NAMES)
    assert C.sizeof(lib.BurstCfg) == bm.CFG_DTYPE.itemsize == 36
    assert C.sizeof(lib.Burst) == bm.BURST_DTYPE.itemsize == F.BURST_DTYPE.itemsize == 40 and F.BURST_DTYPE == bm.BURST_DTYPE
    assert C.sizeof(lib.BurstResult) == bm.RESULT_DTYPE.itemsize == 20
    for dtype, struct in ((bm.BURST_DTYPE, lib.Burst), (bm.CFG_DTYPE, lib.BurstCfg), (bm.RESULT_DTYPE, lib.BurstResult)):
        for name in dtype.names:
            assert dtype.fields[name][1] == getattr(struct, name).offset, name


def test_symbols_exported_and_bound(amd):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fosphor_amd_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["fosphor_amd_burst_stats", "fosphor_amd_bursts", "fosphor_amd_bursts_host"]
    lib = C.CDLL(amd.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
        assert name in amd._lib.SIGNATURES, name
    assert hasattr(amd.Fosphor, "bursts") and hasattr(amd.Fosphor, "burst_stats")


def test_burst_kernels_do_not_spill():
    """-Rpass-analysis=kernel-resource-usage: every kernel of fosphor_burst.hip has 0 bytes of scratch and at most 64 VGPRs (8 waves
    per SIMD)"""
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
    ours = {k: v for k, v in found.items() if re.search(r"k_burst_(runs|rows|scan|init|link|reduce|emit)", k)}
    assert len(ours) == 8, sorted(found)						# k_burst_runs twice: it counts, it writes
    for name, res in ours.items():
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 0) <= 64, (name, res)
