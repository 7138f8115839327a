"""Host side of include/fosphor_amd_psd.h, no GPU: fosphor_amd_psd_host against the numpy statement (tests/psd_model.py), records and
the whole output buffer bit for bit, on every input set the GPU tests use; that the pinned operation tree is a DFT; the twiddles and
the windows; the refusals; psd_n_seg, psd_ratio_from_db, psd_from_extract and psd_derive; known answers; the chain extract_host ->
psd_host; and the compiled kernels' resources.

Bit for bit means tobytes(): signed zeros, subnormals and the one quiet NaN of each width included."""
import ctypes as C
import errno
import math
import os
import re
import subprocess

import numpy as np
import pytest

import psd_model as pm
from _pkg import gr_fosphor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_psd.hip")
HEADER = os.path.join(ROOT, "include", "fosphor_amd_psd.h")
EINVAL = -errno.EINVAL
CASES = pm.cases()
SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def lib():
    return gr_fosphor_amd.load()


@pytest.fixture(scope="module")
def F():
    gr_fosphor_amd.load()
    return gr_fosphor_amd.Fosphor


def host(lib, case, n_samples=None, n_win=None, n_jobs=None, cap=None, null=(), skew=None):
    """-> (return value, records as uint32 [n_jobs + 1][16] and 2 more, the whole output buffer as uint32), both sentinel-filled
    before the call.  cap: out_capacity, GUARD floats of the buffer lie behind it; skew: (pointer name, bytes)"""
    iq, win = pm.buffers(case)
    jobs = np.ascontiguousarray(case[2], pm.JOB_DTYPE)
    size = pm.capacity(jobs) if cap is None else max(cap, 0) + pm.GUARD
    buf = np.full(size + 1, SENTINEL, np.uint32)
    rec = np.full((len(jobs) + 1) * 16 + 2, SENTINEL, np.uint32)
    ptr = {"iq": iq.ctypes.data, "win": win.ctypes.data, "jobs": jobs.ctypes.data, "records": rec.ctypes.data, "out": buf.ctypes.data}
    for k in null:
        ptr[k] = None
    if skew:
        ptr[skew[0]] += skew[1]
    rv = lib.fosphor_amd_psd_host(ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["win"],
                                  len(win) if n_win is None else n_win, ptr["jobs"], len(jobs) if n_jobs is None else n_jobs,
                                  ptr["records"], ptr["out"], size if cap is None else cap)
    return rv, rec, buf[:size]


def records_of(rec, n_jobs):
    assert np.all(rec[16 * n_jobs:] == SENTINEL), "a record beyond the jobs' was written"
    return rec[:16 * n_jobs].view(pm.RECORD_DTYPE)


def header_value(name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, open(HEADER).read())
    assert m, name
    return int(m.group(1))


def test_the_dtypes_mirror_the_structs(F):
    L = gr_fosphor_amd._lib
    assert pm.JOB_DTYPE.itemsize == 56 and C.sizeof(L.PsdJob) == 56
    assert pm.RECORD_DTYPE.itemsize == 64 and C.sizeof(L.PsdRecord) == 64
    assert F.PSD_JOB_DTYPE == pm.JOB_DTYPE and F.PSD_RECORD_DTYPE == pm.RECORD_DTYPE
    for dtype, struct in ((pm.JOB_DTYPE, L.PsdJob), (pm.RECORD_DTYPE, L.PsdRecord)):
        assert [(k, dtype.fields[k][1]) for k in dtype.names] == [(k, getattr(struct, k).offset) for k, _ in struct._fields_]
    assert F.PSD_STATS == pm.STATS and F.PSD_TRACES == pm.TRACES and F.PSD_PRES == pm.PRES and F.PSD_WINDOWS == pm.WINDOWS
    assert (F.PSD_MAX_JOBS, F.PSD_MIN_LOG, F.PSD_MAX_LOG, F.PSD_TILE) == (pm.MAX_JOBS, pm.MIN_LOG, pm.MAX_LOG, pm.TILE)
    for name, want in (("MAX_JOBS", pm.MAX_JOBS), ("MIN_LOG", pm.MIN_LOG), ("MAX_LOG", pm.MAX_LOG), ("TILE", pm.TILE),
                       ("PRE_NONE", pm.NONE), ("PRE_SQUARE", pm.SQUARE), ("PRE_FOURTH", pm.FOURTH), ("PRE_MAGSQ", pm.MAGSQ),
                       ("TRACE_NONE", pm.T_NONE), ("TRACE_POWER", pm.T_POWER), ("WINDOW_RECT", pm.RECT), ("WINDOW_HANN", pm.HANN),
                       ("WINDOW_BLACKMAN_HARRIS", pm.BH), ("LDS_GROUP", F.PSD_LDS["group"]), ("LDS_WAVE", F.PSD_LDS["wave"]),
                       ("LDS_COMBINE", F.PSD_LDS["combine"])):
        assert header_value("FOSPHOR_AMD_PSD_" + name) == want, name
    for name in ("psd", "psd_host", "psd_jobs", "psd_window", "psd_n_seg", "psd_derive", "psd_stats"):
        assert hasattr(F, name), name


def test_the_cases_hold_what_they_promise():
    jobs = np.concatenate([c[2] for name, c in CASES.items() if name != "full_table"])
    segs = np.array([pm.job_n_seg(j) for j in jobs])
    assert set(pm.LOGS) <= set(jobs["fft_len_log"]) and set(pm.SEG_COUNTS) <= set(segs)
    for form in (jobs["fft_len_log"] <= pm.WAVE_MAX_LOG, jobs["fft_len_log"] > pm.WAVE_MAX_LOG):
        assert set(pm.SEG_COUNTS) <= set(segs[form])
    assert {0, 1, 2, 3} <= set(jobs["offset"]) and {0, 1, 2, 3} <= set(jobs["win_offset"] % 4) and {0, 1, 2, 3} <= set(jobs["win_offset"])
    assert {(int(j["offset"]) & 1, int(j["win_offset"]) & 1) for j in jobs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    traced = jobs[jobs["trace"] == pm.T_POWER]
    assert {int(o) & 1 for o in traced["out_offset"]} == {0, 1} and (jobs["trace"] == pm.T_NONE).any()
    iq, _, lj = CASES["loads"]
    assert (lj["offset"] + lj["n"]).max() == len(iq), "a job ends on the buffer's last sample"
    for log in pm.LOGS:
        L = 1 << log
        assert {L - 1, L, L + 36, L + 37} <= set(lj["n"][lj["fft_len_log"] == log])
    hops = {(int(j["hop"]), 1 << int(j["fft_len_log"])) for j in jobs}
    assert {h for h, L in hops} >= {1, 37} and any(h == L // 2 for h, L in hops) and any(h == L for h, L in hops)
    mixed = CASES["mixed"][2]
    ms = np.array([pm.job_n_seg(j) for j in mixed])
    assert set(mixed["pre"]) == {0, 1, 2, 3} and set(mixed["trace"]) == {0, 1} and set(mixed["fft_len_log"]) == set(pm.LOGS)
    assert (ms == 0).any() and (ms > pm.TILE).any() and set(mixed["obw_fraction"]) == {np.float32(1.0), np.float32(0.99), np.float32(0.5)}
    assert set(mixed["xdb_ratio"]) == {np.float32(1.0), np.float32(1e-3)}
    for k in (1, 3, 4, 5):
        wj = CASES["wave_tiles%d" % k][2]
        assert sum(-(-pm.job_n_seg(j) // pm.TILE) for j in wj) == k and np.all(wj["fft_len_log"] <= pm.WAVE_MAX_LOG)
    full = CASES["full_table"][2]
    fs = np.array([pm.job_n_seg(j) for j in full])
    assert len(full) == pm.MAX_JOBS and set(full["fft_len_log"]) == {6} and (fs == 0).sum() >= pm.MAX_JOBS // 11 and fs.max() == 33
    assert set(full["n"][fs > 0]) == set(range(64, 97))


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_model(lib, F, name):
    case = CASES[name]
    jobs = case[2]
    rv, rec, got = host(lib, case)
    assert rv == 0
    want_rec, want = pm.image(case, SENTINEL, key=name)
    got_rec = records_of(rec, len(jobs))
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d got %s want %s" % (i, got_rec[i], want_rec[i]))
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical"
    for i in np.flatnonzero(got != want)[:10]:
        print("float %d got %08x want %08x" % (i, got[i], want[i]))
    assert got.tobytes() == want.tobytes(), "traces bit-identical, every other float at the sentinel"
    iq, win = pm.buffers(case)
    records, views = F.psd_host(iq, jobs, win)
    assert records.tobytes() == want_rec.tobytes(), "the Python front end gives the same records"
    for j, v in zip(jobs, views):
        at = int(j["out_offset"])
        assert (v is None and pm.n_out(j) == 0) or v.view(np.uint32).tobytes() == want[at:at + pm.n_out(j)].tobytes()
    r = want_rec
    if name == "impulses":
        L = 1 << pm.IMPULSE_LOG
        P = views[0]
        assert np.all(P[0::2] == np.float32(2.0 ** -8)) and np.all(P[1::2] == 0.0), "X[b] = 1 + (-1)^b, exactly"
        assert r["peak_bin"][0] == 0 and r["peak_power"][0] == np.float32(2.0 ** -8), "the smallest index wins the tie"
        assert r["total"][0] == 2.0 and (r["obw_lo"][0], r["obw_hi"][0]) == (256, 766) and 256 % (L // pm.BLOCKS) == 0
        assert (r["xdb_lo"][0], r["xdb_hi"][0]) == (0, L - 2)
        assert np.all(views[1] == views[1][0]) and r["peak_bin"][1] == 0 and (r["obw_lo"][1], r["obw_hi"][1]) == (0, L - 1)
        assert (r["xdb_lo"][1], r["xdb_hi"][1]) == (0, L - 1)
        assert r["peak_bin"][2] in (0, L // 2) and views[2][0] == views[2][L // 2], "two bins tie; index 0 wins"
        assert r["peak_bin"][2] == 0 and (r["xdb_lo"][2], r["xdb_hi"][2]) == (0, L // 2)
        assert r["peak_bin"][3] == 0 and (r["obw_lo"][3], r["obw_hi"][3]) == (16, 46)
    if name == "tones":
        for i, b in enumerate(pm.tones_case()[1]):
            L = int(r["fft_len"][i])
            assert r["peak_bin"][i] == (b + L // 2) % L, (i, b)
            if jobs["pre"][i] == pm.NONE:
                assert r["obw_lo"][i] == r["obw_hi"][i] == r["peak_bin"][i], i
        for i, period in pm.tones_case()[2]:					# MAGSQ: DC is |y|^2's mean; the line is the largest beside it
            L = int(r["fft_len"][i])
            beside = views[i].copy()
            beside[L // 2] = 0.0
            assert r["peak_bin"][i] == L // 2 and int(np.argmax(beside)) in (L // 2 - L // period, L // 2 + L // period), i
    if name == "silence":
        for i in range(len(jobs)):
            assert r["total"][i] == 0.0 and (r["obw_lo"][i], r["obw_hi"][i]) == (-1, -1) and r["n_seg"][i] > 0
            assert r["peak_bin"][i] == 0 and r["peak_power"][i] == 0.0 and (r["xdb_lo"][i], r["xdb_hi"][i]) == (0, r["fft_len"][i] - 1)
            assert views[i] is None or not views[i].view(np.uint32).any(), "a trace of +0.0f"
        assert r["win_energy"][3] == 0.0 and r["win_energy"][0] > 0.0
    if name == "nonfinite":
        assert np.all(r["total"][:2].view(np.uint64) == 0x7ff8000000000000) and np.all(views[0].view(np.uint32) == 0x7fc00000)
        assert np.all(r["peak_bin"][:2] == -1) and np.all(r["xdb_lo"][:2] == -1) and np.all(r["obw_hi"][:2] == -1)
        assert np.isfinite(r["total"][3:5]).all() and np.all(r["peak_bin"][3:5] >= 0), "the jobs beside them are not touched"
        assert not np.isfinite(r["total"][5]) and r["total"][6] == np.inf, "FOURTH of 3e38 overflows in double, the plain spectrum in P32"
        assert np.all(r["total"][8:] >= 0.0) and np.isfinite(r["total"][8:]).all(), "subnormals"
        tiny = np.finfo(np.float32).tiny
        assert np.all(r["peak_power"][11:] > 0.0) and np.all(r["peak_power"][11:] < tiny) and np.all(r["total"][11:] > 0.0), "subnormal P32"
        assert np.all(r["obw_lo"][11:] >= 0) and np.all(r["obw_hi"][11:] >= r["obw_lo"][11:])


@pytest.mark.parametrize("log", pm.LOGS)
def test_the_operation_tree_is_a_dft(log):
    """The model's X for random input against numpy.fft.fft in complex128: max|X - Xnp| <= 16 log2(L) 2^-53 ||X||_2, the radix-2
    rounding bound with slack for the reference's own error.  Observed, the largest ratio of the error to the bound over the eight inputs of
    a length: 0.0080 (L = 64), 0.0069 (128), 0.0031 (256), 0.0025 (512) and 0.0018 (1024)."""
    L = 1 << log
    rng = np.random.default_rng(log)
    x = rng.standard_normal((8, L)) + 1j * rng.standard_normal((8, L))
    Xr, Xi = pm.fft(np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag))
    want = np.fft.fft(x, axis=1)
    for s in range(len(x)):
        err = np.abs(Xr[s] + 1j * Xi[s] - want[s]).max()
        bound = 16.0 * log * 2.0 ** -53 * np.linalg.norm(want[s])
        print("L = %d: max error %.3g, bound %.3g, ratio %.4f" % (L, err, bound, err / bound))
        assert err <= bound


def test_twiddles(lib, F):
    """within 2^-52 of numpy's cos and sin, evaluated in long double so that the rounding of the reference's own argument 2 pi m /
    1024 (up to 2^-52 for arguments of 2 .. pi, which alone would use up the bound) does not count; the figure against the
    plain double evaluation is printed"""
    tw = F.psd_twiddles()
    m = np.arange(512)
    x = (8 * np.arctan(np.longdouble(1.0))) * m.astype(np.longdouble) / 1024
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "a long double with more bits than a double"
    print("twiddles against double numpy: %.3g, against long double numpy: %.3g (2^-52 = %.3g)" % (
        max(np.abs(tw.real - np.cos(2 * np.pi * m / 1024)).max(), np.abs(tw.imag + np.sin(2 * np.pi * m / 1024)).max()),
        max(np.abs(tw.real - np.cos(x)).max(), np.abs(tw.imag + np.sin(x)).max()), 2.0 ** -52))
    assert np.abs(tw.real - np.cos(x)).max() <= 2.0 ** -52
    assert np.abs(tw.imag + np.sin(x)).max() <= 2.0 ** -52
    bits = lambda v: np.float64(v).tobytes()
    assert bits(tw[0].real) == bits(1.0) and bits(tw[0].imag) == bits(0.0), "tw[0] = (1, +0)"
    assert bits(tw[256].real) == bits(0.0) and bits(tw[256].imag) == bits(-1.0)
    assert tw[128].real == -tw[128].imag == math.sqrt(0.5)
    assert np.array_equal(tw.real[:257], -tw.imag[256::-1]), "Re tw[m] = -Im tw[256 - m]"
    assert np.array_equal(tw.real[256:], tw.imag[:256]) and np.array_equal(tw.imag[256:], -tw.real[:256]), "tw[256 + m] = -i tw[m]"
    assert lib.fosphor_amd_psd_twiddles(None) == EINVAL


def test_windows(lib, F):
    def ulp_apart(a, b):
        return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()

    for log in pm.LOGS:
        L = 1 << log
        x = 2.0 * np.pi * np.arange(L) / L
        want = {"rect": np.ones(L), "hann": 0.5 - 0.5 * np.cos(x),
                "blackman_harris": 0.35875 - 0.48829 * np.cos(x) + 0.14128 * np.cos(2 * x) - 0.01168 * np.cos(3 * x)}
        for kind, w in want.items():
            got = F.psd_window(kind, log)
            assert got.dtype == np.float32 and len(got) == L
            assert np.all(np.abs(got.astype(np.float64) - w) <= np.spacing(np.abs(w).astype(np.float32))), (kind, log)
            assert got.tobytes() == pm.window(pm.WINDOWS[kind], log).tobytes()
        assert F.psd_window("hann", log)[0] == 0.0 and F.psd_window("hann", log)[L // 2] == 1.0, "periodic: the peak is at L / 2"
    out = np.zeros(64, np.float32)
    for kind, log, ptr in ((-1, 6, out.ctypes.data), (3, 6, out.ctypes.data), (0, 5, out.ctypes.data), (0, 11, out.ctypes.data), (0, 6, None)):
        assert lib.fosphor_amd_psd_window(kind, log, ptr) == EINVAL
    with pytest.raises(ValueError):
        F.psd_window("kaiser", 6)
    with pytest.raises(ValueError):
        F.psd_window("hann", 11)


def test_n_seg_ratio_from_extract(lib, F):
    for log in pm.LOGS:
        L = 1 << log
        for hop in (1, 37, L // 2, L):
            for n in (0, L - 1, L, L + hop - 1, L + hop, 5 * L + 3, 2 ** 31 - 1):
                assert lib.fosphor_amd_psd_n_seg(n, log, hop) == pm.n_seg(n, log, hop) == F.psd_n_seg(n, log, hop)
    assert lib.fosphor_amd_psd_n_seg(2 ** 31 - 1, 6, 1) == 2 ** 31 - 64
    for n, log, hop in ((-1, 6, 1), (0, 5, 1), (0, 11, 1), (0, 6, 0), (0, 6, 65), (0, 6, -1)):
        assert lib.fosphor_amd_psd_n_seg(n, log, hop) == EINVAL
    assert lib.fosphor_amd_psd_ratio_from_db(0.0) == 1.0 and abs(lib.fosphor_amd_psd_ratio_from_db(-3.0) - 10 ** -0.3) < 1e-15
    assert abs(F.psd_ratio_from_db(-26.0) - 10 ** -2.6) < 1e-17 and F.psd_ratio_from_db(-10.0) == 0.1
    assert math.isnan(F.psd_ratio_from_db(0.5)) and math.isnan(F.psd_ratio_from_db(math.nan))
    e = np.zeros(3, F.EXTRACT_DTYPE)
    e["out_offset"], e["n_out"], e["first"], e["decim"], e["n_taps"] = (7, 1000, 2000), (300, 0, 63), (5, 6, 7), 4, 9
    jobs = F.psd_jobs(e, 6, win_offset=11, pre="square", trace="power", obw_fraction=0.5, xdb=-10.0)
    assert jobs.dtype == pm.JOB_DTYPE and list(jobs["offset"]) == [7, 1000, 2000] and list(jobs["n"]) == [300, 0, 63]
    assert list(jobs["out_offset"]) == [0, 64, 64] and set(jobs["trace"]) == {pm.T_POWER} and set(jobs["pre"]) == {pm.SQUARE}
    assert set(jobs["hop"]) == {32} and set(jobs["win_offset"]) == {11} and set(jobs["obw_fraction"]) == {np.float32(0.5)}
    assert set(jobs["xdb_ratio"]) == {np.float32(0.1)} and set(jobs["fft_len_log"]) == {6}
    assert not F.psd_jobs(e, 8, hop=256)["out_offset"].any() and set(F.psd_jobs(e, 8, hop=256)["hop"]) == {256}
    job = gr_fosphor_amd._lib.PsdJob()
    job.out_offset = 99
    assert lib.fosphor_amd_psd_from_extract(e[:1].tobytes(), 5, 7, 64, pm.MAGSQ, pm.T_POWER, 0.99, 0.25, C.byref(job)) == 0
    assert (job.offset, job.out_offset, job.win_offset, job.n, job.fft_len_log, job.hop, job.pre, job.trace, job.xdb_ratio,
            job.reserved) == (7, 0, 5, 300, 7, 64, pm.MAGSQ, pm.T_POWER, 0.25, 0)
    ok = dict(win=0, log=6, hop=1, pre=0, trace=0, obw=0.99, xdb=0.5)
    for bad_e, bad in ((dict(out_offset=-1), {}), (dict(n_out=-1), {}), ({}, dict(win=-1)), ({}, dict(log=5)), ({}, dict(log=11)),
                       ({}, dict(hop=0)), ({}, dict(hop=65)), ({}, dict(pre=4)), ({}, dict(pre=-1)), ({}, dict(trace=2)),
                       ({}, dict(obw=0.0)), ({}, dict(obw=1.5)), ({}, dict(obw=math.nan)), ({}, dict(xdb=0.0)), ({}, dict(xdb=math.nan))):
        x = e[:1].copy()
        for k, v in bad_e.items():
            x[k] = v
        a = dict(ok, **bad)
        assert lib.fosphor_amd_psd_from_extract(x.tobytes(), a["win"], a["log"], a["hop"], a["pre"], a["trace"], a["obw"], a["xdb"],
                                                C.byref(job)) == EINVAL, (bad_e, bad)
    assert lib.fosphor_amd_psd_from_extract(None, 0, 6, 1, 0, 0, 0.99, 0.5, C.byref(job)) == EINVAL
    assert lib.fosphor_amd_psd_from_extract(e[:1].tobytes(), 0, 6, 1, 0, 0, 0.99, 0.5, None) == EINVAL
    with pytest.raises(ValueError):
        F.psd_jobs(e, 6, pre="cube")


def test_derive_and_known_answers(lib, F):
    """a tone on bin k under a rectangular window: derive returns its frequency and, by Parseval, its mean power, to 1e-12.  The
    record is a function of the float32 trace (rule 5), so the mean power carries P32's rounding, 2^-24 relative, unless the
    bin's power is a float32: the tones on +-L / 4 have samples of 0 and +-amp and a power of amp^2, exactly, and are held to
    1e-12; the tones on other bins are held to 2^-23 and their figure is printed."""
    fs = 48000.0
    for log, k, amp in ((6, 16, 0.5), (8, -64, 2.0), (10, 256, 1.0), (6, 5, 0.5), (8, -100, 2.0), (10, 300, 1.0)):
        L = 1 << log
        y = pm.tone(4 * L, k / L, amp)
        power = np.mean(y.astype(np.float64)[:, 0] ** 2 + y.astype(np.float64)[:, 1] ** 2)
        win = F.psd_window("rect", log)
        jobs = pm.make_jobs([(0, 0, 0, 4 * L, log, L, pm.NONE, pm.T_POWER, 0.99, F.psd_ratio_from_db(-3.0))])
        rec, views = F.psd_host(y, jobs, win)
        v = F.psd_derive(rec, fs)[0]
        assert set(v) == set(F.PSD_VALUES)
        assert rec["peak_bin"][0] == k + L // 2 and rec["obw_lo"][0] == rec["obw_hi"][0] == rec["peak_bin"][0]
        assert abs(v["peak_freq"] - k * fs / L) <= 1e-12 * fs and abs(v["centroid"] - k * fs / L) <= 1e-9 * fs
        print("L = %d k = %d: mean power off by %.3g relative" % (L, k, abs(v["mean_power"] - power) / power))
        assert abs(v["mean_power"] - power) <= (1e-12 if abs(k) == L // 4 else 2.0 ** -23) * power, (v["mean_power"], power)
        assert abs(v["peak_db"] - 10 * math.log10(power * L)) < 1e-5, "the whole power in one bin: total = L * the mean power"
        assert v["obw"] == fs / L and v["xdb_bandwidth"] == fs / L and abs(v["obw_centre"] - k * fs / L) <= 1e-12 * fs
        assert v["rms_width"] < 1e-3 * fs / L
        # SQUARE moves the line to 2 k
        sq = jobs.copy()
        sq["pre"] = pm.SQUARE
        assert F.psd_host(y, sq, win)[0]["peak_bin"][0] == (2 * k + L // 2) % L
    # a Hann window over noise: Parseval holds for the windowed signal, total / L = sum |w y|^2 / sum w^2 averaged over the segments
    y = pm.noise(256, 3)
    win = F.psd_window("hann", 8)
    rec, _ = F.psd_host(y, pm.make_jobs([(0, 0, 0, 256, 8, 256, pm.NONE, pm.T_NONE, 0.99, 0.5)]), win)
    w = win.astype(np.float64)
    want = ((y.astype(np.float64) ** 2).sum(1) * w * w).sum() / (w * w).sum()
    assert abs(F.psd_derive(rec, 1.0)[0]["mean_power"] - want) <= 1e-6 * want		# P32 is rounded to float32
    # the zeros
    r = np.zeros(1, pm.RECORD_DTYPE)
    r["fft_len"], r["total"], r["peak_bin"] = 64, 1.0, 3
    assert all(x == 0 for x in F.psd_derive(r, 1.0)[0].values()), "n_seg == 0"
    r["n_seg"] = 1
    for total in (0.0, -1.0, math.inf, math.nan):
        r["total"] = total
        assert all(x == 0 for x in F.psd_derive(r, 1.0)[0].values()), total
    vals = gr_fosphor_amd._lib.PsdValues()
    for rate in (0.0, -1.0, math.inf, math.nan):
        assert lib.fosphor_amd_psd_derive(r.tobytes(), rate, C.byref(vals)) == EINVAL
    assert lib.fosphor_amd_psd_derive(None, 1.0, C.byref(vals)) == EINVAL
    assert lib.fosphor_amd_psd_derive(r.tobytes(), 1.0, None) == EINVAL


def test_einval_table(lib):
    """each refused call leaves every float and every record at the sentinel (the rows of tests/test_gpu_psd.py)"""
    iq = pm.noise(3000, 91)
    win = np.concatenate([pm.window(pm.HANN, 6), pm.window(pm.BH, 8), np.ones(3, np.float32)])	# 64 + 256 + 3 floats
    nw = len(win)
    #        offset out win n    log hop pre      trace       obw   xdb
    good = [(0, 3, 0, 500, 6, 32, pm.NONE, pm.T_POWER, 0.99, 0.1), (2990, 0, 64, 10, 8, 256, pm.SQUARE, pm.T_NONE, 0.5, 1.0),
            (3000, 67, 67, 0, 8, 1, pm.MAGSQ, pm.T_POWER, 1.0, 1e-3), (1, 144, 64, 2999, 8, 100, pm.FOURTH, pm.T_POWER, 0.99, 0.1)]
    cap = 144 + 256
    rv, rec, out = host(lib, (iq, win, pm.make_jobs(good)), cap=cap)
    assert rv == 0 and np.all(out[cap:] == SENTINEL) and np.all(out[144:cap] != SENTINEL) and np.all(out[3:67] != SENTINEL)
    assert np.all(out[67:144] == SENTINEL) and np.all(records_of(rec, 4).view(np.uint32) != SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        rv, rec, out = host(lib, (iq, win, pm.make_jobs(rows)), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL), "nothing is written"

    for what in ("iq", "win", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (pm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=2999); refused(good, n_win=-1); refused(good, n_win=319)
    refused(good, cap=-1); refused(good, cap=cap - 1)
    ok = (0, 0, 0, 100, 6, 16, pm.NONE, pm.T_POWER, 0.99, 0.1)

    def one(**kw):
        row = dict(zip(("offset", "out_offset", "win_offset", "n", "fft_len_log", "hop", "pre", "trace", "obw_fraction", "xdb_ratio"), ok))
        row.update(kw)
        refused([tuple(row.values())])

    one(offset=-1); one(out_offset=-1); one(win_offset=-1); one(n=-1); one(offset=2901); one(offset=3001, n=0)
    one(offset=2 ** 62, n=2 ** 31 - 1); one(fft_len_log=5); one(fft_len_log=11); one(fft_len_log=-1); one(fft_len_log=40)
    one(win_offset=nw - 63); one(win_offset=2 ** 62); one(fft_len_log=9); one(hop=0); one(hop=-1); one(hop=65)
    one(pre=4); one(pre=-1); one(trace=2); one(trace=-1); one(trace=pm.T_NONE, out_offset=1)
    one(obw_fraction=0.0); one(obw_fraction=-0.5); one(obw_fraction=1.0000001); one(obw_fraction=np.nan); one(obw_fraction=np.inf)
    one(xdb_ratio=0.0); one(xdb_ratio=-1.0); one(xdb_ratio=1.5); one(xdb_ratio=np.nan)
    one(out_offset=cap + 1, n=0); one(out_offset=2 ** 62); one(out_offset=cap - 63)
    refused([ok, ok[:1] + (63,) + ok[2:]])						# [0, 64) and [63, 127): one float shared
    refused([ok[:1] + (200,) + ok[2:], (0, 8, 64, 300, 8, 16, 0, 1, 0.5, 0.5)])	# [200, 264) and [8, 264), given in descending order
    for name in ("iq", "records"):
        refused(good, skew=(name, 4))
    refused(good, skew=("out", 2)); refused(good, skew=("win", 2))
    # the last jobs that still fit; traces that touch; jobs without segments anywhere inside
    last = pm.make_jobs([(0, 0, 0, 64, 6, 64, 0, 1, 0.99, 0.1), (0, 64, 0, 65, 6, 1, 0, 1, 0.99, 0.1), (2744, cap - 256, nw - 256, 256, 8, 256, 0, 1, 1.0, 1.0),
                         (3000, cap, nw - 64, 0, 6, 1, 0, 1, 0.99, 0.1), (5, cap, nw - 256, 255, 8, 1, 0, 1, 0.99, 0.1)])
    assert host(lib, (iq, win, last), cap=cap)[0] == 0
    # no job has a trace: no output buffer is needed
    none = pm.make_jobs([(0, 0, 0, 1000, 8, 128, 0, 0, 0.99, 0.1)])
    rv, rec, out = host(lib, (iq, win, none), cap=0, null=("out",))
    assert rv == 0 and records_of(rec, 1).tobytes() == pm.psd((iq, win, none))[0].tobytes()
    many = pm.make_jobs([(0, 64 * i, 0, 64, 6, 64, 0, 1, 0.99, 0.1) for i in range(pm.MAX_JOBS)])
    assert host(lib, (iq, win, many))[0] == 0
    # more than 2^31 - 1 tiles in a form: MAX_JOBS overlapping jobs of 2^31 - 1 samples at hop 1 (2^26 tiles each), refused before
    # a sample is read
    n = 2 ** 31 - 1
    huge = pm.make_jobs([(0, 0, 0, n, 6, 1, 0, 0, 0.99, 0.1) for i in range(pm.MAX_JOBS)])
    rec = np.full(16 * pm.MAX_JOBS, SENTINEL, np.uint32)
    assert lib.fosphor_amd_psd_host(iq.ctypes.data, n, win.ctypes.data, nw, huge.ctypes.data, len(huge), rec.ctypes.data, None, 0) == EINVAL
    assert np.all(rec == SENTINEL)
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    assert lib.fosphor_amd_psd(None, iq.ctypes.data, 3000, win.ctypes.data, nw, none.ctypes.data, 1, rec.ctypes.data, None, 0) == EINVAL
    assert lib.fosphor_amd_psd_stats(None, None) == EINVAL


def test_chain_on_the_host(lib, F):
    """the QPSK preamble of correlate_model's small sc16 stream through fosphor_amd_extract_host and fosphor_amd_psd_host: records
    and traces bit-identical to the model; the plain spectrum is centred on the extraction's centre and the fourth power, which
    strips the QPSK modulation, has its line within a bin of DC"""
    import correlate_model as cm
    raw, ejobs, _, _ = cm.chain_case()
    taps = F.extract_design(cm.CHAIN_DECIM, cm.CHAIN_TAPS, 0.8)
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    out = np.zeros((cap, 2), np.float32)
    assert lib.fosphor_amd_extract_host(raw.ctypes.data, len(raw), 2, ejobs.ctypes.data, len(ejobs), taps.ctypes.data, len(taps),
                                        out.ctypes.data, cap) == 0
    # the burst alone: from the planted lag on, CHAIN_T output samples
    burst = ejobs.copy()
    burst["out_offset"] += cm.CHAIN_LAG
    burst["n_out"] = cm.CHAIN_T
    win = F.psd_window("hann", pm.CHAIN_LOG)
    jobs = np.concatenate([pm.chain_jobs(F, ejobs), pm.chain_jobs(F, burst)])
    jobs["out_offset"][2:] += 2 * ((1 << pm.CHAIN_LOG) + pm.GUARD)
    records, views = F.psd_host(out, jobs, win)
    want_rec, want, _ = pm.psd((out, win, jobs))
    assert records.tobytes() == want_rec.tobytes()
    for v, w in zip(views, want):
        assert v.tobytes() == w.tobytes()
    L = 1 << pm.CHAIN_LOG
    v = F.psd_derive(records, 1.0)
    print("chain: burst peak bins %s, centroid %.4f, fourth-power peak bin %d of %d" % (records["peak_bin"][2:], v[2]["centroid"], records["peak_bin"][3], L))
    assert records["n_seg"][0] > pm.TILE and records["n_seg"][2] == pm.n_seg(cm.CHAIN_T, pm.CHAIN_LOG, L // 2) > 1
    assert abs(int(records["peak_bin"][3]) - L // 2) <= 1, "the carrier line of the fourth power"
    assert abs(v[2]["centroid"]) < 0.05, "the burst's spectrum is centred"


def test_psd_kernels_meet_their_resources(F):
    """-Rpass-analysis=kernel-resource-usage: every kernel of fosphor_psd.hip has 0 bytes of scratch, at most 128 VGPRs and the
    static LDS that the header states for it"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-x", "hip", "--cuda-device-only",
                        "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        for key in ("ScratchSize", "VGPRs", "LDS Size"):
            m = re.search(r"remark:\s+%s( \[bytes/(lane|block)\])?: (\d+)" % key, line)
            if m and cur:
                found.setdefault(cur, {})[key] = int(m.group(3))
    ours = {k: v for k, v in found.items() if "k_psd_" in k}
    assert len(ours) == 3 and len(found) == 3, sorted(found)
    for name, res in ours.items():
        form = re.search(r"k_psd_(group|wave|combine)", name).group(1)
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 1 << 30) <= 128, (name, res)
        assert res.get("LDS Size") == F.PSD_LDS[form] == header_value("FOSPHOR_AMD_PSD_LDS_" + form.upper()), (name, res)
