"""Host side of include/fosphor_amd_symbols.h, no GPU: fosphor_amd_symbols_host against the numpy statement (tests/symbols_model.py),
records and the whole output buffer bit for bit, on every input set the GPU tests use; the twiddles; the refusals; symbols_max_out,
symbols_jobs and symbols_derive; that a job's bytes depend on the job alone; that the estimator finds the symbols of raised-cosine
QPSK and BPSK; the chain resample_host -> symbols_host; and the compiled kernels' resources.

Bit for bit means tobytes(): signed zeros, subnormals and the one quiet NaN of each width included."""
import ctypes as C
import errno
import math
import os
import re
import subprocess

import numpy as np
import pytest

import symbols_model as sm
from _pkg import gr_fosphor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_symbols.hip")
HEADER = os.path.join(ROOT, "include", "fosphor_amd_symbols.h")
EINVAL = -errno.EINVAL
CASES = sm.cases()
SENTINEL = 0x5a5a5a5a
W = sm.RECORD_WORDS


@pytest.fixture(scope="module")
def lib():
    return gr_fosphor_amd.load()


@pytest.fixture(scope="module")
def F():
    gr_fosphor_amd.load()
    return gr_fosphor_amd.Fosphor


def host(lib, case, n_samples=None, n_jobs=None, cap=None, null=(), skew=None):
    """-> (return value, records as uint32 [n_jobs + 1][24] and 2 more, the whole output buffer as uint32 [size][2]), both
    sentinel-filled before the call.  cap: out_capacity, GUARD samples of the buffer lie behind it; skew: (pointer name, bytes)"""
    iq = sm.buffer(case)
    jobs = np.ascontiguousarray(case[1], sm.JOB_DTYPE)
    size = sm.capacity(jobs) if cap is None else max(cap, 0) + sm.GUARD
    buf = np.full((size + 1, 2), SENTINEL, np.uint32)
    rec = np.full((len(jobs) + 1) * W + 2, SENTINEL, np.uint32)
    ptr = {"iq": iq.ctypes.data, "jobs": jobs.ctypes.data, "records": rec.ctypes.data, "out": buf.ctypes.data}
    for k in null:
        ptr[k] = None
    if skew:
        ptr[skew[0]] += skew[1]
    rv = lib.fosphor_amd_symbols_host(ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["jobs"],
                                      len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"], size if cap is None else cap)
    return rv, rec, buf[:size]


def records_of(rec, n_jobs):
    assert np.all(rec[W * n_jobs:] == SENTINEL), "a record beyond the jobs' was written"
    return rec[:W * n_jobs].view(sm.RECORD_DTYPE)


def header_value(name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, open(HEADER).read())
    assert m, name
    return int(m.group(1))


def test_the_dtypes_mirror_the_structs(F):
    L = gr_fosphor_amd._lib
    assert sm.JOB_DTYPE.itemsize == 40 and C.sizeof(L.SymbolsJob) == 40
    assert sm.RECORD_DTYPE.itemsize == 96 and C.sizeof(L.SymbolsRecord) == 96
    assert F.SYMBOLS_JOB_DTYPE == sm.JOB_DTYPE and F.SYMBOLS_RECORD_DTYPE == sm.RECORD_DTYPE
    for dtype, struct in ((sm.JOB_DTYPE, L.SymbolsJob), (sm.RECORD_DTYPE, L.SymbolsRecord)):
        assert [(k, dtype.fields[k][1]) for k in dtype.names] == [(k, getattr(struct, k).offset) for k, _ in struct._fields_]
    assert F.SYMBOLS_STATS == sm.STATS and F.SYMBOLS_MODES == sm.MODES and F.SYMBOLS_STATUS == sm.STATUS
    assert (F.SYMBOLS_MAX_JOBS, F.SYMBOLS_MIN_SPS, F.SYMBOLS_MAX_SPS, F.SYMBOLS_BLOCK, F.SYMBOLS_TILE, F.SYMBOLS_STAGE_SPS) == (
        sm.MAX_JOBS, sm.MIN_SPS, sm.MAX_SPS, sm.BLOCK, sm.TILE, sm.STAGE_SPS)
    for name, want in (("MAX_JOBS", sm.MAX_JOBS), ("MIN_SPS", sm.MIN_SPS), ("MAX_SPS", sm.MAX_SPS), ("BLOCK", sm.BLOCK), ("TILE", sm.TILE),
                       ("STAGE_SPS", sm.STAGE_SPS), ("ESTIMATE", sm.ESTIMATE), ("FIXED", sm.FIXED), ("OK", sm.OK),
                       ("NO_TIMING", sm.NO_TIMING), ("LDS_FOLD", F.SYMBOLS_LDS["fold"]), ("LDS_TIME", F.SYMBOLS_LDS["time"]),
                       ("LDS_PICK", F.SYMBOLS_LDS["pick"]), ("LDS_RECORD", F.SYMBOLS_LDS["record"])):
        assert header_value("FOSPHOR_AMD_SYMBOLS_" + name) == want, name
    for name in ("symbols", "symbols_host", "symbols_jobs", "symbols_derive", "symbols_stats", "symbols_max_out", "symbols_twiddles"):
        assert hasattr(F, name), name


def test_the_cases_hold_what_they_promise():
    jobs = np.concatenate([c[1] for name, c in CASES.items() if "table" not in name and "only" not in name])
    records = np.concatenate([sm.symbols(c)[0] for name, c in CASES.items() if "table" not in name and "only" not in name])
    est, fix = jobs["mode"] == sm.ESTIMATE, jobs["mode"] == sm.FIXED
    assert set(sm.SPS) <= set(jobs["sps"][fix]) and set(sm.SPS[1:]) <= set(jobs["sps"][est])
    assert {(int(j["offset"]) & 1, int(j["out_offset"]) & 1) for j in jobs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    iq, lj = CASES["loads"]
    assert (lj["offset"] + lj["n"]).max() == len(iq), "a job ends on the buffer's last sample"
    fj = CASES["fold"][1]
    assert set(sm.FOLD_COUNTS) <= set((fj["n"] // fj["sps"])[fj["sps"] == 3]) and np.all(fj["n"][fj["sps"] == 3] % 3 != 0)
    assert 65 in set((fj["n"] // fj["sps"])[fj["sps"] == 64])
    pj = CASES["pick"][1]
    pr = sm.symbols(CASES["pick"])[0]
    for sps in (4, 16):
        assert set(sm.PICK_COUNTS) <= set(pr["n_sym"][pj["sps"] == sps]), sps
        assert {3, 4, sps + 3} <= set(pj["n"][pj["sps"] == sps])
        assert {69, 70} <= set(pr["n_sym"][pj["sps"] == sps]), "g + 2 == n - 1 holds and just fails"
    qr = sm.symbols(CASES["phase_fixed"])[0]
    qj = CASES["phase_fixed"][1]
    assert np.all(qr["first"][qj["tau"] == 0.0] == qj["sps"][qj["tau"] == 0.0]), "tau = 0 drops symbol 0: first = sps"
    assert (qr["mu"] == 0.0).sum() >= 10 and np.float32(0.99999994) in set(qj["tau"])
    er = sm.symbols(CASES["phase_estimate"])[0]
    assert list(er["tau"][:6][[0, 1, 2, 3, 4]]) == [0.0, 0.0, 0.5, 0.5, 0.0] and 0.999 < er["tau"][5] < 1.0
    assert er["x_re"][0] == 0.0 and er["x_im"][0] == 0.0 and er["x_im"][1] == 0.0 and er["x_re"][1] > 0.0
    assert er["x_im"][3] < 0.0 and er["x_re"][3] < 0.0 and er["x_im"][4] == 2.0 ** -52 and er["x_re"][4] == 2.0 ** 40
    assert er["status"][12] == sm.NO_TIMING and np.all(er["status"][13] == sm.OK) and er["n_sym"][12] == 0
    assert (records["status"] == sm.NO_TIMING).sum() >= 1 and (records["n_sym"] == 0).sum() >= 5
    nr = sm.symbols(CASES["numbers"])[0]
    assert np.isinf(nr["m2"]).any() and np.isnan(nr["z4_re"]).any() and (nr["m4"] > 1e200).any() and (nr["m2"] < 1e-70).any()
    mixed = CASES["mixed"][1]
    assert set(mixed["mode"]) == {0, 1} and set(mixed["sps"]) == set(sm.SPS) and (mixed["n"] < 4).any()
    for name, modes in (("full_table", {0, 1}), ("only_fixed", {1}), ("only_estimate", {0})):
        full = CASES[name][1]
        assert len(full) == sm.MAX_JOBS and set(full["mode"]) == modes and (full["n"] == 0).sum() >= sm.MAX_JOBS // 11


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_model(lib, F, name):
    case = CASES[name]
    jobs = case[1]
    rv, rec, got = host(lib, case)
    assert rv == 0
    want_rec, want = sm.image(case, SENTINEL, key=name)
    got_rec = records_of(rec, len(jobs))
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical"
    for i in np.flatnonzero((got != want).any(1))[:10]:
        print("sample %d got %s want %s" % (i, got[i], want[i]))
    assert got.tobytes() == want.tobytes(), "symbols bit-identical, every other sample at the sentinel"
    records, views = F.symbols_host(sm.buffer(case), jobs)
    assert records.tobytes() == want_rec.tobytes(), "the Python front end gives the same records"
    for j, r, v in zip(jobs, records, views):
        at = int(j["out_offset"])
        assert len(v) == r["n_sym"] and v.view(np.uint32).tobytes() == want[at:at + len(v)].tobytes()


def test_twiddles(lib, F):
    """exact at whole quarter turns, every zero +0; elsewhere within 2^-52 of numpy's cos and sin evaluated in long double (the
    comparison that tests/test_psd_cpu.py found to hold: in double the reference's own argument rounding uses up the bound)"""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "a long double with more bits than a double"
    bits = lambda v: np.float64(v).tobytes()
    worst = 0.0
    for sps in range(sm.MIN_SPS, sm.MAX_SPS + 1):
        tw = F.symbols_twiddles(sps)
        assert tw.shape == (sps,)
        x = (8 * np.arctan(np.longdouble(1.0))) * np.arange(sps).astype(np.longdouble) / sps
        err = max(np.abs(tw.real - np.cos(x)).max(), np.abs(tw.imag + np.sin(x)).max())
        worst = max(worst, float(err))
        assert err <= 2.0 ** -52, sps
        assert bits(tw[0].real) == bits(1.0) and bits(tw[0].imag) == bits(0.0), "tw[0] = (1, +0)"
        if sps % 2 == 0:
            assert bits(tw[sps // 2].real) == bits(-1.0) and bits(tw[sps // 2].imag) == bits(0.0)
        if sps % 4 == 0:
            assert bits(tw[sps // 4].real) == bits(0.0) and bits(tw[sps // 4].imag) == bits(-1.0)
            assert bits(tw[3 * sps // 4].real) == bits(0.0) and bits(tw[3 * sps // 4].imag) == bits(1.0)
        if sps % 8 == 0:
            assert tw[sps // 8].real == -tw[sps // 8].imag == math.sqrt(0.5)
        assert np.array_equal(tw.real[1:], tw.real[1:][::-1]) and np.array_equal(tw.imag[1:], -tw.imag[1:][::-1]), "tw[sps - k] = conj tw[k]"
        assert tw.tobytes() == (sm.twiddles(sps)[0] + 1j * sm.twiddles(sps)[1]).tobytes()
    print("twiddles against long double numpy: %.3g at worst (2^-52 = %.3g)" % (worst, 2.0 ** -52))
    out = np.zeros(128)
    for sps, ptr in ((1, out.ctypes.data), (65, out.ctypes.data), (-1, out.ctypes.data), (4, None)):
        assert lib.fosphor_amd_symbols_twiddles(sps, ptr) == EINVAL
    with pytest.raises(ValueError):
        F.symbols_twiddles(65)


def test_max_out_and_jobs(lib, F):
    for sps in sm.SPS:
        for n in (0, 3, 4, sps + 3, sps + 4, 5 * sps + 2, 2 ** 31 - 1):
            assert lib.fosphor_amd_symbols_max_out(n, sps) == sm.max_out(n, sps) == F.symbols_max_out(n, sps)
    for n, sps in ((-1, 4), (10, 1), (10, 65), (10, 0)):
        assert lib.fosphor_amd_symbols_max_out(n, sps) == EINVAL
    # whatever tau gives, n_sym stays inside the reservation, and tau just above 0 reaches it
    for sps in sm.SPS:
        for n in range(0, 4 * sps + 8):
            counts = [sm.place_of(np.float64(np.float32(t)), n, sps)[2] for t in (0.0, 0.5 / sps, 1.0 / sps, 0.5, 0.99999994)]
            assert max(counts) == sm.max_out(n, sps) and min(counts) >= 0, (sps, n)
    e = np.zeros(3, F.EXTRACT_DTYPE)
    e["out_offset"], e["n_out"], e["first"], e["decim"], e["n_taps"] = (7, 1000, 2000), (300, 0, 63), (5, 6, 7), 4, 9
    jobs = F.symbols_jobs(e, 4)
    assert jobs.dtype == sm.JOB_DTYPE and list(jobs["offset"]) == [7, 1000, 2000] and list(jobs["n"]) == [300, 0, 63]
    assert list(jobs["out_offset"]) == [0, 75, 75] and set(jobs["mode"]) == {sm.ESTIMATE} and set(jobs["sps"]) == {4}
    assert not jobs["tau"].any() and not jobs["reserved"].any()
    r = np.zeros(2, F.RESAMPLE_JOB_DTYPE)
    r["out_offset"], r["n_out"], r["offset"], r["n"], r["up"], r["down"], r["n_taps"] = (11, 500), (41, 9), 3, 100, 2, 3, 24
    jobs = F.symbols_jobs(r, 2, mode="fixed", tau=0.25)
    assert list(jobs["offset"]) == [11, 500] and list(jobs["n"]) == [41, 9] and list(jobs["out_offset"]) == [0, 19]
    assert set(jobs["mode"]) == {sm.FIXED} and set(jobs["tau"]) == {np.float32(0.25)}
    job = gr_fosphor_amd._lib.SymbolsJob()
    job.out_offset = 99
    assert lib.fosphor_amd_symbols_from_resample(r[:1].tobytes(), 5, sm.ESTIMATE, 0.0, C.byref(job)) == 0
    assert (job.offset, job.out_offset, job.n, job.sps, job.mode, job.tau, job.reserved[0], job.reserved[1]) == (11, 0, 41, 5, 0, 0.0, 0, 0)
    for make, src in ((lib.fosphor_amd_symbols_from_extract, e), (lib.fosphor_amd_symbols_from_resample, r)):
        for bad_src, sps, mode, tau in ((dict(out_offset=-1), 4, 0, 0.0), (dict(n_out=-1), 4, 0, 0.0), ({}, 1, 1, 0.0), ({}, 65, 1, 0.0),
                                        ({}, 2, 0, 0.0), ({}, 4, 2, 0.0), ({}, 4, -1, 0.0), ({}, 4, 0, 0.5), ({}, 4, 1, 1.0),
                                        ({}, 4, 1, -0.1), ({}, 4, 1, math.nan)):
            x = src[:1].copy()
            for k, v in bad_src.items():
                x[k] = v
            assert make(x.tobytes(), sps, mode, tau, C.byref(job)) == EINVAL, (bad_src, sps, mode, tau)
        assert make(None, 4, 0, 0.0, C.byref(job)) == EINVAL and make(src[:1].tobytes(), 4, 0, 0.0, None) == EINVAL
    with pytest.raises(ValueError):
        F.symbols_jobs(e, 4, mode="track")


def test_derive(lib, F):
    """records built by hand"""
    fs = 48000.0
    r = np.zeros(1, sm.RECORD_DTYPE)
    r["n_sym"], r["first"], r["tau"], r["mu"] = 100, 3, 0.8125, 0.25
    r["x_re"], r["x_im"], r["a0"] = 3.0, -4.0, 100.0
    r["m2"], r["m4"] = 100.0, 100.0						# unit modulus, no noise: S = 1, N = 0
    r["z2_re"], r["z2_im"], r["z4_re"], r["z4_im"] = 0.0, 0.0, 0.0, 100.0
    v = F.symbols_derive(r, 4, fs)[0]
    assert set(v) == set(F.SYMBOLS_VALUES)
    assert v["tau"] == 0.8125 and v["t_first"] == 3.25 / fs and v["symbol_rate"] == fs / 4 and v["timing_depth"] == 0.1
    assert v["sym_power"] == 1.0 and v["snr_db"] == 0.0, "N is not positive: 0"
    assert v["lock2"] == 0.0 and v["lock4"] == 1.0 and abs(v["phase4"] - math.pi / 8) < 1e-15 and v["phase2"] == 0.0
    # unit-modulus symbols in complex noise of variance N: M2 = 1 + N, M4 = 1 + 4 N + 2 N^2
    N = 0.1
    r["m2"], r["m4"] = 100.0 * (1 + N), 100.0 * (1 + 4 * N + 2 * N * N)
    r["z2_re"], r["z2_im"] = -55.0, 0.0
    v = F.symbols_derive(r, 4, fs)[0]
    assert abs(v["snr_db"] - 10.0) < 1e-9 and abs(v["sym_power"] - 1.1) < 1e-15
    assert abs(v["phase2"] - math.pi / 2) < 1e-15 and abs(v["lock2"] - 0.5) < 1e-15
    # nothing is ever NaN
    r["n_sym"] = 0
    v = F.symbols_derive(r, 4, fs)[0]
    assert v["tau"] == 0.8125 and v["symbol_rate"] == fs / 4 and all(x == 0 for k, x in v.items() if k not in ("tau", "symbol_rate"))
    r["n_sym"], r["tau"], r["status"] = 0, np.nan, sm.NO_TIMING
    assert all(not math.isnan(x) for x in F.symbols_derive(r, 4, fs)[0].values())
    r["n_sym"], r["tau"] = 5, 0.5
    for field in ("m2", "m4", "z2_re", "z4_im", "a0", "x_re"):
        for bad in (0.0, -1.0, math.inf, math.nan):
            x = r.copy()
            x[field] = bad
            assert all(math.isfinite(y) for y in F.symbols_derive(x, 4, fs)[0].values()), (field, bad)
    vals = gr_fosphor_amd._lib.SymbolsValues()
    for sps, rate in ((4, 0.0), (4, -1.0), (4, math.inf), (4, math.nan), (1, fs), (65, fs)):
        assert lib.fosphor_amd_symbols_derive(r.tobytes(), sps, rate, C.byref(vals)) == EINVAL
    assert lib.fosphor_amd_symbols_derive(None, 4, 1.0, C.byref(vals)) == EINVAL
    assert lib.fosphor_amd_symbols_derive(r.tobytes(), 4, 1.0, None) == EINVAL


def test_a_job_alone_among_others_and_shuffled(F):
    """a record and a job's symbols depend on their job alone"""
    iq, jobs = CASES["mixed"]
    among_rec, among = F.symbols_host(iq, jobs)
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = F.symbols_host(iq, jobs[order])
    assert shuffled_rec.tobytes() == among_rec[order].tobytes()
    for k, i in enumerate(order):
        assert shuffled[k].tobytes() == among[i].tobytes()
    for i in (0, 1, 3, len(jobs) - 1):
        alone_rec, alone = F.symbols_host(iq, jobs[i:i + 1])
        assert alone_rec[0].tobytes() == among_rec[i].tobytes() and alone[0].tobytes() == among[i].tobytes(), i


def test_einval_table(lib):
    """each refused call leaves every sample and every record at the sentinel (the rows of tests/test_gpu_symbols.py)"""
    iq = sm.noise(3000, 91)
    #        offset out  n   sps mode         tau
    good = [(0, 5, 500, 4, sm.ESTIMATE, 0.0), (2990, 0, 10, 2, sm.FIXED, 0.5), (3000, 130, 0, 3, sm.ESTIMATE, 0.0),
            (1, 140, 2999, 64, sm.FIXED, 0.99)]
    cap = 140 + sm.max_out(2999, 64)
    assert sm.max_out(500, 4) == 125 and sm.max_out(10, 2) == 4
    rv, rec, out = host(lib, (iq, sm.make_jobs(good)), cap=cap)
    assert rv == 0 and np.all(out[cap:] == SENTINEL) and np.all(out[130:140] == SENTINEL) and np.all(out[0:4] != SENTINEL)
    assert np.all(records_of(rec, 4).view(np.uint32)[:, None] != SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        jobs = sm.make_jobs(rows)
        for i, res in kw.pop("reserved", []):
            jobs["reserved"][0][i] = res
        rv, rec, out = host(lib, (iq, jobs), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL), "nothing is written"

    for what in ("iq", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (sm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=2999); refused(good, cap=-1); refused(good, cap=cap - 1)
    ok = (0, 0, 100, 4, sm.FIXED, 0.25)

    def one(**kw):
        row = dict(zip(("offset", "out_offset", "n", "sps", "mode", "tau"), ok))
        row.update(kw)
        refused([tuple(row.values())])

    one(offset=-1); one(out_offset=-1); one(n=-1); one(offset=2901); one(offset=3001, n=0); one(offset=2 ** 62, n=2 ** 31 - 1)
    one(offset=2 ** 62); one(sps=1); one(sps=0); one(sps=-4); one(sps=65); one(sps=2, mode=sm.ESTIMATE, tau=0.0)
    one(mode=2); one(mode=-1); one(tau=np.nan); one(tau=1.0); one(tau=-0.25); one(tau=np.inf); one(mode=sm.ESTIMATE, tau=0.25)
    one(out_offset=cap + 1, n=0); one(out_offset=2 ** 62); one(out_offset=cap - 24)
    refused([ok], reserved=[(0, 1)]); refused([ok], reserved=[(1, -1)])
    refused([ok, ok[:1] + (24,) + ok[2:]])					# [0, 25) and [24, 49): one sample shared
    refused([ok[:1] + (200,) + ok[2:], (0, 8, 800, 4, sm.FIXED, 0.0)])		# [200, 225) and [8, 208), given in descending order
    for name in ("iq", "records", "out"):
        refused(good, skew=(name, 4))
    # the reservation counts, not n_sym: tau = 0 drops a symbol, yet the neighbour may not begin inside the reserved range
    refused([(0, 0, 100, 4, sm.FIXED, 0.0), (0, 24, 100, 4, sm.FIXED, 0.0)])
    # the last jobs that still fit; reserved ranges that touch; jobs without a symbol anywhere inside
    last = sm.make_jobs([(0, 0, 100, 4, sm.FIXED, 0.0), (0, 25, 100, 4, sm.FIXED, 0.25), (2900, cap - 25, 100, 4, sm.ESTIMATE, 0.0),
                         (3000, cap, 0, 3, sm.ESTIMATE, 0.0), (5, cap, 3, 8, sm.FIXED, 0.5)])
    rv, rec, out = host(lib, (iq, last), cap=cap)
    want_rec, want = sm.image((iq, last), SENTINEL)
    assert rv == 0 and records_of(rec, 5).tobytes() == want_rec.tobytes() and out[:cap].tobytes() == want[:cap].tobytes()
    assert np.all(out[24] == SENTINEL) and np.all(out[23] != SENTINEL), "tau = 0: 24 of the 25 reserved samples are written"
    many = sm.make_jobs([(0, 25 * i, 100, 4, sm.FIXED, 0.5) for i in range(sm.MAX_JOBS)])
    assert host(lib, (iq, many))[0] == 0
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    rec = np.full(W, SENTINEL, np.uint32)
    out = np.full(64, SENTINEL, np.uint32)
    job = sm.make_jobs([ok])
    assert lib.fosphor_amd_symbols(None, iq.ctypes.data, 3000, job.ctypes.data, 1, rec.ctypes.data, out.ctypes.data, 32) == EINVAL
    assert np.all(rec == SENTINEL) and np.all(out == SENTINEL)
    assert lib.fosphor_amd_symbols_stats(None, None) == EINVAL


# ---- function ---------------------------------------------------------------------------------------------------------------------

BETAS = (0.25, 0.35, 0.5)
DELAYS = (0.0, 0.13, 0.37, 0.5, 0.77, 0.96)
TAU_BAR = 2e-3
EVM_BAR = {3: 0.02, 4: 0.01, 8: 0.002}
N_SYMBOLS, LEAD = 512, 8


def burst(order, sps, delay, beta, seed):
    """(float32 [n][2], the symbols): N_SYMBOLS random symbols of a PSK of `order` points through a raised-cosine pulse under a
    random carrier phase; symbol j sits (LEAD + j + delay) sps samples behind sample 0"""
    rng = np.random.default_rng(seed)
    sym = np.exp(2j * np.pi * (rng.integers(0, order, N_SYMBOLS) / order)) * np.exp(1j * rng.uniform(0.0, 2.0 * np.pi))
    y = sm.modulate(sym, sps, delay, beta, lead=LEAD)
    return np.stack([y.real, y.imag], 1).astype(np.float32), sym


def float64_statement(y, sps):
    """rules 1 to 5 in plain float64 numpy, no pinned order and numpy's own angle -> (tau, first, the symbols as complex128)"""
    z = y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)
    R = len(z) // sps
    A = (np.abs(z[:R * sps]) ** 2).reshape(R, sps).sum(0)
    X = (A * np.exp(-2j * np.pi * np.arange(sps) / sps)).sum()
    e = (np.angle(X.conjugate()) / (2.0 * np.pi)) % 1.0
    base = e * sps
    i0 = int(np.floor(base))
    mu = base - i0
    first = i0 if i0 >= 1 else sps
    n_sym = (len(z) - 3 - first) // sps + 1
    g = first + np.arange(n_sym) * sps
    c = (-mu * (mu - 1) * (mu - 2) / 6, (mu + 1) * (mu - 1) * (mu - 2) / 2, -(mu + 1) * mu * (mu - 2) / 2, (mu + 1) * mu * (mu - 1) / 6)
    return e, first + mu, c[0] * z[g - 1] + c[1] * z[g] + c[2] * z[g + 1] + c[3] * z[g + 2]


def evm_of(s, position, sps, delay, phase4):
    """the error vector magnitude of the output symbols that lie on symbols of the burst, after removing phase4: the rms distance
    to the nearest of 1, i, -1, -i over the rms amplitude.  position: samples from sample 0 to output symbol 0"""
    at = np.rint((position + np.arange(len(s)) * sps) / sps - LEAD - delay).astype(int)
    z = (s * np.exp(-1j * phase4))[(at >= 0) & (at < N_SYMBOLS)]
    assert len(z) >= N_SYMBOLS - 1
    z = z / np.sqrt(np.mean(np.abs(z) ** 2))
    ideal = np.exp(0.5j * np.pi * np.rint(np.angle(z) / (0.5 * np.pi)))
    return float(np.sqrt(np.mean(np.abs(z - ideal) ** 2)))


def wrapped(d):
    return abs((d + 0.5) % 1.0 - 0.5)


@pytest.mark.parametrize("sps", sorted(EVM_BAR))
def test_the_estimator_finds_the_symbols_of_qpsk(F, sps):
    """noiseless QPSK through a raised-cosine pulse: |tau - truth| (mod 1) <= 2e-3 symbols and the EVM after removing phase4 within
    0.02 / 0.01 / 0.002 at sps 3 / 4 / 8, for the host statement and for a plain float64 statement of the same rules alike.
    Observed, the worst over the 18 bursts of an sps, host statement (float64 statement): tau error 1.0e-5 (1.0e-5), 1.1e-6
    (1.1e-6) and 1.8e-7 (1.6e-7) symbols; EVM 0.0092 (0.0092), 0.0031 (0.0031) and 0.00017 (0.00017); timing_depth 0.07 to 0.10."""
    worst = dict(tau=0.0, evm=0.0, tau64=0.0, evm64=0.0)
    seed = 0
    for beta in BETAS:
        for delay in DELAYS:
            seed += 1
            y, _ = burst(4, sps, delay, beta, 100 * sps + seed)
            rec, views = F.symbols_host(y, sm.make_jobs([(0, 0, len(y), sps, sm.ESTIMATE, 0.0)]))
            v = F.symbols_derive(rec, sps, 1.0)[0]
            r = rec[0]
            assert r["status"] == sm.OK and r["n_sym"] >= N_SYMBOLS
            evm = evm_of(views[0].astype(np.complex128), r["first"] + r["mu"], sps, delay, v["phase4"])
            e64, pos64, s64 = float64_statement(y, sps)
            z4 = (s64 ** 4).sum()
            evm64 = evm_of(s64, pos64, sps, delay, np.angle(z4) / 4.0)
            print("sps %d beta %.2f delay %.2f: tau %.6f (float64 %.6f) evm %.5f (%.5f) depth %.3f lock4 %.4f lock2 %.4f snr %.1f dB" % (
                sps, beta, delay, r["tau"], e64, evm, evm64, v["timing_depth"], v["lock4"], v["lock2"], v["snr_db"]))
            worst = dict(tau=max(worst["tau"], wrapped(r["tau"] - delay)), evm=max(worst["evm"], evm),
                         tau64=max(worst["tau64"], wrapped(e64 - delay)), evm64=max(worst["evm64"], evm64))
            assert wrapped(r["tau"] - delay) <= TAU_BAR and wrapped(e64 - delay) <= TAU_BAR
            assert evm <= EVM_BAR[sps] and evm64 <= EVM_BAR[sps]
            assert 0.05 <= v["timing_depth"] <= 0.3
            assert v["lock4"] > 0.9 and v["lock2"] < 0.2
            assert abs(v["t_first"] - (r["first"] + r["mu"])) < 1e-12 and v["symbol_rate"] == 1.0 / sps
    print("sps %d worst: tau error %.3g (float64 %.3g), evm %.3g (float64 %.3g)" % (sps, worst["tau"], worst["tau64"], worst["evm"], worst["evm64"]))


def test_bpsk_locks_the_square(F):
    for sps in sorted(EVM_BAR):
        y, _ = burst(2, sps, 0.37, 0.35, 7 + sps)
        rec, _ = F.symbols_host(y, sm.make_jobs([(0, 0, len(y), sps, sm.ESTIMATE, 0.0)]))
        v = F.symbols_derive(rec, sps, 1.0)[0]
        print("BPSK sps %d: tau %.5f lock2 %.4f lock4 %.4f depth %.3f" % (sps, rec["tau"][0], v["lock2"], v["lock4"], v["timing_depth"]))
        assert wrapped(rec["tau"][0] - 0.37) <= TAU_BAR and v["lock2"] > 0.9 and v["lock4"] > 0.9
    # sps = 2 cannot tell tau from tau + 0.5: it is refused under ESTIMATE (test_einval_table) and taken under FIXED
    y, _ = burst(4, 2, 0.25, 0.35, 9)
    rec, views = F.symbols_host(y, sm.make_jobs([(0, 0, len(y), 2, sm.FIXED, 0.25)]))
    v = F.symbols_derive(rec, 2, 1.0)[0]
    assert rec["n_sym"][0] >= N_SYMBOLS and v["lock4"] > 0.9 and v["timing_depth"] == 0.0


def test_chain_on_the_host(lib, F):
    """the QPSK preamble of resample_model's small sc16 stream through fosphor_amd_extract_host, fosphor_amd_resample_host and
    fosphor_amd_symbols_host: the job that symbols_jobs() makes from the resample job gives the symbols of the same samples handed
    in directly, and both are the model's; over the preamble alone the fourth power locks"""
    import resample_model as rm
    raw, ejobs, _, lag = rm.chain_case()
    taps = F.extract_design(rm.CHAIN_DECIM, rm.CHAIN_TAPS, 0.8)
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    x = np.zeros((cap, 2), np.float32)
    assert lib.fosphor_amd_extract_host(raw.ctypes.data, len(raw), 2, ejobs.ctypes.data, len(ejobs), taps.ctypes.data, len(taps),
                                        x.ctypes.data, cap) == 0
    rtaps = F.resample_design(rm.CHAIN_UP, rm.CHAIN_DOWN, rm.CHAIN_BRANCH)
    rjobs = F.resample_jobs(ejobs, rm.CHAIN_UP, rm.CHAIN_DOWN, len(rtaps))
    rjobs["out_offset"] = 5
    y = F.resample_host(x, rjobs, rtaps)[0]
    whole = np.zeros((5 + len(y), 2), np.float32)
    whole[5:] = y.view(np.float32).reshape(-1, 2)
    jobs = F.symbols_jobs(rjobs, rm.CHAIN_HOLD)
    assert jobs["offset"][0] == 5 and jobs["n"][0] == rjobs["n_out"][0] and jobs["sps"][0] == rm.CHAIN_HOLD
    rec, views = F.symbols_host(whole, jobs)
    direct = sm.make_jobs([(0, 0, len(y), rm.CHAIN_HOLD, sm.ESTIMATE, 0.0)])
    rec_d, views_d = F.symbols_host(y.view(np.float32).reshape(-1, 2), direct)
    assert rec.tobytes() == rec_d.tobytes() and views[0].tobytes() == views_d[0].tobytes()
    want_rec, want = sm.symbols((whole, jobs))
    assert rec.tobytes() == want_rec.tobytes() and views[0].view(np.float32).tobytes() == want[0].tobytes()
    burst_job = jobs.copy()
    burst_job["offset"] += lag
    burst_job["n"] = rm.CHAIN_T
    brec, _ = F.symbols_host(whole, burst_job)
    v = F.symbols_derive(brec, rm.CHAIN_HOLD, 1.0)[0]
    print("chain: the preamble alone: n_sym %d tau %.4f lock4 %.3f lock2 %.3f" % (brec["n_sym"][0], brec["tau"][0], v["lock4"], v["lock2"]))
    assert brec["n_sym"][0] >= rm.CHAIN_SYMBOLS - 2 and v["lock4"] > 0.5 > v["lock2"]


def test_symbols_kernels_meet_their_resources(F):
    """-Rpass-analysis=kernel-resource-usage: every kernel of fosphor_symbols.hip has 0 bytes of scratch, at most 128 VGPRs and
    the static LDS that the header states for it"""
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
    ours = {k: v for k, v in found.items() if "k_sym_" in k}
    assert len(ours) == 4 and len(found) == 4, sorted(found)
    for name, res in ours.items():
        form = re.search(r"k_sym_(fold|time|pick|record)", name).group(1)
        print(form, res)
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 1 << 30) <= 128, (name, res)
        assert res.get("LDS Size") == F.SYMBOLS_LDS[form] == header_value("FOSPHOR_AMD_SYMBOLS_LDS_" + form.upper()), (name, res)
