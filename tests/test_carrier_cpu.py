"""Host side of include/fosphor_amd_carrier.h, no GPU: fosphor_amd_cossin_turns and fosphor_amd_carrier_host against the numpy
statement (tests/carrier_model.py), records and the whole output buffer bit for bit, on every input set the GPU tests use; the
refusals; carrier_jobs and carrier_derive; that a job's bytes depend on the job alone; that the two-lag estimator finds the carrier
of BPSK, QPSK and 8PSK bursts; the chain symbols_host -> carrier_host; and the compiled kernels' resources.

Bit for bit means tobytes(): signed zeros, subnormals and the one quiet NaN of each width included."""
import ctypes as C
import errno
import math
import os
import re
import subprocess

import numpy as np
import pytest

import carrier_model as cm
import symbols_model as sm
from _pkg import gr_fosphor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_carrier.hip")
HEADER = os.path.join(ROOT, "include", "fosphor_amd_carrier.h")
EINVAL = -errno.EINVAL
CASES = cm.cases()
SENTINEL = 0x5a5a5a5a
W = cm.RECORD_WORDS


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
    iq = cm.buffer(case)
    jobs = np.ascontiguousarray(case[1], cm.JOB_DTYPE)
    size = cm.capacity(jobs) if cap is None else max(cap, 0) + cm.GUARD
    buf = np.full((size + 1, 2), SENTINEL, np.uint32)
    rec = np.full((len(jobs) + 1) * W + 2, SENTINEL, np.uint32)
    ptr = {"iq": iq.ctypes.data, "jobs": jobs.ctypes.data, "records": rec.ctypes.data, "out": buf.ctypes.data}
    for k in null:
        ptr[k] = None
    if skew:
        ptr[skew[0]] += skew[1]
    rv = lib.fosphor_amd_carrier_host(ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["jobs"],
                                      len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"], size if cap is None else cap)
    return rv, rec, buf[:size]


def records_of(rec, n_jobs):
    assert np.all(rec[W * n_jobs:] == SENTINEL), "a record beyond the jobs' was written"
    return rec[:W * n_jobs].view(cm.RECORD_DTYPE)


def header_value(name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, open(HEADER).read())
    assert m, name
    return int(m.group(1))


def test_the_dtypes_mirror_the_structs(F):
    L = gr_fosphor_amd._lib
    assert cm.JOB_DTYPE.itemsize == 48 and C.sizeof(L.CarrierJob) == 48
    assert cm.RECORD_DTYPE.itemsize == 96 and C.sizeof(L.CarrierRecord) == 96
    assert F.CARRIER_JOB_DTYPE == cm.JOB_DTYPE and F.CARRIER_RECORD_DTYPE == cm.RECORD_DTYPE
    for dtype, struct in ((cm.JOB_DTYPE, L.CarrierJob), (cm.RECORD_DTYPE, L.CarrierRecord)):
        assert [(k, dtype.fields[k][1]) for k in dtype.names] == [(k, getattr(struct, k).offset) for k, _ in struct._fields_]
    assert F.CARRIER_STATS == cm.STATS and F.CARRIER_MODES == cm.MODES and F.CARRIER_STATUS == cm.STATUS
    assert len(cm.STATS) <= 10 == header_value_of(os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_pass.h"), "FOSPHOR_COUNTERS_MAX")
    assert (F.CARRIER_MAX_JOBS, F.CARRIER_MAX_LAG, F.CARRIER_BLOCK, F.CARRIER_TILE) == (cm.MAX_JOBS, cm.MAX_LAG, cm.BLOCK, cm.TILE)
    for name, want in (("MAX_JOBS", cm.MAX_JOBS), ("MAX_LAG", cm.MAX_LAG), ("BLOCK", cm.BLOCK), ("TILE", cm.TILE),
                       ("FREQ_FIXED", cm.FREQ_FIXED), ("PHASE_FIXED", cm.PHASE_FIXED), ("OK", cm.OK), ("NO_CARRIER", cm.NO_CARRIER),
                       ("LDS_LAG", F.CARRIER_LDS["lag"]), ("LDS_FREQ", F.CARRIER_LDS["freq"]), ("LDS_SUM", F.CARRIER_LDS["sum"]),
                       ("LDS_PHASE", F.CARRIER_LDS["phase"]), ("LDS_TURN", F.CARRIER_LDS["turn"])):
        assert header_value("FOSPHOR_AMD_CARRIER_" + name) == want, name
    for name in ("carrier", "carrier_host", "carrier_jobs", "carrier_derive", "carrier_stats", "cossin_turns"):
        assert hasattr(F, name), name


def header_value_of(path, name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, open(path).read())
    assert m, name
    return int(m.group(1))


def test_the_header_s_functions_are_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fosphor_amd_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["fosphor_amd_carrier", "fosphor_amd_carrier_cossin_turns", "fosphor_amd_carrier_cossin_turns_n",
                        "fosphor_amd_carrier_derive", "fosphor_amd_carrier_from_symbols", "fosphor_amd_carrier_host",
                        "fosphor_amd_carrier_stats", "fosphor_amd_cossin_turns"]
    lib = C.CDLL(gr_fosphor_amd.LIB_PATH)
    for name in declared:
        if name != "fosphor_amd_cossin_turns":						# the inline of the contract
            assert hasattr(lib, name), name
            assert name in gr_fosphor_amd._lib.SIGNATURES, name


def test_the_cases_hold_what_they_promise():
    small = [name for name in CASES if "table" not in name and "only" not in name]
    jobs = np.concatenate([CASES[name][1] for name in small])
    records = np.concatenate([cm.carrier(CASES[name])[0] for name in small])
    assert {(int(j["offset"]) & 1, int(j["out_offset"]) & 1) for j in jobs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    iq, lj = CASES["loads"]
    assert (lj["offset"] + lj["n"]).max() == len(iq), "a job ends on the buffer's last sample"
    assert {int(o) & 3 for o in lj["offset"]} == {0, 1, 2, 3}
    tj = CASES["tiles"][1]
    for M in cm.ORDERS:
        assert set(cm.TILE_COUNTS) <= set(tj["n"][tj["order"] == M]), M
    gj, gr = CASES["lag"][1], cm.carrier(CASES["lag"])[0]
    for L in cm.LAGS:
        mine = gj["lag"] == L
        assert {2 * L - 1, 2 * L, 64 + L, 65 + L, 256 + L, 257 + L, 4096 + L, 4097 + L} <= set(gj["n"][mine])
        assert gr["lag_used"][mine & (gj["n"] == 2 * L - 1)][0] == 1 and gr["lag_used"][mine & (gj["n"] == 2 * L)][0] == L
    mj = CASES["modes"][1]
    assert set(mj["mode"]) == {0, 1, 2, 3} and {0.5, -0.5, 0.0} <= set(mj["freq"][(mj["mode"] & 1) == 1])
    assert {0.5, -0.5} <= set(mj["phase"][(mj["mode"] & 2) == 2])
    nj, nr = CASES["numbers"][1], cm.carrier(CASES["numbers"])[0]
    assert (nr["status"] == cm.NO_CARRIER).sum() >= 8 and (nr["status"] == cm.OK).sum() >= 20
    zero = (nr["m2"] == 0.0) & (nr["status"] == cm.OK) & (nj["mode"] == 0)
    assert zero.any() and np.all(nr["freq"][zero] == 0.0) and np.all(nr["phase"][zero] == 0.0), "all-zero symbols: R = 0, Z = 0"
    assert np.isnan(nr["z_re"]).any() and np.isnan(nr["r1_re"]).any() and np.isinf(nr["mm"]).any()
    assert ((nr["m2"] > 0) & (nr["m2"] < 1e-70)).any(), "subnormal symbols"
    edge = (nj["lag"] == 64) & (nj["mode"] == 0)
    assert edge.sum() == 6 and np.all(np.abs(np.abs(nr["freq"][edge] * nr["order"][edge]) - 0.4999) < 2e-4)
    assert np.all(nr["lag_used"][edge] == 64), "g near +-0.5 with L = 64: k = +-32"
    mixed = CASES["mixed"][1]
    assert set(mixed["mode"]) == {0, 1, 2, 3} and set(mixed["order"]) == set(cm.ORDERS) and (mixed["n"] < 3).any()
    for name, modes in (("full_table", {0, 1, 2, 3}), ("only_fixed", {3})):
        full = CASES[name][1]
        assert len(full) == cm.MAX_JOBS and set(full["mode"]) == modes and (full["n"] == 0).sum() >= cm.MAX_JOBS // 11
        assert full["n"].max() <= 130 and set(full["order"]) == set(cm.ORDERS) and len(set(full["lag"])) == cm.MAX_LAG
    assert (records["status"] == cm.NO_CARRIER).sum() >= 8


def test_cossin_turns(lib, F):
    """the library's wrapper and the model bit for bit; exact at whole quarter turns; within 2e-15 of numpy's long-double cos and
    sin of 2 pi r (the header's derivation: x carries at most 1.8e-16 from its one product, nine Horner steps on values <= 1 add
    at most 1.1e-16 each; 1.8e-16 is what this test sees); NaN for what is not finite"""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "a long double with more bits than a double"
    rng = np.random.default_rng(44)
    sets = [rng.uniform(-4.0, 4.0, 1000000), rng.uniform(-1e6, 1e6, 100000), np.arange(-32, 33) / 16.0]
    two_pi = 8 * np.arctan(np.longdouble(1.0))
    worst = 0.0
    for t in sets:
        c, s = F.cossin_turns(t)
        mc, ms = cm.cossin_turns(t)
        assert c.tobytes() == mc.tobytes() and s.tobytes() == ms.tobytes()
        r = t - np.floor(t)					# exact for these t, or the rule's own rounding, which the error is measured behind
        err = max(np.abs(c - np.cos(two_pi * r.astype(np.longdouble))).max(), np.abs(s - np.sin(two_pi * r.astype(np.longdouble))).max())
        worst = max(worst, float(err))
        assert err <= 2e-15
    print("cossin_turns against long double numpy: %.3g at worst" % worst)
    bits = lambda v: np.float64(v).tobytes()
    for t, wc, ws in ((0.0, 1.0, 0.0), (-0.0, 1.0, 0.0), (0.25, -0.0, 1.0), (0.5, -1.0, -0.0), (0.75, 0.0, -1.0), (1.0, 1.0, 0.0),
                      (-0.25, 0.0, -1.0), (-0.5, -1.0, -0.0), (-0.75, -0.0, 1.0), (-1.0, 1.0, 0.0), (2.0, 1.0, 0.0), (-1e-20, 1.0, 0.0),
                      (1e6 + 0.25, -0.0, 1.0)):
        c, s = C.c_double(), C.c_double()
        assert lib.fosphor_amd_carrier_cossin_turns(t, C.byref(c), C.byref(s)) == 0
        assert bits(c.value) == bits(wc) and bits(s.value) == bits(ws), (t, c.value, s.value)
    c, s = F.cossin_turns([0.125, 0.375, 0.9375])
    assert abs(c[0] - math.sqrt(0.5)) < 2e-16 and abs(s[0] - math.sqrt(0.5)) < 2e-16 and s[1] > 0 > c[1] and s[2] < 0 < c[2]
    c, s = F.cossin_turns([np.nan, np.inf, -np.inf])
    assert np.all(c.view(np.uint64) == 0x7ff8000000000000) and np.all(s.view(np.uint64) == 0x7ff8000000000000)
    assert F.cossin_turns(np.zeros((2, 3)))[0].shape == (2, 3) and F.cossin_turns([])[0].shape == (0,)
    one = C.c_double()
    assert lib.fosphor_amd_carrier_cossin_turns(0.0, None, C.byref(one)) == EINVAL
    assert lib.fosphor_amd_carrier_cossin_turns(0.0, C.byref(one), None) == EINVAL
    buf = np.zeros(4)
    for t, n, pc, ps in ((None, 4, buf.ctypes.data, buf.ctypes.data), (buf.ctypes.data, -1, buf.ctypes.data, buf.ctypes.data),
                         (buf.ctypes.data, 4, None, buf.ctypes.data), (buf.ctypes.data, 4, buf.ctypes.data, None)):
        assert lib.fosphor_amd_carrier_cossin_turns_n(t, n, pc, ps) == EINVAL


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_model(lib, F, name):
    case = CASES[name]
    jobs = case[1]
    rv, rec, got = host(lib, case)
    assert rv == 0
    want_rec, want = cm.image(case, SENTINEL, key=name)
    got_rec = records_of(rec, len(jobs))
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical"
    for i in np.flatnonzero((got != want).any(1))[:10]:
        print("sample %d got %s want %s" % (i, got[i], want[i]))
    assert got.tobytes() == want.tobytes(), "symbols bit-identical, every other sample at the sentinel"
    records, views = F.carrier_host(cm.buffer(case), jobs)
    assert records.tobytes() == want_rec.tobytes(), "the Python front end gives the same records"
    for j, r, v in zip(jobs, records, views):
        at = int(j["out_offset"])
        assert len(v) == (j["n"] if r["status"] == cm.OK else 0) and v.view(np.uint32).tobytes() == want[at:at + len(v)].tobytes()


def test_a_job_alone_among_others_and_shuffled(F):
    """a record and a job's symbols depend on their job alone"""
    iq, jobs = CASES["mixed"]
    among_rec, among = F.carrier_host(iq, jobs)
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = F.carrier_host(iq, jobs[order])
    assert shuffled_rec.tobytes() == among_rec[order].tobytes()
    for k, i in enumerate(order):
        assert shuffled[k].tobytes() == among[i].tobytes()
    for i in (0, 1, 2, 3, 4, len(jobs) - 1):
        alone_rec, alone = F.carrier_host(iq, jobs[i:i + 1])
        assert alone_rec[0].tobytes() == among_rec[i].tobytes() and alone[0].tobytes() == among[i].tobytes(), i


EINVAL_OK = (0, 0, 100, 4, cm.FREQ_FIXED | cm.PHASE_FIXED, 16, 0.25, 0.25)


def einval_rows(cap):
    """one job each that rule 8 refuses, over 3000 samples (the rows of tests/test_gpu_carrier.py)"""
    def one(**kw):
        row = dict(zip(("offset", "out_offset", "n", "order", "mode", "lag", "freq", "phase"), EINVAL_OK))
        row.update(kw)
        return tuple(row.values())

    return [one(offset=-1), one(out_offset=-1), one(n=-1), one(offset=2901), one(offset=3001, n=0), one(offset=2 ** 62, n=2 ** 31 - 1),
            one(offset=2 ** 62), one(out_offset=cap + 1, n=0), one(out_offset=2 ** 62), one(out_offset=cap - 99),
            one(order=0), one(order=1), one(order=3), one(order=6), one(order=16), one(order=-4),
            one(lag=0), one(lag=-1), one(lag=65), one(mode=4), one(mode=7), one(mode=-1),
            one(mode=cm.PHASE_FIXED), one(mode=cm.FREQ_FIXED), one(mode=0), one(mode=0, phase=0.0), one(mode=0, freq=0.0),
            one(freq=np.nan), one(freq=np.inf), one(freq=-np.inf), one(freq=0.5000001), one(freq=-0.5000001),
            one(phase=np.nan), one(phase=np.inf), one(phase=-np.inf), one(phase=0.5000001), one(phase=-0.5000001)]


def test_einval_table(lib):
    """each refused call leaves every sample and every record at the sentinel"""
    iq = cm.psk(3000, 4, 0.01, 0.1, 91, 30.0)
    #        offset out  n   order mode lag freq phase
    good = [(0, 5, 500, 4, cm.ESTIMATE, 16, 0.0, 0.0), (2990, 0, 5, 2, cm.FREQ_FIXED | cm.PHASE_FIXED, 1, 0.5, -0.5),
            (3000, 505, 0, 8, cm.ESTIMATE, 64, 0.0, 0.0), (1, 510, 2999, 8, cm.PHASE_FIXED, 64, 0.0, 0.25)]
    cap = 510 + 2999
    rv, rec, out = host(lib, (iq, cm.make_jobs(good)), cap=cap)
    assert rv == 0 and np.all(out[cap:] == SENTINEL) and np.all(out[505:510] == SENTINEL) and np.all(out[0:5] != SENTINEL)
    assert np.all(records_of(rec, 4).view(np.uint32)[:, None] != SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        rv, rec, out = host(lib, (iq, cm.make_jobs(rows)), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL), "nothing is written"

    for what in ("iq", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (cm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=2999); refused(good, cap=-1); refused(good, cap=cap - 1)
    for row in einval_rows(cap):
        refused([row])
    refused([EINVAL_OK, EINVAL_OK[:1] + (99,) + EINVAL_OK[2:]])			# [0, 100) and [99, 199): one sample shared
    refused([EINVAL_OK[:1] + (200,) + EINVAL_OK[2:], (0, 8, 800, 4, 0, 16, 0.0, 0.0)])	# [200, 300) and [8, 808), in descending order
    for name in ("iq", "records", "out"):
        refused(good, skew=(name, 4))
    # the values at the edge of what is taken: +-0.5, -0.0 without the bit
    edge = cm.make_jobs([(0, 0, 100, 2, 3, 1, 0.5, -0.5), (0, 100, 100, 8, 3, 64, -0.5, 0.5), (0, 200, 100, 4, 0, 16, -0.0, -0.0)])
    assert host(lib, (iq, edge), cap=cap)[0] == 0
    # the last jobs that still fit; outputs that touch; jobs without a symbol anywhere inside
    last = cm.make_jobs([(0, 0, 100, 4, 0, 16, 0.0, 0.0), (0, 100, 100, 2, 0, 64, 0.0, 0.0), (2900, cap - 100, 100, 4, 3, 1, -0.5, 0.5),
                         (3000, cap, 0, 8, 0, 1, 0.0, 0.0), (5, 50, 0, 8, 0, 1, 0.0, 0.0)])
    rv, rec, out = host(lib, (iq, last), cap=cap)
    want_rec, want = cm.image((iq, last), SENTINEL)
    assert rv == 0 and records_of(rec, 5).tobytes() == want_rec.tobytes() and out[:cap].tobytes() == want[:cap].tobytes()
    many = cm.make_jobs([(0, 100 * i, 100, 4, 0, 16, 0.0, 0.0) for i in range(cm.MAX_JOBS)])
    assert host(lib, (iq, many))[0] == 0
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    rec = np.full(W, SENTINEL, np.uint32)
    out = np.full(256, SENTINEL, np.uint32)
    job = cm.make_jobs([EINVAL_OK])
    assert lib.fosphor_amd_carrier(None, iq.ctypes.data, 3000, job.ctypes.data, 1, rec.ctypes.data, out.ctypes.data, 128) == EINVAL
    assert np.all(rec == SENTINEL) and np.all(out == SENTINEL)
    assert lib.fosphor_amd_carrier_stats(None, None) == EINVAL


def test_jobs_and_derive(lib, F):
    sj = sm.make_jobs([(0, 7, 400, 4, sm.ESTIMATE, 0.0), (400, 1000, 40, 4, sm.FIXED, 0.5), (0, 2000, 3, 4, sm.ESTIMATE, 0.0)])
    sr = np.zeros(3, sm.RECORD_DTYPE)
    sr["n_sym"] = (99, 9, 0)
    jobs = F.carrier_jobs(sj, sr, 4)
    assert jobs.dtype == cm.JOB_DTYPE and list(jobs["offset"]) == [7, 1000, 2000] and list(jobs["n"]) == [99, 9, 0]
    assert list(jobs["out_offset"]) == [0, 99, 108] and set(jobs["order"]) == {4} and set(jobs["mode"]) == {0} and set(jobs["lag"]) == {16}
    assert not jobs["freq"].any() and not jobs["phase"].any()
    jobs = F.carrier_jobs(sj, sr, 8, mode="fixed", lag=3, freq=-0.25, phase=0.5)
    assert set(jobs["mode"]) == {3} and set(jobs["lag"]) == {3} and set(jobs["freq"]) == {-0.25} and set(jobs["phase"]) == {0.5}
    job = gr_fosphor_amd._lib.CarrierJob()
    job.out_offset = 99
    make = lib.fosphor_amd_carrier_from_symbols
    assert make(sj[:1].tobytes(), sr[:1].tobytes(), 2, cm.PHASE_FIXED, 64, 0.0, -0.5, C.byref(job)) == 0
    assert (job.offset, job.out_offset, job.n, job.order, job.mode, job.lag, job.freq, job.phase) == (7, 0, 99, 2, 2, 64, 0.0, -0.5)
    for bad_job, bad_rec, order, mode, lag, freq, phase in ((dict(out_offset=-1), {}, 4, 0, 16, 0.0, 0.0), ({}, dict(n_sym=-1), 4, 0, 16, 0.0, 0.0),
                                                            ({}, {}, 3, 0, 16, 0.0, 0.0), ({}, {}, 4, 4, 16, 0.0, 0.0), ({}, {}, 4, 0, 0, 0.0, 0.0),
                                                            ({}, {}, 4, 0, 65, 0.0, 0.0), ({}, {}, 4, 0, 16, 0.1, 0.0), ({}, {}, 4, 0, 16, 0.0, 0.1),
                                                            ({}, {}, 4, 1, 16, 0.6, 0.0), ({}, {}, 4, 2, 16, 0.0, math.nan)):
        s, r = sj[:1].copy(), sr[:1].copy()
        for k, v in bad_job.items():
            s[k] = v
        for k, v in bad_rec.items():
            r[k] = v
        assert make(s.tobytes(), r.tobytes(), order, mode, lag, freq, phase, C.byref(job)) == EINVAL, (bad_job, bad_rec, order, mode, lag)
    assert make(None, sr[:1].tobytes(), 4, 0, 16, 0.0, 0.0, C.byref(job)) == EINVAL
    assert make(sj[:1].tobytes(), None, 4, 0, 16, 0.0, 0.0, C.byref(job)) == EINVAL
    assert make(sj[:1].tobytes(), sr[:1].tobytes(), 4, 0, 16, 0.0, 0.0, None) == EINVAL
    with pytest.raises(ValueError):
        F.carrier_jobs(sj, sr, 4, mode="track")
    with pytest.raises(ValueError):
        F.carrier_jobs(sj, sr[:2], 4)
    # records built by hand
    r = np.zeros(1, cm.RECORD_DTYPE)
    r["n"], r["order"], r["lag_used"], r["freq"], r["phase"] = 100, 4, 16, 0.01, 0.125
    r["r1_re"], r["r1_im"], r["rl_re"], r["rl_im"] = 0.0, 99.0, -42.0, 0.0
    r["z_re"], r["z_im"], r["m2"], r["mm"] = 30.0, -40.0, 100.0, 100.0
    v = F.carrier_derive(r, 2400.0)[0]
    assert set(v) == set(F.CARRIER_VALUES)
    assert v["freq_hz"] == 24.0 and abs(v["phase_rad"] - math.pi / 4) < 1e-15 and v["sym_power"] == 1.0 and v["lock"] == 0.5
    assert abs(v["lag_lock"] - 0.99) < 1e-15 and abs(v["lagl_lock"] - 0.42) < 1e-15
    r["lag_used"] = 1
    assert F.carrier_derive(r, 2400.0)[0]["lagl_lock"] == 0.0
    for field, bad in (("n", 0), ("status", cm.NO_CARRIER)):
        x = r.copy()
        x[field] = bad
        assert all(y == 0.0 for y in F.carrier_derive(x, 2400.0)[0].values()), field
    for field in ("freq", "phase", "r1_re", "rl_im", "z_re", "m2", "mm"):
        for bad in (0.0, -1.0, math.inf, math.nan):
            x = r.copy()
            x[field] = bad
            assert all(math.isfinite(y) for y in F.carrier_derive(x, 2400.0)[0].values()), (field, bad)
    vals = gr_fosphor_amd._lib.CarrierValues()
    for rate in (0.0, -1.0, math.inf, math.nan):
        assert lib.fosphor_amd_carrier_derive(r.tobytes(), rate, C.byref(vals)) == EINVAL
    assert lib.fosphor_amd_carrier_derive(None, 1.0, C.byref(vals)) == EINVAL
    assert lib.fosphor_amd_carrier_derive(r.tobytes(), 1.0, None) == EINVAL


# ---- function ---------------------------------------------------------------------------------------------------------------------

N_SYMBOLS, BURSTS, LAG = 512, 40, 16
ROWS = [(M, snr) for snr in (None, 30.0, 20.0) for M in cm.ORDERS if not (M == 8 and snr == 20.0)]
# (M, snr) -> bars on |f - f0| in turns per symbol, on the phase error at mid-burst in turns modulo 1 / M, and on 1 - lock: twice
# the worst that float64_statement() shows over the BURSTS bursts of the row (the docstring of the test has the observed values)
BARS = {(2, None): (9.2e-10, 1.4e-8, 7.3e-13), (4, None): (4.6e-10, 6.6e-9, 7.3e-13), (8, None): (2.3e-10, 3.8e-9, 7.3e-13),
        (2, 30.0): (1.77e-5, 7.5e-4, 2.4e-3), (4, 30.0): (1.64e-5, 7.8e-4, 9.5e-3), (8, 30.0): (1.68e-5, 8.0e-4, 3.9e-2),
        (2, 20.0): (5.7e-5, 3.1e-3, 2.5e-2), (4, 20.0): (6.5e-5, 2.3e-3, 9.5e-2)}


def bursts_of(M, snr):
    """BURSTS seeded bursts of N_SYMBOLS unit symbols: (float32 [n][2], f0, theta0)"""
    rng = np.random.default_rng(1000 * M + (0 if snr is None else int(snr)))
    for b in range(BURSTS):
        f0, th0 = rng.uniform(-0.4, 0.4) / M, rng.uniform(-0.45, 0.45) / M
        yield cm.psk(N_SYMBOLS, M, f0, th0, int(rng.integers(1 << 30)), snr), f0, th0


def float64_statement(y, M, L):
    """rules 1 to 5 in plain float64 numpy, no pinned order and numpy's own power, angle, sine and cosine -> (f, theta, lock).  The
    three angles are float32, as the rules have them (fosphor_amd_atan2_turns returns one): that rounding, 2^-25 of a turn over L M
    at most, is the rules' own and sets the noiseless figures"""
    z = y[:, 0].astype(np.float64) + 1j * y[:, 1].astype(np.float64)
    p = z ** M
    turns = lambda v: np.float64(np.float32(np.angle(v) / (2.0 * np.pi)))
    Le = L if len(z) >= 2 * L else 1
    g = turns((p[1:] * p[:-1].conj()).sum())
    if Le > 1:
        aL = turns((p[Le:] * p[:-Le].conj()).sum())
        g = (aL + np.floor(Le * g - aL + 0.5)) / Le
    Z = (p * np.exp(-2j * np.pi * g * np.arange(len(z)))).sum()
    return g / M, turns(Z) / M, abs(Z) / (np.abs(z) ** M).sum()


def wrapped(d, period):
    return abs((d + 0.5 * period) % period - 0.5 * period)


def errors(f, theta, lock, f0, th0, M):
    mid = 0.5 * (N_SYMBOLS - 1)
    return abs(f - f0), wrapped((theta + f * mid) - (th0 + f0 * mid), 1.0 / M), 1.0 - lock


def worst_of(F, M, snr, L):
    """the worst errors over the row's bursts -> (of the host statement, of the float64 statement), each (f, phase, 1 - lock)"""
    host_worst, f64_worst = np.zeros(3), np.zeros(3)
    for y, f0, th0 in bursts_of(M, snr):
        rec, _ = F.carrier_host(y, cm.make_jobs([(0, 0, len(y), M, cm.ESTIMATE, L, 0.0, 0.0)]))
        assert rec["status"][0] == cm.OK and rec["lag_used"][0] == L
        lock = F.carrier_derive(rec, 1.0)[0]["lock"]
        host_worst = np.maximum(host_worst, errors(rec["freq"][0], rec["phase"][0], lock, f0, th0, M))
        f64_worst = np.maximum(f64_worst, errors(*float64_statement(y, M, L), f0, th0, M))
    return host_worst, f64_worst


@pytest.mark.parametrize("M,snr", ROWS)
def test_the_estimator_finds_the_carrier(F, M, snr):
    """BURSTS bursts of N_SYMBOLS unit PSK symbols, f0 uniform in +-0.4 / M and theta0 in +-0.45 / M, L = 16: |f - f0|, the phase
    error at mid-burst modulo 1 / M and 1 - lock stay within BARS for the host statement and for a plain float64 statement of the
    same rules alike.  The bars are twice the worst of the float64 statement.  Observed, the worst over the 40 bursts of a row,
    host statement (float64 statement):
      M  SNR        |f - f0|               phase at mid-burst     1 - lock
      2  none       4.60e-10 (4.60e-10)    6.94e-9 (6.94e-9)      3.65e-13 (3.64e-13)
      4  none       2.28e-10 (2.28e-10)    3.29e-9 (3.29e-9)      3.61e-13 (3.62e-13)
      8  none       1.14e-10 (1.14e-10)    1.87e-9 (1.87e-9)      3.63e-13 (3.63e-13)
      2  30 dB      8.81e-6  (8.81e-6)     3.73e-4 (3.73e-4)      1.17e-3  (1.17e-3)
      4  30 dB      8.18e-6  (8.18e-6)     3.87e-4 (3.87e-4)      4.71e-3  (4.71e-3)
      8  30 dB      8.37e-6  (8.37e-6)     3.98e-4 (3.98e-4)      1.93e-2  (1.93e-2)
      2  20 dB      2.81e-5  (2.81e-5)     1.53e-3 (1.53e-3)      1.22e-2  (1.22e-2)
      4  20 dB      3.25e-5  (3.25e-5)     1.12e-3 (1.12e-3)      4.71e-2  (4.71e-2)
    Without noise what is left is the float32 of the three angles.  8PSK at 20 dB is not a row: the eighth power is below its
    threshold there in the float64 statement too."""
    host_worst, f64_worst = worst_of(F, M, snr, LAG)
    print("M %d snr %s: |f - f0| %.3g (%.3g) phase %.3g (%.3g) 1 - lock %.3g (%.3g)" % (
        M, snr, host_worst[0], f64_worst[0], host_worst[1], f64_worst[1], host_worst[2], f64_worst[2]))
    bars = BARS[(M, snr)]
    for k, what in enumerate(("|f - f0|", "the phase at mid-burst", "1 - lock")):
        assert f64_worst[k] <= bars[k], ("the float64 statement", what)
        assert host_worst[k] <= bars[k], ("the host statement", what)


def test_the_long_lag_beats_lag_one(F):
    """QPSK at 20 dB: with L = 1 the frequency is off by up to a few 1e-4 turns per symbol, which unwinds the phase sum over 512
    symbols (lock near 0); with L = 16 it is 16 times finer.  That is the reason the lag exists.  Observed, the worst over the 40 bursts: |f - f0| 3.25e-5 and
    1 - lock 0.047 with L = 16, 4.02e-4 and 0.81 with L = 1"""
    long_worst, _ = worst_of(F, 4, 20.0, LAG)
    worst1 = np.zeros(3)
    for y, f0, th0 in bursts_of(4, 20.0):
        rec, _ = F.carrier_host(y, cm.make_jobs([(0, 0, len(y), 4, cm.ESTIMATE, 1, 0.0, 0.0)]))
        worst1 = np.maximum(worst1, errors(rec["freq"][0], rec["phase"][0], F.carrier_derive(rec, 1.0)[0]["lock"], f0, th0, 4))
    print("QPSK 20 dB: L = 16 |f - f0| %.3g, 1 - lock %.3g; L = 1 |f - f0| %.3g, 1 - lock %.3g" % (long_worst[0], long_worst[2], worst1[0], worst1[2]))
    assert long_worst[0] < worst1[0] and long_worst[2] < worst1[2]
    assert long_worst[0] <= BARS[(4, 20.0)][0] < worst1[0]


def test_chain_on_the_host(lib, F):
    """the QPSK preamble of resample_model's small sc16 stream through fosphor_amd_extract_host, fosphor_amd_resample_host,
    fosphor_amd_symbols_host and, by the jobs that carrier_jobs() makes, fosphor_amd_carrier_host at M = 4: the model's bytes; over
    the preamble alone the carrier locks; and the derotated output, fed back, has no frequency and no phase left (within the
    bars of the noiseless QPSK row)"""
    import resample_model as rm
    raw, ejobs, _, lag = rm.chain_case()
    taps = F.extract_design(rm.CHAIN_DECIM, rm.CHAIN_TAPS, 0.8)
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    x = np.zeros((cap, 2), np.float32)
    assert lib.fosphor_amd_extract_host(raw.ctypes.data, len(raw), 2, ejobs.ctypes.data, len(ejobs), taps.ctypes.data, len(taps),
                                        x.ctypes.data, cap) == 0
    rtaps = F.resample_design(rm.CHAIN_UP, rm.CHAIN_DOWN, rm.CHAIN_BRANCH)
    rjobs = F.resample_jobs(ejobs, rm.CHAIN_UP, rm.CHAIN_DOWN, len(rtaps))
    y = F.resample_host(x, rjobs, rtaps)[0]
    sjobs = np.concatenate([F.symbols_jobs(rjobs, rm.CHAIN_HOLD), F.symbols_jobs(rjobs, rm.CHAIN_HOLD)])
    sjobs["offset"][1] += lag						# the preamble alone
    sjobs["n"][1] = rm.CHAIN_T
    sjobs["out_offset"][1] = sm.job_max_out(sjobs[0]) + sm.GUARD
    srec, sviews = F.symbols_host(y, sjobs)
    s = np.zeros((sm.capacity(sjobs), 2), np.float32)
    for j, v in zip(sjobs, sviews):
        s[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v.view(np.float32).reshape(-1, 2)
    jobs = F.carrier_jobs(sjobs, srec, 4, lag=8)
    assert list(jobs["offset"]) == list(sjobs["out_offset"]) and list(jobs["n"]) == list(srec["n_sym"]) and jobs["n"][1] >= rm.CHAIN_SYMBOLS - 2
    rec, views = F.carrier_host(s, jobs)
    want_rec, want = cm.carrier((s, jobs))
    assert rec.tobytes() == want_rec.tobytes()
    for v, w in zip(views, want):
        assert v.view(np.float32).tobytes() == w.tobytes()
    val = F.carrier_derive(rec, 1.0)[1]
    print("chain: the preamble alone: n %d freq %.3g phase %.4f lock %.3f" % (rec["n"][1], rec["freq"][1], rec["phase"][1], val["lock"]))
    assert rec["status"][1] == cm.OK and val["lock"] > 0.5
    again, _ = F.carrier_host(views[1], cm.make_jobs([(0, 0, len(views[1]), 4, cm.ESTIMATE, 8, 0.0, 0.0)]))
    print("chain: fed back: freq %.3g phase %.3g" % (again["freq"][0], again["phase"][0]))
    assert abs(again["freq"][0]) <= BARS[(4, None)][0] and abs(again["phase"][0]) <= BARS[(4, None)][1]


def test_carrier_kernels_meet_their_resources(F):
    """-Rpass-analysis=kernel-resource-usage: every kernel of fosphor_carrier.hip has 0 bytes of scratch, at most 128 VGPRs and
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
    ours = {k: v for k, v in found.items() if "k_car_" in k}
    assert len(ours) == 5 and len(found) == 5, sorted(found)
    for name, res in ours.items():
        form = re.search(r"k_car_(lag|freq|sum|phase|turn)", name).group(1)
        print(form, res)
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 1 << 30) <= 128, (name, res)
        assert res.get("LDS Size") == F.CARRIER_LDS[form] == header_value("FOSPHOR_AMD_CARRIER_LDS_" + form.upper()), (name, res)
