"""Host side of include/fosphor_amd_correlate.h, no GPU: fosphor_amd_correlate_host against the numpy statement
(tests/correlate_model.py), records and the whole output buffer bit for bit, on every input set the GPU tests use; the cut rule;
the refusals; correlate_n_out, correlate_from_extract and correlate_derive; the chain extract_host -> correlate_host.

Bit for bit means tobytes(): signed zeros, subnormals and the one quiet NaN of each width included."""
import ctypes as C
import errno
import math

import numpy as np
import pytest

import correlate_model as cm
from _pkg import gr_fosphor_amd

EINVAL = -errno.EINVAL
CASES = cm.cases()
SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def lib():
    return gr_fosphor_amd.load()


@pytest.fixture(scope="module")
def F():
    gr_fosphor_amd.load()
    return gr_fosphor_amd.Fosphor


def host(lib, case, n_samples=None, n_tpl=None, n_jobs=None, cap=None, null=(), skew=None):
    """-> (return value, records as bytes [n_jobs + 1][64], the whole output buffer as uint32), both sentinel-filled before the
    call.  cap: out_capacity, GUARD floats of the buffer lie behind it; skew: (pointer name, bytes)"""
    iq, tpl = cm.buffers(case)
    jobs = np.ascontiguousarray(case[2], cm.JOB_DTYPE)
    size = cm.capacity(jobs) if cap is None else max(cap, 0) + cm.GUARD
    buf = np.full(size + 1, SENTINEL, np.uint32)
    rec = np.full((len(jobs) + 1) * 16 + 2, SENTINEL, np.uint32)
    ptr = {"iq": (iq if iq.size else np.zeros((1, 2), np.float32)).ctypes.data, "tpl": tpl.ctypes.data, "jobs": jobs.ctypes.data,
           "records": rec.ctypes.data, "out": buf.ctypes.data}
    keep = (iq, tpl)						# the arrays behind the pointers live until the call returns
    for k in null:
        ptr[k] = None
    if skew:
        ptr[skew[0]] += skew[1]
    rv = lib.fosphor_amd_correlate_host(ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["tpl"],
                                        len(tpl) if n_tpl is None else n_tpl, ptr["jobs"], len(jobs) if n_jobs is None else n_jobs,
                                        ptr["records"], ptr["out"], size if cap is None else cap)
    del keep
    return rv, rec, buf[:size]


def records_of(rec, n_jobs):
    assert np.all(rec[16 * n_jobs:] == SENTINEL), "a record beyond the jobs' was written"
    return rec[:16 * n_jobs].view(cm.RECORD_DTYPE)


def explain(got, want):
    for i in [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()][:6]:
        print("job %d got %s want %s" % (i, got[i], want[i]))


def test_the_dtypes_mirror_the_structs(F):
    L = gr_fosphor_amd._lib
    assert cm.JOB_DTYPE.itemsize == 40 and C.sizeof(L.CorrelateJob) == 40
    assert cm.RECORD_DTYPE.itemsize == 64 and C.sizeof(L.CorrelateRecord) == 64
    assert F.CORRELATE_JOB_DTYPE == cm.JOB_DTYPE and F.CORRELATE_RECORD_DTYPE == cm.RECORD_DTYPE
    for dtype, struct in ((cm.JOB_DTYPE, L.CorrelateJob), (cm.RECORD_DTYPE, L.CorrelateRecord)):
        assert [(k, dtype.fields[k][1]) for k in dtype.names] == [(k, getattr(struct, k).offset) for k, _ in struct._fields_]
    assert F.CORRELATE_STATS == cm.STATS and F.CORRELATE_TRACES == cm.TRACES
    assert (F.CORRELATE_MAX_JOBS, F.CORRELATE_MAX_TPL, F.CORRELATE_TILE) == (cm.MAX_JOBS, cm.MAX_TPL, cm.TILE)


def test_the_cases_hold_what_they_promise():
    """the seams are in the sets, and no set is larger than the model runs in seconds"""
    for name, case in CASES.items():
        assert cm.macs(case[2]) <= cm.MAX_MACS, name
    assert cm.macs(cm.cut_case()[0][2]) <= cm.MAX_MACS
    jobs = np.concatenate([c[2] for c in CASES.values()])
    lags = {cm.n_lags(int(j["n"]), int(j["tpl_len"])) for j in jobs}
    assert set(cm.TS) <= set(jobs["tpl_len"])
    assert {0, 1, 255, 256, 257, 1023, 1024, 1025, 2 * cm.TILE + 1, 3 * cm.TILE + 5} <= lags
    assert {0, 1, 2, 3} <= set(jobs["offset"]) and {0, 1, 2, 3} <= set(jobs["tpl_offset"])
    assert {(int(j["offset"]) & 1, int(j["tpl_offset"]) & 1) for j in jobs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    traced = jobs[jobs["trace"] != cm.NONE]
    assert {int(o) & 1 for o in traced["out_offset"]} == {0, 1}
    iq, _, lj = CASES["lag_counts"]
    assert (lj["offset"] + lj["n"]).max() == len(iq), "a job ends on the buffer's last sample"
    mixed = CASES["mixed257"][2]
    assert len(mixed) == 257 and set(mixed["trace"]) == {cm.NONE, cm.RHO, cm.C}
    assert max(cm.n_lags(int(j["n"]), int(j["tpl_len"])) for j in mixed) > cm.TILE


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_model(lib, F, name):
    case = CASES[name]
    jobs = case[2]
    rv, rec, got = host(lib, case)
    assert rv == 0
    want_rec, want = cm.image(case, SENTINEL)
    got_rec = records_of(rec, len(jobs))
    explain(got_rec, want_rec)
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical"
    for i in np.flatnonzero(got != want)[:10]:
        print("float %d got %08x want %08x" % (i, got[i], want[i]))
    assert got.tobytes() == want.tobytes(), "traces bit-identical, every other float at the sentinel"
    iq, tpl = cm.buffers(case)
    records, views = F.correlate_host(iq, jobs, tpl)
    assert records.tobytes() == want_rec.tobytes(), "the Python front end gives the same records"
    for j, v, w in zip(jobs, views, cm.correlate(case)[1]):
        if j["trace"] == cm.NONE:
            assert v is None
        else:
            assert v.dtype == (np.float32 if j["trace"] == cm.RHO else np.complex64) and v.tobytes() == w.tobytes()
    r = want_rec
    if name == "tie":
        rho = cm.correlate(case)[1][0]
        second = cm.TIE_AT + cm.TILE + 37
        assert rho[cm.TIE_AT].tobytes() == rho[second].tobytes() and cm.TIE_AT // cm.TILE != second // cm.TILE
        assert list(r["peak_lag"]) == [cm.TIE_AT, cm.TIE_AT - 60, cm.TIE_AT - 1, second - cm.TIE_AT - 7], "the smaller lag wins the tie"
        assert r["peak_c_re"][0] == r["peak_energy"][0] == r["tpl_energy"][0] and r["peak_c_im"][0] == 0.0
    if name == "edges":
        on = cm.edges_pattern()
        runs = int(on[0]) + int((on[1:] & ~on[:-1]).sum())
        assert on[cm.TILE - 1] and on[cm.TILE] and not on[cm.TILE - 2] and not on[cm.TILE + 1]
        assert (r["n_above"][0], r["first_above"][0], r["last_above"][0], r["n_edges"][0]) == (on.sum(), 0, len(on) - 1, runs)
        assert r["n_edges"][1] == runs and r["n_edges"][2] == runs - 1, "the job from sample 1 on does not see lag 0's run"
        assert (r["n_above"][4], r["n_edges"][4]) == (len(on), 1) and (r["n_above"][5], r["n_edges"][5]) == (len(on), 1)
        assert (r["n_above"][6], r["first_above"][6], r["last_above"][6], r["n_edges"][6]) == (0, -1, -1, 0)
        assert (r["n_above"][7], r["n_edges"][7]) == (2, 1)
    if name == "silence":
        assert r["peak_rho"][0] == 0.0 and r["peak_lag"][0] == 0 and r["n_above"][0] == r["n_lags"][0] and r["n_edges"][0] == 1
        assert r["tpl_energy"][1] == 0.0 and r["tpl_energy"][2] == 0.0 and r["peak_rho"][2] == 0.0 and r["n_above"][2] == 0
        assert r["n_above"][4] == r["n_lags"][4], "rho 0 is above a threshold of -0"
    if name == "nonfinite":
        rho = cm.correlate(case)[1][0]
        assert np.isnan(rho[285:301]).all() and np.isfinite(rho[[284, 301]]).all() and 0 <= r["peak_lag"][0] and r["peak_rho"][0] > 0.1
        for i in (3, 4, 5, 6):
            assert r["peak_lag"][i] == -1 and r["peak_rho"][i] == 0.0 and r["n_above"][i] == 0 and r["peak_c_re"][i] == 0.0, i
        assert np.isnan(r["tpl_energy"][3]) and r["tpl_energy"][4] == np.inf and r["n_lags"][7] == 0 and np.isnan(r["tpl_energy"][7])
        assert r["tpl_energy"][3:4].view(np.uint64)[0] == 0x7ff8000000000000


def test_the_cut_rule(lib):
    """rule 4: a job gives, bit for bit, the trace and the per-lag facts of the two jobs it is cut into at lag c"""
    case, triples = cm.cut_case()
    jobs = case[2]
    rv, rec, got = host(lib, case)
    assert rv == 0
    want_rec, want = cm.image(case, SENTINEL)
    records = records_of(rec, len(jobs))
    assert records.tobytes() == want_rec.tobytes() and got.tobytes() == want.tobytes()
    traces = [got[int(j["out_offset"]):int(j["out_offset"]) + cm.n_out(int(j["trace"]), int(j["n"]), int(j["tpl_len"]))] for j in jobs]
    cm.assert_cut(records, traces, jobs, triples)
    assert {(int(jobs["tpl_len"][w]), int(jobs["trace"][w])) for w, _, _, _ in triples} == set(cm.CUT_FORMS)
    assert any(records[w]["n_edges"] > 10 for w, _, _, _ in triples), "the thresholds cut through the traces"


def test_n_out_from_extract(lib, F):
    for trace, name in ((cm.NONE, "none"), (cm.RHO, "rho"), (cm.C, "c")):
        for n in (0, 1, 2, 255, 256, 257, 1024, 2 ** 29):
            for T in (1, 2, 3, 255, 256, 1024):
                assert lib.fosphor_amd_correlate_n_out(trace, n, T) == cm.n_out(trace, n, T) == F.correlate_n_out(name, n, T)
    assert lib.fosphor_amd_correlate_n_out(cm.RHO, 2 ** 31 - 1, 1) == 2 ** 31 - 1
    for trace, n, T in ((3, 1, 1), (-1, 1, 1), (0, -1, 1), (0, 1, 0), (0, 1, 1025), (cm.C, 2 ** 31 - 1, 1)):
        assert lib.fosphor_amd_correlate_n_out(trace, n, T) == EINVAL
    with pytest.raises(ValueError):
        F.correlate_n_out("magnitude", 1, 1)
    e = np.zeros(3, F.EXTRACT_DTYPE)
    e["out_offset"], e["n_out"], e["first"], e["decim"], e["n_taps"] = (7, 1000, 2000), (33, 0, 10), (5, 6, 7), 4, 9
    jobs = F.correlate_jobs(e, 11, 4, trace="c", threshold=0.25)
    assert jobs.dtype == cm.JOB_DTYPE and list(jobs["offset"]) == [7, 1000, 2000] and list(jobs["n"]) == [33, 0, 10]
    assert list(jobs["out_offset"]) == [0, 60, 60] and set(jobs["trace"]) == {cm.C} and set(jobs["tpl_len"]) == {4}
    assert set(jobs["tpl_offset"]) == {11} and set(jobs["threshold"]) == {np.float32(0.25)}
    assert list(F.correlate_jobs(e, 0, 4, trace="rho")["out_offset"]) == [0, 30, 30]
    assert list(F.correlate_jobs(e, 0, 5, trace="c")["out_offset"]) == [0, 58, 58]
    e2 = e.copy()
    e2["n_out"] = (6, 9, 10)
    assert list(F.correlate_jobs(e2, 0, 4, trace="rho")["out_offset"]) == [0, 3, 9]
    jc = F.correlate_jobs(e2, 0, 4, trace="c")
    assert list(jc["out_offset"]) == [0, 6, 18] and not (jc["out_offset"] & 1).any()
    assert not F.correlate_jobs(e, 0, 4)["out_offset"].any() and np.all(np.isinf(F.correlate_jobs(e, 0, 4)["threshold"]))
    job = gr_fosphor_amd._lib.CorrelateJob()
    job.out_offset = 99
    assert lib.fosphor_amd_correlate_from_extract(e[:1].tobytes(), 5, 17, cm.RHO, -1.0, C.byref(job)) == 0
    assert (job.offset, job.out_offset, job.tpl_offset, job.n, job.tpl_len, job.trace, job.threshold) == (7, 0, 5, 33, 17, cm.RHO, -1.0)
    for bad, toff, T, trace, thr in ((dict(out_offset=-1), 0, 1, 0, 0.0), (dict(n_out=-1), 0, 1, 0, 0.0), ({}, -1, 1, 0, 0.0),
                                     ({}, 0, 0, 0, 0.0), ({}, 0, 1025, 0, 0.0), ({}, 0, 1, 3, 0.0), ({}, 0, 1, -1, 0.0),
                                     ({}, 0, 1, 0, math.nan)):
        x = e[:1].copy()
        for k, v in bad.items():
            x[k] = v
        assert lib.fosphor_amd_correlate_from_extract(x.tobytes(), toff, T, trace, thr, C.byref(job)) == EINVAL
    assert lib.fosphor_amd_correlate_from_extract(None, 0, 1, 0, 0.0, C.byref(job)) == EINVAL
    assert lib.fosphor_amd_correlate_from_extract(e[:1].tobytes(), 0, 1, 0, 0.0, None) == EINVAL


def test_derive(lib, F):
    """a planted template: y = g t + nothing else gives rho 1, gain g, the phase of g and an infinite snr; and the never-NaN cases"""
    rng = np.random.default_rng(5)
    t = rng.standard_normal((32, 2)).astype(np.float32)
    tc = t[:, 0].astype(np.float64) + 1j * t[:, 1]
    g = 0.5 * np.exp(2j * np.pi * 0.3)
    y = np.zeros((200, 2), np.float32)
    yc = g * tc
    y[70:102, 0], y[70:102, 1] = yc.real, yc.imag
    rec, _ = F.correlate_host(y, cm.make_jobs([(0, 0, 0, 200, 32, cm.NONE, 0.9)]), t)
    v = F.correlate_derive(rec, 1000.0)[0]
    assert set(v) == set(F.CORRELATE_VALUES) and rec["peak_lag"][0] == 70
    assert v["time"] == 0.07 and v["rho"] == float(rec["peak_rho"][0]) and abs(v["rho"] - 1.0) < 1e-6
    assert abs(v["gain_re"] + 1j * v["gain_im"] - g) < 1e-6 and abs(v["gain_db"] - 20 * math.log10(0.5)) < 1e-5
    assert abs(v["phase_turns"] - 0.3) < 1e-6 and v["snr_db"] > 60.0 and v["detections"] >= 1 and isinstance(v["detections"], int)
    r = np.zeros(1, cm.RECORD_DTYPE)
    r["peak_lag"], r["tpl_energy"], r["peak_rho"] = -1, 4.0, 0.5
    assert all(x == 0 for x in F.correlate_derive(r, 1.0)[0].values()), "no peak"
    r["peak_lag"], r["tpl_energy"] = 3, 0.0
    assert all(x == 0 for x in F.correlate_derive(r, 1.0)[0].values()), "Et == 0"
    r["tpl_energy"], r["peak_rho"], r["peak_c_re"], r["peak_energy"], r["n_edges"] = 4.0, np.float32(1.0000001), 2.0, 1.0, 2
    v = F.correlate_derive(r, 2.0)[0]
    assert v["snr_db"] == math.inf and v["time"] == 1.5 and v["gain_re"] == 0.5 and v["gain_im"] == 0.0 and v["detections"] == 2
    assert v["phase_turns"] == 0.0 and abs(v["gain_db"] - 20 * math.log10(0.5)) < 1e-12
    r["peak_rho"], r["peak_c_re"] = 0.0, 0.0
    v = F.correlate_derive(r, 2.0)[0]					# a silent window
    assert not any(math.isnan(x) for x in v.values()) and v["snr_db"] == -math.inf and v["gain_db"] == -math.inf
    r["peak_rho"] = 0.5
    assert F.correlate_derive(r, 2.0)[0]["snr_db"] == 0.0
    vals = gr_fosphor_amd._lib.CorrelateValues()
    for rate in (0.0, -1.0, math.inf, math.nan):
        assert lib.fosphor_amd_correlate_derive(r.tobytes(), rate, C.byref(vals)) == EINVAL
    assert lib.fosphor_amd_correlate_derive(None, 1.0, C.byref(vals)) == EINVAL
    assert lib.fosphor_amd_correlate_derive(r.tobytes(), 1.0, None) == EINVAL


def test_einval_table(lib):
    """each refused call leaves every float and every record at the sentinel"""
    iq, tpl = cm.noise(1000, 91), cm.noise(100, 92)
    #        offset out tpl_offset n   T  trace  threshold
    good = [(0, 3, 0, 110, 11, cm.RHO, 0.1), (990, 0, 90, 10, 10, cm.NONE, 0.1), (1000, 103, 99, 0, 1, cm.C, 0.1),
            (0, 104, 36, 163, 64, cm.C, np.inf), (5, 0, 0, 3, 4, cm.NONE, -1.0)]
    cap = 104 + 200
    rv, rec, out = host(lib, (iq, tpl, cm.make_jobs(good)), cap=cap)
    assert rv == 0 and np.all(out[:3] == SENTINEL) and np.all(out[3:103] != SENTINEL) and np.all(out[cap:] == SENTINEL)
    assert np.all(out[104:cap] != SENTINEL) and np.all(records_of(rec, 5).view(np.uint32) != SENTINEL)

    def refused(rows, src=None, **kw):
        kw.setdefault("cap", cap)
        rv, rec, out = host(lib, (iq, tpl if src is None else src, cm.make_jobs(rows)), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL), "nothing is written"

    for what in ("iq", "tpl", "jobs", "records"):
        refused(good, null=(what,))
    refused(good, null=("out",))							# some job has a trace
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (cm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=999); refused(good, n_tpl=-1); refused(good, n_tpl=99)
    refused(good, cap=-1); refused(good, cap=cap - 1)
    ok = (0, 0, 0, 10, 4, cm.RHO, 0.1)

    def one(**kw):
        row = dict(zip(("offset", "out_offset", "tpl_offset", "n", "tpl_len", "trace", "threshold"), ok))
        row.update(kw)
        refused([tuple(row.values())])

    one(offset=-1); one(out_offset=-1); one(tpl_offset=-1); one(n=-1); one(offset=991); one(offset=1001, n=0)
    one(offset=2 ** 62, n=2 ** 31 - 1); one(tpl_len=0); one(tpl_len=-1); one(tpl_len=cm.MAX_TPL + 1); one(tpl_offset=97)
    one(tpl_offset=101, tpl_len=1); one(tpl_offset=2 ** 62); one(trace=3); one(trace=-1); one(trace=cm.NONE, out_offset=1)
    one(threshold=np.nan); one(out_offset=cap + 1, n=0); one(out_offset=2 ** 62); one(out_offset=cap - 6); one(trace=cm.C, out_offset=cap - 13)
    refused([(0, 0, 0, 10, 1, cm.RHO, 0.1), (0, 9, 0, 10, 1, cm.RHO, 0.1)])	# [0, 10) and [9, 19): one float shared
    refused([(0, 30, 0, 100, 1, cm.RHO, 0.1), (0, 0, 0, 16, 1, cm.C, 0.1)])	# [30, 130) and [0, 32), given in descending order
    for name in ("iq", "tpl", "records"):
        refused(good, skew=(name, 4))
    refused(good, skew=("out", 2))
    # a template of MAX_TPL samples needs a longer template buffer
    refused([(0, 0, 0, 1000, cm.MAX_TPL, cm.NONE, 0.1)])
    # the last jobs that still fit, in the inputs and in the output; traces that touch; jobs without lags anywhere inside
    last = [(0, 0, 0, 10, 1, cm.RHO, 0.1), (0, 10, 0, 10, 1, cm.C, 0.1), (990, cap - 10, 90, 10, 1, cm.RHO, 0.1),
            (1000, cap, 99, 0, 1, cm.C, 0.1), (3, 5, 0, 3, 4, cm.RHO, 0.1), (0, 0, 0, 1000, 100, cm.NONE, 0.1)]
    assert host(lib, (iq, tpl, cm.make_jobs(last)), cap=cap)[0] == 0
    # no job has a trace: no output buffer is needed
    none = cm.make_jobs([(0, 0, 0, 100, 10, cm.NONE, 0.1)])
    rv, rec, out = host(lib, (iq, tpl, none), cap=0, null=("out",))
    assert rv == 0 and records_of(rec, 1).tobytes() == cm.correlate((iq, tpl, none))[0].tobytes()
    many = cm.make_jobs([(0, i, 0, 1, 1, cm.RHO, 0.1) for i in range(cm.MAX_JOBS)])
    assert host(lib, (iq, tpl, many))[0] == 0
    # more than 2^31 - 1 work-groups: MAX_JOBS overlapping jobs of 2^31 - 1 samples (2^21 tiles each), refused before a sample
    # is read; a quarter as many jobs would be accepted and are not tried
    n = 2 ** 31 - 1
    huge = cm.make_jobs([(0, 0, 0, n, 1, cm.NONE, 0.1) for i in range(cm.MAX_JOBS)])
    rec = np.full(16 * cm.MAX_JOBS, SENTINEL, np.uint32)
    assert lib.fosphor_amd_correlate_host(iq.ctypes.data, n, tpl.ctypes.data, 100, huge.ctypes.data, len(huge), rec.ctypes.data,
                                          None, 0) == EINVAL
    assert np.all(rec == SENTINEL)
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    assert lib.fosphor_amd_correlate(None, iq.ctypes.data, 1000, tpl.ctypes.data, 100, none.ctypes.data, 1, rec.ctypes.data, None, 0) == EINVAL
    assert lib.fosphor_amd_correlate_stats(None, None) == EINVAL


def test_chain_on_the_host(lib, F):
    """A preamble planted in noise in a small sc16 stream, through fosphor_amd_extract_host and fosphor_amd_correlate_host: the
    peak lag is the planted lag.  The condition on the input -- the SNR is such that the peak rho is at least twice the largest
    rho more than T / 4 lags away -- is asserted here, with both values printed."""
    raw, ejobs, tpl, planted = cm.chain_case()
    taps = F.extract_design(cm.CHAIN_DECIM, cm.CHAIN_TAPS, 0.8)
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    out = np.zeros((cap, 2), np.float32)
    assert lib.fosphor_amd_extract_host(raw.ctypes.data, len(raw), 2, ejobs.ctypes.data, len(ejobs), taps.ctypes.data, len(taps),
                                        out.ctypes.data, cap) == 0
    jobs = F.correlate_jobs(ejobs, cm.CHAIN_TPL_OFFSET, cm.CHAIN_T, trace="rho", threshold=0.5)
    records, views = F.correlate_host(out, jobs, tpl)
    want_rec, want = cm.correlate((out, tpl, jobs))
    assert records.tobytes() == want_rec.tobytes() and views[0].tobytes() == want[0].tobytes()
    peak, far = cm.chain_margin(views[0], planted)
    print("chain: peak rho %.4f at lag %d (planted %d), largest rho beyond T / 4 lags %.4f" % (peak, records["peak_lag"][0], planted, far))
    assert records["n_lags"][0] > 3 * cm.TILE and planted > cm.TILE
    assert peak >= 2.0 * far, "the condition on the input"
    assert records["peak_lag"][0] == planted
    v = F.correlate_derive(records, 1.0)[0]
    assert v["time"] == planted and v["detections"] == 1 and v["snr_db"] > 0.0
