"""Burst IQ correlated against templates on the device (include/fosphor_amd_correlate.h) against the numpy statement
(tests/correlate_model.py) and against fosphor_amd_correlate_host: records and traces bit for bit, tobytes().

The traces go into a sentinel-filled buffer in which GUARD floats before, behind and between the jobs' ranges belong to no job, and
the records into a sentinel-filled buffer with one record more than there are jobs; both are compared whole with the model's image,
so a float or a record written outside a job's range fails like a wrong one.  Every run ends by checking that the input buffers are
bit-identical, that the instance's ring position, waterfall and spectrum are untouched (the method of tests/test_gpu_demod.py) and
that the stats delta names the kernels that ran, at most two launches per call.

Seams of the kernels (the input sets are cm.cases()):
  the loads            16-byte pairs from the first 16-byte boundary: offset and tpl_offset 0 .. 3 in both parities against each
                       other, T and spans even and odd, a job that ends on the buffer's last sample, the template inside d_iq.
  k_correlate_tile     256 lanes, four lags a lane, TILE lags a work-group: n_lags = 0, 1, 255 .. 257, 1023 .. 1025, 2 TILE + 1,
                       3 TILE + 5; T = 1 .. 1024; odd and even out_offsets for both traces; edges inside a tile and on its ends.
  k_correlate_combine  a peak tie across the seam of two tiles, `above` on both sides of a seam, jobs without tiles (the template's
                       energy all the same), jobs of one tile and of four.
The refusal "more than 2^31 - 1 work-groups" needs MAX_JOBS jobs of 2^31 - 1 samples, 16 GiB of IQ: it is decided by the host code
that tests/test_correlate_cpu.py drives, and has no case here."""
import errno
import os

import numpy as np
import pytest

import correlate_model as cm

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a5a5a5a
CASES = cm.cases()
_MODEL = {}


def model(name):
    """the model's records and its image of a case's output buffer, computed once"""
    if name not in _MODEL:
        _MODEL[name] = cm.image(CASES[name], SENTINEL)
    return _MODEL[name]


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the correlate call through the C ABI"""

    def __init__(self, amd, wf_rows=16):
        self.f = amd.Fosphor(n_bins=128, wf_rows=wf_rows)
        self.n, self.wf_rows = self.f.n, wf_rows
        assert self.f.finish() >= 0			# a new instance fills its buffers at its first wait

    def views(self):
        import torch
        from gr_fosphor_amd.dist import wrap_device_array
        b = self.f.buffers(False)
        assert (b.fft_len, b.wf_rows) == (self.n, self.wf_rows)
        self.pos = b.waterfall_pos
        self.wf = wrap_device_array(b.d_waterfall, (self.wf_rows, self.n), torch.float32)
        self.spec = wrap_device_array(b.d_spectrum, (2, self.n, 2), torch.float32)

    def save(self):
        import torch
        assert self.f.finish() >= 0
        self.views()
        self.saved = (self.wf.view(torch.int32).clone(), self.spec.view(torch.int32).clone(), self.pos)
        torch.cuda.synchronize()

    def assert_untouched(self):
        import torch
        torch.cuda.synchronize()
        self.views()
        assert self.pos == self.saved[2], "the ring position moved"
        assert torch.equal(self.wf.view(torch.int32), self.saved[0]), "the waterfall was written"
        assert torch.equal(self.spec.view(torch.int32), self.saved[1]), "the spectrum lines were written"

    def call(self, case, n_samples=None, n_tpl=None, n_jobs=None, cap=None, null=(), skew=None):
        """-> (return value, the records buffer as uint32 [n_jobs + 1][16], the whole output buffer as uint32, delta of the
        stats).  cap: out_capacity, GUARD floats of the buffer lie behind it; skew: (pointer name, bytes)"""
        import torch
        self.save()
        iq, tpl = cm.buffers(case)
        jobs = np.ascontiguousarray(case[2], cm.JOB_DTYPE)
        d_iq = torch.from_numpy(iq if len(iq) else np.zeros((1, 2), np.float32)).cuda()
        d_tpl = d_iq if case[1] is None else torch.from_numpy(tpl).cuda()		# the templates of such a case lie in d_iq
        size = cm.capacity(jobs) if cap is None else max(cap, 0) + cm.GUARD
        d_out = torch.full((size + 1,), SENTINEL, dtype=torch.int32, device="cuda")
        d_rec = torch.full(((len(jobs) + 1) * 16,), SENTINEL, dtype=torch.int32, device="cuda")
        ptr = {"self": self.f.h, "iq": d_iq.data_ptr(), "tpl": d_tpl.data_ptr(), "jobs": jobs.ctypes.data,
               "records": d_rec.data_ptr(), "out": d_out.data_ptr()}
        for k in null:
            ptr[k] = None
        if skew:
            ptr[skew[0]] += skew[1]
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.correlate_stats()
        rv = self.f.L.fosphor_amd_correlate(ptr["self"], ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["tpl"],
                                            len(tpl) if n_tpl is None else n_tpl, ptr["jobs"],
                                            len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"],
                                            size if cap is None else cap)
        after = self.f.correlate_stats()
        out = d_out.cpu().numpy().view(np.uint32)
        rec = d_rec.cpu().numpy().view(np.uint32)
        assert out[size] == SENTINEL
        if len(iq):
            assert d_iq.cpu().numpy().tobytes() == iq.tobytes(), "the input buffer was written"
        assert d_tpl.cpu().numpy().tobytes() == tpl.tobytes(), "the template buffer was written"
        self.assert_untouched()
        return rv, rec, out[:size], {k: after[k] - before[k] for k in after}

    def run(self, case, tag="", **kw):
        """a call that must succeed: the stats -> (records, the whole output buffer)"""
        rv, rec, out, delta = self.call(case, **kw)
        assert rv == 0, tag
        jobs = case[2]
        lags = [cm.n_lags(int(j["n"]), int(j["tpl_len"])) for j in jobs]
        assert delta == dict(calls=1, k_tile=int(any(lags)), k_combine=1, jobs=len(jobs), lags=sum(lags), macs=cm.macs(jobs)), (tag, delta)
        assert delta["k_tile"] + delta["k_combine"] <= 2
        assert np.all(rec[16 * len(jobs):] == SENTINEL), "a record beyond the jobs' was written"
        return rec[:16 * len(jobs)].view(cm.RECORD_DTYPE), out


def explain(got_rec, want_rec, got, want, jobs):
    """print the first records and floats that differ, with the job that owns them"""
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, tuple(jobs[i]), got_rec[i], want_rec[i]))
    for i in np.flatnonzero(got != want)[:8]:
        own = [k for k, j in enumerate(jobs) if int(j["out_offset"]) <= i < int(j["out_offset"]) + trace_len(j)]
        print("float %d got %08x want %08x job %s" % (i, got[i], want[i], [(k, tuple(jobs[k])) for k in own]))


def trace_len(job):
    return cm.n_out(int(job["trace"]), int(job["n"]), int(job["tpl_len"]))


def trace_of(buf, job):
    at = int(job["out_offset"])
    return buf[at:at + trace_len(job)]


@pytest.fixture(scope="module")
def box(amd):
    b = Box(amd)
    yield b
    b.f.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_model_and_host(amd, box, name):
    case = CASES[name]
    jobs = case[2]
    want_rec, want = model(name)
    got_rec, got = box.run(case, tag=name)
    explain(got_rec, want_rec, got, want, jobs)
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical to the model"
    assert got.tobytes() == want.tobytes(), "traces bit-identical to the model, every other float at the sentinel"
    iq, tpl = cm.buffers(case)
    host_rec, host_views = amd.Fosphor.correlate_host(iq, jobs, tpl)
    assert got_rec.tobytes() == host_rec.tobytes(), "records bit-identical to fosphor_amd_correlate_host"
    for v, j in zip(host_views, jobs):
        assert trace_of(got, j).tobytes() == (b"" if v is None else v.tobytes()), "bit-identical to fosphor_amd_correlate_host"
    again_rec, again = box.run(case, tag=name + " again")
    assert again.tobytes() == got.tobytes() and again_rec.tobytes() == got_rec.tobytes(), "the same call twice is bit-identical"
    if name == "mixed257":
        assert len(jobs) == 257 and set(jobs["trace"]) == {cm.NONE, cm.RHO, cm.C}


def test_a_job_alone_and_among_256_others(box):
    """a record and a trace depend on their job alone: bit-identical alone and among the other jobs of the call"""
    iq, tpl, jobs = CASES["mixed257"]
    among_rec, among = box.run((iq, tpl, jobs), tag="among")
    lags = np.array([cm.n_lags(int(j["n"]), int(j["tpl_len"])) for j in jobs])
    picks = [int(np.flatnonzero((lags > cm.TILE) & (jobs["trace"] == t))[0]) for t in (cm.NONE, cm.RHO, cm.C)]
    picks += [int(np.flatnonzero((lags > 0) & (lags < 256) & (jobs["trace"] == cm.C))[0]), int(np.flatnonzero(lags == 0)[0]), 7]
    for i in picks:
        alone_rec, alone = box.run((iq, tpl, jobs[i:i + 1]), tag="alone %d" % i)
        assert alone_rec[0].tobytes() == among_rec[i].tobytes(), i
        assert trace_of(alone, jobs[i]).tobytes() == trace_of(among, jobs[i]).tobytes(), i


def test_the_cut_rule(box):
    """rule 4 on the device: a job gives, bit for bit, the trace and the per-lag facts of the two jobs it is cut into at lag c"""
    case, triples = cm.cut_case()
    jobs = case[2]
    got_rec, got = box.run(case, tag="cut")
    want_rec, want = cm.image(case, SENTINEL)
    explain(got_rec, want_rec, got, want, jobs)
    assert got_rec.tobytes() == want_rec.tobytes() and got.tobytes() == want.tobytes()
    cm.assert_cut(got_rec, [trace_of(got, j) for j in jobs], jobs, triples)


def test_python_front_end(box):
    import torch
    iq, tpl, _ = CASES["lag_counts"]
    rows = [(1, 2, 2 * cm.TILE + 70, 64, cm.RHO, 0.1), (0, 0, 300, 257, cm.NONE, 0.1), (3, 1, cm.TILE + 9, 10, cm.C, 0.1),
            (2, 0, 5, 64, cm.RHO, 0.1)]
    jobs = cm.make_jobs([(off, at, toff, n, T, trace, thr) for (off, toff, n, T, trace, thr), at in zip(rows, (3, 0, 2 * cm.TILE + 20, 1))])
    want_rec, want = cm.correlate((iq, tpl, jobs))
    d_iq, d_tpl = torch.from_numpy(iq).cuda(), torch.from_numpy(tpl).cuda()
    for records, views in (box.f.correlate(d_iq, jobs, tpl), box.f.correlate(d_iq.view(torch.complex64).reshape(-1), jobs, d_tpl),
                           box.f.correlate(d_iq, jobs, tpl.view(np.complex64).reshape(-1)),
                           box.f.correlate(d_iq.data_ptr(), jobs, d_tpl.data_ptr(), n_samples=len(iq), n_tpl=len(tpl))):
        assert records.dtype == cm.RECORD_DTYPE and records.tobytes() == want_rec.tobytes()
        assert len(views) == len(jobs) and views[1] is None
        assert views[0].dtype == torch.float32 and views[2].dtype == torch.complex64 and len(views[2]) == cm.TILE
        for v, w in zip(views, want):
            assert v is None or v.cpu().numpy().tobytes() == w.tobytes()
    # one burst against another: the template is a range of d_iq itself
    self_jobs = cm.make_jobs([(0, 0, 40, cm.TILE + 100, 32, cm.RHO, 0.5)])
    records, views = box.f.correlate(d_iq, self_jobs, d_iq)
    assert records["peak_lag"][0] == 40 and views[0].cpu().numpy().tobytes() == cm.correlate((iq, None, self_jobs))[1][0].tobytes()
    with pytest.raises(ValueError):
        box.f.correlate(d_iq.data_ptr(), jobs, tpl)
    with pytest.raises(ValueError):
        box.f.correlate(d_iq, jobs, d_tpl.data_ptr())
    with pytest.raises(ValueError):
        box.f.correlate(d_iq.double(), jobs, tpl)
    odd = jobs.copy()
    odd["out_offset"][2] += 1
    with pytest.raises(ValueError):
        box.f.correlate(d_iq, odd, tpl)


def test_einval_table(box):
    """each refused call leaves every float and record at the sentinel, launches nothing and counts nothing"""
    iq, tpl = cm.noise(20000, 91), cm.noise(100, 92)
    #        offset out tpl_offset n   T  trace  threshold
    good = [(0, 3, 0, 110, 11, cm.RHO, 0.1), (19990, 0, 90, 10, 10, cm.NONE, 0.1), (20000, 103, 99, 0, 1, cm.C, 0.1),
            (5, 104, 36, 1163, 64, cm.C, np.inf), (5, 0, 0, 3, 4, cm.NONE, -1.0)]
    cap = 104 + 2200
    rec, out = box.run((iq, tpl, cm.make_jobs(good)), tag="good", cap=cap)
    assert np.all(out[cap:] == SENTINEL) and np.all(out[104:cap] != SENTINEL) and np.all(out[3:103] != SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        rv, rec, out, delta = box.call((iq, tpl, cm.make_jobs(rows)), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "iq", "tpl", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (cm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=19999); refused(good, n_tpl=-1); refused(good, n_tpl=99)
    refused(good, cap=-1); refused(good, cap=cap - 1)
    ok = (0, 0, 0, 10, 4, cm.RHO, 0.1)

    def one(**kw):
        row = dict(zip(("offset", "out_offset", "tpl_offset", "n", "tpl_len", "trace", "threshold"), ok))
        row.update(kw)
        refused([tuple(row.values())])

    one(offset=-1); one(out_offset=-1); one(tpl_offset=-1); one(n=-1); one(offset=19991); one(offset=20001, n=0)
    one(offset=2 ** 62, n=2 ** 31 - 1); one(tpl_len=0); one(tpl_len=-1); one(tpl_len=cm.MAX_TPL + 1); one(tpl_offset=97)
    one(tpl_offset=101, tpl_len=1); one(tpl_offset=2 ** 62); one(trace=3); one(trace=-1); one(trace=cm.NONE, out_offset=1)
    one(threshold=np.nan); one(out_offset=cap + 1, n=0); one(out_offset=2 ** 62); one(out_offset=cap - 6); one(trace=cm.C, out_offset=cap - 13)
    refused([(0, 0, 0, 10, 1, cm.RHO, 0.1), (0, 9, 0, 10, 1, cm.RHO, 0.1)])	# [0, 10) and [9, 19): one float shared
    refused([(0, 30, 0, 100, 1, cm.RHO, 0.1), (0, 0, 0, 16, 1, cm.C, 0.1)])	# [30, 130) and [0, 32), given in descending order
    for name in ("iq", "tpl", "records"):
        refused(good, skew=(name, 4))
    refused(good, skew=("out", 2))
    # the last jobs that still fit, in the inputs and in the output; traces that touch; jobs without lags anywhere inside
    last = cm.make_jobs([(0, 0, 0, 10, 1, cm.RHO, 0.1), (0, 10, 0, 10, 1, cm.C, 0.1), (19990, cap - 10, 90, 10, 1, cm.RHO, 0.1),
                         (20000, cap, 99, 0, 1, cm.C, 0.1), (3, 5, 0, 3, 4, cm.RHO, 0.1), (0, 0, 0, 2000, 100, cm.NONE, 0.1)])
    rec, out = box.run((iq, tpl, last), tag="the last jobs that fit", cap=cap)
    want_rec, want = cm.image((iq, tpl, last), SENTINEL)
    assert rec.tobytes() == want_rec.tobytes()
    assert out[:len(want) - cm.GUARD].tobytes() == want[:-cm.GUARD].tobytes() and np.all(out[cap:] == SENTINEL)
    # no job has a trace: no output buffer; no job has a lag: the records all the same, from one launch
    none = cm.make_jobs([(0, 0, 0, 100, 10, cm.NONE, 0.1)])
    rec, out = box.run((iq, tpl, none), tag="no trace", cap=0, null=("out",))
    assert rec.tobytes() == cm.correlate((iq, tpl, none))[0].tobytes() and np.all(out == SENTINEL)
    empty = cm.make_jobs([(0, 7, 3, 5, 6, cm.RHO, 0.1), (3, 7, 1, 0, 2, cm.C, 0.1)])
    rec, out = box.run((iq, tpl, empty), tag="no job has a lag", cap=cap)
    assert rec.tobytes() == cm.correlate((iq, tpl, empty))[0].tobytes() and np.all(out == SENTINEL)


def test_chain_extract_correlate(amd, box):
    """the preamble planted in correlate_model's small sc16 stream: extract -> correlate over extract's own device buffer, the
    record and the rho trace bit-identical to the model run over that same buffer, and the peak at the planted lag (the condition
    on the input, peak >= 2 * the largest rho more than T / 4 lags away, is held by tests/test_correlate_cpu.py on the host chain
    and printed here)"""
    import torch
    F = amd.Fosphor
    raw, ejobs, tpl, planted = cm.chain_case()
    taps = F.extract_design(cm.CHAIN_DECIM, cm.CHAIN_TAPS, 0.8)
    d_x = torch.from_numpy(raw).cuda()
    views = box.f.extract(d_x, ejobs, taps, iq_format="sc16")
    base = views[0].data_ptr() - 8 * int(ejobs["out_offset"][0])		# extract()'s d_out: the views are slices of one buffer
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    out = np.zeros((cap, 2), np.float32)
    for j, v in zip(ejobs, views):
        out[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] = v.cpu().numpy().view(np.float32).reshape(-1, 2)
    jobs = F.correlate_jobs(ejobs, cm.CHAIN_TPL_OFFSET, cm.CHAIN_T, trace="rho", threshold=0.5)
    before = box.f.correlate_stats()
    records, got = box.f.correlate(base, jobs, tpl, n_samples=cap)
    after = box.f.correlate_stats()
    assert (after["k_tile"] - before["k_tile"], after["k_combine"] - before["k_combine"]) == (1, 1)
    want_rec, want = cm.correlate((out, tpl, jobs))
    rho = got[0].cpu().numpy()
    assert len(rho) > 3 * cm.TILE and rho.tobytes() == want[0].tobytes() and records.tobytes() == want_rec.tobytes()
    peak, far = cm.chain_margin(rho, planted)
    print("chain: peak rho %.4f at lag %d (planted %d), largest rho beyond T / 4 lags %.4f" % (peak, records["peak_lag"][0], planted, far))
    assert records["peak_lag"][0] == planted
    assert F.correlate_derive(records, 1.0)[0]["detections"] == 1
