"""Burst IQ resampled on the device (include/fosphor_amd_resample.h) against the numpy statement (tests/resample_model.py) and
against fosphor_amd_resample_host: every output bit for bit, tobytes().

The outputs go into a sentinel-filled buffer in which GUARD samples before, behind and between the jobs' ranges belong to no job;
it is compared whole with the model's image, so a float written outside a job's range fails like a wrong one.  Every run ends by
checking that the samples and the taps are bit-identical, that the instance's ring position, waterfall and spectrum are untouched
(the method of tests/test_gpu_correlate.py) and that the stats delta names the forms that ran, at most two launches per call.

Seams of the kernels (the input sets are rm.cases()):
  the loads           16-byte pairs from the first 16-byte boundary: offset 0 .. 3 against out_offsets of both parities, taps_offset
                      0 .. 3, spans even and odd, a job that ends on the buffer's last sample, phase0 = (n - Q) U exactly.
  k_resample_tile     256 lanes, two outputs a lane, TILE outputs a work-group: n_out = 0, 1, 255 .. 257, TILE - 1 .. TILE + 1,
                      2 TILE + 1; (U, D) from (1, 1) to (256, 1) and (255, 256); Q = 1, 2, 63, 64; branch 0 and a later branch at
                      output 0.
  k_resample_direct   the same counts; (1, 256); jobs one step of D or of Q beyond the LDS budget, computed from the header's
                      macros; the same job in both forms, bit-identical.
The refusal "more than 2^31 - 1 work-groups" needs MAX_JOBS jobs of 2^31 - 1 samples: it is decided by the host code that
tests/test_resample_cpu.py drives, and has no case here."""
import errno
import os

import numpy as np
import pytest

import resample_model as rm

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a5a5a5a
CASES = rm.cases()
_MODEL = {}


def model(name):
    """the model's image of a case's output buffer, computed once"""
    if name not in _MODEL:
        _MODEL[name] = rm.image(CASES[name], SENTINEL)
    return _MODEL[name]


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the resample call through the C ABI"""

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

    def call(self, case, n_samples=None, n_taps=None, n_jobs=None, cap=None, null=(), skew=None):
        """-> (return value, the whole output buffer as uint32 [2 * size], delta of the stats).  cap: out_capacity, GUARD samples
        of the buffer lie behind it; skew: (pointer name, bytes)"""
        import torch
        self.save()
        iq = np.ascontiguousarray(case[0], np.float32).reshape(-1, 2)
        taps = np.ascontiguousarray(case[1], np.float32)
        jobs = np.ascontiguousarray(case[2], rm.JOB_DTYPE)
        d_iq = torch.from_numpy(iq if len(iq) else np.zeros((1, 2), np.float32)).cuda()
        d_taps = torch.from_numpy(taps).cuda()
        size = rm.capacity(jobs) if cap is None else max(cap, 0) + rm.GUARD
        d_out = torch.full((2 * size + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        ptr = {"self": self.f.h, "iq": d_iq.data_ptr(), "taps": d_taps.data_ptr(), "jobs": jobs.ctypes.data, "out": d_out.data_ptr()}
        for k in null:
            ptr[k] = None
        if skew:
            ptr[skew[0]] += skew[1]
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.resample_stats()
        rv = self.f.L.fosphor_amd_resample(ptr["self"], ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["jobs"],
                                           len(jobs) if n_jobs is None else n_jobs, ptr["taps"],
                                           len(taps) if n_taps is None else n_taps, ptr["out"], size if cap is None else cap)
        after = self.f.resample_stats()
        out = d_out.cpu().numpy().view(np.uint32)
        assert np.all(out[2 * size:] == SENTINEL)
        if len(iq):
            assert d_iq.cpu().numpy().tobytes() == iq.tobytes(), "the input buffer was written"
        assert d_taps.cpu().numpy().tobytes() == taps.tobytes(), "the taps were written"
        self.assert_untouched()
        return rv, out[:2 * size], {k: after[k] - before[k] for k in after}

    def run(self, case, tag="", **kw):
        """a call that must succeed: the stats -> the whole output buffer"""
        rv, out, delta = self.call(case, **kw)
        assert rv == 0, tag
        assert delta == rm.expected_stats(case[2]), (tag, delta)
        assert delta["k_tile"] + delta["k_direct"] <= 2
        return out


def explain(got, want, jobs):
    """print the first floats that differ, with the job that owns them"""
    for i in np.flatnonzero(got != want)[:8]:
        own = [k for k, j in enumerate(jobs) if 2 * int(j["out_offset"]) <= i < 2 * (int(j["out_offset"]) + int(j["n_out"]))]
        print("float %d got %08x want %08x job %s" % (i, got[i], want[i], [(k, tuple(jobs[k])) for k in own]))


@pytest.fixture(scope="module")
def box(amd):
    b = Box(amd)
    yield b
    b.f.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_model_and_host(amd, box, name):
    case = CASES[name]
    jobs = case[2]
    want = model(name)
    got = box.run(case, tag=name)
    explain(got, want, jobs)
    assert got.tobytes() == want.tobytes(), "outputs bit-identical to the model, every other float at the sentinel"
    for v, j in zip(amd.Fosphor.resample_host(case[0], jobs, case[1]), jobs):
        assert rm.outputs_of(got, j).tobytes() == v.tobytes(), "bit-identical to fosphor_amd_resample_host"
    again = box.run(case, tag=name + " again")
    assert again.tobytes() == got.tobytes(), "the same call twice is bit-identical"
    forms = [rm.form(int(j["up"]), int(j["down"]), int(j["n_taps"])) for j in jobs]
    if name == "seam":
        assert forms[:2] == ["tile", "direct"] and jobs["n_out"][0] > rm.TILE
        assert rm.outputs_of(got, jobs[0]).tobytes() == rm.outputs_of(got, jobs[1]).tobytes(), "the same job in both forms"
    if name == "nonfinite":
        for j in jobs:
            o = rm.outputs_of(got, j)
            nan = np.isnan(o.view(np.float32))
            assert nan.any() and not nan.all() and np.all(o[nan] == 0x7fc00000), "one quiet NaN"
    if name == "mixed257":
        assert len(jobs) == 257 and {"tile", "direct"} == set(forms)


def test_a_job_alone_and_among_256_others(box):
    """an output depends on its job alone: bit-identical alone and among the other jobs of the call"""
    iq, taps, jobs = CASES["mixed257"]
    among = box.run((iq, taps, jobs), tag="among")
    forms = np.array([rm.form(int(j["up"]), int(j["down"]), int(j["n_taps"])) for j in jobs])
    picks = [int(np.flatnonzero((jobs["n_out"] > rm.TILE) & (forms == f))[0]) for f in ("tile", "direct")]
    picks += [int(np.flatnonzero((jobs["n_out"] > 0) & (jobs["n_out"] < 256) & (forms == f))[0]) for f in ("tile", "direct")]
    picks += [int(np.flatnonzero(jobs["n_out"] == 0)[0]), 7]
    for i in picks:
        alone = box.run((iq, taps, jobs[i:i + 1]), tag="alone %d" % i)
        assert rm.outputs_of(alone, jobs[i]).tobytes() == rm.outputs_of(among, jobs[i]).tobytes(), i


def test_the_cut_rule(box):
    """rule 3 on the device: a job gives, bit for bit, the outputs of the two jobs it is cut into at output c"""
    case, triples = rm.cut_case()
    jobs = case[2]
    got = box.run(case, tag="cut")
    want = rm.image(case, SENTINEL)
    explain(got, want, jobs)
    assert got.tobytes() == want.tobytes()
    rm.assert_cut([rm.outputs_of(got, j) for j in jobs], triples)


def test_python_front_end(amd, box):
    import torch
    iq, taps, _ = CASES["counts"]
    #       offset out phase0 n    n_out U  D  taps_offset T
    jobs = rm.make_jobs([(1, 3, 2, 2000, 2 * rm.TILE + 70, 3, 2, 1, 12), (0, 0, 0, 3, 0, 3, 2, 0, 12), (3, 2 * rm.TILE + 80, 5, 9000, 300, 1, 16, 2, 5),
                         (2, 1, 0, 5, 2, 1, 1, 7, 4)])
    want = rm.resample((iq, taps, jobs))
    d_iq, d_taps = torch.from_numpy(iq).cuda(), torch.from_numpy(taps).cuda()
    for views in (box.f.resample(d_iq, jobs, taps), box.f.resample(d_iq.view(torch.complex64).reshape(-1), jobs, d_taps),
                  box.f.resample(d_iq.data_ptr(), jobs, list(taps), n_samples=len(iq))):
        assert len(views) == len(jobs) and len(views[1]) == 0
        for v, w in zip(views, want):
            assert v.dtype == torch.complex64 and v.cpu().numpy().tobytes() == w.tobytes()
    # resample_jobs from extract jobs: what extract() wrote, resampled where it lies
    F = amd.Fosphor
    e = np.zeros(2, F.EXTRACT_DTYPE)
    e["out_offset"], e["n_out"], e["first"], e["decim"], e["n_taps"] = (1, 700), (600, 40), 0, 1, 1
    h = F.resample_design(2, 3, 8)
    rjobs = F.resample_jobs(e, 2, 3, len(h))
    assert list(rjobs["offset"]) == [1, 700] and list(rjobs["n_out"]) == [rm.max_n_out(600, 2, 3, 16), rm.max_n_out(40, 2, 3, 16)]
    for v, w in zip(box.f.resample(d_iq, rjobs, h), rm.resample((iq, h, rjobs))):
        assert v.cpu().numpy().tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        box.f.resample(d_iq.data_ptr(), jobs, taps)			# a raw pointer needs n_samples
    with pytest.raises(ValueError):
        box.f.resample(d_iq.double(), jobs, taps)
    with pytest.raises(ValueError):
        box.f.resample(d_iq, jobs, d_taps.double())
    with pytest.raises(ValueError):
        box.f.resample(d_iq, jobs, d_taps.cpu())
    with pytest.raises(RuntimeError):
        bad = jobs.copy()
        bad["n_out"][3] = 3						# one more than is valid
        box.f.resample(d_iq, bad, taps)


def test_einval_table(box):
    """each refused call leaves every float at the sentinel, launches nothing and counts nothing"""
    iq, taps = rm.noise(20000, 91), rm.some_taps(100, 92)
    #        offset out phase0 n    n_out U  D  taps_offset T
    good = [(0, 3, 0, 110, 100, 3, 2, 0, 12), (19990, 0, 0, 10, 3, 1, 4, 90, 2), (20000, 103, 0, 0, 0, 1, 1, 99, 1),
            (5, 104, 5, 19000, 1100, 1, 16, 36, 5), (5, 1210, 7, 3, 0, 2, 1, 0, 8)]
    cap = 104 + 1100 + 10
    out = box.run((iq, taps, rm.make_jobs(good)), tag="good", cap=cap)
    assert np.all(out[:206] != SENTINEL) and np.all(out[206:208] == SENTINEL) and np.all(out[208:2 * 1204] != SENTINEL)
    assert np.all(out[2 * 1204:] == SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        rv, out, delta = box.call((iq, taps, rm.make_jobs(rows)), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "iq", "jobs", "taps", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (rm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=19999); refused(good, n_taps=-1); refused(good, n_taps=99)
    refused(good, cap=-1); refused(good, cap=1203)
    ok = (0, 0, 0, 10, 4, 1, 1, 0, 4)

    def one(**kw):
        row = dict(zip(rm.FIELDS, ok))
        row.update(kw)
        refused([tuple(row.values())])

    one(offset=-1); one(out_offset=-1); one(phase0=-1); one(n=-1); one(n_out=-1); one(offset=19991); one(offset=20001, n=0, n_out=0)
    one(offset=2 ** 62, n=2 ** 31 - 1); one(offset=2 ** 62); one(up=0); one(up=-1); one(up=rm.MAX_UP + 1, n_taps=rm.MAX_UP + 1)
    one(down=0); one(down=-1); one(down=rm.MAX_DOWN + 1); one(n_taps=0); one(n_taps=-4); one(up=3, n_taps=4); one(n_taps=rm.MAX_BRANCH + 1)
    one(up=2, n_taps=2 * rm.MAX_BRANCH + 2); one(taps_offset=-1); one(taps_offset=97); one(taps_offset=101, n_taps=1); one(taps_offset=2 ** 31 - 1)
    one(n_out=8); one(n_out=2 ** 31 - 1); one(phase0=1, n_out=7); one(phase0=7, n_out=1); one(phase0=2 ** 62, n_out=1); one(n=3, n_out=1)
    one(down=2, n_out=5); one(up=2, n_taps=8, n_out=14)
    one(out_offset=cap + 1, n_out=0); one(out_offset=2 ** 62); one(out_offset=cap - 3)
    refused([(0, 0, 0, 10, 7, 1, 1, 0, 4), (0, 6, 0, 10, 7, 1, 1, 0, 4)])		# [0, 7) and [6, 13): one sample shared
    refused([(0, 30, 0, 100, 90, 1, 1, 0, 4), (0, 0, 0, 40, 31, 1, 1, 0, 4)])	# [30, 120) and [0, 31), given in descending order
    for name in ("iq", "out"):
        refused(good, skew=(name, 4))
    refused(good, skew=("taps", 2))
    # the last jobs that still fit, in the inputs, the taps and the output; outputs that touch; jobs without outputs anywhere inside
    last = rm.make_jobs([(0, 0, 0, 10, 7, 1, 1, 0, 4), (0, 7, 6, 10, 1, 1, 1, 96, 4), (19990, cap - 7, 0, 10, 7, 1, 1, 0, 4),
                         (20000, cap, 2 ** 62, 0, 0, 1, 1, 99, 1), (3, 5, 0, 3, 0, 1, 1, 0, 4), (0, 8, 0, 1000, 13, 25, 24, 0, 100),
                         (19000, 30, 0, 1000, 62, 1, 16, 95, 5)])
    out = box.run((iq, taps, last), tag="the last jobs that fit", cap=cap)
    assert out[:2 * cap].tobytes() == rm.image((iq, taps, last), SENTINEL)[:2 * cap].tobytes() and np.all(out[2 * cap:] == SENTINEL)
    # no job has an output: counted, nothing launched
    empty = rm.make_jobs([(0, 7, 0, 3, 0, 1, 1, 0, 4), (3, 7, 2 ** 40, 0, 0, 1, 16, 0, 5)])
    out = box.run((iq, taps, empty), tag="no job has an output", cap=cap)
    assert np.all(out == SENTINEL)


def test_chain_extract_resample_correlate(amd, box):
    """the preamble planted in resample_model's small sc16 stream: extract -> resample -> correlate, each over the device buffer
    the one before it wrote; the resampled IQ and then the record and the rho trace bit-identical to the models run over those same
    buffers, and the peak at the planted lag (the conditions on the input are held by tests/test_resample_cpu.py on the host chain;
    the margin is printed here)"""
    import torch
    import correlate_model as cm
    F = amd.Fosphor
    raw, ejobs, tpl, planted = rm.chain_case()
    taps = F.extract_design(rm.CHAIN_DECIM, rm.CHAIN_TAPS, 0.8)
    d_x = torch.from_numpy(raw).cuda()
    views = box.f.extract(d_x, ejobs, taps, iq_format="sc16")
    base = views[0].data_ptr() - 8 * int(ejobs["out_offset"][0])		# extract()'s d_out: the views are slices of one buffer
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    ext = np.zeros((cap, 2), np.float32)
    for j, v in zip(ejobs, views):
        ext[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] = v.cpu().numpy().view(np.float32).reshape(-1, 2)
    h = F.resample_design(rm.CHAIN_UP, rm.CHAIN_DOWN, rm.CHAIN_BRANCH, 0.8)
    rjobs = F.resample_jobs(ejobs, rm.CHAIN_UP, rm.CHAIN_DOWN, len(h))
    before = box.f.resample_stats()
    res = box.f.resample(base, rjobs, h, n_samples=cap)
    after = box.f.resample_stats()
    assert (after["k_tile"] - before["k_tile"], after["k_direct"] - before["k_direct"]) == (1, 0)
    got = res[0].cpu().numpy()
    assert len(got) > 4 * rm.TILE and got.tobytes() == rm.resample_job(ext, h, rjobs[0]).tobytes()
    cjobs = cm.make_jobs([(0, 0, rm.CHAIN_TPL_OFFSET, len(got), rm.CHAIN_T, cm.RHO, 0.5)])
    records, traces = box.f.correlate(res[0], cjobs, tpl)
    want_rec, want = cm.correlate((got.view(np.float32).reshape(-1, 2), tpl, cjobs))
    rho = traces[0].cpu().numpy()
    assert rho.tobytes() == want[0].tobytes() and records.tobytes() == want_rec.tobytes()
    peak, far = rm.chain_margin(rho, planted)
    print("chain: peak rho %.4f at lag %d (planted %d), largest rho beyond T / 4 lags %.4f" % (peak, records["peak_lag"][0], planted, far))
    assert records["peak_lag"][0] == planted
    assert F.correlate_derive(records, 1.0)[0]["detections"] == 1
