"""The power spectrum of burst IQ on the device (include/fosphor_amd_psd.h) against the numpy statement (tests/psd_model.py) and
against fosphor_amd_psd_host: records and traces bit for bit, tobytes().

The traces go into a sentinel-filled buffer in which GUARD floats before, behind and between the jobs' ranges belong to no job, and
the records into a sentinel-filled buffer with one record more than there are jobs; both are compared whole with the model's image,
so a float or a record written outside a job's range fails like a wrong one.  Every run ends by checking that the input buffers are
bit-identical, that the instance's ring position, waterfall and spectrum are untouched (the method of tests/test_gpu_correlate.py)
and that the stats delta names the kernels that ran, at most three launches per call.

Seams of the kernels (the input sets are pm.cases()):
  the loads       16-byte pairs from the first 16-byte boundary: offset and win_offset 0 .. 3 in both parities, odd and even
                  out_offsets, a job that ends on the buffer's last sample, n = L - 1, L, L + hop - 1 and L + hop.
  the forms       L = 64 and 128 by k_psd_wave, L = 256, 512 and 1024 by k_psd_group, one call with both and with jobs without
                  segments in between; WAVE-form tile counts of 1, 3, 4 and 5, so that a work-group of four is partly filled.
  the tiles       n_seg = 0, 1, 2, 31, 32, 33, 65 and 3 * 32 + 5; the hops 1, 37, L / 2 and L; all four pre-transforms.
  k_psd_combine   the fractions 1.0, 0.99 and 0.5, the ratios 1.0 and 1e-3, a peak tie, a cumulative sum that meets a threshold
                  exactly and passes it at a block seam of rule 5, silence, NaN and inf, overflow to inf under FOURTH, subnormals.
  the prefix      MAX_JOBS jobs in shuffled order, every 11th without a segment.
The refusal "more than 2^31 - 1 tiles in a form" needs MAX_JOBS jobs of 2^29 samples: it is decided by the host code that
tests/test_psd_cpu.py drives, and has no case here."""
import errno
import os

import numpy as np
import pytest

import psd_model as pm

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a5a5a5a
CASES = pm.cases()


def model(name):
    """the model's records and its image of a case's output buffer, computed once a session"""
    return pm.image(CASES[name], SENTINEL, key=name)


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the psd call through the C ABI"""

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

    def call(self, case, n_samples=None, n_win=None, n_jobs=None, cap=None, null=(), skew=None):
        """-> (return value, the records buffer as uint32 [n_jobs + 1][16], the whole output buffer as uint32, delta of the
        stats).  cap: out_capacity, GUARD floats of the buffer lie behind it; skew: (pointer name, bytes)"""
        import torch
        self.save()
        iq, win = pm.buffers(case)
        jobs = np.ascontiguousarray(case[2], pm.JOB_DTYPE)
        d_iq = torch.from_numpy(iq).cuda()
        d_win = torch.from_numpy(win).cuda()
        size = pm.capacity(jobs) if cap is None else max(cap, 0) + pm.GUARD
        d_out = torch.full((size + 1,), SENTINEL, dtype=torch.int32, device="cuda")
        d_rec = torch.full(((len(jobs) + 1) * 16,), SENTINEL, dtype=torch.int32, device="cuda")
        ptr = {"self": self.f.h, "iq": d_iq.data_ptr(), "win": d_win.data_ptr(), "jobs": jobs.ctypes.data,
               "records": d_rec.data_ptr(), "out": d_out.data_ptr()}
        for k in null:
            ptr[k] = None
        if skew:
            ptr[skew[0]] += skew[1]
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.psd_stats()
        rv = self.f.L.fosphor_amd_psd(ptr["self"], ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["win"],
                                      len(win) if n_win is None else n_win, ptr["jobs"], len(jobs) if n_jobs is None else n_jobs,
                                      ptr["records"], ptr["out"], size if cap is None else cap)
        after = self.f.psd_stats()
        out = d_out.cpu().numpy().view(np.uint32)
        rec = d_rec.cpu().numpy().view(np.uint32)
        assert out[size] == SENTINEL
        assert d_iq.cpu().numpy().tobytes() == iq.tobytes(), "the input buffer was written"
        assert d_win.cpu().numpy().tobytes() == win.tobytes(), "the window buffer was written"
        self.assert_untouched()
        return rv, rec, out[:size], {k: after[k] - before[k] for k in after}

    def run(self, case, tag="", **kw):
        """a call that must succeed: the stats -> (records, the whole output buffer)"""
        rv, rec, out, delta = self.call(case, **kw)
        assert rv == 0, tag
        jobs = case[2]
        segs = [pm.job_n_seg(j) for j in jobs]
        group = any(s and j["fft_len_log"] > pm.WAVE_MAX_LOG for s, j in zip(segs, jobs))
        wave = any(s and j["fft_len_log"] <= pm.WAVE_MAX_LOG for s, j in zip(segs, jobs))
        assert delta == dict(calls=1, k_group=int(group), k_wave=int(wave), k_combine=1, jobs=len(jobs), segments=sum(segs)), (tag, delta)
        assert delta["k_group"] + delta["k_wave"] + delta["k_combine"] <= 3
        assert np.all(rec[16 * len(jobs):] == SENTINEL), "a record beyond the jobs' was written"
        return rec[:16 * len(jobs)].view(pm.RECORD_DTYPE), out


def trace_of(buf, job):
    at = int(job["out_offset"])
    return buf[at:at + pm.n_out(job)]


def explain(got_rec, want_rec, got, want, jobs):
    """print the first records and floats that differ, with the job that owns them"""
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, tuple(jobs[i]), got_rec[i], want_rec[i]))
    for i in np.flatnonzero(got != want)[:8]:
        own = [k for k, j in enumerate(jobs) if int(j["out_offset"]) <= i < int(j["out_offset"]) + pm.n_out(j)]
        print("float %d got %08x want %08x job %s" % (i, got[i], want[i], [(k, tuple(jobs[k])) for k in own[:2]]))


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
    iq, win = pm.buffers(case)
    host_rec, host_views = amd.Fosphor.psd_host(iq, jobs, win)
    assert got_rec.tobytes() == host_rec.tobytes(), "records bit-identical to fosphor_amd_psd_host"
    for v, j in zip(host_views, jobs):
        assert trace_of(got, j).tobytes() == (b"" if v is None else v.tobytes()), "bit-identical to fosphor_amd_psd_host"
    again_rec, again = box.run(case, tag=name + " again")
    assert again.tobytes() == got.tobytes() and again_rec.tobytes() == got_rec.tobytes(), "the same call twice is bit-identical"
    if name == "nonfinite":
        assert np.isnan(got_rec["total"][:2]).all() and np.all(got_rec["total"][:2].view(np.uint64) == 0x7ff8000000000000)
        assert np.all(trace_of(got, jobs[0]) == 0x7fc00000) and np.isfinite(got_rec["total"][3:5]).all()


def test_a_job_alone_among_others_and_shuffled(box):
    """a record and a trace depend on their job alone: bit-identical alone, among the other jobs of the call, and with the table
    in another order (the outputs keep their places, the work-groups change theirs)"""
    iq, win, jobs = CASES["mixed"]
    among_rec, among = box.run((iq, win, jobs), tag="among")
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = box.run((iq, win, jobs[order]), tag="shuffled")
    assert shuffled.tobytes() == among.tobytes() and shuffled_rec.tobytes() == among_rec[order].tobytes()
    segs = np.array([pm.job_n_seg(j) for j in jobs])
    picks = [int(np.flatnonzero((segs > pm.TILE) & (jobs["fft_len_log"] == log) & (jobs["trace"] == pm.T_POWER))[0]) for log in (6, 8)]
    picks += [int(np.flatnonzero(segs == 0)[0]), int(np.flatnonzero((jobs["trace"] == pm.T_NONE) & (segs > 0))[0])]
    for i in picks:
        alone_rec, alone = box.run((iq, win, jobs[i:i + 1]), tag="alone %d" % i)
        assert alone_rec[0].tobytes() == among_rec[i].tobytes(), i
        assert trace_of(alone, jobs[i]).tobytes() == trace_of(among, jobs[i]).tobytes(), i


def test_python_front_end(box):
    import torch
    iq, win, jobs = CASES["loads"]
    want_rec, want, _ = pm.psd((iq, win, jobs))
    d_iq, d_win = torch.from_numpy(iq).cuda(), torch.from_numpy(win).cuda()
    for records, views in (box.f.psd(d_iq, jobs, win), box.f.psd(d_iq.view(torch.complex64).reshape(-1), jobs, d_win),
                           box.f.psd(d_iq.data_ptr(), jobs, d_win.data_ptr(), n_samples=len(iq), n_win=len(win))):
        assert records.dtype == pm.RECORD_DTYPE and records.tobytes() == want_rec.tobytes()
        assert len(views) == len(jobs)
        for v, w in zip(views, want):
            assert (v is None and len(w) == 0) or (v.dtype == torch.float32 and v.cpu().numpy().tobytes() == w.tobytes())
    with pytest.raises(ValueError):
        box.f.psd(d_iq.data_ptr(), jobs, win)
    with pytest.raises(ValueError):
        box.f.psd(d_iq, jobs, d_win.data_ptr())
    with pytest.raises(ValueError):
        box.f.psd(d_iq, jobs, d_win.double())


def test_einval_table(box):
    """each refused call leaves every float and record at the sentinel, launches nothing and counts nothing"""
    iq = pm.noise(3000, 91)
    win = np.concatenate([pm.window(pm.HANN, 6), pm.window(pm.BH, 8), np.ones(3, np.float32)])	# 64 + 256 + 3 floats
    nw = len(win)
    #        offset out win n    log hop pre      trace       obw   xdb
    good = [(0, 3, 0, 500, 6, 32, pm.NONE, pm.T_POWER, 0.99, 0.1), (2990, 0, 64, 10, 8, 256, pm.SQUARE, pm.T_NONE, 0.5, 1.0),
            (3000, 67, 67, 0, 8, 1, pm.MAGSQ, pm.T_POWER, 1.0, 1e-3), (1, 144, 64, 2999, 8, 100, pm.FOURTH, pm.T_POWER, 0.99, 0.1)]
    cap = 144 + 256
    rec, out = box.run((iq, win, pm.make_jobs(good)), tag="good", cap=cap)
    assert np.all(out[cap:] == SENTINEL) and np.all(out[144:cap] != SENTINEL) and np.all(out[3:67] != SENTINEL) and np.all(out[67:144] == SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        rv, rec, out, delta = box.call((iq, win, pm.make_jobs(rows)), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "iq", "win", "jobs", "records", "out"):
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
    # the last jobs that still fit, in the inputs and in the output; traces that touch; jobs without segments anywhere inside
    last = pm.make_jobs([(0, 0, 0, 64, 6, 64, 0, 1, 0.99, 0.1), (0, 64, 0, 65, 6, 1, 0, 1, 0.99, 0.1), (2744, cap - 256, nw - 256, 256, 8, 256, 0, 1, 1.0, 1.0),
                         (3000, cap, nw - 64, 0, 6, 1, 0, 1, 0.99, 0.1), (5, cap, nw - 256, 255, 8, 1, 0, 1, 0.99, 0.1)])
    assert cap - 256 >= 128
    rec, out = box.run((iq, win, last), tag="the last jobs that fit", cap=cap)
    want_rec, want = pm.image((iq, win, last), SENTINEL)
    assert rec.tobytes() == want_rec.tobytes()
    assert out[:cap].tobytes() == want[:cap].tobytes() and np.all(out[cap:] == SENTINEL)
    # no job has a trace: no output buffer; no job has a segment: the records all the same, from one launch
    none = pm.make_jobs([(0, 0, 0, 1000, 8, 128, 0, 0, 0.99, 0.1)])
    rec, out = box.run((iq, win, none), tag="no trace", cap=0, null=("out",))
    assert rec.tobytes() == pm.psd((iq, win, none))[0].tobytes() and np.all(out == SENTINEL)
    empty = pm.make_jobs([(0, 7, 0, 63, 6, 6, 0, 1, 0.99, 0.1), (3, 7, 64, 0, 8, 2, 0, 1, 0.99, 0.1)])
    rec, out = box.run((iq, win, empty), tag="no job has a segment", cap=cap)
    assert rec.tobytes() == pm.psd((iq, win, empty))[0].tobytes() and np.all(out == SENTINEL)
    assert list(rec["n_seg"]) == [0, 0] and rec["win_energy"][0] > 0.0


def test_chain_extract_psd(amd, box):
    """the QPSK preamble of correlate_model's small sc16 stream: extract -> psd over extract's own device buffer, records and traces
    bit-identical to the model run over that same buffer; the fourth power shows the carrier line of the extraction's centre at DC"""
    import torch
    import correlate_model as cm
    F = amd.Fosphor
    raw, ejobs, _, _ = cm.chain_case()
    taps = F.extract_design(cm.CHAIN_DECIM, cm.CHAIN_TAPS, 0.8)
    views = box.f.extract(torch.from_numpy(raw).cuda(), ejobs, taps, iq_format="sc16")
    base = views[0].data_ptr() - 8 * int(ejobs["out_offset"][0])		# extract()'s d_out: the views are slices of one buffer
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    out = np.zeros((cap, 2), np.float32)
    for j, v in zip(ejobs, views):
        out[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] = v.cpu().numpy().view(np.float32).reshape(-1, 2)
    win = F.psd_window("hann", pm.CHAIN_LOG)
    jobs = pm.chain_jobs(F, ejobs)
    records, got = box.f.psd(base, jobs, win, n_samples=cap)
    want_rec, want, _ = pm.psd((out, win, jobs))
    assert records.tobytes() == want_rec.tobytes()
    for v, w in zip(got, want):
        assert v.cpu().numpy().tobytes() == w.tobytes()
    assert records["n_seg"][0] > pm.TILE
