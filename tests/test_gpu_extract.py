"""Burst IQ extraction on the device (include/fosphor_amd_extract.h) against the float64 statement (tests/extract_model.py).

Outputs go into a sentinel-filled buffer with GUARD untouched entries before, between and behind the jobs' ranges; every run ends
by checking that the guards hold, that the input buffer is bit-identical and that the instance's ring position, waterfall and
spectrum are untouched (the method of tests/test_gpu_burst.py).

Tolerance, per component: |err| <= (T + 16) * 2^-24 * A, A = sum|h[k]| * max|x| over the job's input span.  It is derived, not
measured: the mixer's sine and cosine are within 4 * 2^-24, the complex product rounds three times, the sum rounds once per fmaf
over T terms of at most |h[k]| * |x| each, the rest is slack; tests/test_extract_cpu.py shows that a plain float32 implementation
stays inside it on every input set used here.

Seams of the kernels (the input sets are em.cases()):
  k_extract_tile  a work-group owns FOSPHOR_AMD_EXTRACT_TILE_OUT = 256 outputs: n_out 0, 1, 255, 256, 257, 513.  Its loads take
                  16 bytes per lane from the first 16-byte boundary on (2 fp32 or 4 fp16 / sc16 samples): first = 0, 1, 2, 3, 5
                  in every format, and a job that ends on the stream's last sample.  Polyphase LDS image of D rows: D = 1, 2, 3,
                  4, 5, 7, 16, 25 (the largest with T = 8 D + 1), T < D.
  k_extract_wave  a wave owns an output, a work-group 4: n_out 0, 1, 3, 4, 5, 9; T below 64 lanes' worth, no multiple of 64, 8192.
  both            a work-group finds its job in a prefix of work-group counts: 257 jobs, mixed forms, one launch per form."""
import errno
import os

import numpy as np
import pytest

import extract_model as em

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a5a5a5a
CASES = em.cases()


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the extract call through the C ABI"""

    def __init__(self, amd, wf_rows=16, iq_format=None):
        self.f = amd.Fosphor(n_bins=128, wf_rows=wf_rows, iq_format=iq_format)
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

    def call(self, fmt, raw, jobs, taps, d_x=None, n_samples=None, n_taps_total=None, cap=None, null=(), skew=0):
        """-> (return value, the whole output buffer as uint32 [cap + GUARD][2], delta of the stats).  d_x: the samples if they
        are on the device already; skew: bytes added to the samples' pointer"""
        import torch
        self.save()
        raw = np.ascontiguousarray(raw)
        jobs = np.ascontiguousarray(jobs, em.JOB_DTYPE)
        taps = np.ascontiguousarray(taps, np.float32)
        if d_x is None:
            d_x = torch.from_numpy(raw).cuda()
        d_taps = torch.from_numpy(taps).cuda()
        cap = em.capacity(jobs) if cap is None else cap
        d_out = torch.full((max(cap, 1) + em.GUARD, 2), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.extract_stats()
        rv = self.f.L.fosphor_amd_extract(None if "self" in null else self.f.h, None if "x" in null else d_x.data_ptr() + skew,
                                          len(raw) if n_samples is None else n_samples, fmt,
                                          None if "jobs" in null else jobs.ctypes.data, len(jobs),
                                          None if "taps" in null else d_taps.data_ptr(),
                                          len(taps) if n_taps_total is None else n_taps_total,
                                          None if "out" in null else d_out.data_ptr(), cap)
        after = self.f.extract_stats()
        out = d_out.cpu().numpy().view(np.uint32)
        assert d_x.cpu().numpy().tobytes() == raw.tobytes(), "the input buffer was written"
        self.assert_untouched()
        return rv, out, {k: after[k] - before[k] for k in after}

    def run(self, fmt, raw, jobs, taps, tag="", **kw):
        """a call that must succeed: guards, stats, and every job against the model within the bound -> the jobs' outputs"""
        rv, out, delta = self.call(fmt, raw, jobs, taps, **kw)
        assert rv == 0, tag
        written = np.zeros(len(out), bool)
        for job in jobs:
            written[int(job["out_offset"]):int(job["out_offset"]) + int(job["n_out"])] = True
        assert np.all(out[~written] == SENTINEL), (tag, "written outside the jobs' ranges")
        live = jobs[jobs["n_out"] > 0]
        forms = np.array([em.form(int(j["decim"]), int(j["n_taps"])) for j in jobs])
        live_forms = forms[jobs["n_out"] > 0]
        assert delta == dict(calls=1, k_tile=int((live_forms == "tile").any()), k_wave=int((live_forms == "wave").any()),
                             jobs_tile=int((forms == "tile").sum()), jobs_wave=int((forms == "wave").sum()),
                             samples=sum(em.need(int(j["n_out"]), int(j["decim"]), int(j["n_taps"])) for j in live)), (tag, delta)
        x = em.widen(raw, fmt if fmt >= 0 else self.f.iq_format)
        got = []
        for job in jobs:
            sl = slice(int(job["out_offset"]), int(job["out_offset"]) + int(job["n_out"]))
            y = out[sl].view(np.float32)
            got.append(out[sl].copy())
            if job["n_out"] == 0:
                continue
            want, tol = em.extract_job(x, job, taps), em.bound(x, job, taps)
            err = max(np.abs(y[:, 0].astype(np.float64) - want.real).max(), np.abs(y[:, 1].astype(np.float64) - want.imag).max())
            print("%s D=%d T=%d n_out=%d %s: err %.3g of %.3g" % (tag, job["decim"], job["n_taps"], job["n_out"],
                                                                   em.form(int(job["decim"]), int(job["n_taps"])), err, tol))
            assert err <= tol, (tag, job, err, tol)
        return got


@pytest.fixture(scope="module")
def box(amd):
    b = Box(amd)
    yield b
    b.f.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_model(box, name):
    fmt, raw, jobs, taps = CASES[name]
    got = box.run(fmt, raw, jobs, taps, tag=name)
    if name.startswith("split"):
        # 64 outputs in one job and in two jobs of 32 whose phase0 continues the first: the phase does not depend on the cut
        assert np.array_equal(got[0], np.concatenate([got[1], got[2]])), name
    if name == "many":
        assert len(jobs) == 257 and (jobs["n_out"] == 0).any() and np.any(np.diff(jobs["out_offset"]) < 0)
        again = box.run(fmt, raw, jobs, taps, tag=name + " again")
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "the same call twice is bit-identical"
    if name.startswith("first"):
        last = max(int(j["first"]) + em.need(int(j["n_out"]), int(j["decim"]), int(j["n_taps"])) for j in jobs)
        assert last == len(raw), "a job ends on the stream's last sample"


def test_form_edge_from_the_stats(box):
    """the largest D of the TILE form and the smallest of the WAVE form (T = 8 D + 1), each alone in a call"""
    fmt, raw, jobs, taps = CASES["form_edge"]
    big, small = em.tile_edge()
    assert (int(jobs["decim"][0]), int(jobs["decim"][1])) == (big, small)
    for job, want in ((jobs[:1], dict(k_tile=1, k_wave=0, jobs_tile=1, jobs_wave=0)),
                      (jobs[1:], dict(k_tile=0, k_wave=1, jobs_tile=0, jobs_wave=1))):
        rv, out, delta = box.call(fmt, raw, job, taps, cap=em.capacity(jobs))
        assert rv == 0 and {k: delta[k] for k in want} == want, delta


def test_formats_agree_bit_for_bit(box):
    """the same values as sc16, as their exact float32 widening and as float16 (the values are chosen representable; the small
    ones are float16 subnormals): the outputs are bit-identical"""
    rng = np.random.default_rng(77)
    raw_sc = em.representable(3000, 78)
    taps, where = em.one_tap_set(rng, [(3, 25), (32, 70)])
    rows = [(1, 300, 3, 0x0f1e2d3c, 7, where[(3, 25)], 25), (2, 9, 32, 0xf0000001, 9, where[(32, 70)], 70)]
    jobs = em.make_jobs(rows)
    outs = [box.run(fmt, em.same_values(raw_sc, fmt), jobs, taps, tag="format %d" % fmt) for fmt in (em.SC16, em.FP32, em.FP16)]
    for other in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], other))


def test_einval_table(box):
    """each refused call leaves every output byte at the sentinel and launches nothing"""
    rng = np.random.default_rng(9)
    raw = em.stream(em.FP32, 1000, 9)
    raw16 = em.stream(em.SC16, 1000, 10)
    taps = em.lowpass(rng, 40)
    good = [(0, 10, 4, 5, 6, 0, 33), (100, 20, 2, 5, 6, 3, 9)]
    box.run(em.FP32, raw, em.make_jobs(good), taps, tag="good")
    box.run(-1, raw, em.make_jobs(good), taps, tag="the instance's format")

    def refused(rows, fmt=em.FP32, x=raw, edit=None, **kw):
        jobs = em.make_jobs(rows)
        if edit:
            edit(jobs)
        rv, out, delta = box.call(fmt, x, jobs, taps, **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    refused(good, fmt=3); refused(good, fmt=-2)
    for what in ("self", "x", "jobs", "taps", "out"):
        refused(good, null=(what,))
    refused(good, skew=4)							# fp32 samples are 8 bytes
    refused(good, fmt=em.SC16, x=raw16, skew=2); refused(good, fmt=em.FP16, x=raw16.view(np.float16), skew=2)
    refused([good[0]] * 4097)
    refused([(-1, 10, 4, 5, 6, 0, 33)]); refused([(0, -1, 4, 5, 6, 0, 33)])
    refused([(0, 10, 0, 5, 6, 0, 33)]); refused([(0, 10, 1025, 5, 6, 0, 33)])
    refused([(0, 10, 4, 5, 6, 0, 0)]); refused([(0, 1, 1, 5, 6, 0, 8193)])
    refused([(0, 10, 4, 5, 6, -1, 33)]); refused([(0, 10, 4, 5, 6, 8, 33)]); refused([good[0]], n_taps_total=32)
    refused([(1000 - 68, 10, 4, 5, 6, 0, 33)]); refused([(1001, 1, 1, 5, 6, 0, 1)]); refused(good, n_samples=146)
    refused(good, cap=em.capacity(em.make_jobs(good)) - em.GUARD - 1)
    refused(good, edit=lambda j: j["out_offset"].__setitem__(0, -1))
    refused(good, edit=lambda j: j["out_offset"].__setitem__(1, j["out_offset"][0] + 9))
    box.run(em.FP32, raw, em.make_jobs([(1000 - 69, 10, 4, 5, 6, 0, 33)]), taps, tag="the last job that fits")


@pytest.mark.parametrize("fmt", ["sc16", "fp32"])
def test_end_to_end_from_the_waterfall_to_baseband(amd, fmt):
    """noise, a tone 40 dB above it at shifted column 700.5 during spectra 64 .. 127 of 256, through process_device in calls of 16
    spectra (every row is stored: row j holds spectrum 255 - j), then bursts -> extract_from_burst -> extract_design -> extract"""
    import torch
    n, rows = 1024, 256
    rng = np.random.default_rng(1234)
    amp = 0.5
    sigma = amp / 100.0 / np.sqrt(2.0)						# noise power 2 sigma^2 = amp^2 / 10^4
    x = sigma * (rng.standard_normal(rows * n) + 1j * rng.standard_normal(rows * n))
    t = np.arange(64 * n, 128 * n)
    x[t] += amp * np.exp(2j * np.pi * ((700.5 - n / 2) / n) * t)
    if fmt == "sc16":
        raw, code = np.round(np.stack([x.real, x.imag], 1) * 32768.0).astype(np.int16), em.SC16
    else:
        raw, code = np.stack([x.real, x.imag], 1).astype(np.float32), em.FP32
    b = Box(amd, wf_rows=rows, iq_format=fmt)
    f = b.f
    d_x = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    for c in range(rows // 16):
        assert f.process_device(d_x[c * 16 * n:], 1, 16) == 0
    assert f.finish() >= 0
    wf = f.waterfall
    thr = float(np.median(wf)) + 1.5						# 30 dB above a noise bin, 40 dB below the tone's bins
    res, recs = f.bursts(thr, max_gap_cols=1)
    assert res["overflow"] == 0 and res["n_found"] == 1, res
    rec = recs[0]
    assert (rec["newest"], rec["oldest"]) == (128, 191) and rec["first_col"] <= 700 and rec["last_col"] >= 701, rec
    width = int(rec["last_col"] - rec["first_col"] + 1)
    assert width <= 12, rec

    job, n_taps = f.extract_from_burst(rec, newest_first_sample=(rows - 1 - 0) * n, row_hop=n, max_decim=64, guard=0.8)
    d = int(job["decim"][0])
    assert job["first"][0] == 64 * n and d == 64 and n_taps == 8 * d + 1
    taps = f.extract_design(d, n_taps, 0.8)
    noise = job.copy()
    noise["first"] = 160 * n
    jobs = np.concatenate([job, noise])
    jobs["out_offset"] = [em.GUARD, 2 * em.GUARD + int(job["n_out"][0])]
    got = b.run(-1, raw, jobs, taps, tag="end to end " + fmt, d_x=d_x)
    y = [g.view(np.float32).astype(np.float64) for g in got]
    y = [v[:, 0] + 1j * v[:, 1] for v in y]
    m = len(y[0])
    peak = int(np.argmax(np.abs(np.fft.fft(y[0]))))
    peak = peak - m if peak > m // 2 else peak
    assert abs(peak) / m <= 0.5 * width * d / n, (peak, m)		# within the burst's extent, scaled by D, of DC
    mid = slice(m // 4, m - m // 4)
    ratio = 10 * np.log10(np.mean(np.abs(y[0][mid]) ** 2) / np.mean(np.abs(y[1][mid]) ** 2))
    print("tone / noise after the filter: %.1f dB" % ratio)
    assert ratio >= 30.0

    # the Python front end gives the same samples
    views = f.extract(d_x, jobs, taps)
    assert [tuple(v.shape) for v in views] == [(m,), (m,)] and views[0].dtype == torch.complex64
    assert np.array_equal(views[0].cpu().numpy().view(np.uint32).reshape(-1, 2), got[0])
    assert np.array_equal(views[1].cpu().numpy().view(np.uint32).reshape(-1, 2), got[1])
    f.close()
