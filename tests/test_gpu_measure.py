"""Burst IQ measured on the device (include/fosphor_amd_measure.h) against the numpy statement (tests/measure_model.py) and against
fosphor_amd_measure_host.

The records go into a sentinel-filled buffer with GUARD untouched records before and behind; every run ends by checking that the
guards hold, that the input buffer is bit-identical, that the instance's ring position, waterfall and spectrum are untouched (the
method of tests/test_gpu_extract.py) and that the stats delta names the kernels that ran.

Integers, the peak, n and the form must equal the model's and the host's.  A sum must be within n * 2^-52 * sum|term| of math.fsum
over its terms: the bound of rule 3, derived there, not measured.

Seams of the kernels (the input sets are mm.cases()):
  k_measure_wave     a wave strides a job 128 samples a round, pairs from the first 16-byte boundary: n = 0, 1, 2, 63, 64, 65, 127,
                     128, 129, WAVE_MAX - 1, WAVE_MAX; offsets 0, 1, 2, 3; a job that ends on the buffer's last sample; four jobs
                     per work-group: 1, 3, 4, 5 jobs.
  k_measure_split    a work-group owns CHUNK samples: n = WAVE_MAX + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 CHUNK + 1, 3 CHUNK + 5 at
                     even and odd offsets; a run above the threshold and the maximum, twice, across a chunk boundary; a rising
                     edge at a chunk's first sample; the maximum again in another chunk, and in other lanes of a wave.
  both               257 jobs of mixed forms in at most three launches, overlapping ranges, thresholds +inf, below zero and
                     exactly a sample's p.
The refusal "more than 2^31 - 1 work-groups in one form" cannot be reached with MAX_JOBS jobs of int32 lengths (the header says
so) and has no case."""
import errno
import os

import numpy as np
import pytest

import measure_model as mm

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a5a5a5a
REC = mm.RECORD_DTYPE.itemsize
CASES = mm.cases()
_MODEL = {}


def model(name):
    """the model's records and the tolerances of a case, computed once"""
    if name not in _MODEL:
        iq, jobs = CASES[name]
        _MODEL[name] = (mm.measure(iq, jobs), mm.tolerance(CASES[name]))
    return _MODEL[name]


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the measure call through the C ABI"""

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

    def call(self, iq, jobs, d_iq=None, n_samples=None, n_jobs=None, null=(), skew_iq=0, skew_rec=0):
        """-> (return value, the whole record buffer as uint32 [GUARD + jobs + GUARD][24], delta of the stats).  d_iq: the samples
        if they are on the device already; skew_*: bytes added to a pointer"""
        import torch
        self.save()
        iq = np.ascontiguousarray(iq, np.float32).reshape(-1, 2)
        jobs = np.ascontiguousarray(jobs, mm.JOB_DTYPE)
        if d_iq is None:
            d_iq = torch.from_numpy(iq if len(iq) else np.zeros((1, 2), np.float32)).cuda()
        d_rec = torch.full((len(jobs) + 2 * mm.GUARD, REC // 4), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.measure_stats()
        rv = self.f.L.fosphor_amd_measure(None if "self" in null else self.f.h, None if "iq" in null else d_iq.data_ptr() + skew_iq,
                                          len(iq) if n_samples is None else n_samples,
                                          None if "jobs" in null else jobs.ctypes.data, len(jobs) if n_jobs is None else n_jobs,
                                          None if "records" in null else d_rec.data_ptr() + mm.GUARD * REC + skew_rec)
        after = self.f.measure_stats()
        out = d_rec.cpu().numpy().view(np.uint32)
        if len(iq):
            assert d_iq.cpu().numpy().tobytes() == iq.tobytes(), "the input buffer was written"
        self.assert_untouched()
        return rv, out, {k: after[k] - before[k] for k in after}

    def run(self, iq, jobs, tag="", **kw):
        """a call that must succeed: guards and stats -> the records"""
        rv, out, delta = self.call(iq, jobs, **kw)
        assert rv == 0, tag
        assert np.all(out[:mm.GUARD] == SENTINEL) and np.all(out[-mm.GUARD:] == SENTINEL), (tag, "written outside the records")
        split = np.array([mm.form(int(n)) == mm.FORM_SPLIT for n in jobs["n"]])
        assert delta == dict(calls=1, k_wave=int((~split).any()), k_split=int(split.any()), k_combine=int(split.any()),
                             jobs_wave=int((~split).sum()), jobs_split=int(split.sum()), samples=int(jobs["n"].sum())), (tag, delta)
        assert delta["k_wave"] + delta["k_split"] + delta["k_combine"] <= 3
        return out[mm.GUARD:-mm.GUARD].copy().view(mm.RECORD_DTYPE).reshape(-1)


@pytest.fixture(scope="module")
def box(amd):
    b = Box(amd)
    yield b
    b.f.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_model_and_host(amd, box, name):
    iq, jobs = CASES[name]
    want, tols = model(name)
    got = box.run(iq, jobs, tag=name)
    for g, w, tol in zip(got, want, tols):
        print("%s n=%d form=%d: %s" % (name, g["n"], g["form"], " ".join(
            "%s %.2g/%.2g" % (k, abs(float(g[k]) - float(w[k])), tol[k]) for k in mm.SUMS if np.isfinite(w[k]))))
    mm.assert_records(got, want, tols, name)
    host = amd.Fosphor.measure_host(iq, jobs)
    for k in mm.INTS:
        assert np.array_equal(got[k], host[k]), (name, k)
    again = box.run(iq, jobs, tag=name + " again")
    assert again.tobytes() == got.tobytes(), "the same call twice is bit-identical"
    if name == "mixed257":
        assert len(jobs) == 257 and len(set(want["form"])) == 2
    if name == "nonfinite":
        assert not np.isfinite(got["s_p"][1]) and not np.isfinite(got["s_p"][5]) and got["peak_power"][5] == np.inf
    if name == "planted":
        assert list(got["peak_index"][:2]) == [mm.CHUNK - 1] * 2 and list(got["n_edges"][:2]) == [4, 4]


def test_a_job_alone_and_among_256_others(box):
    """a record depends on its job alone: bit-identical alone and among the other jobs of the call, in both forms"""
    iq, jobs = CASES["mixed257"]
    among = box.run(iq, jobs, tag="among")
    picks = [int(np.flatnonzero(jobs["n"] > mm.WAVE_MAX)[0]), int(np.flatnonzero((jobs["n"] > 64) & (jobs["n"] <= mm.WAVE_MAX))[0]), 7]
    for i in picks:
        alone = box.run(iq, jobs[i:i + 1], tag="alone %d" % i)
        assert alone.tobytes() == among[i:i + 1].tobytes(), i


def test_python_front_end(box):
    import torch
    iq, jobs = CASES["split_n"]
    got = box.run(iq, jobs, tag="split_n")
    d_iq = torch.from_numpy(iq).cuda()
    assert box.f.measure(d_iq, jobs).tobytes() == got.tobytes()
    assert box.f.measure(d_iq.view(torch.complex64).reshape(-1), jobs).tobytes() == got.tobytes()
    assert box.f.measure(d_iq.data_ptr(), jobs, n_samples=len(iq)).tobytes() == got.tobytes()
    with pytest.raises(ValueError):
        box.f.measure(d_iq.data_ptr(), jobs)


def test_einval_table(box):
    """each refused call leaves every record at the sentinel, launches nothing and counts nothing"""
    iq = mm.bursty(20000, 51)
    good = [(0, 10, 0.3), (19990, 10, 0.3), (20000, 0, 0.3), (5, 9000, 0.3)]
    box.run(iq, mm.make_jobs(good), tag="good")

    def refused(rows, **kw):
        rv, out, delta = box.call(iq, mm.make_jobs(rows), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "iq", "jobs", "records"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (mm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=19999)
    refused([(-1, 10, 0.3)]); refused([(0, -1, 0.3)]); refused([(19991, 10, 0.3)]); refused([(20001, 0, 0.3)])
    refused([(11001, 9000, 0.3)]); refused([(2 ** 62, 2 ** 31 - 1, 0.3)])
    refused([good[0], (0, 10, np.nan)])
    refused(good, skew_iq=4); refused(good, skew_rec=4)
    box.run(iq, mm.make_jobs([(11000, 9000, 0.3)]), tag="the last job that fits")


def test_chain_extract_measure_derive(amd, box):
    """a small sc16 stream with a tone burst and a noise burst: extract -> measure(extract jobs, threshold=) -> measure_derive.
    The device's derived values equal those derived from the model's records of the same d_out: ratios to 1e-9 relative (decibels
    to 10 / ln 10 times that), rise, fall and pulses exactly.  The tone's lag-1 estimate is within 1e-5 cycles per output sample
    of the planted frequency (tests/test_measure_cpu.py holds the model on extract_host's output to 1e-6)."""
    import torch
    F = amd.Fosphor
    raw, ejobs, planted = mm.chain_case()
    taps = F.extract_design(mm.CHAIN_DECIM, mm.CHAIN_TAPS, 0.8)
    d_x = torch.from_numpy(raw).cuda()
    views = box.f.extract(d_x, ejobs, taps, iq_format="sc16")
    base = views[0].data_ptr() - 8 * int(ejobs["out_offset"][0])		# extract()'s d_out: the views are slices of one buffer
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    got = box.f.measure(base, ejobs, n_samples=cap, threshold=mm.CHAIN_THRESHOLD)
    out = np.zeros((cap, 2), np.float32)
    for j, v in zip(ejobs, views):
        out[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] = v.cpu().numpy().view(np.float32).reshape(-1, 2)
    jobs = F.measure_jobs(ejobs, threshold=mm.CHAIN_THRESHOLD)
    want = mm.measure(out, jobs)
    mm.assert_records(got, want, mm.tolerance((out, jobs)), "chain")
    rate = 1.0
    dev, ref = F.measure_derive(got, rate), F.measure_derive(want, rate)
    for d, r in zip(dev, ref):
        print(d)
        for k in ("rise", "fall", "pulses", "duty"):
            assert d[k] == r[k], k
        for k in ("mean_power", "coherence", "kurtosis", "circularity", "dc_fraction", "freq_offset"):
            assert abs(d[k] - r[k]) <= 1e-9 * abs(r[k]), (k, d[k], r[k])
        for k in ("mean_db", "peak_db", "papr_db"):
            assert abs(d[k] - r[k]) <= 10.0 / np.log(10.0) * 1e-9, (k, d[k], r[k])
    print("tone %.9f planted %.9f" % (dev[0]["freq_offset"], planted))
    assert abs(dev[0]["freq_offset"] - planted) <= 1e-5
    assert dev[0]["pulses"] == 1 and dev[0]["duty"] == 1.0 and dev[1]["pulses"] > 10 and dev[2]["pulses"] == 1
