"""Burst IQ demodulated on the device (include/fosphor_amd_demod.h) against the numpy statement (tests/demod_model.py) and against
fosphor_amd_demod_host: bit for bit, tobytes().

The output goes into a sentinel-filled buffer in which GUARD floats before, behind and between the jobs' ranges belong to no job;
the whole buffer is compared with the model's image of it, so a float written outside a job's range fails like a wrong one.  Every
run ends by checking that the input buffer is bit-identical, that the instance's ring position, waterfall and spectrum are untouched
(the method of tests/test_gpu_measure.py) and that the stats delta names the kernels that ran, at most two launches per call.

Seams of the kernels (the input sets are dm.cases()):
  both            a work-group loads its span by 16-byte pairs from the first 16-byte boundary: input offsets 0, 1, 2, 3, even and
                  odd lengths, odd and even out_offsets, a job that ends on the buffer's last sample; n = 0, 1, 2.
  k_demod_direct  256 lanes, TILE values a work-group: n = 63 .. 65, 255 .. 257, 2047 .. 2049, 4097, 3 TILE + 5; in FM the last
                  value of a tile takes y[m + 1] from beyond the tile.
  k_demod_avg     TILE / L outputs a work-group: L = 2, 64, 256 divide TILE, L = 3, 7, 255 leave a remainder; FM with n = 1, L,
                  L + 1; one lane per output (L = 256: 8 lanes) and four outputs per lane (L = 2).
The refusal "more than 2^31 - 1 work-groups in one form" needs MAX_JOBS jobs of 2^31 - 1 samples, 16 GiB of IQ: it is decided by
the host code that tests/test_demod_cpu.py drives, and has no case here."""
import errno
import os

import numpy as np
import pytest

import demod_model as dm
import measure_model as mm

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a5a5a5a
CASES = dm.cases()
_MODEL = {}


def model(name):
    """the model's image of a case's output buffer, computed once"""
    if name not in _MODEL:
        _MODEL[name] = dm.image(*CASES[name], SENTINEL)
    return _MODEL[name]


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the demod call through the C ABI"""

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

    def call(self, iq, jobs, n_samples=None, n_jobs=None, cap=None, null=(), skew_iq=0, skew_out=0):
        """-> (return value, the whole output buffer as uint32, delta of the stats).  cap: out_capacity, GUARD floats of the
        buffer lie behind it; skew_*: bytes added to a pointer"""
        import torch
        self.save()
        iq = np.ascontiguousarray(iq, np.float32).reshape(-1, 2)
        jobs = np.ascontiguousarray(jobs, dm.JOB_DTYPE)
        d_iq = torch.from_numpy(iq if len(iq) else np.zeros((1, 2), np.float32)).cuda()
        size = dm.capacity(jobs) if cap is None else max(cap, 0) + dm.GUARD
        d_out = torch.full((size + 1,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.demod_stats()
        rv = self.f.L.fosphor_amd_demod(None if "self" in null else self.f.h, None if "iq" in null else d_iq.data_ptr() + skew_iq,
                                        len(iq) if n_samples is None else n_samples,
                                        None if "jobs" in null else jobs.ctypes.data, len(jobs) if n_jobs is None else n_jobs,
                                        None if "out" in null else d_out.data_ptr() + skew_out, size if cap is None else cap)
        after = self.f.demod_stats()
        out = d_out.cpu().numpy().view(np.uint32)
        assert out[size] == SENTINEL
        if len(iq):
            assert d_iq.cpu().numpy().tobytes() == iq.tobytes(), "the input buffer was written"
        self.assert_untouched()
        return rv, out[:size], {k: after[k] - before[k] for k in after}

    def run(self, iq, jobs, tag="", **kw):
        """a call that must succeed: the stats -> the whole output buffer"""
        rv, out, delta = self.call(iq, jobs, **kw)
        assert rv == 0, tag
        n_out = np.array([dm.n_out(int(j["mode"]), int(j["n"]), int(j["avg"])) for j in jobs])
        direct = jobs["avg"] == 1
        assert delta == dict(calls=1, k_direct=int((direct & (n_out > 0)).any()), k_avg=int((~direct & (n_out > 0)).any()),
                             jobs_direct=int(direct.sum()), jobs_avg=int((~direct).sum()), samples=int(jobs["n"].sum()),
                             outputs=int(n_out.sum())), (tag, delta)
        assert delta["k_direct"] + delta["k_avg"] <= 2
        return out


def explain(got, want, jobs):
    """print the first floats that differ, with the job that owns them"""
    for i in np.flatnonzero(got != want)[:8]:
        own = [k for k, j in enumerate(jobs) if int(j["out_offset"]) <= i < int(j["out_offset"]) + dm.n_out(int(j["mode"]), int(j["n"]), int(j["avg"]))]
        print("float %d got %08x want %08x job %s" % (i, got[i], want[i], [(k, tuple(jobs[k])) for k in own]))


def outputs(buf, job):
    at = int(job["out_offset"])
    return buf[at:at + dm.n_out(int(job["mode"]), int(job["n"]), int(job["avg"]))]


@pytest.fixture(scope="module")
def box(amd):
    b = Box(amd)
    yield b
    b.f.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_model_and_host(amd, box, name):
    iq, jobs = CASES[name]
    want = model(name)
    got = box.run(iq, jobs, tag=name)
    explain(got, want, jobs)
    assert got.tobytes() == want.tobytes(), "outputs bit-identical to the model, every other float at the sentinel"
    for v, j in zip(amd.Fosphor.demod_host(iq, jobs), jobs):
        assert outputs(got, j).tobytes() == v.tobytes(), "bit-identical to fosphor_amd_demod_host"
    again = box.run(iq, jobs, tag=name + " again")
    assert again.tobytes() == got.tobytes(), "the same call twice is bit-identical"
    if name == "mixed257":
        assert len(jobs) == 257


def test_a_job_alone_and_among_256_others(box):
    """an output depends on its job alone: bit-identical alone and among the other jobs of the call, in both forms"""
    iq, jobs = CASES["mixed257"]
    among = box.run(iq, jobs, tag="among")
    long_ = jobs["n"] > dm.TILE
    picks = [int(np.flatnonzero(long_ & (jobs["avg"] == 1))[0]), int(np.flatnonzero(long_ & (jobs["avg"] > 1))[0]),
             int(np.flatnonzero(~long_ & (jobs["n"] > 300) & (jobs["avg"] > 1) & (jobs["mode"] == dm.FM))[0]), 7]
    for i in picks:
        alone = box.run(iq, jobs[i:i + 1], tag="alone %d" % i)
        assert outputs(alone, jobs[i]).tobytes() == outputs(among, jobs[i]).tobytes(), i


def test_the_cut_rule(box):
    """rule 3 on the device: a job gives, bit for bit, the outputs of the two jobs it is cut into at a multiple of L"""
    iq, jobs, triples = dm.cut_case()
    got = box.run(iq, jobs, tag="cut")
    want = dm.image(iq, jobs, SENTINEL)
    explain(got, want, jobs)
    assert got.tobytes() == want.tobytes()
    for w, a, b, c in triples:
        whole, first, second = outputs(got, jobs[w]), outputs(got, jobs[a]), outputs(got, jobs[b])
        assert len(first) == c and len(first) + len(second) == len(whole) and len(second) >= 1
        assert whole[:c].tobytes() == first.tobytes() and whole[c:].tobytes() == second.tobytes(), (w, c)


def test_python_front_end(box):
    import torch
    iq, jobs = CASES["fm_edges"]
    want = [outputs(model("fm_edges"), j) for j in jobs]
    d_iq = torch.from_numpy(iq).cuda()
    for views in (box.f.demod(d_iq, jobs), box.f.demod(d_iq.view(torch.complex64).reshape(-1), jobs),
                  box.f.demod(d_iq.data_ptr(), jobs, n_samples=len(iq))):
        assert len(views) == len(jobs)
        for v, w in zip(views, want):
            assert v.dtype == torch.float32 and v.cpu().numpy().tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        box.f.demod(d_iq.data_ptr(), jobs)
    with pytest.raises(ValueError):
        box.f.demod(d_iq.double(), jobs)


def test_einval_table(box):
    """each refused call leaves every float at the sentinel, launches nothing and counts nothing"""
    iq = dm.noise(20000, 51)
    good = [(0, 3, 10, dm.POWER, 1), (19990, 13, 10, dm.FM, 1), (20000, 22, 0, dm.PHASE, 1), (5, 22, 9000, dm.PHASE, 4)]
    cap = 22 + 2250
    out = box.run(iq, dm.make_jobs(good), tag="good", cap=cap)
    assert np.all(out[cap:] == SENTINEL) and np.all(out[22:cap] != SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        jobs = dm.make_jobs([r[:5] for r in rows])
        for j, r in zip(jobs, rows):
            j["reserved"] = r[5] if len(r) > 5 else 0
        rv, out, delta = box.call(iq, jobs, **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "iq", "jobs", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (dm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=19999); refused(good, cap=-1); refused(good, cap=cap - 1)
    refused([(-1, 0, 10, 0, 1)]); refused([(0, 0, -1, 0, 1)]); refused([(19991, 0, 10, 0, 1)]); refused([(20001, 0, 0, 0, 1)])
    refused([(11001, 0, 9000, 0, 1)]); refused([(2 ** 62, 0, 2 ** 31 - 1, 0, 1)])
    refused([(0, -1, 10, 0, 1)]); refused([(0, cap + 1, 0, 0, 1)]); refused([(0, 2 ** 62, 10, 0, 1)]); refused([(0, cap - 9, 10, 0, 1)])
    refused([(0, 0, 10, 3, 1)]); refused([(0, 0, 10, -1, 1)]); refused([(0, 0, 10, 0, 0)]); refused([(0, 0, 10, 0, dm.MAX_AVG + 1)])
    refused([(0, 0, 10, 0, 1, 1)])
    refused([(0, 0, 10, dm.POWER, 1), (0, 9, 10, dm.FM, 1)])			# outputs [0, 10) and [9, 18): one float shared
    refused([(0, 30, 100, dm.PHASE, 4), (0, 0, 31, dm.POWER, 1)])		# [30, 55) and [0, 31), given in descending order
    refused(good, skew_iq=4); refused(good, skew_out=2)
    # the last jobs that still fit, in the input and in the output; outputs that touch; jobs without outputs
    ok = [(0, 0, 10, dm.POWER, 1), (0, 10, 10, dm.FM, 1), (11000, cap - 2250, 9000, dm.POWER, 4), (0, cap, 3, dm.FM, 4), (20000, 5, 0, 0, 1)]
    jobs = dm.make_jobs(ok)
    out = box.run(iq, jobs, tag="the last jobs that fit", cap=cap)
    want = dm.image(iq, jobs, SENTINEL)
    assert out[:len(want) - dm.GUARD].tobytes() == want[:-dm.GUARD].tobytes() and np.all(out[cap:] == SENTINEL)
    out = box.run(iq, dm.make_jobs([(0, 7, 1, dm.FM, 1), (3, 7, 5, dm.PHASE, 8)]), tag="no job writes anything", cap=cap)
    assert np.all(out == SENTINEL)


def test_chain_extract_demod(amd, box):
    """measure_model's small sc16 stream with a tone burst and a noise burst: extract -> demod(fm, avg = 1) and demod(power,
    avg = 8) over extract's buffer, both bit-identical to the model run over the same d_out.  The mean of the tone burst's FM trace
    is the planted frequency within 1.992e-7 cycles per output sample: the numpy model over fosphor_amd_extract_host's output of
    this case is off by 9.96e-8 (the stream's noise over 1966 trace values; tests/test_demod_cpu.py::test_chain_on_the_host holds
    that figure), and twice that is allowed."""
    import torch
    F = amd.Fosphor
    raw, ejobs, planted = mm.chain_case()
    taps = F.extract_design(mm.CHAIN_DECIM, mm.CHAIN_TAPS, 0.8)
    d_x = torch.from_numpy(raw).cuda()
    views = box.f.extract(d_x, ejobs, taps, iq_format="sc16")
    base = views[0].data_ptr() - 8 * int(ejobs["out_offset"][0])		# extract()'s d_out: the views are slices of one buffer
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    out = np.zeros((cap, 2), np.float32)
    for j, v in zip(ejobs, views):
        out[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] = v.cpu().numpy().view(np.float32).reshape(-1, 2)
    for mode, avg in (("fm", 1), ("power", 8)):
        jobs = F.demod_jobs(ejobs, mode=mode, avg=avg)
        assert int(jobs["out_offset"][1]) == F.demod_n_out(mode, int(ejobs["n_out"][0]), avg), "back to back"
        before = box.f.demod_stats()
        got = box.f.demod(base, jobs, n_samples=cap)
        after = box.f.demod_stats()
        assert (after["k_direct"] - before["k_direct"], after["k_avg"] - before["k_avg"]) == ((1, 0) if avg == 1 else (0, 1))
        for g, w in zip(got, dm.demod(out, jobs)):
            assert len(w) > 100 and g.cpu().numpy().tobytes() == w.tobytes(), (mode, avg)
        if mode == "fm":
            mean = float(got[0].double().mean())
            print("tone: mean of the FM trace %.10f planted %.10f" % (mean, planted))
            assert abs(mean - planted) <= CHAIN_BOUND


CHAIN_REFERENCE = 9.96e-8		# |mean FM - planted| of the numpy model over extract_host's output of the chain case
CHAIN_BOUND = 2.0 * CHAIN_REFERENCE
