"""Reed-Solomon outer decoding on the device (include/fosphor_amd_rs.h) against the numpy statement (tests/rs_model.py) and against
fosphor_amd_rs_host: records and bytes bit for bit, tobytes().

The data bytes go into a sentinel-filled buffer in which GUARD bytes before, behind and between the jobs' owned ranges belong to
no job, and the records into a sentinel-filled buffer with one record more than there are jobs; both are compared whole with the
model's image, so a byte or a record written outside a job's range fails like a wrong one.  Every run ends by checking that the
input buffer is bit-identical, that the instance's ring position, waterfall and spectrum are untouched (the method of
tests/test_gpu_decode.py) and that the stats delta names the kernels that ran, at most four launches per call.

Seams of the kernels (the input sets are rm.cases()):
  seams         n_code n_roots + 1, 63, 64, 65, 127, 128, 129, 254 and 255 (the halves of k_rs_syn, the four rounds of the root
                search), n_roots 2 .. 32, depths 1 .. 16, 0, 1, t, t + 1 errors and every byte wrong, errors at the first and the
                last position, in the parity only, of value 0xff; input offsets 0 .. 7 mod 8; both fields, both scramble flags.
  over_t        t + 1 and t + 2 errors: failures and miscorrections.
  ccsds, dvb    the two codes everyone knows.
  full_table    MAX_JOBS shuffled jobs of small codes, every 11th clean.
  all_clean     k_rs_fix is not launched.
test_call_limit runs rm.call_limit_case(), MAX_CALL_CODEWORDS codewords, between two small calls on an instance of its own."""
import errno
import os

import numpy as np
import pytest

import rs_model as rm
from test_rs_cpu import CAP, N_IN, changed, chain_symbols, good_jobs, refusal_rows

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a
SENTINEL32 = 0x5a5a5a5a
CASES = rm.cases()
W = rm.RECORD_WORDS
KERNELS = ("k_syn", "k_fix", "k_out", "k_rec")


def model(name):
    """the model's records and its image of a case's output buffer, computed once a session"""
    return rm.image(CASES[name], SENTINEL, key=name)


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the rs call through the C ABI"""

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

    def call(self, case, n_bytes=None, n_jobs=None, cap=None, null=(), skew=None, in_at=None):
        """-> (return value, the records buffer as uint32 [(n_jobs + 1) * 16], the whole output buffer as uint8 [size], delta of
        the stats).  cap: out_capacity, GUARD bytes of the buffer lie behind it; skew: (pointer name, bytes); in_at: (device
        pointer, n_bytes) of bytes that lie on the device already"""
        import torch
        self.save()
        data = np.ascontiguousarray(case[0], np.uint8)
        jobs = np.ascontiguousarray(case[1], rm.JOB_DTYPE)
        size = rm.capacity(jobs) if cap is None else max(cap, 0) + rm.GUARD
        d_in = torch.from_numpy(data).cuda() if len(data) else torch.zeros(8, dtype=torch.uint8, device="cuda")
        d_out = torch.full(((size + 15) // 8,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda").view(torch.uint8)
        d_rec = torch.full(((len(jobs) + 1) * W,), SENTINEL32, dtype=torch.int32, device="cuda")
        ptr = {"self": self.f.h, "in": d_in.data_ptr(), "jobs": jobs.ctypes.data, "records": d_rec.data_ptr(), "out": d_out.data_ptr()}
        count = len(data)
        if in_at:
            ptr["in"], count = in_at
        for k in null:
            ptr[k] = None
        if skew:
            ptr[skew[0]] += skew[1]
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.rs_stats()
        rv = self.f.L.fosphor_amd_rs(ptr["self"], ptr["in"], count if n_bytes is None else n_bytes, ptr["jobs"],
                                     len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"], size if cap is None else cap)
        after = self.f.rs_stats()
        out = d_out.cpu().numpy()
        rec = d_rec.cpu().numpy().view(np.uint32)
        assert np.all(out[size:] == SENTINEL)
        if len(data) and not in_at:
            assert d_in.cpu().numpy().tobytes() == data.tobytes(), "the input buffer was written"
        self.assert_untouched()
        return rv, rec, out[:size], {k: after[k] - before[k] for k in after}

    def run(self, case, tag="", **kw):
        """a call that must succeed: the stats -> (records, the whole output buffer)"""
        rv, rec, out, delta = self.call(case, **kw)
        assert rv == 0, tag
        jobs = case[1]
        assert np.all(rec[W * len(jobs):] == SENTINEL32), "a record beyond the jobs' was written"
        records = rec[:W * len(jobs)].view(rm.RECORD_DTYPE)
        assert delta == rm.expected_stats(records), (tag, delta)
        assert sum(delta[k] for k in KERNELS) <= 4
        return records, out


def bytes_of(buf, job):
    at = int(job["out_offset"])
    return buf[at:at + rm.job_owned(job)]


def explain(got_rec, want_rec, got, want, jobs):
    """print the first records and bytes that differ, with the job that owns them"""
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    for i in np.flatnonzero(got != want)[:8]:
        print("byte %d got %s want %s" % (i, got[i], want[i]))


@pytest.fixture(scope="module")
def box(amd):
    b = Box(amd)
    yield b
    b.f.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_model_and_host(amd, box, name):
    case = CASES[name]
    jobs = case[1]
    want_rec, want = model(name)
    got_rec, got = box.run(case, tag=name)
    explain(got_rec, want_rec, got, want, jobs)
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical to the model"
    assert got.tobytes() == want.tobytes(), "bytes bit-identical to the model, every other byte at the sentinel"
    host_rec, host_views = amd.Fosphor.rs_host(case[0], jobs)
    assert got_rec.tobytes() == host_rec.tobytes(), "records bit-identical to fosphor_amd_rs_host"
    for v, j in zip(host_views, jobs):
        assert bytes_of(got, j)[:len(v)].tobytes() == v.tobytes(), "bit-identical to fosphor_amd_rs_host"
    again_rec, again = box.run(case, tag=name + " again")
    assert again.tobytes() == got.tobytes() and again_rec.tobytes() == got_rec.tobytes(), "the same call twice is bit-identical"
    if name == "over_t":
        assert {rm.OK, rm.FAIL} == set(got_rec["status"])


def test_which_kernels_ran(box):
    """codewords with errors: all four; every codeword clean: k_rs_fix is not launched, and the stats show it"""
    ran = lambda delta: tuple(delta[k] for k in KERNELS)
    rv, rec, out, delta = box.call(CASES["ccsds"])
    assert rv == 0 and ran(delta) == (1, 1, 1, 1), delta
    assert (delta["calls"], delta["codewords"], delta["clean"], delta["failed"]) == (1, 20, 7, 1), delta
    rv, rec, out, delta = box.call(CASES["all_clean"])
    assert rv == 0 and ran(delta) == (1, 0, 1, 1), delta
    assert (delta["codewords"], delta["clean"], delta["failed"]) == (9, 9, 0), delta
    want_rec, want = model("all_clean")
    assert rec[:3 * W].tobytes() == want_rec.tobytes() and out.tobytes() == want.tobytes()
    # the scratch of the clean call holds the corrections of the call before it: nothing of them is applied
    rv, rec2, out2, delta = box.call(CASES["ccsds"])
    rv, rec3, out3, delta = box.call(CASES["all_clean"])
    assert rec3.tobytes() == rec.tobytes() and out3.tobytes() == out.tobytes()


def test_a_job_alone_among_others_and_shuffled(box):
    """a record and a job's bytes depend on their job alone: bit-identical alone, among the other jobs of the call, and with the
    table in another order (the outputs keep their places, the work-groups change theirs)"""
    buf, jobs = CASES["seams"]
    among_rec, among = box.run((buf, jobs), tag="among")
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = box.run((buf, jobs[order]), tag="shuffled")
    assert shuffled.tobytes() == among.tobytes() and shuffled_rec.tobytes() == among_rec[order].tobytes()
    for i in (0, 7, 20, len(jobs) - 1):
        alone_rec, alone = box.run((buf, jobs[i:i + 1]), tag="alone %d" % i)
        assert alone_rec[0].tobytes() == among_rec[i].tobytes(), i
        assert bytes_of(alone, jobs[i]).tobytes() == bytes_of(among, jobs[i]).tobytes(), i


def test_python_front_end(box):
    import torch
    buf, jobs = CASES["dvb"]
    want_rec, want = rm.decode((buf, jobs))
    d_in = torch.from_numpy(buf).cuda()
    for records, views in (box.f.rs(d_in, jobs), box.f.rs(d_in.data_ptr(), jobs, n_bytes=len(buf))):
        assert records.dtype == rm.RECORD_DTYPE and records.tobytes() == want_rec.tobytes()
        assert len(views) == len(jobs)
        for v, w, r in zip(views, want, records):
            assert v.dtype == torch.uint8 and len(v) == r["n_data"] and v.cpu().numpy().tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        box.f.rs(d_in.data_ptr(), jobs)
    with pytest.raises(ValueError):
        box.f.rs(d_in.to(torch.int32), jobs)


def test_einval_table(box):
    """each refused call leaves every byte and record at the sentinel, launches nothing and counts nothing (the rows of
    tests/test_rs_cpu.py)"""
    data = np.random.default_rng(91).integers(0, 256, N_IN).astype(np.uint8)
    good = good_jobs()
    rec, out = box.run((data, good), tag="good", cap=CAP)
    want_rec, want = rm.image((data, good), SENTINEL)
    assert rec.tobytes() == want_rec.tobytes() and out[:CAP].tobytes() == want[:CAP].tobytes() and np.all(out[CAP:] == SENTINEL)

    def refused(jobs, **kw):
        kw.setdefault("cap", CAP)
        rv, rec, out, delta = box.call((data, jobs), **kw)
        assert rv == EINVAL, (jobs, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "in", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused(np.repeat(good[2:3], rm.MAX_JOBS + 1))
    refused(good, n_bytes=-1); refused(good, n_bytes=N_IN - 1); refused(good, cap=-1); refused(good, cap=CAP - 8)
    for row in refusal_rows():
        refused(changed(good[:1], **row))
    refused(np.concatenate([good[:1], changed(good[1:2], out_offset=1112)]))
    refused(np.concatenate([changed(good[1:2], out_offset=2000), changed(good[2:3], out_offset=1984)]))
    for name, by in (("records", 4), ("out", 4), ("out", 1)):
        refused(good, skew=(name, by))
    # d_in needs no alignment: the same bytes at an odd pointer give the same records and bytes
    rec1, out1 = box.run((data, changed(good[:1], offset=1)), tag="aligned", cap=CAP)
    import torch
    d = torch.from_numpy(np.concatenate([np.zeros(7, np.uint8), data])).cuda()
    rec2, out2 = box.run((data, changed(good[:1], offset=1)), tag="odd pointer", cap=CAP, in_at=(d.data_ptr() + 7, N_IN))
    assert rec1.tobytes() == rec2.tobytes() and out1.tobytes() == out2.tobytes()


def test_call_limit(amd):
    """a call of exactly MAX_CALL_CODEWORDS (rm.call_limit_case(): MAX_JOBS frames of MAX_DEPTH codewords) on a fresh instance,
    between two small calls: the scratch grows behind a small call and is reused by one.  All three are bit-identical to
    fosphor_amd_rs_host; one job more is refused, writes nothing, launches nothing and counts nothing"""
    frame, jobs, data = rm.call_limit_case()
    small = CASES["dvb"]
    b = Box(amd)
    try:
        for tag, case in (("small", small), ("limit", (frame, jobs)), ("small again", small)):
            want_rec, want_views = amd.Fosphor.rs_host(case[0], case[1])
            got_rec, got = b.run(case, tag=tag)
            assert got_rec.tobytes() == want_rec.tobytes(), tag + ": records bit-identical to fosphor_amd_rs_host"
            want = np.full(len(got), SENTINEL, np.uint8)
            for j, v in zip(case[1], want_views):
                at = int(j["out_offset"])
                want[at:at + rm.job_owned(j)] = 0
                want[at:at + len(v)] = v
            assert got.tobytes() == want.tobytes(), tag + ": bytes bit-identical to fosphor_amd_rs_host, every other byte at the sentinel"
            if tag == "limit":
                assert got_rec["n_codewords"].sum() == rm.MAX_CALL_CODEWORDS and (got_rec["corrected_symbols"] == 1).all()
        more = rm.place([jobs[:1]] * (rm.MAX_JOBS + 1), gap=0)
        rv, rec, out, delta = b.call((frame, more))
        assert rv == EINVAL and np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")
    finally:
        b.f.close()


def test_chain_decode_rs(amd, box):
    """the frame of tests/test_rs_cpu.py: decode on the device, rs over decode's device buffer by the jobs that rs_jobs() makes, no
    host copy in between; records and bytes are the host chain's, and the data is the planted one although decode's own output has
    byte errors"""
    import torch
    F = amd.Fosphor
    sym, data, frame, job = chain_symbols()
    code = dict(flags="descramble_out", scr_width=15, scr_taps=0x6000, scr_init=0x4a80, **F.RS_DVB)
    drec, dviews = box.f.decode(torch.from_numpy(sym).cuda(), job)
    jobs = F.rs_jobs(job["out_offset"], drec["n_bits"], 204, **code)
    before = box.f.rs_stats()
    base = dviews[0].data_ptr() - int(job["out_offset"][0])
    rec, views = box.f.rs(base, jobs, n_bytes=int(job["out_offset"][0]) + 208)
    after = box.f.rs_stats()
    assert {k: after[k] - before[k] for k in after} == rm.expected_stats(rec)
    hdrec, hdviews = F.decode_host(sym, job)
    assert drec.tobytes() == hdrec.tobytes() and dviews[0].cpu().numpy().tobytes() == hdviews[0].tobytes()
    inner = np.zeros(int(job["out_offset"][0]) + 208, np.uint8)
    inner[int(job["out_offset"][0]):][:len(hdviews[0])] = hdviews[0]
    want_rec, want = F.rs_host(inner, jobs)
    assert rec.tobytes() == want_rec.tobytes() and views[0].cpu().numpy().tobytes() == want[0].tobytes()
    wrong = int((hdviews[0][:204] != frame).sum())
    assert wrong >= 1 and rec["status"][0] == rm.OK and rec["corrected_symbols"][0] == wrong
    assert views[0].cpu().numpy().tobytes() == data.tobytes(), "the RS output is the planted data"
