"""Depuncture, Viterbi and CRC on the device (include/fosphor_amd_decode.h) against the numpy statement (tests/decode_model.py)
and against fosphor_amd_decode_host: records and bytes bit for bit, tobytes().

The bits go into a sentinel-filled buffer in which GUARD bytes before, behind and between the jobs' owned ranges belong to no job,
and the records into a sentinel-filled buffer with one record more than there are jobs; both are compared whole with the model's
image, so a byte or a record written outside a job's range fails like a wrong one.  Every run ends by checking that the input
buffer is bit-identical, that the instance's ring position, waterfall and spectrum are untouched (the method of
tests/test_gpu_decide.py) and that the stats delta names the kernels that ran, at most four launches per call.

Seams of the kernels (the input sets are dm.cases()):
  seams         T = 0, 1, k - 2, k - 1, k, 63, 64, 65, 127, 128, 129, 4095, 4096 and 4097 at k = 3, 5 and 7 (4 at rate 1/3), the
                codes, puncture patterns (none, 2/3, 3/4, 7/8, period 16), orders, CRC widths and TERMINATED taking turns, over
                random bytes: every second coded bit an error, ties abound, bits above b set; input offsets 0 .. 3 mod 4; a job
                that ends on the buffer's last byte.
  codes         every code and pattern at every order: with M = 8 a symbol's three bits straddle the steps.
  frames        encoded frames with channel errors, every CRC width held and failing, SHORT.
  max_steps     one job of MAX_STEPS.
  full_table    MAX_JOBS shuffled jobs with n <= 40, every 11th with n = 0.
test_call_limit runs dm.call_limit_case(), 64 jobs of MAX_STEPS, between two small calls on an instance of its own."""
import errno
import os

import numpy as np
import pytest

import decode_model as dm
from test_decode_cpu import CAP, N_SYM, changed, chain_burst, good_jobs, refusal_rows

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a
SENTINEL32 = 0x5a5a5a5a
CASES = dm.cases()
W = dm.RECORD_WORDS
KERNELS = ("k_bits", "k_acs", "k_trace", "k_rec")


def model(name):
    """the model's records and its image of a case's output buffer, computed once a session"""
    return dm.image(CASES[name], SENTINEL, key=name)


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the decode call through the C ABI"""

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

    def call(self, case, n_bytes=None, n_jobs=None, cap=None, null=(), skew=None, sym_at=None):
        """-> (return value, the records buffer as uint32 [(n_jobs + 1) * 16], the whole output buffer as uint8 [size], delta of
        the stats).  cap: out_capacity, GUARD bytes of the buffer lie behind it; skew: (pointer name, bytes); sym_at: (device
        pointer, n_bytes) of symbols that lie on the device already"""
        import torch
        self.save()
        sym = np.ascontiguousarray(case[0], np.uint8)
        jobs = np.ascontiguousarray(case[1], dm.JOB_DTYPE)
        size = dm.capacity(jobs) if cap is None else max(cap, 0) + dm.GUARD
        d_sym = torch.from_numpy(sym).cuda() if len(sym) else torch.zeros(8, dtype=torch.uint8, device="cuda")
        d_out = torch.full(((size + 15) // 8,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda").view(torch.uint8)
        d_rec = torch.full(((len(jobs) + 1) * W,), SENTINEL32, dtype=torch.int32, device="cuda")
        ptr = {"self": self.f.h, "sym": d_sym.data_ptr(), "jobs": jobs.ctypes.data, "records": d_rec.data_ptr(), "out": d_out.data_ptr()}
        count = len(sym)
        if sym_at:
            ptr["sym"], count = sym_at
        for k in null:
            ptr[k] = None
        if skew:
            ptr[skew[0]] += skew[1]
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.decode_stats()
        rv = self.f.L.fosphor_amd_decode(ptr["self"], ptr["sym"], count if n_bytes is None else n_bytes, ptr["jobs"],
                                         len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"], size if cap is None else cap)
        after = self.f.decode_stats()
        out = d_out.cpu().numpy()
        rec = d_rec.cpu().numpy().view(np.uint32)
        assert np.all(out[size:] == SENTINEL)
        if len(sym) and not sym_at:
            assert d_sym.cpu().numpy().tobytes() == sym.tobytes(), "the input buffer was written"
        self.assert_untouched()
        return rv, rec, out[:size], {k: after[k] - before[k] for k in after}

    def run(self, case, tag="", **kw):
        """a call that must succeed: the stats -> (records, the whole output buffer)"""
        rv, rec, out, delta = self.call(case, **kw)
        assert rv == 0, tag
        jobs = case[1]
        assert np.all(rec[W * len(jobs):] == SENTINEL32), "a record beyond the jobs' was written"
        records = rec[:W * len(jobs)].view(dm.RECORD_DTYPE)
        assert delta == dm.expected_stats(jobs), (tag, delta)
        assert sum(delta[k] for k in KERNELS) <= 4
        return records, out


def bytes_of(buf, job):
    at = int(job["out_offset"])
    return buf[at:at + dm.job_owned(job)]


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
    host_rec, host_views = amd.Fosphor.decode_host(case[0], jobs)
    assert got_rec.tobytes() == host_rec.tobytes(), "records bit-identical to fosphor_amd_decode_host"
    for v, j in zip(host_views, jobs):
        assert bytes_of(got, j)[:len(v)].tobytes() == v.tobytes(), "bit-identical to fosphor_amd_decode_host"
    again_rec, again = box.run(case, tag=name + " again")
    assert again.tobytes() == got.tobytes() and again_rec.tobytes() == got_rec.tobytes(), "the same call twice is bit-identical"
    if name == "frames":
        assert {dm.OK, dm.CRC_FAIL, dm.SHORT} == set(got_rec["status"])
    if name == "max_steps":
        assert (got_rec["n_steps"][0], got_rec["status"][0], got_rec["metric"][0]) == (dm.MAX_STEPS, dm.OK, 2 * dm.MAX_STEPS // 50)


def test_which_kernels_ran(box):
    """jobs with steps: all four; jobs without a step: k_dcd_rec alone, and nothing but the records is written"""
    ran = lambda delta: tuple(delta[k] for k in KERNELS)
    rv, rec, out, delta = box.call(CASES["codes"])
    assert rv == 0 and ran(delta) == (1, 1, 1, 1), delta
    sym = np.arange(64, dtype=np.uint8)
    none = (sym, dm.place([dm.make_job(3, 0, 0, 4, dm.K7, dm.P_NONE, dm.CRC16), dm.make_job(64, 0, 0, 8, dm.K3, dm.P_34, dm.CRC_NONE, 0, 1)]))
    rv, rec, out, delta = box.call(none)
    assert rv == 0 and ran(delta) == (0, 0, 0, 1), delta
    want = dm.decode(none)[0]
    assert rec[:2 * W].tobytes() == want.tobytes() and np.all(out == SENTINEL) and list(want["status"]) == [dm.SHORT, dm.OK]
    # a job without a step among jobs with steps
    mixed = (sym, dm.place([dm.make_job(0, 0, 40, 4, dm.K7, dm.P_NONE), dm.make_job(5, 0, 0, 4, dm.K7, dm.P_NONE),
                            dm.make_job(1, 0, 5, 2, dm.K7, dm.P_NONE, dm.CRC8, 0, 1)]))
    got_rec, got = box.run(mixed, tag="mixed")
    want_rec, want = dm.image(mixed, SENTINEL)
    assert got_rec.tobytes() == want_rec.tobytes() and got.tobytes() == want.tobytes()


def test_a_job_alone_among_others_and_shuffled(box):
    """a record and a job's bytes depend on their job alone: bit-identical alone, among the other jobs of the call, and with the
    table in another order (the outputs keep their places, the work-groups change theirs)"""
    sym, jobs = CASES["codes"]
    among_rec, among = box.run((sym, jobs), tag="among")
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = box.run((sym, jobs[order]), tag="shuffled")
    assert shuffled.tobytes() == among.tobytes() and shuffled_rec.tobytes() == among_rec[order].tobytes()
    for i in (0, 7, 20, len(jobs) - 1):
        alone_rec, alone = box.run((sym, jobs[i:i + 1]), tag="alone %d" % i)
        assert alone_rec[0].tobytes() == among_rec[i].tobytes(), i
        assert bytes_of(alone, jobs[i]).tobytes() == bytes_of(among, jobs[i]).tobytes(), i


def test_python_front_end(box):
    import torch
    sym, jobs = CASES["frames"]
    want_rec, want = dm.decode((sym, jobs))
    d_sym = torch.from_numpy(sym).cuda()
    for records, views in (box.f.decode(d_sym, jobs), box.f.decode(d_sym.data_ptr(), jobs, n_bytes=len(sym))):
        assert records.dtype == dm.RECORD_DTYPE and records.tobytes() == want_rec.tobytes()
        assert len(views) == len(jobs)
        for v, w, r in zip(views, want, records):
            assert v.dtype == torch.uint8 and len(v) == (r["n_bits"] + 7) // 8 and v.cpu().numpy().tobytes() == w[:len(v)].tobytes()
    with pytest.raises(ValueError):
        box.f.decode(d_sym.data_ptr(), jobs)
    with pytest.raises(ValueError):
        box.f.decode(d_sym.to(torch.int32), jobs)


def test_einval_table(box):
    """each refused call leaves every byte and record at the sentinel, launches nothing and counts nothing (the rows of
    tests/test_decode_cpu.py)"""
    sym = np.random.default_rng(91).integers(0, 256, N_SYM).astype(np.uint8)
    good = good_jobs()
    rec, out = box.run((sym, good), tag="good", cap=CAP)
    want_rec, want = dm.image((sym, good), SENTINEL)
    assert rec.tobytes() == want_rec.tobytes() and out[:CAP].tobytes() == want[:CAP].tobytes() and np.all(out[CAP:] == SENTINEL)

    def refused(jobs, **kw):
        kw.setdefault("cap", CAP)
        rv, rec, out, delta = box.call((sym, jobs), **kw)
        assert rv == EINVAL, (jobs, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "sym", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused(np.repeat(good[2:3], dm.MAX_JOBS + 1))
    refused(good, n_bytes=-1); refused(good, n_bytes=2999); refused(good, cap=-1); refused(good, cap=CAP - 8)
    for row in refusal_rows():
        refused(changed(good[:1], **row))
    refused(np.concatenate([good[:1], changed(good[1:2], out_offset=56)]))
    refused(np.concatenate([changed(good[1:2], out_offset=200), changed(good[:1], out_offset=168)]))
    for name, by in (("records", 4), ("out", 4), ("out", 1)):
        refused(good, skew=(name, by))
    long = dm.make_job(0, 0, N_SYM, 8, dm.K3, (16, (1, 0, 0)), dm.CRC_NONE, dm.MAX_STEPS, 0)
    many = np.repeat(long, 65)
    many["out_offset"] = 8192 * np.arange(65)
    many["steps"][64] = 1
    refused(many, cap=65 * 8192)						# 2^22 + 1 steps in the call
    # d_sym needs no alignment: the same symbols a byte further on give the same bits
    rec1, out1 = box.run((sym, changed(good[:1], offset=1)), tag="aligned", cap=CAP)
    import torch
    d = torch.from_numpy(np.concatenate([np.zeros(7, np.uint8), sym])).cuda()
    rec2, out2 = box.run((sym, changed(good[:1], offset=1)), tag="odd pointer", cap=CAP, sym_at=(d.data_ptr() + 7, N_SYM))
    assert rec1.tobytes() == rec2.tobytes() and out1.tobytes() == out2.tobytes()


_HOST = {}


def host_image(amd, case, key):
    """(records, the whole output buffer as fosphor_amd_decode_host leaves it, SENTINEL wherever no job owns a byte), once a session"""
    if key not in _HOST:
        jobs = case[1]
        records, views = amd.Fosphor.decode_host(case[0], jobs)
        out = np.full(dm.capacity(jobs), SENTINEL, np.uint8)
        for j, r, v in zip(jobs, records, views):
            at = int(j["out_offset"])
            out[at:at + dm.owned(r["n_bits"])] = 0
            out[at:at + len(v)] = v
        _HOST[key] = (records, out)
    return _HOST[key]


def test_call_limit(amd):
    """a call of exactly MAX_CALL_STEPS (dm.call_limit_case(): 64 jobs of MAX_STEPS, 32 MiB of survivor decisions, 4 MiB of codes,
    step0 up to 2^22 - 2^16) on a fresh instance, between two small calls: the scratch grows behind a small call and is reused by
    one.  All three are bit-identical to fosphor_amd_decode_host, the whole output and records buffers compared, at most one
    launch a kernel; the job with the largest step0 gives the same record and bytes alone; one step more is refused, writes
    nothing, launches nothing and counts nothing"""
    import torch
    free, total = torch.cuda.mem_get_info()
    if free < 2 ** 30:
        pytest.skip("the call wants 1 GiB of device memory free: %d of %d bytes are" % (free, total))
    small, limit = CASES["frames"], dm.call_limit_case()
    jobs = limit[1]
    assert sum(dm.shape(j)[0] for j in jobs) == dm.MAX_CALL_STEPS and len(jobs) == 64
    b = Box(amd)
    try:
        for tag, case, key in (("small", small, "frames"), ("limit", limit, "call_limit"), ("small again", small, "frames")):
            want_rec, want = host_image(amd, case, key)
            rv, raw, got, delta = b.call(case)
            assert rv == 0, tag
            assert np.all(raw[W * len(case[1]):] == SENTINEL32), "a record beyond the jobs' was written"
            got_rec = raw[:W * len(case[1])].view(dm.RECORD_DTYPE)
            assert delta == dm.expected_stats(case[1]) and all(delta[k] == 1 for k in KERNELS), (tag, delta)
            explain(got_rec, want_rec, got, want, case[1])
            assert got_rec.tobytes() == want_rec.tobytes(), tag + ": records bit-identical to fosphor_amd_decode_host"
            assert got.tobytes() == want.tobytes(), tag + ": bytes bit-identical to fosphor_amd_decode_host, every other byte at the sentinel"
            if tag == "limit":
                limit_rec, limit_out = got_rec, got
        last = len(jobs) - 1							# the table's last job: step0 = 63 MAX_STEPS
        alone_rec, alone = b.run((limit[0], jobs[last:]), tag="alone")
        assert alone_rec[0].tobytes() == limit_rec[last].tobytes()
        assert bytes_of(alone, jobs[last]).tobytes() == bytes_of(limit_out, jobs[last]).tobytes()
        more = dm.one_step_more(limit)
        rv, rec, out, delta = b.call(more)
        assert rv == EINVAL and np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")
    finally:
        b.f.close()


FAR_BYTES = 2 ** 31 + 2 ** 20


def test_far_offset(box):
    """the method of tests/test_gpu_job_far.py: the symbols of the "codes" case copied 2^31 + 2^19 + 3 bytes into a buffer of
    2^31 + 2^20 bytes, every job's offset moved by that, decoy bytes where an offset cut to 31 or 32 bits would look: records and
    bits are bit-identical to the near run, the input and the decoys are unchanged"""
    import torch
    free, total = torch.cuda.mem_get_info()
    if free < FAR_BYTES + 2 ** 30:
        pytest.skip("the far buffer takes %d bytes and wants %d free: %d of %d bytes are" % (FAR_BYTES, FAR_BYTES + 2 ** 30, free, total))
    sym, jobs = CASES["codes"]
    near_rec, near = box.run((sym, jobs), tag="near")
    base = 2 ** 31 + 2 ** 19 + 3
    big = torch.empty(FAR_BYTES, dtype=torch.uint8, device="cuda")
    decoy = torch.from_numpy(np.ascontiguousarray(sym[::-1]) ^ np.uint8(0x15)).cuda()
    aliases = sorted({base % 2 ** 31, base % 2 ** 32, base - 2 ** 31} - {base})
    for a in aliases:
        big[a:a + len(sym)].copy_(decoy)
    big[base:base + len(sym)].copy_(torch.from_numpy(sym).cuda())
    far_jobs = jobs.copy()
    far_jobs["offset"] += base
    assert far_jobs["offset"].min() > 2 ** 31
    far_rec, far = box.run((sym, far_jobs), tag="far", sym_at=(big.data_ptr(), FAR_BYTES))
    assert far_rec.tobytes() == near_rec.tobytes() and far.tobytes() == near.tobytes(), "the far run differs from the near one"
    assert big[base:base + len(sym)].cpu().numpy().tobytes() == sym.tobytes(), "the input was written"
    for a in aliases:
        assert torch.equal(big[a:a + len(sym)], decoy), "a decoy was written"
    del big
    torch.cuda.empty_cache()


def test_chain_decide_decode(amd, box):
    """the synthetic QPSK burst of tests/test_decode_cpu.py: decide on the device, decode over decide's device buffer by the jobs
    that decode_jobs() makes; records and bits are the host chain's, whose values (word at 16, metric 4, CRC 0x77fb held) are
    asserted as they are"""
    import torch
    import decide_model as dec
    F = amd.Fosphor
    iq, word, info, payload = chain_burst()
    djobs = dec.make_jobs([(0, 0, len(iq), 4, dec.UW, 0, 32, 0, 0, 4)])
    code = dict(k=7, polys=(0o171, 0o133), period=3, punct=(0b011, 0b101), steps=422, flags="terminated", crc_width=16, crc_poly=0x1021,
                crc_init=0xffff)
    drec, dviews = box.f.decide(torch.from_numpy(iq).cuda(), djobs, word)
    jobs = F.decode_jobs(djobs, drec, 32, **code)
    before = box.f.decode_stats()
    rec, views = box.f.decode(dviews[0].data_ptr() - int(djobs["out_offset"][0]), jobs, n_bytes=dec.owned(len(iq)))
    after = box.f.decode_stats()
    assert {k: after[k] - before[k] for k in after} == dm.expected_stats(jobs)
    hdrec, hdviews = F.decide_host(iq, djobs, word)
    assert drec.tobytes() == hdrec.tobytes()
    sym = np.zeros(dec.owned(len(iq)), np.uint8)
    sym[:len(iq)] = hdviews[0]
    hjobs = F.decode_jobs(djobs, hdrec, 32, **code)
    assert hjobs.tobytes() == jobs.tobytes()
    want_rec, want = F.decode_host(sym, hjobs)
    assert rec.tobytes() == want_rec.tobytes() and views[0].cpu().numpy().tobytes() == want[0].tobytes()
    assert rec.tobytes() == dm.decode((sym, jobs))[0].tobytes()
    assert (rec["status"][0], rec["metric"][0], rec["crc_calc"][0], rec["crc_recv"][0], rec["n_bits"][0]) == (dm.OK, 4, 0x77fb, 0x77fb, 416)
    assert list(dm.unpack(views[0].cpu().numpy(), len(info))) == list(info), "the decoded bits are the planted ones"
