"""Soft values, soft-input Viterbi and CRC on the device (include/fosphor_amd_soft.h) against fosphor_amd_soft_host: records and
bytes bit for bit, tobytes().  (tests/test_soft_cpu.py holds the host statement to the numpy model on the same input sets.)

The bits go into a sentinel-filled buffer in which GUARD bytes before, behind and between the jobs' owned ranges belong to no job,
and the records into a sentinel-filled buffer with one record more than there are jobs; both are compared whole with the host's
image, so a byte or a record written outside a job's range fails like a wrong one.  Every run ends by checking that the input
buffer is bit-identical, that the instance's ring position, waterfall and spectrum are untouched (the method of
tests/test_gpu_decode.py) and that the stats delta names the kernels that ran, one launch a kernel at the most.

Seams of the kernels (the input sets are sm.cases()):
  seams         T = 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257 and 513, twice each, in one call of mixed K, M, rate,
                labeling, rotation, CRC and TERMINATED: across the 64-step block of k_sft_acs and k_sft_trace and the 256-step
                work-group of k_sft_bits; jobs with T = 0 and with n = 0 among them.
  nan           NaN, infinite and zero parts among live symbols; a job of NaN symbols alone.
  max_steps     one job of MAX_STEPS.
  full_table    MAX_JOBS shuffled jobs with n <= 40, every 11th with n = 0.
  edges         a job a crafted value on a rounding or clamp boundary of rule S2, float32 subnormals, NaN correlations, 4- and 8-PSK
                symbols on decision boundaries: the floating-point path of k_sft_bits.
  contract      8-PSK symbols on which a contracted correlation gives another record than rule S2.
test_call_limit runs sm.call_limit_case(), 64 jobs of MAX_STEPS, between two small calls on an instance of its own."""
import errno
import os

import numpy as np
import pytest

import soft_model as sm
from test_soft_cpu import CHAIN_CODE, CHAIN_INFO, CHAIN_UW, chain_burst, chain_jobs

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a
SENTINEL32 = 0x5a5a5a5a
CASES = sm.cases()
W = sm.RECORD_WORDS
KERNELS = ("k_bits", "k_acs", "k_trace", "k_rec")


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


_HOST = {}


def host_image(amd, case, key=None):
    """(records, the whole output buffer as fosphor_amd_soft_host leaves it, SENTINEL wherever no job owns a byte); with a key the
    result is computed once for all the tests of a session"""
    if key is not None and key in _HOST:
        return _HOST[key]
    jobs = case[1]
    records, views = amd.Fosphor.soft_host(case[0], jobs)
    out = np.full(sm.capacity(jobs), SENTINEL, np.uint8)
    for j, r in zip(jobs, records):
        at, own = int(j["out_offset"]), sm.owned(r["n_bits"])
        out[at:at + own] = 0
    for j, v in zip(jobs, views):
        out[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v
    if key is not None:
        _HOST[key] = (records, out)
    return records, out


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the soft call through the C ABI"""

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

    def call(self, case, n_samples=None, n_jobs=None, cap=None, null=(), skew=None, iq_at=None, out_at=None):
        """-> (return value, the records buffer as uint32 [(n_jobs + 1) * 16], the whole output buffer as uint8 [size], delta of
        the stats).  cap: out_capacity, GUARD bytes of the buffer lie behind it; skew: (pointer name, bytes); iq_at: (device
        pointer, n_samples) of symbols that lie on the device already; out_at: (device tensor, capacity) to write into, returned
        as it is"""
        import torch
        self.save()
        iq = np.ascontiguousarray(case[0], np.float32).reshape(-1, 2)
        jobs = np.ascontiguousarray(case[1], sm.JOB_DTYPE)
        size = sm.capacity(jobs) if cap is None else max(cap, 0) + sm.GUARD
        d_iq = torch.from_numpy(iq).cuda() if len(iq) else torch.zeros((1, 2), dtype=torch.float32, device="cuda")
        if out_at:
            d_out, size = out_at
        else:
            d_out = torch.full(((size + 15) // 8,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda").view(torch.uint8)
        d_rec = torch.full(((len(jobs) + 1) * W,), SENTINEL32, dtype=torch.int32, device="cuda")
        ptr = {"self": self.f.h, "iq": d_iq.data_ptr(), "jobs": jobs.ctypes.data, "records": d_rec.data_ptr(), "out": d_out.data_ptr()}
        count = len(iq)
        if iq_at:
            ptr["iq"], count = iq_at
        for k in null:
            ptr[k] = None
        if skew:
            ptr[skew[0]] += skew[1]
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.soft_stats()
        rv = self.f.L.fosphor_amd_soft(ptr["self"], ptr["iq"], count if n_samples is None else n_samples, ptr["jobs"],
                                       len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"], size if cap is None else cap)
        after = self.f.soft_stats()
        rec = d_rec.cpu().numpy().view(np.uint32)
        if out_at:
            out = None
        else:
            out = d_out.cpu().numpy()
            assert np.all(out[size:] == SENTINEL)
            out = out[:size]
        if len(iq) and not iq_at:
            assert d_iq.cpu().numpy().tobytes() == iq.tobytes(), "the input buffer was written"
        self.assert_untouched()
        return rv, rec, out, {k: after[k] - before[k] for k in after}

    def run(self, case, tag="", **kw):
        """a call that must succeed: the stats -> (records, the whole output buffer)"""
        rv, rec, out, delta = self.call(case, **kw)
        assert rv == 0, tag
        jobs = case[1]
        assert np.all(rec[W * len(jobs):] == SENTINEL32), "a record beyond the jobs' was written"
        records = rec[:W * len(jobs)].view(sm.RECORD_DTYPE)
        assert delta == sm.expected_stats(jobs), (tag, delta)
        assert all(delta[k] <= 1 for k in KERNELS), "one launch a kernel"
        return records, out


def bytes_of(buf, job):
    at = int(job["out_offset"])
    return buf[at:at + sm.job_owned(job)]


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
def test_against_host(amd, box, name):
    case = CASES[name]
    jobs = case[1]
    want_rec, want = host_image(amd, case, key=name)
    got_rec, got = box.run(case, tag=name)
    explain(got_rec, want_rec, got, want, jobs)
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical to fosphor_amd_soft_host"
    assert got.tobytes() == want.tobytes(), "bytes bit-identical to fosphor_amd_soft_host, every other byte at the sentinel"
    again_rec, again = box.run(case, tag=name + " again")
    assert again.tobytes() == got.tobytes() and again_rec.tobytes() == got_rec.tobytes(), "the same call twice is bit-identical"
    if name == "seams":
        steps = {int(r["n_steps"]) for r in got_rec}
        assert set(sm.SEAM_STEPS) | {0} <= steps and {sm.OK, sm.CRC_FAIL, sm.SHORT} == set(got_rec["status"])
    if name == "nan":
        assert (got_rec["erasures"] > 0).all() and got_rec["erasures"][-1] == jobs["n"][-1] and got_rec["abs_sum"][-1] == 0
    if name == "max_steps":
        assert (got_rec["n_steps"][0], got_rec["status"][0], got_rec["end_state"][0]) == (sm.MAX_STEPS, sm.OK, 0) and got_rec["metric"][0] > 0
    if name == "full_table":
        assert len(jobs) == sm.MAX_JOBS
    if name == "edges":
        rows = sm.edge_rows()
        assert (got_rec["saturated"] > 0).any() and (got_rec["erasures"] > 0).any() and (got_rec["abs_sum"] == 0).any()
        for (sr, si, order, rot, gray, scale, want, erasures), r in zip(rows, got_rec):
            if want is not None:
                assert (r["abs_sum"], r["saturated"], r["erasures"]) == (abs(want), int(abs(want) == 127), erasures), (sr, si, scale, r)
    if name == "contract":
        plain, fma_re, fma_im = sm.contract_records()
        assert len(jobs) >= 64 and len(plain) == len(jobs), "the jobs that tell a contracted correlation are in the call"
        for i in range(len(jobs)):
            assert got_rec[i].tobytes() == plain[i].tobytes() and got_rec[i].tobytes() not in (fma_re[i].tobytes(), fma_im[i].tobytes()), (i, jobs[i])


def test_which_kernels_ran(amd, box):
    """jobs with steps: all four; a call whose every job has T = 0: k_sft_rec alone, and nothing but the records is written"""
    import decode_model as dm
    ran = lambda delta: tuple(delta[k] for k in KERNELS)
    rv, rec, out, delta = box.call(CASES["nan"])
    assert rv == 0 and ran(delta) == (1, 1, 1, 1), delta
    iq = sm.pairs(np.exp(2j * np.pi * np.arange(64) / 8))
    none = (iq, sm.place([sm.make_job(3, 0, 0, 4, dm.K7, dm.P_NONE, dm.CRC16, 0, sm.GRAY, 2, 5.0),
                          sm.make_job(64, 0, 0, 8, dm.K3, dm.P_34, dm.CRC_NONE, 0, 1, 7, 1.0),
                          sm.make_job(10, 0, 1, 2, dm.K5, dm.P_NONE, dm.CRC_NONE, 0, 0, 1, 1.0)]))		# a symbol, but less than a step
    rv, rec, out, delta = box.call(none)
    assert rv == 0 and ran(delta) == (0, 0, 0, 1), delta
    want = amd.Fosphor.soft_host(*none)[0]
    assert rec[:3 * W].tobytes() == want.tobytes() and np.all(out == SENTINEL) and list(want["status"]) == [sm.SHORT, sm.OK, sm.OK]
    assert not want["n_steps"].any() and not want["abs_sum"].any()


def test_a_job_alone_among_others_and_shuffled(box):
    """a record and a job's bytes depend on their job alone: bit-identical alone, among the other jobs of the call, and with the
    table in another order (the outputs keep their places, the work-groups and the partials change theirs)"""
    iq, jobs = CASES["seams"]
    among_rec, among = box.run((iq, jobs), tag="among")
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = box.run((iq, jobs[order]), tag="shuffled")
    assert shuffled.tobytes() == among.tobytes() and shuffled_rec.tobytes() == among_rec[order].tobytes()
    for i in (0, 7, 20, len(jobs) - 1):
        alone_rec, alone = box.run((iq, jobs[i:i + 1]), tag="alone %d" % i)
        assert alone_rec[0].tobytes() == among_rec[i].tobytes(), i
        assert bytes_of(alone, jobs[i]).tobytes() == bytes_of(among, jobs[i]).tobytes(), i


def test_python_front_end(amd, box):
    import torch
    iq, jobs = CASES["nan"]
    want_rec, want = amd.Fosphor.soft_host(iq, jobs)
    d_iq = torch.from_numpy(np.ascontiguousarray(iq)).cuda()
    for records, views in (box.f.soft(d_iq, jobs), box.f.soft(d_iq.data_ptr(), jobs, n_samples=len(iq)),
                           box.f.soft(torch.view_as_complex(d_iq), jobs)):
        assert records.dtype == sm.RECORD_DTYPE and records.tobytes() == want_rec.tobytes()
        assert len(views) == len(jobs)
        for v, w, r in zip(views, want, records):
            assert v.dtype == torch.uint8 and len(v) == (r["n_bits"] + 7) // 8 and v.cpu().numpy().tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        box.f.soft(d_iq.data_ptr(), jobs)
    with pytest.raises(ValueError):
        box.f.soft(d_iq.to(torch.float64), jobs)


def test_refusals_launch_and_count_nothing(box):
    """what the host refuses (tests/test_soft_cpu.py has the whole table) leaves every byte and record at the sentinel, launches
    nothing and counts nothing on the device entry point; the nearest calls are accepted"""
    from test_soft_cpu import CAP, N_IQ, changed, good_jobs
    iq = np.random.default_rng(91).standard_normal((N_IQ, 2)).astype(np.float32)
    good = good_jobs()
    box.run((iq, good), tag="good", cap=CAP)

    def refused(jobs, **kw):
        kw.setdefault("cap", CAP)
        rv, rec, out, delta = box.call((iq, jobs), **kw)
        assert rv == EINVAL, (jobs, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "iq", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_samples=2999); refused(good, cap=CAP - 8)
    for row in (dict(rot=4), dict(rot=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=np.inf), dict(scale=np.nan), dict(flags=4), dict(order=3),
                dict(offset=2489), dict(out_offset=4), dict(steps=513), dict(k=8)):
        refused(changed(good[:1], **row))
    for name, by in (("records", 4), ("out", 4), ("iq", 4)):
        refused(good, skew=(name, by))
    nearest = (iq, changed(good[:1], rot=3, scale=1e-45, flags=3))
    got_rec, got = box.run(nearest, tag="nearest", cap=CAP)
    want_rec, views = type(box.f).soft_host(*nearest)
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical to fosphor_amd_soft_host"
    want = np.full(CAP + sm.GUARD, SENTINEL, np.uint8)
    want[:sm.job_owned(nearest[1][0])] = 0
    want[:len(views[0])] = views[0]
    assert got.tobytes() == want.tobytes(), "bytes bit-identical to fosphor_amd_soft_host, every other byte at the sentinel"


def test_call_limit(amd):
    """a call of exactly MAX_CALL_STEPS (sm.call_limit_case(): 64 jobs of MAX_STEPS, 32 MiB of survivor decisions, 16 MiB of soft
    words, 16384 partials, step0 up to 2^22 - 2^16) on a fresh instance, between two small calls: the scratch grows behind a small
    call and is reused by one.  All three are bit-identical to fosphor_amd_soft_host, the whole output and records buffers
    compared, with one launch a kernel; the job with the largest step0 gives the same record and bytes alone; one step more is
    refused, writes nothing, launches nothing and counts nothing"""
    import torch
    free, total = torch.cuda.mem_get_info()
    if free < 2 ** 30:
        pytest.skip("the call wants 1 GiB of device memory free: %d of %d bytes are" % (free, total))
    small, limit = CASES["nan"], sm.call_limit_case()
    jobs = limit[1]
    assert sum(sm.shape(j)[0] for j in jobs) == sm.MAX_CALL_STEPS and len(jobs) == 64
    b = Box(amd)
    try:
        for tag, case, key in (("small", small, "nan"), ("limit", limit, "call_limit"), ("small again", small, "nan")):
            want_rec, want = host_image(amd, case, key=key)
            got_rec, got = b.run(case, tag=tag)
            explain(got_rec, want_rec, got, want, case[1])
            assert got_rec.tobytes() == want_rec.tobytes(), tag + ": records bit-identical to fosphor_amd_soft_host"
            assert got.tobytes() == want.tobytes(), tag + ": bytes bit-identical to fosphor_amd_soft_host, every other byte at the sentinel"
            if tag == "limit":
                limit_rec, limit_out = got_rec, got
        last = len(jobs) - 1							# the table's last job: step0 = 63 MAX_STEPS
        alone_rec, alone = b.run((limit[0], jobs[last:]), tag="alone")
        assert alone_rec[0].tobytes() == limit_rec[last].tobytes()
        assert bytes_of(alone, jobs[last]).tobytes() == bytes_of(limit_out, jobs[last]).tobytes()
        more = sm.one_step_more(limit)
        rv, rec, out, delta = b.call(more)
        assert rv == EINVAL and np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")
    finally:
        b.f.close()


FAR_BYTES = 2 ** 31 + 2 ** 20


def test_far_offset_and_out_offset(amd, box):
    """the buffers of tests/test_gpu_decode.py's far test, 2^31 + 2^20 bytes: the symbols of the "seams" case copied 2^31 + 2^19 + 8
    bytes into one, every job's offset moved by that many samples' worth, and the outputs written 2^31 + 2^19 bytes into another;
    decoy symbols where a byte offset cut to 31 or 32 bits would look.  Records and bits are bit-identical to the near run, the
    input and the decoys are unchanged, and nothing of the output buffer's first bytes is written"""
    import torch
    free, total = torch.cuda.mem_get_info()
    if free < 2 * FAR_BYTES + 2 ** 30:
        pytest.skip("the far buffers take %d bytes and want %d free: %d of %d bytes are" % (2 * FAR_BYTES, 2 * FAR_BYTES + 2 ** 30, free, total))
    iq, jobs = CASES["seams"]
    iq = np.ascontiguousarray(iq, np.float32).reshape(-1, 2)
    near_rec, near = box.run((iq, jobs), tag="near")
    base = 2 ** 31 + 2 ** 19 + 8						# bytes, a multiple of 8
    big = torch.empty(FAR_BYTES, dtype=torch.uint8, device="cuda")
    flat = torch.from_numpy(iq).cuda().view(torch.uint8).reshape(-1)
    decoy = torch.from_numpy(np.ascontiguousarray(-iq[::-1])).cuda().view(torch.uint8).reshape(-1)
    aliases = sorted({base % 2 ** 31, base % 2 ** 32, base - 2 ** 31} - {base})
    for a in aliases:
        big[a:a + len(decoy)].copy_(decoy)
    big[base:base + len(flat)].copy_(flat)
    far_jobs = jobs.copy()
    far_jobs["offset"] += base // 8
    out_base = 2 ** 31 + 2 ** 19
    far_jobs["out_offset"] += out_base
    assert (far_jobs["offset"] * 8).min() > 2 ** 31 and far_jobs["out_offset"].min() > 2 ** 31
    big_out = torch.empty(FAR_BYTES, dtype=torch.uint8, device="cuda")
    size = sm.capacity(jobs)
    big_out[:4096].fill_(SENTINEL)
    big_out[out_base:out_base + size + 64].fill_(SENTINEL)
    out_aliases = sorted({out_base % 2 ** 31, out_base % 2 ** 32, out_base - 2 ** 31} - {out_base})
    for a in out_aliases:
        big_out[a:a + size].fill_(SENTINEL)
    rv, rec, _, delta = box.call((iq, far_jobs), iq_at=(big.data_ptr(), FAR_BYTES // 8), out_at=(big_out, FAR_BYTES))
    assert rv == 0 and delta == sm.expected_stats(jobs)
    far_rec = rec[:W * len(jobs)].view(sm.RECORD_DTYPE)
    far = big_out[out_base:out_base + size].cpu().numpy()
    assert far_rec.tobytes() == near_rec.tobytes() and far.tobytes() == near.tobytes(), "the far run differs from the near one"
    assert bool((big_out[out_base + size:out_base + size + 64] == SENTINEL).all()) and bool((big_out[:4096] == SENTINEL).all())
    for a in out_aliases:
        assert bool((big_out[a:a + size] == SENTINEL).all()), "an output offset was cut"
    assert big[base:base + len(flat)].cpu().numpy().tobytes() == iq.tobytes(), "the input was written"
    for a in aliases:
        assert torch.equal(big[a:a + len(decoy)], decoy), "a decoy was written"
    del big, big_out
    torch.cuda.empty_cache()


def test_chain_carrier_decide_soft(amd, box):
    """the synthetic QPSK burst of tests/test_soft_cpu.py: carrier and decide on the device, soft over carrier's device buffer by
    the jobs that soft_jobs() makes from decide's record; records and bits are the host chain's, and the planted bits come out"""
    import torch
    import decode_model as dm
    F = amd.Fosphor
    iq, word, info, payload = chain_burst()
    cjobs, dflags = chain_jobs(len(iq))
    crec, cviews = box.f.carrier(torch.from_numpy(iq).cuda(), cjobs)
    djobs = F.decide_jobs(cjobs, crec, dflags, 0, CHAIN_UW, 0, 0, 4)
    d_c = cviews[0]
    base = d_c.data_ptr() - 8 * int(cjobs["out_offset"][0])
    drec, dviews = box.f.decide(base, djobs, word, n_samples=int(cjobs["out_offset"][0]) + len(d_c))
    jobs = F.soft_jobs(djobs, drec, CHAIN_UW, **CHAIN_CODE)
    before = box.f.soft_stats()
    rec, views = box.f.soft(base, jobs, n_samples=int(cjobs["out_offset"][0]) + len(d_c))
    after = box.f.soft_stats()
    assert {k: after[k] - before[k] for k in after} == sm.expected_stats(jobs)
    hcrec, hcviews = F.carrier_host(iq, cjobs)
    assert crec.tobytes() == hcrec.tobytes()
    c = hcviews[0].view(np.float32).reshape(-1, 2)
    hdrec, _ = F.decide_host(c, djobs, word)
    assert drec.tobytes() == hdrec.tobytes() and drec["uw_rot"][0] != 0
    hjobs = F.soft_jobs(djobs, hdrec, CHAIN_UW, **CHAIN_CODE)
    assert hjobs.tobytes() == jobs.tobytes()
    want_rec, want = F.soft_host(c, hjobs)
    assert rec.tobytes() == want_rec.tobytes() and views[0].cpu().numpy().tobytes() == want[0].tobytes()
    assert (rec["status"][0], rec["n_bits"][0], rec["crc_calc"][0]) == (sm.OK, 416, dm.crc_bits(info, dm.CRC16))
    assert list(dm.unpack(views[0].cpu().numpy(), CHAIN_INFO)) == list(info), "the decoded bits are the planted ones"
