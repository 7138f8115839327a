"""PSK decisions, unique word and EVM sums on the device (include/fosphor_amd_decide.h) against the numpy statement
(tests/decide_model.py) and against fosphor_amd_decide_host: records and bytes bit for bit, tobytes().

The bytes go into a sentinel-filled buffer in which GUARD bytes before, behind and between the jobs' owned ranges belong to no job,
and the records into a sentinel-filled buffer with one record more than there are jobs; both are compared whole with the model's
image, so a byte or a record written outside a job's range fails like a wrong one.  Every run ends by checking that the input
buffer is bit-identical, that the instance's ring position, waterfall and spectrum are untouched (the method of
tests/test_gpu_carrier.py) and that the stats delta names the kernels that ran, at most four launches per call.

Seams of the kernels (the input sets are dm.cases()):
  tiles, stores n = 0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097 and 2 * 4096 + 5 at M = 2, 4 and 8: the
                four-symbol store with each remainder, both tile seams, DIFF across a tile seam (k_dec_out reads the word before).
  the offsets   input offsets 0 .. 3; a job that ends on the buffer's last sample.
  the windows   a window that starts at 0, and at 1 under DIFF; one that ends on the last position that fits; words across the
                256-position seam of k_dec_uw and across the tile seam of the decisions; uw_len 1, 63 and 64; uw_count 0; windows
                without a candidate (NO_UW); uw_max_errors exceeded.
  the numbers   all-zero symbols; NaN symbols (erasures); inf; subnormals; 3e38.
  the prefixes  MAX_JOBS jobs in shuffled order with everything mixed and n <= 130, every 11th with n = 0.
The refusal "more than 2^31 - 1 work-groups" needs owned bytes beyond any buffer and has no case."""
import errno
import os

import numpy as np
import pytest

import decide_model as dm

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a
SENTINEL32 = 0x5a5a5a5a
CASES = dm.cases()
W = dm.RECORD_WORDS
KERNELS = ("k_hard", "k_uw", "k_job", "k_out")


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
    """an instance, torch views of its waterfall ring and spectrum, and the decide call through the C ABI"""

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

    def call(self, case, n_samples=None, n_jobs=None, n_uw=None, cap=None, null=(), skew=None):
        """-> (return value, the records buffer as uint32 [(n_jobs + 1) * 24], the whole output buffer as uint8 [size], delta of
        the stats).  cap: out_capacity, GUARD bytes of the buffer lie behind it; skew: (pointer name, bytes)"""
        import torch
        self.save()
        iq = dm.buffer(case)
        jobs = np.ascontiguousarray(case[1], dm.JOB_DTYPE)
        uw = np.concatenate([dm.table(case), np.zeros(1, np.uint8)])		# something to point at when the table is empty
        size = dm.capacity(jobs) if cap is None else max(cap, 0) + dm.GUARD
        d_iq = torch.from_numpy(iq).cuda() if len(iq) else torch.zeros((1, 2), dtype=torch.float32, device="cuda")
        d_out = torch.full((size + 4,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_rec = torch.full(((len(jobs) + 1) * W,), SENTINEL32, dtype=torch.int32, device="cuda")
        ptr = {"self": self.f.h, "iq": d_iq.data_ptr(), "jobs": jobs.ctypes.data, "uw": uw.ctypes.data, "records": d_rec.data_ptr(),
               "out": d_out.data_ptr()}
        for k in null:
            ptr[k] = None
        if skew:
            ptr[skew[0]] += skew[1]
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.decide_stats()
        rv = self.f.L.fosphor_amd_decide(ptr["self"], ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["jobs"],
                                         len(jobs) if n_jobs is None else n_jobs, ptr["uw"], len(uw) - 1 if n_uw is None else n_uw,
                                         ptr["records"], ptr["out"], size if cap is None else cap)
        after = self.f.decide_stats()
        out = d_out.cpu().numpy()
        rec = d_rec.cpu().numpy().view(np.uint32)
        assert np.all(out[size:] == SENTINEL)
        if len(iq):
            assert d_iq.cpu().numpy().tobytes() == iq.tobytes(), "the input buffer was written"
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
    return buf[at:at + dm.owned(job["n"])]


def explain(got_rec, want_rec, got, want, jobs):
    """print the first records and bytes that differ, with the job that owns them"""
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    for i in np.flatnonzero(got != want)[:8]:
        own = [k for k, j in enumerate(jobs) if int(j["out_offset"]) <= i < int(j["out_offset"]) + dm.owned(j["n"])]
        print("byte %d got %s want %s job %s" % (i, got[i], want[i], [(k, jobs[k]) for k in own[:2]]))


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
    host_rec, host_views = amd.Fosphor.decide_host(dm.buffer(case), jobs, case[2])
    assert got_rec.tobytes() == host_rec.tobytes(), "records bit-identical to fosphor_amd_decide_host"
    for v, j in zip(host_views, jobs):
        assert bytes_of(got, j)[:len(v)].tobytes() == v.tobytes(), "bit-identical to fosphor_amd_decide_host"
    again_rec, again = box.run(case, tag=name + " again")
    assert again.tobytes() == got.tobytes() and again_rec.tobytes() == got_rec.tobytes(), "the same call twice is bit-identical"
    if name == "numbers":
        assert got_rec["erasures"].sum() >= 8 and (got_rec["status"] == dm.NO_UW).any()
    if name == "windows":
        assert (got_rec["status"] == dm.NO_UW).sum() >= 12 and (got_rec["uw_pos"] == -1).sum() >= 8
        assert {0, 1, 250, 255, 256, 4080, 4095, 4096, 668} <= set(got_rec["uw_pos"])


def test_which_kernels_ran(box):
    """jobs with and without a word: all four; only without: no k_dec_uw; words without a candidate: no k_dec_uw; jobs without a
    symbol: k_dec_job alone"""
    ran = lambda delta: tuple(delta[k] for k in KERNELS)
    rv, rec, out, delta = box.call(CASES["mixed"])
    assert rv == 0 and ran(delta) == (1, 1, 1, 1), delta
    rv, rec, out, delta = box.call(CASES["without_word"])
    assert rv == 0 and ran(delta) == (1, 0, 1, 1), delta
    iq = dm.psk(64, 4, 0.0, 0.26, 5)
    word = np.arange(20, dtype=np.uint8) % 4
    short = (iq, dm.make_jobs([(3, 4, 19, 4, dm.UW, 0, 20, 0, 0, 0), (1, 28, 40, 4, dm.UW | dm.DIFF, 0, 20, 21, 5, 0)]), word)
    rv, rec, out, delta = box.call(short)
    assert rv == 0 and ran(delta) == (1, 0, 1, 1), delta
    want_rec, want = dm.image(short, SENTINEL)
    assert rec[:2 * W].tobytes() == want_rec.tobytes() and out.tobytes() == want.tobytes()
    assert list(want_rec["status"]) == [dm.NO_UW, dm.NO_UW] and list(want_rec["uw_errors"]) == [20, 20]
    none = (iq, dm.make_jobs([(3, 4, 0, 4, 0), (64, 4, 0, 8, dm.UW | dm.GRAY, 0, 1, 0, 0, 0)]), word)
    rv, rec, out, delta = box.call(none)
    assert rv == 0 and ran(delta) == (0, 0, 1, 0), delta
    assert rec[:2 * W].tobytes() == dm.decide(none)[0].tobytes() and np.all(out == SENTINEL)


def test_a_job_alone_among_others_and_shuffled(box):
    """a record and a job's bytes depend on their job alone: bit-identical alone, among the other jobs of the call, and with the
    table in another order (the outputs keep their places, the work-groups change theirs)"""
    iq, jobs, uw = CASES["mixed"]
    among_rec, among = box.run((iq, jobs, uw), tag="among")
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = box.run((iq, jobs[order], uw), tag="shuffled")
    assert shuffled.tobytes() == among.tobytes() and shuffled_rec.tobytes() == among_rec[order].tobytes()
    for flags in (0, dm.DIFF | dm.UW, dm.GRAY | dm.UW, dm.DIFF | dm.GRAY):
        i = int(np.flatnonzero((jobs["flags"] == flags) & (jobs["n"] > 64))[0])
        alone_rec, alone = box.run((iq, jobs[i:i + 1], uw), tag="alone %d" % i)
        assert alone_rec[0].tobytes() == among_rec[i].tobytes(), i
        assert bytes_of(alone, jobs[i]).tobytes() == bytes_of(among, jobs[i]).tobytes(), i


def test_python_front_end(box):
    import torch
    iq, jobs, uw = CASES["mixed"]
    want_rec, want = dm.decide((iq, jobs, uw))
    d_iq = torch.from_numpy(iq).cuda()
    for records, views in (box.f.decide(d_iq, jobs, uw), box.f.decide(d_iq.view(torch.complex64).reshape(-1), jobs, uw),
                           box.f.decide(d_iq.data_ptr(), jobs, uw, n_samples=len(iq))):
        assert records.dtype == dm.RECORD_DTYPE and records.tobytes() == want_rec.tobytes()
        assert len(views) == len(jobs)
        for v, w, j in zip(views, want, jobs):
            assert v.dtype == torch.uint8 and len(v) == j["n"] and v.cpu().numpy().tobytes() == w[:int(j["n"])].tobytes()
    iq, jobs, uw = CASES["without_word"]
    records, views = box.f.decide(torch.from_numpy(iq).cuda(), jobs)
    assert records.tobytes() == dm.decide((iq, jobs, uw))[0].tobytes()
    with pytest.raises(ValueError):
        box.f.decide(d_iq.data_ptr(), jobs)


EINVAL_OK = (0, 0, 100, 4, dm.UW, 0, 32, 0, 0, 0)


def EINVAL_ROWS(cap):
    """one job each that rule 7 refuses, over 3000 samples and a table of 40 symbols below 4 (the rows of
    tests/test_decide_cpu.py)"""
    def one(**kw):
        row = dict(zip(dm.FIELDS, EINVAL_OK))
        row.update(kw)
        return tuple(row.values())

    plain = dict(flags=0, uw_len=0)
    return [one(offset=-1), one(out_offset=-4), one(n=-1), one(offset=2901), one(offset=3001, n=0), one(offset=2 ** 62, n=2 ** 31 - 1),
            one(offset=2 ** 62), one(out_offset=cap + 4, n=0), one(out_offset=2 ** 62), one(out_offset=cap - 96),
            one(out_offset=cap - 100, n=101), one(out_offset=1), one(out_offset=2), one(out_offset=3), one(out_offset=6, n=0),
            one(order=0), one(order=1), one(order=3), one(order=6), one(order=16), one(order=-4),
            one(flags=8 | dm.UW), one(flags=16), one(flags=-1),
            one(uw_len=0), one(uw_len=65), one(uw_len=-1), one(uw_offset=-1), one(uw_offset=9), one(uw_offset=40, uw_len=1),
            one(uw_offset=2 ** 31 - 1), one(order=2), one(uw_first=-1), one(uw_count=-1), one(uw_max_errors=-1),
            one(uw_offset=1, **plain), one(uw_len=1, flags=0), one(uw_first=1, **plain), one(uw_count=1, **plain),
            one(uw_max_errors=1, **plain), one(flags=dm.DIFF | dm.GRAY, uw_len=32)]


def test_einval_table(box):
    """each refused call leaves every byte and record at the sentinel, launches nothing and counts nothing"""
    iq = dm.psk(3000, 4, 0.0, 0.26, 91, 30.0)
    uw = np.concatenate([dm.planted(3000, 4, 91)[100:139], [2]]).astype(np.uint8)		# 40 symbols, the last one a 2
    #        offset out n order flags uw_offset uw_len uw_first uw_count uw_max_errors
    good = [(0, 8, 500, 4, dm.UW, 0, 39, 0, 0, 0), (2990, 0, 5, 2, dm.DIFF), (3000, 508, 0, 8, dm.GRAY), (1, 512, 2999, 8, dm.UW, 1, 39, 5, 0, 39)]
    cap = 512 + 3000
    rec, out = box.run((iq, dm.make_jobs(good), uw), tag="good", cap=cap)
    assert np.all(out[cap:] == SENTINEL) and np.all(out[508:512] == SENTINEL) and np.all(out[0:8] != SENTINEL)
    assert rec["uw_pos"][0] == 100 and rec["uw_rot"][0] == 1 and rec["uw_errors"][0] == 0

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        rv, rec, out, delta = box.call((iq, dm.make_jobs(rows), uw), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "iq", "jobs", "uw", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[1]] * (dm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=2999); refused(good, cap=-1); refused(good, cap=cap - 1)
    refused(good, n_uw=-1); refused(good, n_uw=39); refused(good, n_uw=dm.MAX_UW_TABLE + 1)
    for row in EINVAL_ROWS(cap):
        refused([row])
    reserved = dm.make_jobs([EINVAL_OK] * 4)
    for i in range(4):
        reserved["reserved"][i, i] = 1
        rv, rec, out, delta = box.call((iq, reserved[i:i + 1], uw), cap=cap)
        assert rv == EINVAL and np.all(out == SENTINEL) and np.all(rec == SENTINEL32) and not any(delta.values())
    refused([EINVAL_OK, EINVAL_OK[:1] + (96,) + EINVAL_OK[2:]])				# [0, 100) and [96, 196): a word shared
    refused([EINVAL_OK[:2] + (97,) + EINVAL_OK[3:], EINVAL_OK[:1] + (96,) + EINVAL_OK[2:]])	# the padding of [0, 97) is owned
    refused([EINVAL_OK[:1] + (200,) + EINVAL_OK[2:], (0, 8, 800, 4, 0)])			# [200, 300) and [8, 808), in descending order
    for name, by in (("iq", 4), ("records", 4), ("out", 1), ("out", 2)):
        refused(good, skew=(name, by))
    # the last jobs that still fit, in the input and in the output; outputs that touch; jobs without a symbol anywhere inside; no table
    last = dm.make_jobs([(0, 0, 97, 4, 0), (0, 100, 100, 2, dm.DIFF), (2900, cap - 100, 100, 4, dm.UW, 39, 1, 99, 0, 1),
                         (3000, cap, 0, 8, 0), (5, 52, 0, 8, 0)])
    rec, out = box.run((iq, last, uw), tag="the last jobs that fit", cap=cap)
    want_rec, want = dm.image((iq, last, uw), SENTINEL)
    assert rec.tobytes() == want_rec.tobytes()
    assert out[:cap].tobytes() == want[:cap].tobytes() and np.all(out[cap:] == SENTINEL)
    rv, rec, out, delta = box.call((iq, last[:2], uw), cap=cap, null=("uw",), n_uw=0)
    assert rv == 0 and rec[:2 * W].tobytes() == want_rec[:2].tobytes()


def test_chain_carrier_decide(amd, box):
    """the QPSK preamble of resample_model's small sc16 stream: extract -> resample -> symbols -> carrier -> decide, each pass over
    the device buffer of the one before, at order 4 with DIFF and UW; the word is the 32 planted differential symbols 16 .. 47 of
    the preamble, whose indices chain_case() draws from its rng behind the two noise arrays.  From the buffer that extract wrote on,
    the chain is bit for bit the host statements' chained.  The host chain on the CPU finds the word without an error, at
    uw_pos 16 over the preamble alone and at uw_pos 191 over the whole burst (uw_errors 0 and 0): the device is bit-identical to
    it, so these are asserted as they are."""
    import torch
    import resample_model as rm
    import symbols_model as sm
    F = amd.Fosphor
    rng = np.random.default_rng(4321)
    rng.standard_normal(32000), rng.standard_normal(32000)
    idx = rng.integers(0, 4, rm.CHAIN_SYMBOLS)
    word = ((idx[1:] - idx[:-1]) & 3)[15:47].astype(np.uint8)		# the differences d[16] .. d[47]
    raw, ejobs, _, lag = rm.chain_case()
    assert len(raw) == 32000
    taps = F.extract_design(rm.CHAIN_DECIM, rm.CHAIN_TAPS, 0.8)
    rtaps = F.resample_design(rm.CHAIN_UP, rm.CHAIN_DOWN, rm.CHAIN_BRANCH)
    rjobs = F.resample_jobs(ejobs, rm.CHAIN_UP, rm.CHAIN_DOWN, len(rtaps))
    rjobs["out_offset"] = 5
    sjobs = np.concatenate([F.symbols_jobs(rjobs, rm.CHAIN_HOLD), F.symbols_jobs(rjobs, rm.CHAIN_HOLD)])
    sjobs["offset"][1] += lag						# the preamble alone
    sjobs["n"][1] = rm.CHAIN_T
    sjobs["out_offset"][1] = sm.job_max_out(sjobs[0]) + sm.GUARD
    # the device
    e_views = box.f.extract(torch.from_numpy(raw).cuda(), ejobs, taps, iq_format="sc16")
    e_base = e_views[0].data_ptr() - 8 * int(ejobs["out_offset"][0])
    e_cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    r_views = box.f.resample(e_base, rjobs, rtaps, n_samples=e_cap)
    r_base = r_views[0].data_ptr() - 8 * int(rjobs["out_offset"][0])
    r_cap = int((rjobs["out_offset"] + rjobs["n_out"]).max())
    srec, s_views = box.f.symbols(r_base, sjobs, n_samples=r_cap)
    s_base = s_views[0].data_ptr() - 8 * int(sjobs["out_offset"][0])
    s_cap = int(max(int(j["out_offset"]) + int(r["n_sym"]) for j, r in zip(sjobs, srec)))
    cjobs = F.carrier_jobs(sjobs, srec, 4, lag=8)
    crec, c_views = box.f.carrier(s_base, cjobs, n_samples=s_cap)
    assert list(crec["status"]) == [0, 0]
    c_base = c_views[0].data_ptr() - 8 * int(cjobs["out_offset"][0])
    c_cap = int((cjobs["out_offset"] + cjobs["n"]).max())
    djobs = F.decide_jobs(cjobs, crec, ("diff", "uw"), uw_offset=0, uw_len=32, uw_max_errors=4)
    assert list(djobs["offset"]) == list(cjobs["out_offset"]) and list(djobs["n"]) == list(crec["n"]) and set(djobs["order"]) == {4}
    assert not (djobs["out_offset"] & 3).any() and djobs["out_offset"][1] >= djobs["out_offset"][0] + dm.owned(djobs["n"][0]) + 4
    before = box.f.decide_stats()
    records, views = box.f.decide(c_base, djobs, word, n_samples=c_cap)
    after = box.f.decide_stats()
    assert {k: after[k] - before[k] for k in after} == dm.expected_stats(djobs)
    # the host statements over what extract wrote on the device
    x = np.zeros((e_cap, 2), np.float32)
    for j, v in zip(ejobs, e_views):
        x[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] = v.cpu().numpy().view(np.float32).reshape(-1, 2)
    y = np.zeros((r_cap, 2), np.float32)
    y[5:] = F.resample_host(x, rjobs, rtaps)[0].view(np.float32).reshape(-1, 2)
    hrec, hsyms = F.symbols_host(y, sjobs)
    assert srec.tobytes() == hrec.tobytes()
    s = np.zeros((s_cap, 2), np.float32)
    for j, v in zip(sjobs, hsyms):
        s[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v.view(np.float32).reshape(-1, 2)
    hcrec, hc = F.carrier_host(s, cjobs)
    assert crec.tobytes() == hcrec.tobytes()
    c = np.zeros((c_cap, 2), np.float32)
    for j, v in zip(cjobs, hc):
        c[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v.view(np.float32).reshape(-1, 2)
    want_rec, want = F.decide_host(c, djobs, word)
    assert records.tobytes() == want_rec.tobytes()
    for v, w in zip(views, want):
        assert v.cpu().numpy().tobytes() == w.tobytes()
    model_rec, _ = dm.decide((c, djobs, word))
    assert records.tobytes() == model_rec.tobytes()
    v = F.decide_derive(records, 32)
    print("chain: n %s uw_pos %s uw_errors %s evm %.4f mer %.1f dB" % (records["n"], records["uw_pos"], records["uw_errors"],
                                                                       v[1]["evm_rms"], v[1]["mer_db"]))
    assert list(records["status"]) == [dm.OK, dm.OK] and list(records["uw_errors"]) == [0, 0] and list(records["uw_pos"]) == [191, 16]
    got = views[1].cpu().numpy()[16:48]
    assert got.tobytes() == word.tobytes(), "the decoded differences are the planted ones"
