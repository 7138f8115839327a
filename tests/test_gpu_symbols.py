"""Symbol timing and symbol-rate samples of burst IQ on the device (include/fosphor_amd_symbols.h) against the numpy statement
(tests/symbols_model.py) and against fosphor_amd_symbols_host: records and symbols bit for bit, tobytes().

The symbols go into a sentinel-filled buffer in which GUARD samples before, behind and between the jobs' reserved ranges belong to
no job -- and neither do the reserved samples behind a job's n_sym -- and the records into a sentinel-filled buffer with one record
more than there are jobs; both are compared whole with the model's image, so a sample or a record written outside a job's range
fails like a wrong one.  Every run ends by checking that the input buffer is bit-identical, that the instance's ring position,
waterfall and spectrum are untouched (the method of tests/test_gpu_psd.py) and that the stats delta names the kernels that ran, at
most four launches per call.

Seams of the kernels (the input sets are sm.cases()):
  the loads     16-byte pairs from the first 16-byte boundary: offset 0 .. 3 against odd and even out_offsets, a job that ends on
                the buffer's last sample; sps 2 (FIXED), 3, 4, 5, 8, 16, 63 and 64, staged (<= 8) and direct.
  k_sym_fold    n / sps = 0, 1, 63, 64, 65, 4095, 4096, 4097 and 2 * 4096 + 5 at sps 3, n no multiple of sps; 65 at sps 64; pieces of
                21, 12, 4 and 1 blocks.
  k_sym_pick    n_sym = 0, 1, 63, 64, 65, 4096 and 4097 under FIXED; n = 3, 4 and sps + 3; g + 2 == n - 1 holds and just fails; a
                reserved tile without a symbol.
  k_sym_time    FIXED: tau = 0 (symbol 0 is dropped), a whole base (mu = 0), 0.99999994.  ESTIMATE: X = 0; a = -0, -0.5, a rounded
                +0.5 and a tiny negative whose e + 1.0 is 1.0; a NaN sample (NO_TIMING, nothing written) and an inf sample.
  the numbers   subnormal samples, 1e30, and 3e38 whose interpolated float overflows.
  the prefixes  MAX_JOBS jobs in shuffled order with modes and sps mixed, every 11th with n = 0; only FIXED jobs (no k_sym_fold);
                only ESTIMATE jobs.
The refusal "more than 2^31 - 1 work-groups" cannot arise at this pass's limits (the header says why) and has no case."""
import errno
import os

import numpy as np
import pytest

import symbols_model as sm

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a5a5a5a
CASES = sm.cases()
W = sm.RECORD_WORDS


def model(name):
    """the model's records and its image of a case's output buffer, computed once a session"""
    return sm.image(CASES[name], SENTINEL, key=name)


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the symbols call through the C ABI"""

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

    def call(self, case, n_samples=None, n_jobs=None, cap=None, null=(), skew=None):
        """-> (return value, the records buffer as uint32 [(n_jobs + 1) * 24], the whole output buffer as uint32 [size][2], delta
        of the stats).  cap: out_capacity, GUARD samples of the buffer lie behind it; skew: (pointer name, bytes)"""
        import torch
        self.save()
        iq = sm.buffer(case)
        jobs = np.ascontiguousarray(case[1], sm.JOB_DTYPE)
        d_iq = torch.from_numpy(iq).cuda()
        size = sm.capacity(jobs) if cap is None else max(cap, 0) + sm.GUARD
        d_out = torch.full((size + 1, 2), SENTINEL, dtype=torch.int32, device="cuda")
        d_rec = torch.full(((len(jobs) + 1) * W,), SENTINEL, dtype=torch.int32, device="cuda")
        ptr = {"self": self.f.h, "iq": d_iq.data_ptr(), "jobs": jobs.ctypes.data, "records": d_rec.data_ptr(), "out": d_out.data_ptr()}
        for k in null:
            ptr[k] = None
        if skew:
            ptr[skew[0]] += skew[1]
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.symbols_stats()
        rv = self.f.L.fosphor_amd_symbols(ptr["self"], ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["jobs"],
                                          len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"], size if cap is None else cap)
        after = self.f.symbols_stats()
        out = d_out.cpu().numpy().view(np.uint32)
        rec = d_rec.cpu().numpy().view(np.uint32)
        assert np.all(out[size] == SENTINEL)
        assert d_iq.cpu().numpy().tobytes() == iq.tobytes(), "the input buffer was written"
        self.assert_untouched()
        return rv, rec, out[:size], {k: after[k] - before[k] for k in after}

    def run(self, case, tag="", **kw):
        """a call that must succeed: the stats -> (records, the whole output buffer)"""
        rv, rec, out, delta = self.call(case, **kw)
        assert rv == 0, tag
        jobs = case[1]
        assert np.all(rec[W * len(jobs):] == SENTINEL), "a record beyond the jobs' was written"
        records = rec[:W * len(jobs)].view(sm.RECORD_DTYPE)
        assert delta == sm.expected_stats(jobs, records), (tag, delta)
        assert delta["k_fold"] + delta["k_time"] + delta["k_pick"] + delta["k_record"] <= 4
        return records, out


def symbols_of(buf, job, record):
    at = int(job["out_offset"])
    return buf[at:at + int(record["n_sym"])]


def explain(got_rec, want_rec, got, want, jobs):
    """print the first records and samples that differ, with the job that owns them"""
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    for i in np.flatnonzero((got != want).any(1))[:8]:
        own = [k for k, j in enumerate(jobs) if int(j["out_offset"]) <= i < int(j["out_offset"]) + sm.job_max_out(j)]
        print("sample %d got %s want %s job %s" % (i, got[i], want[i], [(k, jobs[k]) for k in own[:2]]))


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
    assert got.tobytes() == want.tobytes(), "symbols bit-identical to the model, every other sample at the sentinel"
    host_rec, host_views = amd.Fosphor.symbols_host(sm.buffer(case), jobs)
    assert got_rec.tobytes() == host_rec.tobytes(), "records bit-identical to fosphor_amd_symbols_host"
    for v, j, r in zip(host_views, jobs, got_rec):
        assert symbols_of(got, j, r).tobytes() == v.tobytes(), "bit-identical to fosphor_amd_symbols_host"
    again_rec, again = box.run(case, tag=name + " again")
    assert again.tobytes() == got.tobytes() and again_rec.tobytes() == got_rec.tobytes(), "the same call twice is bit-identical"
    if name == "phase_estimate":
        assert got_rec["status"][12] == sm.NO_TIMING and got_rec["tau"][12:13].view(np.uint32)[0] == 0x7fc00000
        assert list(got_rec["tau"][:5]) == [0.0, 0.0, 0.5, 0.5, 0.0]


def test_which_kernels_ran(box):
    """only FIXED jobs: no k_sym_fold; only ESTIMATE jobs: all four; jobs too short for a symbol: k_sym_time and k_sym_record alone"""
    for name, fold in (("only_fixed", 0), ("only_estimate", 1)):
        rv, rec, out, delta = box.call(CASES[name])
        assert rv == 0 and (delta["k_fold"], delta["k_time"], delta["k_pick"], delta["k_record"]) == (fold, 1, 1, 1), delta
    short = (sm.noise(16, 5), sm.make_jobs([(0, 3, 3, 4, sm.ESTIMATE, 0.0), (1, 3, 2, 2, sm.FIXED, 0.5), (16, 3, 0, 64, sm.FIXED, 0.0)]))
    rv, rec, out, delta = box.call(short)
    assert rv == 0 and (delta["k_fold"], delta["k_time"], delta["k_pick"], delta["k_record"]) == (0, 1, 0, 1), delta
    assert rec[:3 * W].tobytes() == sm.symbols(short)[0].tobytes() and np.all(out == SENTINEL)


def test_a_job_alone_among_others_and_shuffled(box):
    """a record and a job's symbols depend on their job alone: bit-identical alone, among the other jobs of the call, and with the
    table in another order (the outputs keep their places, the work-groups change theirs)"""
    iq, jobs = CASES["mixed"]
    among_rec, among = box.run((iq, jobs), tag="among")
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = box.run((iq, jobs[order]), tag="shuffled")
    assert shuffled.tobytes() == among.tobytes() and shuffled_rec.tobytes() == among_rec[order].tobytes()
    est = np.flatnonzero((jobs["mode"] == sm.ESTIMATE) & (among_rec["n_sym"] > 64))
    fix = np.flatnonzero((jobs["mode"] == sm.FIXED) & (among_rec["n_sym"] > 0))
    for i in (int(est[0]), int(est[-1]), int(fix[0]), int(np.flatnonzero(among_rec["n_sym"] == 0)[0])):
        alone_rec, alone = box.run((iq, jobs[i:i + 1]), tag="alone %d" % i)
        assert alone_rec[0].tobytes() == among_rec[i].tobytes(), i
        assert symbols_of(alone, jobs[i], alone_rec[0]).tobytes() == symbols_of(among, jobs[i], among_rec[i]).tobytes(), i


def test_python_front_end(box):
    import torch
    iq, jobs = CASES["loads"]
    want_rec, want = sm.symbols((iq, jobs))
    d_iq = torch.from_numpy(iq).cuda()
    for records, views in (box.f.symbols(d_iq, jobs), box.f.symbols(d_iq.view(torch.complex64).reshape(-1), jobs),
                           box.f.symbols(d_iq.data_ptr(), jobs, n_samples=len(iq))):
        assert records.dtype == sm.RECORD_DTYPE and records.tobytes() == want_rec.tobytes()
        assert len(views) == len(jobs)
        for v, w in zip(views, want):
            assert v.dtype == torch.complex64 and v.cpu().numpy().view(np.float32).tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        box.f.symbols(d_iq.data_ptr(), jobs)


def test_einval_table(box):
    """each refused call leaves every sample and record at the sentinel, launches nothing and counts nothing"""
    iq = sm.noise(3000, 91)
    #        offset out  n   sps mode         tau
    good = [(0, 5, 500, 4, sm.ESTIMATE, 0.0), (2990, 0, 10, 2, sm.FIXED, 0.5), (3000, 130, 0, 3, sm.ESTIMATE, 0.0),
            (1, 140, 2999, 64, sm.FIXED, 0.99)]
    cap = 140 + sm.max_out(2999, 64)
    rec, out = box.run((iq, sm.make_jobs(good)), tag="good", cap=cap)
    assert np.all(out[cap:] == SENTINEL) and np.all(out[130:140] == SENTINEL) and np.all(out[0:4] != SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        jobs = sm.make_jobs(rows)
        for i, res in kw.pop("reserved", []):
            jobs["reserved"][0][i] = res
        rv, rec, out, delta = box.call((iq, jobs), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "iq", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (sm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=2999); refused(good, cap=-1); refused(good, cap=cap - 1)
    ok = (0, 0, 100, 4, sm.FIXED, 0.25)

    def one(**kw):
        row = dict(zip(("offset", "out_offset", "n", "sps", "mode", "tau"), ok))
        row.update(kw)
        refused([tuple(row.values())])

    one(offset=-1); one(out_offset=-1); one(n=-1); one(offset=2901); one(offset=3001, n=0); one(offset=2 ** 62, n=2 ** 31 - 1)
    one(offset=2 ** 62); one(sps=1); one(sps=0); one(sps=-4); one(sps=65); one(sps=2, mode=sm.ESTIMATE, tau=0.0)
    one(mode=2); one(mode=-1); one(tau=np.nan); one(tau=1.0); one(tau=-0.25); one(tau=np.inf); one(mode=sm.ESTIMATE, tau=0.25)
    one(out_offset=cap + 1, n=0); one(out_offset=2 ** 62); one(out_offset=cap - 24)
    refused([ok], reserved=[(0, 1)]); refused([ok], reserved=[(1, -1)])
    refused([ok, ok[:1] + (24,) + ok[2:]])					# [0, 25) and [24, 49): one sample shared
    refused([ok[:1] + (200,) + ok[2:], (0, 8, 800, 4, sm.FIXED, 0.0)])		# [200, 225) and [8, 208), given in descending order
    refused([(0, 0, 100, 4, sm.FIXED, 0.0), (0, 24, 100, 4, sm.FIXED, 0.0)])	# the reservation counts, not n_sym
    for name in ("iq", "records", "out"):
        refused(good, skew=(name, 4))
    # the last jobs that still fit, in the input and in the output; reserved ranges that touch; jobs without a symbol anywhere inside
    last = sm.make_jobs([(0, 0, 100, 4, sm.FIXED, 0.0), (0, 25, 100, 4, sm.FIXED, 0.25), (2900, cap - 25, 100, 4, sm.ESTIMATE, 0.0),
                         (3000, cap, 0, 3, sm.ESTIMATE, 0.0), (5, cap, 3, 8, sm.FIXED, 0.5)])
    rec, out = box.run((iq, last), tag="the last jobs that fit", cap=cap)
    want_rec, want = sm.image((iq, last), SENTINEL)
    assert rec.tobytes() == want_rec.tobytes()
    assert out[:cap].tobytes() == want[:cap].tobytes() and np.all(out[cap:] == SENTINEL)


def test_chain_extract_resample_symbols(amd, box):
    """the QPSK preamble of resample_model's small sc16 stream: extract -> resample -> symbols, each pass over the device buffer of
    the one before, against the three host statements chained.  fosphor_amd_extract.h does not promise the host statement's bits
    (rule 3: float32 sums, within (T + 16) 2^-24 sum|h| max|x| a component), so extract's device output is held to that bound
    against fosphor_amd_extract_host, and from that buffer on -- resample_host, then symbols_host -- the chain is bit for bit"""
    import torch
    import resample_model as rm
    F = amd.Fosphor
    raw, ejobs, _, lag = rm.chain_case()
    taps = F.extract_design(rm.CHAIN_DECIM, rm.CHAIN_TAPS, 0.8)
    rtaps = F.resample_design(rm.CHAIN_UP, rm.CHAIN_DOWN, rm.CHAIN_BRANCH)
    rjobs = F.resample_jobs(ejobs, rm.CHAIN_UP, rm.CHAIN_DOWN, len(rtaps))
    rjobs["out_offset"] = 5
    jobs = np.concatenate([F.symbols_jobs(rjobs, rm.CHAIN_HOLD), F.symbols_jobs(rjobs, rm.CHAIN_HOLD)])
    jobs["offset"][1] += lag						# the preamble alone
    jobs["n"][1] = rm.CHAIN_T
    jobs["out_offset"][1] = sm.job_max_out(jobs[0]) + sm.GUARD
    # the device
    e_views = box.f.extract(torch.from_numpy(raw).cuda(), ejobs, taps, iq_format="sc16")
    e_base = e_views[0].data_ptr() - 8 * int(ejobs["out_offset"][0])		# extract()'s d_out: the views are slices of one buffer
    e_cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    r_views = box.f.resample(e_base, rjobs, rtaps, n_samples=e_cap)
    r_base = r_views[0].data_ptr() - 8 * int(rjobs["out_offset"][0])
    r_cap = int((rjobs["out_offset"] + rjobs["n_out"]).max())
    records, views = box.f.symbols(r_base, jobs, n_samples=r_cap)
    # the host statements
    xh = np.zeros((e_cap, 2), np.float32)
    lib = amd.load()
    assert lib.fosphor_amd_extract_host(raw.ctypes.data, len(raw), 2, ejobs.ctypes.data, len(ejobs), taps.ctypes.data, len(taps),
                                        xh.ctypes.data, e_cap) == 0
    x = np.zeros((e_cap, 2), np.float32)
    for j, v in zip(ejobs, e_views):
        x[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] = v.cpu().numpy().view(np.float32).reshape(-1, 2)
    bound = (len(taps) + 16) * 2.0 ** -24 * np.abs(taps).sum() * np.abs(raw.astype(np.float64) / 32768.0).max()
    print("chain: extract device against host %.3g, bound %.3g" % (np.abs(x.astype(np.float64) - xh).max(), bound))
    assert np.abs(x.astype(np.float64) - xh).max() <= bound
    y = np.zeros((r_cap, 2), np.float32)
    y[5:] = F.resample_host(x, rjobs, rtaps)[0].view(np.float32).reshape(-1, 2)
    want_rec, want = F.symbols_host(y, jobs)
    assert records.tobytes() == want_rec.tobytes()
    for v, w in zip(views, want):
        assert v.cpu().numpy().tobytes() == w.tobytes()
    v = F.symbols_derive(records, rm.CHAIN_HOLD, 1.0)
    print("chain: n_sym %s tau %s lock4 %.3f" % (records["n_sym"], records["tau"], v[1]["lock4"]))
    assert records["n_sym"][0] > sm.BLOCK and records["n_sym"][1] >= rm.CHAIN_SYMBOLS - 2 and v[1]["lock4"] > 0.5
