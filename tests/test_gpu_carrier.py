"""Carrier frequency, phase and derotated symbols on the device (include/fosphor_amd_carrier.h) against the numpy statement
(tests/carrier_model.py) and against fosphor_amd_carrier_host: records and symbols bit for bit, tobytes().

The symbols go into a sentinel-filled buffer in which GUARD samples before, behind and between the jobs' outputs belong to no job
-- and neither do the outputs of a job without a carrier -- and the records into a sentinel-filled buffer with one record more
than there are jobs; both are compared whole with the model's image, so a sample or a record written outside a job's range fails
like a wrong one.  Every run ends by checking that the input buffer is bit-identical, that the instance's ring position, waterfall
and spectrum are untouched (the method of tests/test_gpu_symbols.py) and that the stats delta names the kernels that ran, at most
five launches per call.

Seams of the kernels (the input sets are cm.cases()):
  the loads     16-byte pairs from the first 16-byte boundary into k_car_lag's image: offset 0 .. 3 against odd and even
                out_offsets, a job that ends on the buffer's last sample.
  tiles, blocks n = 0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097 and 2 * 4096 + 5 at M = 2, 4 and 8.
  the lag       L = 1, 2, 16, 63 and 64; n = 2 L - 1 and 2 L, where lag_used switches; n - L on 64, 65, 256, 257, 4096 and 4097,
                so that the last terms of a block, a pass and a tile read symbols of the next.
  the modes     all four combinations of the bits; fixed frequencies of +-0.5 and 0, fixed phases of +-0.5.  Only fixed-fixed
                jobs: k_car_sum, k_car_phase and k_car_turn, neither lag kernel.
  the numbers   all-zero symbols; a NaN symbol (NO_CARRIER, nothing written); an inf symbol; subnormals; 3e38, whose eighth power
                overflows a double; g near +-0.5 with L = 64, where k of rule 3 is at its extremes.
  the prefixes  MAX_JOBS jobs in shuffled order with orders, lags and modes mixed and n <= 130, every 11th with n = 0.
The refusal "more than 2^31 - 1 work-groups" needs 4096 jobs of 2^31 - 4095 outputs each that do not overlap and has no case."""
import errno
import os

import numpy as np
import pytest

import carrier_model as cm

pytestmark = pytest.mark.gpu

EINVAL = -errno.EINVAL
SENTINEL = 0x5a5a5a5a
CASES = cm.cases()
W = cm.RECORD_WORDS
KERNELS = ("k_lag", "k_freq", "k_sum", "k_phase", "k_turn")


def model(name):
    """the model's records and its image of a case's output buffer, computed once a session"""
    return cm.image(CASES[name], SENTINEL, key=name)


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


class Box:
    """an instance, torch views of its waterfall ring and spectrum, and the carrier call through the C ABI"""

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
        iq = cm.buffer(case)
        jobs = np.ascontiguousarray(case[1], cm.JOB_DTYPE)
        d_iq = torch.from_numpy(iq).cuda()
        size = cm.capacity(jobs) if cap is None else max(cap, 0) + cm.GUARD
        d_out = torch.full((size + 1, 2), SENTINEL, dtype=torch.int32, device="cuda")
        d_rec = torch.full(((len(jobs) + 1) * W,), SENTINEL, dtype=torch.int32, device="cuda")
        ptr = {"self": self.f.h, "iq": d_iq.data_ptr(), "jobs": jobs.ctypes.data, "records": d_rec.data_ptr(), "out": d_out.data_ptr()}
        for k in null:
            ptr[k] = None
        if skew:
            ptr[skew[0]] += skew[1]
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        before = self.f.carrier_stats()
        rv = self.f.L.fosphor_amd_carrier(ptr["self"], ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["jobs"],
                                          len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"], size if cap is None else cap)
        after = self.f.carrier_stats()
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
        records = rec[:W * len(jobs)].view(cm.RECORD_DTYPE)
        assert delta == cm.expected_stats(jobs), (tag, delta)
        assert sum(delta[k] for k in KERNELS) <= 5
        return records, out


def symbols_of(buf, job, record):
    at = int(job["out_offset"])
    return buf[at:at + (int(job["n"]) if record["status"] == cm.OK else 0)]


def explain(got_rec, want_rec, got, want, jobs):
    """print the first records and samples that differ, with the job that owns them"""
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    for i in np.flatnonzero((got != want).any(1))[:8]:
        own = [k for k, j in enumerate(jobs) if int(j["out_offset"]) <= i < int(j["out_offset"]) + int(j["n"])]
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
    host_rec, host_views = amd.Fosphor.carrier_host(cm.buffer(case), jobs)
    assert got_rec.tobytes() == host_rec.tobytes(), "records bit-identical to fosphor_amd_carrier_host"
    for v, j, r in zip(host_views, jobs, got_rec):
        assert symbols_of(got, j, r).tobytes() == v.tobytes(), "bit-identical to fosphor_amd_carrier_host"
    again_rec, again = box.run(case, tag=name + " again")
    assert again.tobytes() == got.tobytes() and again_rec.tobytes() == got_rec.tobytes(), "the same call twice is bit-identical"
    if name == "numbers":
        lost = got_rec["status"] == cm.NO_CARRIER
        assert lost.sum() >= 8 and np.all(got_rec["freq"][lost].view(np.uint64) == 0x7ff8000000000000)
        assert np.all(got_rec["phase"][lost].view(np.uint64) == 0x7ff8000000000000)
        for j in jobs[lost]:
            assert np.all(got[int(j["out_offset"]):int(j["out_offset"]) + int(j["n"])] == SENTINEL), "nothing is written"


def test_which_kernels_ran(box):
    """only fixed-fixed jobs: k_car_sum, k_car_phase and k_car_turn, neither lag kernel; every mode: all five; jobs of one symbol
    that estimate: no k_car_lag; jobs without a symbol: k_car_freq and k_car_phase alone"""
    ran = lambda delta: tuple(delta[k] for k in KERNELS)
    rv, rec, out, delta = box.call(CASES["only_fixed"])
    assert rv == 0 and ran(delta) == (0, 0, 1, 1, 1), delta
    rv, rec, out, delta = box.call(CASES["full_table"])
    assert rv == 0 and ran(delta) == (1, 1, 1, 1, 1), delta
    iq = cm.psk(16, 4, 0.01, 0.1, 5)
    one = (iq, cm.make_jobs([(3, 3, 1, 4, cm.ESTIMATE, 16, 0.0, 0.0), (16, 7, 0, 2, cm.ESTIMATE, 1, 0.0, 0.0)]))
    rv, rec, out, delta = box.call(one)
    assert rv == 0 and ran(delta) == (0, 1, 1, 1, 1), delta
    assert rec[:2 * W].tobytes() == cm.carrier(one)[0].tobytes()
    none = (iq, cm.make_jobs([(3, 3, 0, 4, cm.ESTIMATE, 16, 0.0, 0.0), (16, 3, 0, 8, cm.FREQ_FIXED | cm.PHASE_FIXED, 64, 0.5, -0.5)]))
    rv, rec, out, delta = box.call(none)
    assert rv == 0 and ran(delta) == (0, 1, 0, 1, 0), delta
    assert rec[:2 * W].tobytes() == cm.carrier(none)[0].tobytes() and np.all(out == SENTINEL)


def test_a_job_alone_among_others_and_shuffled(box):
    """a record and a job's symbols depend on their job alone: bit-identical alone, among the other jobs of the call, and with the
    table in another order (the outputs keep their places, the work-groups change theirs)"""
    iq, jobs = CASES["mixed"]
    among_rec, among = box.run((iq, jobs), tag="among")
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = box.run((iq, jobs[order]), tag="shuffled")
    assert shuffled.tobytes() == among.tobytes() and shuffled_rec.tobytes() == among_rec[order].tobytes()
    for mode in (cm.ESTIMATE, cm.FREQ_FIXED, cm.PHASE_FIXED, cm.FREQ_FIXED | cm.PHASE_FIXED):
        i = int(np.flatnonzero((jobs["mode"] == mode) & (jobs["n"] > 64))[0])
        alone_rec, alone = box.run((iq, jobs[i:i + 1]), tag="alone %d" % i)
        assert alone_rec[0].tobytes() == among_rec[i].tobytes(), i
        assert symbols_of(alone, jobs[i], alone_rec[0]).tobytes() == symbols_of(among, jobs[i], among_rec[i]).tobytes(), i


def test_python_front_end(box):
    import torch
    iq, jobs = CASES["loads"]
    want_rec, want = cm.carrier((iq, jobs))
    d_iq = torch.from_numpy(iq).cuda()
    for records, views in (box.f.carrier(d_iq, jobs), box.f.carrier(d_iq.view(torch.complex64).reshape(-1), jobs),
                           box.f.carrier(d_iq.data_ptr(), jobs, n_samples=len(iq))):
        assert records.dtype == cm.RECORD_DTYPE and records.tobytes() == want_rec.tobytes()
        assert len(views) == len(jobs)
        for v, w in zip(views, want):
            assert v.dtype == torch.complex64 and v.cpu().numpy().view(np.float32).tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        box.f.carrier(d_iq.data_ptr(), jobs)


def test_einval_table(box):
    """each refused call leaves every sample and record at the sentinel, launches nothing and counts nothing"""
    iq = cm.psk(3000, 4, 0.01, 0.1, 91, 30.0)
    #        offset out  n   order mode lag freq phase
    good = [(0, 5, 500, 4, cm.ESTIMATE, 16, 0.0, 0.0), (2990, 0, 5, 2, cm.FREQ_FIXED | cm.PHASE_FIXED, 1, 0.5, -0.5),
            (3000, 505, 0, 8, cm.ESTIMATE, 64, 0.0, 0.0), (1, 510, 2999, 8, cm.PHASE_FIXED, 64, 0.0, 0.25)]
    cap = 510 + 2999
    rec, out = box.run((iq, cm.make_jobs(good)), tag="good", cap=cap)
    assert np.all(out[cap:] == SENTINEL) and np.all(out[505:510] == SENTINEL) and np.all(out[0:5] != SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        rv, rec, out, delta = box.call((iq, cm.make_jobs(rows)), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL), "nothing is written"
        assert not any(delta.values()), (delta, "nothing is launched or counted")

    for what in ("self", "iq", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (cm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=2999); refused(good, cap=-1); refused(good, cap=cap - 1)
    for row in EINVAL_ROWS(cap):
        refused([row])
    refused([EINVAL_OK, EINVAL_OK[:1] + (99,) + EINVAL_OK[2:]])			# [0, 100) and [99, 199): one sample shared
    refused([EINVAL_OK[:1] + (200,) + EINVAL_OK[2:], (0, 8, 800, 4, 0, 16, 0.0, 0.0)])	# [200, 300) and [8, 808), in descending order
    for name in ("iq", "records", "out"):
        refused(good, skew=(name, 4))
    # the last jobs that still fit, in the input and in the output; outputs that touch; jobs without a symbol anywhere inside
    last = cm.make_jobs([(0, 0, 100, 4, 0, 16, 0.0, 0.0), (0, 100, 100, 2, 0, 64, 0.0, 0.0), (2900, cap - 100, 100, 4, 3, 1, -0.5, 0.5),
                         (3000, cap, 0, 8, 0, 1, 0.0, 0.0), (5, 50, 0, 8, 0, 1, 0.0, 0.0)])
    rec, out = box.run((iq, last), tag="the last jobs that fit", cap=cap)
    want_rec, want = cm.image((iq, last), SENTINEL)
    assert rec.tobytes() == want_rec.tobytes()
    assert out[:cap].tobytes() == want[:cap].tobytes() and np.all(out[cap:] == SENTINEL)


EINVAL_OK = (0, 0, 100, 4, cm.FREQ_FIXED | cm.PHASE_FIXED, 16, 0.25, 0.25)


def EINVAL_ROWS(cap):
    """one job each that rule 8 refuses (the rows of tests/test_carrier_cpu.py)"""
    def one(**kw):
        row = dict(zip(("offset", "out_offset", "n", "order", "mode", "lag", "freq", "phase"), EINVAL_OK))
        row.update(kw)
        return tuple(row.values())

    return [one(offset=-1), one(out_offset=-1), one(n=-1), one(offset=2901), one(offset=3001, n=0), one(offset=2 ** 62, n=2 ** 31 - 1),
            one(offset=2 ** 62), one(out_offset=cap + 1, n=0), one(out_offset=2 ** 62), one(out_offset=cap - 99),
            one(order=0), one(order=1), one(order=3), one(order=6), one(order=16), one(order=-4),
            one(lag=0), one(lag=-1), one(lag=65), one(mode=4), one(mode=7), one(mode=-1),
            one(mode=cm.PHASE_FIXED), one(mode=cm.FREQ_FIXED), one(mode=0), one(mode=0, phase=0.0), one(mode=0, freq=0.0),
            one(freq=np.nan), one(freq=np.inf), one(freq=-np.inf), one(freq=0.5000001), one(freq=-0.5000001),
            one(phase=np.nan), one(phase=np.inf), one(phase=-np.inf), one(phase=0.5000001), one(phase=-0.5000001)]


def test_chain_symbols_carrier(amd, box):
    """the QPSK preamble of resample_model's small sc16 stream: extract -> resample -> symbols -> carrier, each pass over the
    device buffer of the one before.  From the buffer that extract wrote on, the chain is bit for bit the host statements' chained
    (tests/test_gpu_symbols.py holds extract's own bound): resample_host, symbols_host, then carrier_host over the symbols."""
    import torch
    import resample_model as rm
    import symbols_model as sm
    F = amd.Fosphor
    raw, ejobs, _, lag = rm.chain_case()
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
    assert list(cjobs["offset"]) == list(sjobs["out_offset"]) and list(cjobs["n"]) == list(srec["n_sym"])
    before = box.f.carrier_stats()
    records, views = box.f.carrier(s_base, cjobs, n_samples=s_cap)
    after = box.f.carrier_stats()
    assert {k: after[k] - before[k] for k in after} == cm.expected_stats(cjobs)
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
    want_rec, want = F.carrier_host(s, cjobs)
    assert records.tobytes() == want_rec.tobytes()
    for v, w in zip(views, want):
        assert v.cpu().numpy().tobytes() == w.tobytes()
    v = F.carrier_derive(records, 1.0)
    print("chain: n %s freq %s phase %s lock %.3f" % (records["n"], records["freq"], records["phase"], v[1]["lock"]))
    assert records["status"][1] == cm.OK and records["n"][1] >= rm.CHAIN_SYMBOLS - 2 and v[1]["lock"] > 0.5
