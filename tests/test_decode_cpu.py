"""Host side of include/fosphor_amd_decode.h, no GPU: fosphor_amd_decode_host against the numpy statement (tests/decode_model.py),
records and the whole output buffer bit for bit, on every input set the GPU tests use; maximum likelihood by brute force over all
codewords of short frames; the error correction the free distance guarantees; the ties of rules 3 and 4; the CRC check values; the
refusals; a call of exactly MAX_CALL_STEPS and one step more; decode_jobs, decode_steps and decode_derive; that a job's bytes depend on the job alone; the chain decide -> decode on
the host; and the compiled kernels' resources."""
import ctypes as C
import errno
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import decode_model as dm
from _pkg import gr_fosphor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_decode.hip")
HEADER = os.path.join(ROOT, "include", "fosphor_amd_decode.h")
EINVAL = -errno.EINVAL
CASES = dm.cases()
SENTINEL = 0x5a
SENTINEL32 = 0x5a5a5a5a
W = dm.RECORD_WORDS


@pytest.fixture(scope="module")
def lib():
    return gr_fosphor_amd.load()


@pytest.fixture(scope="module")
def F():
    gr_fosphor_amd.load()
    return gr_fosphor_amd.Fosphor


def host(lib, case, n_bytes=None, n_jobs=None, cap=None, null=(), skew=None):
    """-> (return value, records as uint32 [(n_jobs + 1) * 16 + 2], the whole output buffer as uint8 [size]), both sentinel-filled
    before the call.  cap: out_capacity, GUARD bytes of the buffer lie behind it; skew: (pointer name, bytes)"""
    sym = np.ascontiguousarray(case[0], np.uint8)
    keep = sym if len(sym) else np.zeros(8, np.uint8)
    jobs = np.ascontiguousarray(case[1], dm.JOB_DTYPE)
    size = dm.capacity(jobs) if cap is None else max(cap, 0) + dm.GUARD
    buf = np.full((size + 16) // 8, 0x5a5a5a5a5a5a5a5a, np.uint64).view(np.uint8)
    rec = np.full((len(jobs) + 1) * W + 2, SENTINEL32, np.uint32)
    ptr = {"sym": keep.ctypes.data, "jobs": jobs.ctypes.data, "records": rec.ctypes.data, "out": buf.ctypes.data}
    for k in null:
        ptr[k] = None
    if skew:
        ptr[skew[0]] += skew[1]
    rv = lib.fosphor_amd_decode_host(ptr["sym"], len(sym) if n_bytes is None else n_bytes, ptr["jobs"],
                                     len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"], size if cap is None else cap)
    assert np.all(buf[size:] == SENTINEL)
    return rv, rec, buf[:size]


def records_of(rec, n_jobs):
    assert np.all(rec[W * n_jobs:] == SENTINEL32), "a record beyond the jobs' was written"
    return rec[:W * n_jobs].view(dm.RECORD_DTYPE)


def header_value_of(path, name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, open(path).read())
    assert m, name
    return int(m.group(1))


def header_value(name):
    return header_value_of(HEADER, name)


def test_the_dtypes_mirror_the_structs(F):
    L = gr_fosphor_amd._lib
    assert dm.JOB_DTYPE.itemsize == 64 and C.sizeof(L.DecodeJob) == 64
    assert dm.RECORD_DTYPE.itemsize == 64 and C.sizeof(L.DecodeRecord) == 64
    assert F.DECODE_JOB_DTYPE == dm.JOB_DTYPE and F.DECODE_RECORD_DTYPE == dm.RECORD_DTYPE
    for dtype, struct in ((dm.JOB_DTYPE, L.DecodeJob), (dm.RECORD_DTYPE, L.DecodeRecord)):
        assert [(k, dtype.fields[k][1]) for k in dtype.names] == [(k, getattr(struct, k).offset) for k, _ in struct._fields_]
    assert F.DECODE_STATS == dm.STATS and F.DECODE_FLAGS == dm.FLAGS and F.DECODE_STATUS == dm.STATUS
    assert len(dm.STATS) <= 10 == header_value_of(os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_pass.h"), "FOSPHOR_COUNTERS_MAX")
    assert L.SIGNATURES["fosphor_amd_decode_stats"][1][1]._type_._length_ == len(dm.STATS)
    assert (F.DECODE_MAX_JOBS, F.DECODE_MAX_STEPS, F.DECODE_MAX_CALL_STEPS, F.DECODE_BLOCK, F.DECODE_INF) == (
        dm.MAX_JOBS, dm.MAX_STEPS, dm.MAX_CALL_STEPS, dm.BLOCK, dm.INF)
    for name, want in (("MAX_JOBS", dm.MAX_JOBS), ("MAX_STEPS", dm.MAX_STEPS), ("MAX_CALL_STEPS", dm.MAX_CALL_STEPS), ("BLOCK", dm.BLOCK),
                       ("INF", dm.INF), ("TERMINATED", dm.TERMINATED), ("OK", dm.OK), ("CRC_FAIL", dm.CRC_FAIL), ("SHORT", dm.SHORT),
                       ("LDS_BITS", F.DECODE_LDS["bits"]), ("LDS_ACS", F.DECODE_LDS["acs"]), ("LDS_TRACE", F.DECODE_LDS["trace"]),
                       ("LDS_REC", F.DECODE_LDS["rec"])):
        assert header_value("FOSPHOR_AMD_DECODE_" + name) == want, name
    for name in ("decode", "decode_host", "decode_jobs", "decode_steps", "decode_derive", "decode_stats"):
        assert hasattr(F, name), name


def test_the_header_s_functions_are_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fosphor_amd_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["fosphor_amd_decode", "fosphor_amd_decode_derive", "fosphor_amd_decode_from_decide", "fosphor_amd_decode_host",
                        "fosphor_amd_decode_stats", "fosphor_amd_decode_steps"]
    lib = C.CDLL(gr_fosphor_amd.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
        assert name in gr_fosphor_amd._lib.SIGNATURES, name


def test_the_cases_hold_what_they_promise():
    sym, sj = CASES["seams"]
    shapes = [dm.shape(j) for j in sj]
    for k in (3, 5, 7):
        have = {s[0] for s, j in zip(shapes, sj) if j["k"] == k}
        assert set(dm.SEAM_STEPS) | {k - 2, k - 1, k} <= have, (k, sorted(have))
    assert {int(o) & 3 for o in sj["offset"]} == {0, 1, 2, 3} and (sj["offset"] + sj["n"]).max() == len(sym)
    assert set(sj["order"]) == set(dm.ORDERS) and set(sj["n_poly"]) == {2, 3} and set(sj["flags"]) == {0, 1}
    assert set(sj["crc_width"]) == {0, 8, 16, 24, 32} and (sj["steps"] == 0).any() and (sj["steps"] > 0).any()
    assert (sym & 0xf8).any(), "bits above b are set"
    assert {1, 2, 3, 7, 16} <= set(CASES["seams"][1]["period"]) | set(CASES["codes"][1]["period"])
    fr = dm.decode(CASES["frames"])[0]
    fj = CASES["frames"][1]
    for w in (8, 16, 24, 32):
        assert ((fr["status"] == dm.OK) & (fj["crc_width"] == w)).any() and ((fr["status"] == dm.CRC_FAIL) & (fj["crc_width"] == w)).any(), w
    assert (fr["status"] == dm.SHORT).sum() == 1 and (fr["metric"][fj["k"] == 7] == 3).all(), "K = 7 corrects the three planted errors"
    mj = CASES["max_steps"][1]
    mr = dm.image(CASES["max_steps"], SENTINEL, key="max_steps")[0]
    assert dm.shape(mj[0])[0] == dm.MAX_STEPS and mr["status"][0] == dm.OK and mr["metric"][0] == 2 * dm.MAX_STEPS // 50
    full = CASES["full_table"][1]
    assert len(full) == dm.MAX_JOBS and full["n"].max() <= 40 and (full["n"] == 0).sum() >= dm.MAX_JOBS // 11


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_model(lib, F, name):
    case = CASES[name]
    jobs = case[1]
    rv, rec, got = host(lib, case)
    assert rv == 0
    want_rec, want = dm.image(case, SENTINEL, key=name)
    got_rec = records_of(rec, len(jobs))
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical"
    for i in np.flatnonzero(got != want)[:10]:
        print("byte %d got %s want %s" % (i, got[i], want[i]))
    assert got.tobytes() == want.tobytes(), "bytes bit-identical, every other byte at the sentinel"
    records, views = F.decode_host(case[0], jobs)
    assert records.tobytes() == want_rec.tobytes(), "the Python front end gives the same records"
    for j, r, v in zip(jobs, records, views):
        at = int(j["out_offset"])
        assert len(v) == (r["n_bits"] + 7) // 8 and v.tobytes() == want[at:at + len(v)].tobytes()


def test_call_limit(lib):
    """64 jobs of MAX_STEPS, exactly MAX_CALL_STEPS: the host statement against the model, bit for bit; the same table with one
    more job of one step is refused with every byte and record at the sentinel"""
    case = dm.call_limit_case()
    jobs = case[1]
    steps = [dm.shape(j)[0] for j in jobs]
    assert len(jobs) == dm.LIMIT_JOBS == 64 and set(steps) == {dm.MAX_STEPS} and sum(steps) == dm.MAX_CALL_STEPS
    assert len({(int(j["k"]), int(j["period"]), int(j["flags"])) for j in jobs}) == 2
    rv, rec, got = host(lib, case)
    assert rv == 0
    want_rec, want = dm.image(case, SENTINEL, key="call_limit")
    got_rec = records_of(rec, len(jobs))
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical"
    assert got.tobytes() == want.tobytes(), "bytes bit-identical, every other byte at the sentinel"
    assert (got_rec["metric"] > 0).all() and (got_rec["n_steps"] == dm.MAX_STEPS).all() and {dm.OK, dm.CRC_FAIL} == set(got_rec["status"])
    more = dm.one_step_more(case)
    assert sum(dm.shape(j)[0] for j in more[1]) == dm.MAX_CALL_STEPS + 1 and more[1][:64].tobytes() == jobs.tobytes()
    rv, rec, out = host(lib, more)
    assert rv == EINVAL and np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"


def test_a_job_alone_among_others_and_shuffled(F):
    """a record and a job's bytes depend on their job alone"""
    sym, jobs = CASES["codes"]
    among_rec, among = F.decode_host(sym, jobs)
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = F.decode_host(sym, jobs[order])
    assert shuffled_rec.tobytes() == among_rec[order].tobytes()
    for k, i in enumerate(order):
        assert shuffled[k].tobytes() == among[i].tobytes()
    for i in (0, 1, 2, 3, 4, len(jobs) - 1):
        alone_rec, alone = F.decode_host(sym, jobs[i:i + 1])
        assert alone_rec[0].tobytes() == among_rec[i].tobytes() and alone[0].tobytes() == among[i].tobytes(), i


# ---- maximum likelihood -----------------------------------------------------------------------------------------------------------

P_34_THIRD = (3, (0b011, 0b101, 0))			# the 3/4 pattern over a three-stream code: the third stream is never sent


@pytest.mark.parametrize("code", [dm.K3, dm.K5, dm.K4_THIRD], ids=["k3", "k5", "k4_third"])
@pytest.mark.parametrize("punctured", [False, True])
def test_maximum_likelihood_by_brute_force(F, code, punctured):
    """not self-consistency: over random received bits, metric is the least Hamming distance between the received bits and the
    sent bits of ALL 2^T input sequences (2^(T - k + 1) with TERMINATED), found by encoding every one; and the decoded bits,
    encoded again, lie at exactly metric from the input"""
    k, polys = code
    n_poly = 3 if polys[2] else 2
    punct = (P_34_THIRD if n_poly == 3 else dm.P_34) if punctured else (dm.P3_NONE if n_poly == 3 else dm.P_NONE)
    rng = np.random.default_rng(100 * k + punctured)
    parts, jobs, at = [], [], 0
    for T in (1, 2, k - 1, k, 7, 9, 10):
        for term in (0, 1):
            for rep in range(4):
                n = dm.kept(T, *punct)
                parts.append(rng.integers(0, 2, n).astype(np.uint8) | (rng.integers(0, 128, n).astype(np.uint8) << 1))
                jobs.append(dm.make_job(at, 0, n, 2, code, punct, dm.CRC_NONE, T, term))
                at += n
    sym, jobs = np.concatenate(parts), dm.place(jobs)
    rec, views = F.decode_host(sym, jobs)
    assert rec.tobytes() == dm.decode((sym, jobs))[0].tobytes()
    for j, r, v in zip(jobs, rec, views):
        T, n_bits, n_coded = dm.shape(j)
        recv = sym[int(j["offset"]):int(j["offset"]) + n_coded] & 1
        tail = [0] * (T - n_bits)
        least = min(int((dm.puncture(dm.encode(list(msg) + tail, k, polys, n_poly), n_poly, *punct) != recv).sum())
                    for msg in itertools.product((0, 1), repeat=n_bits))
        assert r["metric"] == least, (j, r, least)
        path = list(dm.unpack(v, n_bits)) + tail
        again = dm.puncture(dm.encode(path, k, polys, n_poly), n_poly, *punct)
        assert int((again != recv).sum()) == r["metric"], "the decoded path lies at metric from the input"


def test_k7_corrects_any_four_errors(F):
    """K = 7 (171, 133) has free distance 10: any 4 inverted coded bits of a terminated 200-bit frame are corrected, metric == 4.
    300 random sets of four, and every run of four consecutive bits at 40 places"""
    rng = np.random.default_rng(7)
    info = rng.integers(0, 2, 94)
    sets = [tuple(rng.choice(200, 4, replace=False)) for _ in range(300)] + [tuple(range(a, a + 4)) for a in range(0, 196, 5)]
    parts, jobs = [], []
    for i, flips in enumerate(sets):
        sym, T = dm.frame(info, dm.K7, dm.P_NONE, 4, dm.CRC_NONE, True, flips=flips)
        assert T == 100 and len(sym) == 100
        parts.append(sym)
        jobs.append(dm.make_job(100 * i, 0, 100, 4, dm.K7, dm.P_NONE, dm.CRC_NONE, 0, dm.TERMINATED))
    rec, views = F.decode_host(np.concatenate(parts), dm.place(jobs))
    assert np.all(rec["metric"] == 4) and np.all(rec["n_bits"] == 94) and np.all(rec["end_state"] == 0)
    want = np.packbits(info.astype(np.uint8)).tobytes()
    assert all(v.tobytes() == want for v in views)


def test_the_ties_of_rules_3_and_4(F):
    """K = 3 (7, 5).  One step, received 01: input 0 sends 00 and input 1 sends 11, one error each: states 0 and 2 tie and the
    smaller is best_state.  Five steps of which only the first sends a bit (period 16, stream 0 in step 0): every later comparison
    is a tie but where a path's first input disagrees with that bit; ties go to x = 0, so the received bit comes out first and
    zeros behind it"""
    job = dm.make_job(0, 0, 1, 4, dm.K3, dm.P_NONE, dm.CRC_NONE, 1, 0)
    rec, views = F.decode_host(np.array([0b01], np.uint8), job)
    assert (rec["n_steps"][0], rec["best_state"][0], rec["best_metric"][0], rec["end_state"][0], rec["metric"][0]) == (1, 0, 1, 0, 1)
    assert list(dm.unpack(views[0], 1)) == [0]
    lone = (16, (1, 0, 0))
    for bit, want in ((0, [0, 0, 0, 0, 0]), (1, [1, 0, 0, 0, 0])):
        job = dm.make_job(0, 0, 1, 2, dm.K3, lone, dm.CRC_NONE, 5, 0)
        sym = np.array([bit], np.uint8)
        rec, views = F.decode_host(sym, job)
        assert rec.tobytes() == dm.decode((sym, job))[0].tobytes()
        assert (rec["n_coded"][0], rec["metric"][0], rec["best_state"][0]) == (1, 0, 0) and list(dm.unpack(views[0], 5)) == want
    # TERMINATED with T < k - 1: no bit is left, nothing is owned, the record stands
    for T in (1, 3, 5):
        job = dm.make_job(0, 8, 8, 4, dm.K7, dm.P_NONE, dm.CRC8, T, dm.TERMINATED)
        sym = np.arange(8, dtype=np.uint8)
        rv, raw, out = host(gr_fosphor_amd.load(), (sym, job))
        rec = records_of(raw, 1)
        assert rv == 0 and np.all(out == SENTINEL) and rec.tobytes() == dm.decode((sym, job))[0].tobytes()
        assert (rec["n_steps"][0], rec["n_bits"][0], rec["end_state"][0], rec["status"][0]) == (T, 0, 0, dm.SHORT)
    # no symbol at all
    job = dm.make_job(0, 0, 0, 4, dm.K7, dm.P_NONE)
    rec, views = F.decode_host(np.zeros(0, np.uint8), job)
    want = np.zeros(1, dm.RECORD_DTYPE)
    want["k"] = 7
    assert rec.tobytes() == want.tobytes() and len(views[0]) == 0


@pytest.mark.parametrize("crc,check", [(dm.CRC8, 0xf4), (dm.CRC16, 0x29b1), (dm.CRC24, 0x21cf02), (dm.CRC32, 0x0376e6e7)])
def test_crc_check_values(F, crc, check):
    """the catalogued check values over the ASCII bytes "123456789", through the decoder: crc_calc and crc_recv"""
    info = np.unpackbits(np.frombuffer(b"123456789", np.uint8))
    assert dm.crc_bits(info, crc) == check
    sym, T = dm.frame(info, dm.K7, dm.P_34, 8, crc, True, flips=(5, 70))
    job = dm.make_job(0, 0, len(sym), 8, dm.K7, dm.P_34, crc, T, dm.TERMINATED)
    rec, views = F.decode_host(sym, job)
    assert (rec["crc_calc"][0], rec["crc_recv"][0], rec["status"][0], rec["metric"][0]) == (check, check, dm.OK, 2)
    assert views[0][:9].tobytes() == b"123456789"
    wrong = dm.make_job(0, 0, len(sym), 8, dm.K7, dm.P_34, crc[:2] + (crc[2] ^ 1, crc[3]), T, dm.TERMINATED)
    rec, _ = F.decode_host(sym, wrong)
    assert rec["status"][0] == dm.CRC_FAIL and rec["crc_recv"][0] == check and rec["crc_calc"][0] != check
    short = dm.make_job(0, 0, len(sym), 8, dm.K7, dm.P_34, crc, crc[0] + 5, dm.TERMINATED)	# w - 1 bits are left
    rec, _ = F.decode_host(sym, short)
    assert (rec["n_bits"][0], rec["status"][0], rec["crc_calc"][0], rec["crc_recv"][0]) == (crc[0] - 1, dm.SHORT, 0, 0)


# ---- the refusals -----------------------------------------------------------------------------------------------------------------

N_SYM, CAP = 3000, 4096


def good_jobs():
    """four jobs over 3000 bytes and a capacity of 4096: the first fills d_out[0 .. 64), the last ends on both buffers' last bytes"""
    return np.concatenate([dm.make_job(0, 0, 512, 4, dm.K7, dm.P_NONE, dm.CRC16, 0, dm.TERMINATED),		# 512 steps, 506 bits: 64 bytes
                           dm.make_job(7, 64, 100, 8, dm.K5, dm.P_34, dm.CRC_NONE, 0, 0),			# 225 steps: 32 bytes
                           dm.make_job(3000, 96, 0, 2, dm.K3, dm.P_NONE),					# no symbol, at the end
                           dm.make_job(2000, CAP - 64, 1000, 2, dm.K7, dm.P_NONE, dm.CRC32, 0, 0)])		# 500 steps: 64 bytes


def refusal_rows():
    """one job each that rule 9 refuses: (the fields to change of good_jobs()[0])"""
    big = 2 ** 62
    return [dict(offset=-1), dict(out_offset=-8), dict(n=-1), dict(offset=2489), dict(offset=3001, n=0), dict(offset=big), dict(offset=big, n=2 ** 31 - 1),
            dict(out_offset=CAP - 56), dict(out_offset=CAP + 8, n=0), dict(out_offset=big), dict(out_offset=4), dict(out_offset=1), dict(out_offset=12, n=0),
            dict(order=0), dict(order=1), dict(order=3), dict(order=16), dict(order=-2), dict(k=2), dict(k=8), dict(k=0), dict(n_poly=1), dict(n_poly=4),
            dict(n_poly=0), dict(period=0), dict(period=17), dict(crc_width=1), dict(crc_width=12), dict(crc_width=33), dict(crc_width=64),
            dict(polys=(0, 0o133, 0)), dict(polys=(0o171, 0, 0)), dict(polys=(0o371, 0o133, 0)), dict(polys=(0o171, 128, 0)), dict(polys=(0o171, 0o133, 1)),
            dict(n_poly=3), dict(n_poly=3, polys=(0o171, 0o133, 128), punct=(1, 1, 1)), dict(punct=(2, 1, 0)), dict(punct=(1, 2, 0)), dict(punct=(0, 0, 0)),
            dict(punct=(1, 1, 1)), dict(period=3, punct=(8, 1, 0)), dict(steps=-1), dict(steps=513), dict(steps=dm.MAX_STEPS + 1),
            dict(n=2 ** 31 - 1, offset=0), dict(order=8, n=3000, period=16, punct=(1, 0, 0)), dict(crc_poly=1 << 16), dict(crc_init=1 << 16), dict(crc_xorout=1 << 16), dict(crc_width=0),
            dict(crc_width=0, crc_poly=0, crc_init=1), dict(crc_width=8), dict(flags=2), dict(flags=3), dict(flags=-1), dict(reserved=1), dict(reserved=1 << 31)]


def changed(job, **kw):
    j = job.copy()
    for k, v in kw.items():
        j[k] = v
    return j


def test_einval_table(lib):
    """each refused call leaves every byte and every record at the sentinel; the last jobs that fit are accepted"""
    rng = np.random.default_rng(91)
    sym = rng.integers(0, 256, N_SYM).astype(np.uint8)
    good = good_jobs()
    rv, rec, out = host(lib, (sym, good), cap=CAP)
    want_rec, want = dm.image((sym, good), SENTINEL)
    assert rv == 0 and records_of(rec, 4).tobytes() == want_rec.tobytes() and out[:CAP].tobytes() == want[:CAP].tobytes()
    assert np.all(out[96:CAP - 64] == SENTINEL) and list(want_rec["n_steps"]) == [512, 225, 0, 500]

    def refused(jobs, **kw):
        kw.setdefault("cap", CAP)
        rv, rec, out = host(lib, (sym, jobs), **kw)
        assert rv == EINVAL, (jobs, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"

    for what in ("sym", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused(np.repeat(good[2:3], dm.MAX_JOBS + 1))
    refused(good, n_bytes=-1); refused(good, n_bytes=2999); refused(good, cap=-1); refused(good, cap=CAP - 8)
    for row in refusal_rows():
        refused(changed(good[:1], **row))
    refused(np.concatenate([good[:1], changed(good[1:2], out_offset=56)]))			# [0, 64) and [56, 88)
    refused(np.concatenate([changed(good[1:2], out_offset=200), changed(good[:1], out_offset=168)]))	# [200, 232) and [168, 232), descending
    for name, by in (("records", 4), ("out", 4), ("out", 1)):
        refused(good, skew=(name, by))
    # the sum of the steps of a call: 64 jobs of MAX_STEPS are 2^22 steps and fit, one step more does not
    long = dm.make_job(0, 0, N_SYM, 8, dm.K3, (16, (1, 0, 0)), dm.CRC_NONE, dm.MAX_STEPS, 0)	# one bit in 16 steps: 4096 bits
    many = np.repeat(long, 64)
    many["out_offset"] = 8192 * np.arange(64)
    assert host(lib, (sym, many), cap=64 * 8192)[0] == 0
    refused(np.concatenate([many, changed(long, steps=1, out_offset=64 * 8192)]), cap=65 * 8192)
    # a job without a symbol anywhere inside; d_sym needs no alignment; MAX_JOBS jobs
    rv, rec, out = host(lib, (sym, changed(good[2:3], offset=5, out_offset=CAP)), cap=CAP)
    assert rv == 0 and np.all(out == SENTINEL)
    rv, rec, out = host(lib, (sym[1:], changed(good[:1], offset=0)), cap=CAP, skew=("sym", 0))
    assert rv == 0
    assert host(lib, (sym, np.repeat(good[2:3], dm.MAX_JOBS)), cap=CAP)[0] == 0
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    rec = np.full(W, SENTINEL32, np.uint32)
    out = np.full(256, SENTINEL32, np.uint32)
    assert lib.fosphor_amd_decode(None, sym.ctypes.data, N_SYM, good.ctypes.data, 1, rec.ctypes.data, out.ctypes.data, 1024) == EINVAL
    assert np.all(rec == SENTINEL32) and np.all(out == SENTINEL32)
    assert lib.fosphor_amd_decode_stats(None, None) == EINVAL


def test_steps_from_decide_and_derive(lib, F):
    import decide_model as dec
    for n, order, (period, punct) in itertools.product((0, 1, 2, 7, 100, 301, 2 ** 20), dm.ORDERS, (dm.P_NONE, dm.P_23, dm.P_34, dm.P_78, dm.P_16, dm.P3_16)):
        n_poly = 3 if punct[2] else 2
        T = F.decode_steps(n, order, n_poly, period, punct)
        assert T == dm.steps_that_fit(n, order, period, punct)
        assert dm.kept(T, period, punct) <= n * dm.bits_of(order) < dm.kept(T + 1, period, punct) or dm.kept(T + 1, period, punct) == dm.kept(T, period, punct)
    masks = np.array([1, 1, 0], np.uint16)
    for bad in ((-1, 4, 2, 1), (8, 3, 2, 1), (8, 4, 1, 1), (8, 4, 4, 1), (8, 4, 2, 0), (8, 4, 2, 17)):
        assert lib.fosphor_amd_decode_steps(*bad, masks.ctypes.data) == EINVAL, bad
    assert lib.fosphor_amd_decode_steps(8, 4, 2, 1, None) == EINVAL
    for bad in ((2, 1, 0), (0, 0, 0), (1, 1, 1)):
        assert lib.fosphor_amd_decode_steps(8, 4, 2, 1, np.array(bad, np.uint16).ctypes.data) == EINVAL, bad
    assert lib.fosphor_amd_decode_steps(2 ** 31 - 1, 8, 2, 16, np.array([1, 0, 0], np.uint16).ctypes.data) == EINVAL, "no int holds it"
    with pytest.raises(ValueError):
        F.decode_steps(8, 3)
    # from_decide: behind the word, all of it or n_payload; no word found: nothing; no word asked for: from the job's first byte
    dj = dec.make_jobs([(0, 40, 500, 4, dec.UW, 0, 32, 0, 0, 2), (0, 600, 300, 8, dec.UW, 0, 32, 0, 0, 2), (0, 1000, 200, 2, dec.DIFF)])
    dr = np.zeros(3, dec.RECORD_DTYPE)
    dr["n"], dr["order"], dr["status"], dr["uw_pos"] = (500, 300, 200), (4, 8, 2), (dec.OK, dec.NO_UW, dec.OK), (100, 7, -1)
    jobs = F.decode_jobs(dj, dr, 32)
    assert jobs.dtype == dm.JOB_DTYPE and list(jobs["offset"]) == [40 + 132, 600, 1000] and list(jobs["n"]) == [368, 0, 200]
    assert list(jobs["order"]) == [4, 8, 2] and set(jobs["k"]) == {7} and [tuple(p) for p in jobs["polys"]] == [(0o171, 0o133, 0)] * 3
    assert list(jobs["out_offset"]) == [0, 48 + 8, 56 + 8] and not jobs["reserved"].any()		# 368 steps: 48 bytes; none; 100 steps: 16
    jobs = F.decode_jobs(dj[:1], dr[:1], 32, n_payload=300, k=5, polys=(0o23, 0o35), period=3, punct=(3, 5), flags="terminated", crc_width=16,
                         crc_poly=0x1021, crc_init=0xffff, gap=1)
    j = jobs[0]
    assert (j["n"], j["k"], j["n_poly"], j["period"], j["crc_width"], j["flags"], j["crc_poly"], j["crc_init"]) == (300, 5, 2, 3, 16, 1, 0x1021, 0xffff)
    assert tuple(j["punct"]) == (3, 5, 0) and j["steps"] == 0
    job = gr_fosphor_amd._lib.DecodeJob()
    job.out_offset, job.k = 99, 9
    make = lib.fosphor_amd_decode_from_decide
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), 32, 368, C.byref(job)) == 0
    assert (job.offset, job.out_offset, job.n, job.order, job.steps, job.flags, job.k, job.crc_width, job.reserved) == (172, 0, 368, 4, 0, 0, 0, 0, 0)
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), 32, 369, C.byref(job)) == EINVAL, "the payload runs past the job"
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), 401, 0, C.byref(job)) == EINVAL, "the word runs past the job"
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), 32, -1, C.byref(job)) == EINVAL
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), -1, 0, C.byref(job)) == EINVAL
    assert make(dj[2:].tobytes(), dr[2:].tobytes(), 32, 201, C.byref(job)) == EINVAL
    assert make(dj[2:].tobytes(), dr[2:].tobytes(), 32, 200, C.byref(job)) == 0 and (job.offset, job.n) == (1000, 200)
    assert make(dj[1:2].tobytes(), dr[1:2].tobytes(), 32, 5000, C.byref(job)) == 0 and job.n == 0, "no word: nothing to decode"
    bad = dr[:1].copy()
    bad["order"] = 3
    assert make(dj[:1].tobytes(), bad.tobytes(), 32, 0, C.byref(job)) == EINVAL
    bad = dj[:1].copy()
    bad["out_offset"] = -4
    assert make(bad.tobytes(), dr[:1].tobytes(), 32, 0, C.byref(job)) == EINVAL
    assert make(None, dr[:1].tobytes(), 32, 0, C.byref(job)) == EINVAL and make(dj[:1].tobytes(), None, 32, 0, C.byref(job)) == EINVAL
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), 32, 0, None) == EINVAL
    with pytest.raises(ValueError):
        F.decode_jobs(dj, dr[:2], 32)
    # records built by hand
    r = np.zeros(1, dm.RECORD_DTYPE)
    r["n_steps"], r["n_coded"], r["metric"] = 300, 400, 10
    v = F.decode_derive(r)[0]
    assert set(v) == set(F.DECODE_VALUES) and v == dict(channel_ber=0.025, rate=0.75, crc_ok=1.0)
    r["status"] = dm.CRC_FAIL
    assert F.decode_derive(r)[0]["crc_ok"] == 0.0
    assert F.decode_derive(np.zeros(1, dm.RECORD_DTYPE))[0] == dict(channel_ber=0.0, rate=0.0, crc_ok=1.0), "0 / 0 is 0"
    vals = gr_fosphor_amd._lib.DecodeValues()
    assert lib.fosphor_amd_decode_derive(None, C.byref(vals)) == EINVAL and lib.fosphor_amd_decode_derive(r.tobytes(), None) == EINVAL


# ---- function ---------------------------------------------------------------------------------------------------------------------

CHAIN_SEED, CHAIN_SNR_DB, CHAIN_INFO = 5, 8.0, 400


def chain_burst():
    """a QPSK burst at symbol level: 16 symbols of noise, a 32-symbol word, then a K = 7, 3/4-punctured, CRC-16, terminated payload
    of 400 info bits; white noise at 8 dB -> (iq float32 [n][2], word, info, payload symbols)"""
    rng = np.random.default_rng(CHAIN_SEED)
    word = rng.integers(0, 4, 32).astype(np.uint8)
    info = rng.integers(0, 2, CHAIN_INFO)
    payload, T = dm.frame(info, dm.K7, dm.P_34, 4, dm.CRC16, True)
    idx = np.concatenate([rng.integers(0, 4, 16).astype(np.uint8), word, payload])
    z = np.exp(2j * np.pi * idx / 4) + (rng.standard_normal(len(idx)) + 1j * rng.standard_normal(len(idx))) * 10 ** (-CHAIN_SNR_DB / 20) / np.sqrt(2)
    return np.stack([z.real, z.imag], 1).astype(np.float32), word, info, payload


def test_chain_on_the_host(F):
    """decide_host -> decode_jobs -> decode_host over a synthetic QPSK burst.  Seed and noise were chosen on the CPU (of seeds
    1 .. 8 at 8 dB, seed 5): the word is found at 16 with 1 error of 4 allowed, 3 payload symbols are decided wrong, the decoder
    corrects their 4 coded bits (metric 4) and the CRC, 0x77fb, holds: the values the host gives, asserted as they are"""
    import decide_model as dec
    iq, word, info, payload = chain_burst()
    djobs = dec.make_jobs([(0, 0, len(iq), 4, dec.UW, 0, 32, 0, 0, 4)])
    drec, dviews = F.decide_host(iq, djobs, word)
    assert (drec["status"][0], drec["uw_pos"][0], drec["uw_rot"][0]) == (dec.OK, 16, 0)
    sym = np.zeros(dec.owned(len(iq)), np.uint8)
    sym[:len(iq)] = dviews[0]
    jobs = F.decode_jobs(djobs, drec, 32, k=7, polys=(0o171, 0o133), period=3, punct=(0b011, 0b101), steps=422, flags="terminated",
                         crc_width=16, crc_poly=0x1021, crc_init=0xffff)
    assert (jobs["offset"][0], jobs["n"][0]) == (48, len(payload))
    rec, views = F.decode_host(sym, jobs)
    assert rec.tobytes() == dm.decode((sym, jobs))[0].tobytes()
    got = sym[48:48 + len(payload)]
    wrong = int((got != payload).sum())
    coded = lambda s: ((s[:, None] >> (1, 0)) & 1).reshape(-1)[:563]
    bit_errors = int((coded(got) != coded(payload)).sum())
    v = F.decode_derive(rec)[0]
    print("chain: uw_errors %d, %d symbols wrong, %d coded bits wrong, metric %d, status %d, ber %.4f rate %.4f"
          % (drec["uw_errors"][0], wrong, bit_errors, rec["metric"][0], rec["status"][0], v["channel_ber"], v["rate"]))
    assert (drec["uw_errors"][0], wrong, bit_errors) == (1, 3, 4), "the input: what the channel did"
    assert rec["metric"][0] == 4 == bit_errors, "every channel error is corrected and counted"
    assert (rec["status"][0], rec["n_steps"][0], rec["n_bits"][0], rec["n_coded"][0], rec["end_state"][0]) == (dm.OK, 422, 416, 563, 0)
    assert rec["crc_calc"][0] == rec["crc_recv"][0] == dm.crc_bits(info, dm.CRC16) == 0x77fb
    assert list(dm.unpack(views[0], CHAIN_INFO)) == list(info), "the decoded bits are the planted ones"
    assert v["crc_ok"] == 1.0 and abs(v["rate"] - 0.75) < 0.002 and v["channel_ber"] == rec["metric"][0] / 563


def test_decode_kernels_meet_their_resources(F):
    """-Rpass-analysis=kernel-resource-usage: every kernel of fosphor_decode.hip has 0 bytes of scratch, at most 64 VGPRs and the
    static LDS that the header states for it"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-x", "hip", "--cuda-device-only",
                        "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        for key in ("ScratchSize", "VGPRs", "LDS Size"):
            m = re.search(r"remark:\s+%s( \[bytes/(lane|block)\])?: (\d+)" % key, line)
            if m and cur:
                found.setdefault(cur, {})[key] = int(m.group(3))
    ours = {k: v for k, v in found.items() if "k_dcd_" in k}
    assert len(ours) == 4 and len(found) == 4, sorted(found)
    for name, res in ours.items():
        form = re.search(r"k_dcd_(bits|acs|trace|rec)", name).group(1)
        print(form, res)
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 1 << 30) <= 64, (name, res)
        assert res.get("LDS Size") == F.DECODE_LDS[form] == header_value("FOSPHOR_AMD_DECODE_LDS_" + form.upper()), (name, res)
