"""Host side of include/fosphor_amd_rs.h, no GPU: the known answers of the field, the generators and the scrambler;
fosphor_amd_rs_host against the numpy statement (tests/rs_model.py), records and the whole output buffer bit for bit, on every
input set the GPU tests use; every pattern of up to t errors corrected; what a status of OK promises; the encoder against the
model and round trips with both scramble flags; the refusals; a call of exactly MAX_CALL_CODEWORDS and one job more; rs_jobs and
rs_derive; that a job's bytes depend on the job alone; the chain decode -> rs on the host; and the compiled kernels' resources."""
import ctypes as C
import errno
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import rs_model as rm
from _pkg import gr_fosphor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_rs.hip")
HEADER = os.path.join(ROOT, "include", "fosphor_amd_rs.h")
EINVAL = -errno.EINVAL
CASES = rm.cases()
SENTINEL = 0x5a
SENTINEL32 = 0x5a5a5a5a
W = rm.RECORD_WORDS


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
    data = np.ascontiguousarray(case[0], np.uint8)
    keep = data if len(data) else np.zeros(8, np.uint8)
    jobs = np.ascontiguousarray(case[1], rm.JOB_DTYPE)
    size = rm.capacity(jobs) if cap is None else max(cap, 0) + rm.GUARD
    buf = np.full((size + 16) // 8, 0x5a5a5a5a5a5a5a5a, np.uint64).view(np.uint8)
    rec = np.full((len(jobs) + 1) * W + 2, SENTINEL32, np.uint32)
    ptr = {"in": keep.ctypes.data, "jobs": jobs.ctypes.data, "records": rec.ctypes.data, "out": buf.ctypes.data}
    for k in null:
        ptr[k] = None
    if skew:
        ptr[skew[0]] += skew[1]
    rv = lib.fosphor_amd_rs_host(ptr["in"], len(data) if n_bytes is None else n_bytes, ptr["jobs"],
                                 len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"], size if cap is None else cap)
    assert np.all(buf[size:] == SENTINEL)
    return rv, rec, buf[:size]


def records_of(rec, n_jobs):
    assert np.all(rec[W * n_jobs:] == SENTINEL32), "a record beyond the jobs' was written"
    return rec[:W * n_jobs].view(rm.RECORD_DTYPE)


def header_value_of(path, name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, open(path).read())
    assert m, name
    return int(m.group(1))


def header_value(name):
    return header_value_of(HEADER, name)


def test_the_dtypes_mirror_the_structs(F):
    L = gr_fosphor_amd._lib
    assert rm.JOB_DTYPE.itemsize == 64 and C.sizeof(L.RsJob) == 64
    assert rm.RECORD_DTYPE.itemsize == 64 and C.sizeof(L.RsRecord) == 64
    assert F.RS_JOB_DTYPE == rm.JOB_DTYPE and F.RS_RECORD_DTYPE == rm.RECORD_DTYPE
    for dtype, struct in ((rm.JOB_DTYPE, L.RsJob), (rm.RECORD_DTYPE, L.RsRecord)):
        assert [(k, dtype.fields[k][1]) for k in dtype.names] == [(k, getattr(struct, k).offset) for k, _ in struct._fields_]
    assert F.RS_STATS == rm.STATS and F.RS_FLAGS == rm.FLAGS and F.RS_STATUS == rm.STATUS and F.RS_FAILED == rm.FAILED
    assert len(rm.STATS) <= header_value_of(os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_pass.h"), "FOSPHOR_COUNTERS_MAX")
    assert L.SIGNATURES["fosphor_amd_rs_stats"][1][1]._type_._length_ == len(rm.STATS)
    assert (F.RS_MAX_JOBS, F.RS_MAX_ROOTS, F.RS_MAX_DEPTH, F.RS_MAX_CALL_CODEWORDS) == (rm.MAX_JOBS, rm.MAX_ROOTS, rm.MAX_DEPTH, rm.MAX_CALL_CODEWORDS)
    for name, want in (("MAX_JOBS", rm.MAX_JOBS), ("MAX_ROOTS", rm.MAX_ROOTS), ("MAX_DEPTH", rm.MAX_DEPTH),
                       ("MAX_CALL_CODEWORDS", rm.MAX_CALL_CODEWORDS), ("DESCRAMBLE_IN", rm.IN), ("DESCRAMBLE_OUT", rm.OUT), ("OK", rm.OK),
                       ("FAIL", rm.FAIL), ("FAILED", rm.FAILED), ("LDS_SYN", F.RS_LDS["syn"]), ("LDS_FIX", F.RS_LDS["fix"]),
                       ("LDS_OUT", F.RS_LDS["out"]), ("LDS_REC", F.RS_LDS["rec"])):
        assert header_value("FOSPHOR_AMD_RS_" + name) == want, name
    assert F.RS_CCSDS == dict(zip(("gf_poly", "fcr", "prim", "n_roots"), rm.CCSDS)) and tuple(F.RS_DVB.values()) == rm.DVB
    for name in ("rs", "rs_host", "rs_encode", "rs_jobs", "rs_derive", "rs_stats"):
        assert hasattr(F, name), name


def test_the_header_s_functions_are_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fosphor_amd_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["fosphor_amd_rs", "fosphor_amd_rs_derive", "fosphor_amd_rs_encode_host", "fosphor_amd_rs_from_decode",
                        "fosphor_amd_rs_host", "fosphor_amd_rs_stats"]
    lib = C.CDLL(gr_fosphor_amd.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
        assert name in gr_fosphor_amd._lib.SIGNATURES, name


# ---- known answers ------------------------------------------------------------------------------------------------------------------

QR_DATA = (32, 91, 11, 120, 209, 114, 220, 77, 67, 64, 236, 17, 236, 17, 236, 17)
QR_PARITY = (196, 35, 39, 119, 235, 215, 231, 226, 93, 23)


def host_generator(F, code):
    """g(x) highest coefficient first through the library: the parity of the data 0 .. 0 1 is x^n_roots mod g(x) = g(x) - x^n_roots"""
    k = 5
    job = rm.make_job(0, 0, k + code[3], 1, code)
    frame = F.rs_encode(np.array([0] * (k - 1) + [1], np.uint8), job)
    return [1] + [int(v) for v in frame[k:]]


def test_known_answers(F):
    """the QR code's example codeword, the coefficient logs of two generators over 0x11d, the palindromic CCSDS generator and the
    CCSDS pseudo-random sequence: the model and the library"""
    job = rm.make_job(0, 0, 26, 1, rm.QR10)
    assert tuple(rm.parity(QR_DATA, rm.QR10)) == QR_PARITY
    assert tuple(F.rs_encode(np.array(QR_DATA, np.uint8), job)) == QR_DATA + QR_PARITY
    log = rm.field(0x11d)[1]
    for code, logs in ((rm.QR10, (0, 251, 67, 46, 61, 118, 70, 64, 94, 32, 45)),
                       ((0x11d, 0, 1, 16), (0, 120, 104, 107, 109, 102, 161, 76, 3, 91, 191, 147, 169, 182, 194, 225, 120))):
        assert tuple(int(log[c]) for c in rm.generator(code)) == logs
        assert tuple(int(log[c]) for c in host_generator(F, code)) == logs
    for g in (rm.generator(rm.CCSDS), host_generator(F, rm.CCSDS)):
        assert len(g) == 33 and g == g[::-1] and g[:6] == [1, 91, 127, 86, 16, 30]
    assert rm.scramble(*rm.CCSDS_SCR, 8).tobytes() == bytes.fromhex("ff480ec09a0d70bc")
    # through the library: a frame of zeros, scrambled on its way in, is the sequence itself
    job = rm.make_job(0, 0, 12, 1, (0x11d, 0, 1, 4), rm.CCSDS_SCR, rm.IN)
    assert F.rs_encode(np.zeros(8, np.uint8), job)[:8].tobytes() == bytes.fromhex("ff480ec09a0d70bc")
    for poly in range(0x100, 0x200):
        j = rm.make_job(0, 0, 12, 1, (poly, 0, 1, 4))
        rv = host(gr_fosphor_amd.load(), (np.zeros(12, np.uint8), rm.place([j])))[0]
        assert (rv == 0) == rm.primitive(poly), hex(poly)
    assert sum(rm.primitive(p) for p in range(0x100, 0x200)) == 16


def test_the_cases_hold_what_they_promise():
    buf, sj = CASES["seams"]
    assert {int(j["n_code"]) for j in sj} >= {63, 64, 65, 127, 128, 129, 254, 255} | {r + 1 for r in rm.SEAM_ROOTS}
    assert {int(j["n_roots"]) for j in sj} == set(rm.SEAM_ROOTS) and {int(j["depth"]) for j in sj} == set(rm.SEAM_DEPTHS)
    assert {int(o) & 7 for o in sj["offset"]} == set(range(8))
    assert max(int(j["offset"]) + int(j["depth"]) * int(j["n_code"]) for j in sj) == len(buf), "a job ends on the buffer's last byte"
    assert {(int(j["scr_width"]), int(j["flags"])) for j in sj} == {(s[0], f) for s, f in rm.TURNS}
    assert {int(j["gf_poly"]) for j in sj} == {0x11d, 0x187, 0x12b}
    planted = [c for _, counts in rm.PLANTED["seams"] for c in counts]
    assert {0, 1} <= set(planted) and max(planted) == 255
    rec = rm.image(CASES["seams"], SENTINEL, key="seams")[0]
    assert {rm.OK, rm.FAIL} == set(rec["status"]) and rec["max_errors"].max() == 16
    # over_t: a FAIL, a miscorrection, and nothing with <= t errors fails
    for name in ("over_t", "seams", "ccsds", "dvb", "full_table"):
        jobs = CASES[name][1]
        rec, out = rm.image(CASES[name], SENTINEL, key=name)
        fails = wrong = 0
        for j, r, (data, counts) in zip(jobs, rec, rm.PLANTED[name]):
            t = int(j["n_roots"]) // 2
            at = int(j["out_offset"])
            got = out[at:at + len(data)]
            for c, count in enumerate(counts):
                same = got[c::int(j["depth"])].tobytes() == data[c::int(j["depth"])].tobytes()
                if count <= t:
                    assert r["errors"][c] == count and same, (name, j, c, "a codeword with <= t errors is corrected")
                else:
                    assert r["errors"][c] == rm.FAILED or not same
                    fails += r["errors"][c] == rm.FAILED
                    wrong += r["errors"][c] != rm.FAILED
        if name == "over_t":
            assert fails >= 1 and wrong >= 1, (fails, wrong)
            assert any(r["status"] == rm.FAIL for r in rec)
            hits = [i for i, (j, r, (d, _)) in enumerate(zip(jobs, rec, rm.PLANTED[name]))
                    if r["status"] == rm.OK and out[int(j["out_offset"]):int(j["out_offset"]) + len(d)].tobytes() != d.tobytes()]
            print("over_t: miscorrected jobs", hits, "failed jobs", int((rec["status"] == rm.FAIL).sum()))
            assert hits, "a miscorrection: status OK with output that is not the data"
    cj = CASES["ccsds"][1]
    assert set(cj["depth"]) == {5} and set(cj["n_code"]) == {255} and set(cj["flags"]) == {rm.IN}
    dj = CASES["dvb"][1]
    assert set(dj["depth"]) == {1} and set(dj["n_code"]) == {204} and set(dj["gf_poly"]) == {0x11d} and set(dj["n_roots"]) == {16}
    full = CASES["full_table"][1]
    frec = rm.image(CASES["full_table"], SENTINEL, key="full_table")[0]
    assert len(full) == rm.MAX_JOBS and full["n_code"].max() < 16
    assert (frec["n_clean"] == frec["n_codewords"]).sum() >= rm.MAX_JOBS // 11 and not np.all(np.diff(full["offset"]) > 0), "shuffled"
    arec = rm.image(CASES["all_clean"], SENTINEL, key="all_clean")[0]
    assert (arec["n_clean"] == arec["n_codewords"]).all() and rm.expected_stats(arec)["k_fix"] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_model(lib, F, name):
    case = CASES[name]
    jobs = case[1]
    rv, rec, got = host(lib, case)
    assert rv == 0
    want_rec, want = rm.image(case, SENTINEL, key=name)
    got_rec = records_of(rec, len(jobs))
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical"
    for i in np.flatnonzero(got != want)[:10]:
        print("byte %d got %s want %s" % (i, got[i], want[i]))
    assert got.tobytes() == want.tobytes(), "bytes bit-identical, every other byte at the sentinel"
    records, views = F.rs_host(case[0], jobs)
    assert records.tobytes() == want_rec.tobytes(), "the Python front end gives the same records"
    for j, r, v in zip(jobs, records, views):
        at = int(j["out_offset"])
        assert len(v) == r["n_data"] and v.tobytes() == want[at:at + len(v)].tobytes()


def test_a_job_alone_among_others_and_shuffled(F):
    """a record and a job's bytes depend on their job alone"""
    buf, jobs = CASES["seams"]
    among_rec, among = F.rs_host(buf, jobs)
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = F.rs_host(buf, jobs[order])
    assert shuffled_rec.tobytes() == among_rec[order].tobytes()
    for k, i in enumerate(order):
        assert shuffled[k].tobytes() == among[i].tobytes()
    for i in (0, 1, 2, 30, len(jobs) - 1):
        alone_rec, alone = F.rs_host(buf, jobs[i:i + 1])
        assert alone_rec[0].tobytes() == among_rec[i].tobytes() and alone[0].tobytes() == among[i].tobytes(), i


# ---- correction ---------------------------------------------------------------------------------------------------------------------

def test_every_single_and_double_error_of_a_small_code(F):
    """(12, 8) over 0x11d, t = 2: all 12 single and all 66 double error positions, each with a spread of values, as the codewords of
    frames of depth 13: every one is corrected, counted, and its bits are counted"""
    code = (0x11d, 1, 1, 4)
    rng = np.random.default_rng(12)
    values = (1, 0x80, 0xff, 0x5a, 0x03)
    patterns = [((a,), (v,)) for a in range(12) for v in values]
    patterns += [((a, b), (v, w)) for a, b in itertools.combinations(range(12), 2) for v, w in ((1, 1), (0xff, 0x80), (0x5a, 0xa5), (7, 0xff))]
    depth = 13
    while len(patterns) % depth:
        patterns.append(((), ()))
    parts, jobs, datas = [], [], []
    for at in range(0, len(patterns), depth):
        j = rm.make_job(sum(len(p) for p in parts), 0, 12, depth, code, rm.CCSDS_SCR, rm.IN)
        data = rng.integers(0, 256, 8 * depth).astype(np.uint8)
        frame = rm.encode_frame(data, j[0])
        for c, (pos, val) in enumerate(patterns[at:at + depth]):
            for q, v in zip(pos, val):
                frame[q * depth + c] ^= v
        parts.append(frame)
        jobs.append(j)
        datas.append(data)
    jobs = rm.place(jobs)
    rec, views = F.rs_host(np.concatenate(parts), jobs)
    assert rec.tobytes() == rm.decode((np.concatenate(parts), jobs))[0].tobytes()
    for k, (r, v, d) in enumerate(zip(rec, views, datas)):
        mine = patterns[k * depth:(k + 1) * depth]
        assert r["status"] == rm.OK and v.tobytes() == d.tobytes(), k
        assert list(r["errors"][:depth]) == [len(p[0]) for p in mine]
        assert r["corrected_bits"] == sum(bin(x).count("1") for p in mine for x in p[1])
        assert r["corrected_symbols"] == sum(len(p[0]) for p in mine) and r["max_errors"] == max(len(p[0]) for p in mine)


@pytest.mark.parametrize("shape", ["ccsds", "dvb"])
def test_random_patterns_up_to_t_are_corrected(F, shape):
    code, n_code, depth, scr, flags = (rm.CCSDS, 255, 5, rm.CCSDS_SCR, rm.IN) if shape == "ccsds" else (rm.DVB, 204, 1, rm.DVB_SCR, rm.OUT)
    t = code[3] // 2
    rng = np.random.default_rng(40 + len(shape))
    specs = [(n_code, depth, code, scr, flags, tuple(int(v) for v in rng.integers(0, t + 1, depth)), i % 8) for i in range(24)]
    specs.append((n_code, depth, code, scr, flags, (t,), 1))
    buf, jobs = rm.build("random_" + shape, specs, 41)
    rec, views = F.rs_host(buf, jobs)
    for r, v, (data, counts) in zip(rec, views, rm.PLANTED["random_" + shape]):
        assert r["status"] == rm.OK and v.tobytes() == data.tobytes() and list(r["errors"][:depth]) == counts


@pytest.mark.parametrize("name", ["seams", "over_t", "ccsds", "dvb"])
def test_what_ok_promises(F, name):
    """whenever the status is OK the output, encoded again, has the corrected frame's parity: the corrected frame is a codeword
    that differs from the descrambled input in errors[c] <= t bytes of codeword c, exactly"""
    buf, jobs = CASES[name]
    rec, views = F.rs_host(buf, jobs)
    seen = 0
    for j, r, v in zip(jobs, rec, views):
        if r["status"] != rm.OK:
            continue
        seen += 1
        I, n = int(j["depth"]), int(j["n_code"])
        at = rm.make_job(0, 0, n, I, rm.code_of(j), rm.scr_of(j), int(j["flags"]))
        again = F.rs_encode(v, at)
        assert again.tobytes() == rm.encode_frame(v, at[0]).tobytes(), "the encoder is the model's"
        diff = again != buf[int(j["offset"]):int(j["offset"]) + I * n]
        for c in range(I):
            assert int(diff[c::I].sum()) == r["errors"][c] <= int(j["n_roots"]) // 2
    assert seen


@pytest.mark.parametrize("flags,scr", [(0, rm.NO_SCR), (rm.IN, rm.CCSDS_SCR), (rm.OUT, rm.DVB_SCR), (rm.IN, rm.WIDE_SCR), (rm.OUT, rm.WIDE_SCR), (0, rm.DVB_SCR)])
def test_round_trip(F, flags, scr):
    rng = np.random.default_rng(17)
    jobs = rm.place([rm.make_job(3, 0, 255, 5, rm.CCSDS, scr, flags), rm.make_job(3 + 1275, 0, 204, 1, rm.DVB, scr, flags),
                     rm.make_job(3 + 1275 + 204, 0, 40, 16, (0x12b, 254, 7, 31), scr, flags)])
    data = rng.integers(0, 256, rm.capacity(jobs)).astype(np.uint8)
    frames = F.rs_encode(data, jobs)
    assert len(frames) == 3 + 1275 + 204 + 640 and not frames[:3].any()
    for j in jobs:
        at = int(j["offset"])
        want = rm.encode_frame(data[int(j["out_offset"]):int(j["out_offset"]) + rm.n_data_of(j)], j)
        assert frames[at:at + len(want)].tobytes() == want.tobytes()
    if flags:
        plain = jobs.copy()
        plain["flags"] = 0
        assert F.rs_encode(data, plain).tobytes() != frames.tobytes(), "the scrambler does something"
    rec, views = F.rs_host(frames, jobs)
    assert (rec["n_clean"] == rec["n_codewords"]).all() and not rec["status"].any()
    for j, v in zip(jobs, views):
        assert v.tobytes() == data[int(j["out_offset"]):int(j["out_offset"]) + len(v)].tobytes()


# ---- the refusals -------------------------------------------------------------------------------------------------------------------

N_IN, CAP = 3000, 4096


def good_jobs():
    """three jobs over 3000 bytes and a capacity of 4096: the first fills d_out[0 .. 1120), the last ends on both buffers' last bytes"""
    return np.concatenate([rm.make_job(0, 0, 255, 5, rm.CCSDS, rm.CCSDS_SCR, rm.IN),			# 1275 in, 1115 data: 1120 owned
                           rm.make_job(7, 1120, 204, 1, rm.DVB, rm.DVB_SCR, rm.OUT),			# 188 data: 192 owned
                           rm.make_job(N_IN - 36, CAP - 24, 12, 3, (0x11d, 0, 1, 4))])			# 36 in, 24 data


def refusal_rows():
    """one job each that rule 7 refuses: (the fields to change of good_jobs()[0])"""
    big = 2 ** 62
    return [dict(offset=-1), dict(out_offset=-8), dict(offset=N_IN - 1274), dict(offset=N_IN + 1), dict(offset=big), dict(offset=2 ** 63 - 1),
            dict(out_offset=CAP - 1112), dict(out_offset=CAP + 8), dict(out_offset=big), dict(out_offset=4), dict(out_offset=1),
            dict(gf_poly=0xff), dict(gf_poly=0x200), dict(gf_poly=0), dict(gf_poly=0x11b), dict(gf_poly=0x100), dict(gf_poly=0x1ff),
            dict(fcr=255), dict(prim=0), dict(prim=255), dict(prim=3), dict(prim=5), dict(prim=17), dict(prim=51), dict(prim=85),
            dict(n_roots=0), dict(n_roots=1), dict(n_roots=33), dict(n_roots=255), dict(n_code=32), dict(n_code=0), dict(n_code=31),
            dict(depth=0), dict(depth=17), dict(depth=255), dict(scr_width=1), dict(scr_width=33), dict(scr_width=255),
            dict(scr_taps=0x100), dict(scr_init=0x100), dict(scr_taps=2 ** 32 - 1), dict(scr_width=0), dict(scr_width=0, scr_taps=0, scr_init=0),
            dict(scr_width=0, scr_taps=0, scr_init=1, flags=0), dict(scr_width=0, scr_taps=1, scr_init=0, flags=0),
            dict(flags=3), dict(flags=4), dict(flags=5), dict(flags=-1), dict(flags=1 << 31 - 1),
            dict(reserved=(1, 0, 0, 0, 0, 0, 0)), dict(reserved=(0, 0, 0, 0, 0, 0, 1 << 31)), dict(reserved=(0, 0, 0, 7, 0, 0, 0))]


def changed(job, **kw):
    j = job.copy()
    for k, v in kw.items():
        j[k] = v
    return j


def test_einval_table(lib):
    """each refused call leaves every byte and every record at the sentinel; the last jobs that fit are accepted"""
    rng = np.random.default_rng(91)
    data = rng.integers(0, 256, N_IN).astype(np.uint8)
    good = good_jobs()
    rv, rec, out = host(lib, (data, good), cap=CAP)
    want_rec, want = rm.image((data, good), SENTINEL)
    assert rv == 0 and records_of(rec, 3).tobytes() == want_rec.tobytes() and out[:CAP].tobytes() == want[:CAP].tobytes()
    assert np.all(out[1312:CAP - 24] == SENTINEL)

    def refused(jobs, **kw):
        kw.setdefault("cap", CAP)
        rv, rec, out = host(lib, (data, jobs), **kw)
        assert rv == EINVAL, (jobs, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"

    for what in ("in", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused(np.repeat(good[2:3], rm.MAX_JOBS + 1))
    refused(good, n_bytes=-1); refused(good, n_bytes=N_IN - 1); refused(good, cap=-1); refused(good, cap=CAP - 8)
    for row in refusal_rows():
        refused(changed(good[:1], **row))
    refused(np.concatenate([good[:1], changed(good[1:2], out_offset=1112)]))			# [0, 1120) and [1112, 1304)
    refused(np.concatenate([changed(good[1:2], out_offset=2000), changed(good[2:3], out_offset=1984)]))	# descending, [1984, 2008)
    for name, by in (("records", 4), ("out", 4), ("out", 1)):
        refused(good, skew=(name, by))
    # what still fits: the other scramble flag, every limit at its end, d_in without alignment, input ranges that overlap
    for row in (dict(flags=rm.OUT), dict(flags=0), dict(fcr=254), dict(prim=254), dict(prim=2), dict(n_roots=2, n_code=3), dict(n_code=33),
                dict(depth=1), dict(scr_width=32, scr_taps=2 ** 32 - 1, scr_init=2 ** 32 - 1), dict(scr_width=2, scr_taps=3, scr_init=3),
                dict(offset=N_IN - 1275), dict(out_offset=CAP - 1120)):
        assert host(lib, (data, changed(good[:1], **row)), cap=CAP)[0] == 0, row
    assert host(lib, (data[1:], changed(good[:1], offset=0)), cap=CAP)[0] == 0
    assert host(lib, (data, np.concatenate([good[:1], changed(good[1:2], offset=0)])), cap=CAP)[0] == 0
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    rec = np.full(W, SENTINEL32, np.uint32)
    out = np.full(1024, SENTINEL32, np.uint32)
    assert lib.fosphor_amd_rs(None, data.ctypes.data, N_IN, good.ctypes.data, 1, rec.ctypes.data, out.ctypes.data, 4096) == EINVAL
    assert np.all(rec == SENTINEL32) and np.all(out == SENTINEL32)
    assert lib.fosphor_amd_rs_stats(None, None) == EINVAL
    # the encoder: the same fields, its own ranges
    frames = np.full(N_IN, SENTINEL, np.uint8)
    enc = lambda jobs, n_jobs=None, cap=CAP, n=N_IN, d=data, f=frames: lib.fosphor_amd_rs_encode_host(
        None if d is None else np.resize(d, CAP + 8).ctypes.data, cap, jobs.ctypes.data, len(jobs) if n_jobs is None else n_jobs,
        None if f is None else f.ctypes.data, n)
    for row in refusal_rows():
        if "out_offset" in row and row["out_offset"] in (4, 1):
            continue						# the data needs no alignment
        assert enc(changed(good[:1], **row)) == EINVAL, row
    assert enc(good, d=None) == EINVAL and enc(good, f=None) == EINVAL and enc(good, n_jobs=0) == EINVAL and enc(good, cap=-1) == EINVAL
    assert enc(good, n=N_IN - 1) == EINVAL and enc(good, cap=CAP - 1) == EINVAL
    assert enc(np.concatenate([good[:1], changed(good[1:2], offset=1274)])) == EINVAL, "frames that overlap"
    assert np.all(frames == SENTINEL), "nothing is written"
    assert enc(good) == EINVAL and np.all(frames == SENTINEL), "the frames of good_jobs() overlap: input ranges may, frames to write may not"
    apart = np.concatenate([good[:1], changed(good[1:2], offset=1275), good[2:]])
    assert enc(apart) == 0 and not np.all(frames[:1479] == SENTINEL) and np.all(frames[1479:N_IN - 36] == SENTINEL)


def test_call_limit(lib, F):
    """MAX_JOBS frames of MAX_DEPTH codewords are exactly MAX_CALL_CODEWORDS: the host statement against the model; one job more
    is refused with every byte and record at the sentinel"""
    frame, jobs, data = rm.call_limit_case()
    assert len(jobs) == rm.MAX_JOBS and int(jobs["depth"].sum()) == rm.MAX_CALL_CODEWORDS
    rv, rec, got = host(lib, (frame, jobs))
    assert rv == 0
    one_rec, one = rm.decode((frame, jobs[:1]))
    got_rec = records_of(rec, len(jobs))
    assert (one_rec["corrected_symbols"][0], one_rec["errors"][0][5], one_rec["corrected_bits"][0], one_rec["n_clean"][0]) == (1, 1, 1, 15)
    assert one[0].tobytes() == data.tobytes()
    assert got_rec.tobytes() == np.repeat(one_rec, rm.MAX_JOBS).tobytes()
    for j in (jobs[0], jobs[1], jobs[-1]):
        assert got[int(j["out_offset"]):int(j["out_offset"]) + len(data)].tobytes() == data.tobytes()
    assert np.all(got[:rm.GUARD] == SENTINEL) and np.all(got[-rm.GUARD:] == SENTINEL)
    more = rm.place([jobs[:1]] * (rm.MAX_JOBS + 1), gap=0)
    rv, rec, out = host(lib, (frame, more))
    assert rv == EINVAL and np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"


def test_jobs_from_decode_and_derive(lib, F):
    jobs = F.rs_jobs([0, 2048, 5000], [8 * 1275, 8 * 1279 + 7, 8 * 1275 + 32], 255, depth=5, flags="descramble_in",
                     scr_width=8, scr_taps=0x95, scr_init=0xff, **F.RS_CCSDS)
    assert jobs.dtype == rm.JOB_DTYPE and list(jobs["offset"]) == [0, 2048, 5000] and list(jobs["out_offset"]) == [0, 1128, 2256]
    assert set(jobs["flags"]) == {rm.IN} and set(jobs["n_code"]) == {255} and set(jobs["depth"]) == {5} and not jobs["reserved"].any()
    assert rm.code_of(jobs[0]) == rm.CCSDS and rm.scr_of(jobs[1]) == rm.CCSDS_SCR
    assert list(F.rs_jobs([16], [8 * 1279], 255, depth=5, skip_bytes=4, gap=0)["offset"]) == [20]
    job = gr_fosphor_amd._lib.RsJob()
    job.out_offset, job.fcr = 99, 9
    make = lib.fosphor_amd_rs_from_decode
    assert make(16, 8 * 1279, 4, 255, 5, C.byref(job)) == 0
    assert (job.offset, job.out_offset, job.fcr, job.n_code, job.depth, job.flags, job.gf_poly) == (20, 0, 0, 255, 5, 0, 0)
    assert make(16, 8 * 1279 - 1, 4, 255, 5, C.byref(job)) == EINVAL, "n_bits does not cover the frame"
    assert make(16, 8 * 1279, 5, 255, 5, C.byref(job)) == EINVAL
    for bad in ((-1, 80000, 0, 255, 5), (0, -1, 0, 255, 5), (0, 80000, -1, 255, 5), (0, 80000, 0, 2, 5), (0, 80000, 0, 256, 5),
                (0, 80000, 0, 255, 0), (0, 80000, 0, 255, 17), (0, 80000, 2 ** 62, 255, 5), (2 ** 63 - 1, 2 ** 31 - 1, 1, 3, 1)):
        assert make(*bad, C.byref(job)) == EINVAL, bad
    assert make(2 ** 62, 2 ** 31 - 1, 2 ** 28 - 4081, 255, 16, C.byref(job)) == 0 and job.offset == 2 ** 62 + 2 ** 28 - 4081
    assert make(0, 80000, 0, 255, 5, None) == EINVAL
    with pytest.raises(ValueError):
        F.rs_jobs([0], [8 * 1274], 255, depth=5)
    with pytest.raises(ValueError):
        F.rs_jobs([0, 1], [8 * 1275], 255, depth=5)
    r = np.zeros(1, rm.RECORD_DTYPE)
    r["n_codewords"], r["n_failed"], r["corrected_symbols"], r["n_code"], r["status"] = 5, 1, 51, 255, rm.FAIL
    v = F.rs_derive(r)[0]
    assert set(v) == set(F.RS_VALUES) and v == dict(byte_error_rate=0.05, failed_share=0.2, ok=0.0)
    assert F.rs_derive(np.zeros(1, rm.RECORD_DTYPE))[0] == dict(byte_error_rate=0.0, failed_share=0.0, ok=1.0), "0 / 0 is 0"
    vals = gr_fosphor_amd._lib.RsValues()
    assert lib.fosphor_amd_rs_derive(None, C.byref(vals)) == EINVAL and lib.fosphor_amd_rs_derive(r.tobytes(), None) == EINVAL


# ---- function -----------------------------------------------------------------------------------------------------------------------

CHAIN_FLIPS = (5, 6, 7, 9, 11, 12, 700, 701, 703, 704, 706, 1500)


def chain_symbols():
    """a DVB-shaped RS(204,188) frame, scrambled before encoding, sent through the K = 7 (171, 133) code at rate 1/2 over QPSK with
    two bursts of channel errors that the inner decoder cannot correct -> (symbols, data, decode job)"""
    import decode_model as dm
    rng = np.random.default_rng(23)
    data = rng.integers(0, 256, 188).astype(np.uint8)
    rsj = rm.make_job(0, 0, 204, 1, rm.DVB, rm.DVB_SCR, rm.OUT)
    frame = gr_fosphor_amd.Fosphor.rs_encode(data, rsj)
    assert frame.tobytes() == rm.encode_frame(data, rsj[0]).tobytes()
    sym, T = dm.frame(np.unpackbits(frame), dm.K7, dm.P_NONE, 4, dm.CRC_NONE, True, flips=CHAIN_FLIPS)
    job = dm.place([dm.make_job(0, 0, len(sym), 4, dm.K7, dm.P_NONE, dm.CRC_NONE, T, dm.TERMINATED)])
    return sym, data, frame, job


def test_chain_on_the_host(F):
    """rs_encode -> convolutional encoder of tests/decode_model.py -> planted channel errors -> decode_host -> rs_jobs -> rs_host: the
    inner decoder leaves byte errors in its output, the outer code corrects them and counts them, and the data is the planted one"""
    sym, data, frame, job = chain_symbols()
    drec, dviews = F.decode_host(sym, job)
    assert drec["n_bits"][0] == 8 * 204
    inner = dviews[0][:204]
    wrong = int((inner != frame).sum())
    jobs = F.rs_jobs(job["out_offset"], drec["n_bits"], 204, flags="descramble_out", scr_width=15, scr_taps=0x6000, scr_init=0x4a80, **F.RS_DVB)
    out = np.zeros(int(job["out_offset"][0]) + 208, np.uint8)
    out[int(job["out_offset"][0]):][:len(dviews[0])] = dviews[0]
    rec, views = F.rs_host(out, jobs)
    print("chain: inner decoder left %d wrong bytes, metric %d; rs corrected %d symbols, %d bits" %
          (wrong, drec["metric"][0], rec["corrected_symbols"][0], rec["corrected_bits"][0]))
    assert 1 <= wrong <= 8, "decode's own output has byte errors, within t"
    assert rec["status"][0] == rm.OK and rec["corrected_symbols"][0] == wrong and rec["errors"][0][0] == wrong
    assert rec["corrected_bits"][0] == int(np.unpackbits(inner ^ frame).sum())
    assert views[0].tobytes() == data.tobytes(), "the RS output is the planted data"
    assert rec.tobytes() == rm.decode((out, jobs))[0].tobytes()
    assert F.rs_derive(rec)[0] == dict(byte_error_rate=wrong / 204, failed_share=0.0, ok=1.0)


def test_rs_kernels_meet_their_resources(F):
    """-Rpass-analysis=kernel-resource-usage: fosphor_rs.hip has exactly four kernels, each with 0 bytes of scratch, at most 64
    VGPRs (eight waves a SIMD) and the static LDS that the header states for it"""
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
    ours = {k: v for k, v in found.items() if "k_rs_" in k}
    assert len(ours) == 4 and len(found) == 4, sorted(found)
    for name, res in ours.items():
        form = re.search(r"k_rs_(syn|fix|out|rec)", name).group(1)
        print(form, res)
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 1 << 30) <= 64, (name, res)
        assert res.get("LDS Size") == F.RS_LDS[form] == header_value("FOSPHOR_AMD_RS_LDS_" + form.upper()), (name, res)
