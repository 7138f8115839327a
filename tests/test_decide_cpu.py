"""Host side of include/fosphor_amd_decide.h, no GPU: fosphor_amd_decide_host against the numpy statement (tests/decide_model.py),
records and the whole output buffer bit for bit, on every input set the GPU tests use; the refusals; the seams of rule 1; the ties
of rule 4; decide_jobs and decide_derive; that a job's bytes depend on the job alone; that the decisions are the planted indices
under every rotation, with and without a unique word, differential decoding and Gray demapping; the chain down from extract_host;
and the compiled kernels' resources.

Bit for bit means tobytes(): signed zeros and the one quiet NaN included."""
import ctypes as C
import errno
import math
import os
import re
import subprocess

import numpy as np
import pytest

import decide_model as dm
from _pkg import gr_fosphor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_decide.hip")
HEADER = os.path.join(ROOT, "include", "fosphor_amd_decide.h")
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


def host(lib, case, n_samples=None, n_jobs=None, n_uw=None, cap=None, null=(), skew=None):
    """-> (return value, records as uint32 [n_jobs + 1][24] and 2 more, the whole output buffer as uint8 [size]), both
    sentinel-filled before the call.  cap: out_capacity, GUARD bytes of the buffer lie behind it; skew: (pointer name, bytes)"""
    iq = dm.buffer(case)
    keep = iq if len(iq) else np.zeros((1, 2), np.float32)
    jobs = np.ascontiguousarray(case[1], dm.JOB_DTYPE)
    uw = np.concatenate([dm.table(case), np.zeros(1, np.uint8)])		# something to point at when the table is empty
    size = dm.capacity(jobs) if cap is None else max(cap, 0) + dm.GUARD
    buf = np.full((size + 8) // 4, SENTINEL32, np.uint32).view(np.uint8)
    rec = np.full((len(jobs) + 1) * W + 2, SENTINEL32, np.uint32)
    ptr = {"iq": keep.ctypes.data, "jobs": jobs.ctypes.data, "uw": uw.ctypes.data, "records": rec.ctypes.data, "out": buf.ctypes.data}
    for k in null:
        ptr[k] = None
    if skew:
        ptr[skew[0]] += skew[1]
    rv = lib.fosphor_amd_decide_host(ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["jobs"],
                                     len(jobs) if n_jobs is None else n_jobs, ptr["uw"], len(uw) - 1 if n_uw is None else n_uw,
                                     ptr["records"], ptr["out"], size if cap is None else cap)
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
    assert dm.JOB_DTYPE.itemsize == 64 and C.sizeof(L.DecideJob) == 64
    assert dm.RECORD_DTYPE.itemsize == 96 and C.sizeof(L.DecideRecord) == 96
    assert F.DECIDE_JOB_DTYPE == dm.JOB_DTYPE and F.DECIDE_RECORD_DTYPE == dm.RECORD_DTYPE
    for dtype, struct in ((dm.JOB_DTYPE, L.DecideJob), (dm.RECORD_DTYPE, L.DecideRecord)):
        assert [(k, dtype.fields[k][1]) for k in dtype.names] == [(k, getattr(struct, k).offset) for k, _ in struct._fields_]
    assert F.DECIDE_STATS == dm.STATS and F.DECIDE_FLAGS == dm.FLAGS and F.DECIDE_STATUS == dm.STATUS
    assert len(dm.STATS) <= 10 == header_value_of(os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_pass.h"), "FOSPHOR_COUNTERS_MAX")
    assert (F.DECIDE_MAX_JOBS, F.DECIDE_MAX_UW, F.DECIDE_MAX_UW_TABLE, F.DECIDE_BLOCK, F.DECIDE_TILE, F.DECIDE_UW_GROUP) == (
        dm.MAX_JOBS, dm.MAX_UW, dm.MAX_UW_TABLE, dm.BLOCK, dm.TILE, dm.UW_GROUP)
    for name, want in (("MAX_JOBS", dm.MAX_JOBS), ("MAX_UW", dm.MAX_UW), ("MAX_UW_TABLE", dm.MAX_UW_TABLE), ("BLOCK", dm.BLOCK),
                       ("TILE", dm.TILE), ("UW_GROUP", dm.UW_GROUP), ("DIFF", dm.DIFF), ("GRAY", dm.GRAY), ("UW", dm.UW), ("OK", dm.OK),
                       ("NO_UW", dm.NO_UW), ("LDS_HARD", F.DECIDE_LDS["hard"]), ("LDS_UW", F.DECIDE_LDS["uw"]),
                       ("LDS_JOB", F.DECIDE_LDS["job"]), ("LDS_OUT", F.DECIDE_LDS["out"])):
        assert header_value("FOSPHOR_AMD_DECIDE_" + name) == want, name
    for name in ("decide", "decide_host", "decide_jobs", "decide_derive", "decide_stats"):
        assert hasattr(F, name), name


def test_the_header_s_functions_are_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fosphor_amd_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["fosphor_amd_decide", "fosphor_amd_decide_derive", "fosphor_amd_decide_from_carrier", "fosphor_amd_decide_host",
                        "fosphor_amd_decide_stats"]
    lib = C.CDLL(gr_fosphor_amd.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
        assert name in gr_fosphor_amd._lib.SIGNATURES, name


def test_the_cases_hold_what_they_promise():
    tj = CASES["tiles"][1]
    for M in dm.ORDERS:
        assert set(dm.TILE_COUNTS) <= set(tj["n"][tj["order"] == M]), M
        assert {4097, 2 * 4096 + 5} <= set(tj["n"][(tj["order"] == M) & ((tj["flags"] & dm.DIFF) != 0)]), "DIFF across a tile seam"
    iq, oj, _ = CASES["offsets"]
    assert {int(o) & 3 for o in oj["offset"]} == {0, 1, 2, 3} and (oj["offset"] + oj["n"]).max() == len(iq)
    wj, wr = CASES["windows"][1], dm.decide(CASES["windows"])[0]
    found = wr["status"] == dm.OK
    assert np.all(wr["uw_errors"][found & (wj["uw_max_errors"] == 0)] == 0)
    assert {0, 1, 250, 255, 256, 4080, 4095, 4096, 700 - 32} <= set(wr["uw_pos"][found]) and {1, 63, 64} <= set(wj["uw_len"][found])
    assert (wr["uw_rot"][found & ((wj["flags"] & dm.DIFF) == 0)] == 1).all() and (wr["uw_rot"][(wj["flags"] & dm.DIFF) != 0] == 0).all()
    last = found & (wr["uw_pos"] == wj["n"] - wj["uw_len"])
    assert (last & (wj["uw_count"] == 0)).any() and (last & (wj["uw_count"] > 0)).any(), "the last position that fits"
    lost = wr["status"] == dm.NO_UW
    assert (lost & (wr["uw_pos"] == -1)).sum() >= 12 and np.all(wr["uw_errors"][wr["uw_pos"] == -1] == wj["uw_len"][wr["uw_pos"] == -1])
    assert (lost & (wr["uw_pos"] >= 0) & (wr["uw_errors"] == 3)).sum() == 3 and (found & (wr["uw_errors"] == 3)).sum() == 3
    nr = dm.decide(CASES["numbers"])[0]
    assert nr["erasures"].max() >= 3 and np.isnan(nr["a"]).any() and np.isinf(nr["m2"]).any() and ((nr["m2"] > 0) & (nr["m2"] < 1e-70)).any()
    zero = nr["m2"] == 0.0
    assert zero.any() and np.all(nr["erasures"][zero] == 0) and np.all(nr["hist"][zero][:, 0] == nr["n"][zero]), "all-zero symbols: k = 0"
    mj = CASES["mixed"][1]
    assert set(mj["flags"]) == set(range(8)) - {dm.UW | 8} and set(mj["order"]) == set(dm.ORDERS) and (mj["n"] < 3).any()
    assert not (CASES["without_word"][1]["flags"] & dm.UW).any()
    full = CASES["full_table"][1]
    assert len(full) == dm.MAX_JOBS and set(full["flags"]) == set(range(8)) and (full["n"] == 0).sum() >= dm.MAX_JOBS // 11
    assert full["n"].max() <= 130 and set(full["order"]) == set(dm.ORDERS)


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
    records, views = F.decide_host(dm.buffer(case), jobs, case[2])
    assert records.tobytes() == want_rec.tobytes(), "the Python front end gives the same records"
    for j, v in zip(jobs, views):
        at = int(j["out_offset"])
        assert len(v) == j["n"] and v.tobytes() == want[at:at + len(v)].tobytes()


def test_a_job_alone_among_others_and_shuffled(F):
    """a record and a job's bytes depend on their job alone"""
    iq, jobs, uw = CASES["mixed"]
    among_rec, among = F.decide_host(iq, jobs, uw)
    order = np.random.default_rng(3).permutation(len(jobs))
    shuffled_rec, shuffled = F.decide_host(iq, jobs[order], uw)
    assert shuffled_rec.tobytes() == among_rec[order].tobytes()
    for k, i in enumerate(order):
        assert shuffled[k].tobytes() == among[i].tobytes()
    for i in (0, 1, 2, 3, 4, len(jobs) - 1):
        alone_rec, alone = F.decide_host(iq, jobs[i:i + 1], uw)
        assert alone_rec[0].tobytes() == among_rec[i].tobytes() and alone[0].tobytes() == among[i].tobytes(), i


EINVAL_OK = (0, 0, 100, 4, dm.UW, 0, 32, 0, 0, 0)


def einval_rows(cap):
    """one job each that rule 7 refuses, over 3000 samples and a table of 40 symbols below 4 (the rows of
    tests/test_gpu_decide.py)"""
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


def test_einval_table(lib):
    """each refused call leaves every byte and every record at the sentinel"""
    iq = dm.psk(3000, 4, 0.0, 0.26, 91, 30.0)
    uw = np.concatenate([dm.planted(3000, 4, 91)[100:139], [2]]).astype(np.uint8)		# 40 symbols, the last one a 2
    #        offset out n order flags uw_offset uw_len uw_first uw_count uw_max_errors
    good = [(0, 8, 500, 4, dm.UW, 0, 39, 0, 0, 0), (2990, 0, 5, 2, dm.DIFF), (3000, 508, 0, 8, dm.GRAY), (1, 512, 2999, 8, dm.UW, 1, 39, 5, 0, 39)]
    cap = 512 + 3000
    rv, rec, out = host(lib, (iq, dm.make_jobs(good), uw), cap=cap)
    assert rv == 0 and np.all(out[cap:] == SENTINEL) and np.all(out[508:512] == SENTINEL) and np.all(out[0:8] != SENTINEL)
    r = records_of(rec, 4)
    assert r["uw_pos"][0] == 100 and r["uw_rot"][0] == 1 and r["uw_errors"][0] == 0

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        jobs = rows if isinstance(rows, np.ndarray) else dm.make_jobs(rows)
        rv, rec, out = host(lib, (iq, jobs, uw), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"

    for what in ("iq", "jobs", "uw", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[1]] * (dm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=2999); refused(good, cap=-1); refused(good, cap=cap - 1)
    refused(good, n_uw=-1); refused(good, n_uw=39); refused(good, n_uw=dm.MAX_UW_TABLE + 1)
    for row in einval_rows(cap):
        refused([row])
    reserved = dm.make_jobs([EINVAL_OK] * 4)
    for i in range(4):
        reserved["reserved"][i, i] = 1
        refused(reserved[i:i + 1])
    refused([EINVAL_OK, EINVAL_OK[:1] + (96,) + EINVAL_OK[2:]])				# [0, 100) and [96, 196): a word shared
    refused([EINVAL_OK[:2] + (97,) + EINVAL_OK[3:], EINVAL_OK[:1] + (96,) + EINVAL_OK[2:]])	# the padding of [0, 97) is owned
    refused([EINVAL_OK[:1] + (200,) + EINVAL_OK[2:], (0, 8, 800, 4, 0)])			# [200, 300) and [8, 808), in descending order
    for name, by in (("iq", 4), ("records", 4), ("out", 1), ("out", 2)):
        refused(good, skew=(name, by))
    # the last jobs that still fit; outputs that touch; jobs without a symbol anywhere inside; then no table at all
    last = dm.make_jobs([(0, 0, 97, 4, 0), (0, 100, 100, 2, dm.DIFF), (2900, cap - 100, 100, 4, dm.UW, 39, 1, 99, 0, 1),
                         (3000, cap, 0, 8, 0), (5, 52, 0, 8, 0)])
    rv, rec, out = host(lib, (iq, last, uw), cap=cap)
    want_rec, want = dm.image((iq, last, uw), SENTINEL)
    assert rv == 0 and records_of(rec, 5).tobytes() == want_rec.tobytes() and out[:cap].tobytes() == want[:cap].tobytes()
    rv, rec, out = host(lib, (iq, last[:2], uw), cap=cap, null=("uw",), n_uw=0)
    assert rv == 0 and records_of(rec, 2).tobytes() == want_rec[:2].tobytes()
    many = dm.make_jobs([(0, 100 * i, 100, 4, 0) for i in range(dm.MAX_JOBS)])
    assert host(lib, (iq, many, uw))[0] == 0
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    rec = np.full(W, SENTINEL32, np.uint32)
    out = np.full(256, SENTINEL32, np.uint32)
    job = dm.make_jobs([EINVAL_OK])
    assert lib.fosphor_amd_decide(None, iq.ctypes.data, 3000, job.ctypes.data, 1, uw.ctypes.data, 40, rec.ctypes.data, out.ctypes.data, 128) == EINVAL
    assert np.all(rec == SENTINEL32) and np.all(out == SENTINEL32)
    assert lib.fosphor_amd_decide_stats(None, None) == EINVAL


def test_the_seams_of_rule_1(F):
    """symbols exactly on a decision boundary, at angles (k + 0.5) / M built from exact floats, go to k + 1: (1, 1) at M = 4 is
    index 1, (0, 1) at M = 2 is index 1 and (0, -1) index 0.  (+0, +0) has the angle 0 and is no erasure; a -0 real part has the
    angle of half a turn, as it has for atan2, so (-0, +-0) is index M / 2.  Infinite parts have angles; a NaN part is an erasure
    and index 0.  The model and the host statement agree at every order; the indices at M = 4 and 2 are written out here"""
    inf, nan = np.inf, np.nan
    pts = [(1, 1), (-1, 1), (-1, -1), (1, -1), (0, 1), (0, -1), (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (1, 0), (1, -0.0),
           (-1, 0.0), (-1, -0.0), (inf, 1), (1, inf), (-inf, -inf), (inf, -inf), (-inf, 1), (1, -inf), (nan, 1), (1, nan), (nan, nan),
           (nan, inf), (2, 2), (3e38, 3e38), (1e-45, 1e-45)]
    iq = np.array(pts, np.float32)
    want = {4: [1, 2, 3, 0, 1, 3, 0, 2, 0, 2, 0, 0, 2, 2, 0, 1, 3, 0, 2, 3, 0, 0, 0, 0, 1, 1, 1],
            2: [0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]}
    for M in dm.ORDERS:
        jobs = dm.make_jobs([(0, 0, len(iq), M, 0)])
        rec, views = F.decide_host(iq, jobs)
        mrec, mouts = dm.decide((iq, jobs, np.zeros(0, np.uint8)))
        assert rec.tobytes() == mrec.tobytes() and views[0].tobytes() == mouts[0][:len(iq)].tobytes(), M
        assert rec["erasures"][0] == 4 and rec["hist"][0].sum() == len(iq) and not rec["hist"][0][M:].any()
        if M in want:
            assert list(views[0]) == want[M], (M, list(views[0]))
    # every symbol alone gives the same index: nothing depends on a neighbour
    for i in range(len(iq)):
        rec, views = F.decide_host(iq, dm.make_jobs([(i, 0, 1, 4, 0)]))
        assert views[0][0] == want[4][i] and rec["erasures"][0] == int(np.isnan(iq[i]).any())


def test_the_ties_of_rule_4(F):
    """a word that matches equally at two positions and under two rotations resolves to the smallest p, then the smallest r"""
    point = lambda k, M: (np.round(np.cos(2 * np.pi * np.asarray(k) / M)), np.round(np.sin(2 * np.pi * np.asarray(k) / M)))
    sym = lambda k: np.stack(point(k, 4), 1).astype(np.float32)
    # [0 0 0 0] is at 0 under r = 1 and at 5 under r = 0, four matches each: the smaller p wins though its r is larger
    k = [1, 1, 1, 1, 3, 0, 0, 0, 0, 2]
    rec, views = F.decide_host(sym(k), dm.make_jobs([(0, 0, len(k), 4, dm.UW, 0, 4, 0, 0, 0)]), np.zeros(4, np.uint8))
    assert (rec["uw_pos"][0], rec["uw_rot"][0], rec["uw_errors"][0], rec["status"][0]) == (0, 1, 0, dm.OK)
    assert list(views[0]) == [(v - 1) & 3 for v in k]
    # ... and from position 1 on the other one is found
    rec, _ = F.decide_host(sym(k), dm.make_jobs([(0, 0, len(k), 4, dm.UW, 0, 4, 1, 0, 0)]), np.zeros(4, np.uint8))
    assert (rec["uw_pos"][0], rec["uw_rot"][0], rec["uw_errors"][0]) == (5, 0, 0)
    # [0 1] over [1 3]: one match under r = 1 and one under r = 2, none under 0 and 3
    rec, views = F.decide_host(sym([1, 3]), dm.make_jobs([(0, 0, 2, 4, dm.UW, 0, 2, 0, 0, 1)]), np.array([0, 1], np.uint8))
    assert (rec["uw_pos"][0], rec["uw_rot"][0], rec["uw_errors"][0], rec["status"][0]) == (0, 1, 1, dm.OK)
    assert list(views[0]) == [0, 2]
    # [0 1] over [1 3 0 1 3]: [3 0] at 1 is the word under r = 3 and [0 1] at 2 the word itself: the smaller p wins, not the smaller r
    k = [1, 3, 0, 1, 3]
    rec, _ = F.decide_host(sym(k), dm.make_jobs([(0, 0, 5, 4, dm.UW, 0, 2, 0, 0, 0)]), np.array([0, 1], np.uint8))
    mrec = dm.decide((sym(k), dm.make_jobs([(0, 0, 5, 4, dm.UW, 0, 2, 0, 0, 0)]), np.array([0, 1], np.uint8)))[0]
    assert rec.tobytes() == mrec.tobytes()
    assert (rec["uw_pos"][0], rec["uw_rot"][0], rec["uw_errors"][0], rec["status"][0]) == (1, 3, 0, dm.OK)
    # [0 1] over [1 3 2 1 3]: one match at every position, under two rotations each: position 0, and of r = 1 and 2 the smaller
    k = [1, 3, 2, 1, 3]
    rec, _ = F.decide_host(sym(k), dm.make_jobs([(0, 0, 5, 4, dm.UW, 0, 2, 0, 0, 0)]), np.array([0, 1], np.uint8))
    assert (rec["uw_pos"][0], rec["uw_rot"][0], rec["uw_errors"][0], rec["status"][0]) == (0, 1, 1, dm.NO_UW)


def test_jobs_and_derive(lib, F):
    import carrier_model as cm
    cj = cm.make_jobs([(0, 7, 400, 4, 0, 16, 0.0, 0.0), (400, 1000, 40, 8, 0, 16, 0.0, 0.0), (0, 2000, 3, 2, 0, 16, 0.0, 0.0)])
    cr = np.zeros(3, cm.RECORD_DTYPE)
    cr["n"], cr["order"], cr["status"] = (400, 40, 3), (4, 8, 2), (0, 0, cm.NO_CARRIER)
    jobs = F.decide_jobs(cj, cr)
    assert jobs.dtype == dm.JOB_DTYPE and list(jobs["offset"]) == [7, 1000, 2000] and list(jobs["n"]) == [400, 40, 0]
    assert list(jobs["out_offset"]) == [0, 404, 448] and list(jobs["order"]) == [4, 8, 2] and not jobs["flags"].any()
    jobs = F.decide_jobs(cj[:2], cr[:2], ("diff", "uw"), uw_offset=3, uw_len=32, uw_first=5, uw_count=9, uw_max_errors=2, gap=7)
    assert set(jobs["flags"]) == {5} and list(jobs["out_offset"]) == [0, 408]
    assert [set(jobs[k]) for k in ("uw_offset", "uw_len", "uw_first", "uw_count", "uw_max_errors")] == [{3}, {32}, {5}, {9}, {2}]
    assert F.decide_jobs(cj[:1], cr[:1], "gray")["flags"][0] == dm.GRAY and F.decide_jobs(cj[:1], cr[:1], 3)["flags"][0] == 3
    job = gr_fosphor_amd._lib.DecideJob()
    job.out_offset = 99
    make = lib.fosphor_amd_decide_from_carrier
    assert make(cj[:1].tobytes(), cr[:1].tobytes(), dm.UW | dm.GRAY, 1, 64, 2, 3, 4, C.byref(job)) == 0
    assert (job.offset, job.out_offset, job.n, job.order, job.flags, job.uw_offset, job.uw_len, job.uw_first, job.uw_count,
            job.uw_max_errors, list(job.reserved)) == (7, 0, 400, 4, 6, 1, 64, 2, 3, 4, [0, 0, 0, 0])
    for bad_job, bad_rec, args in ((dict(out_offset=-1), {}, (0, 0, 0, 0, 0, 0)), ({}, dict(n=-1), (0, 0, 0, 0, 0, 0)),
                                   ({}, dict(order=3), (0, 0, 0, 0, 0, 0)), ({}, {}, (8, 0, 0, 0, 0, 0)), ({}, {}, (0, 0, 1, 0, 0, 0)),
                                   ({}, {}, (4, 0, 0, 0, 0, 0)), ({}, {}, (4, 0, 65, 0, 0, 0)), ({}, {}, (4, -1, 8, 0, 0, 0)),
                                   ({}, {}, (4, 0, 8, -1, 0, 0)), ({}, {}, (4, 0, 8, 0, -1, 0)), ({}, {}, (4, 0, 8, 0, 0, -1))):
        s, r = cj[:1].copy(), cr[:1].copy()
        for k, v in bad_job.items():
            s[k] = v
        for k, v in bad_rec.items():
            r[k] = v
        assert make(s.tobytes(), r.tobytes(), *args, C.byref(job)) == EINVAL, (bad_job, bad_rec, args)
    assert make(None, cr[:1].tobytes(), 0, 0, 0, 0, 0, 0, C.byref(job)) == EINVAL
    assert make(cj[:1].tobytes(), None, 0, 0, 0, 0, 0, 0, C.byref(job)) == EINVAL
    assert make(cj[:1].tobytes(), cr[:1].tobytes(), 0, 0, 0, 0, 0, 0, None) == EINVAL
    with pytest.raises(ValueError):
        F.decide_jobs(cj, cr, "soft")
    with pytest.raises(ValueError):
        F.decide_jobs(cj, cr[:2])
    # records built by hand
    r = np.zeros(1, dm.RECORD_DTYPE)
    r["n"], r["a"], r["b"], r["m2"], r["uw_errors"] = 100, 200.0, 200.0, 404.0, 8
    v = F.decide_derive(r, 32)[0]
    assert set(v) == set(F.DECIDE_VALUES)
    assert v["gain"] == 2.0 and abs(v["evm_rms"] - 0.1) < 1e-15 and abs(v["mer_db"] - 20.0) < 1e-12
    assert abs(v["phase_err_rad"] - math.pi / 4) < 1e-15 and v["uw_error_rate"] == 0.25
    assert F.decide_derive(r, 0)[0]["uw_error_rate"] == 0.0
    x = r.copy()
    x["m2"] = 399.0								# below a^2 / n: the max with 0
    assert F.decide_derive(x, 0)[0]["evm_rms"] == 0.0 and F.decide_derive(x, 0)[0]["mer_db"] == 0.0
    x = r.copy()
    x["n"] = 0
    assert all(y == 0.0 for k, y in F.decide_derive(x, 0)[0].items())
    for field in ("a", "b", "m2"):
        for bad in (0.0, -1.0, math.inf, math.nan):
            x = r.copy()
            x[field] = bad
            assert all(math.isfinite(y) for y in F.decide_derive(x, 32)[0].values()), (field, bad)
    vals = gr_fosphor_amd._lib.DecideValues()
    for bad in (-1, 65):
        assert lib.fosphor_amd_decide_derive(r.tobytes(), bad, C.byref(vals)) == EINVAL
    assert lib.fosphor_amd_decide_derive(None, 0, C.byref(vals)) == EINVAL
    assert lib.fosphor_amd_decide_derive(r.tobytes(), 0, None) == EINVAL


# ---- function ---------------------------------------------------------------------------------------------------------------------

N_SYMBOLS, WORD_AT, WORD_LEN = 2048, 100, 32


@pytest.mark.parametrize("M", dm.ORDERS)
def test_the_decisions_are_the_planted_indices(F, M):
    """noiseless psk(n = 2048, M, f0 = 0, theta0 = r / M) for every r: without a word q is the planted indices plus r; with the 32
    planted indices from position 100 on as the word, uw_pos = 100, uw_rot = r, no error and q is the planted indices; with DIFF d
    is the planted differences whatever r is, and the word of differences is found under r = 0; GRAY gives q ^ (q >> 1)"""
    for r in range(M):
        seed = 100 * M + r
        iq = dm.psk(N_SYMBOLS, M, 0.0, r / M, seed)
        idx = dm.planted(N_SYMBOLS, M, seed)
        dif = (idx[1:] - idx[:-1]) & (M - 1)
        uw = np.concatenate([idx[WORD_AT:WORD_AT + WORD_LEN], dif[WORD_AT - 1:WORD_AT - 1 + WORD_LEN]]).astype(np.uint8)
        rows = [(0, 0, N_SYMBOLS, M, flags) for flags in dm.ALL_FLAGS]
        rows += [(0, 0, N_SYMBOLS, M, flags | dm.UW, WORD_LEN if flags & dm.DIFF else 0, WORD_LEN, 0, 0, 0) for flags in dm.ALL_FLAGS]
        jobs = dm.make_jobs(rows)
        jobs["out_offset"] = 2048 * np.arange(8)
        rec, views = F.decide_host(iq, jobs, uw)
        gray = lambda q: q ^ (q >> 1)
        assert not rec["erasures"].any() and np.all(rec["status"] == dm.OK)
        assert np.array_equal(rec["hist"][0], np.bincount((idx + r) % M, minlength=8)), "the histogram is taken before any rotation"
        assert np.array_equal(views[0], (idx + r) % M) and np.array_equal(views[2], gray((idx + r) % M))
        assert np.array_equal(views[1][1:], dif) and views[1][0] == (idx[0] + r) % M and np.array_equal(views[3][1:], gray(dif))
        assert list(rec["uw_pos"][:4]) == [-1] * 4 and not rec["uw_rot"][:4].any() and not rec["uw_errors"].any()
        assert list(rec["uw_pos"][4:]) == [WORD_AT] * 4 and list(rec["uw_rot"][4:]) == [r, 0, r, 0]
        assert np.array_equal(views[4], idx) and np.array_equal(views[6], gray(idx))
        assert np.array_equal(views[5][1:], dif) and np.array_equal(views[7][1:], gray(dif))
        v = F.decide_derive(rec, 0)
        assert all(abs(x["gain"] - 1.0) < 1e-6 and x["evm_rms"] < 1e-6 and abs(x["phase_err_rad"]) < 1e-6 for x in v)


SEED_20DB = 7


def test_8psk_at_20_db(F):
    """8PSK, 4096 symbols at 20 dB SNR (seed 7): the model decides every symbol as planted (a condition on the input, checked
    first) and so does the host statement; evm_rms of decide_derive is within 10 % of 10^(-20 / 20) = 0.1: a statement about the
    estimator.  The float64 value here is 0.099641 (gain 1.000122, mer 20.031 dB, phase error 1.04e-4 rad): 0.36 % off,
    so the 10 % holds as it stands"""
    n, M = 4096, 8
    iq = dm.psk(n, M, 0.0, 0.0, SEED_20DB, 20.0)
    idx = dm.planted(n, M, SEED_20DB)
    k, erased = dm.decisions(iq, M)
    assert int((k != idx).sum()) == 0 and not erased.any(), "the input: no symbol error in the model"
    rec, views = F.decide_host(iq, dm.make_jobs([(0, 0, n, M, 0)]))
    assert int((views[0] != idx).sum()) == 0
    v = F.decide_derive(rec, 0)[0]
    print("8PSK 20 dB: evm_rms %.6f gain %.6f mer %.3f dB phase %.3g rad" % (v["evm_rms"], v["gain"], v["mer_db"], v["phase_err_rad"]))
    assert abs(v["evm_rms"] - 0.1) <= 0.01
    assert abs(v["mer_db"] - 20.0) <= 1.0 and abs(v["gain"] - 1.0) < 0.01 and abs(v["phase_err_rad"]) < 0.01


def test_chain_on_the_host(lib, F):
    """the QPSK preamble of resample_model's small sc16 stream through the host statements of extract, resample, symbols and
    carrier and, by the jobs that decide_jobs() makes, fosphor_amd_decide_host at M = 4 with DIFF and UW: the model's bytes; the
    word of the planted differential symbols 16 .. 47 is found without an error, at 16 over the preamble alone and at 191 over
    the whole burst"""
    import resample_model as rm
    import symbols_model as sm
    rng = np.random.default_rng(4321)
    rng.standard_normal(32000), rng.standard_normal(32000)
    idx = rng.integers(0, 4, rm.CHAIN_SYMBOLS)
    word = ((idx[1:] - idx[:-1]) & 3)[15:47].astype(np.uint8)
    raw, ejobs, _, lag = rm.chain_case()
    taps = F.extract_design(rm.CHAIN_DECIM, rm.CHAIN_TAPS, 0.8)
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    x = np.zeros((cap, 2), np.float32)
    assert lib.fosphor_amd_extract_host(raw.ctypes.data, len(raw), 2, ejobs.ctypes.data, len(ejobs), taps.ctypes.data, len(taps),
                                        x.ctypes.data, cap) == 0
    rtaps = F.resample_design(rm.CHAIN_UP, rm.CHAIN_DOWN, rm.CHAIN_BRANCH)
    rjobs = F.resample_jobs(ejobs, rm.CHAIN_UP, rm.CHAIN_DOWN, len(rtaps))
    y = F.resample_host(x, rjobs, rtaps)[0]
    sjobs = np.concatenate([F.symbols_jobs(rjobs, rm.CHAIN_HOLD), F.symbols_jobs(rjobs, rm.CHAIN_HOLD)])
    sjobs["offset"][1] += lag						# the preamble alone
    sjobs["n"][1] = rm.CHAIN_T
    sjobs["out_offset"][1] = sm.job_max_out(sjobs[0]) + sm.GUARD
    srec, sviews = F.symbols_host(y, sjobs)
    s = np.zeros((sm.capacity(sjobs), 2), np.float32)
    for j, v in zip(sjobs, sviews):
        s[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v.view(np.float32).reshape(-1, 2)
    cjobs = F.carrier_jobs(sjobs, srec, 4, lag=8)
    crec, cviews = F.carrier_host(s, cjobs)
    c = np.zeros((int((cjobs["out_offset"] + cjobs["n"]).max()), 2), np.float32)
    for j, v in zip(cjobs, cviews):
        c[int(j["out_offset"]):int(j["out_offset"]) + len(v)] = v.view(np.float32).reshape(-1, 2)
    jobs = F.decide_jobs(cjobs, crec, ("diff", "uw"), uw_offset=0, uw_len=32, uw_max_errors=4)
    rec, views = F.decide_host(c, jobs, word)
    want_rec, want = dm.decide((c, jobs, word))
    assert rec.tobytes() == want_rec.tobytes()
    for v, w in zip(views, want):
        assert v.tobytes() == w[:len(v)].tobytes()
    val = F.decide_derive(rec, 32)
    print("chain: n %s uw_pos %s uw_errors %s evm %.4f mer %.1f dB" % (rec["n"], rec["uw_pos"], rec["uw_errors"], val[1]["evm_rms"],
                                                                       val[1]["mer_db"]))
    assert list(rec["status"]) == [dm.OK, dm.OK] and list(rec["uw_errors"]) == [0, 0] and list(rec["uw_pos"]) == [191, 16]
    assert views[1][16:48].tobytes() == word.tobytes() and val[1]["uw_error_rate"] == 0.0 and val[1]["mer_db"] > 20.0


def test_decide_kernels_meet_their_resources(F):
    """-Rpass-analysis=kernel-resource-usage: every kernel of fosphor_decide.hip has 0 bytes of scratch, at most 64 VGPRs and the
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
    ours = {k: v for k, v in found.items() if "k_dec_" in k}
    assert len(ours) == 4 and len(found) == 4, sorted(found)
    for name, res in ours.items():
        form = re.search(r"k_dec_(hard|uw|job|out)", name).group(1)
        print(form, res)
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 1 << 30) <= 64, (name, res)
        assert res.get("LDS Size") == F.DECIDE_LDS[form] == header_value("FOSPHOR_AMD_DECIDE_LDS_" + form.upper()), (name, res)
