"""Host side of include/fosphor_amd_soft.h, no GPU: fosphor_amd_soft_host against the numpy statement (tests/soft_model.py), records
and the whole output buffer bit for bit, on every input set the GPU tests use and over every constraint length, stream count,
order, labeling, rotation and puncture pattern; maximum likelihood by brute force over all inputs of short frames; a frame that the
soft decoder reads and the hard chain decide -> decode cannot; saturated soft values against the hard decoder; the coding gain
over noise; the numerical edges of rule S2; a call of exactly MAX_CALL_STEPS and one step more; the refusals, each beside the
nearest call that is accepted; soft_jobs and soft_derive; the chain carrier -> decide -> soft on the host; and the compiled kernels' resources."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import decode_model as dm
import soft_model as sm
from _pkg import gr_fosphor_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_soft.hip")
HEADER = os.path.join(ROOT, "include", "fosphor_amd_soft.h")
EINVAL = -errno.EINVAL
CASES = sm.cases()
SENTINEL = 0x5a
SENTINEL32 = 0x5a5a5a5a
W = sm.RECORD_WORDS


@pytest.fixture(scope="module")
def lib():
    return gr_fosphor_amd.load()


@pytest.fixture(scope="module")
def F():
    gr_fosphor_amd.load()
    return gr_fosphor_amd.Fosphor


def host(lib, case, n_samples=None, n_jobs=None, cap=None, null=(), skew=None):
    """-> (return value, records as uint32 [(n_jobs + 1) * 16 + 2], the whole output buffer as uint8 [size]), both sentinel-filled
    before the call.  cap: out_capacity, GUARD bytes of the buffer lie behind it; skew: (pointer name, bytes)"""
    iq = np.ascontiguousarray(case[0], np.float32).reshape(-1, 2)
    keep = iq if len(iq) else np.zeros((1, 2), np.float32)
    jobs = np.ascontiguousarray(case[1], sm.JOB_DTYPE)
    size = sm.capacity(jobs) if cap is None else max(cap, 0) + sm.GUARD
    buf = np.full((size + 16) // 8, 0x5a5a5a5a5a5a5a5a, np.uint64).view(np.uint8)
    rec = np.full((len(jobs) + 1) * W + 2, SENTINEL32, np.uint32)
    ptr = {"iq": keep.ctypes.data, "jobs": jobs.ctypes.data, "records": rec.ctypes.data, "out": buf.ctypes.data}
    for k in null:
        ptr[k] = None
    if skew:
        ptr[skew[0]] += skew[1]
    rv = lib.fosphor_amd_soft_host(ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["jobs"],
                                   len(jobs) if n_jobs is None else n_jobs, ptr["records"], ptr["out"], size if cap is None else cap)
    assert np.all(buf[size:] == SENTINEL)
    return rv, rec, buf[:size]


def records_of(rec, n_jobs):
    assert np.all(rec[W * n_jobs:] == SENTINEL32), "a record beyond the jobs' was written"
    return rec[:W * n_jobs].view(sm.RECORD_DTYPE)


def header_value_of(path, name):
    m = re.search(r"#define\s+%s\s+(\w+)" % name, open(path).read())
    assert m, name
    v = m.group(1)
    return int(v) if v.isdigit() else header_value_of(os.path.join(ROOT, "include", "fosphor_amd_decode.h"), v)


def header_value(name):
    return header_value_of(HEADER, name)


def agree(lib, F, case, key=None):
    """host and model bit for bit -> the records"""
    jobs = case[1]
    rv, rec, got = host(lib, case)
    assert rv == 0
    want_rec, want = sm.image(case, SENTINEL, key=key)
    got_rec = records_of(rec, len(jobs))
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical"
    for i in np.flatnonzero(got != want)[:10]:
        print("byte %d got %s want %s" % (i, got[i], want[i]))
    assert got.tobytes() == want.tobytes(), "bytes bit-identical, every other byte at the sentinel"
    records, views = F.soft_host(case[0], jobs)
    assert records.tobytes() == want_rec.tobytes(), "the Python front end gives the same records"
    for j, r, v in zip(jobs, records, views):
        at = int(j["out_offset"])
        assert len(v) == (r["n_bits"] + 7) // 8 and v.tobytes() == want[at:at + len(v)].tobytes()
    return got_rec


def test_the_dtypes_mirror_the_structs(F):
    L = gr_fosphor_amd._lib
    assert sm.JOB_DTYPE.itemsize == 64 and C.sizeof(L.SoftJob) == 64
    assert sm.RECORD_DTYPE.itemsize == 64 and C.sizeof(L.SoftRecord) == 64
    assert F.SOFT_JOB_DTYPE == sm.JOB_DTYPE and F.SOFT_RECORD_DTYPE == sm.RECORD_DTYPE
    for dtype, struct in ((sm.JOB_DTYPE, L.SoftJob), (sm.RECORD_DTYPE, L.SoftRecord)):
        assert [(k, dtype.fields[k][1]) for k in dtype.names] == [(k, getattr(struct, k).offset) for k, _ in struct._fields_]
    # the record is the decode record with its reserved words in use; the job has every field of the decode job but reserved
    assert sm.RECORD_DTYPE.names[:12] == dm.RECORD_DTYPE.names[:12]
    assert [sm.RECORD_DTYPE.fields[k][1] for k in sm.RECORD_DTYPE.names[:12]] == [dm.RECORD_DTYPE.fields[k][1] for k in dm.RECORD_DTYPE.names[:12]]
    assert set(dm.JOB_DTYPE.names) - set(sm.JOB_DTYPE.names) == {"reserved"} and set(sm.JOB_DTYPE.names) - set(dm.JOB_DTYPE.names) == {"rot", "scale"}
    assert F.SOFT_STATS == sm.STATS and F.SOFT_FLAGS == sm.FLAGS and F.SOFT_STATUS == sm.STATUS
    assert len(sm.STATS) <= 10 == header_value_of(os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_pass.h"), "FOSPHOR_COUNTERS_MAX")
    assert L.SIGNATURES["fosphor_amd_soft_stats"][1][1]._type_._length_ == len(sm.STATS)
    assert (F.SOFT_MAX_JOBS, F.SOFT_MAX_STEPS, F.SOFT_MAX_CALL_STEPS, F.SOFT_BLOCK, F.SOFT_GROUP, F.SOFT_MAX_VALUE, F.SOFT_INF) == (
        sm.MAX_JOBS, sm.MAX_STEPS, sm.MAX_CALL_STEPS, sm.BLOCK, sm.GROUP, sm.MAX_VALUE, sm.INF)
    assert (sm.MAX_JOBS, sm.MAX_STEPS, sm.MAX_CALL_STEPS) == (dm.MAX_JOBS, dm.MAX_STEPS, dm.MAX_CALL_STEPS), "the decode pass's limits"
    assert sm.INF == 1 << 25 and sm.INF + 3 * sm.MAX_VALUE * sm.MAX_STEPS < 1 << 26
    assert ((sm.INF + 3 * sm.MAX_VALUE * sm.MAX_STEPS) << 6 | 63) < 0xffffffff, "the worst key lies below an idle lane's"
    for name, want in (("MAX_JOBS", sm.MAX_JOBS), ("MAX_STEPS", sm.MAX_STEPS), ("MAX_CALL_STEPS", sm.MAX_CALL_STEPS), ("BLOCK", sm.BLOCK),
                       ("GROUP", sm.GROUP), ("MAX_VALUE", sm.MAX_VALUE), ("INF", sm.INF), ("TERMINATED", sm.TERMINATED), ("GRAY", sm.GRAY),
                       ("OK", sm.OK), ("CRC_FAIL", sm.CRC_FAIL), ("SHORT", sm.SHORT), ("LDS_BITS", F.SOFT_LDS["bits"]),
                       ("LDS_ACS", F.SOFT_LDS["acs"]), ("LDS_TRACE", F.SOFT_LDS["trace"]), ("LDS_REC", F.SOFT_LDS["rec"])):
        assert header_value("FOSPHOR_AMD_SOFT_" + name) == want, name
    import decide_model as dec
    assert sm.GRAY == dec.GRAY, "GRAY is copied from the decide job bit for bit"
    for name in ("soft", "soft_host", "soft_jobs", "soft_derive", "soft_stats"):
        assert hasattr(F, name), name


def test_the_header_s_functions_are_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fosphor_amd_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["fosphor_amd_soft", "fosphor_amd_soft_derive", "fosphor_amd_soft_from_decide", "fosphor_amd_soft_host",
                        "fosphor_amd_soft_stats"]
    lib = C.CDLL(gr_fosphor_amd.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
        assert name in gr_fosphor_amd._lib.SIGNATURES, name


def test_the_cases_hold_what_they_promise():
    iq, sj = CASES["seams"]
    steps = [sm.shape(j)[0] for j in sj]
    assert set(sm.SEAM_STEPS) | {0} <= set(steps) and (sj["n"] == 0).any() and ((sj["n"] > 0) & (np.array(steps) == 0)).any()
    assert {int(o) & 1 for o in sj["offset"]} == {0, 1} and set(sj["order"]) == set(sm.ORDERS) and set(sj["n_poly"]) == {2, 3}
    assert set(sj["flags"]) == {0, 1, 2, 3} and set(sj["crc_width"]) == {0, 8, 16, 24, 32} and (sj["rot"] > 0).any()
    assert {1, 2, 3, 7, 16} <= set(sj["period"]) and {3, 4, 5, 6, 7} <= set(sj["k"])
    rec = sm.image(CASES["seams"], SENTINEL, key="seams")[0]
    assert {sm.OK, sm.CRC_FAIL, sm.SHORT} == set(rec["status"]) and (rec["saturated"] > 0).any() and (rec["metric"] > 0).any()
    nj = CASES["nan"][1]
    nrec = sm.image(CASES["nan"], SENTINEL, key="nan")[0]
    assert (nrec["erasures"][:6] == 12).all(), "four of the thirteen odd symbols have a NaN part, planted three times"
    assert nrec["erasures"][6] == 40 == nj["n"][6] and nrec["abs_sum"][6] == 0
    mj = CASES["max_steps"][1]
    assert sm.shape(mj[0])[0] == sm.MAX_STEPS
    full = CASES["full_table"][1]
    assert len(full) == sm.MAX_JOBS and full["n"].max() <= 40 and (full["n"] == 0).sum() >= sm.MAX_JOBS // 11
    # edges: a job a crafted value, then the 36 jobs over the odd symbols; the record carries the expected v out
    rows, ej = sm.edge_rows(), CASES["edges"][1]
    erec = sm.image(CASES["edges"], SENTINEL, key="edges")[0]
    assert len(ej) == len(rows) + 36 and len(sm.EDGE_VALUES) == 23 and (ej["n"][len(rows):] == 600).all()
    assert {(int(j["order"]), int(j["flags"]), int(j["rot"])) for j in ej[:len(rows)] if j["order"] > 2} == {
        (M, g, r) for M in (4, 8) for g in (0, sm.GRAY) for r in (0, M - 1)}
    for (sr, si, order, rot, gray, scale, want, erasures), r in zip(rows, erec):
        assert (r["n_steps"], r["n_coded"], r["erasures"]) == (1, dm.bits_of(order) if order > 2 else 2, erasures), (sr, si, r)
        if want is not None:
            assert (r["abs_sum"], r["saturated"]) == (abs(want), int(abs(want) == 127)), (sr, scale, r)
    for sr, scale, want in sm.EDGE_SUBNORMAL:
        tiny = np.finfo(np.float32).tiny
        assert want != 0 and (0 < np.float32(sr) < tiny or 0 < np.float32(scale) < tiny), "a float32 subnormal decides a value that is not 0"
    assert (erec["saturated"] > 0).any() and (erec["erasures"] > 0).any() and (erec["saturated"][len(rows):] > 0).all()
    # contract: every job tells rule S2 from a correlation contracted either way, from the model alone
    cj = CASES["contract"][1]
    plain, fma_re, fma_im = sm.contract_records()
    assert 64 <= len(cj) <= sm.CONTRACT_MAX_JOBS and len(plain) == len(cj) and set(cj["order"]) == {8} and (cj["n"] == 1).all()
    ciq = CASES["contract"][0]
    for j in cj:
        y, how = ciq[int(j["offset"]):int(j["offset"]) + 1], (8, j["rot"], int(j["flags"]) & sm.GRAY, j["scale"])
        assert sm.contracted_values(y[0], *how, sm.S2) == list(sm.soft_values(y, *how)[0][0]), "the rational arithmetic gives numpy's values"
    for i in range(len(cj)):
        assert plain[i].tobytes() != fma_re[i].tobytes() and plain[i].tobytes() != fma_im[i].tobytes(), (i, cj[i])
    sectors = {int(np.floor(np.arctan2(ciq[int(j["offset"]), 1], ciq[int(j["offset"]), 0]) / (np.pi / 4))) for j in cj}
    print("contract: %d jobs, %d of the 8 boundaries, labelings %s, rotations %s" % (len(cj), len(sectors), sorted(set(cj["flags"])), sorted(set(cj["rot"]))))
    assert len(sectors) > 1 and set(cj["flags"]) == {0, sm.GRAY} and len(set(cj["rot"])) > 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_model(lib, F, name):
    rec = agree(lib, F, CASES[name], key=name)
    if name == "max_steps":
        assert (rec["n_steps"][0], rec["status"][0], rec["end_state"][0]) == (sm.MAX_STEPS, sm.OK, 0) and rec["metric"][0] > 0


GRID_STEPS = 45


def grid_case(n_poly):
    """K = 3 .. 7 at n_poly streams, M = 2, 4 and 8, both labelings, every rotation, the four puncture patterns (the one of period 3
    lets an 8PSK symbol straddle two steps), with and without TERMINATED: noisy frames of 45 steps"""
    rng = np.random.default_rng(77 + n_poly)
    parts, jobs, at = [], [], 0
    for k in (3, 4, 5, 6, 7):
        code = (sm.CODES2 if n_poly == 2 else sm.CODES3)[k]
        for punct in (sm.PUNCT2 if n_poly == 2 else sm.PUNCT3):
            for order in sm.ORDERS:
                for gray in (0, 1):
                    for rot in range(order):
                        for term in (0, 1):
                            bits = rng.integers(0, 2, GRID_STEPS)
                            if term:
                                bits[GRID_STEPS - (k - 1):] = 0
                            coded = dm.puncture(dm.encode(bits, k, code[1], n_poly), n_poly, punct[0], punct[1])
                            sym = dm.to_symbols(coded, order)
                            z = sm.modulate(sym, order, rot, gray, 1.0) + sm.noise(rng, len(sym), 0.45)
                            parts.append(sm.pairs(z))
                            jobs.append(sm.make_job(at, 0, len(sym), order, code, punct, dm.CRC8, GRID_STEPS, term | (sm.GRAY if gray else 0), rot,
                                                    40.0))
                            at += len(sym)
    return np.concatenate(parts), sm.place(jobs)


@pytest.mark.parametrize("n_poly", [2, 3])
def test_model_agreement_over_codes_orders_labelings_rotations_and_patterns(lib, F, n_poly):
    case = grid_case(n_poly)
    jobs = case[1]
    assert len(jobs) == 5 * 4 * (2 + 4 + 8) * 2 * 2 and set(jobs["k"]) == {3, 4, 5, 6, 7} and set(jobs["period"]) == {1, 2, 3, 7}
    rec = agree(lib, F, case)
    # the frames are noisy, not hopeless: most paths end where the encoder did, and soft values of every size occur
    assert (rec["metric"] > 0).mean() > 0.9 and (rec["saturated"] > 0).any() and (rec["saturated"] < rec["n_coded"]).all()


# ---- maximum likelihood -----------------------------------------------------------------------------------------------------------

def all_inputs(n):
    return ((np.arange(1 << n)[:, None] >> (n - 1 - np.arange(n))) & 1).astype(np.int64)


def encode_all(msgs, k, polys, n_poly):
    """decode_model.encode over many inputs at once: [N][T] -> [N][T][n_poly]"""
    N, T = msgs.shape
    u = np.concatenate([np.zeros((N, k - 1), np.int64), msgs], 1)
    out = np.zeros((N, T, n_poly), np.int64)
    for i in range(n_poly):
        for j in range(k):
            if (int(polys[i]) >> j) & 1:
                out[:, :, i] ^= u[:, j:j + T]
    return out


@pytest.mark.parametrize("scale", [24.0, 1.5], ids=["fine", "coarse"])
def test_maximum_likelihood_by_brute_force(F, scale):
    """not self-consistency: K = 3, T <= 12.  metric is the least cost of rule S3 over ALL 2^n_bits inputs, found by encoding every
    one and pricing it against the model's soft values; where one input alone has that cost, it is what comes out; where several
    have it (the coarse scale leaves |v| <= 2 and many ties), the decoded input is one of them and the one the numpy statement of
    rule 3 picks: ties go to x = 0"""
    k, polys = dm.K3
    rng = np.random.default_rng(int(scale * 10))
    parts, jobs, at = [], [], 0
    for T in (1, 2, 3, 5, 8, 11, 12):
        for punct in (dm.P_NONE, dm.P_34):
            for order, gray in ((2, 0), (4, 1), (8, 1), (8, 0)):
                for term in (0, 1):
                    n = dm.symbols_for(T, order, punct)
                    z = sm.modulate(rng.integers(0, order, n), order, 1, gray) + sm.noise(rng, n, 0.6)
                    parts.append(sm.pairs(z))
                    jobs.append(sm.make_job(at, 0, n, order, dm.K3, punct, dm.CRC_NONE, T, term | (sm.GRAY if gray else 0), 1, scale))
                    at += n
    iq, jobs = np.concatenate(parts), sm.place(jobs)
    rec, views = F.soft_host(iq, jobs)
    mrec, mouts = sm.decode((iq, jobs))
    assert rec.tobytes() == mrec.tobytes()
    unique = several = 0
    for j, r, v in zip(jobs, rec, views):
        T, n_bits, n_coded = sm.shape(j)
        values, sent, _ = sm.step_values(iq, j, T)				# [T][3], 0 where not sent
        msgs = np.concatenate([all_inputs(n_bits), np.zeros((1 << n_bits, T - n_bits), np.int64)], 1)
        e = np.zeros((len(msgs), T, 3), np.int64)
        e[:, :, :2] = encode_all(msgs, k, polys, 2)
        cost = np.where(e == 1, np.maximum(values, 0)[None], np.maximum(-values, 0)[None]).sum((1, 2))
        least = int(cost.min())
        assert r["metric"] == least, (j, r, least)
        best = np.flatnonzero(cost == least)
        got = list(dm.unpack(v, n_bits))
        assert any(list(msgs[b][:n_bits]) == got for b in best), "the decoded input is a minimiser"
        if len(best) == 1:
            unique += 1
        else:
            several += 1
    print("brute force at scale %g: %d jobs with one minimiser, %d with several" % (scale, unique, several))
    assert unique > 0 and (several > 10 if scale < 2 else True)


def test_ties_go_to_x_0(F):
    """rule 3 with the costs of rule S3, by hand.  K = 3 (7, 5), BPSK, two symbols a step.  All symbols (0, 0): every v is 0, every
    comparison a tie, x = 0 wins throughout, the survivors lead back to state 0: zeros come out and best_state is 0.  One step with
    v = (+8, -8): input 0 sends 00 and pays 8 for stream 1, input 1 sends 11 and pays 8 for stream 0: states 0 and 2 tie at 8 and
    the smaller is best_state"""
    z = np.zeros((10, 2), np.float32)
    rec, views = F.soft_host(z, sm.make_job(0, 0, 10, 2, dm.K3, dm.P_NONE, dm.CRC_NONE, 5, 0, 0, 32.0))
    assert (rec["metric"][0], rec["best_state"][0], rec["abs_sum"][0], rec["erasures"][0]) == (0, 0, 0, 0) and list(dm.unpack(views[0], 5)) == [0] * 5
    iq = np.array([[0.25, 0.0], [-0.25, 0.0]], np.float32)
    rec, views = F.soft_host(iq, sm.make_job(0, 0, 2, 2, dm.K3, dm.P_NONE, dm.CRC_NONE, 1, 0, 0, 16.0))		# L = +-0.5, v = +-8
    assert (rec["abs_sum"][0], rec["best_state"][0], rec["best_metric"][0], rec["end_state"][0], rec["metric"][0]) == (16, 0, 8, 0, 8)
    assert list(dm.unpack(views[0], 1)) == [0]


# ---- soft against hard ----------------------------------------------------------------------------------------------------------

def hard_chain(F, iq, order, gray, code, punct, crc, steps, term, n_frames, per):
    """decide_host -> decode_host over n_frames frames of `per` symbols each that lie back to back -> the decode records and views"""
    import decide_model as dec
    djobs = dec.make_jobs([(per * i, dec.owned(per) * i, per, order, dec.GRAY if gray else 0) for i in range(n_frames)])
    drec, dviews = F.decide_host(iq, djobs)
    sym = np.zeros(dec.owned(per) * n_frames, np.uint8)
    for j, v in zip(djobs, dviews):
        sym[int(j["out_offset"]):int(j["out_offset"]) + per] = v
    jobs = dm.place([dm.make_job(dec.owned(per) * i, 0, per, order, code, punct, crc, steps, dm.TERMINATED if term else 0) for i in range(n_frames)])
    return F.decode_host(sym, jobs)


def soft_frames(F, iq, order, gray, code, punct, crc, steps, term, n_frames, per, scale):
    jobs = sm.place([sm.make_job(per * i, 0, per, order, code, punct, crc, steps, (sm.TERMINATED if term else 0) | (sm.GRAY if gray else 0), 0, scale)
                     for i in range(n_frames)])
    return F.soft_host(iq, jobs)


def test_soft_reads_a_frame_that_the_hard_chain_cannot(F):
    """deterministic.  K = 7 (171, 133), BPSK, terminated, CRC-16, 60 info bits.  The encoder's answer to a single 1 at input 20 has
    weight 10.  Six of those ten coded bits are sent at amplitude 0.1 with the wrong sign, everything else at amplitude 1.  The
    received hard word lies 6 from what was sent and 4 from the neighbour (the same input with bit 20 inverted), so the hard chain
    decodes the neighbour and its CRC fails.  To the soft decoder the six are worth |v| = 6 each and the neighbour's four 64 each:
    it pays 36, decodes what was sent and the CRC holds"""
    rng = np.random.default_rng(10)
    info = rng.integers(0, 2, 60)
    bits = np.concatenate([dm.with_crc(info, dm.CRC16), np.zeros(6, np.uint8)])
    T = len(bits)
    coded = dm.encode(bits, 7, dm.K7[1], 2).reshape(-1)
    other = bits.copy()
    other[20] ^= 1
    differ = np.flatnonzero(coded != dm.encode(other, 7, dm.K7[1], 2).reshape(-1))
    assert len(differ) == 10, "the free distance of (171, 133)"
    weak = differ[[0, 2, 3, 5, 7, 9]]
    x = 1.0 - 2.0 * coded							# bit 0 at +1
    x[weak] *= -0.1
    iq = sm.pairs(x.astype(np.complex128))
    hrec, hviews = hard_chain(F, iq, 2, 0, dm.K7, dm.P_NONE, dm.CRC16, 0, True, 1, len(iq))
    assert (hrec["status"][0], hrec["metric"][0], hrec["n_steps"][0]) == (dm.CRC_FAIL, 4, T), "the hard chain decodes the neighbour"
    assert list(dm.unpack(hviews[0], T - 6)) == list(other[:T - 6])
    rec, views = soft_frames(F, iq, 2, 0, dm.K7, dm.P_NONE, dm.CRC16, 0, True, 1, len(iq), 32.0)
    small = np.abs(sm.soft_values(iq[weak], 2, 0, 0, 32.0)[0]).reshape(-1)
    assert list(small) == [6] * 6
    assert (rec["status"][0], rec["metric"][0], rec["end_state"][0], rec["n_bits"][0]) == (sm.OK, int(small.sum()), 0, T - 6)
    assert list(dm.unpack(views[0], 60)) == list(info), "the planted bits"
    assert rec["abs_sum"][0] == 64 * (2 * T - 6) + 6 * 6 and rec["saturated"][0] == 0 and rec["crc_calc"][0] == rec["crc_recv"][0]


@pytest.mark.parametrize("order", sm.ORDERS)
@pytest.mark.parametrize("gray", [0, 1])
def test_saturated_values_meet_the_hard_decoder(F, order, gray):
    """clean symbols away from the decision boundaries, one in eight replaced by another point, behind a unique word under which
    decide finds a rotation that is not 0; scale = 1e6, so every sent |v| is 127.  The costs are then 127 times the hard decoder's,
    comparison for comparison: the bits are those of fosphor_amd_decode_host over decide's bytes, metric is 127 times its metric
    and saturated is n_coded"""
    import decide_model as dec
    rng = np.random.default_rng(100 + 2 * order + gray)
    rot = order - 1
    word = rng.integers(0, order, 24).astype(np.uint8)
    code, punct = ((dm.K7, dm.P_34), (dm.K5, dm.P_23), (dm.K7_THIRD, dm.P3_NONE))[order % 3]
    info = rng.integers(0, 2, 120)
    sym, T = dm.frame(info, code, punct, order, dm.CRC16, True)
    hit = rng.choice(len(sym), len(sym) // 8, replace=False)
    sent = sym.copy()
    sent[hit] = (sent[hit] + rng.integers(1, order, len(hit))) & (order - 1)
    z = np.concatenate([np.exp(2j * np.pi * ((word.astype(np.int64) + rot) & (order - 1)) / order), sm.modulate(sent, order, rot, gray)])
    z = z * np.exp(2j * np.pi * rng.uniform(-0.2, 0.2, len(z)) / order) * rng.uniform(0.5, 1.5, len(z))	# within 0.2 of a sector
    iq = sm.pairs(z)
    djobs = dec.make_jobs([(0, 0, len(iq), order, dec.UW | (dec.GRAY if gray else 0), 0, len(word), 0, 1, 0)])
    drec, dviews = F.decide_host(iq, djobs, word)
    assert (drec["status"][0], drec["uw_pos"][0], drec["uw_rot"][0], drec["uw_errors"][0]) == (dec.OK, 0, rot, 0) and rot != 0
    shared = dict(k=code[0], polys=code[1], period=punct[0], punct=punct[1], steps=T, flags="terminated", crc_width=16, crc_poly=0x1021, crc_init=0xffff)
    bytes_ = np.zeros(dec.owned(len(iq)), np.uint8)
    bytes_[:len(iq)] = dviews[0]
    hrec, hviews = F.decode_host(bytes_, F.decode_jobs(djobs, drec, len(word), **shared))
    jobs = F.soft_jobs(djobs, drec, len(word), **shared)
    assert (jobs["rot"][0], jobs["offset"][0], jobs["n"][0], jobs["flags"][0]) == (rot, len(word), len(sym), sm.TERMINATED | (sm.GRAY if gray else 0))
    jobs["scale"] = 1e6
    rec, views = F.soft_host(iq, jobs)
    assert rec.tobytes() == sm.decode((iq, jobs))[0].tobytes()
    assert hrec["metric"][0] > 0, "there is something to correct"
    assert views[0].tobytes() == hviews[0].tobytes() and rec["n_bits"][0] == hrec["n_bits"][0]
    assert rec["metric"][0] == 127 * hrec["metric"][0] and rec["best_metric"][0] == 127 * hrec["best_metric"][0]
    assert rec["saturated"][0] == rec["n_coded"][0] == hrec["n_coded"][0] and rec["abs_sum"][0] == 127 * rec["n_coded"][0]
    assert (rec["status"][0], rec["crc_calc"][0], rec["crc_recv"][0]) == (hrec["status"][0], hrec["crc_calc"][0], hrec["crc_recv"][0])


GAIN_SEED, GAIN_FRAMES, GAIN_INFO = 2024, 300, 180
GAIN_SIGMAS = (0.44, 0.52, 0.61)		# noise a part at Es = 1: Es / N0 of 4.12, 2.67 and 1.28 dB; from the sweep in profiles/r24_soft.md


def gain_frames(sigma, seed=GAIN_SEED, n_frames=GAIN_FRAMES):
    """n_frames QPSK frames, Gray, K = 7 at rate 1/2, CRC-16, terminated: 180 info bits, 202 steps, 202 symbols each"""
    rng = np.random.default_rng([seed, int(round(sigma * 1000))])
    parts = []
    for i in range(n_frames):
        iq, T, info = sm.noisy_frame(rng, GAIN_INFO, dm.K7, dm.P_NONE, 4, dm.CRC16, True, 0, True, sigma)
        parts.append(iq)
    return np.concatenate(parts), T


def test_coding_gain_over_noise(F):
    """fixed seeds; at each of three noise levels 300 frames of 202 steps through the hard chain decide_host -> decode_host and
    through fosphor_amd_soft_host at the scale that soft_from_decide would give a unit-length symbol (16): at every level the soft
    decoder fails no more CRCs than the hard chain, in total strictly fewer.  No dB figure is fixed here; the sweep from which the
    levels were chosen is in profiles/r24_soft.md"""
    total_soft = total_hard = 0
    for sigma in GAIN_SIGMAS:
        iq, T = gain_frames(sigma)
        hrec, _ = hard_chain(F, iq, 4, 1, dm.K7, dm.P_NONE, dm.CRC16, 0, True, GAIN_FRAMES, T)
        rec, _ = soft_frames(F, iq, 4, 1, dm.K7, dm.P_NONE, dm.CRC16, 0, True, GAIN_FRAMES, T, 16.0)
        hard, soft = int((hrec["status"] != dm.OK).sum()), int((rec["status"] != sm.OK).sum())
        print("sigma %.2f: CRC failures of %d frames: hard %d, soft %d" % (sigma, GAIN_FRAMES, hard, soft))
        assert soft <= hard, sigma
        total_soft += soft
        total_hard += hard
    assert total_soft < total_hard


# ---- the numerical edges of rule S2 -----------------------------------------------------------------------------------------------

def one_value(F, sr, si, scale, order=2, rot=0, gray=0):
    """v of bit 0 of one symbol, read back through a record (sm.value_job()): K = 3 (7, 5), one step, BPSK: the second symbol is
    (0, 0) and worth nothing; abs_sum is |v| and the decoded bit is 1 exactly when v < 0 (input 1 sends 11).  -> (v, the record)"""
    n, job = sm.value_job(0, order, rot, gray, scale)
    iq = np.array([[sr, si], [0.0, 0.0]][:n], np.float32)
    rec, views = F.soft_host(iq, job)
    assert rec.tobytes() == sm.decode((iq, job))[0].tobytes(), (sr, si, scale)
    mag = int(rec["abs_sum"][0])
    return (-mag if dm.unpack(views[0], 1)[0] else mag), rec[0]


def test_numerical_edges(F):
    """the rows of sm.edges_case(), each with the v it expects, against the host and the model.  BPSK at rot 0: the points are
    (1, +0) and (-1, -0), L = 2 sr exactly, x = 2 sr scale + 0.5"""
    assert len(sm.EDGE_VALUES) == 23
    for sr, scale, want in sm.EDGE_VALUES + sm.EDGE_SUBNORMAL:
        v, r = one_value(F, sr, 0.0, scale)
        assert v == want, (sr, scale, v, want)
        assert (r["erasures"], r["saturated"], r["abs_sum"]) == (0, int(abs(want) == 127), abs(want)), (sr, scale, r)
        assert sm.soft_values(np.array([[sr, 0.0]], np.float32), 2, 0, 0, scale)[0][0][0] == want, "the model alone"
    # float32 subnormals survive the widening to double: flushed to zero, both rows would give 0
    for sr, scale, want in sm.EDGE_SUBNORMAL:
        assert want != 0
    # a NaN part: v = 0 and one erasure, whatever the other part is; an infinite imaginary part meets the zero of the points' sines:
    # both correlations are NaN, none is the largest, L = -inf - -inf is a NaN: v = 0, and no erasure
    for sr, si in sm.EDGE_NAN:
        v, r = one_value(F, sr, si, 32.0)
        assert (v, r["erasures"], r["saturated"], r["abs_sum"]) == (0, 1, 0, 0), (sr, si)
    for sr, si in sm.EDGE_INF:
        v, r = one_value(F, sr, si, 32.0)
        assert (v, r["erasures"], r["abs_sum"]) == (0, 0, 0), (sr, si)
    # QPSK at rot 0, where the points lie on the axes and every product is exact: L_0 = sr + si for both labelings;
    # L_1 = |sr| - |si| with the plain labels and max(sr, -si) - max(si, -sr) with Gray's.  (1, 1) lies on the boundary of bit 1: L = 0
    for sr, si in sm.EDGE_PSK_SYMBOLS:
        for scale in sm.EDGE_PSK_SCALES:
            for gray in (0, 1):
                L = (sr + si, max(sr, -si) - max(si, -sr) if gray else abs(sr) - abs(si))
                want = [int(np.clip(np.floor(l * scale + 0.5), -127, 127)) for l in L]
                y = np.array([[sr, si]], np.float32)
                assert list(sm.soft_values(y, 4, 0, gray, scale)[0][0]) == want, (sr, si, scale, gray)
                v, r = one_value(F, sr, si, scale, 4, 0, gray)
                assert (r["abs_sum"], r["erasures"]) == (sum(abs(w) for w in want), 0), (sr, si, scale, gray, r)
    assert list(sm.soft_values(np.array([[1.0, 1.0]], np.float32), 4, 0, 0, 63.5)[0][0]) == [127, 0]
    # 8-PSK and rot = M - 1: against the model alone (one_value() holds the host to it)
    for sr, si, order, rot, gray, scale, want, erasures in sm.edge_rows():
        if order > 2:
            one_value(F, sr, si, scale, order, rot, gray)
    # QPSK, Gray, rot 1: the point of value 0 lies at a quarter turn; (inf, 1) has one NaN correlation (inf times the zero of that
    # point's cosine) and the others decide: bit 0 separates left from right... asserted against the model alone
    rng = np.random.default_rng(5)
    odd = np.array(sm.EDGE_ODD, np.float32)
    iq = np.stack([rng.choice(odd, 600), rng.choice(odd, 600)], 1)
    jobs = sm.place(sm.edge_odd_jobs(0))
    assert len(jobs) == 36 and iq.tobytes() == CASES["edges"][0][-600:].tobytes(), "the symbols of the edges case"
    rec, views = F.soft_host(iq, jobs)
    mrec, mouts = sm.decode((iq, jobs))
    assert rec.tobytes() == mrec.tobytes() and all(v.tobytes() == m[:len(v)].tobytes() for v, m in zip(views, mouts))
    nan = np.isnan(iq).any(1)
    for j, r in zip(jobs, rec):
        used = (r["n_coded"] + dm.bits_of(j["order"]) - 1) // dm.bits_of(j["order"])
        assert r["erasures"] == nan[:used].sum() > 0 and r["saturated"] > 0


def test_call_limit(lib):
    """64 jobs of MAX_STEPS, exactly MAX_CALL_STEPS: the host statement against the model, bit for bit; the same table with one
    more job of one step is refused with every byte and record at the sentinel"""
    case = sm.call_limit_case()
    jobs = case[1]
    steps = [sm.shape(j)[0] for j in jobs]
    assert len(jobs) == sm.LIMIT_JOBS == 64 and set(steps) == {sm.MAX_STEPS} and sum(steps) == sm.MAX_CALL_STEPS
    assert len({(int(j["k"]), int(j["n_poly"]), int(j["flags"]) & sm.TERMINATED) for j in jobs}) == 2 and list(jobs["out_offset"]) == sorted(jobs["out_offset"])
    rv, rec, got = host(lib, case)
    assert rv == 0
    want_rec, want = sm.image(case, SENTINEL, key="call_limit")
    got_rec = records_of(rec, len(jobs))
    for i in [i for i in range(len(want_rec)) if got_rec[i].tobytes() != want_rec[i].tobytes()][:6]:
        print("job %d %s got %s want %s" % (i, jobs[i], got_rec[i], want_rec[i]))
    assert got_rec.tobytes() == want_rec.tobytes(), "records bit-identical"
    assert got.tobytes() == want.tobytes(), "bytes bit-identical, every other byte at the sentinel"
    third = got_rec[jobs["n_poly"] == 3]
    assert (third["saturated"] > 0.99 * third["n_coded"]).all() and (third["abs_sum"] > 0.99 * 127 * 3 * sm.MAX_STEPS).all()
    assert (got_rec["metric"] > 0).all() and (got_rec["n_steps"] == sm.MAX_STEPS).all()
    more = sm.one_step_more(case)
    assert sum(sm.shape(j)[0] for j in more[1]) == sm.MAX_CALL_STEPS + 1 and more[1][:64].tobytes() == jobs.tobytes()
    rv, rec, out = host(lib, more)
    assert rv == EINVAL and np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"


# ---- the refusals -----------------------------------------------------------------------------------------------------------------

N_IQ, CAP = 3000, 4096


def good_jobs():
    """four jobs over 3000 samples and a capacity of 4096: the first fills d_out[0 .. 64), the last ends on both buffers' last bytes"""
    return np.concatenate([sm.make_job(0, 0, 512, 4, dm.K7, dm.P_NONE, dm.CRC16, 0, sm.TERMINATED, 3, 32.0),		# 512 steps, 506 bits: 64 bytes
                           sm.make_job(7, 64, 100, 8, dm.K5, dm.P_34, dm.CRC_NONE, 0, sm.GRAY, 7, 1e-3),			# 225 steps: 32 bytes
                           sm.make_job(3000, 96, 0, 2, dm.K3, dm.P_NONE, dm.CRC_NONE, 0, 0, 1, 1.0),				# no symbol, at the end
                           sm.make_job(2000, CAP - 64, 1000, 2, dm.K7, dm.P_NONE, dm.CRC32, 0, 3, 0, 3e38)])		# 500 steps: 64 bytes


F32_MAX, F32_TINY = float(np.finfo(np.float32).max), 1e-45


def refusal_pairs():
    """(the fields to change of good_jobs()[0] for a call that rule S5 refuses, the nearest change that is accepted)"""
    big = 2 ** 62
    return [(dict(offset=-1), dict(offset=0)), (dict(out_offset=-8), dict(out_offset=0)), (dict(n=-1), dict(n=0)),
            (dict(offset=2489), dict(offset=2488)), (dict(offset=3001, n=0), dict(offset=3000, n=0)), (dict(offset=big), dict(offset=2488)),
            (dict(offset=big, n=2 ** 31 - 1), dict(offset=0, n=3000, steps=1)),
            (dict(out_offset=CAP - 56), dict(out_offset=CAP - 64)), (dict(out_offset=CAP + 8, n=0), dict(out_offset=CAP, n=0)),
            (dict(out_offset=big), dict(out_offset=CAP - 64)), (dict(out_offset=4), dict(out_offset=8)), (dict(out_offset=1), dict(out_offset=0)),
            (dict(out_offset=12, n=0), dict(out_offset=16, n=0)),
            (dict(order=0), dict(order=2, rot=1)), (dict(order=1), dict(order=2, rot=0)), (dict(order=3), dict(order=4)), (dict(order=16), dict(order=8)),
            (dict(order=-2), dict(order=2, rot=0)), (dict(k=2, polys=(3, 1, 0)), dict(k=3, polys=(3, 1, 0))), (dict(k=8), dict(k=7)), (dict(k=0), dict(k=7)),
            (dict(n_poly=1), dict(n_poly=2)), (dict(n_poly=4), dict(n_poly=3, polys=(0o171, 0o133, 0o165))), (dict(n_poly=0), dict(n_poly=2)),
            (dict(period=0), dict(period=1)), (dict(period=17), dict(period=16)),
            (dict(crc_width=1), dict(crc_width=8, crc_poly=7, crc_init=0)), (dict(crc_width=12), dict(crc_width=16)),
            (dict(crc_width=33), dict(crc_width=32)), (dict(crc_width=64), dict(crc_width=32)),
            (dict(polys=(0, 0o133, 0)), dict(polys=(1, 0o133, 0))), (dict(polys=(0o171, 0, 0)), dict(polys=(0o171, 1, 0))),
            (dict(polys=(0o371, 0o133, 0)), dict(polys=(0o177, 0o133, 0))), (dict(polys=(0o171, 128, 0)), dict(polys=(0o171, 127, 0))),
            (dict(polys=(0o171, 0o133, 1)), dict(n_poly=3, polys=(0o171, 0o133, 1))), (dict(n_poly=3), dict(n_poly=3, polys=(0o171, 0o133, 1))),
            (dict(n_poly=3, polys=(0o171, 0o133, 128), punct=(1, 1, 1)), dict(n_poly=3, polys=(0o171, 0o133, 127), punct=(1, 1, 1))),
            (dict(punct=(2, 1, 0)), dict(punct=(1, 1, 0))), (dict(punct=(1, 2, 0)), dict(period=2, punct=(1, 2, 0))),
            (dict(punct=(0, 0, 0)), dict(punct=(1, 0, 0))), (dict(punct=(1, 1, 1)), dict(n_poly=3, polys=(0o171, 0o133, 1), punct=(1, 1, 1))),
            (dict(period=3, punct=(8, 1, 0)), dict(period=3, punct=(7, 1, 0))), (dict(steps=-1), dict(steps=0)), (dict(steps=513), dict(steps=512)),
            (dict(steps=sm.MAX_STEPS + 1, n=3000, period=16, punct=(1, 0, 0)), dict(steps=sm.MAX_STEPS, n=3000, period=16, punct=(1, 0, 0), out_offset=0, flags=0)),
            (dict(n=2 ** 31 - 1, offset=0), dict(n=3000, offset=0, steps=1)),
            (dict(order=8, n=3000, period=16, punct=(1, 0, 0)), dict(order=8, n=3000, period=16, punct=(1, 0, 0), steps=sm.MAX_STEPS, flags=0)),
            (dict(crc_poly=1 << 16), dict(crc_poly=0xffff)), (dict(crc_init=1 << 16), dict(crc_init=0xffff)), (dict(crc_xorout=1 << 16), dict(crc_xorout=0xffff)),
            (dict(crc_width=0), dict(crc_width=0, crc_poly=0, crc_init=0)), (dict(crc_width=0, crc_poly=0, crc_init=1), dict(crc_width=0, crc_poly=0, crc_init=0)),
            (dict(crc_width=8), dict(crc_width=8, crc_poly=0xff, crc_init=0xff)),
            # what this pass adds
            (dict(flags=4), dict(flags=3)), (dict(flags=8), dict(flags=2)), (dict(flags=-1), dict(flags=0)), (dict(flags=1 << 14), dict(flags=1)),
            (dict(rot=4), dict(rot=3)), (dict(rot=-1), dict(rot=0)), (dict(order=2, rot=2), dict(order=2, rot=1)), (dict(order=8, rot=8), dict(order=8, rot=7)),
            (dict(rot=2 ** 31 - 1), dict(rot=3)),
            (dict(scale=0.0), dict(scale=F32_TINY)), (dict(scale=-0.0), dict(scale=F32_TINY)), (dict(scale=-1.0), dict(scale=1.0)),
            (dict(scale=-F32_TINY), dict(scale=F32_TINY)), (dict(scale=np.inf), dict(scale=F32_MAX)), (dict(scale=-np.inf), dict(scale=F32_MAX)),
            (dict(scale=np.nan), dict(scale=1.0))]


def changed(job, **kw):
    j = job.copy()
    for k, v in kw.items():
        j[k] = v
    return j


def test_einval_table(lib):
    """each refused call leaves every byte and every record at the sentinel; beside each stands the nearest call that is accepted,
    and it gives what the model gives"""
    rng = np.random.default_rng(91)
    iq = rng.standard_normal((N_IQ, 2)).astype(np.float32)
    good = good_jobs()
    rv, rec, out = host(lib, (iq, good), cap=CAP)
    want_rec, want = sm.image((iq, good), SENTINEL)
    assert rv == 0 and records_of(rec, 4).tobytes() == want_rec.tobytes() and out[:CAP].tobytes() == want[:CAP].tobytes()
    assert np.all(out[96:CAP - 64] == SENTINEL) and list(want_rec["n_steps"]) == [512, 225, 0, 500]

    def refused(jobs, **kw):
        kw.setdefault("cap", CAP)
        rv, rec, out = host(lib, (iq, jobs), **kw)
        assert rv == EINVAL, (jobs, kw)
        assert np.all(out == SENTINEL) and np.all(rec == SENTINEL32), "nothing is written"

    def accepted(jobs, **kw):
        kw.setdefault("cap", CAP)
        rv, rec, out = host(lib, (iq, jobs), **kw)
        assert rv == 0, (jobs, kw)
        return records_of(rec, len(jobs))

    for what in ("iq", "jobs", "records", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); accepted(good[:1], n_jobs=1)
    refused(good, n_jobs=-1); refused(np.repeat(good[2:3], sm.MAX_JOBS + 1)); accepted(np.repeat(good[2:3], sm.MAX_JOBS))
    refused(good, n_samples=-1); refused(good, n_samples=2999); accepted(good, n_samples=3000)
    refused(good, cap=-1); refused(good, cap=CAP - 8); accepted(good, cap=CAP)
    for no, yes in refusal_pairs():
        refused(changed(good[:1], **no))
        job = changed(good[:1], **yes)
        cap = max(CAP, int(job["out_offset"][0]) + sm.job_owned(job[0]))
        got = accepted(job, cap=cap)
        assert got.tobytes() == sm.decode((iq, job))[0].tobytes(), yes
    refused(np.concatenate([good[:1], changed(good[1:2], out_offset=56)]))			# [0, 64) and [56, 88)
    accepted(np.concatenate([good[:1], changed(good[1:2], out_offset=64)]))
    refused(np.concatenate([changed(good[1:2], out_offset=200), changed(good[:1], out_offset=168)]))	# [200, 232) and [168, 232), descending
    accepted(np.concatenate([changed(good[1:2], out_offset=232), changed(good[:1], out_offset=168)]))
    for name, by in (("records", 4), ("out", 4), ("out", 1), ("iq", 4)):
        refused(good, skew=(name, by))
    # the sum of the steps of a call: 64 jobs of MAX_STEPS are 2^22 steps and fit, one step more does not
    long = sm.make_job(0, 0, N_IQ, 8, dm.K3, (16, (1, 0, 0)), dm.CRC_NONE, sm.MAX_STEPS, 0, 0, 1.0)	# one bit in 16 steps: 4096 bits
    many = np.repeat(long, 64)
    many["out_offset"] = 8192 * np.arange(64)
    assert host(lib, (iq, many), cap=64 * 8192)[0] == 0
    refused(np.concatenate([many, changed(long, steps=1, out_offset=64 * 8192)]), cap=65 * 8192)
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    rec = np.full(W, SENTINEL32, np.uint32)
    out = np.full(256, SENTINEL32, np.uint32)
    assert lib.fosphor_amd_soft(None, iq.ctypes.data, N_IQ, good.ctypes.data, 1, rec.ctypes.data, out.ctypes.data, 1024) == EINVAL
    assert np.all(rec == SENTINEL32) and np.all(out == SENTINEL32)
    assert lib.fosphor_amd_soft_stats(None, None) == EINVAL


# ---- the helpers and the chain ------------------------------------------------------------------------------------------------------

def test_from_decide_and_derive(lib, F):
    import decide_model as dec
    L = gr_fosphor_amd._lib
    # behind the word, all of it or n_payload; no word found: nothing; no word asked for: from the job's first symbol, rot 0
    dj = dec.make_jobs([(40, 0, 500, 4, dec.UW | dec.GRAY, 0, 32, 0, 0, 2), (600, 512, 300, 8, dec.UW, 0, 32, 0, 0, 2), (1000, 1024, 200, 2, 0)])
    dr = np.zeros(3, dec.RECORD_DTYPE)
    dr["n"], dr["order"], dr["status"], dr["uw_pos"], dr["uw_rot"] = (500, 300, 200), (4, 8, 2), (dec.OK, dec.NO_UW, dec.OK), (100, 7, -1), (3, 5, 0)
    dr["a"] = (250.0, 300.0, 800.0)
    jobs = F.soft_jobs(dj, dr, 32)
    assert jobs.dtype == sm.JOB_DTYPE and list(jobs["offset"]) == [40 + 132, 600, 1000] and list(jobs["n"]) == [368, 0, 200]
    assert list(jobs["order"]) == [4, 8, 2] and list(jobs["rot"]) == [3, 0, 0] and list(jobs["flags"]) == [sm.GRAY, 0, 0]
    assert list(jobs["scale"]) == [np.float32(16.0 * 500 / 250.0), np.float32(1.0), np.float32(16.0 * 200 / 800.0)]
    assert set(jobs["k"]) == {7} and [tuple(p) for p in jobs["polys"]] == [(0o171, 0o133, 0)] * 3
    assert list(jobs["out_offset"]) == [0, 48 + 8, 56 + 8]						# 368 steps: 48 bytes; none; 100 steps: 16
    # a BPSK symbol of the mean length a / n gets |v| = 32
    mean = 250.0 / 500
    iq = np.array([[mean, 0.0], [-mean, 0.0]], np.float32)
    rec, _ = F.soft_host(iq, sm.make_job(0, 0, 2, 2, dm.K3, dm.P_NONE, dm.CRC_NONE, 1, 0, 0, jobs["scale"][0]))
    assert rec["abs_sum"][0] == 64 and rec["metric"][0] == 32
    jobs = F.soft_jobs(dj[:1], dr[:1], 32, n_payload=300, k=5, polys=(0o23, 0o35), period=3, punct=(3, 5), flags="terminated", crc_width=16,
                       crc_poly=0x1021, crc_init=0xffff, gap=1)
    j = jobs[0]
    assert (j["n"], j["k"], j["n_poly"], j["period"], j["crc_width"], j["flags"], j["crc_poly"], j["crc_init"]) == (300, 5, 2, 3, 16, 3, 0x1021, 0xffff)
    assert tuple(j["punct"]) == (3, 5, 0) and j["steps"] == 0 and j["rot"] == 3
    with pytest.raises(ValueError):
        F.soft_jobs(dj, dr, 32, flags="diff")
    job = L.SoftJob()
    job.out_offset, job.k = 99, 9
    make = lib.fosphor_amd_soft_from_decide
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), 32, 368, C.byref(job)) == 0
    assert (job.offset, job.out_offset, job.n, job.order, job.steps, job.flags, job.k, job.crc_width, job.rot, job.scale) == (172, 0, 368, 4, 0, 2, 0, 0, 3, 32.0)
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), 32, 369, C.byref(job)) == EINVAL, "the payload runs past the job"
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), 401, 0, C.byref(job)) == EINVAL, "the word runs past the job"
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), 32, -1, C.byref(job)) == EINVAL
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), -1, 0, C.byref(job)) == EINVAL
    assert make(dj[2:].tobytes(), dr[2:].tobytes(), 32, 201, C.byref(job)) == EINVAL
    assert make(dj[2:].tobytes(), dr[2:].tobytes(), 32, 200, C.byref(job)) == 0 and (job.offset, job.n, job.rot) == (1000, 200, 0)
    assert make(dj[1:2].tobytes(), dr[1:2].tobytes(), 32, 5000, C.byref(job)) == 0 and (job.n, job.offset, job.scale) == (0, 600, 1.0), "no word: nothing to decode"

    def with_(arr, **kw):
        a = arr.copy()
        for k, v in kw.items():
            a[k] = v
        return a.tobytes()

    for flags in (dec.DIFF, dec.DIFF | dec.UW, dec.DIFF | dec.GRAY):
        assert make(with_(dj[:1], flags=flags), dr[:1].tobytes(), 32, 0, C.byref(job)) == EINVAL, "differential decisions have no soft form"
    for a in (0.0, -1.0, np.inf, -np.inf, np.nan, 1e-300, 1e300):			# the last two: a scale that float32 cannot hold above 0
        assert make(dj[:1].tobytes(), with_(dr[:1], a=a), 32, 0, C.byref(job)) == EINVAL, a
        assert make(dj[1:2].tobytes(), with_(dr[1:2], a=a), 32, 0, C.byref(job)) == 0, "n = 0: a is not looked at"
    assert make(dj[:1].tobytes(), with_(dr[:1], a=1e-30), 32, 0, C.byref(job)) == 0 and job.scale == np.float32(16.0 * 500 / 1e-30)
    assert make(dj[:1].tobytes(), with_(dr[:1], uw_rot=4), 32, 0, C.byref(job)) == EINVAL
    assert make(dj[:1].tobytes(), with_(dr[:1], uw_rot=-1), 32, 0, C.byref(job)) == EINVAL
    assert make(dj[:1].tobytes(), with_(dr[:1], order=3), 32, 0, C.byref(job)) == EINVAL
    assert make(with_(dj[:1], offset=-4), dr[:1].tobytes(), 32, 0, C.byref(job)) == EINVAL
    assert make(None, dr[:1].tobytes(), 32, 0, C.byref(job)) == EINVAL and make(dj[:1].tobytes(), None, 32, 0, C.byref(job)) == EINVAL
    assert make(dj[:1].tobytes(), dr[:1].tobytes(), 32, 0, None) == EINVAL
    with pytest.raises(ValueError):
        F.soft_jobs(dj, dr[:2], 32)
    # records built by hand
    r = np.zeros(1, sm.RECORD_DTYPE)
    r["n_steps"], r["n_coded"], r["metric"], r["abs_sum"] = 300, 400, 10, 8000
    v = F.soft_derive(r)[0]
    assert set(v) == set(F.SOFT_VALUES) and v == dict(mean_abs=20.0, corrected_share=0.00125, rate=0.75, crc_ok=1.0)
    r["status"] = sm.CRC_FAIL
    assert F.soft_derive(r)[0]["crc_ok"] == 0.0
    assert F.soft_derive(np.zeros(1, sm.RECORD_DTYPE))[0] == dict(mean_abs=0.0, corrected_share=0.0, rate=0.0, crc_ok=1.0), "0 / 0 is 0"
    r["abs_sum"] = 0
    assert F.soft_derive(r)[0]["corrected_share"] == 0.0, "10 / 0 is 0"
    vals = L.SoftValues()
    assert lib.fosphor_amd_soft_derive(None, C.byref(vals)) == EINVAL and lib.fosphor_amd_soft_derive(r.tobytes(), None) == EINVAL


CHAIN_SEED, CHAIN_SIGMA, CHAIN_INFO, CHAIN_UW = 11, 0.3, 400, 32
CHAIN_CODE = dict(k=7, polys=(0o171, 0o133), period=3, punct=(0b011, 0b101), steps=422, flags="terminated", crc_width=16, crc_poly=0x1021,
                  crc_init=0xffff)


def chain_burst():
    """a QPSK burst at symbol level, Gray: 16 symbols of noise, a 32-symbol word, then a K = 7, 3/4-punctured, CRC-16, terminated
    payload of 400 info bits; a carrier of 0.3 turns and 2e-4 turns a symbol, so that fosphor_amd_carrier leaves a quarter turn to
    the unique word; white noise of 0.3 a part (Es / N0 = 7.4 dB) -> (iq float32 [n][2], word, info, payload symbols).  The carrier
    job takes the frequency as known (FREQ_FIXED) and estimates the phase: the test is about the steps behind it, not about the
    threshold of the lag-16 frequency estimate over fourth powers of noisy symbols"""
    rng = np.random.default_rng(CHAIN_SEED)
    word = rng.integers(0, 4, CHAIN_UW).astype(np.uint8)
    info = rng.integers(0, 2, CHAIN_INFO)
    payload, T = dm.frame(info, dm.K7, dm.P_34, 4, dm.CRC16, True)
    assert T == CHAIN_CODE["steps"]
    z = np.concatenate([sm.noise(rng, 16, 0.7), np.exp(2j * np.pi * word / 4), sm.modulate(payload, 4, 0, True)])
    z = z * np.exp(2j * np.pi * (0.3 + 2e-4 * np.arange(len(z)))) + sm.noise(rng, len(z), CHAIN_SIGMA)
    return sm.pairs(z), word, info, payload


def chain_jobs(n):
    import carrier_model as cm
    import decide_model as dec
    return cm.make_jobs([(0, 0, n, 4, cm.FREQ_FIXED, 16, 2e-4, 0.0)]), dec.UW | dec.GRAY


def test_chain_on_the_host(F):
    """carrier_host -> decide_host -> soft_jobs -> soft_host over the synthetic burst: the word is found behind the 16 noise symbols
    under a rotation that is not 0, the hard chain over the same symbols corrects coded bits, and the soft decoder returns the
    planted bits with the CRC held.  Seed and noise were chosen on the CPU; the values are asserted as the host gives them"""
    import decide_model as dec
    iq, word, info, payload = chain_burst()
    cjobs, dflags = chain_jobs(len(iq))
    crec, cviews = F.carrier_host(iq, cjobs)
    assert crec["status"][0] == 0
    c = cviews[0].view(np.float32).reshape(-1, 2)
    djobs = F.decide_jobs(cjobs, crec, dflags, 0, CHAIN_UW, 0, 0, 4)
    drec, dviews = F.decide_host(c, djobs, word)
    assert (drec["status"][0], drec["uw_pos"][0]) == (dec.OK, 16) and drec["uw_rot"][0] != 0
    jobs = F.soft_jobs(djobs, drec, CHAIN_UW, **CHAIN_CODE)
    assert (jobs["offset"][0], jobs["n"][0], jobs["rot"][0], jobs["flags"][0]) == (48, len(payload), drec["uw_rot"][0], 3)
    assert jobs["scale"][0] == np.float32(16.0 * drec["n"][0] / drec["a"][0]) and 12.0 < jobs["scale"][0] < 20.0
    rec, views = F.soft_host(c, jobs)
    assert rec.tobytes() == sm.decode((c, jobs))[0].tobytes()
    sym = np.zeros(dec.owned(len(iq)), np.uint8)
    sym[:len(iq)] = dviews[0]
    hrec, hviews = F.decode_host(sym, F.decode_jobs(djobs, drec, CHAIN_UW, **CHAIN_CODE))
    v = F.soft_derive(rec)[0]
    print("chain: rot %d, scale %.3f, hard metric %d status %d; soft metric %d status %d mean |v| %.2f corrected share %.4f saturated %d"
          % (drec["uw_rot"][0], jobs["scale"][0], hrec["metric"][0], hrec["status"][0], rec["metric"][0], rec["status"][0], v["mean_abs"],
             v["corrected_share"], rec["saturated"][0]))
    assert hrec["metric"][0] > 0, "the channel inverted coded bits"
    assert (rec["status"][0], rec["n_steps"][0], rec["n_bits"][0], rec["n_coded"][0], rec["end_state"][0]) == (sm.OK, 422, 416, 563, 0)
    assert rec["crc_calc"][0] == rec["crc_recv"][0] == dm.crc_bits(info, dm.CRC16)
    assert list(dm.unpack(views[0], CHAIN_INFO)) == list(info), "the decoded bits are the planted ones"
    assert v["crc_ok"] == 1.0 and abs(v["rate"] - 0.75) < 0.002 and 0 < v["corrected_share"] < 0.1 and rec["erasures"][0] == 0


def test_soft_kernels_meet_their_resources(F):
    """-Rpass-analysis=kernel-resource-usage: fosphor_soft.hip has exactly four kernels, each with 0 bytes of scratch and the
    static LDS that the header states for it; the VGPR counts are printed (profiles/r24_soft.md has them), no cap is set on them"""
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
    ours = {k: v for k, v in found.items() if "k_sft_" in k}
    assert len(ours) == 4 and len(found) == 4, sorted(found)
    forms = set()
    for name, res in ours.items():
        form = re.search(r"k_sft_(bits|acs|trace|rec)", name).group(1)
        forms.add(form)
        print(form, res)
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("LDS Size") == F.SOFT_LDS[form] == header_value("FOSPHOR_AMD_SOFT_LDS_" + form.upper()), (name, res)
    assert forms == {"bits", "acs", "trace", "rec"}
