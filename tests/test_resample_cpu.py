"""Host side of include/fosphor_amd_resample.h, no GPU: fosphor_amd_resample_host against the numpy statement
(tests/resample_model.py), the whole output buffer bit for bit, on every input set the GPU tests use; the model against a plain
zero-stuff-and-correlate reference; the identity job; the cut rule; resample_n_out, resample_design, resample_ratio and
resample_from_extract; the refusals; the chain extract_host -> resample_host -> correlate_host.

Bit for bit means tobytes(): signed zeros, subnormals and the one quiet NaN included."""
import ctypes as C
import errno
import math

import numpy as np
import pytest

import resample_model as rm
from _pkg import gr_fosphor_amd

EINVAL = -errno.EINVAL
CASES = rm.cases()
SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def lib():
    return gr_fosphor_amd.load()


@pytest.fixture(scope="module")
def F():
    gr_fosphor_amd.load()
    return gr_fosphor_amd.Fosphor


def host(lib, case, n_samples=None, n_taps=None, n_jobs=None, cap=None, null=(), skew=None):
    """-> (return value, the whole output buffer as uint32 [2 * size]), sentinel-filled before the call.  cap: out_capacity,
    GUARD samples of the buffer lie behind it; skew: (pointer name, bytes)"""
    iq = np.ascontiguousarray(case[0], np.float32).reshape(-1, 2)
    taps = np.ascontiguousarray(case[1], np.float32)
    jobs = np.ascontiguousarray(case[2], rm.JOB_DTYPE)
    size = rm.capacity(jobs) if cap is None else max(cap, 0) + rm.GUARD
    buf = np.full(2 * size + 2, SENTINEL, np.uint32)
    ptr = {"iq": (iq if iq.size else np.zeros((1, 2), np.float32)).ctypes.data, "taps": taps.ctypes.data, "jobs": jobs.ctypes.data,
           "out": buf.ctypes.data}
    keep = (iq, taps)						# the arrays behind the pointers live until the call returns
    for k in null:
        ptr[k] = None
    if skew:
        ptr[skew[0]] += skew[1]
    rv = lib.fosphor_amd_resample_host(ptr["iq"], len(iq) if n_samples is None else n_samples, ptr["jobs"],
                                       len(jobs) if n_jobs is None else n_jobs, ptr["taps"], len(taps) if n_taps is None else n_taps,
                                       ptr["out"], size if cap is None else cap)
    del keep
    return rv, buf[:2 * size]


def explain(got, want, jobs):
    for i in np.flatnonzero(got != want)[:8]:
        own = [k for k, j in enumerate(jobs) if 2 * int(j["out_offset"]) <= i < 2 * (int(j["out_offset"]) + int(j["n_out"]))]
        print("float %d got %08x want %08x job %s" % (i, got[i], want[i], [(k, tuple(jobs[k])) for k in own]))


def test_the_dtype_mirrors_the_struct(F):
    L = gr_fosphor_amd._lib
    assert rm.JOB_DTYPE.itemsize == 48 and C.sizeof(L.ResampleJob) == 48 and F.RESAMPLE_JOB_DTYPE == rm.JOB_DTYPE
    assert [(k, rm.JOB_DTYPE.fields[k][1]) for k in rm.JOB_DTYPE.names] == [(k, getattr(L.ResampleJob, k).offset)
                                                                             for k, _ in L.ResampleJob._fields_]
    assert F.RESAMPLE_STATS == rm.STATS
    assert (F.RESAMPLE_MAX_JOBS, F.RESAMPLE_MAX_UP, F.RESAMPLE_MAX_DOWN, F.RESAMPLE_MAX_BRANCH) == (rm.MAX_JOBS, rm.MAX_UP, rm.MAX_DOWN,
                                                                                                   rm.MAX_BRANCH)
    assert (F.RESAMPLE_TILE, F.RESAMPLE_TILE_LDS, F.RESAMPLE_DIRECT_OUT) == (rm.TILE, rm.TILE_LDS, rm.DIRECT_OUT)
    header = open(gr_fosphor_amd._lib.ROOT + "/include/fosphor_amd_resample.h").read()
    for name, value in (("MAX_JOBS", rm.MAX_JOBS), ("MAX_UP", rm.MAX_UP), ("MAX_DOWN", rm.MAX_DOWN), ("MAX_BRANCH", rm.MAX_BRANCH),
                        ("TILE", rm.TILE), ("TILE_LDS", rm.TILE_LDS), ("DIRECT_OUT", rm.DIRECT_OUT)):
        assert "#define FOSPHOR_AMD_RESAMPLE_%s " % name in header.replace("\t", " ")
        line = [l for l in header.splitlines() if l.startswith("#define FOSPHOR_AMD_RESAMPLE_%s" % name) and l.split()[1].endswith(name)][0]
        assert int(line.split()[2]) == value, name
    for U, D, T in ((1, 1, 1), (1, 9, 8), (1, 10, 8), (256, 1, 39 * 256), (256, 1, 40 * 256), (1, 256, 1), (255, 256, 255)):
        assert F.resample_form(U, D, T) == rm.form(U, D, T)


def test_the_cases_hold_what_they_promise():
    """the seams are in the sets, and no set is larger than the model runs in seconds"""
    for name, case in CASES.items():
        assert rm.macs(case[2]) <= rm.MAX_MACS, name
    assert rm.macs(rm.cut_case()[0][2]) <= rm.MAX_MACS
    jobs = np.concatenate([c[2] for c in CASES.values()])
    for j in jobs:
        assert 0 <= j["n_out"] <= rm.max_n_out(int(j["n"]), int(j["up"]), int(j["down"]), int(j["n_taps"]), int(j["phase0"]))
    assert set(rm.COUNTS) <= set(jobs["n_out"]) and {0, 1, 255, 256, 257, rm.TILE - 1, rm.TILE, rm.TILE + 1, 2 * rm.TILE + 1} == set(rm.COUNTS)
    assert {(int(j["up"]), int(j["down"])) for j in jobs} >= set(rm.RATIOS)
    assert {(int(j["up"]), int(j["down"]), int(j["n_taps"]) // int(j["up"])) for j in CASES["ratios"][2]} == {(u, d, q) for u, d in rm.RATIOS
                                                                                                               for q in rm.QS}
    assert {(int(j["offset"]) & 1, int(j["out_offset"]) & 1) for j in jobs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {0, 1, 2, 3} <= set(jobs["offset"]) and {0, 1, 2, 3} <= set(jobs["taps_offset"])
    firsts = {(int(j["phase0"]) % int(j["up"]) == 0) for j in jobs if j["up"] > 1}
    assert firsts == {True, False}, "branch 0 and a later branch at output 0"
    iq, _, cj = CASES["counts"]
    assert (cj["offset"] + cj["n"]).max() == len(iq), "a job ends on the buffer's last sample"
    exact = [j for j in cj if j["n_out"] == 1 and j["phase0"] == (int(j["n"]) - int(j["n_taps"]) // int(j["up"])) * int(j["up"])]
    assert len(exact) >= 2, "phase0 = (n - Q) U exactly, in both forms"
    for name in ("counts", "nonfinite", "mixed257", "seam"):
        forms = {rm.form(int(j["up"]), int(j["down"]), int(j["n_taps"])) for j in CASES[name][2] if j["n_out"] > 0}
        assert forms == {"tile", "direct"}, (name, "a call with both forms")
    sj = CASES["seam"][2]
    assert [rm.form(int(j["up"]), int(j["down"]), int(j["n_taps"])) for j in sj] == ["tile", "direct"] * 3
    assert sj["down"][3] == sj["down"][2] + 1 and sj["n_taps"][1] == sj["n_taps"][0] + 256 and sj["n_taps"][5] == sj["n_taps"][4] + 255
    assert all(sj[k][0] == sj[k][1] for k in ("offset", "phase0", "n", "n_out", "up", "down")), "the same job in both forms"
    mixed = CASES["mixed257"][2]
    assert len(mixed) == 257 and mixed["n_out"].max() > 2 * rm.TILE


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_model(lib, F, name):
    case = CASES[name]
    jobs = case[2]
    rv, got = host(lib, case)
    assert rv == 0
    want = rm.image(case, SENTINEL)
    explain(got, want, jobs)
    assert got.tobytes() == want.tobytes(), "outputs bit-identical, every other float at the sentinel"
    views = F.resample_host(case[0], jobs, case[1])
    for j, v in zip(jobs, views):
        assert v.dtype == np.complex64 and v.tobytes() == rm.outputs_of(want, j).tobytes(), "the Python front end gives the same"
    if name == "seam":
        a, b = rm.outputs_of(got, jobs[0]), rm.outputs_of(got, jobs[1])
        assert len(a) == 2 * (rm.TILE + 5) and a.tobytes() == b.tobytes(), "the same job in both forms is bit-identical"
    if name == "nonfinite":
        f = got.view(np.float32)
        for j in jobs:
            o = rm.outputs_of(f, j).reshape(-1, 2)
            nan = np.isnan(o)
            assert nan.any() and not nan.all() and np.isinf(o).any()
            assert np.all(rm.outputs_of(got, j).reshape(-1, 2)[nan] == 0x7fc00000), "one quiet NaN"
        # U = D = T = 1: output m is taps[0] * x[m]: the inf stays an inf, the subnormal samples stay subnormal
        copy = rm.outputs_of(f, jobs[4]).reshape(-1, 2)
        assert np.isinf(copy[900, 0]) and np.isnan(copy[291, 0])
        assert np.all(np.abs(copy[2000:2040]) < 1.2e-38) and np.any(copy[2000:2040] != 0.0)
        tile = rm.outputs_of(f, jobs[0]).reshape(-1, 2)		# (3, 2, 4): taps 5 and 6 are zeros: inf * 0
        assert np.isnan(tile[:, 0]).sum() > 4


def test_model_against_a_plain_reference():
    """The polyphase sum of rule 1 against what it stands for: zero-stuff x by U in float64, correlate with h as written
    (np.correlate, "valid"), pick phase0 + m D.  The tolerance is derived, not measured: one float32 rounding of the result,
    2^-24 |ref|, and Q additions in double of terms bounded by |h| max|x| each, Q 2^-52 sum|h| max|x| (the reference's own
    additions of exact zeros add nothing; its non-zero terms are the model's in another order)."""
    rng = np.random.default_rng(3)
    for U, D, Q, phase0 in ((1, 1, 1, 0), (3, 2, 4, 0), (3, 2, 4, 5), (2, 3, 5, 1), (7, 5, 3, 11), (1, 4, 9, 2), (5, 1, 2, 3),
                            (16, 15, 8, 40)):
        n = 90
        x = rm.noise(n, 100 + U)
        h = rng.standard_normal(Q * U).astype(np.float32)
        n_out = rm.max_n_out(n, U, D, Q * U, phase0)
        assert n_out > 3
        job = rm.make_jobs([(0, 0, phase0, n, n_out, U, D, 0, Q * U)])[0]
        got = rm.resample_job(x, h, job).astype(np.float64)
        assert len(rm.resample_job(x, h, job)) == n_out
        xc = x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)
        xu = np.zeros(n * U, np.complex128)			# U - 1 zeros behind every sample, the last included
        xu[::U] = xc
        h64 = h.astype(np.float64)
        full = np.correlate(xu, h64, "valid")			# full[p] = sum over k of xu[p + k] h[k] (h is real)
        pos = phase0 + np.arange(n_out) * D
        assert pos[-1] < len(full) <= phase0 + n_out * D, "n_out is the largest valid: one more output would leave the samples"
        ref = full[pos]
        bound = Q * 2.0 ** -52 * np.abs(h64).sum() * np.abs(x).max()
        for part, r in ((got[:, 0], ref.real), (got[:, 1], ref.imag)):
            err = np.abs(part - r)
            tol = 2.0 ** -24 * np.abs(r) + bound
            print("U %d D %d Q %d phase0 %d: worst error / tolerance %.3f" % (U, D, Q, phase0, (err / tol).max()))
            assert np.all(err <= tol)


def test_identity_job(lib, F):
    """U = D = 1, T = 1, h = { 1.0f } copies bit for bit: zeros, subnormals and infinities included.  What rule 2 pins leaves two
    exceptions, which the header states: the sum begins at +0.0, so a sample of -0.0 comes out as +0.0 (0.0 + -0.0), and a NaN
    comes out as the quiet NaN"""
    iq = rm.noise(700, 7)
    iq[3] = (0.0, 0.0)
    iq[4] = (np.float32(1e-42), np.float32(-3e-45))
    iq[5] = (np.inf, -np.inf)
    iq[6, 1] = np.nan
    jobs = rm.make_jobs([(1, 2, 0, 650, 650, 1, 1, 1, 1)])
    out = F.resample_host(iq, jobs, np.array([0.5, 1.0], np.float32))[0]
    want = iq[1:651].copy()
    want[5, 1] = rm.QNAN
    assert out.tobytes() == want.tobytes() and out.tobytes() == rm.resample_job(iq, [0.5, 1.0], jobs[0]).tobytes()
    iq[3] = (-0.0, -0.0)
    out = F.resample_host(iq, jobs, np.array([0.5, 1.0], np.float32))[0]
    assert out.tobytes() == want.tobytes(), "-0.0 comes out as +0.0"


def test_the_cut_rule(lib):
    """rule 3: a job gives, bit for bit, the outputs of the two jobs it is cut into at output c"""
    case, triples = rm.cut_case()
    jobs = case[2]
    rv, got = host(lib, case)
    assert rv == 0
    want = rm.image(case, SENTINEL)
    assert got.tobytes() == want.tobytes()
    rm.assert_cut([rm.outputs_of(got, j) for j in jobs], triples)
    assert {(int(jobs["up"][w]), int(jobs["down"][w]), int(jobs["n_taps"][w]) // int(jobs["up"][w])) for w, _, _, _ in triples} == set(rm.CUT_FORMS)
    assert {rm.form(u, d, q * u) for u, d, q in rm.CUT_FORMS} == {"tile", "direct"}


def test_n_out_helper(lib, F):
    """the largest valid n_out against brute force: the count of m = 0, 1, .. for which b + Q <= n"""
    every = np.arange(40 * 8 + 2)
    for U in range(1, 9):
        for D in range(1, 9):
            for Q in range(1, 5):
                for n in range(0, 41):
                    for phase0 in range(0, 2 * U + 1):
                        m = int((-(-(phase0 + every * D) // U) + Q <= n).sum())
                        assert lib.fosphor_amd_resample_n_out(n, U, D, Q * U, phase0) == m == rm.max_n_out(n, U, D, Q * U, phase0), (U, D, Q, n, phase0)
    assert F.resample_n_out(100, 3, 2, 12) == rm.max_n_out(100, 3, 2, 12) == 145 and F.resample_n_out(100, 3, 2, 12, phase0=288) == 1
    assert F.resample_n_out(100, 3, 2, 12, phase0=289) == 0 and F.resample_n_out(100, 3, 2, 12, phase0=2 ** 62) == 0
    assert lib.fosphor_amd_resample_n_out(2 ** 31 - 1, 1, 1, 1, 0) == 2 ** 31 - 1
    for n, U, D, T, ph in ((-1, 1, 1, 1, 0), (1, 0, 1, 1, 0), (1, 257, 1, 257, 0), (1, 1, 0, 1, 0), (1, 1, 257, 1, 0), (1, 2, 1, 3, 0),
                           (1, 1, 1, 0, 0), (1, 1, 1, 65, 0), (1, 2, 1, 130, 0), (1, 1, 1, 1, -1), (2 ** 31 - 1, 2, 1, 2, 0)):
        assert lib.fosphor_amd_resample_n_out(n, U, D, T, ph) == EINVAL, (n, U, D, T, ph)
    with pytest.raises(ValueError):
        F.resample_n_out(10, 2, 1, 3)


def test_design(lib, F):
    for U, D, Q, guard in ((1, 1, 1, 0.8), (1, 1, 33, 0.8), (3, 2, 4, 0.8), (2, 3, 12, 0.8), (7, 5, 3, 1.0), (256, 1, 64, 0.5),
                           (1, 256, 64, 0.8), (255, 256, 9, 0.9), (160, 147, 16, 0.8)):
        h = F.resample_design(U, D, Q, guard)
        T = Q * U
        assert h.dtype == np.float32 and len(h) == T
        assert h.tobytes() == h[::-1].tobytes(), "symmetric to the bit"
        # each tap is rounded once, by at most 2^-24 of itself, and no tap of a windowed sinc that sums to U is above U
        assert abs(h.astype(np.float64).sum() - U) <= T * 2.0 ** -24 * U, (U, D, Q)
        for s in range(U if Q >= 8 else 0):
            assert abs(h[s::U].astype(np.float64).sum() - 1.0) < 0.05, "every branch has a gain near 1"
    # U = D = 1: the formulas coincide -- fc = guard / 2, the same window, g / sum * 1 -- so the taps are extract's, bit for bit
    for T in (1, 2, 9, 64):
        assert F.resample_design(1, 1, T, 0.7).tobytes() == F.extract_design(1, T, 0.7).tobytes()
    # a decimator's prototype is extract's for the same D and T
    assert F.resample_design(1, 8, 64, 0.8).tobytes() == F.extract_design(8, 64, 0.8).tobytes()
    out = np.zeros(8, np.float32)
    for U, D, Q, guard in ((0, 1, 1, 0.8), (257, 1, 1, 0.8), (1, 0, 1, 0.8), (1, 257, 1, 0.8), (1, 1, 0, 0.8), (1, 1, 65, 0.8), (1, 1, 1, 0.0),
                           (1, 1, 1, 1.5), (1, 1, 1, math.nan)):
        assert lib.fosphor_amd_resample_design(U, D, Q, guard, out.ctypes.data) == EINVAL
    assert lib.fosphor_amd_resample_design(1, 1, 1, 0.8, None) == EINVAL
    with pytest.raises(ValueError):
        F.resample_design(1, 1, 65)


def best_ratio(r, cap):
    """brute force over all up, down <= cap: the smallest |up / down - r|"""
    u, d = np.meshgrid(np.arange(1, cap + 1), np.arange(1, cap + 1))
    return float(np.abs(u / d - r).min())


def test_ratio(lib, F):
    assert F.resample_ratio(2.0, 3.0)[:2] == (3, 2) and F.resample_ratio(2.0, 3.0)[2] == 0.0
    assert F.resample_ratio(3e6, 2e6, 3)[:2] == (2, 3) and F.resample_ratio(48000.0, 44100.0)[:2] == (147, 160)
    for k, want in ((1, (25, 1536)), (2, (25, 768)), (4, (25, 384)), (8, (25, 192)), (10, (125, 768)), (16, (25, 96)), (20, (125, 384))):
        up, down, err = F.resample_ratio(61.44e6, 1e6 * k)
        r = 1e6 * k / 61.44e6
        if want[1] <= 256:
            assert (up, down) == want and abs(err) < 1e-15, k
        assert abs(up / down - r) == best_ratio(r, 256) and math.gcd(up, down) == 1, k
        assert abs(err - (61.44e6 * up / down - 1e6 * k) / (1e6 * k)) < 1e-15
    rng = np.random.default_rng(9)
    targets = [math.pi, math.e, math.sqrt(2.0), 1.0 / math.pi, math.sqrt(0.5), (1.0 + math.sqrt(5.0)) / 2.0, 1e-3, 1e3, 255.5, 1.0 / 255.5]
    targets += list(np.exp(rng.uniform(-6.0, 6.0, 200)))
    for r in targets:
        for cap in (1, 2, 3, 7, 16, 100, 256, 1000):
            up, down, err = F.resample_ratio(1.0, r, cap)
            top = min(cap, 256)
            assert 1 <= up <= top and 1 <= down <= top and math.gcd(up, down) == 1
            assert abs(up / down - r) == best_ratio(r, top), (r, cap, up, down)
    assert F.resample_ratio(1.0, math.pi, 1)[:2] == (1, 1) and F.resample_ratio(1.0, math.pi, 7)[:2] == (3, 1)
    assert F.resample_ratio(1.0, math.pi, 22)[:2] == (22, 7) and F.resample_ratio(1.0, 1.0 / math.pi, 22)[:2] == (7, 22)
    up, down, err = C.c_int(0), C.c_int(0), C.c_double(0.0)
    assert lib.fosphor_amd_resample_ratio(1.0, 2.0, 4, C.byref(up), C.byref(down), None) == 0 and (up.value, down.value) == (2, 1)
    for a, b, cap in ((0.0, 1.0, 4), (1.0, 0.0, 4), (-1.0, 1.0, 4), (math.inf, 1.0, 4), (1.0, math.inf, 4), (math.nan, 1.0, 4), (1.0, math.nan, 4),
                      (1.0, 1.0, 0), (1.0, 1.0, -3)):
        assert lib.fosphor_amd_resample_ratio(a, b, cap, C.byref(up), C.byref(down), C.byref(err)) == EINVAL
    assert lib.fosphor_amd_resample_ratio(1.0, 1.0, 4, None, C.byref(down), None) == EINVAL
    assert lib.fosphor_amd_resample_ratio(1.0, 1.0, 4, C.byref(up), None, None) == EINVAL
    with pytest.raises(ValueError):
        F.resample_ratio(0.0, 1.0)


def test_from_extract(lib, F):
    e = np.zeros(3, F.EXTRACT_DTYPE)
    e["out_offset"], e["n_out"], e["first"], e["decim"], e["n_taps"] = (7, 1000, 2000), (33, 0, 10), (5, 6, 7), 4, 9
    jobs = F.resample_jobs(e, 2, 3, 24)
    assert jobs.dtype == rm.JOB_DTYPE and list(jobs["offset"]) == [7, 1000, 2000] and list(jobs["n"]) == [33, 0, 10]
    assert list(jobs["n_out"]) == [rm.max_n_out(33, 2, 3, 24), 0, 0] == [15, 0, 0] and list(jobs["out_offset"]) == [0, 15, 15]
    assert set(jobs["up"]) == {2} and set(jobs["down"]) == {3} and set(jobs["n_taps"]) == {24} and not jobs["phase0"].any()
    assert not jobs["taps_offset"].any()
    assert list(F.resample_jobs(e, 3, 1, 6)["out_offset"]) == [0, 94, 94]
    job = gr_fosphor_amd._lib.ResampleJob()
    job.out_offset = job.phase0 = job.taps_offset = 99
    assert lib.fosphor_amd_resample_from_extract(e[:1].tobytes(), 3, 2, 12, C.byref(job)) == 0
    assert (job.offset, job.out_offset, job.phase0, job.n, job.n_out, job.up, job.down, job.taps_offset, job.n_taps) == (7, 0, 0, 33, 44, 3, 2, 0, 12)
    for bad, U, D, T in ((dict(out_offset=-1), 1, 1, 1), (dict(n_out=-1), 1, 1, 1), ({}, 0, 1, 1), ({}, 1, 0, 1), ({}, 257, 1, 257), ({}, 1, 257, 1),
                         ({}, 2, 1, 3), ({}, 1, 1, 65), ({}, 1, 1, 0)):
        x = e[:1].copy()
        for k, v in bad.items():
            x[k] = v
        assert lib.fosphor_amd_resample_from_extract(x.tobytes(), U, D, T, C.byref(job)) == EINVAL
    assert lib.fosphor_amd_resample_from_extract(None, 1, 1, 1, C.byref(job)) == EINVAL
    assert lib.fosphor_amd_resample_from_extract(e[:1].tobytes(), 1, 1, 1, None) == EINVAL
    with pytest.raises(ValueError):
        F.resample_jobs(e, 2, 3, 25)


def test_einval_table(lib):
    """each refused call leaves every float at the sentinel"""
    iq, taps = rm.noise(1000, 91), rm.some_taps(100, 92)
    #        offset out phase0 n    n_out U  D  taps_offset T
    good = [(0, 3, 0, 110, 100, 3, 2, 0, 12), (990, 0, 0, 10, 3, 1, 4, 90, 2), (1000, 103, 0, 0, 0, 1, 1, 99, 1),
            (0, 104, 5, 500, 30, 1, 16, 36, 5), (5, 140, 7, 3, 0, 2, 1, 0, 8)]
    cap = 104 + 30 + 10
    rv, out = host(lib, (iq, taps, rm.make_jobs(good)), cap=cap)
    assert rv == 0 and np.all(out[:206] != SENTINEL) and np.all(out[206:208] == SENTINEL) and np.all(out[208:268] != SENTINEL)
    assert np.all(out[268:] == SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        rv, out = host(lib, (iq, taps, rm.make_jobs(rows)), **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL), "nothing is written"

    for what in ("iq", "jobs", "taps", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (rm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=999); refused(good, n_taps=-1); refused(good, n_taps=99)
    refused(good, cap=-1); refused(good, cap=133)
    ok = (0, 0, 0, 10, 4, 1, 1, 0, 4)

    def one(**kw):
        row = dict(zip(rm.FIELDS, ok))
        row.update(kw)
        refused([tuple(row.values())])

    one(offset=-1); one(out_offset=-1); one(phase0=-1); one(n=-1); one(n_out=-1); one(offset=991); one(offset=1001, n=0, n_out=0)
    one(offset=2 ** 62, n=2 ** 31 - 1); one(offset=2 ** 62); one(up=0); one(up=-1); one(up=rm.MAX_UP + 1, n_taps=rm.MAX_UP + 1)
    one(down=0); one(down=-1); one(down=rm.MAX_DOWN + 1); one(n_taps=0); one(n_taps=-4); one(up=3, n_taps=4); one(n_taps=rm.MAX_BRANCH + 1)
    one(up=2, n_taps=2 * rm.MAX_BRANCH + 2); one(taps_offset=-1); one(taps_offset=97); one(taps_offset=101, n_taps=1); one(taps_offset=2 ** 31 - 1)
    one(n_out=8); one(n_out=2 ** 31 - 1); one(phase0=1, n_out=7); one(phase0=7, n_out=1); one(phase0=2 ** 62, n_out=1); one(n=3, n_out=1)
    one(down=2, n_out=5); one(up=2, n_taps=8, n_out=14)
    one(out_offset=cap + 1, n_out=0); one(out_offset=2 ** 62); one(out_offset=cap - 3)
    refused([(0, 0, 0, 10, 7, 1, 1, 0, 4), (0, 6, 0, 10, 7, 1, 1, 0, 4)])		# [0, 7) and [6, 13): one sample shared
    refused([(0, 30, 0, 100, 90, 1, 1, 0, 4), (0, 0, 0, 40, 31, 1, 1, 0, 4)])	# [30, 120) and [0, 31), given in descending order
    for name in ("iq", "out"):
        refused(good, skew=(name, 4))
    refused(good, skew=("taps", 2))
    # the last jobs that still fit, in the inputs, the taps and the output; outputs that touch; jobs without outputs anywhere inside
    last = [(0, 0, 0, 10, 7, 1, 1, 0, 4), (0, 7, 6, 10, 1, 1, 1, 96, 4), (990, cap - 7, 0, 10, 7, 1, 1, 0, 4), (1000, cap, 2 ** 62, 0, 0, 1, 1, 99, 1),
            (3, 5, 0, 3, 0, 1, 1, 0, 4), (0, 8, 0, 1000, 13, 25, 24, 0, 100)]
    rv, out = host(lib, (iq, taps, rm.make_jobs(last)), cap=cap)
    assert rv == 0 and out[:2 * cap].tobytes() == rm.image((iq, taps, rm.make_jobs(last)), SENTINEL)[:2 * cap].tobytes()
    many = rm.make_jobs([(0, i, 0, 1, 1, 1, 1, 0, 1) for i in range(rm.MAX_JOBS)])
    assert host(lib, (iq, taps, many))[0] == 0
    # more than 2^31 - 1 work-groups in one form: MAX_JOBS copies of 2^31 - 1 samples (2^22 tiles each), their outputs side by
    # side in a capacity that exists as a number only; refused before a sample is read or written.  A quarter as many jobs
    # would be accepted and are not tried
    n = 2 ** 31 - 1
    huge = rm.make_jobs([(0, i * n, 0, n, n, 1, 1, 0, 1) for i in range(rm.MAX_JOBS)])
    buf = np.full(16, SENTINEL, np.uint32)
    assert lib.fosphor_amd_resample_host(iq.ctypes.data, n, huge.ctypes.data, len(huge), taps.ctypes.data, 100, buf.ctypes.data,
                                         rm.MAX_JOBS * n) == EINVAL
    assert np.all(buf == SENTINEL)
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    assert lib.fosphor_amd_resample(None, iq.ctypes.data, 1000, many.ctypes.data, 1, taps.ctypes.data, 100, buf.ctypes.data, 8) == EINVAL
    assert lib.fosphor_amd_resample_stats(None, None) == EINVAL
    assert np.all(buf == SENTINEL)


def test_chain_on_the_host(lib, F):
    """A preamble planted in noise in a small sc16 stream at 3 / 2 extract-output samples per template sample, through
    fosphor_amd_extract_host, fosphor_amd_resample_host (2 / 3) and fosphor_amd_correlate_host.  The conditions on the input
    are asserted here, with the values printed: after resampling the peak is at the planted lag and at least twice the largest
    rho more than T / 4 lags away; correlating the extract output as it is gives a peak rho below half the resampled one."""
    import correlate_model as cm
    raw, ejobs, tpl, planted = rm.chain_case()
    taps = F.extract_design(rm.CHAIN_DECIM, rm.CHAIN_TAPS, 0.8)
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    ext = np.zeros((cap, 2), np.float32)
    assert lib.fosphor_amd_extract_host(raw.ctypes.data, len(raw), 2, ejobs.ctypes.data, len(ejobs), taps.ctypes.data, len(taps),
                                        ext.ctypes.data, cap) == 0
    h = F.resample_design(rm.CHAIN_UP, rm.CHAIN_DOWN, rm.CHAIN_BRANCH, 0.8)
    rjobs = F.resample_jobs(ejobs, rm.CHAIN_UP, rm.CHAIN_DOWN, len(h))
    assert rm.form(rm.CHAIN_UP, rm.CHAIN_DOWN, len(h)) == "tile" and rjobs["n_out"][0] > 4 * rm.TILE
    res = F.resample_host(ext, rjobs, h)[0]
    assert res.tobytes() == rm.resample_job(ext, h, rjobs[0]).tobytes()

    def correlate(iq, n):
        jobs = cm.make_jobs([(0, 0, rm.CHAIN_TPL_OFFSET, n, rm.CHAIN_T, cm.RHO, 0.5)])
        records, views = F.correlate_host(iq, jobs, tpl)
        return records, views[0]

    records, rho = correlate(res, len(res))
    peak, far = rm.chain_margin(rho, planted)
    plain_records, _ = correlate(ext[int(ejobs["out_offset"][0]):], int(ejobs["n_out"][0]))
    print("chain: resampled peak rho %.4f at lag %d (planted %d), largest rho beyond T / 4 lags %.4f; not resampled: peak rho %.4f"
          % (peak, records["peak_lag"][0], planted, far, plain_records["peak_rho"][0]))
    assert planted > rm.TILE and records["n_lags"][0] > 2 * cm.TILE
    assert records["peak_lag"][0] == planted
    assert peak >= 2.0 * far, "the condition on the input"
    assert plain_records["peak_rho"][0] < 0.5 * records["peak_rho"][0], "the template does not fit the extract output's rate"
    assert F.correlate_derive(records, 1.0)[0]["detections"] == 1
