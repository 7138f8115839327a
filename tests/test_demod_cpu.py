"""Host side of include/fosphor_amd_demod.h, no GPU: fosphor_amd_atan2_turns and fosphor_amd_demod_host against the numpy statement
(tests/demod_model.py), bit for bit, on every input set the GPU tests use; the cut rule; the refusals; demod_n_out and
demod_from_extract; planted tones.

Bit for bit means tobytes(): signed zeros, subnormals and the one quiet NaN included."""
import ctypes as C
import errno

import numpy as np
import pytest

import demod_model as dm
import measure_model as mm
from _pkg import gr_fosphor_amd

EINVAL = -errno.EINVAL
CASES = dm.cases()
SENTINEL = 0x5a5a5a5a


@pytest.fixture(scope="module")
def lib():
    return gr_fosphor_amd.load()


@pytest.fixture(scope="module")
def F():
    gr_fosphor_amd.load()
    return gr_fosphor_amd.Fosphor


def host(lib, iq, jobs, n_samples=None, n_jobs=None, cap=None, null=(), skew_iq=0, skew_out=0):
    """-> (return value, the whole output buffer as uint32, sentinel-filled before the call)"""
    iq = np.ascontiguousarray(iq, np.float32).reshape(-1, 2)
    jobs = np.ascontiguousarray(jobs, dm.JOB_DTYPE)
    size = dm.capacity(jobs) if cap is None else max(cap, 0) + dm.GUARD
    buf = np.full(size + 1, SENTINEL, np.uint32)
    keep = iq if iq.size else np.zeros((1, 2), np.float32)
    rv = lib.fosphor_amd_demod_host(None if "iq" in null else keep.ctypes.data + skew_iq, len(iq) if n_samples is None else n_samples,
                                    None if "jobs" in null else jobs.ctypes.data, len(jobs) if n_jobs is None else n_jobs,
                                    None if "out" in null else buf.ctypes.data + skew_out, size if cap is None else cap)
    return rv, buf[:size]


def test_the_dtype_mirrors_the_struct(F):
    assert dm.JOB_DTYPE.itemsize == 32 and C.sizeof(gr_fosphor_amd._lib.DemodJob) == 32
    assert F.DEMOD_JOB_DTYPE == dm.JOB_DTYPE and F.DEMOD_STATS == dm.STATS and F.DEMOD_MODES == dm.MODES
    assert (F.DEMOD_MAX_JOBS, F.DEMOD_MAX_AVG, F.DEMOD_TILE) == (dm.MAX_JOBS, dm.MAX_AVG, dm.TILE)


def test_atan2_turns_seam_table(lib, F):
    """the table of rule 2, value for value and sign for sign"""
    inf = np.inf
    table = [((0.0, 1.0), 0.0), ((-0.0, 1.0), -0.0), ((0.0, -1.0), 0.5), ((-0.0, -1.0), -0.5), ((1.0, 0.0), 0.25),
             ((-1.0, 0.0), -0.25), ((1.0, 1.0), 0.125), ((1.0, -1.0), 0.375), ((0.0, 0.0), 0.0), ((inf, inf), 0.125),
             ((inf, 1.0), 0.25), ((1.0, -inf), 0.5)]
    for (y, x), want in table:
        for got in (lib.fosphor_amd_demod_atan2_turns(y, x), float(F.atan2_turns(y, x)), float(dm.atan2_turns(y, x))):
            assert got == want and np.signbit(got) == np.signbit(want), (y, x, got, want)
    for y, x in ((np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.nan, np.inf)):
        assert np.isnan(lib.fosphor_amd_demod_atan2_turns(y, x))
    assert lib.fosphor_amd_demod_atan2_turns_n(None, None, 1, None) == EINVAL


def test_atan2_turns_equals_the_model_on_the_seams(F):
    y, x = dm.seam_pairs()
    assert len(y) > 100
    got, want = F.atan2_turns(y, x), dm.atan2_turns(y, x)
    for i in np.flatnonzero(got.view(np.uint32) != want.view(np.uint32)):
        print("y %r x %r got %r want %r" % (y[i], x[i], got[i], want[i]))
    assert got.tobytes() == want.tobytes()
    assert np.all(np.abs(want[~np.isnan(want)]) <= 0.5)
    sub = want[(want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)]
    assert len(sub) >= 2, "the set reaches subnormal float32 results of both signs"


def random_pairs(count, seed):
    """float32 pairs with magnitudes over e^+-20, as float64"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((count, 2)) * np.exp(rng.uniform(-20.0, 20.0, (count, 2)))).astype(np.float32).astype(np.float64)
    return a[:, 0], a[:, 1]


def test_atan2_turns_equals_the_model_on_a_million_random_pairs(F):
    y, x = random_pairs(10 ** 6, 1)
    assert F.atan2_turns(y, x).tobytes() == dm.atan2_turns(y, x).tobytes()


def test_atan2_turns_is_within_one_ulp_of_arctan2(F):
    """Derived, not measured: the double chain is within 4e-12 relative of atan2 / (2 pi) -- the series for atan(u) / u is cut at
    z^13 / 27 <= 0.1716^13 / 27 = 4.1e-12 with |u| <= tan(pi / 8), and the twenty-odd double roundings add some 1e-15 -- which
    is 7e-5 float32 ulp; the one rounding to float32 costs at most 0.5 ulp.  np.arctan2 / (2 pi) in float64 stands for the exact
    value (good to 1e-15).  Within 1 ulp of float32 AT the exact value.  The inputs are such that the exact result is zero or a
    normal float32: magnitudes over e^+-20 keep |result| above 1e-18."""
    y, x = random_pairs(200000, 2)
    sy, sx = dm.seam_pairs()
    ok = np.isfinite(sy) & np.isfinite(sx) & ((sy != 0) | (sx != 0))
    y, x = np.concatenate([y, sy[ok]]), np.concatenate([x, sx[ok]])
    exact = np.arctan2(y, x) / (2.0 * np.pi)
    keep = (exact == 0) | (np.abs(exact) >= np.finfo(np.float32).tiny)
    y, x, exact = y[keep], x[keep], exact[keep]
    got = F.atan2_turns(y, x).astype(np.float64)
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    err = np.abs(got - exact) / ulp
    print("largest error %.6f ulp over %d pairs" % (err.max(), len(err)))
    assert np.all(err <= 1.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_model(lib, F, name):
    iq, jobs = CASES[name]
    rv, got = host(lib, iq, jobs)
    assert rv == 0
    want = dm.image(iq, jobs, SENTINEL)
    for i in np.flatnonzero(got != want)[:10]:
        print("float %d got %08x want %08x" % (i, got[i], want[i]))
    assert got.tobytes() == want.tobytes(), "outputs bit-identical, every other float at the sentinel"
    views = F.demod_host(iq, jobs)
    for v, w in zip(views, dm.demod(iq, jobs)):
        assert v.tobytes() == w.tobytes(), "the Python front end gives the same traces"
    if name == "nonfinite":
        out = dm.demod(iq, jobs)
        assert np.isnan(out[0][100]) and out[0][200] == np.inf and np.isfinite(out[0][[99, 101, 199, 201]]).all()
        assert np.isnan(out[4][[99, 100]]).all() and np.isfinite(out[4][[98, 101]]).all()		# FM: a sample is in two values
        assert np.isnan(out[3][25]) and np.isfinite(out[3][[24, 26]]).all()					# PHASE, L = 4
        assert out[2][2600] == 0.0											# the angle of (0, 0)
    if name == "mixed257":
        assert len(jobs) == 257 and set(jobs["mode"]) == {0, 1, 2} and (jobs["avg"] == 1).any() and (jobs["avg"] > 1).any()


def test_the_cut_rule(lib):
    """rule 3: a job gives, bit for bit, the outputs of the two jobs it is cut into at a multiple of L; for FM they share a sample"""
    iq, jobs, triples = dm.cut_case()
    rv, got = host(lib, iq, jobs)
    assert rv == 0
    assert got.tobytes() == dm.image(iq, jobs, SENTINEL).tobytes()
    assert {(int(jobs["mode"][w]), int(jobs["avg"][w])) for w, _, _, _ in triples} == {(m, L) for m in (0, 1, 2) for L in (1, 3, 64)}

    def outputs(i):
        j = jobs[i]
        at = int(j["out_offset"])
        return got[at:at + dm.n_out(int(j["mode"]), int(j["n"]), int(j["avg"]))]

    for w, a, b, c in triples:
        whole, first, second = outputs(w), outputs(a), outputs(b)
        assert len(first) == c and len(first) + len(second) == len(whole) and len(second) >= 1
        assert whole[:c].tobytes() == first.tobytes() and whole[c:].tobytes() == second.tobytes(), (w, c)


def test_n_out_and_from_extract(lib, F):
    for mode, name in ((dm.POWER, "power"), (dm.PHASE, "phase"), (dm.FM, "fm")):
        for n in (0, 1, 2, 255, 256, 257, 2 ** 31 - 1):
            for L in (1, 2, 3, 255, 256):
                assert lib.fosphor_amd_demod_n_out(mode, n, L) == dm.n_out(mode, n, L) == F.demod_n_out(name, n, L)
    for mode, n, L in ((3, 1, 1), (-1, 1, 1), (0, -1, 1), (0, 1, 0), (0, 1, 257)):
        assert lib.fosphor_amd_demod_n_out(mode, n, L) == EINVAL
    with pytest.raises(ValueError):
        F.demod_n_out("magnitude", 1)
    e = np.zeros(3, F.EXTRACT_DTYPE)
    e["out_offset"], e["n_out"], e["first"], e["decim"], e["n_taps"] = (7, 1000, 2000), (33, 0, 10), (5, 6, 7), 4, 9
    jobs = F.demod_jobs(e, mode="fm", avg=4)
    assert jobs.dtype == dm.JOB_DTYPE and list(jobs["offset"]) == [7, 1000, 2000] and list(jobs["n"]) == [33, 0, 10]
    assert list(jobs["out_offset"]) == [0, 8, 8] and set(jobs["mode"]) == {dm.FM} and set(jobs["avg"]) == {4} and not jobs["reserved"].any()
    assert list(F.demod_jobs(e, mode="power", avg=1)["out_offset"]) == [0, 33, 33]
    job = gr_fosphor_amd._lib.DemodJob()
    job.out_offset, job.reserved = 99, 99
    assert lib.fosphor_amd_demod_from_extract(e[:1].tobytes(), dm.PHASE, 2, C.byref(job)) == 0
    assert (job.offset, job.out_offset, job.n, job.mode, job.avg, job.reserved) == (7, 0, 33, dm.PHASE, 2, 0)
    for bad, mode, L in ((dict(out_offset=-1), 0, 1), (dict(n_out=-1), 0, 1), ({}, 3, 1), ({}, 0, 0), ({}, 0, 257)):
        x = e[:1].copy()
        for k, v in bad.items():
            x[k] = v
        assert lib.fosphor_amd_demod_from_extract(x.tobytes(), mode, L, C.byref(job)) == EINVAL
    assert lib.fosphor_amd_demod_from_extract(None, 0, 1, C.byref(job)) == EINVAL
    assert lib.fosphor_amd_demod_from_extract(e[:1].tobytes(), 0, 1, None) == EINVAL


def test_einval_table(lib):
    iq = dm.noise(1000, 41)
    good = [(0, 3, 10, dm.POWER, 1), (990, 13, 10, dm.FM, 1), (1000, 22, 0, dm.PHASE, 1), (0, 22, 1000, dm.PHASE, 4)]
    cap = 22 + 250
    rv, out = host(lib, iq, dm.make_jobs(good), cap=cap)
    assert rv == 0 and np.all(out[:3] == SENTINEL) and np.all(out[3:13] != SENTINEL) and np.all(out[cap:] == SENTINEL)

    def refused(rows, **kw):
        kw.setdefault("cap", cap)
        jobs = dm.make_jobs([r[:5] for r in rows])
        for j, r in zip(jobs, rows):
            j["reserved"] = r[5] if len(r) > 5 else 0
        rv, out = host(lib, iq, jobs, **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL), "nothing is written"

    for what in ("iq", "jobs", "out"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (dm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=999); refused(good, cap=-1); refused(good, cap=cap - 1)
    refused([(-1, 0, 10, 0, 1)]); refused([(0, 0, -1, 0, 1)]); refused([(991, 0, 10, 0, 1)]); refused([(1001, 0, 0, 0, 1)])
    refused([(2 ** 62, 0, 2 ** 31 - 1, 0, 1)]); refused([(0, -1, 10, 0, 1)]); refused([(0, cap + 1, 0, 0, 1)])
    refused([(0, 2 ** 62, 10, 0, 1)])
    refused([(0, 0, 10, 3, 1)]); refused([(0, 0, 10, -1, 1)]); refused([(0, 0, 10, 0, 0)]); refused([(0, 0, 10, 0, dm.MAX_AVG + 1)])
    refused([(0, 0, 10, 0, 1, 1)])
    refused([(0, 0, 10, dm.POWER, 1), (0, 9, 10, dm.FM, 1)])			# outputs [0, 10) and [9, 18): one float shared
    refused([(0, 30, 100, dm.PHASE, 4), (0, 0, 31, dm.POWER, 1)])		# [30, 55) and [0, 31), given in descending order
    refused(good, skew_iq=4); refused(good, skew_out=2)
    # the last jobs that still fit, in the input and in the output; outputs that touch; a job without outputs anywhere inside
    ok = [(0, 0, 10, dm.POWER, 1), (0, 10, 10, dm.FM, 1), (0, cap - 250, 1000, dm.POWER, 4), (0, cap, 3, dm.FM, 4), (1000, 5, 0, 0, 1)]
    assert host(lib, iq, dm.make_jobs(ok), cap=cap)[0] == 0
    many = dm.make_jobs([(0, i, 1, dm.POWER, 1) for i in range(dm.MAX_JOBS)])
    assert host(lib, iq, many)[0] == 0
    # more than 2^31 - 1 work-groups in one form: MAX_JOBS overlapping jobs of 2^31 - 1 samples (2^20 DIRECT tiles each), refused
    # before a sample is read; half as many jobs would be accepted and are not tried
    n = 2 ** 31 - 1
    huge = dm.make_jobs([(0, i * 2 ** 31, n, dm.POWER, 1) for i in range(dm.MAX_JOBS)])
    buf = np.full(8, SENTINEL, np.uint32)
    assert lib.fosphor_amd_demod_host(iq.ctypes.data, n, huge.ctypes.data, len(huge), buf.ctypes.data, 2 ** 44) == EINVAL
    assert np.all(buf == SENTINEL)
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    assert lib.fosphor_amd_demod(None, iq.ctypes.data, 1000, dm.make_jobs(good).ctypes.data, 4, iq.ctypes.data, cap) == EINVAL
    assert lib.fosphor_amd_demod_stats(None, None) == EINVAL


TONES = (0.0, 0.01, -0.01, 0.25, -0.25, 0.49)


@pytest.mark.parametrize("f", TONES)
def test_phase_and_fm_of_a_planted_tone(F, f):
    """The samples are the float32 roundings of the unit phasor exp(2 pi i (f m + 0.1)): each component moves by at most 2^-25
    (half an ulp below 1), so a sample's angle is off by less than sqrt(2) * 2^-25 < 2^-24 rad = 2^-24 / (2 pi) < 2^-26 turn.
    PHASE: that, the angle's own error (4e-12 relative) and its rounding to float32 (at most 2^-26 turn for a result in
    [-0.5, 0.5]) stay below 2^-25 turn per sample: inside the 2^-23 asked for.  The trace differs from f m + 0.1 by whole turns
    only: unwrapped, it is f m + 0.1 within 2^-23 turn at every sample.
    FM: two samples' angle errors, below 2^-25 turn together, the rounding of z (2^-53 relative) and of the result (at most 2^-26)
    stay below 2^-24 turn: inside the 2^-22 asked for.  |f| < 0.5 so the step never wraps."""
    n = 4096
    iq = dm.tone(n, f)
    jobs = dm.place([(0, n, dm.PHASE, 1), (0, n, dm.FM, 1), (0, n, dm.FM, 16)])
    phase, fm, fm16 = (v.astype(np.float64) for v in F.demod_host(iq, jobs))
    want = f * np.arange(n) + 0.1
    d = phase - want
    err = np.abs(d - np.round(d))
    print("f %g: phase %.3g turn, fm %.3g, fm16 %.3g" % (f, err.max(), np.abs(fm - f).max(), np.abs(fm16 - f).max()))
    assert np.all(err <= 2.0 ** -23)
    assert len(fm) == n - 1 and np.all(np.abs(fm - f) <= 2.0 ** -22)
    assert len(fm16) == (n - 1) // 16 and np.all(np.abs(fm16 - f) <= 2.0 ** -22)
    assert abs(fm.mean() - f) <= 2.0 ** -22


def test_chain_on_the_host(lib, F):
    """extract_host's float32 output of measure_model's chain stream, then the model's FM trace of the tone burst: its mean is off
    the planted frequency by 9.96e-8 cycles per output sample (the stream's noise, averaged over 1966 trace values).  The GPU test
    allows the device chain twice this figure; it is held here from both sides so that it stays what the reference shows."""
    raw, ejobs, planted = mm.chain_case()
    taps = F.extract_design(mm.CHAIN_DECIM, mm.CHAIN_TAPS, 0.8)
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    out = np.zeros((cap, 2), np.float32)
    assert lib.fosphor_amd_extract_host(raw.ctypes.data, len(raw), 2, ejobs.ctypes.data, len(ejobs), taps.ctypes.data, len(taps),
                                        out.ctypes.data, cap) == 0
    for mode, avg in (("fm", 1), ("power", 8)):
        jobs = F.demod_jobs(ejobs, mode=mode, avg=avg)
        want = dm.demod(out, jobs)
        for g, w in zip(F.demod_host(out, jobs), want):
            assert len(w) > 100 and g.tobytes() == w.tobytes()
        if mode == "fm":
            off = abs(float(want[0].astype(np.float64).mean()) - planted)
            print("tone: mean of the FM trace off by %.4g over %d values" % (off, len(want[0])))
            assert 9.9e-8 <= off <= 9.96e-8
