"""Host side of include/fosphor_amd_measure.h, no GPU: fosphor_amd_measure_host against the numpy statement
(tests/measure_model.py) on every input set the GPU tests use, a job cut in two, the refusals, measure_from_extract, and
measure_derive on records whose answers are known.

Integers must be equal; a sum must be within n * 2^-52 * sum|term| of math.fsum over its terms (mm.tolerance: derived in rule 3 of
the header, not measured)."""
import ctypes as C
import errno

import numpy as np
import pytest

import measure_model as mm
from _pkg import gr_fosphor_amd

EINVAL = -errno.EINVAL
CASES = mm.cases()


@pytest.fixture(scope="module")
def lib():
    return gr_fosphor_amd.load()


@pytest.fixture(scope="module")
def F():
    gr_fosphor_amd.load()
    return gr_fosphor_amd.Fosphor


def host(lib, iq, jobs, n_samples=None, n_jobs=None, null=(), skew_iq=0, skew_rec=0):
    """-> (return value, records)"""
    iq = np.ascontiguousarray(iq, np.float32).reshape(-1, 2)
    jobs = np.ascontiguousarray(jobs, mm.JOB_DTYPE)
    buf = np.zeros((len(jobs) + 1) * mm.RECORD_DTYPE.itemsize + 8, np.uint8)
    keep = iq if iq.size else np.zeros((1, 2), np.float32)
    rv = lib.fosphor_amd_measure_host(None if "iq" in null else keep.ctypes.data + skew_iq, len(iq) if n_samples is None else n_samples,
                                      None if "jobs" in null else jobs.ctypes.data, len(jobs) if n_jobs is None else n_jobs,
                                      None if "records" in null else buf.ctypes.data + skew_rec)
    return rv, buf[skew_rec:skew_rec + len(jobs) * mm.RECORD_DTYPE.itemsize].view(mm.RECORD_DTYPE)


def test_the_dtypes_mirror_the_structs(F):
    assert mm.JOB_DTYPE.itemsize == 16 and mm.RECORD_DTYPE.itemsize == 96
    assert F.MEASURE_JOB_DTYPE == mm.JOB_DTYPE and F.MEASURE_RECORD_DTYPE == mm.RECORD_DTYPE
    assert F.MEASURE_STATS == mm.STATS and (F.MEASURE_WAVE_MAX, F.MEASURE_CHUNK, F.MEASURE_MAX_JOBS) == (mm.WAVE_MAX, mm.CHUNK, mm.MAX_JOBS)
    assert [F.measure_form(n) for n in (0, mm.WAVE_MAX, mm.WAVE_MAX + 1)] == ["wave", "wave", "split"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_against_model(lib, F, name):
    iq, jobs = CASES[name]
    rv, got = host(lib, iq, jobs)
    assert rv == 0
    mm.assert_records(got, mm.measure(iq, jobs), mm.tolerance(CASES[name]), name)
    assert np.array_equal(F.measure_host(iq, jobs).tobytes(), got.tobytes()), "the Python front end gives the same records"
    if name == "planted":
        n = int(jobs["n"][0])
        for r in got[:2]:
            assert (r["peak_index"], r["first_above"], r["last_above"]) == (mm.CHUNK - 1, mm.CHUNK - 3, n - 1)
            assert (r["n_edges"], r["n_above"]) == (4, 6 + 70 + 1 + 1)
    if name == "nonfinite":
        assert got["peak_power"][1] == np.inf and got["peak_index"][1] == 11 and got["peak_index"][2] == -1
        assert not np.isfinite(got["s_p"][1])


@pytest.mark.parametrize("cut", [1, 2, 777, 4096, 8191, 8192, 8193, 9999])
def test_a_job_cut_in_two_recombines(lib, cut):
    """the integers recombine exactly (indices offset, the edge at the cut counted once); the sums add inside the tolerance, r1
    after the one term at the cut, y[cut] * conj(y[cut - 1]), is put back"""
    iq = mm.bursty(10001, 31)
    iq[cut - 1] = iq[cut] = (0.9, 0.1) if cut % 2 else iq[cut]		# odd cuts: above on both sides of the cut
    n, thr = 10000, 0.3
    rv, rec = host(lib, iq, mm.make_jobs([(1, n, thr), (1, cut, thr), (1 + cut, n - cut, thr)]))
    assert rv == 0
    w, a, b = rec
    p = mm.power(iq[1:1 + n])
    both = bool(p[cut - 1] >= np.float32(thr)) and bool(p[cut] >= np.float32(thr))
    shift = lambda v: -1 if v < 0 else v + cut
    assert w["n_above"] == a["n_above"] + b["n_above"]
    assert w["first_above"] == (a["first_above"] if a["first_above"] >= 0 else shift(b["first_above"]))
    assert w["last_above"] == (shift(b["last_above"]) if b["last_above"] >= 0 else a["last_above"])
    assert w["n_edges"] == a["n_edges"] + b["n_edges"] - int(both)
    best = (a["peak_power"], a["peak_index"]) if a["peak_power"] >= b["peak_power"] else (b["peak_power"], b["peak_index"] + cut)
    assert (w["peak_power"], w["peak_index"]) == best
    tol = mm.job_tolerance(iq, mm.make_jobs([(1, n, thr)])[0])
    y = iq[1:1 + n].astype(np.float64)
    at = {"r1_re": y[cut, 0] * y[cut - 1, 0] + y[cut, 1] * y[cut - 1, 1], "r1_im": y[cut, 1] * y[cut - 1, 0] - y[cut, 0] * y[cut - 1, 1]}
    for k in mm.SUMS:
        assert abs(float(w[k]) - (float(a[k]) + float(b[k]) + at.get(k, 0.0))) <= tol[k], (k, cut)


def test_einval_table(lib):
    iq = mm.bursty(1000, 41)
    good = [(0, 10, 0.3), (990, 10, 0.3), (1000, 0, 0.3)]
    rv, rec = host(lib, iq, mm.make_jobs(good))
    assert rv == 0 and list(rec["n"]) == [10, 10, 0]

    def refused(rows, **kw):
        rv, rec = host(lib, iq, mm.make_jobs(rows), **kw)
        assert rv == EINVAL, (rows, kw)
        assert not rec.tobytes().strip(b"\0"), "nothing is written"

    for what in ("iq", "jobs", "records"):
        refused(good, null=(what,))
    refused(good, n_jobs=0); refused(good, n_jobs=-1); refused([good[0]] * (mm.MAX_JOBS + 1))
    refused(good, n_samples=-1); refused(good, n_samples=999)
    refused([(-1, 10, 0.3)]); refused([(0, -1, 0.3)]); refused([(991, 10, 0.3)]); refused([(1001, 0, 0.3)])
    refused([(2 ** 62, 2 ** 31 - 1, 0.3)])
    refused([(0, 10, np.nan)])
    refused(good, skew_iq=4); refused(good, skew_rec=4)
    assert host(lib, iq, mm.make_jobs([good[0]] * mm.MAX_JOBS))[0] == 0
    assert host(lib, iq, mm.make_jobs([(0, 1000, np.inf), (0, 1000, -np.inf), (0, 1000, -1.0)]))[0] == 0
    # the device entry point decides the same on the host, before it touches the instance: no instance, nothing to touch
    assert lib.fosphor_amd_measure(None, iq.ctypes.data, 1000, mm.make_jobs(good).ctypes.data, 3, iq.ctypes.data) == EINVAL
    assert lib.fosphor_amd_measure_stats(None, None) == EINVAL


def test_measure_from_extract(lib, F):
    e = np.zeros(2, mm.EXTRACT_DTYPE)
    e["out_offset"], e["n_out"], e["first"], e["decim"], e["n_taps"] = (7, 1000), (33, 0), (5, 6), 4, 9
    jobs = F.measure_jobs(e, threshold=0.25)
    assert jobs.dtype == mm.JOB_DTYPE and list(jobs["offset"]) == [7, 1000] and list(jobs["n"]) == [33, 0]
    assert np.all(jobs["threshold"] == np.float32(0.25))
    job = gr_fosphor_amd._lib.MeasureJob()
    for bad, thr in ((dict(out_offset=-1), 0.5), (dict(n_out=-1), 0.5), ({}, np.nan)):
        x = e[:1].copy()
        for k, v in bad.items():
            x[k] = v
        assert lib.fosphor_amd_measure_from_extract(x.tobytes(), thr, C.byref(job)) == EINVAL
    assert lib.fosphor_amd_measure_from_extract(None, 0.5, C.byref(job)) == EINVAL
    assert lib.fosphor_amd_measure_from_extract(e[:1].tobytes(), 0.5, None) == EINVAL
    with pytest.raises(ValueError):
        F.measure_jobs(e)						# extract jobs need a threshold
    with pytest.raises(ValueError):
        F.measure_jobs(mm.make_jobs([(0, 1, 0.5)]), threshold=0.5)


def derived(F, iq, thr=0.25, rate=1.0, model=False):
    iq = np.ascontiguousarray(iq, np.float32)
    jobs = mm.make_jobs([(0, len(iq), thr)])
    rec = mm.measure(iq, jobs) if model else F.measure_host(iq, jobs)
    return F.measure_derive(rec, rate)[0]


def pairs(z):
    return np.stack([z.real, z.imag], 1).astype(np.float32)


@pytest.mark.parametrize("model", [True, False])
def test_derive_tone(F, model):
    """a noise-free tone of 64 whole periods in 8000 samples: the lag-1 estimate finds its frequency, the envelope is constant and
    y * y sums to nothing"""
    n, f = 8000, 64 / 8000
    v = derived(F, pairs(0.5 * np.exp(2j * np.pi * (f * np.arange(n) + 0.1))), thr=0.2, rate=1.0, model=model)
    assert abs(v["freq_offset"] - f) <= 1e-6, v
    assert abs(v["kurtosis"] - 1.0) <= 1e-6 and v["circularity"] < 1e-3 and abs(v["coherence"] - (n - 1) / n) <= 1e-6, v
    assert abs(v["mean_db"] - 10 * np.log10(0.25)) <= 1e-5 and abs(v["papr_db"]) <= 1e-5 and v["dc_fraction"] < 1e-6, v
    assert (v["duty"], v["rise"], v["fall"], v["pulses"]) == (1.0, 0.0, float(n), 1)
    # negative offsets, and Hz: the estimate scales with the sample rate
    w = derived(F, pairs(np.exp(-2j * np.pi * 0.125 * np.arange(4096))), rate=48000.0, model=model)
    assert abs(w["freq_offset"] + 6000.0) <= 48000.0 * 1e-6 and w["fall"] == 4096 / 48000.0


def test_derive_real_signal_is_not_circular(F):
    rng = np.random.default_rng(5)
    x = rng.standard_normal(5000)
    v = derived(F, np.stack([x, np.zeros_like(x)], 1))
    assert abs(v["circularity"] - 1.0) <= 2.0 ** -24		# s_zz sums re * re exactly, s_p sums it rounded to float32 (rule 1)
    v = derived(F, pairs(np.exp(0.7j) * np.where(rng.integers(0, 2, 5000) > 0, 1.0, -1.0)))		# BPSK at an angle
    assert abs(v["circularity"] - 1.0) <= 1e-6 and abs(v["kurtosis"] - 1.0) <= 1e-6


def test_derive_gaussian_noise(F):
    """65536 samples of complex Gaussian noise: the kurtosis estimator's standard deviation is sqrt(Var(p^2) / n) / E[p]^2 =
    sqrt(20 / 65536) = 0.0175, so (1.9, 2.1) is about six of them either way"""
    rng = np.random.default_rng(2024)
    iq = np.stack([rng.standard_normal(65536), rng.standard_normal(65536)], 1).astype(np.float32)
    m = derived(F, iq, model=True)
    assert 1.9 < m["kurtosis"] < 2.1, m
    v = derived(F, iq)
    assert 1.9 < v["kurtosis"] < 2.1 and abs(v["kurtosis"] - m["kurtosis"]) <= 1e-9
    assert v["circularity"] < 0.03 and v["coherence"] < 0.03 and v["dc_fraction"] < 1e-3, v
    assert abs(v["mean_power"] - 2.0) < 0.05


def test_derive_two_pulses(F):
    iq = np.zeros((1000, 2), np.float32)
    iq[100:250, 0] = 1.0
    iq[600:700, 1] = -1.0
    v = derived(F, iq, thr=0.5, rate=1000.0)
    assert v["pulses"] == 2 and v["rise"] == 0.1 and v["fall"] == 0.7 and v["duty"] == 0.25
    assert abs(v["papr_db"] - 10 * np.log10(4.0)) <= 1e-9 and v["peak_db"] == 0.0


def test_derive_degenerate_records_are_zeros(lib, F):
    empty = F.measure_host(np.zeros((4, 2), np.float32), mm.make_jobs([(4, 0, 0.5)]))
    silent = F.measure_host(np.zeros((64, 2), np.float32), mm.make_jobs([(0, 64, 0.5)]))
    quiet = F.measure_host(np.full((64, 2), 0.25, np.float32), mm.make_jobs([(0, 64, np.inf)]))
    assert (empty["peak_index"][0], empty["first_above"][0], empty["last_above"][0], empty["n"][0]) == (-1, -1, -1, 0)
    assert not empty.tobytes()[24:88].strip(b"\0")
    for rec in (empty, silent):
        v = F.measure_derive(rec, 1e6)[0]
        assert all(x == 0 for x in v.values()), v
    v = F.measure_derive(quiet, 1e6)[0]
    assert all(np.isfinite(x) for x in v.values()) and (v["duty"], v["rise"], v["fall"], v["pulses"]) == (0, 0, 0, 0)
    assert v["mean_power"] == 0.125 and v["dc_fraction"] == 1.0
    out = gr_fosphor_amd._lib.MeasureValues()
    for rate in (0.0, -1.0, np.inf, np.nan):
        assert lib.fosphor_amd_measure_derive(quiet.tobytes(), rate, C.byref(out)) == EINVAL
    assert lib.fosphor_amd_measure_derive(None, 1.0, C.byref(out)) == EINVAL
    assert lib.fosphor_amd_measure_derive(quiet.tobytes(), 1.0, None) == EINVAL


def test_chain_on_the_host(lib, F):
    """extract_host's float32 output of the chain's stream, then the model and derive: the tone job's lag-1 estimate is within 1e-6
    cycles per output sample of the planted frequency (the GPU test allows the device's float32 extraction 1e-5)"""
    raw, ejobs, planted = mm.chain_case()
    taps = F.extract_design(mm.CHAIN_DECIM, mm.CHAIN_TAPS, 0.8)
    cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
    out = np.zeros((cap, 2), np.float32)
    assert lib.fosphor_amd_extract_host(raw.ctypes.data, len(raw), 2, ejobs.ctypes.data, len(ejobs), taps.ctypes.data, len(taps),
                                        out.ctypes.data, cap) == 0
    jobs = F.measure_jobs(ejobs, threshold=mm.CHAIN_THRESHOLD)
    tone, noise, whole = F.measure_derive(mm.measure(out, jobs), 1.0)
    print("tone %.9f planted %.9f" % (tone["freq_offset"], planted))
    assert abs(tone["freq_offset"] - planted) <= 1e-6
    assert abs(tone["kurtosis"] - 1.0) < 1e-3 and tone["duty"] == 1.0 and tone["pulses"] == 1
    assert 1.7 < noise["kurtosis"] < 2.3 and noise["pulses"] > 10 and 0.2 < noise["duty"] < 0.95
    assert whole["pulses"] == 1 and 0.7 < whole["duty"] < 0.85 and abs(whole["freq_offset"] - planted) < 1e-4
    host_rec = F.measure_host(out, jobs)
    mm.assert_records(host_rec, mm.measure(out, jobs), mm.tolerance((out, jobs)), "chain")
