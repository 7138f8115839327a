"""Burst IQ extraction (include/fosphor_amd_extract.h), the parts that need no GPU: the numpy model against three plain loops, the
library's host function against the model in all three formats, the filter design and the burst-to-job helper, the -EINVAL table,
the header against its Python mirrors, the compiled kernels' resources, and the float32 emulation that confirms, on every input
set of tests/test_gpu_extract.py, that the tolerance those tests use is one a plain float32 implementation meets."""
import ctypes as C
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import extract_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fosphor_amd_extract.h")
SRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_extract.hip")
EINVAL = -errno.EINVAL
SENTINEL = np.float32(-7.25)


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


@pytest.fixture(scope="module")
def all_cases():
    return em.cases()


def host(amd, fmt, raw, jobs, taps, n_samples=None, n_taps_total=None, cap=None, null=()):
    """fosphor_amd_extract_host into a sentinel-filled buffer -> (return value, [cap] complex64 with the sentinel elsewhere)"""
    raw = np.ascontiguousarray(raw)
    jobs = np.ascontiguousarray(jobs, em.JOB_DTYPE)
    taps = np.ascontiguousarray(taps, np.float32)
    cap = em.capacity(jobs) if cap is None else cap
    out = np.full((max(cap, 1) + em.GUARD, 2), SENTINEL, np.float32)
    rv = amd.load().fosphor_amd_extract_host(None if "x" in null else raw.ctypes.data, len(raw) if n_samples is None else n_samples,
                                             fmt, None if "jobs" in null else jobs.ctypes.data, len(jobs),
                                             None if "taps" in null else taps.ctypes.data,
                                             len(taps) if n_taps_total is None else n_taps_total,
                                             None if "out" in null else out.ctypes.data, cap)
    return rv, out


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def test_model_against_three_loops():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(400) + 1j * rng.standard_normal(400)
    taps = rng.standard_normal(40).astype(np.float32)
    rows = [(0, 7, 1, 1, 0xfffffff0, 0, 1), (5, 9, 1, 0x7fffffff, 3, 1, 33), (2, 11, 4, 0x80000000, 0xffffffff, 3, 3),
            (1, 6, 16, 0xffffffff, 0x80000000, 0, 40), (9, 13, 3, 0x9e3779b9, 12345, 7, 25), (0, 0, 5, 1, 1, 0, 9)]
    for job in em.make_jobs(rows):
        want, got = em.extract_naive(x, job, taps), em.extract_job(x, job, taps)
        assert got.shape == want.shape == (job["n_out"],)
        assert np.all(np.abs(got - want) <= 1e-12), job
    # phi is an integer: it wraps exactly, and a job cut in two continues the phase
    job = em.make_jobs([(0, 1, 1, 0xffffffff, 0xfffffff0, 0, 1)])[0]
    assert em.phases(job, [0, 1, 0x10, 0x11, (1 << 32) + 1]).tolist() == [0xfffffff0, 0xffffffef, 0xffffffe0, 0xffffffdf, 0xffffffef]


@pytest.mark.parametrize("fmt", [em.FP32, em.FP16, em.SC16])
def test_host_function_against_model(amd, fmt):
    """within 1 float32 ulp of the float64 value, per component; sc16 -32768 and float16 subnormals are among the samples"""
    _, raw, jobs, taps = em.simple_case(fmt, 40 + fmt, [(1, 1, 50), (1, 33, 70), (4, 3, 40), (16, 129, 9), (3, 25, 31), (26, 209, 5)],
                                        first=3)
    if fmt == em.SC16:
        assert (raw == -32768).any()
    if fmt == em.FP16:
        tiny = np.abs(raw.astype(np.float64))
        assert ((tiny > 0) & (tiny < 2.0 ** -14)).any()
    rv, out = host(amd, fmt, raw, jobs, taps)
    assert rv == 0
    written = np.zeros(len(out), bool)
    for job, want in zip(jobs, em.extract(raw, fmt, jobs, taps)):
        sl = slice(int(job["out_offset"]), int(job["out_offset"]) + int(job["n_out"]))
        written[sl] = True
        for got, ref in ((out[sl, 0], want.real), (out[sl, 1], want.imag)):
            assert np.all(np.abs(got.astype(np.float64) - ref) <= ulp32(ref)), job
    assert np.all(out[~written] == SENTINEL), "only the jobs' ranges are written"


def test_design_against_formula(amd):
    for decim, n_taps, guard in ((1, 1, 1.0), (1, 9, 0.8), (4, 33, 0.8), (16, 129, 1.0), (3, 24, 0.5), (1024, 8192, 0.9), (64, 513, 0.8)):
        h = amd.Fosphor.extract_design(decim, n_taps, guard)
        want = em.design(decim, n_taps, guard)
        assert h.dtype == np.float32 and h.shape == (n_taps,)
        assert np.all(np.abs(h.astype(np.float64) - want) <= 1e-7), (decim, n_taps)
        assert abs(want.sum() - 1.0) < 1e-12 and abs(h.astype(np.float64).sum() - 1.0) < n_taps * 2.0 ** -25
        assert np.array_equal(h, h[::-1]), "symmetric to the bit"
    h = amd.Fosphor.extract_design(8, 65, 0.8).astype(np.float64)
    resp = np.abs(np.fft.fft(h, 4096))
    assert resp[0] > 0.999 and resp[4096 // 16 + 150:2048].max() < 0.01, "a low-pass: nothing from well behind 1 / (2 D) on"
    L = amd.load()
    buf = np.zeros(16, np.float32)
    for bad in ((0, 9, 0.8), (1025, 9, 0.8), (4, 0, 0.8), (4, 8193, 0.8), (4, 9, 0.0), (4, 9, 1.5), (4, 9, float("nan"))):
        assert L.fosphor_amd_extract_design(bad[0], bad[1], bad[2], buf.ctypes.data) == EINVAL, bad
    assert L.fosphor_amd_extract_design(4, 9, 0.8, None) == EINVAL


def burst(newest, oldest, first_col, last_col):
    return (newest, oldest, first_col, last_col, 1, newest, first_col, 0.0, 0.0, 0)


def from_burst(amd, rec, fft_len=1024, newest_first=255 * 1024, row_hop=1024, max_decim=64, guard=0.8):
    b = amd._lib.Burst(*rec)
    job, taps = amd._lib.ExtractJob(), C.c_int(-1)
    rv = amd.load().fosphor_amd_extract_from_burst(C.byref(b), fft_len, newest_first, row_hop, max_decim, guard, C.byref(job),
                                                   C.byref(taps))
    return rv, job, taps.value


def test_from_burst_by_hand(amd):
    # columns 500 .. 523 straddle N / 2 = 512: centre (500 + 523 + 1) / 2 - 512 = 0, width 24, D = floor(0.8 * 1024 / 24) = 34
    rv, job, taps = from_burst(amd, burst(10, 13, 500, 523))
    assert rv == 0 and job.phase_inc == 0 and job.decim == 34 and taps == job.n_taps == 273
    assert job.first == (255 - 13) * 1024 and job.phase0 == 0 and job.out_offset == 0 and job.taps_offset == 0
    assert job.n_out == (4 * 1024 - 273) // 34 + 1				# (oldest - newest) * hop + N = 4096 samples
    assert (job.n_out - 1) * 34 + 273 <= 4096 < job.n_out * 34 + 273
    # columns 0 .. 3 straddle nothing but touch column 0: centre 2 - 512 = -510 columns, a negative frequency
    rv, job, taps = from_burst(amd, burst(0, 0, 0, 3))
    assert rv == 0 and job.phase_inc == ((-510 << 32) // 1024) % (1 << 32) and job.phase_inc >= 0x80000000
    assert job.decim == 64 and job.first == 255 * 1024 and job.n_out == (1024 - 513) // 64 + 1		# max_decim caps D
    # one column, 700: centre 700.5 - 512 = 188.5 columns
    rv, job, taps = from_burst(amd, burst(2, 2, 700, 700), max_decim=1024)
    assert rv == 0 and job.phase_inc == (377 << 32) // 2048 and job.decim == 819 and taps == 8 * 819 + 1
    assert job.n_out == 0							# 1024 samples are fewer than the taps
    # wider than guard allows at D = 2 (0.8 * 1024 / 2 = 409.6 columns): D = 1
    rv, job, taps = from_burst(amd, burst(0, 1, 100, 509))
    assert rv == 0 and job.decim == 1 and taps == 9 and job.n_out == 2048 - 9 + 1
    rv, job, taps = from_burst(amd, burst(0, 1, 100, 508))
    assert rv == 0 and job.decim == 2
    # the last column: the highest centre there is, 511.5 columns
    rv, job, taps = from_burst(amd, burst(0, 0, 1023, 1023))
    assert rv == 0 and job.phase_inc == (1023 << 32) // 2048
    # first < 0; records that are no burst of that geometry
    assert from_burst(amd, burst(0, 256, 10, 20))[0] == EINVAL
    assert from_burst(amd, burst(0, 255, 10, 20))[0] == 0
    for rec in (burst(-1, 3, 1, 2), burst(4, 3, 1, 2), burst(0, 3, -1, 2), burst(0, 3, 1, 1024), burst(0, 3, 5, 4)):
        assert from_burst(amd, rec)[0] == EINVAL, rec
    for kw in (dict(fft_len=1000), dict(fft_len=1), dict(row_hop=0), dict(max_decim=0), dict(guard=0.0), dict(guard=1.25)):
        assert from_burst(amd, burst(0, 3, 1, 2), **kw)[0] == EINVAL, kw
    # the Python mirror gives the same job
    f_job = np.frombuffer(bytes(from_burst(amd, burst(10, 13, 500, 523))[1]), em.JOB_DTYPE)
    assert f_job["decim"][0] == 34 and f_job["n_taps"][0] == 273


def test_host_einval_table(amd):
    rng = np.random.default_rng(9)
    raw = em.stream(em.FP32, 1000, 9)
    taps = em.lowpass(rng, 40)
    good = [(0, 10, 4, 5, 6, 0, 33), (100, 20, 2, 5, 6, 3, 9)]
    rv, out = host(amd, em.FP32, raw, em.make_jobs(good), taps)
    assert rv == 0

    def refused(rows, fmt=em.FP32, edit=None, **kw):
        jobs = em.make_jobs(rows)
        if edit:
            edit(jobs)
        rv, out = host(amd, fmt, raw, jobs, taps, **kw)
        assert rv == EINVAL, (rows, kw)
        assert np.all(out == SENTINEL), "nothing is written"

    refused(good, fmt=-1)
    refused(good, fmt=3)
    refused(good, null=("x",)); refused(good, null=("jobs",)); refused(good, null=("taps",)); refused(good, null=("out",))
    refused([good[0]] * 4097)
    refused([(-1, 10, 4, 5, 6, 0, 33)])					# first < 0
    refused([(0, -1, 4, 5, 6, 0, 33)])					# n_out < 0
    refused([(0, 10, 0, 5, 6, 0, 33)]); refused([(0, 10, 1025, 5, 6, 0, 33)])	# decim
    refused([(0, 10, 4, 5, 6, 0, 0)]); refused([(0, 1, 1, 5, 6, 0, 8193)])	# n_taps
    refused([(0, 10, 4, 5, 6, -1, 33)]); refused([(0, 10, 4, 5, 6, 8, 33)])	# taps outside [0, 40)
    refused([(0, 10, 4, 5, 6, 0, 33)], n_taps_total=32)
    refused([(1000 - 68, 10, 4, 5, 6, 0, 33)])				# reads one sample past the end: 9 * 4 + 33 = 69
    refused([(1001, 1, 1, 5, 6, 0, 1)])
    refused(good, n_samples=100 + 19 * 2 + 9 - 1)
    refused(good, cap=em.capacity(em.make_jobs(good)) - em.GUARD - 1)	# the last output lies outside
    refused(good, edit=lambda j: j["out_offset"].__setitem__(0, -1))
    refused(good, edit=lambda j: j["out_offset"].__setitem__(1, j["out_offset"][0] + 9))	# overlaps by one output
    rv, _ = host(amd, em.FP32, raw, em.make_jobs([(1000 - 69, 10, 4, 5, 6, 0, 33)]), taps)	# the last job that fits
    assert rv == 0
    jobs = em.make_jobs(good)
    jobs["out_offset"][1] = jobs["out_offset"][0] + 10				# adjacent ranges are fine
    assert host(amd, em.FP32, raw, jobs, taps)[0] == 0
    jobs = em.make_jobs([(0, 10, 4, 5, 6, 0, 33), (2000, 0, 4, 5, 6, 0, 33)])	# a job that writes nothing reads nothing
    jobs["out_offset"][1] = jobs["out_offset"][0] + 5
    assert host(amd, em.FP32, raw, jobs, taps)[0] == 0


def test_device_entries_refuse_null_without_a_device(amd):
    L = amd.load()
    job = amd._lib.ExtractJob(0, 0, 1, 1, 0, 0, 0, 1)
    assert L.fosphor_amd_extract(None, 8, 16, 0, C.byref(job), 1, 8, 1, 8, 1) == EINVAL
    assert L.fosphor_amd_extract_stats(None, None) == EINVAL


def test_header_matches_python(amd):
    text = open(HEADER).read()
    F, lib = amd.Fosphor, amd._lib
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(FOSPHOR_AMD_\w+)\s+(\d+)u?\b", text)}
    assert F.EXTRACT_MAX_JOBS == em.MAX_JOBS == defs["FOSPHOR_AMD_EXTRACT_MAX_JOBS"] == 4096
    assert F.EXTRACT_MAX_DECIM == em.MAX_DECIM == defs["FOSPHOR_AMD_EXTRACT_MAX_DECIM"] == 1024
    assert F.EXTRACT_MAX_TAPS == em.MAX_TAPS == defs["FOSPHOR_AMD_EXTRACT_MAX_TAPS"] == 8192
    assert F.EXTRACT_TILE_OUT == em.TILE_OUT == defs["FOSPHOR_AMD_EXTRACT_TILE_OUT"]
    assert F.EXTRACT_TILE_LDS == em.TILE_LDS == defs["FOSPHOR_AMD_EXTRACT_TILE_LDS"]
    assert F.EXTRACT_WAVE_OUT == em.WAVE_OUT == defs["FOSPHOR_AMD_EXTRACT_WAVE_OUT"]
    for d, t in ((1, 1), (16, 129), (25, 201), (26, 209), (1024, 8192), (4, 8192), (25, 8192)):
        assert F.extract_form(d, t) == em.form(d, t)
    assert em.tile_edge() == (25, 26)
    m = re.search(r"enum\s*\{([^}]*FOSPHOR_AMD_EXTRACT_STATS[^}]*)\}", text)
    names = [s.strip() for s in m.group(1).split(",") if s.strip()]
    assert names == ["FOSPHOR_AMD_EXTRACT_" + k.upper() for k in F.EXTRACT_STATS] + ["FOSPHOR_AMD_EXTRACT_STATS"]
    assert F.EXTRACT_STATS == em.STATS
    assert lib.SIGNATURES["fosphor_amd_extract_stats"][1][1]._type_._length_ == len(F.EXTRACT_STATS)
    body = re.split(r"struct fosphor_amd_extract_job\b[^{;()]*\{", text)[1].split("};")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip().split()[-1] for d in body.split(";") if d.strip()]
    assert [n for n, _ in lib.ExtractJob._fields_] == fields == list(em.JOB_DTYPE.names) == list(F.EXTRACT_DTYPE.names)
    assert C.sizeof(lib.ExtractJob) == em.JOB_DTYPE.itemsize == 40 and F.EXTRACT_DTYPE == em.JOB_DTYPE
    for name in em.JOB_DTYPE.names:
        assert em.JOB_DTYPE.fields[name][1] == getattr(lib.ExtractJob, name).offset, name


def test_symbols_exported_and_bound(amd):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fosphor_amd_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["fosphor_amd_extract", "fosphor_amd_extract_design", "fosphor_amd_extract_from_burst",
                        "fosphor_amd_extract_host", "fosphor_amd_extract_stats"]
    lib = C.CDLL(amd.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
        assert name in amd._lib.SIGNATURES, name
    for name in ("extract", "extract_design", "extract_from_burst", "extract_stats", "EXTRACT_DTYPE"):
        assert hasattr(amd.Fosphor, name), name


def test_extract_kernels_do_not_spill():
    """-Rpass-analysis=kernel-resource-usage: every kernel of fosphor_extract.hip (two forms x three formats) has 0 bytes of
    scratch, at most 64 VGPRs, and a static LDS image of at most 64 KiB"""
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
    ours = {k: v for k, v in found.items() if re.search(r"k_extract_(tile|wave)", k)}
    assert len(ours) == 6, sorted(found)
    for name, res in ours.items():
        assert res.get("ScratchSize") == 0, (name, res)
        assert res.get("VGPRs", 0) <= 64, (name, res)
        assert res.get("LDS Size", 1 << 30) <= 65536, (name, res)
        if "tile" in name:
            assert res["LDS Size"] == 8 * em.TILE_LDS, (name, res)


def test_float32_emulation_stays_inside_the_gpu_tolerance(all_cases):
    """every input set of the GPU tests: a plain float32 implementation (mixer rounded to float32, sequential fmaf sum) is within
    (T + 16) * 2^-24 * sum|h| * max|x| of the float64 model, per component -- the bound is derived in the issue, this shows that
    it is not tighter than float32 allows"""
    worst = 0.0
    for name, (fmt, raw, jobs, taps) in all_cases.items():
        x = em.widen(raw, fmt)
        for job in jobs:
            if job["n_out"] == 0:
                continue
            want, got, tol = em.extract_job(x, job, taps), em.extract_job_f32(x, job, taps), em.bound(x, job, taps)
            err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
            assert err <= tol, (name, job, err, tol)
            worst = max(worst, err / tol)
    assert 0.0 < worst < 1.0
