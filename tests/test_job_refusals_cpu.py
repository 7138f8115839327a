"""The refusals that the passes over burst IQ share (gr-fosphor_amd/csrc/fosphor_jobs.h), asked of all four host twins with the same
malformed tables: fosphor_amd_extract_host, _measure_host, _demod_host and _correlate_host.  No GPU.

Every pass is driven with its plainest job, so that a job of n samples at `offset` writes n outputs at `out_offset`: extract with
one tap of 1.0 and no decimation, demod in power mode without averaging, correlate against a one-sample template with a rho trace;
measure writes a record per job and has no output range.  The calls go to the C entry points of the library that the package loads,
with the package's job and record types, because n_samples and the capacity are the arguments under test and the Python wrappers
derive both from their inputs; the accepted tables also go through the wrappers where the package has one (extract has none)."""
import errno

import numpy as np
import pytest

EINVAL = -errno.EINVAL
N = 64					# samples of the stream
PASSES = ("extract", "measure", "demod", "correlate")
WITH_OUTPUTS = ("extract", "demod", "correlate")


@pytest.fixture(scope="module")
def amd():
    import os
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


@pytest.fixture(scope="module")
def iq():
    rng = np.random.default_rng(16)
    return rng.standard_normal((N, 2)).astype(np.float32)


class Pass:
    """one pass: rows of (offset, n, out_offset) -> its jobs, and the call of its host twin"""

    def __init__(self, amd, name, iq):
        self.F, self.L, self.name, self.iq = amd.Fosphor, amd.load(), name, iq
        self.max_jobs = getattr(self.F, name.upper() + "_MAX_JOBS")
        self.one = np.array([1.0, 0.0], np.float32)		# extract's tap (its first float) and correlate's template 1 + 0j

    def jobs(self, rows):
        F = self.F
        if self.name == "extract":
            return np.array([(o, at, n, 1, 0, 0, 0, 1) for o, n, at in rows], F.EXTRACT_DTYPE)
        if self.name == "measure":
            return np.array([(o, n, 0.5) for o, n, at in rows], F.MEASURE_JOB_DTYPE)
        if self.name == "demod":
            return np.array([(o, at, n, F.DEMOD_MODES["power"], 1, 0) for o, n, at in rows], F.DEMOD_JOB_DTYPE)
        return np.array([(o, at, 0, n, 1, F.CORRELATE_TRACES["rho"], 0.5) for o, n, at in rows], F.CORRELATE_JOB_DTYPE)

    def call(self, rows, n_samples=N, cap=None, n_jobs=None):
        """-> (return value, per job the bytes of what it wrote: its outputs, and its record where the pass has records)"""
        jobs = self.jobs(rows)
        n_jobs = len(jobs) if n_jobs is None else n_jobs
        need = max([at + n for o, n, at in rows] + [0])
        cap = need if cap is None else cap
        width = 2 if self.name == "extract" else 1
        out = np.zeros(max(need, cap, 1) * width, np.float32)
        iq, jp, L = self.iq.ctypes.data, jobs.ctypes.data, self.L
        if self.name == "extract":
            rv = L.fosphor_amd_extract_host(iq, n_samples, 0, jp, n_jobs, self.one.ctypes.data, 1, out.ctypes.data, cap)
            records = None
        elif self.name == "measure":
            records = np.zeros(max(len(jobs), 1), self.F.MEASURE_RECORD_DTYPE)
            rv = L.fosphor_amd_measure_host(iq, n_samples, jp, n_jobs, records.ctypes.data)
        elif self.name == "demod":
            rv = L.fosphor_amd_demod_host(iq, n_samples, jp, n_jobs, out.ctypes.data, cap)
            records = None
        else:
            records = np.zeros(max(len(jobs), 1), self.F.CORRELATE_RECORD_DTYPE)
            rv = L.fosphor_amd_correlate_host(iq, n_samples, self.one.ctypes.data, 1, jp, n_jobs, records.ctypes.data,
                                              out.ctypes.data, cap)
        wrote = []
        for k, (o, n, at) in enumerate(rows):
            b = out[at * width:(at + n) * width].tobytes() if self.name != "measure" else b""
            wrote.append(b + (records[k].tobytes() if records is not None else b""))
        return rv, wrote

    def wrapper(self, rows):
        """the same jobs through the package's Python wrapper -> per job the bytes of what it wrote, or None without a wrapper"""
        jobs = self.jobs(rows)
        if self.name == "measure":
            return [r.tobytes() for r in self.F.measure_host(self.iq, jobs)]
        if self.name == "demod":
            return [v.tobytes() for v in self.F.demod_host(self.iq, jobs)]
        if self.name == "correlate":
            records, views = self.F.correlate_host(self.iq, jobs, self.one)
            return [v.tobytes() + r.tobytes() for v, r in zip(views, records)]
        return None


@pytest.fixture(scope="module", params=PASSES)
def any_pass(request, amd, iq):
    return Pass(amd, request.param, iq)


@pytest.fixture(scope="module", params=WITH_OUTPUTS)
def out_pass(request, amd, iq):
    return Pass(amd, request.param, iq)


def accepted(p, rows, **kw):
    rv, wrote = p.call(rows, **kw)
    assert rv == 0, (p.name, rows, kw)
    return wrote


def refused(p, rows, **kw):
    assert p.call(rows, **kw)[0] == EINVAL, (p.name, rows, kw)


def test_job_count(any_pass):
    p = any_pass
    row = (3, 5, 0)
    accepted(p, [row])
    refused(p, [row], n_jobs=0)
    refused(p, [(0, 1, k) for k in range(p.max_jobs + 1)])


def test_sample_range(any_pass):
    p = any_pass
    refused(p, [(-1, 5, 0)])
    accepted(p, [(N - 5, 5, 0)])			# ends on the last sample
    refused(p, [(N - 5, 6, 0)])				# one past it
    refused(p, [(N - 5, 5, 0)], n_samples=N - 1)


def test_output_range(out_pass):
    p = out_pass
    accepted(p, [(0, 5, 7)], cap=12)			# ends on the last element
    refused(p, [(0, 5, 7)], cap=11)			# one past it
    refused(p, [(0, 5, 8)], cap=12)


def test_overlap_and_touch(out_pass):
    p = out_pass
    a, b = (1, 10, 0), (20, 9, 10)
    refused(p, [a, (20, 9, 9)])				# [0, 10) and [9, 18): one element shared
    refused(p, [(20, 9, 9), a])				# the same, given in descending order
    both = accepted(p, [a, b])				# [0, 10) and [10, 19) touch
    assert both == accepted(p, [a]) + accepted(p, [b]), "touching jobs give what each gives alone"
    assert both == accepted(p, [b, a])[::-1]
    w = p.wrapper([a, b])
    assert w is None or w == both


def test_largest_table(any_pass):
    """MAX_JOBS jobs of one sample -- one output, one lag -- are accepted, and a job among them gives what it gives alone"""
    p = any_pass
    rows = [(k % N, 1, k) for k in range(p.max_jobs)]
    wrote = accepted(p, rows)
    for k in (0, 1, N - 1, p.max_jobs - 1):
        o, n, at = rows[k]
        assert wrote[k] == accepted(p, [(o, n, 0)])[0], k
    w = p.wrapper(rows)
    assert w is None or w == wrote
