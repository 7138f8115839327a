"""The scenario table of tests/persistence_cases.py, checked without a GPU.

Every scenario: the table is consistent (entry points, 16-spectrum multiples, capacity, stream lengths, device / host byte budgets,
the oracle's work within the budgets of both modules).  Then every scenario runs through the oracle alone and the walker's floors
and band population are asserted on the oracle's state: a scenario that stops exercising its transition fails here.  P1, P4s, P5
and P8 run in FULL; P2, P3, P4, P6, P7, P9a/b/c and P10 run in the REDUCED form of persistence_cases.reduced(): the same calls,
batches, segments and constants on an oracle of 2^cpu_log2n columns with the power range shifted so that the same dB bins are
occupied (64 columns for the N = 1024 / 8192 scenarios, 16 for P10, 1024 for P6, 256 for P7 and P9c; row floors scaled with the
rows per bin).  Each run prints which form ran, the transition counts and the population of the band |h - 0.01| < 2e-4 at the
compare points."""
import numpy as np
import pytest

import persistence_cases as pc
from shard_emul import oracle_threads

ENTRY_POINTS = ("process", "process_device", "process_device_overlap", "accumulate", "merge_sliced")


@pytest.mark.parametrize("sid", sorted(pc.SCENARIOS))
def test_scenario_table_is_consistent(sid):
    s = pc.SCENARIOS[sid]
    n = pc.n_of(s)
    assert s["log2n"] in (10, 13, 16) and s["fmt"] in pc.SAMPLE_BYTES and n % s["overlap"] == 0
    assert s["fmt"] != "fp16" or s["log2n"] == 16
    assert s["wf_rows"] & (s["wf_rows"] - 1) == 0 and s["n_bins"] % 16 == 0 and 16 <= s["n_bins"] <= 512
    t0r, t0d, alpha = s["consts"]
    assert 1.0 / t0r + 1.0 / t0d < 1.0 and 0.0 < alpha < 1.0		# 1 - c of display.cl:244-245 stays positive
    assert set(s["env"]) <= set(pc.KNOBS)
    assert s["cpu"] or 4 <= s["cpu_log2n"] < s["log2n"] and (s["log2n"] != 16 or s["cpu_log2n"] >= 6)	# (a row is 64 columns)
    max_spectra, max_batches = pc.capacity(s)
    assert any(c["cmp"] for c in s["calls"]) and s["calls"][-1]["cmp"]
    for c in s["calls"]:
        assert c["ep"] in ENTRY_POINTS
        assert c["batch"] >= 16 and c["batch"] % 16 == 0 and 1 <= c["nb"] <= max_batches and pc.call_spectra(c) <= max_spectra
        if c["ep"] == "process":
            assert c["nb"] == 1 and c["batch"] <= 1024 and s["overlap"] == 1	# cl.c:885-886
        if c["ep"] in ("accumulate", "merge_sliced"):
            assert c["nb"] == 1
        if c["ep"] == "merge_sliced":
            assert s.get("world", 1) > 1 and (s["n_bins"] * n) % s["world"] == 0
        assert (c["ep"] == "process_device_overlap") == (s["overlap"] > 1) or c["ep"] in ("accumulate", "merge_sliced")
        hop = n // s["overlap"]
        assert pc.call_stream_samples(s, c) == (pc.call_spectra(c) - 1) * hop + n
        if c["seg"][0] == "seq":
            assert sum(cnt for cnt, _ in c["seg"][1]) == pc.call_spectra(c), (sid, c["seg"])
    if s.get("world", 1) > 1:
        assert all(c["ep"] == "merge_sliced" for c in s["calls"])
    dev, host = pc.scenario_bytes(s)
    assert dev <= pc.DEVICE_BUDGET, "%s needs %.2f GiB on the device" % (sid, dev / 2 ** 30)
    assert host <= pc.HOST_BUDGET, "%s needs %.2f GiB on the host" % (sid, host / 2 ** 30)
    # the launch shapes the scenario is there for (what merge_stats must then prove on the GPU)
    if "smax" in s:
        lo, hi = s["smax"]
        assert lo <= max(c["nb"] for c in s["calls"] if c["ep"] == "process_device") == hi
    if s["forms"]:
        # one merge launch takes a whole device call only if the call is not cut into sub-launches
        sub = 1 << int(s["env"].get("FOSPHOR_AMD_SUB_LOG2", 30 if s["log2n"] == 13 else 26))
        assert all(c["nb"] == 1 or pc.call_spectra(c) * n <= sub for c in s["calls"] if c["ep"].startswith("process_device"))


def test_oracle_work_fits_the_budgets():
    cpu = sum(pc.oracle_samples(pc.reduced(s)) for s in pc.SCENARIOS.values())
    gpu = sum(pc.oracle_samples(s) for s in pc.SCENARIOS.values()) + pc.RANDOM_SAMPLES
    print("oracle work: %.1f Mi samples in the CPU module, %.1f Mi in the GPU module" % (cpu / 2 ** 20, gpu / 2 ** 20))
    assert cpu <= pc.CPU_BUDGET and gpu <= pc.GPU_BUDGET


def test_segment_builders():
    rng = np.random.default_rng(1)
    n = 1024
    x = pc.build_segment(("seq", [(2, pc.Z), (1, ("const", 0.25)), (1, ("clip",))]), 4 * n, n, rng)
    assert not x[:2 * n].any() and np.all(x[2 * n:3 * n] == 0.25) and np.all(x[3 * n:] == -1.0)
    q, q32 = pc.to_format(x, "sc16")
    assert q.dtype == np.int16 and q[-1] == -32768 and q32[-1, 0] == -1.0 and q32.dtype == np.float32
    # a tone on a bin: all its energy in that FFT output; a burst: in its columns
    t = pc.build_segment(("bintone", 0.5, 37), n, n, rng)
    sp = np.abs(np.fft.fft(t[:, 0] + 1j * t[:, 1]))
    assert sp.argmax() == 37 and np.delete(sp, 37).max() < 1e-6 * sp[37]		# (float32 samples)
    b = pc.build_segment(("burst", 0.1, 100, 200, 0.0), 2 * n, n, rng)
    sp = np.abs(np.fft.fft((b[:, 0] + 1j * b[:, 1]).reshape(2, n), axis=1))
    assert sp[:, 100:200].min() > 0 and np.delete(sp, np.s_[100:200], axis=1).max() < 1e-6 * sp.max()
    h, h32 = pc.to_format(pc.build_segment(pc.B, n, n, rng), "fp16")
    assert h.dtype == np.float16 and np.array_equal(h32, h.astype(np.float32)) and np.count_nonzero(h32) > 0.99 * h32.size


@pytest.mark.parametrize("sid", sorted(pc.SCENARIOS))
def test_scenario_through_the_oracle(oracle_built, sid):
    s = pc.reduced(pc.SCENARIOS[sid])
    print("%s: %s form, %d columns" % (sid, "full" if s is pc.SCENARIOS[sid] else "reduced", pc.n_of(s)))
    w = pc.Walk(s, oracle_threads())
    for idx in range(len(s["calls"])):
        x, x32 = pc.make_call_input(s, idx)
        assert x32.shape == (pc.call_stream_samples(s, s["calls"][idx]), 2) and x32.dtype == np.float32
        assert x.size == 2 * x32.shape[0] and x.dtype.itemsize * 2 == pc.SAMPLE_BYTES[s["fmt"]]
        w.call(idx, x32)
    print(w.report(sid))
    assert w.samples == pc.oracle_samples(s)
    w.assert_floors(sid)
    assert max(w.bands) == s["band"], "%s: band population %d, the table says %s" % (sid, max(w.bands), s["band"])
