"""The persistence merge fed signals that appear, move and vanish (the scenario table in tests/persistence_cases.py).

Every scenario: a HIP instance and the oracle take the same calls.  After every call the table marks as a compare point: ring
position, hit counts bit for bit, every column's counts summing to the batch, waterfall / live / max-hold (assert_close) and the
histogram (assert_hist_close), both helpers as test_gpu_parity has them.  The walker of persistence_cases counts the transitions on
the oracle's state alone and its floors are asserted here at full size (the CPU module walks the reduced forms).  At the end
fosphor_amd_merge_stats must show the merge form(s) the scenario is there for and none other, so that no scenario passes on
another branch than its own.  At N = 65536 the number of rows every compared sparse launch listed must be the number the oracle's
state says are alive: a hot flag that is never cleared changes no result, only this.  The scenarios with a sparse form (P5-P8,
P9c) run a second time with FOSPHOR_AMD_ROWMASK=0: the dense form applies the same per-cell arithmetic in the same order and must
leave identical bits in every buffer at every compare point."""
import numpy as np
import pytest

import persistence_cases as pc
from oracle_lib import Oracle, digest
from shard_emul import oracle_threads
from test_gpu_parity import amd, torch_cuda, assert_close, assert_hist_close, compare_state, overlap_cc_reference	# noqa: F401

pytestmark = pytest.mark.gpu

FORMS = ("dense16", "dense16_long4", "dense16_long", "table32", "eval32", "sparse16", "sparse16_long")
DENSE_TWIN = {"sparse16": "dense16", "sparse16_long": "dense16_long4"}	# what FOSPHOR_AMD_ROWMASK=0 runs instead (<= 4 long batches)


def _set_env(monkeypatch, s, rowmask_off=False):
    for k in pc.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in s["env"].items():
        monkeypatch.setenv(k, v)
    if rowmask_off:
        monkeypatch.setenv("FOSPHOR_AMD_ROWMASK", "0")


def _make(amd, s):
    max_spectra, max_batches = pc.capacity(s)
    t0r, t0d, alpha = s["consts"]
    f = amd.Fosphor(fft_len_log=s["log2n"], n_bins=s["n_bins"], wf_rows=s["wf_rows"], t0r=t0r, t0d=t0d, alpha=alpha,
                    max_spectra=max_spectra, max_batches=max_batches, iq_format=s["fmt"])
    f.set_power_range(*s["power"])
    return f


def _issue(torch, ranks, s, c, x, keep):
    """one call of the table on the instance (on every rank of a sliced scenario)"""
    f = ranks[0]
    if c["ep"] == "process":
        assert f.process(x) == 0
        return
    d = torch.from_numpy(x).cuda()
    keep.append(d)
    torch.cuda.synchronize()
    if c["ep"] == "process_device":
        assert f.process_device(d, c["nb"], c["batch"]) == 0
    elif c["ep"] == "process_device_overlap":
        assert f.process_device_overlap(d, c["nb"], c["batch"], s["overlap"]) == 0
    elif c["ep"] == "accumulate":
        assert f.accumulate_device(d, c["batch"], 0, c["batch"], overlap=s["overlap"]) == 0
        assert f.merge(c["batch"]) == 0
    else:
        for r, fr in enumerate(ranks):
            assert fr.accumulate_device(d, c["batch"], 0, c["batch"], overlap=s["overlap"]) == 0
            assert fr.merge_sliced(c["batch"], len(ranks), r) == 0


def _histogram(ranks):
    """the instance's histogram; of a sliced scenario, what the all-gather of the ranks' slices would hold"""
    if len(ranks) == 1:
        return ranks[0].histogram
    hs = [fr.histogram for fr in ranks]
    per = hs[0].size // len(ranks)
    return np.concatenate([h.reshape(-1)[r * per:(r + 1) * per] for r, h in enumerate(hs)]).reshape(hs[0].shape)


def _compare(ranks, o, c, what):
    for fr in ranks:
        assert fr.finish() >= 0
        assert fr.waterfall_pos == o.waterfall_pos, what + ": ring position"
        hc_gpu, hc_ref = fr.hitcount, o.hitcount.T
        assert np.array_equal(hc_gpu, hc_ref), "%s: hit counts differ in %d cells" % (what, (hc_gpu != hc_ref).sum())
        assert np.all(hc_gpu.sum(0, dtype=np.int64) == c["batch"]), what + ": a column's counts do not sum to the batch"
        assert_close(fr.waterfall, o.waterfall, what + " waterfall")
        sp_g, sp_o = fr.spectrum, o.spectrum
        assert_close(sp_g[0, :, 1], sp_o[0, :, 1], what + " live")
        assert_close(sp_g[1, :, 1], sp_o[1, :, 1], what + " max-hold")
    assert_hist_close(_histogram(ranks), o.histogram, what + " histogram")


def _digests(fr):
    """every buffer of the instance (floats by their bits, NaNs canonical)"""
    assert fr.finish() >= 0
    return {"hit counts": digest(fr.hitcount), "histogram": digest(fr.histogram), "waterfall": digest(fr.waterfall),
            "spectrum": digest(fr.spectrum), "ring position": fr.waterfall_pos}


def _assert_listed_rows(s, f, w, idx, sid):
    """the sparse merge of call idx listed exactly the rows the oracle says are alive -- hot before the call or hit in it -- or,
    when its flags had to be rebuilt (first launch, or the call before took another form), every row"""
    c = s["calls"][idx]
    if s["log2n"] != 16 or c["ep"] != "process_device":
        return
    flags_valid = idx > 0 and s["calls"][idx - 1]["ep"] == "process_device"
    want = w.alive_rows if flags_valid else s["n_bins"] * (pc.n_of(s) // 64)
    got = f.merge_stats()["sparse_listed_rows"]
    assert got == want, "%s call %d: the sparse merge listed %d rows, %d are alive (flags %s)" % (
        sid, idx, got, want, "valid" if flags_valid else "rebuilt")


def _assert_forms(s, st, sid, rowmask_off=False):
    want = {DENSE_TWIN.get(k, k) for k in s["forms"]} if rowmask_off else set(s["forms"])
    for k in FORMS:
        assert (st[k] > 0) == (k in want), "%s: merge form %s launched %d times, wanted %s (%s)" % (sid, k, st[k], sorted(want), st)
    if rowmask_off:
        return
    long_launches = st["dense16_long4"] + st["dense16_long"] + st["sparse16_long"]
    if "mem" in s:
        assert st["table_in_memory"] == (long_launches if s["mem"] == "all" else 0), "%s: %s" % (sid, st)
    if "smax" in s:
        got = st["sparse_long_max_batches"] if "sparse16_long" in s["forms"] else st["sparse_max_batches"]
        assert s["smax"][0] <= got == s["smax"][1], "%s: the largest sparse launch merged %d batches (%s)" % (sid, got, st)


@pytest.mark.parametrize("sid", sorted(pc.SCENARIOS))
def test_persistence_scenario(amd, torch_cuda, oracle_built, monkeypatch, sid):
    torch = torch_cuda
    s = pc.SCENARIOS[sid]
    _set_env(monkeypatch, s)
    ranks = [_make(amd, s) for _ in range(s.get("world", 1))]
    w = pc.Walk(s, oracle_threads())
    for fr in ranks:
        assert fr.histo_scale == w.o.histo_scale and fr.histo_offset == w.o.histo_offset
    keep, first = [], []
    for idx, c in enumerate(s["calls"]):
        x, x32 = pc.make_call_input(s, idx)
        _issue(torch, ranks, s, c, x, keep)
        w.call(idx, x32)
        del x32
        if c["cmp"]:
            _compare(ranks, w.o, c, "%s call %d (%s, %d x %d, %s)" % (sid, idx, c["ep"], c["nb"], c["batch"], c["seg"][0]))
            _assert_listed_rows(s, ranks[0], w, idx, sid)
            first.append(_digests(ranks[0]))
            del keep[:]
    print(w.report(sid))
    w.assert_floors(sid)
    assert max(w.bands) == s["band"], "%s: band population %d, the table says %s" % (sid, max(w.bands), s["band"])
    stats = [fr.merge_stats() for fr in ranks]
    print("%s: merge_stats %s" % (sid, stats[0]))
    for st in stats:
        _assert_forms(s, st, sid)
    for fr in ranks:
        fr.close()
    if s["forms"] and s["forms"] & set(DENSE_TWIN):
        # the same calls through the dense form: identical bits in every buffer at every compare point
        _set_env(monkeypatch, s, rowmask_off=True)
        twin = [_make(amd, s)]
        at = 0
        for idx, c in enumerate(s["calls"]):
            x, _ = pc.make_call_input(s, idx)
            _issue(torch, twin, s, c, x, keep)
            if c["cmp"]:
                for name, b in _digests(twin[0]).items():
                    assert first[at][name] == b, "%s call %d: %s differs between the sparse and the dense form" % (sid, idx, name)
                at += 1
                del keep[:]
        assert at == len(first)
        st = twin[0].merge_stats()
        _assert_forms(s, st, sid, rowmask_off=True)
        assert st["sparse_listed_rows"] == -1
        twin[0].close()


def test_merge_stats_arguments(amd, torch_cuda):
    import errno
    L = amd.load()
    f = amd.Fosphor(max_spectra=16)
    st = f.merge_stats()
    assert st.pop("sparse_listed_rows") == -1 and set(st.values()) == {0}		# nothing launched yet
    assert L.fosphor_amd_merge_stats(f.h, None) == 0
    assert L.fosphor_amd_merge_stats(None, None) == -errno.EINVAL
    d = torch_cuda.zeros((16 * 1024, 2), dtype=torch_cuda.float32, device="cuda")
    assert f.process_device(d, 1, 16) == 0 and f.finish() >= 0
    st = f.merge_stats()
    assert st.pop("sparse_listed_rows") == -1 and st["dense16"] == 1 and sum(st.values()) == 1
    f.close()


RANDOM_LIMIT = {(13, 1): 14, (13, 2): 11, (16, 1): 27, (16, 2): 36}	# Mi samples a sequence may put through the oracle
assert sum(RANDOM_LIMIT.values()) << 20 <= pc.RANDOM_SAMPLES
SEGMENTS = [pc.A, pc.B, pc.M, pc.Z, ("tone", pc.HI, 0.123, pc.LO), ("const", 0.25), ("clip",), "burst"]


@pytest.mark.parametrize("log2n,seed", [(13, 1), (13, 2), (16, 1), (16, 2)])
def test_random_call_sequences_long(amd, torch_cuda, oracle_built, monkeypatch, log2n, seed):
    """test_random_call_sequences (test_gpu_parity) at N = 8192 and N = 65536: random mixes of fosphor_process, device calls of 1..6
    (N = 65536: 1..4) batches, fused-overlap calls and sharded frames held by one rank, with fast constants (a cell is below 0.01 two silent batches
    after its plateau) and the level of every step drawn from the primitives of persistence_cases, against the oracle fed the same
    spectra in the same order."""
    torch = torch_cuda
    for k in pc.KNOBS:
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(9500 + 10 * log2n + seed)
    n = 1 << log2n
    fmt = "fp16" if log2n == 16 else "fp32"
    consts = (2.0, 4.0, 0.01)
    f = amd.Fosphor(fft_len_log=log2n, n_bins=128, wf_rows=64, t0r=consts[0], t0d=consts[1], alpha=consts[2], max_spectra=768,
                    max_batches=8, iq_format=fmt)
    o = Oracle(fft_len_log=log2n, n_bins=128, wf_rows=64)
    o.set_constants(*consts)
    keep, samples = [], 0
    for step in range(12):
        kind = int(rng.integers(0, 5))
        seg = SEGMENTS[int(rng.integers(0, len(SEGMENTS)))]
        if seg == "burst":
            seg = ("burst", pc.HI, n // 8, n // 4, pc.LO)
        over = int(rng.choice([2, 4])) if kind == 3 else 1
        nb = 1 if kind in (0, 4) else int(rng.integers(1, 5 if log2n == 16 else 7))
        b = int(rng.choice([16, 32] if log2n == 16 else [16, 48, 128]))
        data = np.random.default_rng(95000 + 1000 * log2n + 100 * seed + step)	# (the choices do not depend on how much data a step draws)
        x = pc.build_segment(seg, (nb * b - 1) * (n // over) + n, n, data, t0=step * 4099)
        x, x32 = pc.to_format(x, fmt)
        if kind == 0:
            assert f.process(x) == 0
        else:
            keep.append(torch.from_numpy(x).cuda()); torch.cuda.synchronize()
            if kind in (1, 2):
                assert f.process_device(keep[-1], nb, b) == 0
            elif kind == 3:
                assert f.process_device_overlap(keep[-1], nb, b, over) == 0
            else:
                assert f.accumulate_device(keep[-1], b, 0, b) == 0 and f.merge(b) == 0
        ex = x32 if over == 1 else overlap_cc_reference(x32, n, over)
        for k in range(nb):
            assert o.process(ex[k * b * n:(k + 1) * b * n], strict=False, nthreads=oracle_threads()) == 0
        samples += nb * b * n
        if rng.integers(0, 3) == 0:
            assert f.draw() == o.waterfall_pos
            compare_state(f, o, "N %d seed %d step %d (kind %d, %s)" % (n, seed, step, kind, seg[0]))
    compare_state(f, o, "N %d seed %d, end" % (n, seed))
    st = f.merge_stats()
    print("N %d seed %d: %.1f Mi samples, merge_stats %s" % (n, seed, samples / 2 ** 20, st))
    assert samples <= RANDOM_LIMIT[(log2n, seed)] << 20
    f.close()
