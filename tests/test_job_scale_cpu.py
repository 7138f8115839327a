"""The conditions on the inputs of tests/test_gpu_job_scale.py and tests/test_gpu_job_far.py, no GPU: the long cases have the
partials, plants and ties their docstrings state, the full tables are full, the bases and aliases of the far buffer lie where they
must; and the long cases and full tables through fosphor_amd_*_host agree with the numpy models as each contract says, so the
reference side alone meets every assertion the GPU tests make.  For psd and symbols also: the tile counts of their long cases, the
cut rule of a FIXED symbols job, the periodic helpers against the whole model and the host twin on blocks short enough to
materialise, and the geometry of the long far jobs."""
import numpy as np
import pytest

import correlate_model as cm
import extract_model as em
import job_scale_cases as jc
import measure_model as mm
import psd_model as pm
import resample_model as rm
import symbols_model as sm
from _pkg import gr_fosphor_amd


@pytest.fixture(scope="module")
def F():
    gr_fosphor_amd.load()
    return gr_fosphor_amd.Fosphor


def part_of(sample):
    return sample // mm.CHUNK


def test_long_measure_plants_and_record():
    case = jc.case_of("long measure")
    jobs, n, cut = case.jobs, jc.LONG_MEASURE_N, jc.LONG_MEASURE_CUT
    chunks = [-(-int(k) // mm.CHUNK) for k in jobs["n"]]
    assert chunks[:5] == [131, 131, 64, 65, 65] and chunks[5] == 131 - 64, "one round, two rounds, three rounds of 64 partials"
    assert jobs["offset"][0] % 2 == 1 and jobs["offset"][1] % 2 == 0 and jobs["n"][3] == cut + 1
    P = jc.LONG_MEASURE_PLANTS
    assert [part_of(P[k][0]) for k in ("top in part 5", "top in part 70", "top in part 129")] == [5, 70, 129]
    first, last, _ = P["run over the round boundary"]
    assert (part_of(first), part_of(last)) == (63, 64) and (first, last) == (cut - 3, cut + 2)
    assert P["rising edge at a part's first sample"][0] == 128 * mm.CHUNK and P["the last sample"][0] == n - 1
    tops = [v[0] for v in P.values() if v[2]]
    y = case.iq[1:1 + n]
    assert len({y[t].tobytes() for t in tops}) == 1, "the maximum is bit-identical where it is planted"
    p = mm.power(y)
    assert sorted(np.flatnonzero(p == p.max())) == sorted(tops)
    want = jc.model_of("long measure").records
    above = sum(v[1] - v[0] + 1 for v in P.values())
    for r in want[:2]:
        assert (r["n_edges"], r["n_above"], r["first_above"], r["last_above"]) == (len(P), above, min(tops), n - 1)
        assert r["peak_index"] == min(tops) and r["form"] == mm.FORM_SPLIT
    assert (want[2]["last_above"], want[2]["n_edges"]) == (cut - 1, 2), "64 parts exactly end inside the run"
    assert (want[5]["first_above"], want[5]["peak_index"]) == (0, tops[1] - cut), "the second half begins inside the run"


def test_long_correlate_plants_and_records():
    T = cm.TILE
    on = jc.long_edges_pattern()
    assert len(on) == jc.LONG_LAGS and -(-len(on) // T) == 131 > 128
    assert on[64 * T - 1] and on[64 * T] and on[128 * T - 1] and on[128 * T], "runs over the seams 63|64 and 127|128"
    assert on[65 * T - 1] and not on[65 * T] and not on[129 * T - 1] and on[129 * T]
    edges = int(on[0]) + int((on[1:] & ~on[:-1]).sum())
    want = jc.model_of("long edges").records
    assert list(want["n_lags"]) == [len(on), len(on), len(on) - 1]
    assert list(want["n_edges"][:2]) == [edges] * 2 and list(want["n_above"][:2]) == [int(on.sum())] * 2
    assert want["n_edges"][2] == edges - 1 and want["last_above"][0] == len(on) - 1, "without lag 0 one edge fewer"

    case = jc.case_of("long tie")
    lags = jc.TIE_LAGS
    assert [k // T for k in lags[:3]] == [3, 67, 70] and lags[3] > jc.LONG_LAGS
    assert (67 - 3) % 64 == 0 and (70 - 3) % 64 != 0, "tiles 3 and 67 meet inside lane 3, tile 70 comes from lane 6"
    second = [k - jc.TIE_SECOND for k in lags[1:]]
    assert [k // T for k in second] == [64, 66, 128] and lags[0] < jc.TIE_SECOND, "the second job's windows: all beyond tile 63"
    for at in lags[1:]:
        assert case.iq[at:at + jc.TIE_T].tobytes() == case.iq[lags[0]:lags[0] + jc.TIE_T].tobytes()
    model = jc.model_of("long tie")
    want = model.records
    assert list(want["peak_lag"]) == [lags[0], lags[0], second[0]], "the smallest lag of the largest rho"
    assert list(want["n_lags"]) == [jc.LONG_LAGS, jc.LONG_LAGS, jc.TIE_SECOND_LAGS]
    rho = model.image[int(case.jobs["out_offset"][0]):][:jc.LONG_LAGS].view(np.float32)
    assert sorted(np.flatnonzero(rho == rho.max())) == list(lags[:3]) and rho.max() == want["peak_rho"][0]


def test_long_resample_positions():
    case = jc.case_of("long resample")
    rows = jc.rs_rows()
    assert {rm.form(jc.RS_UP, D, Q * jc.RS_UP) for _, _, D, Q, _ in rows[:5]} == {"tile"}
    assert {rm.form(jc.RS_UP, D, Q * jc.RS_UP) for _, _, D, Q, _ in rows[5:]} == {"direct"} and len(rows) == 10
    for ph, n_out, D, Q, _ in rows:
        room = (jc.RS_N - Q) * jc.RS_UP
        assert 2 ** 32 < room < 2 ** 32 + 2 ** 14 and ph + (n_out - 1) * D == room, "the last output sits at (n - Q) U"
        assert n_out == rm.max_n_out(jc.RS_N, jc.RS_UP, D, Q * jc.RS_UP, ph)
        first_read = -(-ph // jc.RS_UP)
        assert first_read >= jc.RS_N - jc.RS_TAIL, "only the tail is read"
    crossing = [r for r in rows if r[0] < 2 ** 32]
    assert len(crossing) == 4, "k = 40 and the job of 570 outputs begin below 2^32, in both forms"
    ph, n_out, D, Q, _ = rows[4]
    assert n_out > rm.TILE and ph < 2 ** 32 < ph + rm.TILE * D, "the second tile's m0 * D carries p0 across 2^32"
    assert not case.iq[:jc.RS_N - jc.RS_TAIL].any() and len(case.iq) == jc.RS_N


@pytest.mark.parametrize("name", jc.PASSES)
def test_full_tables_are_full(name):
    case = jc.case_of("full " + name)
    jobs = case.jobs
    assert len(jobs) == jc.MAX_JOBS == jc.MODELS[name].MAX_JOBS
    forms = set(jc.forms(name, jobs))
    assert len(forms) == (1 if name in ("correlate", "psd") else 2), forms	# psd's table is the WAVE form's: the deepest search of one prefix
    work = np.array([jc.has_work(name, j) for j in jobs])
    assert 300 <= (~work).sum() and work.sum() >= 2000
    if name in ("psd", "symbols"):				# the models' own tables: every 11th job of the order they were drawn in
        assert (~work).sum() == len(range(0, jc.MAX_JOBS, 11))
        idle = jobs["n"] < 64 if name == "psd" else jobs["n"] == 0
        assert np.array_equal(idle, ~work)
    ranges = jc.out_ranges(name, jobs)
    assert jc.disjoint(ranges)
    if name not in ("measure", "psd", "symbols"):		# the two models shuffle the jobs' shapes and place the outputs in table order
        starts = [a for a, _ in ranges]
        assert starts != sorted(starts), "outputs out of order"
    for j in jobs:
        assert 0 <= jc.in_span(name, j)[0] <= jc.in_span(name, j)[1] <= len(case.iq)
    one = jc.one_job_of(case)
    records = jc.Model(one).records if name == "symbols" else None		# its counter of symbols is the records' n_sym
    assert len(one.jobs) == 1 and sum(jc.expected_stats(name, one.jobs, records).values()) > 1


@pytest.mark.parametrize("key", ["long measure", "long edges", "long tie", "long resample", "long psd", "long symbols"]
                         + ["full " + k for k in jc.PASSES])
def test_host_twins_meet_the_models(F, key):
    case = jc.case_of(key)
    model = jc.model_of(key)
    if case.name == "extract":
        fmt, raw, jobs, taps = case.model_case()
        x = em.widen(raw, fmt)
        for j, want, tol in zip(jobs, model.outs, model.tols):
            if j["n_out"]:
                got = em.extract_job_f32(x, j, taps)
                assert max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()) <= tol
        return
    rec, words = jc.host_twin(F, case)
    model.check(rec, words, key)
    if key == "long measure":
        jc.assert_long_measure_cut(case, rec, model.tols[0])


def test_long_psd_and_symbols_tiles():
    case = jc.case_of("long psd")
    jobs = case.jobs
    segs = [pm.job_n_seg(j) for j in jobs]
    tiles = [-(-s // pm.TILE) for s in segs]
    assert tiles == [131, 131, 131, 131, 131, 64, 0, 65] and segs[0] % pm.TILE == 5 and segs[5] == 64 * pm.TILE and segs[7] == 64 * pm.TILE + 1
    assert [(int(j["fft_len_log"]), int(j["hop"])) for j in jobs[:3]] == [(6, 1), (8, 3), (10, 7)]
    assert jc.forms("psd", jobs)[:3] == ["wave", "group", "group"]
    assert set(jobs["offset"][:5] % 2) == {0, 1} and jobs["pre"][3] == pm.FOURTH and jobs["trace"][4] == pm.T_NONE
    assert jobs["n"][6] == (1 << int(jobs["fft_len_log"][6])) - 1 and all(jc.in_span("psd", j)[1] <= len(case.iq) for j in jobs)
    w = case.win[int(jobs["win_offset"][2]):][:1024]
    assert w.tobytes() == pm.window(pm.HANN, 10).tobytes()

    case = jc.case_of("long symbols")
    jobs, rec = case.jobs, jc.model_of("long symbols").records
    fold = [-(-(int(j["n"]) // int(j["sps"])) // sm.TILE) if j["mode"] == sm.ESTIMATE else 0 for j in jobs]
    assert fold == [20, 20, 0, 0, 8, 9], "two unrolled bodies of 8 and a remainder of 4; one body exactly; one body and one"
    assert [int(j["n"]) // int(j["sps"]) for j in jobs[[0, 1, 4, 5]]] == [jc.LONG_SYMS, jc.LONG_SYMS, 8 * sm.TILE, 8 * sm.TILE + 1]
    pick = [-(-int(r["n_sym"]) // sm.TILE) for r in rec]
    assert pick == [20, 20, 20, 0, 8, 9] and [-(-sm.job_max_out(j) // sm.TILE) for j in jobs] == [20, 20, 20, 0, 8, 9]
    assert rec["n_sym"][2] == jc.LONG_SYMS and np.all(rec["status"] == sm.OK)
    assert [(int(j["sps"]), int(j["mode"])) for j in jobs[:3]] == [(3, sm.ESTIMATE), (64, sm.ESTIMATE), (2, sm.FIXED)]
    assert jobs["tau"][2] == 0.25 and jobs["n"][3] == 0 and set(jobs["offset"] % 2) == {0, 1}
    assert all(jc.in_span("symbols", j)[1] <= len(case.iq) for j in jobs)


def test_fixed_symbols_obey_the_cut_rule(F):
    case = jc.case_of("long symbols")
    rec, words = jc.host_twin(F, case)
    job, r = case.jobs[2], rec[2]
    at = int(job["out_offset"]) + int(r["n_sym"]) - 64
    want = words[2 * at:2 * (at + 64)]
    tail = jc.advanced_symbols(job, int(r["n_sym"]) - 64)
    tail["out_offset"] = jc.GUARD
    short = jc.Case("symbols", tail, case.iq)
    for trec, twords in (jc.host_twin(F, short), (jc.Model(short).records, jc.Model(short).image)):
        assert trec["n_sym"][0] == 64 and (trec["first"][0], trec["mu"][0]) == (r["first"], r["mu"])
        assert twords[2 * jc.GUARD:2 * (jc.GUARD + 64)].tobytes() == want.tobytes(), "the last 64 symbols do not depend on the cut"


@pytest.mark.parametrize("cycle", [1, 3])
@pytest.mark.parametrize("pre", [pm.NONE, pm.FOURTH])
def test_periodic_psd_is_the_model(F, cycle, pre):
    """a block of `cycle` tile strides (TILE hop samples each) and a job of 5 blocks and a partial tile from an odd offset"""
    log, hop = 6, 5
    stride = pm.TILE * hop
    block = pm.noise(cycle * stride, 11 + cycle)
    win = np.concatenate([np.full(3, 7.0, np.float32), pm.window(pm.HANN, log)])
    segs = 5 * cycle * pm.TILE + 7
    job = pm.make_jobs([(3, jc.GUARD, 3, jc.psd_n_for(segs, log, hop) + 2, log, hop, pre, pm.T_POWER, 0.99, 1e-2)])
    iq = np.tile(block, (6, 1))[:int(job["offset"][0]) + int(job["n"][0])]
    assert pm.job_n_seg(job[0]) == segs and len(iq) > 5 * len(block)
    rec, trace = jc.periodic_psd(block, win, job[0])
    want_rec, want, _ = pm.psd((iq, win, job))
    assert rec.tobytes() == want_rec.tobytes() and trace.tobytes() == want[0].tobytes() and len(trace) == 64
    host_rec, host = F.psd_host(iq, job, win)
    assert rec.tobytes() == host_rec.tobytes() and trace.tobytes() == host[0].tobytes()


@pytest.mark.parametrize("cycle", [1, 3])
@pytest.mark.parametrize("mode,tau", [(sm.ESTIMATE, 0.0), (sm.FIXED, 0.4)])
def test_periodic_symbols_is_the_model(F, cycle, mode, tau):
    """a block of `cycle` tile strides (TILE sps samples each) and a job of 5 blocks and a partial tile from an odd offset"""
    sps = 3
    stride = sm.TILE * sps
    block = sm.noise(cycle * stride, 21 + cycle)
    n = 5 * cycle * stride + 700 * sps + 2
    job = sm.make_jobs([(5, jc.GUARD, n, sps, mode, tau)])
    iq = np.tile(block, (6, 1))[:5 + n]
    assert len(iq) == 5 + n
    rec, head, last = jc.periodic_symbols(block, job[0])
    want_rec, want = sm.symbols((iq, job))
    n_sym = int(want_rec["n_sym"][0])
    assert n_sym // sm.TILE == 5 * cycle and 0 < n_sym % sm.TILE < sm.TILE
    assert rec.tobytes() == want_rec.tobytes()
    assert head.tobytes() == want[0][:cycle * sm.TILE].tobytes() and last.tobytes() == want[0][5 * cycle * sm.TILE:].tobytes()
    host_rec, host = F.symbols_host(iq, job)
    assert rec.tobytes() == host_rec.tobytes()
    got = host[0].view(np.float32).reshape(-1, 2)
    assert head.tobytes() == got[:cycle * sm.TILE].tobytes() and last.tobytes() == got[5 * cycle * sm.TILE:].tobytes()
    whole = got[:5 * cycle * sm.TILE].reshape(5, cycle * sm.TILE, 2)
    assert all(w.tobytes() == head.tobytes() for w in whole), "every period of the output is the first"


def test_long_far_jobs_geometry():
    P = jc.PERIOD
    assert P == 3 * 2 ** 18 and jc.FAR_SAMPLES % P == 0 and 2 ** 31 % P == 2 ** 19 and 2 ** 32 % P == 2 ** 18
    for spec in jc.SYM_LONG.values():
        assert P % (sm.TILE * spec["sps"]) == 0
        assert spec["offset"] % 2 == 1 and spec["n"] == 2 ** 31 - 1 and spec["offset"] + spec["n"] <= jc.FAR_SAMPLES
    assert [s["sps"] for s in jc.SYM_LONG.values()] == [64, 3] and jc.SYM_LONG["sps 3"]["mode"] == sm.FIXED
    for spec in (jc.PSD_LONG, jc.PSD_LONG_PARTS):
        assert P % (pm.TILE * spec["hop"]) == 0 and spec["offset"] == 1 and spec["n"] == 2 ** 31 - 1
        assert spec["offset"] + spec["n"] <= jc.FAR_SAMPLES and spec["fft_len_log"] == 10
    segs = [pm.job_n_seg(jc.long_psd_job(s)[0]) for s in (jc.PSD_LONG, jc.PSD_LONG_PARTS)]
    tiles = [-(-s // pm.TILE) for s in segs]
    assert segs == [2 ** 21 - 1, 2 ** 24 - 8] and tiles == [2 ** 16, 2 ** 19] and all(s % pm.TILE for s in segs), "the last tile is partial"
    # the partials are 2^32 bytes exactly and lie behind the table and the twiddles: the last tile's lie beyond byte 2^32 of the scratch
    assert 8 * tiles[1] * 1024 >= 2 ** 32 and tiles[1] < 2 ** 31 and 8 * tiles[0] * 1024 == 2 ** 29
    # the FIXED job: as many symbols as it reserves, 64 and more tiles, and a tail job that begins beyond sample 2^31
    job = jc.long_symbols_job(jc.SYM_LONG["sps 3"])[0]
    first, mu, n_sym = sm.place_of(np.float64(np.float32(0.4)), int(job["n"]), 3)
    assert n_sym == sm.job_max_out(job) and n_sym % sm.TILE and n_sym // sm.TILE > 64 * 2730
    tail = jc.advanced_symbols(job, n_sym - 64)
    assert tail["offset"][0] > 2 ** 31 and tail["offset"][0] + tail["n"][0] == job["offset"] + job["n"] <= jc.FAR_SAMPLES
    job = jc.long_symbols_job(jc.SYM_LONG["sps 64"])[0]
    assert (int(job["n"]) // 64) // sm.TILE == 2 ** 13 - 1 and (int(job["n"]) // 64) % sm.TILE == sm.TILE - 1
    # the windows' base
    case = jc.case_of("psd tiles")
    assert jc.WIN_BASE == 2 ** 32 + 64 and jc.WIN_BASE % 4 == 0 and jc.WIN_BASE + len(case.win) <= 2 * jc.FAR_SAMPLES
    assert jc.aliases(jc.WIN_BASE, 4) == [64] and 64 + len(case.win) <= jc.WIN_BASE


def test_far_geometry():
    total = {8: jc.FAR_SAMPLES, 4: 2 * jc.FAR_SAMPLES}
    assert jc.FAR_BYTES == 8 * (2 ** 31 + 2 ** 20) and total[4] == 2 ** 32 + 2 ** 21
    assert 8 * jc.BASES_FP32[0] > 2 ** 32 and jc.BASES_FP32[1] > 2 ** 31 and 8 * jc.BASES_FP32[1] > 2 ** 34 and jc.BASES_16[2] > 2 ** 32
    for key in jc.RELOCATE:
        case = jc.case_of(key)
        unit = jc.sample_bytes(case)
        n = len(case.iq)
        assert all(jc.in_span(case.name, j)[1] <= n for j in case.jobs)
        for base in jc.bases_of(case):
            assert base % 16 == 0 and base + n <= total[unit], (key, base)
            found = jc.aliases(base, unit)
            assert found or base * unit < 2 ** 32, "a base beyond byte 2^32 has an alias inside the buffer"
            for a in found:
                assert 0 <= a and a + n <= base, (key, base, a, "a decoy lies inside the buffer and before the case")
        words = jc.OUT_WORDS[case.name]
        if words:
            base, cap = jc.OUT_BASE[words], jc.capacity(case.name, case.jobs)
            unit = 4 * words
            assert base % 16 == 0 and base - jc.FAR_GUARD >= 0 and base + cap + jc.FAR_GUARD <= total[unit]
            assert base > (2 ** 31 if words == 2 else 2 ** 32)
            for a in jc.aliases(base, unit):
                assert a + cap + jc.FAR_GUARD <= base - jc.FAR_GUARD, "the alias's guards lie before the far range's"
    case = jc.case_of("correlate lag_counts")
    assert jc.TPL_BASE % 16 == 0 and jc.TPL_BASE + len(case.tpl) <= jc.FAR_SAMPLES and jc.aliases(jc.TPL_BASE, 8) == [48]


def test_long_extract_jobs():
    """the two long jobs of the far buffer: forms, spans and positions; the hashed stream against a plain loop; the cut rule"""
    w, t = jc.WAVE_LONG, jc.TILE_LONG
    assert em.form(w["decim"], w["n_taps"]) == "wave" and em.form(t["decim"], t["n_taps"]) == "tile"
    assert w["phase_inc"] % 2 == 1 and w["phase0"] > 2 ** 32 - 2 ** 8
    span = em.need(w["n_out"], w["decim"], w["n_taps"])
    assert 2 ** 32 < span and w["first"] + span <= 2 * jc.FAR_SAMPLES
    assert t["n_out"] == -(-2 ** 31 // 25) + 600
    span = em.need(t["n_out"], t["decim"], t["n_taps"])
    assert 2 ** 31 < span and t["first"] + span <= 2 * jc.FAR_SAMPLES
    tiles = -(-t["n_out"] // em.TILE_OUT)
    k = 2 ** 31 // (t["decim"] * em.TILE_OUT)
    assert k * em.TILE_OUT * t["decim"] < 2 ** 31 <= (k + 1) * em.TILE_OUT * t["decim"]
    assert k + 1 == tiles - 2, "the 600 outputs beyond 2^31 / 25: the two tiles from 2^31 on are the last two"
    assert t["n_out"] % em.TILE_OUT not in (0, em.TILE_OUT - 1), "the last tile is short"
    x = jc.HashedStream()
    idx = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5], np.int64)
    for i, v in zip(idx, x[idx]):
        word = ((int(i) * jc.HASH_MUL + (int(i) >> 31) * jc.HASH_HIGH + jc.HASH_ADD) & 0xffffffff)
        word ^= word >> 15
        word = (word * 0x9E5 + (word >> 7)) & 0xffffffff
        re, im = word & 0xffff, word >> 16
        assert v == complex((re - 65536 if re >= 32768 else re) / 32768.0, (im - 65536 if im >= 32768 else im) / 32768.0)
    low = np.arange(0, 2 ** 20, 997, dtype=np.int64)
    for high in (2 ** 31, 2 ** 32):
        assert np.count_nonzero(jc.hash_words(low) == jc.hash_words(low + high)) <= 1, "a truncated index reads other samples"
    taps = em.lowpass(np.random.default_rng(1), 3)
    job = jc.long_extract_job(w, 7)[0]
    tail = jc.advanced(job, w["n_out"] - 64)[0]
    assert tail["n_out"] == 64 and 2 ** 31 < tail["first"] < 2 ** 32 < tail["first"] + 63 * w["decim"], "the short job spans 2^32"
    whole = job.copy()
    whole["n_out"] = 64
    near = em.extract_job(x, jc.advanced(whole, 0)[0], taps)
    assert np.array_equal(em.extract_job(x, jc.advanced(whole, 32)[0], taps), near[32:]), "the model obeys the cut rule"
