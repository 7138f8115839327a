"""The conditions on the inputs of tests/test_gpu_job_scale.py and tests/test_gpu_job_far.py, no GPU: the long cases have the
partials, plants and ties their docstrings state, the full tables are full, the bases and aliases of the far buffer lie where they
must; and the long cases and full tables through fosphor_amd_*_host agree with the numpy models as each contract says, so the
reference side alone meets every assertion the GPU tests make.  For psd and symbols also: the tile counts of their long cases, the
cut rule of a FIXED symbols job, the periodic helpers against the whole model and the host twin on blocks short enough to
materialise, and the geometry of the long far jobs.  For carrier and decide: the tile and group counts of their long cases, where
the plants of "long decide words" lie and which of them rule 4 picks, the exactness that makes a carrier job with dyadic frequency
and phase periodic, and periodic_carrier and periodic_decide against the whole models on jobs shaped like the five long far ones."""
import numpy as np
import pytest

import carrier_model as car
import correlate_model as cm
import decide_model as dec
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
    if name in ("psd", "symbols", "carrier", "decide"):	# the models' own tables: every 11th job of the order they were drawn in
        assert (~work).sum() == len(range(0, jc.MAX_JOBS, 11))
        idle = jobs["n"] < 64 if name == "psd" else jobs["n"] == 0
        assert np.array_equal(idle, ~work)
    ranges = jc.out_ranges(name, jobs)
    assert jc.disjoint(ranges)
    if name not in ("measure", "psd", "symbols", "carrier", "decide"):	# the models shuffle the jobs' shapes and place the outputs in table order
        starts = [a for a, _ in ranges]
        assert starts != sorted(starts), "outputs out of order"
    for j in jobs:
        assert 0 <= jc.in_span(name, j)[0] <= jc.in_span(name, j)[1] <= len(case.iq)
    one = jc.one_job_of(case)
    records = jc.Model(one).records if name == "symbols" else None		# its counter of symbols is the records' n_sym
    assert len(one.jobs) == 1 and sum(jc.expected_stats(name, one.jobs, records).values()) > 1


@pytest.mark.parametrize("key", ["long measure", "long edges", "long tie", "long resample", "long psd", "long symbols", "long carrier",
                                 "long decide", "long decide words"] + ["full " + k for k in jc.PASSES])
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


def test_long_carrier_and_decide_tiles():
    T = car.TILE
    jobs, rec = jc.case_of("long carrier").jobs, jc.model_of("long carrier").records
    n = [int(v) for v in jobs["n"]]
    assert n == [jc.LONG_CAR] * 12 + [0, 8 * T, 8 * T + 1, 8 * T + 2] and jc.LONG_CAR == 19 * T + 5
    est = (jobs["mode"] & car.FREQ_FIXED) == 0
    sum_tiles = [-(-k // T) for k in n]
    lag_tiles = [-(-max(k - 1, 0) // T) if e else 0 for k, e in zip(n, est)]
    assert sum_tiles == [20] * 12 + [0, 8, 9, 9], "two unrolled bodies of 8 and a remainder of 4; none; one body; one body and one"
    assert lag_tiles == [20] * 9 + [0, 20, 0, 0, 8, 8, 9], "k_car_freq and k_car_phase differ at 8 TILE + 1"
    assert [(int(j["order"]), int(j["lag"])) for j in jobs[:9]] == [(M, L) for M in car.ORDERS for L in (1, 16, 64)]
    assert [int(m) for m in jobs["mode"][9:12]] == [car.FREQ_FIXED, car.PHASE_FIXED, car.FREQ_FIXED | car.PHASE_FIXED]
    assert [int(o) % 4 for o in jobs["offset"][:4]] == [1, 2, 3, 0]
    assert np.all(rec["status"] == car.OK) and list(rec["lag_used"][:3]) == [1, 16, 64], "ESTIMATE locks at every order"
    assert np.all(np.abs(rec["freq"][:9] - jc.LONG_CAR_F0) < 1e-5)

    jobs = jc.case_of("long decide").jobs
    T = dec.TILE
    per_order = [jc.LONG_DEC] * 4 + [0, 8 * T, 8 * T + 1]
    assert [int(v) for v in jobs["n"]] == per_order * 3 and [-(-k // T) for k in per_order] == [20] * 4 + [0, 8, 9]
    assert [int(v) for v in jobs["flags"][:7]] == list(dec.ALL_FLAGS) + [dec.GRAY, dec.DIFF | dec.GRAY, dec.DIFF]
    assert [int(v) for v in jobs["order"]] == [M for M in dec.ORDERS for _ in per_order] and not (jobs["flags"] & dec.UW).any()


def test_long_decide_words_plants_and_winners():
    case, want = jc.long_decide_words()
    jobs, L, G = case.jobs, jc.WORD_LEN, dec.UW_GROUP
    rec = jc.model_of("long decide words").records
    assert len(jobs) == 19 == len(want) and np.all(jobs["n"] == jc.LONG_DEC) and np.all(jobs["uw_count"] == 0)
    for j in jobs[:18]:
        first, count = dec.candidates(j)
        groups = -(-count // G)
        assert groups > 300 and -(-groups // 64) == 5, "five trips of a lane through the job's keys"
    # where the plants lie: the group of a position is (p - the first candidate) / 256
    for first in (0, 1):					# without and with DIFF
        g = [(p - first) // G for p in jc.WORD_TIES]
        assert g == [3, 67, 70, 131] and g[1] % 64 == g[2] % 64 - 3 == g[3] % 64 == 3, "one lane's three trips and another lane between"
        assert [(p - first) // G for p in jc.WORD_LATER] == [5, 69, 133], "one lane, the exact copy in its third trip"
    behind = jc.WORD_TIES[0] + 1
    assert [(p - behind) // G for p in jc.WORD_TIES[1:]] == [64, 67, 128], "all beyond the first trip; lane 0 twice"
    for i, M in enumerate(dec.ORDERS):
        at = int(jobs["offset"][6 * i])
        assert np.all(jobs["offset"][6 * i:6 * i + 6] == at) and np.all(jobs["order"][6 * i:6 * i + 6] == M)
        burst = case.iq[at:at + jc.LONG_DEC]
        for plants in (jc.WORD_TIES, jc.WORD_LATER):
            for p in plants[1:]:
                same = burst[p - 1:p + L - 1].tobytes() == burst[plants[0] - 1:plants[0] + L - 1].tobytes()
                assert same, "the same bytes but for the last symbol"
        for p in jc.WORD_TIES[1:]:
            assert burst[p + L - 1].tobytes() == burst[jc.WORD_TIES[0] + L - 1].tobytes()
        k = dec.decisions(burst, M)[0]
        for p in jc.WORD_LATER[:2]:
            assert (k[p + L - 1] - k[jc.WORD_LATER[2] + L - 1]) % M == 1, "the last symbol of the two earlier copies is the next point"
        for flags, at_job in ((0, 6 * i), (dec.DIFF, 6 * i + 3)):
            assert [int(f) & dec.DIFF for f in jobs["flags"][at_job:at_job + 3]] == [flags] * 3
            d = dec.difference(k, M, flags)
            u = lambda job: case.uw[int(job["uw_offset"]):int(job["uw_offset"]) + int(job["uw_len"])].astype(np.int64)
            rot = 0 if flags else 1
            errors = lambda job, p: int((((d[p:p + len(u(job))] - u(job) - rot) & (M - 1)) != 0).sum())
            assert [errors(jobs[at_job], p) for p in jc.WORD_TIES] == [0] * 4
            assert [errors(jobs[at_job + 1], p) for p in jc.WORD_LATER] == [1, 1, 0], "a later position has one more match"
            assert jobs["uw_first"][at_job + 2] == behind and jobs["uw_first"][at_job] == 0
    # the winners, by the model
    got = [(int(r["uw_pos"]), int(r["uw_rot"]), int(r["uw_errors"])) for r in rec]
    assert got == want and np.all(rec["status"] == dec.OK)
    assert want[0] == (jc.WORD_TIES[0], 1, 0) and want[1] == (jc.WORD_LATER[2], 1, 0) and want[2] == (jc.WORD_TIES[1], 1, 0)
    assert want[3] == (jc.WORD_TIES[0], 0, 0) and want[4] == (jc.WORD_LATER[2], 0, 0) and want[5] == (jc.WORD_TIES[1], 0, 0)
    # the job of two rotations: 32 matches under each at its position, fewer under every rotation anywhere else
    p, r0, r1 = jc.WORD_TWO_ROTATIONS
    job = jobs[18]
    assert (int(job["order"]), int(job["flags"]), int(job["uw_len"])) == (8, dec.UW, 64) and p // G == 200
    at = int(job["offset"])
    k = dec.decisions(case.iq[at:at + jc.LONG_DEC], 8)[0]
    u = case.uw[int(job["uw_offset"]):][:64].astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(k, 64)
    matches = np.stack([(((win - u) & 7) == r).sum(1) for r in range(8)], 1)
    assert sorted(np.flatnonzero(matches[p] == 32)) == sorted((r0, r1)) and matches[p].max() == 32
    matches[p] = 0
    assert matches.max() < 32
    assert want[18] == (p, min(r0, r1), 32), "the smaller rotation wins"


CAR_SHORT = 7 * car.TILE + 5


@pytest.mark.parametrize("n", [CAR_SHORT, 7 * car.TILE + 1, 7 * car.TILE + 10, 6 * car.TILE])
@pytest.mark.parametrize("name", sorted(jc.CAR_LONG))
def test_periodic_carrier_is_the_model(F, name, n):
    """a block of 3 tiles and jobs shaped like C, D and E of 7 tiles and 5 symbols from an odd offset; and with 1 and 10 symbols
    in the last tile, where the tile before the last loses terms of lag 16, and with none"""
    block = car.psk(3 * car.TILE, 4, jc.CAR_LONG_FREQ, 0.02, 31, 30.0)
    job = jc.long_carrier_job(dict(jc.CAR_LONG[name], n=n, offset=5))
    iq = np.tile(block, (4, 1))[:5 + n]
    want_rec, want = car.carrier((iq, job))
    host_rec, host = F.carrier_host(iq, job)
    rec = jc.periodic_carrier(block, job[0])
    assert want_rec["status"][0] == car.OK and want_rec.tobytes() == host_rec.tobytes()
    if name == "E":
        for k in jc.CAR_E_FIELDS:
            assert rec[k].tobytes() == want_rec[k].tobytes(), k
        return
    assert jc.exact_products(job[0])
    assert rec.tobytes() == want_rec.tobytes(), (rec, want_rec)
    for j0, count in ((0, 2 * car.TILE), (3 * car.TILE - 7, 300), (n - n % car.TILE, n % car.TILE)):
        got = jc.carrier_symbols(block, job[0], rec, j0, count)
        assert got.tobytes() == want[0][j0:j0 + count].tobytes() == host[0].view(np.float32).reshape(-1, 2)[j0:j0 + count].tobytes()
    if name == "C":						# every period of the output is the first
        whole = want[0][:6 * car.TILE].reshape(2, 3 * car.TILE, 2)
        assert whole[0].tobytes() == whole[1].tobytes()


def test_carrier_products_are_exact():
    """what makes jobs C and D periodic: g = freq M and f = g / M are exact, g j and theta + f j are exact up to j = 2^31 - 2, and
    g TILE is a whole number; and a frequency that is not dyadic fails the same test"""
    for name in ("C", "D"):
        job = jc.long_carrier_job(jc.CAR_LONG[name])[0]
        assert jc.exact_products(job) and int(job["n"]) - 1 == 2 ** 31 - 2
    g = np.float64(jc.CAR_LONG_FREQ) * np.float64(4)
    j = np.float64(2 ** 31 - 2)
    assert (g * j) / j == g and float(g * j) == 4 * jc.CAR_LONG_A * (2 ** 31 - 2) / 4096.0
    phi = np.float64(jc.CAR_LONG_PHASE) + (np.float64(jc.CAR_LONG_FREQ) * j)
    assert (phi - np.float64(jc.CAR_LONG_FREQ) * j) == jc.CAR_LONG_PHASE and (g * car.TILE) % 1.0 == 0.0
    c0, s0 = car.cossin_turns(np.float64(jc.CAR_LONG_PHASE) + np.float64(jc.CAR_LONG_FREQ) * np.float64(5))
    c1, s1 = car.cossin_turns(np.float64(jc.CAR_LONG_PHASE) + np.float64(jc.CAR_LONG_FREQ) * np.float64(5 + 2 ** 31 - 4096))
    assert (c0, s0) == (c1, s1), "the rotation repeats every TILE symbols"
    off = jc.long_carrier_job(dict(jc.CAR_LONG["C"], freq=0.009))[0]
    assert not jc.exact_products(off)


@pytest.mark.parametrize("name", ["A", "B", "B, the word in the last group"])
def test_periodic_decide_is_the_model(F, name):
    """a block of 3 tiles and jobs shaped like A and B of 7 tiles and 5 symbols from an odd offset"""
    n, L = 7 * dec.TILE + 5, jc.DEC_LONG_WORD
    block = dec.psk(3 * dec.TILE, 4, 0.0, 0.2525, 32, 30.0)
    spec = dict(jc.DEC_LONG[name[0]], n=n, offset=5)
    if name[0] == "B":
        spec["uw_first"] = n - L - 600
    job, word = jc.long_decide_job(spec, block)
    if name == "A":						# a word of the second tile: found there, not a period later
        k = dec.decisions(jc.wrapped(block, 5 + 5000, L), 4)[0]
        word = ((k - 1) & 3).astype(np.uint8)
    iq = np.tile(block, (4, 1))[:5 + n]
    want_rec, want = dec.decide((iq, job, word))
    host_rec, host = F.decide_host(iq, job, word)
    rec, out_bytes = jc.periodic_decide(block, job[0], word)
    assert rec.tobytes() == want_rec.tobytes() == host_rec.tobytes(), (rec, want_rec)
    assert rec["status"][0] == dec.OK and rec["uw_errors"][0] == 0
    if name == "A":
        assert (rec["uw_pos"][0], rec["uw_rot"][0]) == (5000, 1)
    else:
        first, count = dec.candidates(job[0])
        assert count == 601 and (rec["uw_pos"][0] - first) // dec.UW_GROUP == 2 == -(-count // dec.UW_GROUP) - 1, "in the last group"
        assert rec["uw_pos"][0] == n - L - 50 and first + count + L - 1 == n, "the last group's decisions end on the job's last"
    assert out_bytes(0, n).tobytes() == want[0][:n].tobytes() == host[0][:n].tobytes()
    assert out_bytes(6 * dec.TILE, dec.TILE + 5).tobytes() == want[0][6 * dec.TILE:n].tobytes()
    P = 3 * dec.TILE
    assert want[0][1:P].tobytes() == want[0][P + 1:2 * P].tobytes(), "every period equals the first from byte 1 on"


def test_long_carrier_and_decide_far_geometry():
    P, T = jc.PERIOD, car.TILE
    assert P % T == 0 and P // T == 192
    for spec in list(jc.CAR_LONG.values()) + list(jc.DEC_LONG.values()):
        assert spec["n"] == 2 ** 31 - 1 and spec["offset"] % 2 == 1 and spec["offset"] + spec["n"] <= jc.FAR_SAMPLES
    assert -(-(2 ** 31 - 1) // T) == 2 ** 19 == -(-(2 ** 31 - 2) // T), "2^19 sum tiles and 2^19 lag tiles"
    assert (jc.CAR_LONG_FREQ * P) % 1.0 == 0.0, "the block repeated is one continuous burst"
    assert abs(jc.CAR_LONG_FREQ * 8) <= 0.5 and abs(jc.CAR_LONG_PHASE) <= 0.5
    block = jc.decide_block()
    job, word = jc.long_decide_job(jc.DEC_LONG["A"], block)
    first, count = dec.candidates(job[0])
    assert (first, -(-count // dec.UW_GROUP)) == (0, 2 ** 23) and len(word) == 16
    job, word = jc.long_decide_job(jc.DEC_LONG["B"], block)
    first, count = dec.candidates(job[0])
    n, L = 2 ** 31 - 1, jc.DEC_LONG_WORD
    assert count == 601 and -(-count // dec.UW_GROUP) == 3 and first + count - 1 + L == n
    # the last work-group of k_dec_uw: lo + span == n, so the unfixed ((lo + span + 3) >> 2) passed 2^31 - 1
    p0 = first + 2 * dec.UW_GROUP
    lo, span = p0 - 1, (first + count - p0) + L - 1 + 1
    assert lo + span == n and lo + span + 3 > 2 ** 31 - 1 and ((lo + span - 1) >> 2) + 1 - (lo >> 2) == -(-(lo % 4 + span) // 4)
    rec, _ = jc.periodic_decide(block, job[0], word)
    assert rec["uw_pos"][0] == n - L - 50 > 2 ** 31 - 700 and (rec["uw_pos"][0] - first) // dec.UW_GROUP == 2 and rec["status"][0] == dec.OK


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
    total = {8: jc.FAR_SAMPLES, 4: 2 * jc.FAR_SAMPLES, 1: jc.FAR_BYTES}
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
        unit = jc.OUT_BYTES[case.name]
        if unit:
            base, cap = jc.OUT_BASE[unit], jc.capacity(case.name, case.jobs)
            assert base % 16 == 0 and base - jc.FAR_GUARD >= 0 and base + cap + jc.FAR_GUARD <= total[unit]
            assert base > (2 ** 31 if unit == 8 else 2 ** 32)
            assert cap * unit % 4 == 0 and jc.FAR_GUARD * unit % 4 == 0, "the ranges and their guards are whole words"
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
