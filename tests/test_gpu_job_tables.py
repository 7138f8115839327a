"""The job tables of eight passes over burst IQ (gr-fosphor_amd/csrc/fosphor_jobs.h) on one instance: extract, then measure,
demod, correlate, psd and symbols over what extract wrote, carrier over what symbols wrote and decide over what carrier wrote, three
times with tables of 3, 300 and 2 jobs -- every scratch buffer of the instance grows once and is then reused larger than the table
needs.

A job's length comes from what can break the shared code: nothing (between live jobs and as the last job of a table), 1, one
work-group's worth, one more, and two work-groups' worth plus 3 -- of extract's TILE_OUT 256 and WAVE_OUT 4 outputs, measure's CHUNK
of 8192 samples (and WAVE_MAX 4096, the longest job a wave takes), demod's TILE of 2048 trace values at avg 1 and 3, correlate's TILE
of 1024 lags with templates of 1, 2 and 33 samples.  psd's lengths are its own: nothing, L - 1 (no segment), L, L + hop, one TILE of
32 segments, one more, and two and 3, at L = 64 (WAVE) and L = 256 (GROUP); symbols': nothing, 3 samples (no symbol), and what gives
1, 4096, 4097 and 2 * 4096 + 3 symbols, at sps 2 under FIXED and sps 5 under ESTIMATE.  Offsets walk through 0, 1, 2, 3, so spans begin
on and off a 16-byte boundary.  carrier's and decide's jobs come from fosphor_amd_carrier_from_symbols and
fosphor_amd_decide_from_carrier over the records of the pass before, so their lengths are those symbol counts (the tiles of both are
4096 symbols); carrier takes the orders, its four modes and the lags 1, 16 and 64 in turn, decide its four flag sets, every third
job with a word of 8 symbols cut from the decisions of the host chain.
The single-module tests (tests/test_gpu_extract.py, _measure, _demod, _correlate, _psd, _symbols, _carrier, _decide) hold each pass's
own seams at one table size; what is new here is the alternation of sizes on one instance, the chain, and jobs without work between and behind the live ones.

What is compared: demod's traces, correlate's and psd's records and traces and symbols' records and symbols with
fosphor_amd_demod_host, fosphor_amd_correlate_host, fosphor_amd_psd_host and fosphor_amd_symbols_host over the same buffer, bit for
bit; carrier's records and symbols and decide's records and bytes with fosphor_amd_carrier_host and fosphor_amd_decide_host over the
host chain (the host's symbols, then the host's derotated symbols), bit for bit; measure's integer fields and peak with
fosphor_amd_measure_host bit for bit, its eight sums in double
within measure_model.job_tolerance of the host's, because the header leaves the order of the additions open (rule 3) and the kernels
use that; extract against the float64 model within extract_model.bound, as tests/test_gpu_extract.py does, because extract's host
function is a float64 statement and no bit-exact twin.  Every stats delta is what the table predicts."""
import os

import numpy as np
import pytest

import carrier_model as car
import correlate_model as cm
import decide_model as dec
import demod_model as dm
import extract_model as em
import job_scale_cases as jc
import measure_model as mm
import psd_model as pm
import symbols_model as sm

pytestmark = pytest.mark.gpu

LONG = 42000				# outputs of the first extract job of every table: what the other passes read
TILE_DT, WAVE_DT = (2, 9), (32, 257)	# (decim, taps) of the two extract forms
TPL = 40


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


def lengths(per):
    return [0, 1, per, per + 1, 2 * per + 3]


def pick(kinds, count, nothing):
    """count rows out of kinds, in turn; kinds[1] is a job without work, which so lies between live jobs, and a table of more or
    fewer than 3 jobs ends with one"""
    rows = [kinds[k % len(kinds)] for k in range(count)]
    if count != 3:
        rows[-1] = nothing
    return rows


def extract_table(count):
    """the long TILE job first; then both forms at every length, `first` walking through 0 .. 3"""
    assert em.form(*TILE_DT) == "tile" and em.form(*WAVE_DT) == "wave"
    kinds = [(0, LONG) + TILE_DT, (1, 0) + TILE_DT]
    kinds += [(k % 4, n) + TILE_DT for k, n in enumerate(lengths(256)[1:])]
    kinds += [(k % 4, n) + WAVE_DT for k, n in enumerate(lengths(4))]
    rows = pick(kinds, count, (1, 0) + WAVE_DT)
    return em.make_jobs([(first, n, d, (0x01234567 * (k + 1)) & 0xffffffff, 77 * k, 0 if t == TILE_DT[1] else TILE_DT[1], t)
                         for k, (first, n, d, t) in enumerate(rows)])


def measure_table(count, at, thr):
    kinds = [(n, k % 4) for k, n in enumerate([mm.WAVE_MAX, 0, 1, mm.CHUNK, mm.CHUNK + 1, 2 * mm.CHUNK + 3])]
    return mm.make_jobs([(at + off, n, thr) for n, off in pick(kinds, count, (0, 1))])


def demod_table(count, at):
    kinds = []
    for avg in (1, 3):
        for k, n_out in enumerate(lengths(dm.TILE // avg)):
            mode = (dm.POWER, dm.PHASE, dm.FM)[(k + avg) % 3]
            n = n_out * avg + (avg - 1 if n_out else 0) + (1 if mode == dm.FM and n_out else 0)	# a remainder that gives no output
            kinds.append((at + k % 4, n, mode, avg))
    kinds[0], kinds[1] = kinds[1], kinds[0]			# a live job first: kinds[1] is the one without outputs
    assert [dm.n_out(mode, n, avg) for _, n, mode, avg in kinds[:3]] == [1, 0, dm.TILE]
    return dm.place(pick(kinds, count, (at + 2, 1, dm.FM, 1)))


def correlate_table(count, at):
    kinds = []
    for i, T in enumerate((33, 1, 2)):
        for k, n_lags in enumerate(lengths(1024)):
            n = n_lags + T - 1 if n_lags else (T - 1) * (k & 1)		# without lags: no samples, or one too few
            kinds.append((at + (k + i) % 4, i & 1, n, T, (cm.RHO, cm.C, cm.NONE)[(k + i) % 3], 0.3))
    kinds[0], kinds[1] = kinds[1], kinds[0]
    assert [cm.n_lags(k[2], k[3]) for k in kinds[:3]] == [1, 0, 1024]
    jobs = cm.place(pick(kinds, count, (at + 1, 0, 0, 2, cm.RHO, 0.3)))
    odd = (jobs["trace"] == cm.C) & (jobs["out_offset"] & 1 != 0)
    jobs["out_offset"][odd] -= 1				# a complex64 view begins on an even float; GUARD keeps the ranges apart
    return jobs


PSD_SHAPES = ((6, 16, 0), (8, 100, 64))	# (fft_len_log, hop, win_offset): WAVE and GROUP


def psd_table(count, at):
    kinds = []
    for log, hop, woff in PSD_SHAPES:
        L = 1 << log
        for k, n in enumerate([0, L - 1, L, L + hop] + [jc.psd_n_for(c, log, hop) for c in (pm.TILE, pm.TILE + 1, 2 * pm.TILE + 3)]):
            kinds.append((at + k % 4, woff, n, log, hop, (pm.NONE, pm.SQUARE, pm.FOURTH, pm.MAGSQ)[(k + log) % 4],
                          pm.T_NONE if k % 3 == 2 and n != L else pm.T_POWER, 0.99, 1e-2))
    kinds[0], kinds[2] = kinds[2], kinds[0]			# a live job first; kinds[1] has no segment
    assert [pm.n_seg(k[2], k[3], k[4]) for k in kinds[:3]] == [1, 0, 0] and kinds[0][6] == pm.T_POWER
    assert max(k[0] + k[2] for k in kinds) <= at + LONG
    return pm.place(pick(kinds, count, (at + 1, 0, 63, 6, 16, pm.NONE, pm.T_POWER, 0.99, 1e-2)))


def symbols_table(count, at):
    kinds = []
    for sps, mode, tau, first in ((2, sm.FIXED, 0.25, 2), (5, sm.ESTIMATE, 0.0, 5)):	# first: the latest the first symbol can lie
        for k, n in enumerate([0, 3] + [sm.n_for(c, first, sps) for c in (1, sm.TILE, sm.TILE + 1, 2 * sm.TILE + 3)]):
            kinds.append((at + k % 4, n, sps, mode, tau))
    kinds[0], kinds[2] = kinds[2], kinds[0]			# a live job first; kinds[1] has no symbol
    assert [sm.max_out(k[1], k[2]) for k in kinds[:3]] == [1, 0, 0]
    assert max(k[0] + k[1] for k in kinds) <= at + LONG
    return sm.place(pick(kinds, count, (at + 1, 0, 5, sm.ESTIMATE, 0.0)))


def carrier_table(F, sjobs, srec):
    """a carrier job per symbols job and record: the orders, the four modes and three lags in turn, the outputs one behind the
    other with 0 or 1 symbols between them"""
    out, at = [], 0
    for i in range(len(sjobs)):
        mode = i % 4
        j = F.carrier_jobs(sjobs[i:i + 1], srec[i:i + 1], car.ORDERS[i % 3], mode=mode, lag=(1, 16, 64)[(i // 3) % 3],
                           freq=0.01 if mode & car.FREQ_FIXED else 0.0, phase=-0.125 if mode & car.PHASE_FIXED else 0.0)
        j["out_offset"] = at
        at += int(j["n"][0]) + (i & 1)
        out.append(j)
    return np.concatenate(out)


WORD = 8


def decide_table(F, cjobs, crec, yc):
    """a decide job per carrier job and record: the four flag sets in turn; every third job that is long enough looks over all its
    positions for the WORD differences (or decisions) that fosphor_amd_decide_host finds in its middle -> (jobs, the word table)"""
    plain = np.concatenate([F.decide_jobs(cjobs[i:i + 1], crec[i:i + 1], flags=dec.ALL_FLAGS[i % 4] & dec.DIFF) for i in range(len(cjobs))])
    at = 0
    for j in plain:
        j["out_offset"] = at
        at += dec.owned(j["n"])
    _, d = F.decide_host(yc, plain)				# without GRAY and a word the bytes are rule 3's d
    out, words, at = [], [], 0
    for i in range(len(cjobs)):
        flags, n = dec.ALL_FLAGS[i % 4], int(plain["n"][i])
        word = {}
        if i % 3 == 0 and n > 2 * WORD:
            word = dict(uw_offset=WORD * len(words), uw_len=WORD)
            words.append(np.array(d[i][n // 2:n // 2 + WORD], np.uint8))
            flags |= dec.UW
        j = F.decide_jobs(cjobs[i:i + 1], crec[i:i + 1], flags=flags, **word)
        j["out_offset"] = at
        at += dec.owned(j["n"][0]) + dec.GUARD * (1 + (i & 1))
        out.append(j)
    return np.concatenate(out), (np.concatenate(words) if words else np.zeros(0, np.uint8))


def delta(stats, before):
    after = stats()
    return {k: after[k] - before[k] for k in after}


@pytest.fixture(scope="module")
def stream():
    rng = np.random.default_rng(1616)
    x = (rng.standard_normal((2 * LONG + 4200, 2)) * 0.5).astype(np.float32)
    taps = np.concatenate([em.design(*TILE_DT, 0.8), em.design(*WAVE_DT, 0.8)]).astype(np.float32)
    tpl = (rng.standard_normal((TPL, 2)) * 0.5).astype(np.float32)
    return x, taps, tpl


def test_tables_of_3_300_2_jobs(amd, stream):
    import torch
    F = amd.Fosphor
    x, taps, tpl = stream
    win = np.concatenate([F.psd_window("hann", 6), F.psd_window("blackman_harris", 8)])
    xc = x.astype(np.float64) @ np.array([1.0, 1.0j])
    d_x, d_tpl = torch.from_numpy(x).cuda(), torch.from_numpy(tpl).cuda()
    f = F(n_bins=128, wf_rows=16)
    try:
        for count in (3, 300, 2):
            # extract
            ejobs = extract_table(count)
            assert len(ejobs) == count and ejobs["n_out"][-1 if count != 3 else 1] == 0
            before = f.extract_stats()
            views = f.extract(d_x, ejobs, taps)
            forms = np.array([em.form(int(j["decim"]), int(j["n_taps"])) for j in ejobs])
            live = ejobs["n_out"] > 0
            assert delta(f.extract_stats, before) == dict(
                calls=1, k_tile=int((forms[live] == "tile").any()), k_wave=int((forms[live] == "wave").any()),
                jobs_tile=int((forms == "tile").sum()), jobs_wave=int((forms == "wave").sum()),
                samples=sum(em.need(int(j["n_out"]), int(j["decim"]), int(j["n_taps"])) for j in ejobs[live])), count
            cap = int((ejobs["out_offset"] + ejobs["n_out"]).max())
            y = np.zeros((cap, 2), np.float32)
            for j, v in zip(ejobs, views):
                got = v.cpu().numpy().view(np.float32).reshape(-1, 2)
                assert len(got) == j["n_out"]
                y[int(j["out_offset"]):int(j["out_offset"]) + int(j["n_out"])] = got
                if j["n_out"]:
                    want, tol = em.extract_job(xc, j, taps), em.bound(xc, j, taps)
                    err = max(np.abs(got[:, 0] - want.real).max(), np.abs(got[:, 1] - want.imag).max())
                    assert err <= tol, (count, j, err, tol)
            base = views[0].data_ptr() - 8 * int(ejobs["out_offset"][0])	# extract()'s buffer: the views are slices of it
            at = int(ejobs["out_offset"][0])					# the long job's outputs: what the others read
            assert ejobs["n_out"][0] == LONG

            # measure
            thr = np.float32((y[at:at + LONG].astype(np.float64) ** 2).sum(axis=1).mean())
            jobs = measure_table(count, at, thr)
            before = f.measure_stats()
            got = f.measure(base, jobs, n_samples=cap)
            split = jobs["n"] > mm.WAVE_MAX
            assert delta(f.measure_stats, before) == dict(
                calls=1, k_wave=int((~split).any()), k_split=int(split.any()), k_combine=int(split.any()),
                jobs_wave=int((~split).sum()), jobs_split=int(split.sum()), samples=int(jobs["n"].sum())), count
            host = F.measure_host(y, jobs)
            worst = 0.0
            for i, (g, h, j) in enumerate(zip(got, host, jobs)):
                for k in mm.INTS:
                    assert g[k].tobytes() == h[k].tobytes(), (count, i, k, g[k], h[k])
                tol = mm.job_tolerance(y, j)
                for k in mm.SUMS:
                    err = abs(float(g[k]) - float(h[k]))
                    assert err <= tol[k], (count, i, k, float(g[k]), float(h[k]), tol[k])
                    worst = max(worst, err / tol[k] if tol[k] else 0.0)
            print("table of %d: measure's sums differ from the host's by at most %.3g of the tolerance" % (count, worst))

            # demod
            jobs = demod_table(count, at)
            n_out = np.array([dm.n_out(int(j["mode"]), int(j["n"]), int(j["avg"])) for j in jobs])
            before = f.demod_stats()
            got = f.demod(base, jobs, n_samples=cap)
            direct = jobs["avg"] == 1
            assert delta(f.demod_stats, before) == dict(
                calls=1, k_direct=int((direct & (n_out > 0)).any()), k_avg=int((~direct & (n_out > 0)).any()),
                jobs_direct=int(direct.sum()), jobs_avg=int((~direct).sum()), samples=int(jobs["n"].sum()),
                outputs=int(n_out.sum())), count
            for i, (g, h) in enumerate(zip(got, F.demod_host(y, jobs))):
                assert len(h) == n_out[i] and g.cpu().numpy().tobytes() == h.tobytes(), (count, i, tuple(jobs[i]))

            # correlate
            jobs = correlate_table(count, at)
            lags = [cm.n_lags(int(j["n"]), int(j["tpl_len"])) for j in jobs]
            before = f.correlate_stats()
            rec, got = f.correlate(base, jobs, d_tpl, n_samples=cap)
            assert delta(f.correlate_stats, before) == dict(calls=1, k_tile=int(any(lags)), k_combine=1, jobs=len(jobs),
                                                            lags=sum(lags), macs=cm.macs(jobs)), count
            hrec, hviews = F.correlate_host(y, jobs, tpl)
            assert rec.tobytes() == hrec.tobytes(), (count, [i for i in range(len(jobs)) if rec[i] != hrec[i]][:4])
            for i, (g, h) in enumerate(zip(got, hviews)):
                assert (g is None) == (h is None) == (jobs["trace"][i] == cm.NONE)
                if h is not None:
                    assert g.cpu().numpy().tobytes() == h.tobytes(), (count, i, tuple(jobs[i]))

            # psd
            jobs = psd_table(count, at)
            assert len(jobs) == count and pm.job_n_seg(jobs[-1 if count != 3 else 1]) == 0
            before = f.psd_stats()
            rec, got = f.psd(base, jobs, win, n_samples=cap)
            assert delta(f.psd_stats, before) == jc.expected_stats("psd", jobs), count
            hrec, hviews = F.psd_host(y, jobs, win)
            assert rec.tobytes() == hrec.tobytes(), (count, [i for i in range(len(jobs)) if rec[i] != hrec[i]][:4])
            for i, (g, h) in enumerate(zip(got, hviews)):
                assert (g is None) == (h is None) == (pm.n_out(jobs[i]) == 0)
                if h is not None:
                    assert g.cpu().numpy().tobytes() == h.tobytes(), (count, i, tuple(jobs[i]))
            if count == 300:
                assert sorted(set(rec["n_seg"])) == [0, 1, 2, pm.TILE, pm.TILE + 1, 2 * pm.TILE + 3]

            # symbols
            jobs = symbols_table(count, at)
            assert len(jobs) == count and sm.job_max_out(jobs[-1 if count != 3 else 1]) == 0
            before = f.symbols_stats()
            rec, got = f.symbols(base, jobs, n_samples=cap)
            assert delta(f.symbols_stats, before) == sm.expected_stats(jobs, rec), count
            hrec, hviews = F.symbols_host(y, jobs)
            assert rec.tobytes() == hrec.tobytes(), (count, [i for i in range(len(jobs)) if rec[i] != hrec[i]][:4])
            for i, (g, h) in enumerate(zip(got, hviews)):
                assert len(h) == rec["n_sym"][i] and g.cpu().numpy().tobytes() == h.tobytes(), (count, i, tuple(jobs[i]))
            if count == 300:
                assert {1, sm.TILE, sm.TILE + 1, 2 * sm.TILE + 3} <= set(rec["n_sym"]) and np.all(rec["status"] == sm.OK)

            # carrier, over what symbols wrote: on the device its buffer, on the host the host's
            sym_base = got[0].data_ptr() - 8 * int(jobs["out_offset"][0])
            ys = np.asarray(hviews[0].base).view(np.float32).reshape(-1, 2)
            cjobs = carrier_table(F, jobs, hrec)
            assert len(cjobs) == count and cjobs["n"][-1 if count != 3 else 1] == 0 and np.array_equal(cjobs["n"], hrec["n_sym"])
            before = f.carrier_stats()
            rec, got = f.carrier(sym_base, cjobs, n_samples=len(ys))
            assert delta(f.carrier_stats, before) == car.expected_stats(cjobs), count
            hrec, hviews = F.carrier_host(ys, cjobs)
            assert rec.tobytes() == hrec.tobytes(), (count, [i for i in range(len(cjobs)) if rec[i] != hrec[i]][:4])
            for i, (g, h) in enumerate(zip(got, hviews)):
                assert len(h) == (cjobs["n"][i] if hrec["status"][i] == car.OK else 0)
                assert g.cpu().numpy().tobytes() == h.tobytes(), (count, i, tuple(cjobs[i]))
            if count == 300:
                assert {1, car.TILE, car.TILE + 1, 2 * car.TILE + 3} <= set(rec["n"][rec["status"] == car.OK])
                assert set(cjobs["mode"]) == {0, 1, 2, 3} and set(cjobs["lag"]) == {1, 16, 64} and set(cjobs["order"]) == set(car.ORDERS)

            # decide, over what carrier wrote
            car_base = got[0].data_ptr() - 8 * int(cjobs["out_offset"][0])
            yc = np.asarray(hviews[0].base).view(np.float32).reshape(-1, 2)
            djobs, uw = decide_table(F, cjobs, hrec, yc)
            assert len(djobs) == count and djobs["n"][-1 if count != 3 else 1] == 0
            before = f.decide_stats()
            rec, got = f.decide(car_base, djobs, uw, n_samples=len(yc))
            assert delta(f.decide_stats, before) == dec.expected_stats(djobs), count
            hrec, hviews = F.decide_host(yc, djobs, uw)
            assert rec.tobytes() == hrec.tobytes(), (count, [i for i in range(len(djobs)) if rec[i] != hrec[i]][:4])
            for i, (g, h) in enumerate(zip(got, hviews)):
                assert len(h) == djobs["n"][i] and g.cpu().numpy().tobytes() == h.tobytes(), (count, i, tuple(djobs[i]))
            if count == 300:
                assert {1, dec.TILE, dec.TILE + 1, 2 * dec.TILE + 3} <= set(rec["n"]) and set(djobs["flags"] & 3) == {0, 1, 2, 3}
                with_word = (djobs["flags"] & dec.UW) != 0
                assert with_word.sum() >= 50 and np.all(rec["status"][with_word] == dec.OK) and np.all(rec["uw_pos"][with_word] >= 0)
    finally:
        f.close()
