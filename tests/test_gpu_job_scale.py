"""The passes over burst IQ on long jobs and full tables (the input sets are tests/job_scale_cases.py; tests/test_job_scale_cpu.py
holds the conditions on them and runs the host twins over them).

The single-module tests (tests/test_gpu_extract.py, _resample, _measure, _demod, _correlate, _psd, _symbols, _carrier, _decide) work
in buffers of a few tens of thousands of samples: no job there has more than four partials and no call of the five older passes more
than 257 jobs.
Here
  long jobs    measure over 131 chunks and correlate over 131 tiles: k_measure_combine and k_correlate_combine fold 64 partials a
               round, so their second and third rounds run -- a lane that holds several partials, the seam rule at partials 64 and
               128, the peak's tie inside a lane across rounds and between lanes, best_tile chosen in a later round.  The cut rule
               of measure at the round boundary.  Resample at positions of the up-sampled rate around 2^32, in both forms.
               psd over 131, 64 and 65 tiles, which k_psd_combine adds one after the other, at L = 64, 256 and 1024; symbols over
               20, 8 and 9 fold and pick tiles, so the loops of k_sym_time and k_sym_record under `#pragma unroll 8` run whole
               bodies and a remainder.  carrier over 20, 8 and 9 sum tiles and 20, 8, 8 and 9 lag tiles (job_sums under `#pragma
               unroll 8` in k_car_freq and k_car_phase, which differ at 8 TILE + 1 symbols), every order, mode and three lags; decide
               over 20, 8 and 9 tiles with every flag set, and with words over 304 groups of k_dec_uw, five trips of a lane of
               k_dec_job through the keys: ties of one lane across three trips and with another lane, a later position with one
               more match, one position under two rotations -- the expected uw_pos and uw_rot asserted by name.
  full tables  every pass with exactly MAX_JOBS jobs in shuffled order, every 11th without work: the deepest search of the prefix
               and the largest table; and on a fresh instance a call of one job, the full table and the one job again, so the
               scratch slot of the pass grows behind a first, smaller call.
Every call goes through the C ABI into sentinel-filled buffers that are compared whole: bit for bit with demod_model,
correlate_model, resample_model, psd_model and symbols_model, inside measure_model.job_tolerance and extract_model.bound for the two passes whose contracts
leave the order of the additions open.  Inputs, taps and windows are compared with their host copies after the call, the ring
position, the waterfall and the spectrum with what they were before, and the stats delta with what the jobs predict.  The same call
twice is bit-identical.  carrier and decide compare bit for bit with carrier_model and decide_model, records and the whole image."""
import os

import numpy as np
import pytest

import job_scale_cases as jc
import measure_model as mm

pytestmark = pytest.mark.gpu

LONG = ("long measure", "long edges", "long tie", "long resample", "long psd", "long symbols", "long carrier", "long decide",
        "long decide words")


@pytest.fixture(scope="module")
def amd():
    from _pkg import gr_fosphor_amd
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    gr_fosphor_amd.load()
    return gr_fosphor_amd


@pytest.fixture(scope="module")
def dev(amd):
    d = jc.Dev(amd)
    yield d
    d.f.close()


def same(a, b):
    """two results of Dev.run: records and words bit-identical"""
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def assert_host(amd, case, rec, words, tag):
    """against fosphor_amd_*_host: bit for bit, but measure's sums (rule 3 leaves their order open: the model's tolerance holds them)"""
    if case.name == "extract":
        return							# its host function is a float64 statement, no twin
    host_rec, host_words = jc.host_twin(amd.Fosphor, case)
    if case.name == "measure":
        for k in mm.INTS:
            assert np.array_equal(rec[k], host_rec[k]), (tag, k)
        return
    assert words.tobytes() == host_words.tobytes(), (tag, "words differ from the host's")
    if host_rec is not None:
        assert rec.tobytes() == host_rec.tobytes(), (tag, "records differ from the host's")


@pytest.mark.parametrize("key", LONG)
def test_long_jobs(amd, dev, key):
    case, model = jc.case_of(key), jc.model_of(key)
    got = dev.run(case, tag=key)
    model.check(*got, tag=key)
    assert_host(amd, case, *got, tag=key)
    assert same(dev.run(case, tag=key + " again"), got), "the same call twice is bit-identical"
    if key == "long measure":
        rec = got[0]
        assert list(rec["peak_index"][:2]) == [jc.LONG_MEASURE_PLANTS["top in part 5"][0]] * 2
        assert list(rec["n_edges"][:2]) == [len(jc.LONG_MEASURE_PLANTS)] * 2
        jc.assert_long_measure_cut(case, rec, model.tols[0])
    if key == "long tie":
        assert list(got[0]["peak_lag"]) == [jc.TIE_LAGS[0], jc.TIE_LAGS[0], jc.TIE_LAGS[1] - jc.TIE_SECOND]
    if key == "long decide words":
        rec, want = got[0], jc.long_decide_words()[1]
        assert [(int(r["uw_pos"]), int(r["uw_rot"]), int(r["uw_errors"])) for r in rec] == want
        ties, later = jc.WORD_TIES, jc.WORD_LATER
        for at in (0, 6, 12):					# per order: without DIFF (uw_rot 1), then with (uw_rot 0)
            assert list(rec["uw_pos"][at:at + 6]) == [ties[0], later[2], ties[1]] * 2, "the smallest of equal positions; one more match"
            assert list(rec["uw_rot"][at:at + 6]) == [1, 1, 1, 0, 0, 0]
        assert (rec["uw_pos"][18], rec["uw_rot"][18]) == (jc.WORD_TWO_ROTATIONS[0], min(jc.WORD_TWO_ROTATIONS[1:])), "the smaller rotation"


@pytest.mark.parametrize("name", jc.PASSES)
def test_full_table(amd, dev, name):
    key = "full " + name
    case, model = jc.case_of(key), jc.model_of(key)
    assert len(case.jobs) == jc.MAX_JOBS
    got = dev.run(case, tag=key)
    model.check(*got, tag=key)
    assert_host(amd, case, *got, tag=key)
    assert same(dev.run(case, tag=key + " again"), got), "the same call twice is bit-identical"


@pytest.mark.parametrize("name", jc.PASSES)
def test_the_scratch_grows_behind_a_small_call(amd, name):
    """a fresh instance: one job, the full table, the one job again"""
    key = "full " + name
    case = jc.case_of(key)
    one = jc.one_job_of(case)
    d = jc.Dev(amd)
    try:
        first = d.run(one, tag=key + ": one job")
        full = d.run(case, tag=key + ": the full table")
        third = d.run(one, tag=key + ": one job again")
    finally:
        d.f.close()
    jc.Model(one).check(*first, tag=key + ": one job")
    jc.model_of(key).check(*full, tag=key + ": the full table behind a small call")
    assert same(first, third), "the one job gives the same bits before and behind the full table"
