"""The burst-IQ passes at the sizes their interface is built for: the input sets tests/test_job_scale_cpu.py,
tests/test_gpu_job_scale.py and tests/test_gpu_job_far.py share, one view of the nine passes over them, and the geometry of the far
buffer.

A case here is a Case: the pass, its jobs and the host copies of its buffers.  The nine models stay what they are
(tests/extract_model.py, resample_model.py, measure_model.py, demod_model.py, correlate_model.py, psd_model.py, symbols_model.py,
carrier_model.py, decide_model.py; carrier's rules 5 and 6 take the index of their first symbol);
this file only names, per pass, the job field that places the input, the width of an output element in bytes (decide's out_offset
counts bytes, in multiples of 4, and a job owns 4 ceil(n / 4) of them), the stats a call must leave
and the comparison the pass's contract allows: bit for bit where the contract pins the order of the operations (resample, demod,
correlate, psd, symbols, carrier, decide), inside measure_model.job_tolerance and extract_model.bound where it leaves the order open.

The long cases
  measure    130 * CHUNK + 5 samples: k_measure_combine folds 64 partials a round, so three rounds.  Plants (LONG_MEASURE_PLANTS)
             relative to the job's sample 0.
  correlate  130 * TILE + 5 lags: k_correlate_combine gives lane l the tiles l, l + 64, l + 128.  An edges pattern with runs over
             the seams 63|64 and 127|128, and a tie of bit-identical windows in tiles 3, 67 and 70 -- tile 67 is lane 3's second
             tile, so the tie is met inside a lane in a later round as well as between lanes -- and, in a second job that begins
             behind the first window, in tiles 64, 66 and 128: all beyond the first round, 64 and 128 in lane 0.
  resample   U = 256 and an input of 2^24 + 64 samples of which only the tail is read: positions p = phase0 + m D of the up-sampled
             rate around (n - Q) U, just beyond 2^32.
  psd        130 * TILE + 5 segments at L = 64 (hop 1, WAVE), 256 (hop 3) and 1024 (hop 7, GROUP): k_psd_combine adds 131 tiles one
             after the other, the last of 5 segments; copies cut to 64 * TILE and 64 * TILE + 1 segments (64 and 65 tiles) with a
             job without a segment between them; FOURTH, and a job without a trace.
  symbols    R = 19 * TILE + 5 symbols at sps 3 and 64 (ESTIMATE) and 2 (FIXED): 20 fold tiles and 20 pick tiles, which
             k_sym_time and k_sym_record add under `#pragma unroll 8` -- two unrolled bodies and a remainder of 4; sps 8 with
             8 * TILE (one body exactly) and 8 * TILE + 1 symbols; a job of n = 0 in between.
  carrier    19 * TILE + 5 symbols (20 sum tiles, 20 lag tiles: job_sums, under `#pragma unroll 8`, runs two bodies and a
             remainder of 4) at every order under ESTIMATE with lags 1, 16 and 64 and under the three other modes; 8 * TILE,
             8 * TILE + 1 (9 sum tiles, 8 lag tiles: where k_car_freq and k_car_phase differ) and 8 * TILE + 2; n = 0 in between.
  decide     19 * TILE + 5, 8 * TILE and 8 * TILE + 1 symbols at every order, every flag set without a word, DIFF over every tile
             seam (the sum loop of k_dec_job under `#pragma unroll 8`).  "long decide words": 304 groups of k_dec_uw a job, five
             trips of a lane of k_dec_job; the same word in the groups 3, 67, 131 (one lane) and 70; a later position with one more
             match; a window that begins behind the first copy; one position under two rotations (long_decide_words).
The full tables: exactly MAX_JOBS jobs of tiny shapes in shuffled order, every 11th without work (psd's, symbols', carrier's and
decide's are their models' own full_table_case()).
The far buffer: FAR_SAMPLES float2 samples, about 16.01 GiB; bases and their aliases below.
The long far jobs of psd and symbols read n = 2^31 - 1 samples, which no model can hold: the far buffer is one noise block of
PERIOD samples repeated, PERIOD a multiple of the job's tile stride (TILE hop, TILE sps), so tile c of the job sees the samples of
tile c mod (PERIOD / stride).  periodic_psd and periodic_symbols compute those PERIOD / stride distinct full tiles and the last,
partial one with the models' own functions and add them in the pinned serial order: the whole record, the whole trace, and the
symbols of the first period and of the last tile, bit for bit.  PERIOD = 3 * 2^18 divides neither 2^31 nor 2^32 (both leave
2^18 or 2^19 samples), so a position truncated to 31 or 32 bits reads other samples.
The long far jobs of carrier and decide (CAR_LONG, DEC_LONG) run over the same kind of buffer with 192 tiles a period.  A decision
does not depend on j, so decide is periodic as it stands (periodic_decide).  carrier's g j and theta + f j are periodic only where
they are exact: with freq = 37 / 2^12 and a dyadic phase they are, and repeat every TILE symbols but for whole turns, which
fosphor_amd_cossin_turns takes off exactly (exact_products, periodic_carrier); under ESTIMATE only the lag sums, m2 and mm are.

What these cases are aimed at: every expression of the kernels that forms an address or a position from offset, first, out_offset,
tpl_offset, phase0, m0, k0, c or blockIdx.x, with the type it is evaluated in, as read in gr-fosphor_amd/csrc (all are 64-bit, or
below 2^31 because the prefix gives a job no work-group beyond its n, n_out or n_lags, which are int32):
  find_job (fosphor_jobs.h)  lo, hi, mid: int, below MAX_JOBS; prefix[] and g: uint32, at most 2^31 - 1 work-groups a launch
  k_extract_tile    m0 = (int)(blockIdx.x - prefix[j]) * 256: int, < n_out.  base = (int64_t)m0 * D: int64.
                    src = (elem *)x + first + base: pointer + int64 + int64.  phi0 = phase0 + (uint32_t)(uint64_t)base * phase_inc
                    and phi0 + (uint32_t)i * inc: uint32 on purpose, the phase is taken mod 2^32.  span, head + g * per,
                    tail0 + tid, r * R + q: int / uint32, below D * R <= 6656.  out[out_offset + m0 + tid]: int64 + int + int.
  k_extract_wave    m = (int64_t)(blockIdx.x - prefix[j]) * 4 + wave, n0 = m * decim: int64.  src = x + first + n0: pointer +
                    int64 + int64; src + k: k < T <= 8192.  phi0: uint32 as above.  out[out_offset + m]: int64.
  k_resample_tile   m0 = (int)(..) * 512: int, < n_out.  p0 = phase0 + (int64_t)m0 * D, b0 = (p0 + U - 1) / U: int64.
                    s0 = (int)(b0 * U - p0): an int64 difference in 0 .. U - 1.  iq + offset + b0: pointer + int64 + int64.
                    span, pos = k * D - s0, db, db * U - pos: int, below 512 * 256 + 256.  out + out_offset + m0: pointer + int64.
  k_resample_direct m = (int64_t)(..) * 256 + threadIdx.x, pos = phase0 + m * down, b: int64.  iq + offset + b: pointer + int64.
                    taps + taps_offset + (int)(b * U - pos): an int64 difference below U.  out[out_offset + m]: int64.
  k_measure_wave    j = blockIdx.x * 4 + wave: int, below MAX_JOBS.  iq + offset: pointer + int64.  scan(): m, m0 + 2 g: int, < n.
  k_measure_split   c = (int)(blockIdx.x - prefix[j]), m0 = c * 8192: int, < n.  m1 = min(n - m0, 8192) + m0: int, <= n, written so
                    that nothing passes n.  parts + part0 + c: pointer + int + int, each below the launch's 2^31 - 1 work-groups.
  k_measure_combine parts + part0 + c0 + lane: pointer + int, c0 + lane < chunks.  records + record: below MAX_JOBS.
  k_demod_direct    t0 = c * 2048: int, < n_out.  iq + offset + t0, out + out_offset + t0: pointer + int64 + int.
  k_demod_avg       o0 = c * (2048 / L): int, < n_out.  iq + offset + (int64_t)o0 * L: int64 (o0 * L < n all the same).
                    out + out_offset + o0: pointer + int64 + int.  row * stride + ..: int, below 3072.
  k_correlate_tile  k0 = c * 1024: int, < n_lags.  iq + offset + k0, tpl + tpl_offset: pointer + int64 (+ int).
                    out[out_offset + k0 + q]: int64 + int + int.  out + out_offset + 2 * (int64_t)k0: int64.
                    parts + blockIdx.x: pointer + uint32.
  k_correlate_combine  parts + prefix[j]: pointer + uint32; parts[c], parts[c - 1], parts[best_tile]: int, < tiles.
                    records + j: below MAX_JOBS.  tpl + tpl_offset: pointer + int64.
  psd_tile          (k_psd_group: c = (int)(blockIdx.x - prefix[j]); k_psd_wave: g = blockIdx.x * 4 + wave: uint32, below the
                    form's tiles, c = (int)(g - prefix[j]))  s0 = c * 32, s1 = min(s0 + 32, n_seg): int, s0 < n_seg <= 2^31 - 64.
                    y = iq + offset: pointer + int64.  y + (int64_t)s * hop: int64 (s hop + L <= n all the same).
                    win + win_offset: pointer + int64; w[i], i < L.  parts + part0 + (int64_t)c * L: pointer + int64 + int64, up to
                    2^29 doubles in one job and 2^41 in a call.  bitrev, pad, i0, i1, j << (kLog - tt): int, below 1088.
  k_psd_combine     j = blockIdx.x * 4 + wave: int, below MAX_JOBS.  tiles = (n_seg + 31) / 32: int, n_seg + 31 < 2^31.
                    T = parts + part0 + ((i + half) & (L - 1)): pointer + int64 + int; T[(int64_t)c * L]: int64.
                    out[out_offset + i]: int64 + int.  records[record]: below MAX_JOBS.  (double)n_seg: exact.
  k_sym_fold        c = (int)(blockIdx.x - fold_prefix[j]); n / sps - c * 4096: int, c * 4096 <= n / sps.
                    tile = iq + offset + (int64_t)c * 4096 * sps: pointer + int64 + int64.  tile + s0 * sps: int, below 4096 * 64.
                    i + (i / row) * sps, b * (row + sps) + k: int, below 4160.  parts[part0 + (int64_t)c * sps + t]: int64.
  k_sym_time        j: int, below MAX_JOBS.  tiles = (R + 4095) / 4096: int, R <= (2^31 - 1) / 3.  parts + part0 + lane: pointer +
                    int64 + int; T[(int64_t)c * sps]: int64.  tw + tw0: int, below 2 * 64 * 63.  state_of: base = e * sps in double,
                    n - 3 - first: int, first <= 64.
  k_sym_pick        j0 = (int)(blockIdx.x - pick_prefix[j]) * 4096: int, < max_out <= 2^30.  y = iq + offset: pointer + int64.
                    out = out + out_offset + j0: pointer + int64 + int.  span = y + (first - 1) + (int64_t)(j0 + s0) * sps: int +
                    int64, j0 + s0 < n_sym.  span + t * sps, (count - 1) * sps + 4: int, below 256 * 64.  out[s0 + t]: int, < 4096.
                    mom[(mom0 + j0 / 4096) * 6 + t]: int64.
  k_sym_record      tiles = min((n_sym + 4095) / 4096, tiles_max): int.  mom + mom0 * 6 + lane: pointer + int64 + int;
                    T[(int64_t)c * 6]: int64.  records[j], counts[j]: below MAX_JOBS.
  k_car_lag         c = (int)(blockIdx.x - lag_prefix[j]), j0 = c * 4096: int, < n - 1.  terms = min(n - 1 - j0, 4096), span =
                    min(n - (j0 + s0), count + Le), count_l = min(n - Le - (j0 + s0), count): int, differences of values <= n (count_l
                    may be negative: no term).  y = iq + offset + j0: pointer + int64 + int.  y + s0, s_p[at + t + Le]: int, below
                    4096 + 321.  lag_parts + (lag0 + c) * 4: pointer + (int64 + int) * int.  lag_used_of: 2 * lag <= 128.
  k_car_freq        j = blockIdx.x * 4 + wave: int, below MAX_JOBS.  tiles_of(max(n - 1, 0)): the sum n + 4095 in int64.
                    job_sums: lag_parts + lag0 * 4 + lane: pointer + int64; T[(int64_t)c * 4]: int64.  (double)Le * a1: exact.
  k_car_sum         j0 = c * 4096: int, < n.  syms = min(n - j0, 4096).  y = iq + offset + j0: pointer + int64 + int; y[s0 + t]: int,
                    < 4096.  (int64_t)j0 + s0 + t: int64, < n; (double) of it exact.  sum_parts + (sum0 + c) * 4: int64.
  k_car_phase       tiles_of(n): int64 inside.  sum_parts + sum0 * 4: pointer + int64.  records[j], turn[j]: below MAX_JOBS.
  k_car_turn        j0 as in k_car_sum.  out = out + out_offset + j0: pointer + int64 + int.  y[s], out[s]: int, < 4096.
                    (int64_t)j0 + s: int64; theta + f * (double)j in double.
  k_dec_hard        j0 = c * 4096: int, < n.  y = iq + offset + j0: pointer + int64 + int.  dec = dec + (tile0 + c) * 1024: pointer +
                    (int64 + int) * int, up to 2^19 tiles of 4 KiB in one job.  dec[(s0 + t) >> 2]: int, < 1024.  parts + (tile0 + c):
                    int64.  the counts: 16-bit fields of at most 16, summed over 64 lanes and 4 waves.
  k_dec_uw          g = (int)(blockIdx.x - uw_prefix[j]); p0 = p_first + g * 256: int, a candidate, so <= n - uw_len.  count =
                    min(p_first + p_count - p0, 256): p_first + p_count <= n - uw_len + 1 <= 2^31 - 1.  lo = p0 - diff >= 0.
                    span = count + uw_len - 1 + diff <= 320, and lo + span <= n.  words = ((lo + span - 1) >> 2) + 1 - (lo >> 2):
                    int, nothing passes n -- it was ((lo + span + 3) >> 2) - (lo >> 2), whose sum passes 2^31 - 1 in the last
                    work-group of a job of n >= 2^31 - 3 symbols whose candidates run to its last position (DEC_LONG["B"]); the one
                    expression of the nine kernels that had to change.  dec + tile0 * 1024: pointer + int64; dec[w0 + t]: int,
                    w0 < 2^29.  uw[uw_at + t]: int, below MAX_UW_TABLE.  key_of: 0x7fffffff - p with 0 <= p < 2^31, then uint64.
                    keys[key0 + g]: int64 + int.
  k_dec_job         j: int, below MAX_JOBS.  tiles_of(n): int64 inside.  parts + tile0: pointer + int64; parts[c]: int, < 2^19.
                    count += parts[c].cnt[..]: int, at most n in all.  groups = ((int64_t)p_count + 255) / 256: int64, then int
                    <= 2^23.  keys[key0 + g]: int64 + int.  records[j], rot[j]: below MAX_JOBS.
  k_dec_out         j0 = c * 4096: int, < n.  dec + (tile0 + c) * 1024: int64.  out + (out_offset >> 2) + (j0 >> 2): pointer + int64 +
                    int, in words.  j0 + s > 0: int, < n.  dec[w - 1]: the word before, of the tile before where w = 0 (c > 0 then).
None other is a 32-bit product or sum that can pass 2^31 - 1 within what the rules of the headers accept."""
import fractions
import functools

import numpy as np

import carrier_model as car
import correlate_model as cm
import decide_model as dec
import demod_model as dm
import extract_model as em
import measure_model as mm
import psd_model as pm
import resample_model as rm
import symbols_model as sm

SENTINEL = 0x5a5a5a5a
PASSES = ("extract", "resample", "measure", "demod", "correlate", "psd", "symbols", "carrier", "decide")
MODELS = {"extract": em, "resample": rm, "measure": mm, "demod": dm, "correlate": cm, "psd": pm, "symbols": sm, "carrier": car,
          "decide": dec}
MAX_JOBS = 4096
GUARD = 3						# every model's: output elements before, between and behind the jobs' ranges


class Case:
    """name: the pass; jobs; iq: float32 [n][2], or int16 / float16 [n][2] with fmt; taps: float32 (extract, resample); tpl:
    float32 [n][2] or None where the templates lie in iq (correlate); win: float32, the windows (psd); uw: uint8, the call's table
    of unique-word symbols (decide), a host buffer like the jobs"""

    def __init__(self, name, jobs, iq, taps=None, tpl=None, fmt=em.FP32, win=None, uw=None):
        self.name, self.jobs, self.fmt = name, np.ascontiguousarray(jobs, MODELS[name].JOB_DTYPE), fmt
        self.iq = np.ascontiguousarray(iq, em.RAW_DTYPE[fmt]).reshape(-1, 2)
        self.taps = None if taps is None else np.ascontiguousarray(taps, np.float32)
        self.tpl = None if tpl is None else np.ascontiguousarray(tpl, np.float32).reshape(-1, 2)
        self.win = None if win is None else np.ascontiguousarray(win, np.float32).reshape(-1)
        self.uw = None if uw is None else np.ascontiguousarray(uw, np.uint8).reshape(-1)

    def with_jobs(self, jobs):
        return Case(self.name, jobs, self.iq, self.taps, self.tpl, self.fmt, self.win, self.uw)

    def model_case(self):
        """the case as its model's functions take it"""
        return {"extract": (self.fmt, self.iq, self.jobs, self.taps), "resample": (self.iq, self.taps, self.jobs),
                "measure": (self.iq, self.jobs), "demod": (self.iq, self.jobs), "correlate": (self.iq, self.tpl, self.jobs),
                "psd": (self.iq, self.win, self.jobs), "symbols": (self.iq, self.jobs), "carrier": (self.iq, self.jobs),
                "decide": (self.iq, self.jobs, self.uw)}[self.name]


def from_model(name, case):
    """a case of one of the models' cases() as a Case"""
    if name == "extract":
        fmt, raw, jobs, taps = case
        return Case(name, jobs, raw, taps=taps, fmt=fmt)
    if name == "resample":
        return Case(name, case[2], case[0], taps=case[1])
    if name == "correlate":
        return Case(name, case[2], case[0], tpl=case[1])
    if name == "psd":
        return Case(name, case[2], case[0], win=case[1])
    if name == "decide":
        return Case(name, case[1], case[0], uw=case[2])
    return Case(name, case[1], case[0])


# ---- one view of the nine passes --------------------------------------------------------------------------------------------------

IN_FIELD = {"extract": "first", "resample": "offset", "measure": "offset", "demod": "offset", "correlate": "offset", "psd": "offset",
            "symbols": "offset", "carrier": "offset", "decide": "offset"}
# bytes of an out_offset unit: complex64, float32, or -- decide -- the byte itself, at out_offsets that are multiples of 4
OUT_BYTES = {"extract": 8, "resample": 8, "measure": 0, "demod": 4, "correlate": 4, "psd": 4, "symbols": 8, "carrier": 8, "decide": 1}
WITH_RECORDS = ("measure", "correlate", "psd", "symbols", "carrier", "decide")


def guard(name):
    """output elements before, between and behind the jobs' ranges: every model's GUARD, decide's 4 bytes"""
    return dec.GUARD if name == "decide" else GUARD


def out_words(name, elements):
    """the 32-bit words of `elements` units of out_offset; decide's bytes come in fours"""
    assert (elements * OUT_BYTES[name]) % 4 == 0, (name, elements)
    return elements * OUT_BYTES[name] // 4


def sample_bytes(case):
    return 8 if case.fmt == em.FP32 else 4


def n_out(name, job):
    """the output elements of a job, in units of its out_offset; a symbols job reserves its max_out, a decide job owns
    4 ceil(n / 4) bytes, a carrier job its n symbols also where it finds no carrier and writes none"""
    if name in ("extract", "resample"):
        return int(job["n_out"])
    if name == "demod":
        return dm.n_out(int(job["mode"]), int(job["n"]), int(job["avg"]))
    if name == "correlate":
        return cm.n_out(int(job["trace"]), int(job["n"]), int(job["tpl_len"]))
    if name == "psd":
        return pm.n_out(job)
    if name == "symbols":
        return sm.job_max_out(job)
    if name == "carrier":
        return int(job["n"])
    if name == "decide":
        return dec.owned(job["n"])
    return 0


def has_out(name, job):
    """does out_offset of the job mean anything?  A correlate or psd job without a trace must leave it 0"""
    if name == "psd":
        return int(job["trace"]) != pm.T_NONE
    return name != "measure" and not (name == "correlate" and int(job["trace"]) == cm.NONE)


def has_work(name, job):
    """does the job give a work-group something to do?"""
    if name == "measure":
        return int(job["n"]) > 0
    if name == "psd":
        return pm.job_n_seg(job) > 0
    return n_out(name, job) > 0


def capacity(name, jobs):
    """output elements of a case's buffer: the last one written and guard(name) behind it"""
    return max([int(j["out_offset"]) + n_out(name, j) for j in jobs if has_out(name, j)] + [0]) + guard(name)


def in_span(name, job):
    """[begin, end) of the input samples a job may read"""
    if name == "extract":
        return int(job["first"]), int(job["first"]) + em.need(int(job["n_out"]), int(job["decim"]), int(job["n_taps"]))
    return int(job["offset"]), int(job["offset"]) + int(job["n"])


def out_ranges(name, jobs):
    """[begin, end) of the output elements of the jobs that write some"""
    return [(int(j["out_offset"]), int(j["out_offset"]) + n_out(name, j)) for j in jobs if has_out(name, j) and n_out(name, j)]


def disjoint(ranges):
    ranges = sorted(ranges)
    return all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))


def forms(name, jobs):
    """the kernel form of every job, as the pass's stats name it"""
    if name == "extract":
        return [em.form(int(j["decim"]), int(j["n_taps"])) for j in jobs]
    if name == "resample":
        return [rm.form(int(j["up"]), int(j["down"]), int(j["n_taps"])) for j in jobs]
    if name == "measure":
        return ["wave" if mm.form(int(j["n"])) == mm.FORM_WAVE else "split" for j in jobs]
    if name == "demod":
        return ["direct" if j["avg"] == 1 else "avg" for j in jobs]
    if name == "psd":
        return ["group" if int(j["fft_len_log"]) > pm.WAVE_MAX_LOG else "wave" for j in jobs]
    if name == "symbols":
        return ["estimate" if int(j["mode"]) == sm.ESTIMATE else "fixed" for j in jobs]
    if name == "carrier":					# jobs_freq: does k_car_lag and k_car_freq work for the job?
        return ["fixed" if int(j["mode"]) & car.FREQ_FIXED else "estimate" for j in jobs]
    if name == "decide":					# jobs_uw
        return ["word" if int(j["flags"]) & dec.UW else "plain" for j in jobs]
    return ["tile"] * len(jobs)


def expected_stats(name, jobs, records=None):
    """the stats delta one successful call leaves: the forms that ran, and what they were given.  records: what the call wrote
    (symbols alone: its counter of symbols is the records' n_sym, which the caller holds to the model)"""
    f = np.array(forms(name, jobs))
    if name == "resample":
        return rm.expected_stats(jobs)
    if name == "symbols":
        return sm.expected_stats(jobs, records)
    if name in ("carrier", "decide"):
        return MODELS[name].expected_stats(jobs)
    if name == "psd":					# what tests/test_gpu_psd.py's Box.run asserts
        segs = np.array([pm.job_n_seg(j) for j in jobs])
        return dict(calls=1, k_group=int(((f == "group") & (segs > 0)).any()), k_wave=int(((f == "wave") & (segs > 0)).any()),
                    k_combine=1, jobs=len(jobs), segments=int(segs.sum()))
    if name == "extract":
        live = jobs["n_out"] > 0
        return dict(calls=1, k_tile=int((f[live] == "tile").any()), k_wave=int((f[live] == "wave").any()),
                    jobs_tile=int((f == "tile").sum()), jobs_wave=int((f == "wave").sum()),
                    samples=sum(em.need(int(j["n_out"]), int(j["decim"]), int(j["n_taps"])) for j in jobs[live]))
    if name == "measure":
        split = f == "split"
        return dict(calls=1, k_wave=int((~split).any()), k_split=int(split.any()), k_combine=int(split.any()),
                    jobs_wave=int((~split).sum()), jobs_split=int(split.sum()), samples=int(jobs["n"].astype(np.int64).sum()))
    if name == "demod":
        outs = np.array([n_out(name, j) for j in jobs])
        direct = f == "direct"
        return dict(calls=1, k_direct=int((direct & (outs > 0)).any()), k_avg=int((~direct & (outs > 0)).any()),
                    jobs_direct=int(direct.sum()), jobs_avg=int((~direct).sum()), samples=int(jobs["n"].astype(np.int64).sum()),
                    outputs=int(outs.sum()))
    lags = [cm.n_lags(int(j["n"]), int(j["tpl_len"])) for j in jobs]
    return dict(calls=1, k_tile=int(any(lags)), k_combine=1, jobs=len(jobs), lags=sum(lags), macs=cm.macs(jobs))


class Model:
    """what the model says of a case, computed once: records (measure, correlate, psd, symbols, carrier, decide), the image of the
    output buffer as uint32 words with SENTINEL wherever no job writes (resample, demod, correlate, psd, symbols, carrier, decide:
    a carrier job without a carrier writes nothing, a decide job all the bytes it owns), or the float64 outputs and bounds per job
    (extract)"""

    def __init__(self, case):
        name, jobs = case.name, case.jobs
        self.case, self.records, self.image, self.tols, self.outs = case, None, None, None, None
        if name == "measure":
            self.records = mm.measure(case.iq, jobs)
            self.tols = [mm.job_tolerance(case.iq, j) for j in jobs]
        elif name == "demod":
            self.image = dm.image(case.iq, jobs, SENTINEL)
        elif name == "resample":
            self.image = rm.image(case.model_case(), SENTINEL)
        elif name == "correlate":
            self.records, self.image = cm.image(case.model_case(), SENTINEL)
        elif name == "psd":
            self.records, self.image = pm.image(case.model_case(), SENTINEL)
        elif name == "symbols":
            self.records, image = sm.image(case.model_case(), SENTINEL)
            self.image = image.reshape(-1)
        elif name == "carrier":
            self.records, image = car.image(case.model_case(), SENTINEL)
            self.image = image.reshape(-1)
        elif name == "decide":
            self.records, image = dec.image(case.model_case(), SENTINEL & 0xff)
            self.image = image.view(np.uint32)
        else:
            x = em.widen(case.iq, case.fmt)
            self.outs = [em.extract_job(x, j, case.taps) for j in jobs]
            self.tols = [em.bound(x, j, case.taps) for j in jobs]

    def check(self, rec, words, tag=""):
        """rec: the records as the pass left them, or None; words: the whole output buffer as uint32 [out_words(capacity)]"""
        name, jobs = self.case.name, self.case.jobs
        if name == "measure":
            mm.assert_records(rec, self.records, self.tols, tag)
            return
        assert len(words) == out_words(name, capacity(name, jobs)), tag
        if name in ("correlate", "psd", "symbols", "carrier", "decide"):
            bad = [i for i in range(len(jobs)) if rec[i].tobytes() != self.records[i].tobytes()]
            assert not bad, (tag, "records differ from the model's", bad[:4], rec[bad[:2]], self.records[bad[:2]])
        if name != "extract":
            bad = np.flatnonzero(words != self.image)
            assert not len(bad), (tag, "words differ from the model's image", bad[:8], words[bad[:8]], self.image[bad[:8]])
            return
        out = words.reshape(-1, 2)
        written = np.zeros(len(out), bool)
        for j, want, tol in zip(jobs, self.outs, self.tols):
            sl = slice(int(j["out_offset"]), int(j["out_offset"]) + int(j["n_out"]))
            written[sl] = True
            if j["n_out"]:
                y = out[sl].view(np.float32).astype(np.float64)
                err = max(np.abs(y[:, 0] - want.real).max(), np.abs(y[:, 1] - want.imag).max())
                assert err <= tol, (tag, tuple(j), err, tol)
        assert np.all(out[~written] == SENTINEL), (tag, "written outside the jobs' ranges")


@functools.lru_cache(maxsize=None)
def model_of(key):
    """the Model of the case CASES[key]() builds; both computed once"""
    return Model(case_of(key))


@functools.lru_cache(maxsize=None)
def case_of(key):
    return CASES[key]()


def host_twin(F, case):
    """the case through fosphor_amd_*_host -> (records or None, the output buffer as uint32 words or None), laid out as a device
    run lays them out but for the words no job writes.  extract's host function is a float64 statement, no twin: not here."""
    name, jobs = case.name, case.jobs
    if name == "measure":
        return F.measure_host(case.iq, jobs), None
    words = np.full(out_words(name, capacity(name, jobs)), SENTINEL, np.uint32)
    rec = None
    if name == "demod":
        views = F.demod_host(case.iq, jobs)
    elif name == "resample":
        views = F.resample_host(case.iq, jobs, case.taps)
    elif name == "psd":
        rec, views = F.psd_host(case.iq, jobs, case.win)
    elif name == "symbols":
        rec, views = F.symbols_host(case.iq, jobs)
    elif name == "carrier":
        rec, views = F.carrier_host(case.iq, jobs)
    elif name == "decide":
        rec, views = F.decide_host(case.iq, jobs, case.uw)
        whole = views[0].base if len(views) else None	# the host's buffer: a job owns the bytes up to the next multiple of 4
        views = [whole.view(np.uint8)[int(j["out_offset"]):int(j["out_offset"]) + dec.owned(j["n"])] for j in jobs]
    else:
        rec, views = F.correlate_host(case.iq, jobs, case.iq if case.tpl is None else case.tpl)
    for j, v in zip(jobs, views):
        if v is not None and v.size:
            w = np.ascontiguousarray(v).view(np.uint32).reshape(-1)
            at = out_words(name, int(j["out_offset"]))
            words[at:at + len(w)] = w
    return rec, words


# ---- the long cases -----------------------------------------------------------------------------------------------------------------

LONG_PARTS = 130
LONG_MEASURE_N = LONG_PARTS * mm.CHUNK + 5
LONG_MEASURE_CUT = 64 * mm.CHUNK
LONG_MEASURE_THRESHOLD = 0.5
# name -> (first sample, last sample, is it the maximum?), relative to the job's sample 0
LONG_MEASURE_PLANTS = {
    "top in part 5": (5 * mm.CHUNK + 100, 5 * mm.CHUNK + 100, True),
    "run over the round boundary": (64 * mm.CHUNK - 3, 64 * mm.CHUNK + 2, False),
    "top in part 70": (70 * mm.CHUNK + 17, 70 * mm.CHUNK + 17, True),
    "rising edge at a part's first sample": (128 * mm.CHUNK, 128 * mm.CHUNK + 8, False),
    "top in part 129": (129 * mm.CHUNK + 40, 129 * mm.CHUNK + 40, True),
    "the last sample": (LONG_MEASURE_N - 1, LONG_MEASURE_N - 1, False),
}


def long_measure_case():
    """quiet noise (p around 2e-4) with LONG_MEASURE_PLANTS, twice: from sample 1 and from an even sample.  The jobs: the whole at
    the odd and at the even offset; exactly 64 parts, one sample more, 65 parts; and what is left of the whole behind
    LONG_MEASURE_CUT, which with the job of 64 parts is the whole cut in two."""
    rng = np.random.default_rng(6464)
    n, cut, thr = LONG_MEASURE_N, LONG_MEASURE_CUT, LONG_MEASURE_THRESHOLD
    base = (rng.standard_normal((n, 2)) * 0.01).astype(np.float32)
    big, top = np.float32([0.75, -0.5]), np.float32([1.5, 0.25])
    for first, last, is_top in LONG_MEASURE_PLANTS.values():
        base[first:last + 1] = top if is_top else big
    even = n + 3 + ((n + 3) & 1)
    iq = np.zeros((even + n, 2), np.float32)
    iq[1:1 + n] = base
    iq[even:even + n] = base
    rows = [(1, n, thr), (even, n, thr), (1, cut, thr), (even, cut + 1, thr), (1, 65 * mm.CHUNK, thr), (1 + cut, n - cut, thr)]
    return Case("measure", mm.make_jobs(rows), iq)


def assert_long_measure_cut(case, rec, tol):
    """the cut rule over the records of long_measure_case(): the whole against the two jobs it is cut into at LONG_MEASURE_CUT, as
    tests/test_measure_cpu.py cuts -- the edge at the cut counted once, r1 after the one term at the cut is put back.  tol: the
    whole job's mm.job_tolerance"""
    cut, n, thr = LONG_MEASURE_CUT, LONG_MEASURE_N, np.float32(LONG_MEASURE_THRESHOLD)
    w, a, b = rec[0], rec[2], rec[5]
    assert (a["n"], b["n"]) == (cut, n - cut)
    y = case.iq[1:1 + n]
    p = mm.power(y[cut - 1:cut + 1])
    both = bool(p[0] >= thr) and bool(p[1] >= thr)
    assert both, "the cut lies inside a run"
    assert w["n_above"] == a["n_above"] + b["n_above"] and w["n_edges"] == a["n_edges"] + b["n_edges"] - int(both)
    y = y[cut - 1:cut + 1].astype(np.float64)
    at = {"r1_re": y[1, 0] * y[0, 0] + y[1, 1] * y[0, 1], "r1_im": y[1, 1] * y[0, 0] - y[1, 0] * y[0, 1]}
    for k in mm.SUMS:
        assert abs(float(w[k]) - (float(a[k]) + float(b[k]) + at.get(k, 0.0))) <= tol[k], k


LONG_TILES = 130
LONG_LAGS =LONG_TILES * cm.TILE + 5


def long_edges_pattern():
    """which of LONG_LAGS lags are above, for T = 1: cm.edges_pattern()'s kinds at the seams a later round of the combine settles"""
    T = cm.TILE
    on = np.zeros(LONG_LAGS, bool)
    on[0] = True
    on[5:9] = True
    on[3 * T] = True						# a tile ends below, the next begins above
    on[64 * T - 1:64 * T + 1] = True				# one edge over the seam 63|64: lane 0's second tile
    on[65 * T - 1] = True					# tile 64 ends above, tile 65 begins below
    on[128 * T - 2:128 * T + 3] = True				# one edge over the seam 127|128: lane 0's third tile
    on[129 * T] = True						# tile 128 ends below, tile 129 begins above
    on[LONG_LAGS - 3:] = True					# up to the last lag
    rng = np.random.default_rng(41)
    for tile in (1, 100):
        on[tile * T + 50:(tile + 1) * T - 50] = rng.random(T - 100) < 0.3
    return on


def long_edges_case():
    """T = 1 with the template (1, 0), as cm.edges_case(): `above` is long_edges_pattern() at the threshold 0.5.  All three traces;
    the C job begins one sample in, so its seams cut the pattern one lag earlier."""
    on = long_edges_pattern()
    iq = cm.noise(len(on), 40)
    iq[~on] = 0.0
    tpl = np.array([(1.0, 0.0), (0.6, -0.8)], np.float32)
    n = len(on)
    rows = [(0, 0, n, 1, cm.RHO, 0.5), (0, 0, n, 1, cm.NONE, 0.5), (1, 0, n - 1, 1, cm.C, 0.5)]
    return Case("correlate", cm.place(rows), iq, tpl=tpl)


TIE_T = 48
TIE_LAGS = tuple(t * cm.TILE + k for t, k in ((3, 100), (67, 333), (70, 137), (131, 277)))	# where the window lies in iq
TIE_SECOND = 3 * cm.TILE + 200				# the second job's first sample: behind the first window's first sample
TIE_SECOND_LAGS = 128 * cm.TILE + 300


def long_tie_case():
    """cm.tie_case() extended: the template is iq[TIE_LAGS[0] ..] itself and the same T samples lie at the other TIE_LAGS, so rho
    is the same float at those lags and the largest of all; the smallest lag wins.  Job 0 (rho trace) and job 1 (no trace) have
    LONG_LAGS lags and see the windows in tiles 3, 67 and 70; job 2 (C trace) begins at TIE_SECOND and sees those of tiles 67, 70
    and the fourth in its tiles 64, 66 and 128."""
    total = TIE_SECOND + TIE_SECOND_LAGS + TIE_T - 1
    iq = cm.noise(total, 30)
    for at in TIE_LAGS[1:]:
        iq[at:at + TIE_T] = iq[TIE_LAGS[0]:TIE_LAGS[0] + TIE_T]
    n = LONG_LAGS + TIE_T - 1
    rows = [(0, TIE_LAGS[0], n, TIE_T, cm.RHO, 0.5), (0, TIE_LAGS[0], n, TIE_T, cm.NONE, 0.5),
            (TIE_SECOND, TIE_LAGS[0], TIE_SECOND_LAGS + TIE_T - 1, TIE_T, cm.C, 0.5)]
    return Case("correlate", cm.place(rows), iq)


RS_N = 2 ** 24 + 64					# input samples of the long resample case
RS_UP = 256
RS_TAIL = 4096						# the samples that are not zero: the last ones
RS_TILE = (255, 2)					# (D, Q) of the TILE form
RS_DIRECT = (251, rm.seam_of(RS_UP, down=251) + 1)	# of the DIRECT form: with U = 256 the form is DIRECT from this Q on, whatever D


def rs_rows():
    """(phase0, n_out, D, Q, taps_offset) of the long resample jobs: per form, the outputs that end at (n - Q) U exactly for
    k = 1, 2, 40, the one output at (n - Q) U, and a job of 570 outputs whose second TILE tile begins beyond 2^32 while its first
    begins below"""
    rows, at = [], 1
    for D, Q in (RS_TILE, RS_DIRECT):
        room = (RS_N - Q) * RS_UP
        for k in (1, 2, 40):
            rows.append((room - 3 * D * k, 3 * k + 1, D, Q, at))
        rows.append((room, 1, D, Q, at))
        rows.append((room - 569 * D, 570, D, Q, at))
        at += Q * RS_UP + 3
    return rows


def long_resample_case():
    """U = 256 over RS_N samples of which the last RS_TAIL are noise and the rest zero; the jobs of rs_rows(), offset 0 and the
    whole buffer each"""
    iq = np.zeros((RS_N, 2), np.float32)
    iq[RS_N - RS_TAIL:] = rm.noise(RS_TAIL, 90)
    rows = [(0, ph, RS_N, n_out, RS_UP, D, toff, Q * RS_UP) for ph, n_out, D, Q, toff in rs_rows()]
    taps = rm.some_taps(1 + (RS_TILE[1] + RS_DIRECT[1]) * RS_UP + 6, 91)
    return Case("resample", rm.place(rows), iq, taps=taps)


LONG_SEGS = 130 * pm.TILE + 5
LONG_PSD_SHAPES = ((6, 1), (8, 3), (10, 7))		# (fft_len_log, hop): WAVE; GROUP below its longest transform; GROUP at it


def psd_n_for(segs, log, hop):
    """the shortest n that gives `segs` segments"""
    return (1 << log) + (segs - 1) * hop if segs else (1 << log) - 1


def long_psd_case():
    """ordinary noise under a Hann window.  Jobs 0 .. 2: LONG_SEGS segments at LONG_PSD_SHAPES, offsets 1, 2, 1.  Job 3: the second
    shape under FOURTH from the other parity; job 4: the first shape without a trace.  Then job 2 cut to 64 * TILE segments, a job
    without a segment, and job 0 cut to 64 * TILE + 1 segments."""
    bank, rows = pm.Bank(), []
    for i, (log, hop) in enumerate(LONG_PSD_SHAPES):
        rows.append((1 + (i & 1), bank.at(log, pm.HANN, i), psd_n_for(LONG_SEGS, log, hop), log, hop, pm.NONE, pm.T_POWER, 0.99, 1e-2))
    (log0, hop0), (log1, hop1), (log2, hop2) = LONG_PSD_SHAPES
    rows.append((1, bank.at(log1, pm.HANN, 1), psd_n_for(LONG_SEGS, log1, hop1), log1, hop1, pm.FOURTH, pm.T_POWER, 0.5, 1e-3))
    rows.append((2, bank.at(log0, pm.HANN, 0), psd_n_for(LONG_SEGS, log0, hop0), log0, hop0, pm.NONE, pm.T_NONE, 0.99, 1e-2))
    rows.append((1, bank.at(log2, pm.HANN, 2), psd_n_for(64 * pm.TILE, log2, hop2), log2, hop2, pm.NONE, pm.T_POWER, 0.99, 1e-2))
    rows.append((3, bank.at(log1, pm.HANN, 1), psd_n_for(0, log1, hop1), log1, hop1, pm.NONE, pm.T_POWER, 0.99, 1e-2))
    rows.append((1, bank.at(log0, pm.HANN, 0), psd_n_for(64 * pm.TILE + 1, log0, hop0), log0, hop0, pm.NONE, pm.T_POWER, 0.99, 1e-2))
    longest = max(r[0] + r[2] for r in rows)
    return Case("psd", pm.place(rows), pm.noise(longest, 6565), win=bank.buffer())


LONG_SYMS = 19 * sm.TILE + 5


def long_symbols_case():
    """ordinary noise.  n / sps = LONG_SYMS at sps 3 and 64 under ESTIMATE, n a few samples more than a multiple of sps, so max_out
    is LONG_SYMS as well; n_sym = LONG_SYMS at sps 2 under FIXED (tau 0.25: first = 2); a job of n = 0; sps 8 under ESTIMATE with
    n / sps = 8 * TILE and 8 * TILE + 1.  The offsets 1, 2, 3, 0, 2, 1."""
    R = LONG_SYMS
    rows = [(1, 3 * R + 1, 3, sm.ESTIMATE, 0.0), (2, 64 * R + 37, 64, sm.ESTIMATE, 0.0),
            (3, sm.n_for(R, 2, 2, extra=1), 2, sm.FIXED, 0.25), (0, 0, 5, sm.ESTIMATE, 0.0),
            (2, 8 * (8 * sm.TILE) + 3, 8, sm.ESTIMATE, 0.0), (1, 8 * (8 * sm.TILE + 1) + 7, 8, sm.ESTIMATE, 0.0)]
    longest = max(r[0] + r[1] for r in rows)
    return Case("symbols", sm.place(rows), sm.noise(longest, 6566))


LONG_CAR = 19 * car.TILE + 5
LONG_CAR_F0, LONG_CAR_THETA0 = 0.004, 0.03		# turns per symbol and turns of the buffer's carrier: g = M f0 <= 0.032


def long_carrier_case():
    """one BPSK buffer with a carrier offset in 30 dB of noise: its M-th power is a constant turned by M f0 a symbol at M = 2, 4 and
    8 alike, so ESTIMATE locks at every order.  Jobs 0 .. 8: LONG_CAR symbols (20 sum tiles and 20 lag tiles: two unrolled bodies
    of job_sums and a remainder of 4) under ESTIMATE at every order with the lags 1, 16 and 64; then the same n under FREQ_FIXED,
    PHASE_FIXED and both; a job of n = 0; and 8 TILE (8 and 8 tiles: one body exactly), 8 TILE + 1 (9 sum tiles, 8 lag tiles) and
    8 TILE + 2 (9 and 9) under ESTIMATE.  The offsets walk through 1, 2, 3, 0."""
    iq = car.psk(LONG_CAR + 4, 2, LONG_CAR_F0, LONG_CAR_THETA0, 6567, 30.0)
    rows = [(LONG_CAR, M, car.ESTIMATE, lag, 0.0, 0.0) for M in car.ORDERS for lag in (1, 16, 64)]
    rows += [(LONG_CAR, 4, car.FREQ_FIXED, 16, LONG_CAR_F0, 0.0), (LONG_CAR, 2, car.PHASE_FIXED, 64, 0.0, 0.125),
             (LONG_CAR, 8, car.FREQ_FIXED | car.PHASE_FIXED, 1, -0.0123, -0.25), (0, 4, car.ESTIMATE, 16, 0.0, 0.0)]
    rows += [(n, M, car.ESTIMATE, 16, 0.0, 0.0) for n, M in ((8 * car.TILE, 2), (8 * car.TILE + 1, 4), (8 * car.TILE + 2, 8))]
    return Case("carrier", car.place([((i + 1) % 4,) + r for i, r in enumerate(rows)]), iq)


LONG_DEC = 19 * dec.TILE + 5


def long_decide_case():
    """planted PSK (decide_model.three_bursts, turned by 1 / M turns).  Per order: LONG_DEC symbols (20 tiles, which k_dec_job adds
    under `#pragma unroll 8`: two bodies and a remainder of 4) with each of the four flag sets without a word -- the two with DIFF
    take a difference over each of the 19 tile seams --, a job of n = 0, then 8 TILE (one body exactly) and 8 TILE + 1 symbols under
    DIFF | GRAY and DIFF.  The offsets walk through 1, 2, 3, 0."""
    iq, at, _ = dec.three_bursts(LONG_DEC + 4, 6568)
    rows = []
    for M in dec.ORDERS:
        rows += [(LONG_DEC, M, flags) for flags in dec.ALL_FLAGS]
        rows += [(0, M, dec.GRAY), (8 * dec.TILE, M, dec.DIFF | dec.GRAY), (8 * dec.TILE + 1, M, dec.DIFF)]
    rows = [(at[M] + (i + 1) % 4, n, M, flags) for i, (n, M, flags) in enumerate(rows)]
    return Case("decide", dec.place(rows), iq, uw=np.zeros(0, np.uint8))


WORD_LEN = 40
# job-relative positions of the same WORD_LEN (and one before, for the differences) symbols: with uw_first = 0 they fall in the
# groups 3, 67, 70 and 131 of k_dec_uw -- 3, 67 and 131 are lane 3's first, second and third trip through k_dec_job's keys, 70 is
# lane 6's second -- and in a job whose window begins behind the first of them in the groups 64, 67 and 128: lane 0's second and
# third trip and lane 3's second
WORD_TIES = tuple(g * dec.UW_GROUP + k for g, k in ((3, 10), (67, 100), (70, 137), (131, 200)))
# ... of a word whose copies at the first two positions have their last symbol turned by 1 / M turns: one error there under every
# flag set, none at the third -- groups 5 and 69 (lane 5's first and second trip) and 133 (its third)
WORD_LATER = tuple(g * dec.UW_GROUP + k for g, k in ((5, 20), (69, 50), (133, 90)))
WORD_TWO_ROTATIONS = (200 * dec.UW_GROUP + 31, 2, 5)	# (position, the two rotations): an 8PSK word of 64 symbols, half under each


@functools.lru_cache(maxsize=None)
def long_decide_words():
    """-> (the Case "long decide words", [(uw_pos, uw_rot, uw_errors) that rule 4 must give per job]).
    Per order one burst of LONG_DEC symbols with the plants of WORD_TIES and WORD_LATER copied into it (long_tie_case's method: the
    same bytes, so the same decisions), and per order and without / with DIFF three jobs over all of it, uw_first = uw_count = 0,
    LONG_DEC - WORD_LEN + 1 candidates in 304 groups, five trips of a lane of k_dec_job:
      the word of WORD_TIES: four positions without an error, the smallest wins;
      the word of WORD_LATER: one error at the two earlier positions, none at the third, which wins from lane 5's third trip;
      the word of WORD_TIES in a window that begins one position behind the first: the second position wins, from a second trip.
    Without DIFF the words are the decisions less 1, so uw_rot = 1.  The last job, 8PSK without DIFF: a word of 64 symbols that
    meets WORD_TWO_ROTATIONS' position with 32 matches under each of two rotations and no other position with as many: the smaller
    rotation wins."""
    L = WORD_LEN
    iq, at, _ = dec.three_bursts(LONG_DEC + 4, 6569)
    iq = iq.copy()
    start = {M: at[M] + 1 + i for i, M in enumerate(dec.ORDERS)}		# the jobs' first symbol
    for M in dec.ORDERS:
        burst = iq[start[M]:start[M] + LONG_DEC]
        for plants in (WORD_TIES, WORD_LATER):
            for p in plants[1:]:
                burst[p - 1:p + L] = burst[plants[0] - 1:plants[0] + L]
        turn = np.exp(2j * np.pi / M)
        for p in WORD_LATER[:2]:						# the last symbol of the word, turned to the next point
            z = complex(burst[p + L - 1, 0], burst[p + L - 1, 1]) * turn
            burst[p + L - 1] = (z.real, z.imag)
    words, rows, want = [], [], []

    def add(M, flags, word, first, max_errors, expect):
        rows.append((start[M], LONG_DEC, M, flags | dec.UW, sum(len(w) for w in words), len(word), first, 0, max_errors))
        words.append(np.asarray(word, np.uint8))
        want.append(expect)

    for M in dec.ORDERS:
        k = dec.decisions(iq[start[M]:start[M] + LONG_DEC], M)[0]
        for flags in (0, dec.DIFF):
            d = dec.difference(k, M, flags)
            rot = 0 if flags else 1
            cut = lambda p: (d[p:p + L] - rot) & (M - 1)
            add(M, flags, cut(WORD_TIES[0]), 0, 0, (WORD_TIES[0], rot, 0))
            add(M, flags | dec.GRAY, cut(WORD_LATER[2]), 0, 0, (WORD_LATER[2], rot, 0))
            add(M, flags, cut(WORD_TIES[0]), WORD_TIES[0] + 1, 0, (WORD_TIES[1], rot, 0))
    p, r0, r1 = WORD_TWO_ROTATIONS
    k = dec.decisions(iq[start[8]:start[8] + LONG_DEC], 8)[0]
    word = np.concatenate([k[p:p + 32] - r1, k[p + 32:p + 64] - r0]) & 7
    add(8, 0, word, 0, 32, (p, min(r0, r1), 32))
    return Case("decide", dec.place(rows), iq, uw=np.concatenate(words)), want


# ---- the full tables ----------------------------------------------------------------------------------------------------------------

def shuffled(jobs, seed):
    """the jobs in another order: their outputs are then out of order"""
    return jobs[np.random.default_rng(seed).permutation(len(jobs))]


def full_extract_case():
    """MAX_JOBS sc16 jobs: TILE (2, 9) and (3, 25), WAVE (32, 70), up to 12 and 5 outputs; every 11th writes nothing"""
    rng = np.random.default_rng(4096)
    shapes = [(2, 9), (32, 70), (3, 25)]
    taps, where = em.one_tap_set(rng, shapes)
    n, rows = 3000, []
    for i in range(MAX_JOBS):
        d, t = shapes[i % 3]
        k = 0 if i % 11 == 0 else int(rng.integers(1, 6 if em.form(d, t) == "wave" else 13))
        rows.append((int(rng.integers(0, n - em.need(k, d, t) + 1)), k, d, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)),
                     where[(d, t)], t))
    return Case("extract", shuffled(em.make_jobs(rows), 1), em.stream(em.SC16, n, 4097), taps=taps, fmt=em.SC16)


def full_resample_case():
    """MAX_JOBS jobs of rm.COUNT_FORMS -- TILE (3, 2, 4) and DIRECT (1, 16, 5) -- up to 12 outputs; every 11th writes nothing"""
    rng = np.random.default_rng(4098)
    total, rows = 3000, []
    for i in range(MAX_JOBS):
        U, D, Q = rm.COUNT_FORMS[i % 2]
        k = 0 if i % 11 == 0 else int(rng.integers(1, 13))
        ph = int(rng.integers(0, 3 * U))
        n = rm.need(U, D, Q, ph, k) + int(rng.integers(0, 3))
        rows.append((int(rng.integers(0, total - n + 1)), ph, n, k, U, D, int(rng.integers(0, 4)), Q * U))
    return Case("resample", shuffled(rm.place(rows), 2), rm.noise(total, 4099), taps=rm.some_taps(64, 4100))


def full_measure_case():
    """MAX_JOBS jobs: up to 120 samples (WAVE), every 64th a few samples more than WAVE_MAX (SPLIT, one chunk) and every 11th none"""
    rng = np.random.default_rng(4101)
    total, rows = mm.WAVE_MAX + 1500, []
    for i in range(MAX_JOBS):
        n = 0 if i % 11 == 0 else mm.WAVE_MAX + 1 + int(rng.integers(0, 100)) if i % 64 == 5 else int(rng.integers(1, 121))
        rows.append((int(rng.integers(0, total - n + 1)), n, 0.3))
    return Case("measure", shuffled(mm.make_jobs(rows), 3), mm.bursty(total, 4102))


def full_demod_case():
    """MAX_JOBS jobs of all modes, L = 1 (DIRECT) and 2, 3, 7 (AVG), up to 40 samples; every 11th has none"""
    rng = np.random.default_rng(4103)
    total, rows = 3000, []
    for i in range(MAX_JOBS):
        n = 0 if i % 11 == 0 else int(rng.integers(1, 41))
        rows.append((int(rng.integers(0, total - n + 1)), n, i % 3, (1, 2, 1, 3, 7)[i % 5]))
    return Case("demod", shuffled(dm.place(rows), 4), dm.noise(total, 4104))


def full_correlate_case():
    """MAX_JOBS jobs of all traces, T = 1, 2, 7, 16, up to 30 lags; every 11th has too few samples for a lag"""
    rng = np.random.default_rng(4105)
    total, rows = 3000, []
    for i in range(MAX_JOBS):
        T = (1, 2, 7, 16)[i % 4]
        n = (T - 1) * (i & 1) if i % 11 == 0 else T - 1 + int(rng.integers(1, 31))
        rows.append((int(rng.integers(0, total - n + 1)), int(rng.integers(0, 40 - T + 1)), n, T, i % 3, 1.5 / T))
    jobs = cm.place(rows)
    odd = (jobs["trace"] == cm.C) & (jobs["out_offset"] & 1 != 0)
    jobs["out_offset"][odd] -= 1				# GUARD keeps the ranges apart all the same
    return Case("correlate", shuffled(jobs, 5), cm.noise(total, 4106), tpl=cm.noise(40, 4107))


FULL = {"extract": full_extract_case, "resample": full_resample_case, "measure": full_measure_case, "demod": full_demod_case,
        "correlate": full_correlate_case, "psd": lambda: from_model("psd", pm.full_table_case()),
        "symbols": lambda: from_model("symbols", sm.full_table_case()),
        "carrier": lambda: from_model("carrier", car.full_table_case()),
        "decide": lambda: from_model("decide", dec.full_table_case())}


def one_job_of(case):
    """the first job of a full table that has work, alone: the small call before and behind the full one"""
    name = case.name
    work = [i for i, j in enumerate(case.jobs) if has_work(name, j) and (name != "psd" or n_out(name, j))]	# psd: one with a trace
    return case.with_jobs(case.jobs[work[0]:work[0] + 1])


# ---- the relocation cases and the far buffer ------------------------------------------------------------------------------------------

FAR_SAMPLES = 2 ** 31 + 2 ** 20				# float2 samples of the far buffer
FAR_BYTES = 8 * FAR_SAMPLES
FAR_FREE_NEEDED = 20 * 2 ** 30
FAR_GUARD = 4096					# sentinel elements either side of a far output range
BASES_FP32 = (2 ** 29 + 16, 2 ** 31 + 16)		# in float2 samples: byte offset beyond 2^32; sample index beyond int32
BASES_16 = BASES_FP32 + (2 ** 32 + 32,)			# in 4-byte samples
# by OUT_BYTES: beyond 2^31 complex outputs, beyond 2^32 floats, beyond byte 2^32 of the buffer
OUT_BASE = {8: 2 ** 31 + 16, 4: 2 ** 32 + 32, 1: 2 ** 32 + 2 ** 16}
TPL_BASE = 2 ** 31 + 48
WIN_BASE = 2 ** 32 + 64					# in floats: inside the buffer's 2^32 + 2^21

RELOCATE = {
    "psd loads": lambda: from_model("psd", pm.loads_case()),
    "psd tiles": lambda: from_model("psd", pm.tiles_case()),
    "symbols loads": lambda: from_model("symbols", sm.loads_case()),
    "symbols pick": lambda: from_model("symbols", sm.pick_case()),
    "carrier loads": lambda: from_model("carrier", car.loads_case()),
    "carrier lag": lambda: from_model("carrier", car.lag_case()),
    "decide offsets": lambda: from_model("decide", dec.offsets_case()),
    "decide windows": lambda: from_model("decide", dec.windows_case()),
    "extract n_out_seams": lambda: from_model("extract", em.cases()["n_out_seams"]),
    "extract first1_fp32": lambda: from_model("extract", em.cases()["first1_fp32"]),
    "extract first3_fp16": lambda: from_model("extract", em.cases()["first3_fp16"]),
    "extract first5_sc16": lambda: from_model("extract", em.cases()["first5_sc16"]),
    "resample counts": lambda: from_model("resample", rm.counts_case()),
    "demod seams": lambda: from_model("demod", dm.seams_case()),
    "correlate lag_counts": lambda: from_model("correlate", cm.lag_counts_case()),
    "measure split_n": lambda: from_model("measure", mm.split_n_case()),
    "measure planted": lambda: from_model("measure", mm.planted_case()),
}


def bases_of(case):
    return BASES_FP32 if sample_bytes(case) == 8 else BASES_16


def aliases(base, unit):
    """where an element at `base` (in units of `unit` bytes) is looked for by code that truncates: the index to 32 and to 31 bits,
    the byte offset to 32 bits -> the distinct element indices other than base itself"""
    found = {base % 2 ** 32, base % 2 ** 31, (base * unit) % 2 ** 32 // unit}
    return sorted(found - {base})


def shifted(case, field, by):
    """the case with `field` of every job (of every job that has an output, for out_offset) moved by `by`"""
    jobs = case.jobs.copy()
    for j in jobs:
        if field != "out_offset" or has_out(case.name, j):
            j[field] += by
    return case.with_jobs(jobs)


# ---- the long extract jobs of the far buffer --------------------------------------------------------------------------------------------

HASH_MUL, HASH_HIGH, HASH_ADD = 0x2545F491, 0x3C6EF35F, 0x7F4A7C15


def hash_words(index):
    """the 32-bit word (an sc16 sample: re in the low half) at 4-byte index `index` of the far buffer, from int64 arithmetic that
    numpy arrays and torch tensors perform alike: index < 2^33 and HASH_MUL < 2^30, so nothing overflows"""
    v = (index * HASH_MUL + (index >> 31) * HASH_HIGH + HASH_ADD) & 0xffffffff	# the bits from 2^31 up count: no alias has the same word
    v = v ^ (v >> 15)
    return (v * 0x9E5 + (v >> 7)) & 0xffffffff


class HashedStream:
    """the sc16 stream of hash_words as extract_model indexes it: x[indices] -> complex128, without the 2^32 samples in memory"""

    def __getitem__(self, index):
        w = hash_words(np.asarray(index, np.int64))
        re, im = (w & 0xffff).astype(np.uint16).view(np.int16), (w >> 16).astype(np.uint16).view(np.int16)
        return re.astype(np.float64) * 2.0 ** -15 + 1j * (im.astype(np.float64) * 2.0 ** -15)


def hashed_bound(job, taps):
    """em.bound with max|x| = sqrt(2), which no sc16 sample exceeds: the stream is too long to look at"""
    t = int(job["n_taps"])
    h = np.asarray(taps, np.float32)[int(job["taps_offset"]):int(job["taps_offset"]) + t].astype(np.float64)
    return (t + 16) * 2.0 ** -24 * np.abs(h).sum() * np.sqrt(2.0)


def advanced(job, m):
    """the job that computes outputs m .. of `job` as its outputs 0 ..: first and phase0 advanced (the cut rule of em.split_case)"""
    out = np.array(job, em.JOB_DTYPE).copy().reshape(1)
    d = int(job["decim"])
    out["first"] = int(job["first"]) + m * d
    out["phase0"] = (int(job["phase0"]) + m * d * int(job["phase_inc"])) % (1 << 32)
    out["n_out"] = int(job["n_out"]) - m
    return out


WAVE_LONG = dict(decim=1024, n_taps=3, n_out=2 ** 22 + 9, first=5, phase_inc=0x1234567b, phase0=0xfffffff0)
TILE_LONG = dict(decim=25, n_taps=33, n_out=-(-2 ** 31 // 25) + 600, first=3, phase_inc=0x0f1e2d3d, phase0=0xdeadbeef)


def long_extract_job(spec, out_offset):
    job = np.zeros(1, em.JOB_DTYPE)
    for k, v in spec.items():
        job[k] = v
    job["out_offset"] = out_offset
    return job


# ---- the long psd and symbols jobs of the far buffer: periodic input ----------------------------------------------------------------------

PERIOD = 3 * 2 ** 18					# float2 samples of the noise block the far buffer repeats
LONG_N = 2 ** 31 - 1
PSD_LONG = dict(fft_len_log=10, hop=1024, offset=1, n=LONG_N)		# 2^21 - 1 segments, 2^16 tiles, 512 MiB of partials
PSD_LONG_PARTS = dict(fft_len_log=10, hop=128, offset=1, n=LONG_N)	# 2^24 - 8 segments, 2^19 tiles, 4 GiB of partials
# the FIXED job begins 1024 samples further in, so that it ends beyond sample 2^31 and a short job of its last symbols begins there
SYM_LONG = {"sps 64": dict(sps=64, mode=sm.ESTIMATE, tau=0.0, offset=1, n=LONG_N),
            "sps 3": dict(sps=3, mode=sm.FIXED, tau=0.4, offset=1025, n=LONG_N)}


def long_psd_job(spec, out_offset=GUARD, win_offset=0):
    return pm.make_jobs([(spec["offset"], out_offset, win_offset, spec["n"], spec["fft_len_log"], spec["hop"], pm.NONE, pm.T_POWER,
                          0.99, 1e-2)])


def long_symbols_job(spec, out_offset=GUARD):
    return sm.make_jobs([(spec["offset"], out_offset, spec["n"], spec["sps"], spec["mode"], spec["tau"])])


def advanced_symbols(job, m):
    """the FIXED job that computes symbols m .. of `job` as its symbols 0 ..: offset advanced by m sps, n shortened by as much (the
    phase is the job's own tau, so first and mu stay)"""
    out = np.array(job, sm.JOB_DTYPE).copy().reshape(1)
    assert out["mode"][0] == sm.FIXED
    out["offset"] += m * int(job["sps"])
    out["n"] -= m * int(job["sps"])
    return out


def wrapped(block, first, count):
    """samples first .. first + count of `block` repeated for ever"""
    return block[(first + np.arange(count, dtype=np.int64)) % len(block)]


def serial_sum(distinct, count, last=None):
    """rows 0, 1, .. count - 1 of `distinct` taken cyclically, then `last` if there is one, added one after the other in that order
    from 0.0 -> float64 [K]"""
    distinct = np.asarray(distinct, np.float64)
    S = np.zeros(distinct.shape[1])
    with np.errstate(all="ignore"):
        for c in range(count):
            S = S + distinct[c % len(distinct)]
        if last is not None:
            S = S + last
    return S


def periodic_psd(block, win, job):
    """the psd job over `block` repeated for ever, len(block) a multiple of the tile stride TILE hop: tile c of the job is tile
    c mod (len(block) / stride).  Those distinct full tiles and the last, partial one by psd_model's functions, added in rule 4's
    order -> (a RECORD_DTYPE array [1], the trace float32 [L] or [0])"""
    block, win = pm.buffers((block, win))
    log, hop, nseg = int(job["fft_len_log"]), int(job["hop"]), pm.job_n_seg(job)
    L, stride = 1 << log, pm.TILE * hop
    assert len(block) % stride == 0
    full, rest = divmod(nseg, pm.TILE)

    def tile(c, segs):
        y = wrapped(block, int(job["offset"]) + c * stride, (segs - 1) * hop + L)
        p = pm.powers(y, win, np.arange(segs, dtype=np.int64) * hop, np.full(segs, int(job["win_offset"]), np.int64),
                      np.full(segs, int(job["pre"])), L)
        with np.errstate(all="ignore"):
            return pm.ordered_sum(p)

    S = None
    if nseg:
        distinct = [tile(c, pm.TILE) for c in range(min(len(block) // stride, full))] or np.zeros((1, L))
        S = serial_sum(distinct, full, tile(full, rest) if rest else None)
    record, P32 = pm.result_of(job, S, win)
    return record, (P32 if P32 is not None and int(job["trace"]) == pm.T_POWER else np.zeros(0, np.float32))


def periodic_symbols(block, job):
    """the symbols job over `block` repeated for ever, len(block) a multiple of the tile stride TILE sps: fold tile and output tile
    c are those of c mod (len(block) / stride).  The distinct full tiles and the last, partial ones by symbols_model's functions,
    added in the order of rules 1 and 6 -> (a RECORD_DTYPE array [1], the symbols of the first len(block) / sps (or of all, if
    there are fewer) float32 [..][2], the symbols of the last, partial output tile float32 [..][2])"""
    block = sm.buffer((block,))
    sps, n, off = int(job["sps"]), int(job["n"]), int(job["offset"])
    stride = sm.TILE * sps
    assert len(block) % stride == 0
    cycle = len(block) // stride
    xyz = None
    if int(job["mode"]) == sm.ESTIMATE:
        full, rest = divmod(n // sps, sm.TILE)

        def fold(c, syms):
            y = wrapped(block, off + c * stride, syms * sps).astype(np.float64)
            with np.errstate(all="ignore"):
                return sm.three_level(((y[:, 0] * y[:, 0]) + (y[:, 1] * y[:, 1])).reshape(syms, sps))

        distinct = [fold(c, sm.TILE) for c in range(min(cycle, full))] or np.zeros((1, sps))
        xyz = sm.line_of(serial_sum(distinct, full, fold(full, rest) if rest else None), sps)
    r = sm.timing_of(job, xyz)
    none = np.zeros((0, 2), np.float32)
    if r["status"][0] == sm.NO_TIMING:
        return r, none, none
    first, mu = int(r["first"][0]), r["mu"][0]
    full, rest = divmod(int(r["n_sym"][0]), sm.TILE)

    def pick(c, syms):
        return sm.interpolate(wrapped(block, off + c * stride, first + (syms - 1) * sps + 3), first, mu, syms, sps)

    outs = [pick(c, sm.TILE) for c in range(min(cycle, full))]
    last = pick(full, rest) if rest else none
    m = serial_sum([sm.moments(o) for o in outs] or np.zeros((1, len(sm.MOMENTS))), full, sm.moments(last) if rest else None)
    for k, v in zip(sm.MOMENTS, m):
        r[k] = sm.quiet64(v)
    return r, (np.concatenate(outs) if outs else last), last


# ---- the long carrier and decide jobs of the far buffer ---------------------------------------------------------------------------------

CAR_LONG_A = 37						# the fixed frequency is CAR_LONG_A / 2^12 turns a symbol, the block's own carrier
CAR_LONG_FREQ = CAR_LONG_A / 2.0 ** 12
CAR_LONG_PHASE = 1.0 / 8 + 1.0 / 1024
CAR_LONG = {"C": dict(order=4, mode=car.FREQ_FIXED | car.PHASE_FIXED, lag=16, freq=CAR_LONG_FREQ, phase=CAR_LONG_PHASE, offset=1, n=LONG_N),
            "D": dict(order=4, mode=car.FREQ_FIXED, lag=16, freq=CAR_LONG_FREQ, phase=0.0, offset=1, n=LONG_N),
            "E": dict(order=4, mode=car.ESTIMATE, lag=16, freq=0.0, phase=0.0, offset=1, n=LONG_N)}
CAR_E_FIELDS = ("n", "order", "lag_used", "status", "freq", "r1_re", "r1_im", "rl_re", "rl_im", "m2", "mm")	# what job E has a model of
DEC_LONG_WORD = 16					# symbols of the far jobs' word
DEC_LONG_AT = 100000					# where job A's word is cut from the block's first period, job-relative
DEC_LONG = {"A": dict(order=4, flags=dec.UW, offset=1, n=LONG_N, uw_first=0),
            "B": dict(order=4, flags=dec.UW | dec.DIFF, offset=1, n=LONG_N, uw_first=LONG_N - DEC_LONG_WORD - 600)}


def carrier_block(order=4):
    """PERIOD symbols of a PSK whose carrier turns by CAR_LONG_FREQ a symbol -- a whole number of turns a period, so the block
    repeated is one continuous burst -- in 30 dB of noise"""
    return car.psk(PERIOD, order, CAR_LONG_FREQ, 0.02, 7373, 30.0)


def decide_block(order=4):
    """PERIOD symbols of a planted PSK turned by 1 / M turns in 30 dB of noise"""
    return dec.psk(PERIOD, order, 0.0, 1.0 / order + 0.01 / order, 7474, 30.0)


def long_carrier_job(spec, out_offset=GUARD):
    return car.make_jobs([(spec["offset"], out_offset, spec["n"], spec["order"], spec["mode"], spec["lag"], spec["freq"], spec["phase"])])


def long_decide_job(spec, block, out_offset=dec.GUARD):
    """-> (the job, its word).  Job A's word: the DEC_LONG_WORD decisions at DEC_LONG_AT of the first period, less 1 (uw_rot = 1).
    Job B's: the differences at a position of the job's last group"""
    n, M, flags, off = spec["n"], spec["order"], spec["flags"], spec["offset"]
    L = DEC_LONG_WORD
    p = n - L - 50 if flags & dec.DIFF else DEC_LONG_AT
    k = dec.decisions(wrapped(block, off + p - 1, L + 1), M)[0]
    word = ((k[1:] - k[:-1]) if flags & dec.DIFF else (k[1:] - 1)) & (M - 1)
    return dec.make_jobs([(off, out_offset, n, M, flags, 0, L, spec["uw_first"], 0, 0)]), word.astype(np.uint8)


def exact_products(job):
    """are g j and theta + f j of a carrier job with fixed frequency and phase exact up to its last symbol?  Then, with g TILE a
    whole number, both repeat every TILE symbols but for whole turns, which fosphor_amd_cossin_turns takes off exactly (t -
    floor(t)), and the job over a periodic buffer is periodic"""
    Fr = fractions.Fraction
    M = int(job["order"])
    f = Fr(float(job["freq"]))
    g = Fr(float(np.float64(job["freq"]) * np.float64(M)))
    ok = g == f * M and Fr(float(g / M)) == f and (g * car.TILE).denominator == 1 and (f * car.TILE).denominator == 1
    for j in (1, car.TILE - 1, 2 ** 30 + 1, int(job["n"]) - 1):
        ok = ok and Fr(float(np.float64(float(g)) * np.float64(j))) == g * j
        if int(job["mode"]) & car.PHASE_FIXED:
            th = Fr(float(job["phase"]))
            ok = ok and Fr(float(np.float64(float(th)) + (np.float64(float(f)) * np.float64(j)))) == th + f * j
    return bool(ok)


def more_tiles(S, tiles):
    """S and then every row of `tiles`, one after the other"""
    with np.errstate(all="ignore"):
        for t in tiles:
            S = S + t
    return S


def periodic_carrier(block, job):
    """the carrier job over `block` repeated for ever, len(block) a multiple of TILE: tile c of the lag terms and of the symbols sees
    the samples of tile c mod (len(block) / TILE).  Lag tile c is periodic as long as all its terms of lag Le exist ((c + 1) TILE +
    Le <= n); those tiles and every later one by carrier_model's functions, added in the order of rule 2.  The sums w and |s|^M of
    rule 5 are periodic as they stand; its Z only where g j repeats every TILE symbols (exact_products): the tile of symbol j is
    computed with j mod len(block), so for another g the model's z_re, z_im and phase are not the job's -- ESTIMATE at this length
    has no model of them, and the caller compares CAR_E_FIELDS alone.
    -> a RECORD_DTYPE array [1]"""
    block = car.buffer((block,))
    n, M, mode, L, off = int(job["n"]), int(job["order"]), int(job["mode"]), int(job["lag"]), int(job["offset"])
    T, P = car.TILE, len(block)
    assert P % T == 0
    cycle = P // T
    r = np.zeros(1, car.RECORD_DTYPE)
    r["n"], r["order"] = n, M
    if mode & car.FREQ_FIXED:
        g = np.float64(job["freq"]) * np.float64(M)
    else:
        Le = car.lag_used(n, L)

        def lag_tile(c):
            """the four sums of the lag terms c TILE .. of the job"""
            j0 = c * T
            terms = min(n - 1 - j0, T)
            pr, pi, _, _ = car.power(wrapped(block, off + j0, min(terms + Le, n - j0)), M)
            t = np.zeros((terms, 4))
            with np.errstate(all="ignore"):
                ar, ai, br, bi = pr[1:terms + 1], pi[1:terms + 1], pr[:terms], pi[:terms]
                t[:, 0], t[:, 1] = (ar * br) + (ai * bi), (ai * br) - (ar * bi)
                tl = max(min(n - Le - j0, terms), 0) if Le > 1 else 0
                ar, ai, br, bi = pr[Le:Le + tl], pi[Le:Le + tl], pr[:tl], pi[:tl]
                t[:tl, 2], t[:tl, 3] = (ar * br) + (ai * bi), (ai * br) - (ar * bi)
                return car.three_level(t)			# one tile: the third level adds it to 0.0

        tiles = -(-max(n - 1, 0) // T)
        whole = min(max((n - Le) // T, 0), tiles)
        distinct = [lag_tile(c) for c in range(min(cycle, whole))] or np.zeros((1, 4))
        R = more_tiles(serial_sum(distinct, whole), [lag_tile(c) for c in range(whole, tiles)])
        r["lag_used"] = Le
        r["r1_re"], r["r1_im"], r["rl_re"], r["rl_im"] = (car.quiet64(v) for v in R)
        g = car.frequency(tuple(R), Le)
        if g is None:
            r["status"], r["freq"], r["phase"] = car.NO_CARRIER, car.QNAN64, car.QNAN64
            return r
    f = g / np.float64(M)
    full, rest = divmod(n, T)

    def sum_tile(c, syms):
        j0 = (c % cycle) * T
        return car.phase_sums(*car.power(wrapped(block, off + j0, syms), M), g, j0)

    distinct = [sum_tile(c, T) for c in range(min(cycle, full))] or np.zeros((1, 4))
    Z = serial_sum(distinct, full, sum_tile(full, rest) if rest else None)
    r["z_re"], r["z_im"], r["m2"], r["mm"] = (car.quiet64(v) for v in Z)
    if mode & car.PHASE_FIXED:
        theta = np.float64(job["phase"])
    else:
        thM = dm.atan2_turns(Z[1], Z[0])
        if np.isnan(thM):
            r["status"], r["freq"], r["phase"] = car.NO_CARRIER, car.QNAN64, car.QNAN64
            return r
        theta = np.float64(thM) / np.float64(M)
    r["freq"], r["phase"] = f, theta
    return r


def carrier_symbols(block, job, record, j0, count):
    """the derotated symbols j0 .. j0 + count of the job over `block` repeated, by rule 6 with the true index j"""
    return car.derotate(wrapped(car.buffer((block,)), int(job["offset"]) + j0, count), record["phase"][0], record["freq"][0], j0)


def periodic_decide(block, job, uw):
    """the decide job over `block` repeated for ever, len(block) a multiple of TILE.  A decision and its terms of rule 2 do not
    depend on j, so tile c is tile c mod (len(block) / TILE): the distinct tiles and the last, partial one by decide_model's
    functions, their sums added in the order of rule 2, their counts as integers.  The differences repeat from d[1] on.  The search
    of rule 4 runs over the first len(block) candidates: a later candidate sees the decisions of the one len(block) before it,
    which is a candidate too, so it repeats that one's key with a larger p and cannot win -- the result is exact.
    -> (a RECORD_DTYPE array [1], bytes(j0, count): the bytes of symbols j0 .. j0 + count of the job as the record's rotation
    leaves them, uint8)"""
    block = dec.buffer((block,))
    n, M, flags, off = int(job["n"]), int(job["order"]), int(job["flags"]), int(job["offset"])
    T, P = dec.TILE, len(block)
    assert P % T == 0
    cycle = P // T
    full, rest = divmod(n, T)

    def tile(c, syms):
        y = wrapped(block, off + (c % cycle) * T, syms)
        k, erased = dec.decisions(y, M)
        return dec.three_level(dec.terms(y, k, M)), np.concatenate([np.bincount(k, minlength=8), [int(erased.sum())]])

    tiles = [tile(c, T) for c in range(min(cycle, full))]
    last = tile(full, rest) if rest else None
    S = serial_sum([t[0] for t in tiles] or np.zeros((1, 3)), full, last[0] if rest else None)
    counts = np.zeros(9, np.int64)
    if tiles:
        per = np.array([t[1] for t in tiles], np.int64)
        counts += (full // len(tiles)) * per.sum(0) + per[:full % len(tiles)].sum(0)
    if rest:
        counts += last[1]
    r = np.zeros(1, dec.RECORD_DTYPE)
    r["n"], r["order"], r["flags"], r["uw_pos"] = n, M, flags, -1
    r["erasures"], r["hist"][0] = counts[8], counts[:8]
    r["a"], r["b"], r["m2"] = (dec.quiet64(v) for v in S)
    diff = 1 if flags & dec.DIFF else 0

    def differences(j0, count):
        """d[j0 .. j0 + count] of the job"""
        before = 1 if diff and j0 else 0
        k = dec.decisions(wrapped(block, off + j0 - before, count + before), M)[0]
        if not diff:
            return k
        d = (k[1:] - k[:-1]) & (M - 1)
        return d if before else np.concatenate([k[:1], d])

    if flags & dec.UW:
        L = int(job["uw_len"])
        u = np.asarray(uw, np.int64)[int(job["uw_offset"]):int(job["uw_offset"]) + L]
        first, count = dec.candidates(job)
        r["uw_errors"] = L
        if count:
            seen = min(count, P)
            pos, rot, matches = dec.find_word(differences(first, seen + L - 1), u, M, flags, 0, seen)
            r["uw_pos"], r["uw_rot"], r["uw_errors"] = first + pos, rot, L - matches
        if not count or r["uw_errors"][0] > int(job["uw_max_errors"]):
            r["status"] = dec.NO_UW
    rot = int(r["uw_rot"][0])

    def out_bytes(j0, count):
        q = (differences(j0, count) - rot) & (M - 1)
        return (q ^ (q >> 1) if flags & dec.GRAY else q).astype(np.uint8)

    return r, out_bytes


CASES = dict(RELOCATE)
CASES.update({"long measure": long_measure_case, "long edges": long_edges_case, "long tie": long_tie_case,
              "long resample": long_resample_case, "long psd": long_psd_case, "long symbols": long_symbols_case,
              "long carrier": long_carrier_case, "long decide": long_decide_case, "long decide words": lambda: long_decide_words()[0]})
CASES.update({"full " + k: v for k, v in FULL.items()})


# ---- driving the passes on the device (torch is imported where it is used: the CPU tests import this file too) ----------------------

class Dev:
    """an instance, torch views of its waterfall ring and spectrum, and the nine passes through the C ABI by raw device pointers"""

    def __init__(self, amd, wf_rows=16):
        self.f = amd.Fosphor(n_bins=128, wf_rows=wf_rows)
        self.n, self.wf_rows = self.f.n, wf_rows
        assert self.f.finish() >= 0			# a new instance fills its buffers at its first wait

    def views(self):
        import torch
        from gr_fosphor_amd.dist import wrap_device_array
        b = self.f.buffers(False)
        assert (b.fft_len, b.wf_rows) == (self.n, self.wf_rows)
        self.pos = b.waterfall_pos
        self.wf = wrap_device_array(b.d_waterfall, (self.wf_rows, self.n), torch.float32)
        self.spec = wrap_device_array(b.d_spectrum, (2, self.n, 2), torch.float32)

    def save(self):
        import torch
        assert self.f.finish() >= 0
        self.views()
        self.saved = (self.wf.view(torch.int32).clone(), self.spec.view(torch.int32).clone(), self.pos)
        torch.cuda.synchronize()

    def assert_untouched(self):
        import torch
        torch.cuda.synchronize()
        self.views()
        assert self.pos == self.saved[2], "the ring position moved"
        assert torch.equal(self.wf.view(torch.int32), self.saved[0]), "the waterfall was written"
        assert torch.equal(self.spec.view(torch.int32), self.saved[1]), "the spectrum lines were written"

    def call(self, name, jobs, fmt, iq, n_iq, out=None, cap=0, taps=None, n_taps=0, tpl=None, n_tpl=0, rec=None, win=None, n_win=0,
             uw=None, tag=""):
        """one call that must succeed, every buffer a device pointer (uw: decide's table, a host array): the ring, the waterfall
        and the spectrum untouched and the stats delta what the jobs predict (symbols: the jobs and the n_sym of the records it
        wrote)"""
        import torch
        jobs = np.ascontiguousarray(jobs, MODELS[name].JOB_DTYPE)
        self.save()
        torch.cuda.synchronize()			# the fills and uploads run on torch's stream, the pass on the instance's
        L, h, stats = self.f.L, self.f.h, getattr(self.f, name + "_stats")
        before = stats()
        if name == "extract":
            rv = L.fosphor_amd_extract(h, iq, n_iq, fmt, jobs.ctypes.data, len(jobs), taps, n_taps, out, cap)
        elif name == "resample":
            rv = L.fosphor_amd_resample(h, iq, n_iq, jobs.ctypes.data, len(jobs), taps, n_taps, out, cap)
        elif name == "measure":
            rv = L.fosphor_amd_measure(h, iq, n_iq, jobs.ctypes.data, len(jobs), rec)
        elif name == "demod":
            rv = L.fosphor_amd_demod(h, iq, n_iq, jobs.ctypes.data, len(jobs), out, cap)
        elif name == "psd":
            rv = L.fosphor_amd_psd(h, iq, n_iq, win, n_win, jobs.ctypes.data, len(jobs), rec, out, cap)
        elif name == "symbols":
            rv = L.fosphor_amd_symbols(h, iq, n_iq, jobs.ctypes.data, len(jobs), rec, out, cap)
        elif name == "carrier":
            rv = L.fosphor_amd_carrier(h, iq, n_iq, jobs.ctypes.data, len(jobs), rec, out, cap)
        elif name == "decide":
            n_uw = 0 if uw is None else len(uw)
            rv = L.fosphor_amd_decide(h, iq, n_iq, jobs.ctypes.data, len(jobs), uw.ctypes.data if n_uw else None, n_uw, rec, out, cap)
        else:
            rv = L.fosphor_amd_correlate(h, iq, n_iq, tpl, n_tpl, jobs.ctypes.data, len(jobs), rec, out, cap)
        after = stats()
        self.assert_untouched()
        assert rv == 0, (tag, name, rv)
        delta = {k: after[k] - before[k] for k in after}
        records = None
        if name == "symbols":
            from gr_fosphor_amd.dist import wrap_device_array
            records = wrap_device_array(rec, (len(jobs) * sm.RECORD_WORDS,), torch.int32).cpu().numpy().view(sm.RECORD_DTYPE)
        assert delta == expected_stats(name, jobs, records), (tag, name, delta)

    def run(self, case, tag="", iq_at=None, out_at=None, tpl_at=None, win_at=None):
        """the case in sentinel-filled buffers of its own -> (records or None, the whole output buffer as uint32 words or None);
        inputs, taps and windows are compared with their host copies afterwards.
        iq_at, tpl_at: (device pointer, samples there, base): the case's samples or templates lie there from `base` on already --
        the jobs' offsets are moved by base, and the caller looks after that buffer.
        win_at: (device pointer, floats there, base): the same for psd's windows and win_offset.
        out_at: (device pointer, capacity there, base): the outputs go there, out_offset moved by base; no words are returned."""
        import torch
        name, jobs = case.name, case.jobs
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int16)).cuda()
        held = {}
        if iq_at is None:
            held["iq"] = (up(case.iq if len(case.iq) else np.zeros((1, 2), case.iq.dtype)), case.iq)
            iq, n_iq = held["iq"][0].data_ptr(), len(case.iq)
        else:
            iq, n_iq = iq_at[0], iq_at[1]
            jobs = shifted(case, IN_FIELD[name], iq_at[2]).jobs
        taps = n_taps = tpl = n_tpl = rec = d_rec = out = d_out = win = n_win = None
        if case.taps is not None:
            held["taps"] = (up(case.taps), case.taps)
            taps, n_taps = held["taps"][0].data_ptr(), len(case.taps)
        if name == "psd":
            if win_at is not None:
                win, n_win = win_at[0], win_at[1]
                jobs = shifted(case.with_jobs(jobs), "win_offset", win_at[2]).jobs
            else:
                held["win"] = (up(case.win), case.win)
                win, n_win = held["win"][0].data_ptr(), len(case.win)
        if name == "correlate":
            if tpl_at is not None:
                tpl, n_tpl = tpl_at[0], tpl_at[1]
                jobs = shifted(case.with_jobs(jobs), "tpl_offset", tpl_at[2]).jobs
            elif case.tpl is None:
                tpl, n_tpl = iq, n_iq
                if iq_at is not None:
                    jobs = shifted(case.with_jobs(jobs), "tpl_offset", iq_at[2]).jobs
            else:
                held["tpl"] = (up(case.tpl), case.tpl)
                tpl, n_tpl = held["tpl"][0].data_ptr(), len(case.tpl)
        if name in WITH_RECORDS:
            words = MODELS[name].RECORD_DTYPE.itemsize // 4
            d_rec = torch.full(((len(jobs) + 2 * GUARD) * words,), SENTINEL, dtype=torch.int32, device="cuda")
            rec = d_rec.data_ptr() + 4 * GUARD * words
        cap = capacity(name, jobs)
        if out_at is not None:
            out, cap = out_at[0], out_at[1]
            jobs = shifted(case.with_jobs(jobs), "out_offset", out_at[2]).jobs
        elif OUT_BYTES[name]:
            d_out = torch.full((out_words(name, cap) + 2,), SENTINEL, dtype=torch.int32, device="cuda")
            out = d_out.data_ptr()
        self.call(name, jobs, case.fmt, iq, n_iq, out=out, cap=cap, taps=taps, n_taps=n_taps or 0, tpl=tpl, n_tpl=n_tpl or 0, rec=rec,
                  win=win, n_win=n_win or 0, uw=case.uw, tag=tag)
        for k, (d, host) in held.items():
            assert d.cpu().numpy().tobytes() == host.tobytes(), (tag, "the %s buffer was written" % k)
        got = words_out = None
        if d_rec is not None:
            r = d_rec.cpu().numpy().view(np.uint32).reshape(len(jobs) + 2 * GUARD, -1)
            assert np.all(r[:GUARD] == SENTINEL) and np.all(r[-GUARD:] == SENTINEL), (tag, "written outside the records")
            got = r[GUARD:-GUARD].copy().view(MODELS[name].RECORD_DTYPE).reshape(-1)
        if d_out is not None:
            w = d_out.cpu().numpy().view(np.uint32)
            assert np.all(w[-2:] == SENTINEL), (tag, "written behind the capacity")
            words_out = w[:-2].copy()
        return got, words_out
