"""The passes over burst IQ far into a buffer: inputs, outputs and templates beyond byte 2^32 and beyond sample 2^31, and extract
jobs whose positions inside the job pass 2^31 and 2^32 (the input sets and the geometry are tests/job_scale_cases.py;
tests/test_job_scale_cpu.py holds the conditions on them).

One module-scoped device buffer of 2^31 + 2^20 float2 samples, about 16.01 GiB, allocated uninitialised; the module is skipped
only where less than 20 GiB of device memory is free, with both numbers in the reason.

  relocation    a case of every pass runs near, in buffers of its own, and far: the same bytes copied into the buffer at a base
                (a multiple of 16 samples, so every head / tail split of the loads is the one of the near run) and every job's
                input offset moved by the base.  Decoy data lies where a truncated index or byte offset would look
                (jc.aliases).  The far results are bit-identical to the near ones -- also for extract and measure: their kernels
                have no atomics, and no order of their additions depends on an address beyond its low four bits -- and the near
                ones are held to the model as everywhere.
  far outputs   the buffer as d_out with a small input of its own: out_offset beyond 2^31 complex outputs (extract, resample,
                symbols, carrier), beyond 2^32 floats (demod, correlate, psd) and beyond byte 2^32 (decide, whose out_offset counts
                bytes); FAR_GUARD sentinel elements either side of the range and the same at the aliases of the output offset, all
                checked afterwards.  One run with the buffer as correlate's d_tpl.
  long extract  WAVE: D = 1024, T = 3 over a span of 2^32 + 8195 sc16 samples, phase0 near 2^32; exactly the samples it reads
                are written, from a hash of the index that numpy recomputes.  TILE: D = 25, T = 33, base = m0 * D beyond 2^31,
                input and output in disjoint regions of the buffer; the tiles at the ends and on both sides of 2^31 against the
                model, every output word written (a sentinel count on the device), the last outputs bit-identical to a short
                job advanced to there (the cut rule of extract_model.split_case).
  windows       psd's windows at WIN_BASE, beyond 2^32 floats, decoys at its aliases: bit-identical to the near run.
  long psd      one job of n = 2^31 - 1 samples at L = 1024 over the buffer filled with one noise block of PERIOD samples, repeated
                (jc.periodic_psd says how that makes a model possible): hop 1024 is 2^21 - 1 segments in 2^16 tiles; hop 128 is
                2^24 - 8 segments in 2^19 tiles, whose partials take 2^32 bytes of the scratch behind the table, so the last
                tile's lie beyond byte 2^32 of it.  Record and trace bit-identical to the model, the input unchanged (every row of
                the buffer as [k][PERIOD] against the first, on the device).
  long symbols  n = 2^31 - 1 at sps 64 under ESTIMATE (2^13 fold tiles) and at sps 3 under FIXED (174763 output tiles, 5.4 GiB of
                symbols): the record bit-identical to jc.periodic_symbols, every period of the output equal to the first on the
                device, the first period and the last tile equal to the model's, sentinels either side; the FIXED job's last 64
                symbols from a short job that begins beyond sample 2^31.
  long decide   n = 2^31 - 1 planted QPSK symbols over the periodic buffer, a word of 16 symbols.  Job A: no DIFF, every position
                a candidate (2^23 groups of k_dec_uw, 2^17 trips of a lane of k_dec_job): the record bit-identical to
                jc.periodic_decide -- the sums of 2^19 tiles, hist, erasures, uw_pos the word's first occurrence, uw_rot 1 --,
                every period of the output bytes equal to the first on the device, the first period and the last tile equal to
                the model's, the one byte behind the last symbol 0, sentinels either side.  Job B: DIFF, the window is the last
                601 positions, the word lies in the last group at a position above 2^31 - 700: the last work-group of k_dec_uw
                has lo + span = n, where the count of words it loads was formed as (lo + span + 3) >> 2 in int before this job
                existed (now ((lo + span - 1) >> 2) + 1; the unfixed line was never run at this length).  Byte 0 is no difference,
                so period 0 is held to the model and the periods from 1 on to period 1.
  long carrier  n = 2^31 - 1 QPSK symbols with a carrier of 37 / 2^12 turns a symbol over the periodic buffer, 2^19 sum tiles and
                2^19 lag tiles.  Job C: frequency and phase fixed and dyadic, so g j and theta + f j are exact and repeat every
                4096 symbols (jc.exact_products): the record bit-identical to jc.periodic_carrier, every period of the output
                equal to the first, the first period and the last tile equal to the model's.  Job D: the frequency fixed, the
                phase estimated: the record bit-identical; theta + f j rounds, so the output is not periodic: the first two tiles,
                the two either side of j = 2^30 and the last against carrier_model.derotate with the true j.  Job E: ESTIMATE --
                every lag tile is periodic: n, order, lag_used, status, freq, r1_*, rl_*, m2 and mm bit-identical; z_*, phase
                and the output depend on g j with a g that is not dyadic and have no model at this length: not compared (jobs C
                and D carry k_car_sum and k_car_turn at this length, job E is there for k_car_lag and k_car_freq).
Measured once on an MI355X, the call alone and in brackets the whole test with its fills, its model and its comparisons:
PSD_LONG 0.55 s (0.84 s), PSD_LONG_PARTS 3.55 s (4.29 s), symbols at sps 3 0.02 s (0.12 s), at sps 64 0.01 s (0.06 s).
Decide A 0.21 s (0.65 s), decide B 0.15 s (0.50 s), carrier C 0.06 s (0.85 s), carrier D 0.06 s (0.32 s), carrier E 0.11 s (0.56 s):
all far below the 5 s at which a job would have been shortened, so all five run at n = 2^31 - 1.  The decide jobs want 2 GiB of
output and about 2.1 GiB of scratch, the carrier jobs 16 GiB of output beside the buffer; each is skipped, with both numbers in the
reason, where that much more was not free when the buffer was taken.
PSD_LONG_PARTS wants 4 GiB of scratch and the sps 3 job 5.4 GiB of symbols beside the buffer: each is skipped, with both numbers in
the reason, where that much more was not free when the buffer was taken."""
import os
import time

import numpy as np
import pytest

import carrier_model as car
import decide_model as dec
import extract_model as em
import job_scale_cases as jc
import psd_model as pm
import symbols_model as sm

pytestmark = pytest.mark.gpu

SENTINEL = jc.SENTINEL
G = jc.FAR_GUARD
WITH_OUTPUT = sorted(k for k in jc.RELOCATE if jc.OUT_BYTES[k.split()[0]])


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


class Far:
    """the far buffer as 32-bit words"""

    def __init__(self, torch):
        self.torch = torch
        self.big = torch.empty((jc.FAR_SAMPLES, 2), dtype=torch.float32, device="cuda")
        self.words = self.big.view(torch.int32).view(-1)
        self.ptr = self.big.data_ptr()
        assert self.words.numel() == jc.FAR_BYTES // 4 and self.ptr % 16 == 0

    def put(self, at, host):
        """host words (uint32) to words at ..."""
        self.words[at:at + len(host)].copy_(self.torch.from_numpy(host.view(np.int32)).cuda())

    def get(self, at, n):
        return self.words[at:at + n].cpu().numpy().view(np.uint32)

    def fill(self, at, n, value=SENTINEL):
        self.words[at:at + n].fill_(value)

    def count(self, at, n, value=SENTINEL):
        return int((self.words[at:at + n] == value).sum().item())

    def hashed(self, at, n):
        """jc.hash_words of the word indices at .. at + n, as int32"""
        torch = self.torch
        v = jc.hash_words(torch.arange(at, at + n, dtype=torch.int64, device="cuda"))
        return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


@pytest.fixture(scope="module")
def far():
    import torch
    free, total = torch.cuda.mem_get_info()
    if free < jc.FAR_FREE_NEEDED:
        pytest.skip("the far buffer takes %d bytes and wants %d free: %d of %d bytes are" % (jc.FAR_BYTES, jc.FAR_FREE_NEEDED, free, total))
    print("device memory: %d of %d bytes free; the far buffer takes %d" % (free, total, jc.FAR_BYTES))
    f = Far(torch)
    f.free = free					# before the buffer was taken: what the tests that want more go by
    yield f
    f.words = f.big = None
    torch.cuda.empty_cache()


def words_of(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def decoy_of(data):
    """other samples of the same kind: the case's in reverse order with one bit of every 16 flipped"""
    return np.ascontiguousarray(data[::-1]) ^ np.uint32(0x00100010)


def same(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("key", sorted(jc.RELOCATE))
def test_relocated_input(dev, far, key):
    case, model = jc.case_of(key), jc.model_of(key)
    near = dev.run(case, tag=key)
    model.check(*near, tag=key)
    unit = jc.sample_bytes(case)
    per = unit // 4						# words of a sample
    data = words_of(case.iq)
    decoy = decoy_of(data)
    assert not np.array_equal(decoy, data)
    for base in jc.bases_of(case):
        found = jc.aliases(base, unit)
        for a in found:
            far.put(a * per, decoy)
        far.put(base * per, data)
        got = dev.run(case, tag="%s at %d" % (key, base), iq_at=(far.ptr, jc.FAR_BYTES // unit, base))
        assert same(got, near), (key, base, "the far run differs from the near one")
        model.check(*got, tag=key)
        assert far.get(base * per, len(data)).tobytes() == data.tobytes(), "the input was written"
        for a in found:
            assert far.get(a * per, len(decoy)).tobytes() == decoy.tobytes(), "a decoy was written"


@pytest.mark.parametrize("key", WITH_OUTPUT)
def test_relocated_output(dev, far, key):
    case = jc.case_of(key)
    near = dev.run(case, tag=key)
    jc.model_of(key).check(*near, tag=key)
    unit = jc.OUT_BYTES[case.name]				# bytes of an output element: 8, 4, or decide's 1
    w = lambda elements: jc.out_words(case.name, elements)	# every base, guard and capacity here is a whole number of words
    base, cap = jc.OUT_BASE[unit], jc.capacity(case.name, case.jobs)
    spans = [(max(a - G, 0), a + cap + G) for a in jc.aliases(base, unit)]
    for a, b in spans + [(base - G, base + cap + G)]:
        far.fill(w(a), w(b - a))
    rec, _ = dev.run(case, tag=key + " far out", out_at=(far.ptr, jc.FAR_BYTES // unit, base))
    got = far.get(w(base - G), w(cap + 2 * G))
    assert np.all(got[:w(G)] == SENTINEL) and np.all(got[-w(G):] == SENTINEL), "written beside the far range"
    assert got[w(G):-w(G)].tobytes() == near[1].tobytes(), "the far outputs differ from the near ones"
    assert same((rec,), near[:1])
    for a, b in spans:
        assert far.count(w(a), w(b - a)) == w(b - a), "written at an alias of the output offset"


def test_relocated_templates(dev, far):
    key = "correlate lag_counts"
    case = jc.case_of(key)
    near = dev.run(case, tag=key)
    data = words_of(case.tpl)
    decoy = decoy_of(data)
    found = jc.aliases(jc.TPL_BASE, 8)
    for a in found:
        far.put(2 * a, decoy)
    far.put(2 * jc.TPL_BASE, data)
    got = dev.run(case, tag=key + " far templates", tpl_at=(far.ptr, jc.FAR_SAMPLES, jc.TPL_BASE))
    assert same(got, near)
    assert far.get(2 * jc.TPL_BASE, len(data)).tobytes() == data.tobytes(), "the templates were written"


@pytest.mark.parametrize("key", ["psd loads", "psd tiles"])
def test_relocated_windows(dev, far, key):
    case = jc.case_of(key)
    near = dev.run(case, tag=key)
    data = words_of(case.win)
    decoy = decoy_of(data)
    assert not np.array_equal(decoy, data)
    found = jc.aliases(jc.WIN_BASE, 4)
    assert found
    for a in found:
        far.put(a, decoy)
    far.put(jc.WIN_BASE, data)
    got = dev.run(case, tag=key + " far windows", win_at=(far.ptr, 2 * jc.FAR_SAMPLES, jc.WIN_BASE))
    assert same(got, near), (key, "the run with far windows differs from the near one")
    jc.model_of(key).check(*got, tag=key)
    assert far.get(jc.WIN_BASE, len(data)).tobytes() == data.tobytes(), "the windows were written"
    for a in found:
        assert far.get(a, len(decoy)).tobytes() == decoy.tobytes(), "a decoy was written"


def fill_periodic(far, block):
    """the far buffer as [k][PERIOD] samples, every row the block -> (the rows as int32 [k][2 PERIOD], the block on the device)"""
    torch = far.torch
    assert len(block) == jc.PERIOD and jc.FAR_SAMPLES % jc.PERIOD == 0
    k = jc.FAR_SAMPLES // jc.PERIOD
    d_block = torch.from_numpy(words_of(block).view(np.int32)).cuda()
    rows = far.words.view(k, 2 * jc.PERIOD)
    rows.copy_(d_block.unsqueeze(0).expand(k, -1))
    return rows, d_block


def assert_rows_equal(torch, rows, first, what):
    """every row of int32 [k][..] is `first`, compared on the device a piece at a time"""
    step = max(1, 2 ** 27 // rows.shape[1])
    for a in range(0, rows.shape[0], step):
        assert bool((rows[a:a + step] == first).all().item()), what


def guarded(torch, words):
    """a sentinel-filled int32 buffer of `words` on the device; the caller counts its guards in"""
    return torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("name", ["PSD_LONG", "PSD_LONG_PARTS"])
def test_long_psd_job(dev, far, name):
    """2^21 - 1 segments in 2^16 tiles, and 2^24 - 8 segments in 2^19 tiles with 4 GiB of partials.  Measured once on an MI355X:
    the call takes 0.55 s and 3.55 s (2^24 transforms of 1024 points in double, then one wave that adds 2^19 tiles), below the 5 s
    at which the second parameter would have been left out; the tests 0.84 s and 4.29 s."""
    import torch
    spec = getattr(jc, name)
    if name == "PSD_LONG_PARTS" and far.free < jc.FAR_FREE_NEEDED + 5 * 2 ** 30:
        pytest.skip("4 GiB of scratch beside the far buffer want %d bytes free: %d were" % (jc.FAR_FREE_NEEDED + 5 * 2 ** 30, far.free))
    t_test = time.perf_counter()
    block = pm.noise(jc.PERIOD, 7171)
    rows, d_block = fill_periodic(far, block)
    win = pm.window(pm.HANN, spec["fft_len_log"])
    d_win = torch.from_numpy(win).cuda()
    L, W = len(win), pm.RECORD_DTYPE.itemsize // 4
    job = jc.long_psd_job(spec, out_offset=jc.GUARD)
    d_out = guarded(torch, L + 2 * jc.GUARD)
    d_rec = guarded(torch, (1 + 2 * jc.GUARD) * W)
    t_call = time.perf_counter()
    dev.call("psd", job, em.FP32, far.ptr, jc.FAR_SAMPLES, out=d_out.data_ptr(), cap=L + 2 * jc.GUARD, rec=d_rec.data_ptr() + 4 * W * jc.GUARD,
             win=d_win.data_ptr(), n_win=L, tag=name)
    t_call = time.perf_counter() - t_call
    want_rec, want = jc.periodic_psd(block, win, job[0])
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(-1, W)
    out = d_out.cpu().numpy().view(np.uint32)
    assert np.all(rec[:jc.GUARD] == SENTINEL) and np.all(rec[-jc.GUARD:] == SENTINEL), "written outside the record"
    assert np.all(out[:jc.GUARD] == SENTINEL) and np.all(out[-jc.GUARD:] == SENTINEL), "written outside the trace"
    got_rec = rec[jc.GUARD].copy().view(pm.RECORD_DTYPE)
    assert got_rec["n_seg"][0] == pm.job_n_seg(job[0]) and got_rec["peak_bin"][0] >= 0
    assert got_rec.tobytes() == want_rec.tobytes(), (name, got_rec, want_rec)
    assert out[jc.GUARD:-jc.GUARD].tobytes() == want.tobytes(), "the trace differs from the periodic model's"
    assert torch.equal(rows[0], d_block) and d_win.cpu().numpy().tobytes() == win.tobytes(), "the input was written"
    assert_rows_equal(torch, rows, rows[0], "the input was written")
    print("%s: the call %.2f s, the test %.2f s" % (name, t_call, time.perf_counter() - t_test))


@pytest.mark.parametrize("key", sorted(jc.SYM_LONG))
def test_long_symbols_job(dev, far, key):
    """Measured once on an MI355X: the call takes 0.02 s (sps 3, FIXED, 715827882 symbols) and 0.01 s (sps 64, ESTIMATE, 2^25
    symbols), the tests 0.12 s and 0.06 s."""
    import torch
    spec = jc.SYM_LONG[key]
    sps, W = spec["sps"], sm.RECORD_WORDS
    job = jc.long_symbols_job(spec, out_offset=G)
    max_out = sm.job_max_out(job[0])
    cap = max_out + 2 * G
    if far.free < jc.FAR_FREE_NEEDED + 8 * cap + 2 ** 30:
        pytest.skip("%d bytes of symbols beside the far buffer want %d bytes free: %d were" % (8 * cap, jc.FAR_FREE_NEEDED + 8 * cap + 2 ** 30,
                                                                                          far.free))
    t_test = time.perf_counter()
    block = sm.noise(jc.PERIOD, 7272)
    rows, d_block = fill_periodic(far, block)
    d_out = guarded(torch, 2 * cap)
    d_rec = guarded(torch, (1 + 2 * jc.GUARD) * W)
    t_call = time.perf_counter()
    dev.call("symbols", job, em.FP32, far.ptr, jc.FAR_SAMPLES, out=d_out.data_ptr(), cap=cap, rec=d_rec.data_ptr() + 4 * W * jc.GUARD, tag=key)
    t_call = time.perf_counter() - t_call
    want_rec, head, last = jc.periodic_symbols(block, job[0])
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(-1, W)
    assert np.all(rec[:jc.GUARD] == SENTINEL) and np.all(rec[-jc.GUARD:] == SENTINEL), "written outside the record"
    got_rec = rec[jc.GUARD].copy().view(sm.RECORD_DTYPE)
    assert got_rec.tobytes() == want_rec.tobytes(), (key, got_rec, want_rec)
    n_sym = int(got_rec["n_sym"][0])
    assert got_rec["status"][0] == sm.OK and max_out - 64 // sps - 1 <= n_sym <= max_out
    # the output, on the device: sentinels before, behind n_sym (the reserved rest and the guard); every period equal to the first
    assert bool((d_out[:2 * G] == SENTINEL).all().item()) and bool((d_out[2 * (G + n_sym):] == SENTINEL).all().item()), "written beside the symbols"
    sym = d_out[2 * G:2 * (G + n_sym)]
    per = jc.PERIOD // sps					# symbols of a period of the input
    k = n_sym // per
    assert k >= 2730 and len(head) == per
    whole = sym[:2 * k * per].view(k, 2 * per)
    assert_rows_equal(torch, whole, whole[0], "a period of the output differs from the first")
    rest = sym[2 * k * per:]
    assert torch.equal(rest, whole[0][:rest.numel()]), "the last, partial period differs from the first"
    assert whole[0].cpu().numpy().tobytes() == head.tobytes(), "the first period differs from the periodic model's"
    tail_tile = n_sym % sm.TILE					# the last tile: partial, or (sps 64: n_sym is 2^25) a full one of the cycle
    assert len(last) == tail_tile
    if not tail_tile:
        c = (n_sym // sm.TILE - 1) % (per // sm.TILE)
        tail_tile, last = sm.TILE, head[c * sm.TILE:(c + 1) * sm.TILE]
    assert sym[2 * (n_sym - tail_tile):].cpu().numpy().tobytes() == last.tobytes(), "the last tile differs from the periodic model's"
    assert torch.equal(rows[0], d_block), "the input was written"
    assert_rows_equal(torch, rows, rows[0], "the input was written")
    if spec["mode"] == sm.FIXED:
        # the cut rule: the last 64 symbols as a job of their own, its offset advanced
        tail = jc.advanced_symbols(job[0], n_sym - 64)
        tail["out_offset"] = jc.GUARD
        assert tail["offset"][0] > 2 ** 31
        d_tail = guarded(torch, 2 * (64 + 2 * jc.GUARD))
        d_trec = guarded(torch, W)
        dev.call("symbols", tail, em.FP32, far.ptr, jc.FAR_SAMPLES, out=d_tail.data_ptr(), cap=64 + 2 * jc.GUARD, rec=d_trec.data_ptr(),
                 tag=key + ", the tail")
        short = d_tail.cpu().numpy().view(np.uint32).reshape(-1, 2)
        assert np.all(short[:jc.GUARD] == SENTINEL) and np.all(short[-jc.GUARD:] == SENTINEL)
        assert d_trec.cpu().numpy().view(sm.RECORD_DTYPE)["n_sym"][0] == 64
        assert short[jc.GUARD:-jc.GUARD].tobytes() == sym[-128:].cpu().numpy().tobytes(), "the last 64 symbols do not depend on the cut"
    print("%s: the call %.2f s, the test %.2f s" % (key, t_call, time.perf_counter() - t_test))


@pytest.mark.parametrize("name", sorted(jc.DEC_LONG))
def test_long_decide_job(dev, far, name):
    """2^19 tiles, which one wave of k_dec_job adds; job A's 2^23 keys, job B's last group at the end of the job.  The output is
    2 GiB and the scratch (partial records, decisions, keys) about 2.1 GiB beside the far buffer."""
    import torch
    spec = jc.DEC_LONG[name]
    n, W, T, P = spec["n"], dec.RECORD_WORDS, dec.TILE, jc.PERIOD
    own = dec.owned(n)
    need = jc.FAR_FREE_NEEDED + own + 3 * 2 ** 30
    if far.free < need:
        pytest.skip("%d bytes of output and about %d of scratch beside the far buffer want %d bytes free: %d were"
                    % (own + 2 * G, 2 ** 31 + 2 ** 28, need, far.free))
    t_test = time.perf_counter()
    block = jc.decide_block(spec["order"])
    rows, d_block = fill_periodic(far, block)
    job, word = jc.long_decide_job(spec, block, out_offset=G)
    cap = own + 2 * G
    d_out = guarded(torch, cap // 4)
    d_rec = guarded(torch, (1 + 2 * jc.GUARD) * W)
    t_call = time.perf_counter()
    dev.call("decide", job, em.FP32, far.ptr, jc.FAR_SAMPLES, out=d_out.data_ptr(), cap=cap, rec=d_rec.data_ptr() + 4 * W * jc.GUARD,
             uw=word, tag="decide " + name)
    t_call = time.perf_counter() - t_call
    want_rec, out_bytes = jc.periodic_decide(block, job[0], word)
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(-1, W)
    assert np.all(rec[:jc.GUARD] == SENTINEL) and np.all(rec[-jc.GUARD:] == SENTINEL), "written outside the record"
    got_rec = rec[jc.GUARD].copy().view(dec.RECORD_DTYPE)
    assert got_rec.tobytes() == want_rec.tobytes(), (name, got_rec, want_rec)
    L = jc.DEC_LONG_WORD
    want_pos = n - L - 50 if name == "B" else jc.DEC_LONG_AT
    assert (got_rec["uw_pos"][0], got_rec["uw_rot"][0], got_rec["uw_errors"][0], got_rec["status"][0]) == (want_pos, name == "A", 0, dec.OK)
    assert name == "A" or want_pos > 2 ** 31 - 700
    # the bytes, on the device: sentinels before and behind what the job owns, 0 behind its last symbol
    out = d_out.view(torch.uint8)
    sent = SENTINEL & 0xff
    assert bool((out[:G] == sent).all().item()) and bool((out[G + own:] == sent).all().item()), "written beside the owned bytes"
    assert bool((out[G + n:G + own] == 0).all().item()) and own - n == 1
    sym = out[G:G + n]
    k = n // P
    assert k == 2730 and n % T == T - 1
    whole = sym[:k * P].view(k, P)
    ref = 0 if name == "A" else 1				# under DIFF byte 0 is k[0], no difference: period 0 stands alone
    assert_rows_equal(torch, whole[ref:], whole[ref], "a period of the output differs from period %d" % ref)
    rest = sym[k * P:]
    assert torch.equal(rest, whole[ref][:rest.numel()]), "the last, partial period differs"
    for r in range(ref + 1):
        assert whole[r].cpu().numpy().tobytes() == out_bytes(r * P, P).tobytes(), "period %d differs from the periodic model's" % r
    assert sym[n - (T - 1):].cpu().numpy().tobytes() == out_bytes(n - (T - 1), T - 1).tobytes(), "the last tile differs from the model's"
    assert torch.equal(rows[0], d_block), "the input was written"
    assert_rows_equal(torch, rows, rows[0], "the input was written")
    print("decide %s: the call %.2f s, the test %.2f s" % (name, t_call, time.perf_counter() - t_test))


@pytest.mark.parametrize("name", sorted(jc.CAR_LONG))
def test_long_carrier_job(dev, far, name):
    """2^19 sum tiles and (job E) 2^19 lag tiles, which one wave of k_car_phase and of k_car_freq adds; (double)j up to 2^31 - 2 in
    k_car_sum and k_car_turn.  The output is 16 GiB beside the far buffer.  Job E's z_re, z_im, phase and output have no model at
    this length and are not compared."""
    import torch
    spec = jc.CAR_LONG[name]
    n, W, T, P = spec["n"], car.RECORD_WORDS, car.TILE, jc.PERIOD
    cap = n + 2 * G
    need = jc.FAR_FREE_NEEDED + 8 * cap + 6 * 2 ** 30
    if far.free < need:
        pytest.skip("%d bytes of output beside the far buffer's %d want %d bytes free: %d were" % (8 * cap, jc.FAR_BYTES, need, far.free))
    t_test = time.perf_counter()
    block = jc.carrier_block(spec["order"])
    rows, d_block = fill_periodic(far, block)
    job = jc.long_carrier_job(spec, out_offset=G)
    d_out = guarded(torch, 2 * cap)
    d_rec = guarded(torch, (1 + 2 * jc.GUARD) * W)
    t_call = time.perf_counter()
    dev.call("carrier", job, em.FP32, far.ptr, jc.FAR_SAMPLES, out=d_out.data_ptr(), cap=cap, rec=d_rec.data_ptr() + 4 * W * jc.GUARD,
             tag="carrier " + name)
    t_call = time.perf_counter() - t_call
    want_rec = jc.periodic_carrier(block, job[0])
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(-1, W)
    assert np.all(rec[:jc.GUARD] == SENTINEL) and np.all(rec[-jc.GUARD:] == SENTINEL), "written outside the record"
    got_rec = rec[jc.GUARD].copy().view(car.RECORD_DTYPE)
    assert got_rec["status"][0] == car.OK
    for k in (jc.CAR_E_FIELDS if name == "E" else car.RECORD_DTYPE.names):
        assert got_rec[k].tobytes() == want_rec[k].tobytes(), (name, k, got_rec, want_rec)
    assert bool((d_out[:2 * G] == SENTINEL).all().item()) and bool((d_out[2 * (G + n):] == SENTINEL).all().item()), "written beside the symbols"
    sym = d_out[2 * G:2 * (G + n)]
    piece = 2 ** 28
    for at in range(0, 2 * n, piece):
        assert not bool((sym[at:at + piece] == SENTINEL).any().item()), "an output word was not written"
    tiles = lambda j0, count: sym[2 * j0:2 * (j0 + count)].cpu().numpy().tobytes()
    model = lambda j0, count: jc.carrier_symbols(block, job[0], want_rec, j0, count).tobytes()
    assert n % T == T - 1
    if name == "C":
        assert jc.exact_products(job[0])
        k = n // P
        whole = sym[:2 * k * P].view(k, 2 * P)
        assert_rows_equal(torch, whole, whole[0], "a period of the output differs from the first")
        rest = sym[2 * k * P:]
        assert torch.equal(rest, whole[0][:rest.numel()]), "the last, partial period differs from the first"
        assert tiles(0, P) == model(0, P), "the first period differs from the model's"
        assert tiles(n - (T - 1), T - 1) == model(n - (T - 1), T - 1), "the last tile differs from the model's"
    if name == "D":
        for j0, count in ((0, 2 * T), (2 ** 30 - T, 2 * T), (n - (T - 1), T - 1)):
            assert tiles(j0, count) == model(j0, count), ("the symbols from %d on differ from rule 6 with the true j" % j0)
    assert torch.equal(rows[0], d_block), "the input was written"
    assert_rows_equal(torch, rows, rows[0], "the input was written")
    print("carrier %s: the call %.2f s, the test %.2f s" % (name, t_call, time.perf_counter() - t_test))


def worst(got, want):
    y = got.view(np.float32).reshape(-1, 2).astype(np.float64)
    return max(np.abs(y[:, 0] - want.real).max(), np.abs(y[:, 1] - want.imag).max())


def test_long_wave_job(dev, far):
    import torch
    spec = jc.WAVE_LONG
    n_out, D, T, first = spec["n_out"], spec["decim"], spec["n_taps"], spec["first"]
    taps = em.lowpass(np.random.default_rng(77), T)
    d_taps = torch.from_numpy(taps).cuda()
    # exactly the samples the job reads: rows of T words, D words apart
    rows = far.words.as_strided((n_out, T), (D, 1), first)
    index = first + torch.arange(n_out, dtype=torch.int64, device="cuda")[:, None] * D + torch.arange(T, dtype=torch.int64, device="cuda")
    v = jc.hash_words(index)
    vals = torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)
    rows.copy_(vals)
    del index, v

    job = jc.long_extract_job(spec, jc.GUARD)
    cap = n_out + 2 * jc.GUARD
    d_out = torch.full((2 * cap,), SENTINEL, dtype=torch.int32, device="cuda")
    dev.call("extract", job, em.SC16, far.ptr, 2 * jc.FAR_SAMPLES, out=d_out.data_ptr(), cap=cap, taps=d_taps.data_ptr(), n_taps=T,
             tag="long wave")
    out = d_out.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert np.all(out[:jc.GUARD] == SENTINEL) and np.all(out[-jc.GUARD:] == SENTINEL), "written outside the job's range"
    assert torch.equal(rows, vals), "the input was written"
    assert d_taps.cpu().numpy().tobytes() == taps.tobytes()
    got = out[jc.GUARD:-jc.GUARD]
    x, tol, err = jc.HashedStream(), jc.hashed_bound(job[0], taps), 0.0
    step = 2 ** 19
    for m0 in range(0, n_out, step):				# the model over all outputs, a piece at a time
        sub = jc.advanced(job[0], m0)
        sub["n_out"] = min(step, n_out - m0)
        err = max(err, worst(got[m0:m0 + step], em.extract_job(x, sub[0], taps)))
    print("long wave: err %.3g of %.3g" % (err, tol))
    assert err <= tol

    # the cut rule: the last 64 outputs as a job of their own, first and phase0 advanced
    tail = jc.advanced(job[0], n_out - 64)
    tail["out_offset"] = jc.GUARD
    assert 2 ** 31 < tail["first"][0] < 2 ** 32 < tail["first"][0] + 63 * D
    d_tail = torch.full((2 * (64 + 2 * jc.GUARD),), SENTINEL, dtype=torch.int32, device="cuda")
    dev.call("extract", tail, em.SC16, far.ptr, 2 * jc.FAR_SAMPLES, out=d_tail.data_ptr(), cap=64 + 2 * jc.GUARD, taps=d_taps.data_ptr(),
             n_taps=T, tag="long wave, the tail")
    short = d_tail.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert np.all(short[:jc.GUARD] == SENTINEL) and np.all(short[-jc.GUARD:] == SENTINEL)
    assert short[jc.GUARD:-jc.GUARD].tobytes() == got[-64:].tobytes(), "the last 64 outputs do not depend on the cut"


def test_long_tile_job(dev, far):
    import torch
    spec = jc.TILE_LONG
    n_out, D, T, first = spec["n_out"], spec["decim"], spec["n_taps"], spec["first"]
    taps = em.lowpass(np.random.default_rng(78), T)
    d_taps = torch.from_numpy(taps).cuda()
    end = first + em.need(n_out, D, T)				# the words the job reads end here
    out_offset = jc.FAR_SAMPLES - n_out - G - 1
    assert end <= 2 * (out_offset - G), "input and output lie in disjoint regions"
    piece = 2 ** 26
    for at in range(0, end, piece):
        far.words[at:min(at + piece, end)].copy_(far.hashed(at, min(piece, end - at)))
    far.fill(2 * (out_offset - G), 2 * (n_out + 2 * G))

    job = jc.long_extract_job(spec, out_offset)
    dev.call("extract", job, em.SC16, far.ptr, 2 * jc.FAR_SAMPLES, out=far.ptr, cap=jc.FAR_SAMPLES, taps=d_taps.data_ptr(), n_taps=T,
             tag="long tile")
    assert far.count(2 * (out_offset - G), 2 * G) == 2 * G and far.count(2 * (out_offset + n_out), 2 * G) == 2 * G, "written beside the range"
    assert far.count(2 * out_offset, 2 * n_out) == 0, "an output word was not written"
    for at in range(0, end, piece):
        assert torch.equal(far.words[at:min(at + piece, end)], far.hashed(at, min(piece, end - at))), "the input was written"

    x, tol = jc.HashedStream(), jc.hashed_bound(job[0], taps)
    tiles = -(-n_out // em.TILE_OUT)
    k = 2 ** 31 // (D * em.TILE_OUT)				# the last tile whose base m0 * D is below 2^31
    assert k + 1 == tiles - 2
    for t in (0, k - 1, k + 1):					# two tiles each: the first, below 2^31, and from 2^31 on: the last, one short
        m0 = t * em.TILE_OUT
        sub = jc.advanced(job[0], m0)
        sub["n_out"] = min(2 * em.TILE_OUT, n_out - m0)
        got = far.get(2 * (out_offset + m0), 2 * int(sub["n_out"][0]))
        err = worst(got, em.extract_job(x, sub[0], taps))
        print("long tile: tiles %d and %d: err %.3g of %.3g" % (t, t + 1, err, tol))
        assert err <= tol, (t, err, tol)

    # the cut rule: the last 300 outputs as a job of their own, first and phase0 advanced
    tail = jc.advanced(job[0], n_out - 300)
    tail["out_offset"] = jc.GUARD
    assert tail["first"][0] > 2 ** 31
    d_tail = torch.full((2 * (300 + 2 * jc.GUARD),), SENTINEL, dtype=torch.int32, device="cuda")
    dev.call("extract", tail, em.SC16, far.ptr, 2 * jc.FAR_SAMPLES, out=d_tail.data_ptr(), cap=300 + 2 * jc.GUARD, taps=d_taps.data_ptr(),
             n_taps=T, tag="long tile, the tail")
    short = d_tail.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert np.all(short[:jc.GUARD] == SENTINEL) and np.all(short[-jc.GUARD:] == SENTINEL)
    assert short[jc.GUARD:-jc.GUARD].reshape(-1).tobytes() == far.get(2 * (out_offset + n_out - 300), 600).tobytes()
