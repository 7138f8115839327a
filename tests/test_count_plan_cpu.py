"""fosphor_amd_plan_count without a GPU: the one host function every launch site takes its count hand-off from (which buffer the
count kernel fills and the merge kernel reads, the chunking, the merge form), against the expectations the GPU suites carry by hand
-- `forms` / `mem` / `smax` of tests/persistence_cases.py, `launches` of tests/shard_emul.py -- and against the rules the comments in
fosphor_api.cpp and include/fosphor_amd.h state.  None of the expectations comes from the function under test."""
import ctypes as C
import errno

import pytest

import persistence_cases as pc
import shard_emul as se
from test_boundary_cpu import amd		# noqa: F401  (the fixture: builds the library when it is missing)
from test_gpu_persistence import DENSE_TWIN, FORMS

DIRECT16, SUM16, COUNT32 = 0, 1, 2		# FOSPHOR_AMD_COUNT_*
LONG_FORMS = ("dense16_long4", "dense16_long", "sparse16_long")


def _plan(amd, log2n, n_bins, slab_chunks, rowmask_off, no_sum16, n_batches, batch, pipelined):
    from gr_fosphor_amd._lib import CountPlan
    p = CountPlan()
    rv = amd.load().fosphor_amd_plan_count(log2n, n_bins, slab_chunks, rowmask_off, no_sum16, n_batches, batch, pipelined, C.byref(p))
    assert rv == 0, (rv, log2n, n_bins, slab_chunks, n_batches, batch, pipelined)
    return p


def _slab_chunks(max_spectra):
    """fosphor_amd_init: one count slab per 1024-spectrum chunk of the largest launch, on instances of more than 1024 spectra"""
    return max_spectra // 1024 if max_spectra > 1024 else 0


def _sub_samples(env, log2n):
    return 1 << int(env.get("FOSPHOR_AMD_SUB_LOG2", 30 if log2n == 13 else 26))


def _merge_launches(amd, s, rowmask_off):
    """(call, batches in the launch, plan) of every merge launch of a scenario: a process call is one launch, a device call one per
    piece of fosphor_amd_plan_piece_batches, an accumulate + merge (sliced or not) one launch over the partial arrays"""
    env = s["env"]
    geom = (s["log2n"], s["n_bins"], _slab_chunks(pc.capacity(s)[0]), int(rowmask_off or env.get("FOSPHOR_AMD_ROWMASK") == "0"),
            int("FOSPHOR_AMD_NO_SUM16" in env))
    streams = int(env.get("FOSPHOR_AMD_OVERLAP") != "0")
    out = []
    for c in s["calls"]:
        if c["ep"] in ("accumulate", "merge_sliced"):
            out.append((c, 1, _plan(amd, *geom, 1, c["batch"], 0)))
            continue
        sub_b = amd.load().fosphor_amd_plan_piece_batches(s["log2n"], streams, c["nb"], c["batch"], _sub_samples(env, s["log2n"]))
        assert 1 <= sub_b <= c["nb"]
        for b0 in range(0, c["nb"], sub_b):
            nb = min(sub_b, c["nb"] - b0)
            out.append((c, nb, _plan(amd, *geom, nb, c["batch"], 1)))
    return out


@pytest.mark.parametrize("sid", sorted(pc.SCENARIOS))
def test_plan_names_the_merge_forms_the_persistence_scenarios_declare(amd, sid):
    s = pc.SCENARIOS[sid]
    launches = _merge_launches(amd, s, rowmask_off=False)
    seen = set()
    for c, nb, p in launches:
        form = FORMS[p.merge_form]
        assert form in s["forms"], "%s: a launch of %d x %d (%s) takes form %s, the table declares %s" % (
            sid, nb, c["batch"], c["ep"], form, sorted(s["forms"]))
        seen.add(form)
        # include/fosphor_amd.h, FOSPHOR_AMD_MERGE_TABLE_IN_MEMORY: every SPARSE16_LONG launch; the dense long ones above 4096 spectra
        in_memory = form == "sparse16_long" or (form in LONG_FORMS and c["batch"] > 4096)
        assert bool(p.table_in_memory) == in_memory, (sid, nb, c["batch"], form)
    assert seen == set(s["forms"]), "%s: the table declares %s, the plans reach %s" % (sid, sorted(s["forms"]), sorted(seen))
    if "mem" in s:
        long_launches = [p for _, _, p in launches if FORMS[p.merge_form] in LONG_FORMS]
        assert long_launches
        assert sum(p.table_in_memory for p in long_launches) == (len(long_launches) if s["mem"] == "all" else 0)
    if "smax" in s:
        want = "sparse16_long" if "sparse16_long" in s["forms"] else "sparse16"
        got = max(nb for _, nb, p in launches if FORMS[p.merge_form] == want)
        assert s["smax"][0] <= got == s["smax"][1]
    if s["forms"] & set(DENSE_TWIN):
        # the second pass of the GPU test, FOSPHOR_AMD_ROWMASK=0: the dense twin of every sparse form and nothing else
        twin = {FORMS[p.merge_form] for _, _, p in _merge_launches(amd, s, rowmask_off=True)}
        assert twin == {DENSE_TWIN.get(k, k) for k in s["forms"]}
        assert not any(p.rowmask for _, _, p in _merge_launches(amd, s, rowmask_off=True))


@pytest.mark.parametrize("cid", sorted(se.CASES))
def test_plan_reproduces_the_launch_counts_of_the_shard_cases(amd, cid):
    """Per rank of a case: (FFT pieces, k2c chunk sums, k2b chunk reduces) of one frame from the plan of the shard's count launch.
    The rule accumulate() applies around the plan, from its comment: a shard of several whole 1024-spectrum chunks (the plan's slab
    sum) that is longer than a sub-launch of sub_c chunks runs like a device-resident call -- ceil(chunks / sub_c) pieces, each with
    a count kernel of its own, and ONE chunk sum at the end; every other shard is one FFT launch and one count launch, followed by
    the chunk sum or the chunk reduce of the plan when the batch has more than one chunk."""
    c = se.CASES[cid]
    n = 1 << c["log2n"]
    sub_c = max(_sub_samples(c["env"], c["log2n"]) // (1024 * n), 1)
    for (off, cnt), declared in zip(c["shards"], c["launches"]):
        p = _plan(amd, c["log2n"], c["n_bins"], _slab_chunks(cnt), 0, int("FOSPHOR_AMD_NO_SUM16" in c["env"]), 1, cnt, 0)
        assert p.handoff in (SUM16, COUNT32) and p.cpb * p.chunk == cnt
        if p.handoff == SUM16 and p.cpb > sub_c:
            want = (-(-p.cpb // sub_c), 1, 0)
        else:
            want = (1, int(p.handoff == SUM16), int(p.handoff == COUNT32 and p.cpb > 1))
        assert want == declared, "case %s shard (%d, %d): the plan gives %s, the table declares %s" % (cid, off, cnt, want, declared)
        # the frame's merge reads the exchanged 32-bit partial arrays: with the table up to 8192 spectra, evaluated beyond
        m = _plan(amd, c["log2n"], c["n_bins"], _slab_chunks(cnt), 0, 0, 1, c["total"], 0)
        assert FORMS[m.merge_form] == ("table32" if c["total"] <= 8192 else "eval32") and not m.rowmask and not m.two_sets


BATCHES = (16, 48, 1008, 1024, 1040, 2048, 2080, 3024, 4096, 4112, 8176, 8192, 8208, 16384, 65520, 65536)


@pytest.mark.parametrize("log2n", [10, 13, 16])
def test_plan_follows_the_rules_the_comments_state(amd, log2n):
    n = 1 << log2n
    for batch in BATCHES:
        for nb in (1, 2, 3, 7, 8, 64):
            for slab_chunks in (0, 4, 64, 4096):
                for rowmask_off in (0, 1):
                    for no_sum16 in (0, 1):
                        for pipelined in (0, 1):
                            p = _plan(amd, log2n, 128, slab_chunks, rowmask_off, no_sum16, nb, batch, pipelined)
                            what = (log2n, batch, nb, slab_chunks, rowmask_off, no_sum16, pipelined)
                            # the 16-bit hand-off: batches up to 1024 spectra; up to 8192 counted as ONE chunk where the launch
                            # has at least 128 slabs of 64 columns; never beyond the (d, e) table; never for the partial arrays
                            if not pipelined or batch > 8192:
                                direct = False
                            elif batch <= 1024:
                                direct = True
                            else:
                                direct = (n // 64) * nb >= 128
                            assert (p.handoff == DIRECT16) == direct, what
                            assert bool(p.table) == (batch <= 8192), what
                            assert bool(p.two_sets) == (direct and batch <= 1024), what
                            assert bool(p.rowmask) == (direct and log2n == 16 and not rowmask_off), what
                            # chunks: whole, equal, at most 1024 spectra unless the batch is counted as one chunk
                            assert p.chunk >= 1 and batch % p.chunk == 0 and p.cpb == batch // p.chunk, what
                            assert p.chunk <= 1024 or (p.cpb == 1 and direct), what
                            assert p.chunk % 16 == 0, what		# (batches are multiples of 16 spectra)
                            if direct or batch <= 1024:
                                assert p.cpb == 1, what
                            # slab sums: whole 1024-spectrum chunks, several of them, room for all the launch's slabs, knob not set
                            sum16 = (not direct and batch % 1024 == 0 and batch > 1024 and nb * (batch // 1024) <= slab_chunks
                                     and not no_sum16)
                            assert (p.handoff == SUM16) == sum16, what
                            if sum16:
                                assert p.chunk == 1024, what
                            # the merge form (include/fosphor_amd.h, fosphor_amd_merge_stats)
                            if not direct:
                                form = "table32" if batch <= 8192 else "eval32"
                            elif p.rowmask:
                                form = "sparse16" if batch <= 1024 else "sparse16_long"
                            elif batch <= 1024:
                                form = "dense16"
                            else:
                                form = "dense16_long4" if nb <= 4 else "dense16_long"
                            assert FORMS[p.merge_form] == form, what
                            assert bool(p.table_in_memory) == (form == "sparse16_long" or (form in LONG_FORMS and batch > 4096)), what


def test_plan_rejects_nonsense(amd):
    from gr_fosphor_amd._lib import CountPlan
    f = amd.load().fosphor_amd_plan_count
    p = CountPlan()
    assert f(10, 128, 0, 0, 0, 1, 16, 1, C.byref(p)) == 0
    for bad in [(0, 128, 0, 0, 0, 4, 64, 1), (31, 128, 0, 0, 0, 4, 64, 1), (10, 128, 0, 0, 0, 0, 64, 1), (10, 128, 0, 0, 0, 4, 0, 1),
                (10, 0, 0, 0, 0, 4, 64, 1), (10, 128, -1, 0, 0, 4, 64, 1)]:
        assert f(*bad, C.byref(p)) == -errno.EINVAL, bad
    assert f(10, 128, 0, 0, 0, 1, 16, 1, None) == -errno.EINVAL
