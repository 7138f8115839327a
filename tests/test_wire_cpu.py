"""The compact wire formats of the sharded frame's hit counts (include/fosphor_amd_wire.h) without a GPU: the numpy statement of
the formats in gr_fosphor_amd.dist -- what tests/test_gpu_wire.py holds the kernels to --, the C ABI's symbols and their binding,
and the conditions the GPU test's inputs must keep, computed from the oracle alone."""
import os
import re

import numpy as np
import pytest

import shard_emul as se
import wire_cases as wc
from _pkg import gr_fosphor_amd
from gr_fosphor_amd import _lib
from gr_fosphor_amd.dist import (wire_mask_numpy, wire_pack_numpy, wire_unpack_numpy, wire_union_rows, resolve_wire,
                                 combine_partials_numpy)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sum(ranks):
    return np.sum([r.astype(np.uint64) for r in ranks], axis=0).astype(np.uint32)


def test_dense_round_trip_and_sum_of_words_is_packing_of_sums():
    rng = np.random.default_rng(1)
    ranks = [rng.integers(0, 65536 // 8, 4096).astype(np.uint32) for _ in range(8)]
    for hc in ranks:
        hc[[10, 11, 4094, 4095]] = 65520 // 8		# adjacent cells that both reach 65520 in the sum
        hc[20], hc[21] = 65520 // 8, 0
        hc[31], hc[30] = 65520 // 8, 0
    total = _sum(ranks)
    assert total[10] == total[11] == total[4094] == total[4095] == 65520 and total.max() <= 65535
    words = [wire_pack_numpy(hc) for hc in ranks]
    assert all(w.dtype == np.uint32 and w.shape == (2048,) for w in words)
    assert words[0][5] == (ranks[0][10] | ranks[0][11] << 16)
    for hc, w in zip(ranks, words):
        assert np.array_equal(wire_unpack_numpy(w, 4096), hc)
    summed = np.sum([w.astype(np.uint64) for w in words], axis=0)
    assert summed.max() < 1 << 32
    assert np.array_equal(summed.astype(np.uint32), wire_pack_numpy(total))
    assert np.array_equal(wire_unpack_numpy(summed.astype(np.uint32), 4096), total)
    assert np.array_equal(total, combine_partials_numpy([(r, np.zeros(1, np.float32), np.zeros(1, np.float32)) for r in ranks])[0])


def test_synthetic_dense_counts_keep_their_conditions():
    ranks = wc.dense_counts()
    total = _sum(ranks)
    assert len(ranks) == wc.SYN_WORLD and all(r.shape == (wc.SYN_CELLS,) and r.dtype == np.uint32 for r in ranks)
    assert total.max() == 65532 and total.max() <= wc.SYN_TOTAL
    assert {0, 1, 65535 // wc.SYN_WORLD, wc.PER_RANK_BIG} <= set(np.unique(ranks[0]).tolist())
    for c in (0, 62, 64, 1000, wc.SYN_CELLS - 2):
        assert total[c] == total[c + 1] == 65520		# both halves of word c / 2
    assert (total[2000], total[2001], total[3000], total[3001]) == (65520, 0, 0, 65520)
    words = np.sum([wire_pack_numpy(r).astype(np.uint64) for r in ranks], axis=0).astype(np.uint32)
    assert words[0] == 0xFFF0FFF0 and np.array_equal(wire_unpack_numpy(words, wc.SYN_CELLS), total)


@pytest.mark.parametrize("pattern,n_live,fall_back", [("few", None, False), ("half", wc.SYN_ROWS // 2, False),
                                                       ("over", wc.SYN_ROWS // 2 + 1, True)])
def test_union_rows_and_sparse_round_trip(pattern, n_live, fall_back):
    by_rank = wc.sparse_rows(pattern)
    ranks = wc.sparse_counts(pattern)
    masks = np.stack([wire_mask_numpy(hc) for hc in ranks])
    assert masks.shape == (wc.SYN_WORLD, wc.SYN_ROWS // 32) and masks.dtype == np.uint32
    for rows, m in zip(by_rank, masks):		# a rank's bits are its rows: bit r & 31 of word r >> 5
        assert sorted(32 * w + b for w in range(m.size) for b in range(32) if m[w] >> b & 1) == rows
    rows, fb = wire_union_rows(masks)
    assert rows.tolist() == sorted(set().union(*by_rank)) and fb == fall_back
    if n_live is not None:
        assert rows.size == n_live
    if pattern == "few":
        assert rows[0] == 0 and rows[-1] == wc.SYN_ROWS - 1 and rows.size < wc.SYN_ROWS // 4
        only = [r for r in rows if sum(r in set(b) for b in by_rank) == 1]
        assert 33 in only and wc.SYN_ROWS - 1 in only and 2047 in only and 2048 in only
        assert all(0 in b and 63 in b and 64 in b for b in by_rank)		# rows live on every rank
    total = _sum(ranks)
    assert total.max() == 65520 and total.reshape(-1, 64)[0, 10] == total.reshape(-1, 64)[0, 11] == 65520
    words = [wire_pack_numpy(hc, rows) for hc in ranks]
    assert all(w.shape == (rows.size * 32,) for w in words)
    r1 = by_rank[1]
    dead_on_1 = next(i for i, r in enumerate(rows) if r not in r1)	# live elsewhere, empty here: packed as zeros
    assert not words[1][32 * dead_on_1:32 * dead_on_1 + 32].any()
    summed = np.sum([w.astype(np.uint64) for w in words], axis=0).astype(np.uint32)
    assert np.array_equal(summed, wire_pack_numpy(total, rows))
    assert np.array_equal(wire_unpack_numpy(summed, wc.SYN_CELLS, rows), total)		# every cell, dead rows included


def test_auto_resolution():
    assert resolve_wire("auto", 65536, 1 << 30) == "u32"
    assert resolve_wire("auto", 65535, 16 << 20) == "sparse16"
    assert resolve_wire("auto", 65535, (16 << 20) - 4) == "packed16"
    assert resolve_wire("u32", 16, 0) == "u32" and resolve_wire("sparse16", 16, 0) == "sparse16"
    with pytest.raises(ValueError):
        resolve_wire("u16", 16, 0)


def test_every_declared_function_is_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "fosphor_amd_wire.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\bint\s+(fosphor_amd_\w+)\s*\(", src))
    assert {"fosphor_amd_wire_mask", "fosphor_amd_wire_pack", "fosphor_amd_wire_unpack", "fosphor_amd_exchange_compact",
            "fosphor_amd_wire_stats"} <= declared
    L = _lib.load()
    for name in sorted(declared):
        assert name in _lib.SIGNATURES, name + " is not bound in _lib.py"
        assert getattr(L, name, None) is not None, name + " is not exported by the library"
    f = gr_fosphor_amd.Fosphor
    for m in ("wire_mask", "wire_pack", "wire_unpack", "wire_info", "wire_stats", "exchange_compact", "wire_kernel_times"):
        assert callable(getattr(f, m))
    assert gr_fosphor_amd.core.WIRE_FORMS == {"packed16": 1, "sparse16": 2}
    assert re.search(r"#define\s+FOSPHOR_AMD_WIRE_PACKED16\s+1\b", src) and re.search(r"#define\s+FOSPHOR_AMD_WIRE_SPARSE16\s+2\b", src)


@pytest.mark.parametrize("cid", sorted(wc.WHOLE))
def test_whole_frame_inputs_through_the_oracle(oracle_built, cid):
    """What the GPU test relies on, from the oracle's counts alone: every sample counted once; at N = 8192 both halves of the bin
    range hold hits; and the N = 65536 frames leave a union live-row fraction strictly between 1 % and 50 % (found: 0.334 and
    0.335 of 524288 rows), with rows that are live in the first frame and dead in the second."""
    c = wc.WHOLE[cid]
    n = 1 << c["log2n"]
    at = 0
    for off, cnt in c["shards"]:
        assert off == at and cnt % 16 == 0 and cnt >= 16
        at += cnt
    assert at == c["total"] <= 65535 and (c["n_bins"] * n) % 2048 == 0
    o = se.make_oracle(c)
    prev = None
    for frame in range(c["frames"]):
        x, x32 = se.make_stream(c, frame)
        se.oracle_frame(o, c, x32)
        hc = wc.oracle_counts(o)
        assert int(hc.sum(dtype=np.uint64)) == c["total"] * n and hc.max() <= c["total"]
        frac = wc.live_rows(hc) / (hc.size // 64)
        print("case %s frame %d: %.4f of %d rows live" % (cid, frame, frac, hc.size // 64))
        if cid == "p13":
            lo, hi = se.plane_fractions(o)
            assert lo >= 0.01 and hi >= 0.01
        if c["form"] == "sparse16":
            assert 0.01 < frac < 0.5, "case %s frame %d: %.4f of the rows live" % (cid, frame, frac)
            rows, fb = wire_union_rows(wire_mask_numpy(hc))
            assert not fb and rows.size == wc.live_rows(hc)
            live = hc.reshape(-1, 64).any(axis=1)
            if prev is not None:
                assert (prev & ~live).sum() > 1000, "no row dies between the frames"
            prev = live
