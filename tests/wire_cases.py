"""Inputs of the compact-wire tests (include/fosphor_amd_wire.h): data shared by tests/test_wire_cpu.py, which checks the inputs
and the numpy statement of the formats without a GPU, and tests/test_gpu_wire.py, which runs the kernels against them.

Synthetic counts are written straight into the partial slots of small instances; whole frames go through the emulated ranks of
tests/shard_emul.py, whose case dictionaries these are."""
import numpy as np

import shard_emul as se

# ---- synthetic counts: N = 1024, 256 bins, 4 ranks -------------------------------------------------------------------------
SYN_LOG2N, SYN_BINS, SYN_WORLD = 10, 256, 4
SYN_CELLS = SYN_BINS << SYN_LOG2N		# 262144 cells
SYN_ROWS = SYN_CELLS // 64			# 4096 rows, 128 mask words per rank
SYN_TOTAL = 65535				# the frame the counts could come from: every cell and every sum stays at or below it
PER_RANK_BIG = 65520 // SYN_WORLD		# 16380: four of them reach 65520 = 0xFFF0 in one half of a word


def dense_counts():
    """Per rank uint32[SYN_CELLS]: cells of 0, 1, 65535 // world and 65520 // world all over; words whose two halves BOTH reach 65520
    in the sum (cells 2 w and 2 w + 1 at 16380 on every rank) at the start, the end and across a row border; a word with 65520 in
    the low half only and one with it in the high half only, where a carry or a wrong shift would show."""
    rng = np.random.default_rng(4242)
    choices = np.array([0, 0, 0, 1, 1, 65535 // SYN_WORLD, PER_RANK_BIG], dtype=np.uint32)
    ranks = [choices[rng.integers(0, choices.size, SYN_CELLS)] for _ in range(SYN_WORLD)]
    both = [0, 1, 62, 63, 64, 65, 1000, 1001, SYN_CELLS - 2, SYN_CELLS - 1]
    low_only, high_only = (2000, 2001), (3000, 3001)
    for hc in ranks:
        hc[both] = PER_RANK_BIG
        hc[low_only[0]], hc[low_only[1]] = PER_RANK_BIG, 0
        hc[high_only[0]], hc[high_only[1]] = 0, PER_RANK_BIG
    return ranks


def _rows_to_counts(rows_by_rank, seed):
    """counts with exactly the given rows live on each rank: a live row holds 1 .. 64 cells of 1 .. 16380, among them -- in rows
    live on every rank -- a pair of neighbours at 16380, so that the sums reach 65520 in both halves of a word"""
    rng = np.random.default_rng(seed)
    common = set.intersection(*[set(r) for r in rows_by_rank])
    out = []
    for rows in rows_by_rank:
        hc = np.zeros((SYN_ROWS, 64), dtype=np.uint32)
        for r in rows:
            k = int(rng.integers(1, 65))
            cols = rng.choice(64, size=k, replace=False)
            hc[r, cols] = rng.integers(1, PER_RANK_BIG + 1, size=k)
            if r in common:
                hc[r, 10:12] = PER_RANK_BIG
        out.append(hc.reshape(-1))
    return out


def sparse_rows(pattern):
    """The rows live on each of the SYN_WORLD ranks.
    "few":   the first row on every rank, the last row on rank 3 only, row 33 on rank 1 only, rows 2047 / 2048 (either side of the
             middle, in different mask words) on ranks 0 / 2, rows 63, 64 (either side of a 64-row group) on every rank, and
             300 random rows on random subsets of ranks 0, 1, 3 (rank 2 has four rows in all)
    "half":  exactly half of the rows live in the union (every even row on one rank in turn, multiples of 64 on rank 0 too, row 0 on
             every rank): stays sparse
    "over":  the same plus row 1: one row more than half, falls back"""
    if pattern == "few":
        rng = np.random.default_rng(77)
        rows = [{0, 63, 64} for _ in range(SYN_WORLD)]
        rows[3].add(SYN_ROWS - 1)
        rows[1].add(33)
        rows[0].add(2047)
        rows[2].add(2048)
        for r in rng.choice(np.arange(100, 4000), size=300, replace=False):
            for q in rng.choice([0, 1, 3], size=int(rng.integers(1, 4)), replace=False):
                rows[int(q)].add(int(r))
        return [sorted(s) for s in rows]
    if pattern in ("half", "over"):
        rows = [set() for _ in range(SYN_WORLD)]
        for r in range(0, SYN_ROWS, 2):
            rows[(r // 2) % SYN_WORLD].add(r)
            if r % 64 == 0:
                rows[0].add(r)
        for q in range(SYN_WORLD):
            rows[q].add(0)
        if pattern == "over":
            rows[2].add(1)
        return [sorted(s) for s in rows]
    raise KeyError(pattern)


def sparse_counts(pattern):
    return _rows_to_counts(sparse_rows(pattern), {"few": 1, "half": 2, "over": 3}[pattern])


# ---- whole frames against one oracle launch (dictionaries in the shape of shard_emul.CASES) -----------------------------------------
# The sparse case needs a frame whose union of live rows is a real subset: strictly between 1 % and 50 % of the rows, else the
# sparse form is either trivial or falls back.  The power range was chosen on the CPU from the oracle's counts
# (tests/test_wire_cpu.py asserts the bounds on both frames); fraction of the 524288 rows that hold a hit, N = 65536, fp16,
# sigma 0.05 + tone 0.05, 64 spectra, frame 0 / frame 1:
#   (-46 dB, 5 dB/div), shard_emul's range for this length:  0.593 / 0.593  -> would fall back
#   (-20 dB, 10 dB/div):                                     0.340 / 0.340
#   (0 dB, 10 dB/div), the range used here:                  0.334 / 0.335
# The native test's frames (N = 1024, 256 bins, (0 dB, 10 dB/div), sigma 0.05 + tone 0.1): 16 / 32 / 64 / 128 spectra leave
# 0.310 / 0.345 / 0.375 / 0.406 of the 4096 rows live, so frames of up to 128 spectra go out sparse.
WHOLE = {
    "p10": dict(log2n=10, fmt="fp32", n_bins=256, wf_rows=1024, total=64, overlap=1, frames=1, shards=[(0, 16), (16, 48)],
                power=(0, 10), seed=9101, form="packed16"),
    # shard_emul case "d"'s range: both halves of the bin range hold hits
    "p13": dict(log2n=13, fmt="fp32", n_bins=512, wf_rows=1024, total=32, overlap=1, frames=1, shards=[(0, 16), (16, 16)],
                power=se.CASES["d"]["power"], seed=9102, form="packed16"),
    "s16": dict(log2n=16, fmt="fp16", n_bins=512, wf_rows=64, total=64, overlap=2, frames=2, shards=[(0, 16), (16, 48)],
                power=(0, 10), seed=9103, form="sparse16"),
}


def oracle_counts(o):
    """the oracle's counts of its last launch in the library's layout: uint32 [bin][x], flattened"""
    return np.ascontiguousarray(o.hitcount.T).astype(np.uint32).reshape(-1)


def live_rows(hc):
    """rows of flattened [bin][x] counts that hold a hit"""
    return int(np.asarray(hc).reshape(-1, 64).any(axis=1).sum())
