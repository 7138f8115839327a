"""The shard-shape table of tests/shard_emul.py, checked without a GPU: a broken table or input builder fails here."""
import numpy as np
import pytest

import shard_emul as se


@pytest.mark.parametrize("cid", sorted(se.CASES))
def test_case_table_is_consistent(cid):
    c = se.CASES[cid]
    n, total = 1 << c["log2n"], c["total"]
    assert c["log2n"] in (10, 13, 16) and c["fmt"] in se.SAMPLE_BYTES and n % c["overlap"] == 0
    assert c["wf_rows"] & (c["wf_rows"] - 1) == 0 and c["n_bins"] % 16 == 0 and c["frames"] in (1, 2)
    # shards: whole groups of 16 spectra that tile [0, total) exactly once, in order
    at = 0
    for off, cnt in c["shards"]:
        assert off == at and cnt >= 16 and off % 16 == 0 and cnt % 16 == 0, (cid, off, cnt)
        at += cnt
    assert at == total
    assert len(c["launches"]) == len(c["shards"])
    # every rank is made with max_spectra = its shard (se.make_ranks), the tightest capacity that accepts it
    for _, cnt in c["shards"]:
        assert 16 <= cnt <= total
    dev, host = se.case_bytes(c)
    assert dev <= se.DEVICE_BUDGET, "%s needs %.2f GiB on the device" % (cid, dev / 2 ** 30)
    assert host <= se.HOST_BUDGET, "%s needs %.2f GiB on the host" % (cid, host / 2 ** 30)
    hop = n // c["overlap"]
    assert se.stream_samples(c) == (total - 1) * hop + n
    # every shard's slice ends inside the stream, the last one exactly at its end
    for off, cnt in c["shards"]:
        assert off * hop + (cnt - 1) * hop + n <= se.stream_samples(c)
    off, cnt = c["shards"][-1]
    assert off * hop + (cnt - 1) * hop + n == se.stream_samples(c)
    # the environment a case sets is one the library reads, with values it does not ignore (FOSPHOR_AMD_SUB_LOG2 < 14 is)
    assert set(c["env"]) <= set(se.KNOBS)
    if cid in se.BIN_COUNT_CASES:
        assert len(c["shards"]) == 2 and c["n_bins"] not in (128, 256, 512) and 16 <= c["n_bins"] <= 512
    if "FOSPHOR_AMD_SUB_LOG2" in c["env"]:
        assert 14 <= int(c["env"]["FOSPHOR_AMD_SUB_LOG2"]) <= 34


def test_bin_count_cases_are_the_listed_ones():
    assert set(se.BIN_COUNT_CASES) <= set(se.CASES)
    got = sorted((se.CASES[k]["log2n"], se.CASES[k]["n_bins"]) for k in se.BIN_COUNT_CASES)
    assert got == [(10, 16), (13, 48), (13, 272), (16, 496)]
    assert se.CASES["m"]["total"] in (32, 64)


def test_case_table_launch_counts_follow_the_documented_rules():
    """The expected launch counts restated from the rules in DESIGN.md (sharded frames): a shard of k > 1 whole 1024-spectrum chunks
    longer than a sub-launch (sub_c chunks) goes out in ceil(k / sub_c) pieces and one k2c sum; any other shard in one piece, with
    a k2c sum when it is whole chunks, a k2b reduce when it is longer than 1024 spectra and not, and neither up to 1024."""
    for cid, c in se.CASES.items():
        n = 1 << c["log2n"]
        log2 = int(c["env"].get("FOSPHOR_AMD_SUB_LOG2", 30 if c["log2n"] == 13 else 26))
        sub_c = max((1 << log2) // (1024 * n), 1)
        for (off, cnt), got in zip(c["shards"], c["launches"]):
            k = cnt // 1024
            if cnt % 1024 == 0 and k > 1:
                want = ((k + sub_c - 1) // sub_c if k > sub_c else 1, 1, 0)
            elif cnt > 1024:
                want = (1, 0, 1)
            else:
                want = (1, 0, 0)
            assert got == want, (cid, off, cnt)


def _smallest_per_length():
    """of the shard-shape cases (the bin-count cases are all run, below)"""
    best = {}
    for cid, c in sorted(se.CASES.items()):
        if cid in se.BIN_COUNT_CASES:
            continue
        size = c["total"] << c["log2n"]
        if c["log2n"] not in best or size < best[c["log2n"]][0]:
            best[c["log2n"]] = (size, cid)
    return sorted(cid for _, cid in best.values())


@pytest.mark.parametrize("cid", sorted(set(_smallest_per_length()) | {k for k, c in se.CASES.items() if c["n_bins"] > 256}
                                        | set(se.BIN_COUNT_CASES)))
def test_case_inputs_through_the_oracle(oracle_built, cid):
    """The input builder and the oracle on the expanded frame: every sample of the frame is counted once, and above 256 bins
    both sides of row 256 -- the planes of the 9th index bit -- hold at least 1 % of the hits."""
    c = se.CASES[cid]
    n = 1 << c["log2n"]
    x, x32 = se.make_stream(c)
    assert x32.shape == (se.stream_samples(c), 2) and x32.dtype == np.float32
    assert x.size == 2 * se.stream_samples(c) and x.dtype.itemsize * 2 == se.SAMPLE_BYTES[c["fmt"]]
    o = se.make_oracle(c)
    se.oracle_frame(o, c, x32)
    assert int(o.hitcount.sum(dtype=np.uint64)) == c["total"] * n
    if c["n_bins"] > 256:
        lo, hi = se.plane_fractions(o)
        print("case %s: %.3f of the hits in bins < 256, %.3f in bins >= 256" % (cid, lo, hi))
        assert lo >= 0.01 and hi >= 0.01, "case %s: bins < 256 hold %.4f, bins >= 256 hold %.4f of the hits" % (cid, lo, hi)
    # the rows a rank computes: together the ranks cover the last min(total, wf_rows) spectra once
    rows = [r for s in c["shards"] for r in se.computed_rows(o, s, c["total"], c["wf_rows"])]
    assert len(rows) == min(c["total"], c["wf_rows"]) == len(set(rows))
