"""Time-sharded display frames at every FFT length, IQ format, overlap and split (the table in tests/shard_emul.py).

Every case: emulated ranks on this one GPU accumulate their shard of the unexpanded stream, the partials are combined as the
all-reduce would, every rank merges -- and must hold the state of ONE display launch over the whole materialised frame (the
oracle's).  Counts are exact; floats use test_gpu_parity's bars.  Each case also asserts, from fosphor_amd_launch_stats, which
path every accumulate call took (FFT pieces, k2c chunk sums, k2b chunk reduces), so that a case cannot pass on another branch
than the one it is there for."""
import numpy as np
import pytest

import shard_emul as se
from test_gpu_parity import amd, torch_cuda		# noqa: F401  (fixtures)
from test_gpu_iq_sc16 import assert_same_state

pytestmark = pytest.mark.gpu


def _set_env(monkeypatch, case):
    for k in se.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("cid", sorted(se.CASES))
def test_sharded_frame_matrix(amd, torch_cuda, oracle_built, monkeypatch, cid):
    torch = torch_cuda
    c = se.CASES[cid]
    n, total, wf_rows = 1 << c["log2n"], c["total"], c["wf_rows"]
    _set_env(monkeypatch, c)
    o = se.make_oracle(c)
    ranks = se.make_ranks(amd, c)
    twins = se.make_ranks(amd, c, fmt="fp32") if c["twin"] else []
    for fr in ranks:
        assert fr.histo_scale == o.histo_scale and fr.histo_offset == o.histo_offset
    keep = []
    for frame in range(c["frames"]):
        x, x32 = se.make_stream(c, frame)
        se.oracle_frame(o, c, x32)
        if c["n_bins"] > 256:
            # on the oracle's result, before the GPU's is looked at: both planes of the 9th bin-index bit are under test
            lo, hi = se.plane_fractions(o)
            assert lo >= 0.01 and hi >= 0.01, "case %s: bins < 256 hold %.4f, bins >= 256 hold %.4f of the hits" % (cid, lo, hi)
        shared0 = [sum(fr.share_stats()[:2]) for fr in ranks]
        keep.append(torch.from_numpy(x).cuda())
        res = se.run_sharded_frame(amd, torch, ranks, keep[-1], c["shards"], total, overlap=c["overlap"])
        print("case %s frame %d: launches %s" % (cid, frame, res["launches"]))
        assert res["launches"] == c["launches"], "case %s frame %d took another path" % (cid, frame)
        # every rank counted its own spectra once, before anything was exchanged
        assert res["hc_sums"] == [cnt * n for _, cnt in c["shards"]], "case %s frame %d: partial counts" % (cid, frame)
        if c["log2n"] == 13:
            # fosphor_amd_share_stats counts every FFT launch at this length, in one form or the other
            grown = [sum(fr.share_stats()[:2]) - s for fr, s in zip(ranks, shared0)]
            assert grown == [p for p, _, _ in c["launches"]]
        for r, (fr, shard) in enumerate(zip(ranks, c["shards"])):
            se.assert_frame_state(fr, o, shard, total, wf_rows, "case %s frame %d rank %d" % (cid, frame, r),
                                  others_boot=(frame == 0))
        if twins:
            keep.append(torch.from_numpy(x32).cuda())
            res32 = se.run_sharded_frame(amd, torch, twins, keep[-1], c["shards"], total, overlap=c["overlap"])
            assert res32["launches"] == c["launches"]
            for r, (a, b) in enumerate(zip(ranks, twins)):
                assert_same_state(a, b, "case %s rank %d: sc16 vs fp32 ranks fed the widened values" % (cid, r))
    for fr in ranks + twins:
        fr.close()
