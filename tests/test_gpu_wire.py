"""GPU: the compact wire formats of the sharded frame's hit counts (include/fosphor_amd_wire.h, kernels in fosphor_wire.hip).

The staged C ABI -- wire_mask, wire_pack, wire_unpack -- is driven on emulated ranks (instances of their own on this one GPU), with
torch standing in for the collectives between the stages on the buffers the ABI exposes: the all-gather copies every rank's mask
part to every rank, the all-reduce sums the wire words as 32-bit integers.  Every comparison of counts, masks and words is
array_equal against the numpy statement of the formats (gr_fosphor_amd.dist.wire_*_numpy); whole frames are held to ONE oracle
launch with shard_emul.assert_frame_state, whose float tolerances are the only ones here.  The native path
(fosphor_amd_exchange_compact on the library's own RCCL communicator) runs on one rank in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import shard_emul as se
import wire_cases as wc
from test_gpu_parity import amd, torch_cuda		# noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
FORMS = {"packed16": 1, "sparse16": 2}


def _views(torch, ranks):
    from gr_fosphor_amd.dist import wrap_device_array
    parts = [f.partials() for f in ranks]
    return ([wrap_device_array(p.d_hc, (p.n_hc,), torch.int32) for p in parts],
            [wrap_device_array(p.d_live_sum, (p.n_cols,), torch.float32) for p in parts],
            [wrap_device_array(p.d_max, (p.n_cols,), torch.float32) for p in parts])


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def emulated_compact_exchange(torch, ranks, total, form, floats=True):
    """mask -> all-gather -> pack -> all-reduce -> unpack on every rank's current slot.  Returns what went over the "wire": the
    gathered masks, every rank's struct fosphor_amd_wire, every rank's words before the sum, the summed words."""
    from gr_fosphor_amd.dist import wrap_device_array
    world = len(ranks)
    hc, ls, mx = _views(torch, ranks)
    masks = None
    if form == "sparse16":
        for r, f in enumerate(ranks):
            assert f.wire_mask(total, world, r) == 0
        torch.cuda.synchronize()
        infos = [f.wire_info() for f in ranks]
        assert all(i.world == world and i.mask_words == i.rows // 32 and i.rows == hc[0].numel() // 64 for i in infos)
        mviews = [wrap_device_array(i.d_masks, (world, i.mask_words), torch.int32) for i in infos]
        own = torch.stack([mviews[r][r] for r in range(world)])		# the all-gather: part r comes from rank r
        for v in mviews:
            v.copy_(own)
        torch.cuda.synchronize()
        masks = _u32(own)
    packs = []
    for f in ranks:
        rv, w = f.wire_pack(total, form, world)
        assert rv == 0
        packs.append(w)
    torch.cuda.synchronize()
    assert len({(w.n_words, w.form, w.live_rows, w.rows) for w in packs}) == 1, "the ranks disagree on the layout"
    words = [wrap_device_array(w.d_words, (w.n_words,), torch.int32) for w in packs]
    before = [_u32(w) for w in words]
    wsum = torch.stack(words).sum(0, dtype=torch.int32)			# the all-reduce: 32-bit integer sum
    for w in words:
        w.copy_(wsum)
    if floats:
        ls_sum, mx_max = torch.stack(ls).sum(0), torch.stack(mx).max(0).values
        for r in range(world):
            ls[r].copy_(ls_sum); mx[r].copy_(mx_max)
    torch.cuda.synchronize()
    for f in ranks:
        assert f.wire_unpack() == 0
    torch.cuda.synchronize()
    for f in ranks:
        assert f.wire_unpack() == EINVAL		# a pack is unpacked once
    return {"masks": masks, "packs": packs, "words": before, "summed": _u32(wsum)}


@pytest.fixture(scope="module")
def syn_ranks(amd, torch_cuda):
    ranks = [amd.Fosphor(fft_len_log=wc.SYN_LOG2N, n_bins=wc.SYN_BINS, max_spectra=16, max_batches=2) for _ in range(wc.SYN_WORLD)]
    yield ranks
    for f in ranks:
        f.close()


def _write_slots(torch, ranks, counts):
    hc, _, _ = _views(torch, ranks)
    for v, c in zip(hc, counts):
        v.copy_(torch.from_numpy(c.view(np.int32)).cuda())
    torch.cuda.synchronize()
    return hc


def _sum(counts):
    return np.sum([c.astype(np.uint64) for c in counts], axis=0).astype(np.uint32)


def test_dense_round_trip(syn_ranks, torch_cuda):
    from gr_fosphor_amd.dist import wire_pack_numpy
    torch, ranks = torch_cuda, syn_ranks
    counts = wc.dense_counts()
    hc = _write_slots(torch, ranks, counts)
    st0 = [f.wire_stats() for f in ranks]
    res = emulated_compact_exchange(torch, ranks, wc.SYN_TOTAL, "packed16", floats=False)
    for r, (c, w) in enumerate(zip(counts, res["words"])):
        assert np.array_equal(w, wire_pack_numpy(c)), "rank %d: packed words" % r
    total = _sum(counts)
    assert total[0] == total[1] == 65520
    assert np.array_equal(res["summed"], wire_pack_numpy(total))
    for r, v in enumerate(hc):
        assert np.array_equal(_u32(v), total), "rank %d: slot after the unpack" % r
    for f, a, w in zip(ranks, st0, res["packs"]):
        b = f.wire_stats()
        assert (w.form, w.n_words, w.live_rows) == (FORMS["packed16"], wc.SYN_CELLS // 2, -1)
        assert b["packed16"] == a["packed16"] + 1 and b["sparse16"] == a["sparse16"] and b["fell_back"] == a["fell_back"]
        assert b["wire_bytes"] == 2 * wc.SYN_CELLS and b["live_rows"] == -1


@pytest.mark.parametrize("pattern", ["few", "half", "over"])
def test_sparse_round_trip(syn_ranks, torch_cuda, pattern):
    from gr_fosphor_amd.dist import wire_pack_numpy, wire_mask_numpy, wire_union_rows
    torch, ranks = torch_cuda, syn_ranks
    counts = wc.sparse_counts(pattern)
    hc = _write_slots(torch, ranks, counts)
    st0 = [f.wire_stats() for f in ranks]
    res = emulated_compact_exchange(torch, ranks, wc.SYN_TOTAL, "sparse16", floats=False)
    masks = np.stack([wire_mask_numpy(c) for c in counts])
    assert np.array_equal(res["masks"], masks), "presence bits"
    rows, fall_back = wire_union_rows(masks)
    assert fall_back == (pattern == "over")
    total = _sum(counts)
    for r, (c, w, p) in enumerate(zip(counts, res["words"], res["packs"])):
        assert p.live_rows == rows.size and p.rows == wc.SYN_ROWS
        if fall_back:
            assert (p.form, p.n_words) == (FORMS["packed16"], wc.SYN_CELLS // 2)
            assert np.array_equal(w, wire_pack_numpy(c)), "rank %d: packed words of the fallen-back frame" % r
        else:
            assert (p.form, p.n_words) == (FORMS["sparse16"], rows.size * 32)
            assert np.array_equal(w, wire_pack_numpy(c, rows)), "rank %d: the union's rows, in order" % r
    assert np.array_equal(res["summed"], wire_pack_numpy(total, None if fall_back else rows))
    for r, v in enumerate(hc):
        got = _u32(v)
        assert np.array_equal(got, total), "rank %d: slot differs in %d cells" % (r, (got != total).sum())	# dead rows included
    mask_bytes = 4 * wc.SYN_WORLD * (wc.SYN_ROWS // 32)
    for f, a in zip(ranks, st0):
        b = f.wire_stats()
        assert b["packed16"] == a["packed16"] and b["live_rows"] == rows.size
        if fall_back:
            assert b["fell_back"] == a["fell_back"] + 1 and b["sparse16"] == a["sparse16"]
            assert b["wire_bytes"] == 2 * wc.SYN_CELLS + mask_bytes
        else:
            assert b["sparse16"] == a["sparse16"] + 1 and b["fell_back"] == a["fell_back"]
            assert b["wire_bytes"] == 128 * rows.size + mask_bytes


def test_refusals_leave_the_slot_untouched(syn_ranks, torch_cuda):
    torch, f = torch_cuda, syn_ranks[0]
    counts = wc.sparse_counts("few")[:1]
    hc = _write_slots(torch, [f], counts)
    before = f.wire_stats()
    assert f.wire_pack(65536, "packed16", 1)[0] == EINVAL		# 16 bits do not hold the counts
    assert f.wire_pack(65536, "sparse16", 1)[0] == EINVAL
    assert f.wire_mask(65536, 1, 0) == EINVAL
    assert f.wire_pack(8, "packed16", 1)[0] == EINVAL
    assert f.wire_pack(64, 0, 1)[0] == EINVAL and f.wire_pack(64, 3, 1)[0] == EINVAL	# unknown forms
    assert f.wire_pack(64, "packed16", 0)[0] == EINVAL			# world < 1
    assert f.wire_mask(64, 2, 2) == EINVAL and f.wire_mask(64, 2, -1) == EINVAL	# rank outside the world
    assert f.wire_mask(64, 0, 0) == EINVAL
    for form in (1, 2):
        assert f.exchange_compact(None, 64, form, 1, 0) == EINVAL
    assert f.wire_unpack() == EINVAL					# nothing is packed
    assert f.wire_pack(64, "sparse16", 1)[0] == EINVAL			# sparse pack without its mask stage
    assert f.wire_mask(64, 2, 0) == 0
    assert f.wire_pack(64, "sparse16", 1)[0] == EINVAL			# ... or with the mask stage of another world
    assert f.wire_mask(64, 1, 0) == 0
    f.set_partial_slot(1)
    assert f.wire_pack(64, "sparse16", 1)[0] == EINVAL			# ... or with the mask stage of the other slot
    f.set_partial_slot(0)
    rv, w = f.wire_pack(64, "sparse16", 1)
    assert rv == 0 and w.form == FORMS["sparse16"]
    assert f.wire_pack(64, "sparse16", 1)[0] == EINVAL			# the mask stage is used up
    f.set_partial_slot(1)
    assert f.wire_unpack() == EINVAL					# the other slot is the one that was packed
    f.set_partial_slot(0)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(hc[0]), counts[0]), "a refused call (or a mask / pack stage) changed the slot"
    after = f.wire_stats()
    assert after["sparse16"] == before["sparse16"] + 1 and after["packed16"] == before["packed16"]
    assert f.wire_unpack() == 0
    torch.cuda.synchronize()
    assert np.array_equal(_u32(hc[0]), counts[0])


def _accumulate(torch, ranks, d_stream, c):
    flat = d_stream.reshape(-1)
    for fr, (off, cnt) in zip(ranks, c["shards"]):
        hop = fr.n // c["overlap"]
        lo, ln = off * hop, (cnt - 1) * hop + fr.n
        assert fr.accumulate_device(flat[lo * 2:(lo + ln) * 2], cnt, off, c["total"], overlap=c["overlap"]) == 0
    for fr in ranks:
        assert fr.finish() >= 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("cid", sorted(wc.WHOLE))
def test_whole_frames_against_one_oracle_launch(amd, torch_cuda, oracle_built, monkeypatch, cid):
    from gr_fosphor_amd.dist import wire_pack_numpy, wire_mask_numpy, wire_union_rows
    torch = torch_cuda
    c = wc.WHOLE[cid]
    for k in se.KNOBS:
        monkeypatch.delenv(k, raising=False)
    n, total = 1 << c["log2n"], c["total"]
    o = se.make_oracle(c)
    ranks = se.make_ranks(amd, c)
    keep = []
    for frame in range(c["frames"]):
        x, x32 = se.make_stream(c, frame)
        se.oracle_frame(o, c, x32)
        want = wc.oracle_counts(o)
        keep.append(torch.from_numpy(x).cuda())
        _accumulate(torch, ranks, keep[-1], c)
        hc, _, _ = _views(torch, ranks)
        assert [int(h.sum(dtype=torch.int64)) for h in hc] == [cnt * n for _, cnt in c["shards"]]
        st0 = [f.wire_stats() for f in ranks]
        res = emulated_compact_exchange(torch, ranks, total, c["form"])
        d_want = torch.from_numpy(want.view(np.int32)).cuda()
        for r, h in enumerate(hc):
            assert torch.equal(h, d_want), "case %s frame %d rank %d: slot after the unpack" % (cid, frame, r)
        if c["form"] == "sparse16":
            live = wc.live_rows(want)
            print("case %s frame %d: %d of %d rows live (%.4f), %d wire bytes per rank against %d as uint32"
                  % (cid, frame, live, want.size // 64, live / (want.size // 64), ranks[0].wire_stats()["wire_bytes"], 4 * want.size))
            rows, fall_back = wire_union_rows(wire_mask_numpy(want))
            assert not fall_back
            for f, a, p in zip(ranks, st0, res["packs"]):
                b = f.wire_stats()
                assert b["sparse16"] == a["sparse16"] + 1 and b["fell_back"] == a["fell_back"], "the sparse form did not run"
                assert p.form == FORMS["sparse16"] and p.live_rows == b["live_rows"] == live and p.n_words == 32 * live
            # the union's rows and nothing else, in order: no row of the frame before survives in the wire
            assert np.array_equal(np.bitwise_or.reduce(res["masks"], axis=0), wire_mask_numpy(want))
            assert np.array_equal(res["summed"], wire_pack_numpy(want, rows))
        else:
            assert all(p.form == FORMS["packed16"] for p in res["packs"])
            assert np.array_equal(res["summed"], wire_pack_numpy(want))
        for fr in ranks:
            assert fr.merge(total) == 0
        for fr in ranks:
            assert fr.finish() >= 0
        for r, (fr, shard) in enumerate(zip(ranks, c["shards"])):
            se.assert_frame_state(fr, o, shard, total, c["wf_rows"], "case %s frame %d rank %d" % (cid, frame, r),
                                  others_boot=(frame == 0))
    for fr in ranks:
        fr.close()


NATIVE = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["FOSPHOR_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FOSPHOR_ROOT"], "tests"))
import torch
from _pkg import gr_fosphor_amd
from gr_fosphor_amd.dist import ShardedFosphor
from oracle_lib import Oracle, gaussian_iq, add_tone

# One rank, the library's own RCCL communicator: accumulate -> fosphor_amd_exchange_compact (mask, ncclAllGather, pack, ncclGroup
# of three all-reduces, unpack, all on the count / merge stream) -> merge, four frames back to back.
torch.cuda.set_device(0)
N = 1024
wire, sliced = os.environ["FOSPHOR_TEST_WIRE"], os.environ["FOSPHOR_TEST_SLICED"] == "1"
frames = [64, 16, 128, 32]		# (wire_cases.py: up to 128 spectra leave less than half of the rows live)
sf = ShardedFosphor(gr_fosphor_amd.Fosphor, 0, 1, exchange="rccl", force_exchange=True, sliced=sliced, wire=wire,
                    n_bins=256, max_spectra=128)
assert sf.comm is not None and sf.sliced == sliced and sf.wire_form(64) == wire
sf.f.profile(True)
o = Oracle(n_bins=256)
t0 = 0
keep = []
for k, total in enumerate(frames):
    x = add_tone(gaussian_iq(total * N, 170 + k), 0.1, 0.09 + 0.02 * k, t0=t0)
    t0 += total * N
    keep.append(torch.from_numpy(x).cuda())
    sf.frame(keep[-1], total)
    assert o.process(x, strict=False, nthreads=4) == 0
    if wire == "sparse16":
        live = int(np.ascontiguousarray(o.hitcount.T).reshape(-1, 64).any(axis=1).sum())
        assert sf.f.wire_stats()["live_rows"] == live, "frame %d: live rows" % k
sf.gather_state()
f = sf.f
assert f.finish() >= 0
ms, count = f.exchange_time()
assert count == 4, "exchange_time reports %d exchanges" % count
st = f.wire_stats()
if wire == "packed16":
    assert (st["packed16"], st["sparse16"], st["fell_back"]) == (4, 0, 0), st
    assert st["wire_bytes"] == 2 * 256 * N
else:
    assert (st["packed16"], st["sparse16"], st["fell_back"]) == (0, 4, 0), st
    assert st["wire_bytes"] == 128 * st["live_rows"] + 4 * (256 * N // 2048)
assert f.waterfall_pos == o.waterfall_pos
assert np.array_equal(f.hitcount, o.hitcount.T), "hit counts differ from the oracle"
assert np.allclose(f.histogram, o.histogram, rtol=1e-4, atol=2e-6)
assert np.allclose(f.spectrum[..., 1], o.spectrum[..., 1], rtol=1e-4, atol=1e-6)
rows = (o.waterfall_pos - sum(frames) + np.arange(sum(frames))) & 1023
assert np.allclose(f.waterfall[rows], o.waterfall[rows], rtol=1e-4, atol=1e-6)
sf.close()
print("native ok %s" % st)
'''


@pytest.mark.parametrize("sliced", ["0", "1"])
@pytest.mark.parametrize("wire", ["packed16", "sparse16"])
def test_native_compact_exchange_single_rank(tmp_path, wire, sliced):
    """fosphor_amd_exchange_compact on a real RCCL communicator of one rank, both forms, with the whole-state and the
    frequency-sliced merge: state equal to the oracle's after four frames, four exchanges timed."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    script = tmp_path / "native_wire.py"
    script.write_text(NATIVE)
    env = dict(os.environ, FOSPHOR_ROOT=ROOT, FOSPHOR_TEST_WIRE=wire, FOSPHOR_TEST_SLICED=sliced)
    env.pop("FOSPHOR_AMD_WIRE", None)
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    assert p.returncode == 0 and "native ok" in p.stdout, p.stdout[-3000:]


GLOO = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["FOSPHOR_ROOT"]); sys.path.insert(0, os.path.join(os.environ["FOSPHOR_ROOT"], "tests"))
import torch, torch.distributed as dist
from _pkg import gr_fosphor_amd
from gr_fosphor_amd.dist import ShardedFosphor, shard_range
from oracle_lib import Oracle, gaussian_iq, add_tone

# The torch transport of the compact wire: two ranks share this GPU, gloo all-gathers views of the mask buffer and all-reduces
# views of the wire words between the library's stages.
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
wire = os.environ["FOSPHOR_TEST_WIRE"]
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
N = 1024
frames = [64, 32, 128]
sf = ShardedFosphor(gr_fosphor_amd.Fosphor, rank, world, exchange="torch", wire=wire, n_bins=256, max_spectra=64)
o = Oracle(n_bins=256)
t0 = 0
for k, total in enumerate(frames):
    x = add_tone(gaussian_iq(total * N, 370 + k), 0.1, 0.11 + 0.02 * k, t0=t0)
    t0 += total * N
    off, n = shard_range(total, rank, world)
    d = torch.from_numpy(x[off * N:(off + n) * N]).cuda()
    sf.frame(d, total, overlap=True)
    assert o.process(x, strict=False, nthreads=4) == 0
sf.flush()
f = sf.f
assert f.finish() >= 0
st = f.wire_stats()
assert (st["packed16"], st["sparse16"] + st["fell_back"]) == ((3, 0) if wire == "packed16" else (0, 3)), st
if wire == "sparse16":
    assert st["sparse16"] >= 1 and st["live_rows"] == int(np.ascontiguousarray(o.hitcount.T).reshape(-1, 64).any(axis=1).sum())
assert f.waterfall_pos == o.waterfall_pos
assert np.array_equal(f.hitcount, o.hitcount.T), "rank %d: hit counts differ from the oracle" % rank
assert np.allclose(f.histogram, o.histogram, rtol=1e-4, atol=2e-6), "rank %d histogram" % rank
assert np.allclose(f.spectrum[..., 1], o.spectrum[..., 1], rtol=1e-4, atol=1e-6), "rank %d spectrum" % rank
dist.barrier()
dist.destroy_process_group()
print("rank %d ok" % rank)
'''


@pytest.mark.parametrize("wire", ["packed16", "sparse16"])
def test_torch_transport_two_ranks_on_one_gpu(tmp_path, wire):
    """ShardedFosphor(exchange="torch", wire=...): the staged ABI with torch.distributed (gloo) as the collective."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    script = tmp_path / "gloo_wire.py"
    script.write_text(GLOO)
    env = dict(os.environ, FOSPHOR_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29671", WORLD_SIZE="2", FOSPHOR_TEST_WIRE=wire)
    env.pop("FOSPHOR_AMD_WIRE", None)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
        outs.append(out)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, out[-3000:])
        assert "rank %d ok" % r in out
