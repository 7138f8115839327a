"""The host side of the Reed-Solomon pass under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU.

tests/c/rs_sanitized.cpp, a program with its own main, is compiled with -fsanitize=address,undefined together with
gr-fosphor_amd/csrc/fosphor_rs_host.cpp and nothing else: the host statement, the encoder and from_decode need no other source, no
HIP header and no device.  The program runs as a child process with no device visible and nothing preloaded; nothing of this
runs on a GPU or inside Python.

The calls: fosphor_amd_rs_host over every named case of tests/rs_model.py but the 4096-job table, the call of exactly
MAX_CALL_CODEWORDS, the refusal rows of tests/test_rs_cpu.py with the last jobs that fit, fosphor_amd_rs_encode_host over the
cases' jobs turned into frames that do not overlap and over the refusal rows, and fosphor_amd_rs_from_decode at the ends of its
ranges.  Every buffer is a heap allocation of exactly its contracted size -- n_bytes of input, 64 n_jobs of jobs and of records,
out_capacity of output -- so the sanitizer's red zones stand where a byte past the contract lands.  Return values and every
output are compared byte for byte with the plain library's through ctypes on exact-size copies; a refused call leaves its outputs
at the fill."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rs_model as rm
from _pkg import gr_fosphor_amd
from test_rs_cpu import CAP, N_IN, changed, good_jobs, refusal_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "c", "rs_sanitized.cpp"), os.path.join(ROOT, "gr-fosphor_amd", "csrc", "fosphor_rs_host.cpp")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
FILL = 0xa5
EINVAL = -22


def buf(data):
    data = bytes(data)
    return struct.pack("<Q", len(data)) + data


def size(n):
    return struct.pack("<Q", max(int(n), 0))


def rs_call(data, jobs, n_bytes=None, n_jobs=None, cap=None, nulls=0):
    data, jobs = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(jobs, rm.JOB_DTYPE)
    n_bytes = len(data) if n_bytes is None else n_bytes
    n_jobs = len(jobs) if n_jobs is None else n_jobs
    cap = rm.capacity(jobs) if cap is None else cap
    return dict(kind=0, n_bytes=n_bytes, n_jobs=n_jobs, cap=cap, nulls=nulls, data=data[:max(n_bytes, 0)].tobytes(),
                jobs=jobs[:max(n_jobs, 0)].tobytes(), outs=[64 * max(min(n_jobs, len(jobs)), 0), max(cap, 0)])


def encode_call(data, jobs, cap=None, n_jobs=None, n_bytes=None, nulls=0):
    data, jobs = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(jobs, rm.JOB_DTYPE)
    cap = len(data) if cap is None else cap
    n_jobs = len(jobs) if n_jobs is None else n_jobs
    return dict(kind=1, cap=cap, n_jobs=n_jobs, n_bytes=n_bytes, nulls=nulls, data=data[:max(cap, 0)].tobytes(),
                jobs=jobs[:max(n_jobs, 0)].tobytes(), outs=[max(n_bytes, 0)])


def from_decode_call(*args, nulls=0):
    return dict(kind=2, args=args, nulls=nulls, outs=[64])


def calls():
    out = []
    for name, case in sorted(rm.cases().items()):
        if name != "full_table":
            out.append(rs_call(*case))
    frame, jobs, _ = rm.call_limit_case()
    out.append(rs_call(frame, jobs))
    out.append(rs_call(frame, rm.place([jobs[:1]] * (rm.MAX_JOBS + 1), gap=0)))
    data = np.random.default_rng(91).integers(0, 256, N_IN).astype(np.uint8)
    good = good_jobs()
    out.append(rs_call(data, good, cap=CAP))
    for bit in range(4):
        out.append(rs_call(data, good, cap=CAP, nulls=1 << bit))
    for kw in (dict(n_jobs=0), dict(n_jobs=-1), dict(n_bytes=-1), dict(n_bytes=N_IN - 1), dict(cap=-1), dict(cap=CAP - 8)):
        out.append(rs_call(data, good, **dict(dict(cap=CAP), **kw)))
    for row in refusal_rows():
        out.append(rs_call(data, changed(good[:1], **row), cap=CAP))
    out.append(rs_call(data, np.concatenate([good[:1], changed(good[1:2], out_offset=1112)]), cap=CAP))
    for row in (dict(offset=N_IN - 1275), dict(out_offset=CAP - 1120), dict(n_roots=2, n_code=3), dict(scr_width=32, scr_taps=2 ** 32 - 1, scr_init=2 ** 32 - 1)):
        out.append(rs_call(data, changed(good[:1], **row), cap=CAP))
    # the encoder: the cases' jobs with frames one behind the other, data of exactly the capacity the jobs read
    for name, case in sorted(rm.cases().items()):
        if name == "full_table":
            continue
        jobs = case[1].copy()
        jobs["offset"] = np.cumsum([0] + [int(j["depth"]) * int(j["n_code"]) for j in jobs])[:-1]
        cap = max(int(j["out_offset"]) + rm.n_data_of(j) for j in jobs)
        n = int(jobs["offset"][-1]) + int(jobs["depth"][-1]) * int(jobs["n_code"][-1])
        out.append(encode_call(np.random.default_rng(5).integers(0, 256, cap).astype(np.uint8), jobs, n_bytes=n))
        out.append(encode_call(np.random.default_rng(5).integers(0, 256, cap).astype(np.uint8), jobs, cap=cap - 1, n_bytes=n))
        out.append(encode_call(np.random.default_rng(5).integers(0, 256, cap).astype(np.uint8), jobs, n_bytes=n - 1))
    for row in refusal_rows():
        out.append(encode_call(data, changed(good[:1], **row), n_bytes=N_IN))
    for bit in range(3):
        out.append(encode_call(data, good[:1], n_bytes=N_IN, nulls=1 << bit))
    for args in ((16, 8 * 1279, 4, 255, 5), (16, 8 * 1279 - 1, 4, 255, 5), (-1, 80000, 0, 255, 5), (0, -1, 0, 255, 5), (0, 80000, -1, 255, 5),
                 (0, 80000, 0, 2, 5), (0, 80000, 0, 256, 5), (0, 80000, 0, 255, 0), (0, 80000, 0, 255, 17), (0, 80000, 2 ** 62, 255, 5),
                 (2 ** 63 - 1, 2 ** 31 - 1, 1, 3, 1), (2 ** 62, 2 ** 31 - 1, 2 ** 28 - 4081, 255, 16), (0, 24, 0, 3, 1)):
        out.append(from_decode_call(*args))
    out.append(from_decode_call(0, 80000, 0, 255, 5, nulls=1))
    return out


def encode(call):
    if call["kind"] == 0:
        return (struct.pack("<BqiqB", 0, call["n_bytes"], call["n_jobs"], call["cap"], call["nulls"]) + buf(call["data"]) + buf(call["jobs"])
                + size(call["outs"][0]) + size(call["outs"][1]))
    if call["kind"] == 1:
        return (struct.pack("<BqiqB", 1, call["cap"], call["n_jobs"], call["n_bytes"], call["nulls"]) + buf(call["data"]) + buf(call["jobs"])
                + size(call["outs"][0]))
    return struct.pack("<BqiqiiB", 2, *call["args"], call["nulls"])


def plain(lib, call):
    """the same call through ctypes into the plain library, on exact-size copies -> (return value, outputs)"""
    def arg(data, bit):
        if (call["nulls"] >> bit) & 1:
            return None, None
        b = C.create_string_buffer(bytes(data), max(len(data), 1))
        return b, C.cast(b, C.c_void_p)
    outs = [bytes([FILL]) * n for n in call["outs"]]
    if call["kind"] == 0:
        keep = [arg(call["data"], 0), arg(call["jobs"], 1), arg(outs[0], 2), arg(outs[1], 3)]
        rv = lib.fosphor_amd_rs_host(keep[0][1], call["n_bytes"], keep[1][1], call["n_jobs"], keep[2][1], keep[3][1], call["cap"])
        res = keep[2:]
    elif call["kind"] == 1:
        keep = [arg(call["data"], 0), arg(call["jobs"], 1), arg(outs[0], 2)]
        rv = lib.fosphor_amd_rs_encode_host(keep[0][1], call["cap"], keep[1][1], call["n_jobs"], keep[2][1], call["n_bytes"])
        res = keep[2:]
    else:
        job = (C.c_uint8 * 64)(*([FILL] * 64))
        rv = lib.fosphor_amd_rs_from_decode(*call["args"], None if call["nulls"] & 1 else C.cast(job, C.POINTER(gr_fosphor_amd._lib.RsJob)))
        return rv, [bytes(job)]
    return rv, [(b.raw[:n] if b is not None else o) for (b, _), n, o in zip(res, call["outs"], outs)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    compiler = shutil.which("hipcc") or shutil.which("clang++") or shutil.which("g++")
    if not compiler:
        pytest.skip("no C++ compiler on PATH")
    work = tmp_path_factory.mktemp("rs_sanitized")
    exe = str(work / "rs_sanitized")
    r = subprocess.run([compiler, "-x", "c++", "-std=c++17", "-O1", "-g"] + SANITIZE + ["-I" + os.path.join(ROOT, "include")] + SOURCES
                       + ["-o", exe], capture_output=True, text=True, timeout=300)
    if r.returncode and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()) and "error:" not in r.stderr:
        pytest.skip("sanitizer runtime missing: " + r.stderr.strip()[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, str(work)


def test_rs_host_side_under_sanitizers(program):
    exe, work = program
    todo = calls()
    cases, results = os.path.join(work, "cases"), os.path.join(work, "results")
    with open(cases, "wb") as f:
        f.write(struct.pack("<I", len(todo)) + b"".join(encode(c) for c in todo))
    env = {k: v for k, v in os.environ.items() if k in ("PATH", "HOME", "LD_LIBRARY_PATH", "ROCM_PATH", "TMPDIR")}
    env.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    assert "LD_PRELOAD" not in env
    r = subprocess.run([exe, cases, results], env=env, capture_output=True, text=True, timeout=120)
    lines = r.stderr.splitlines()
    report = "\n".join(l for l in lines if not l.startswith("case "))
    last = [l for l in lines if l.startswith("case ")][-1:]
    bad = r.returncode != 0 or "AddressSanitizer" in r.stderr or "runtime error:" in r.stderr
    assert not bad, "exit %d after %s:\n%s" % (r.returncode, last, report[:3000])
    assert lines and lines[-1] == "done %d" % len(todo)
    blob = open(results, "rb").read()
    lib = gr_fosphor_amd.load()
    at = refusals = accepted = 0
    for i, call in enumerate(todo):
        rv = struct.unpack_from("<i", blob, at)[0]
        at += 4
        got = []
        for n in call["outs"]:
            got.append(blob[at:at + n])
            at += n
        want_rv, want = plain(lib, call)
        assert rv == want_rv, (i, call["kind"], rv, want_rv)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, "call %d kind %d: output %d differs from the plain library's" % (i, call["kind"], k)
        if rv == EINVAL:
            refusals += 1
            assert all(g == bytes([FILL]) * len(g) for g in got), "call %d: a refused call wrote into a buffer" % i
        else:
            assert rv == 0
            accepted += 1
    assert at == len(blob)
    print("rs_sanitized: %d calls, %d accepted, %d refused" % (len(todo), accepted, refusals))
    assert accepted >= 20 and refusals >= 100
