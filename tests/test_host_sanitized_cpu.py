"""The library's host side under AddressSanitizer and UndefinedBehaviorSanitizer, on the CPU.

Every device pass is held, bit for bit, to a host statement (fosphor_amd_*_host), and about forty more host-only entry points size
the buffers that callers and tests allocate.  The suite reaches them through ctypes only, in the -O3 library, with numpy arrays
that the tests pad with guards: a read one element past a buffer, or a signed overflow in a size rule, shows nowhere.  Here the
library's sources are compiled once more with -fsanitize=address,undefined and linked into tests/c/host_sanitized.cpp, a program
with its own main that calls only entry points without a struct fosphor * and no HIP function.  Nothing is preloaded into Python.

Where the calls come from.  No case is invented here: the calls are the ones the suite's own CPU tests make.  The listed test
functions (HARVEST) run once against the plain library while a recorder stands between them and ctypes; it notes the entry point,
the scalar arguments and, for every pointer, exactly as many bytes as the header's contract promises for those arguments
(CONTRACT) -- not the padded numpy array the test handed over.  That covers the named cases of the twelve model modules (through the modules' own
test_host_against_model), the refusal tables (test_einval_table of every pass, tests/test_job_refusals_cpu.py) with the last jobs that fit, which those tables end with, the planners over
tests/test_count_plan_cpu.py and tests/tile_walk_cases.py, and the views of tests/test_view_cpu.py.  extremes() adds the size
rules, constructors, designs and derive functions at the ends of their ranges, with the argument tuples of
tests/job_scale_cases.py (n = 2^31 - 1, 65536-entry tables); no host statement runs at that n.  For decode and soft, whose host
statements read kept(T) coded bits from ceil(n_coded / b) symbols and write 8 ceil(n_bits / 64) owned bytes, the harvest takes the
modules' named cases, refusal tables, numerical edges and from_decide / derive tests, and extremes() adds fosphor_amd_decode_steps
around MAX_STEPS and at n = 2^31 - 1 and both from_decide constructors over a decide job at offsets of 2^62.

The rule for buffers.  The driver puts every buffer of a call into a heap allocation of its own of exactly the recorded size: the
IQ, the job table, taps, templates, windows, the unique word, the thresholds, the records and each output.  The sanitizer's red
zones then stand where a read or write one element past the contract lands.  A NULL stays NULL.  Outputs are filled with 0xa5
first; a refused call must leave every buffer as it was.

What is compared.  The driver's return value and every buffer after the call, byte for byte, with the same call through ctypes
into the plain library on exact-size copies (instrumentation does not change IEEE results, and with -ffp-contract=off the
optimisation level does not either); no tolerance.  The size rules are also compared with the integer arithmetic the model
modules state for them (extremes()).

Not reproduced: calls in which a test skews a pointer off its 8-byte boundary to see the alignment refused (the buffers of numpy
and ctypes all begin on one, and so does an allocation of its own): they are not recorded.  A call that claims more than
MAX_BYTES for a buffer must be a refusal and gets an empty buffer in its place, which the refusal must not read.

Dropped for time (whole named interior cases; every last-fit, refusal and extreme-argument case is kept): none.  The calls of
MAX_CALL_STEPS of decode and soft (test_call_limit of both modules, 2^22 steps each) are in: their children end within seconds.

fosphor_amd_measure_host pins, in its source, which of two NaN operands an operation hands on, so that both builds give the same
bytes on measure_model's case "nonfinite".
"""
import concurrent.futures
import ctypes as C
import inspect
import itertools
import os
import shutil
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

from _pkg import gr_fosphor_amd

L_ = gr_fosphor_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gr-fosphor_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "c", "host_sanitized.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
MAX_BYTES = 1 << 26			# a buffer a case may claim
FILL = 0xa5
ALIGN = 8				# what the headers ask of a pointer at the most, and what numpy and ctypes give every buffer at the least
JOBS = 16				# compilers at a time
CHILD_TIMEOUT = 120			# seconds, per child process
MIN_REFUSED, MIN_ACCEPTED = 3, 3		# calls of each host statement the harvest must hold; mask_row_host's table has 3 refusals
BUILD_TIMEOUT = 900			# seconds, per compiler or linker

# ---- the contract: bytes behind every pointer, from the call's own arguments ------------------------------------------------------

sz = C.sizeof
REC = {k: getattr(gr_fosphor_amd.Fosphor, k.upper() + "_RECORD_DTYPE").itemsize
       for k in ("measure", "correlate", "psd", "symbols", "carrier", "decide", "decode", "soft")}
IQ_BYTES = {0: 8, 1: 4, 2: 4}		# fp32, fp16, sc16 pairs


def _log_len(log):
    return 4 << log if 0 <= log <= 16 else 0


# name -> {argument index: (bytes from the argument list a, is an output)}
CONTRACT = {
    "fosphor_amd_extract_host": {0: (lambda a: a[1] * IQ_BYTES.get(a[2], 8), 0), 3: (lambda a: a[4] * sz(L_.ExtractJob), 0),
                                 5: (lambda a: a[6] * 4, 0), 7: (lambda a: a[8] * 8, 1)},
    "fosphor_amd_measure_host": {0: (lambda a: a[1] * 8, 0), 2: (lambda a: a[3] * sz(L_.MeasureJob), 0),
                                 4: (lambda a: a[3] * REC["measure"], 1)},
    "fosphor_amd_demod_host": {0: (lambda a: a[1] * 8, 0), 2: (lambda a: a[3] * sz(L_.DemodJob), 0), 4: (lambda a: a[5] * 4, 1)},
    "fosphor_amd_correlate_host": {0: (lambda a: a[1] * 8, 0), 2: (lambda a: a[3] * 8, 0), 4: (lambda a: a[5] * sz(L_.CorrelateJob), 0),
                                   6: (lambda a: a[5] * REC["correlate"], 1), 7: (lambda a: a[8] * 4, 1)},
    "fosphor_amd_resample_host": {0: (lambda a: a[1] * 8, 0), 2: (lambda a: a[3] * sz(L_.ResampleJob), 0), 4: (lambda a: a[5] * 4, 0),
                                  6: (lambda a: a[7] * 8, 1)},
    "fosphor_amd_psd_host": {0: (lambda a: a[1] * 8, 0), 2: (lambda a: a[3] * 4, 0), 4: (lambda a: a[5] * sz(L_.PsdJob), 0),
                             6: (lambda a: a[5] * REC["psd"], 1), 7: (lambda a: a[8] * 4, 1)},
    "fosphor_amd_symbols_host": {0: (lambda a: a[1] * 8, 0), 2: (lambda a: a[3] * sz(L_.SymbolsJob), 0),
                                 4: (lambda a: a[3] * REC["symbols"], 1), 5: (lambda a: a[6] * 8, 1)},
    "fosphor_amd_carrier_host": {0: (lambda a: a[1] * 8, 0), 2: (lambda a: a[3] * sz(L_.CarrierJob), 0),
                                 4: (lambda a: a[3] * REC["carrier"], 1), 5: (lambda a: a[6] * 8, 1)},
    "fosphor_amd_decide_host": {0: (lambda a: a[1] * 8, 0), 2: (lambda a: a[3] * sz(L_.DecideJob), 0), 4: (lambda a: a[5], 0),
                                6: (lambda a: a[3] * REC["decide"], 1), 7: (lambda a: a[8], 1)},
    "fosphor_amd_decode_host": {0: (lambda a: a[1], 0), 2: (lambda a: a[3] * sz(L_.DecodeJob), 0),
                                4: (lambda a: a[3] * REC["decode"], 1), 5: (lambda a: a[6], 1)},
    "fosphor_amd_soft_host": {0: (lambda a: a[1] * 8, 0), 2: (lambda a: a[3] * sz(L_.SoftJob), 0),
                              4: (lambda a: a[3] * REC["soft"], 1), 5: (lambda a: a[6], 1)},
    "fosphor_amd_bursts_host": {0: (lambda a: max(a[1], 0) * max(a[2], 0) * 4, 0), 3: (lambda a: a[2] * 4, 0),
                                4: (lambda a: sz(L_.BurstCfg), 0), 5: (lambda a: sz(L_.BurstResult), 1),
                                6: (lambda a: a[7] * sz(L_.Burst), 1)},
    "fosphor_amd_mask_row_host": {0: (lambda a: a[3] * 4, 0), 1: (lambda a: a[3] * 4, 0), 2: (lambda a: a[3] * 4, 0),
                                  4: (lambda a: sz(L_.MaskRow), 1)},
    "fosphor_amd_detect_bands_host": {0: (lambda a: a[1] * 4, 0), 5: (lambda a: a[6] * sz(L_.Band), 1), 7: (lambda a: 4, 1)},
    "fosphor_amd_demod_n_out": {}, "fosphor_amd_correlate_n_out": {}, "fosphor_amd_resample_n_out": {},
    "fosphor_amd_psd_n_seg": {}, "fosphor_amd_symbols_max_out": {},
    "fosphor_amd_decode_steps": {4: (lambda a: 3 * 2, 0)},				# "const uint16_t punct[3]"
    "fosphor_amd_extract_from_burst": {0: (lambda a: sz(L_.Burst), 0), 6: (lambda a: sz(L_.ExtractJob), 1), 7: (lambda a: 4, 1)},
    "fosphor_amd_measure_from_extract": {0: (lambda a: sz(L_.ExtractJob), 0), 2: (lambda a: sz(L_.MeasureJob), 1)},
    "fosphor_amd_demod_from_extract": {0: (lambda a: sz(L_.ExtractJob), 0), 3: (lambda a: sz(L_.DemodJob), 1)},
    "fosphor_amd_correlate_from_extract": {0: (lambda a: sz(L_.ExtractJob), 0), 5: (lambda a: sz(L_.CorrelateJob), 1)},
    "fosphor_amd_resample_from_extract": {0: (lambda a: sz(L_.ExtractJob), 0), 4: (lambda a: sz(L_.ResampleJob), 1)},
    "fosphor_amd_psd_from_extract": {0: (lambda a: sz(L_.ExtractJob), 0), 8: (lambda a: sz(L_.PsdJob), 1)},
    "fosphor_amd_symbols_from_extract": {0: (lambda a: sz(L_.ExtractJob), 0), 4: (lambda a: sz(L_.SymbolsJob), 1)},
    "fosphor_amd_symbols_from_resample": {0: (lambda a: sz(L_.ResampleJob), 0), 4: (lambda a: sz(L_.SymbolsJob), 1)},
    "fosphor_amd_carrier_from_symbols": {0: (lambda a: sz(L_.SymbolsJob), 0), 1: (lambda a: REC["symbols"], 0),
                                         7: (lambda a: sz(L_.CarrierJob), 1)},
    "fosphor_amd_decide_from_carrier": {0: (lambda a: sz(L_.CarrierJob), 0), 1: (lambda a: REC["carrier"], 0),
                                        8: (lambda a: sz(L_.DecideJob), 1)},
    "fosphor_amd_decode_from_decide": {0: (lambda a: sz(L_.DecideJob), 0), 1: (lambda a: REC["decide"], 0),
                                       4: (lambda a: sz(L_.DecodeJob), 1)},
    "fosphor_amd_soft_from_decide": {0: (lambda a: sz(L_.DecideJob), 0), 1: (lambda a: REC["decide"], 0),
                                     4: (lambda a: sz(L_.SoftJob), 1)},
    "fosphor_amd_view_from_render": {2: (lambda a: sz(L_.Render), 0), 5: (lambda a: sz(L_.View), 1)},
    "fosphor_amd_extract_design": {3: (lambda a: a[1] * 4, 1)},
    "fosphor_amd_resample_design": {4: (lambda a: max(a[0], 0) * max(a[2], 0) * 4, 1)},
    "fosphor_amd_resample_ratio": {3: (lambda a: 4, 1), 4: (lambda a: 4, 1), 5: (lambda a: 8, 1)},
    "fosphor_amd_psd_window": {2: (lambda a: _log_len(a[1]), 1)},
    "fosphor_amd_psd_twiddles": {0: (lambda a: 512 * 16, 1)},
    "fosphor_amd_symbols_twiddles": {1: (lambda a: a[0] * 16, 1)},
    "fosphor_amd_measure_derive": {0: (lambda a: REC["measure"], 0), 2: (lambda a: sz(L_.MeasureValues), 1)},
    "fosphor_amd_correlate_derive": {0: (lambda a: REC["correlate"], 0), 2: (lambda a: sz(L_.CorrelateValues), 1)},
    "fosphor_amd_psd_derive": {0: (lambda a: REC["psd"], 0), 2: (lambda a: sz(L_.PsdValues), 1)},
    "fosphor_amd_symbols_derive": {0: (lambda a: REC["symbols"], 0), 3: (lambda a: sz(L_.SymbolsValues), 1)},
    "fosphor_amd_carrier_derive": {0: (lambda a: REC["carrier"], 0), 2: (lambda a: sz(L_.CarrierValues), 1)},
    "fosphor_amd_decide_derive": {0: (lambda a: REC["decide"], 0), 2: (lambda a: sz(L_.DecideValues), 1)},
    "fosphor_amd_decode_derive": {0: (lambda a: REC["decode"], 0), 1: (lambda a: sz(L_.DecodeValues), 1)},
    "fosphor_amd_soft_derive": {0: (lambda a: REC["soft"], 0), 1: (lambda a: sz(L_.SoftValues), 1)},
    "fosphor_amd_view_span": {3: (lambda a: 4, 1), 4: (lambda a: 4, 1)},
    "fosphor_amd_mask_from_points": {1: (lambda a: a[3] * 8, 0), 2: (lambda a: a[3] * 4, 0), 4: (lambda a: a[0] * 4, 1)},
    "fosphor_amd_detect_bin_y": {3: (lambda a: a[0] * 4, 1)},
    "fosphor_amd_cmap_generate": {1: (lambda a: a[2] * 4, 1)},
    "fosphor_amd_freq_axis_build": {0: (lambda a: sz(L_.FreqAxis), 1)},
    "fosphor_amd_freq_axis_render": {0: (lambda a: sz(L_.FreqAxis), 0), 1: (lambda a: 32, 1)},		# "str (>= 32 bytes)"
    "fosphor_amd_host_thresholds": {3: (lambda a: (a[0] + 1) * 8, 1)},
    "fosphor_amd_host_twiddle_count": {},
    "fosphor_amd_host_twiddles": {0: (lambda a: 2 * 4 * gr_fosphor_amd.load().fosphor_amd_host_twiddle_count(), 1)},
    "fosphor_amd_plan_piece_batches": {},
    "fosphor_amd_plan_count": {8: (lambda a: sz(L_.CountPlan), 1)},
    "fosphor_amd_plan_k1": {10: (lambda a: sz(L_.K1Plan), 1)},
    "fosphor_amd_demod_atan2_turns": {},
    "fosphor_amd_demod_atan2_turns_n": {0: (lambda a: a[2] * 8, 0), 1: (lambda a: a[2] * 8, 0), 3: (lambda a: a[2] * 4, 1)},
    "fosphor_amd_carrier_cossin_turns": {1: (lambda a: 8, 1), 2: (lambda a: 8, 1)},
    "fosphor_amd_carrier_cossin_turns_n": {0: (lambda a: a[1] * 8, 0), 2: (lambda a: a[1] * 8, 1), 3: (lambda a: a[1] * 8, 1)},
    "fosphor_amd_psd_ratio_from_db": {},
    "fosphor_amd_version": {},
}


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents")


def _address(v):
    """the address a ctypes call would pass for v"""
    if v is None:
        return None
    if isinstance(v, int):
        return v
    if isinstance(v, (bytes, bytearray)):
        return C.cast(C.c_char_p(bytes(v)), C.c_void_p).value
    if hasattr(v, "_obj"):				# byref()
        return C.addressof(v._obj)
    if isinstance(v, C.c_void_p):
        return v.value
    if hasattr(v, "contents"):				# a POINTER instance
        return C.cast(v, C.c_void_p).value
    return C.addressof(v)				# a structure or an array


class Call:
    """one recorded call: the entry point, its arguments (("i", v), ("d", v), ("null",) or ("buf", bytes, is_output)) and where
    in the suite it was made"""

    def __init__(self, name, args, origin):
        self.name, self.args, self.origin = name, args, origin


class Recorder:
    """stands between the suite's code and the plain library's CDLL; notes the calls of CONTRACT, passes every call on"""

    def __init__(self, real):
        self._real, self.calls, self.origin = real, [], "?"
        self.misaligned, self.oversize, self.ran = 0, 0, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in CONTRACT:
            return fn

        def recorded(*args):
            call = self._note(name, args)
            rv = fn(*args)
            if call is not None:
                call.plain_rv = rv
                self.calls.append(call)
            return rv
        return recorded

    def _note(self, name, args):
        types = L_.SIGNATURES[name][1]
        assert len(args) == len(types), name
        flat = []
        for v, t in zip(args, types):
            if _is_pointer(t):
                flat.append(None)
            elif t in (C.c_float, C.c_double):
                flat.append(float(v))
            else:
                flat.append(int(v))
        out, oversize = [], False
        for i, (v, t) in enumerate(zip(args, types)):
            if not _is_pointer(t):
                if t is C.c_float:
                    out.append(("d", float(np.float32(flat[i]))))
                elif t is C.c_double:
                    out.append(("d", flat[i]))
                else:
                    out.append(("i", flat[i]))
                continue
            at = _address(v)
            if at is None:
                out.append(("null",))
                continue
            if at % ALIGN:				# a test skewed the pointer (by 2 or 4 bytes): a call about alignment, and an
                self.misaligned += 1			# allocation of its own is aligned.  Left out before a byte of it is read
                return None
            size, is_out = CONTRACT[name][i]
            size = max(int(size(flat)), 0)
            if size > MAX_BYTES:
                size, oversize = 0, True
            data = C.string_at(at, size)
            if is_out:
                data = bytes([FILL]) * size
            out.append(("buf", data, is_out))
        if oversize:
            self.oversize += 1
            # the claim cannot be met: the call must be a refusal, and is handed empty buffers in the claim's place
        call = Call(name, out, self.origin)
        call.must_refuse = oversize
        return call


def replay_plain(call):
    """the same call through ctypes into the plain library, on exact-size copies -> (return value as 8 bytes, buffers after)"""
    fn = getattr(L_.load() if not isinstance(L_._lib, Recorder) else L_._lib._real, call.name)
    res = L_.SIGNATURES[call.name][0]
    keep, args = [], []
    for a in call.args:
        if a[0] == "buf":
            b = C.create_string_buffer(a[1], len(a[1])) if len(a[1]) else C.create_string_buffer(1)
            keep.append((b, len(a[1])))
            args.append(C.cast(b, C.c_void_p))
        elif a[0] == "null":
            args.append(None)
        else:
            args.append(a[1])
    types = L_.SIGNATURES[call.name][1]
    args = [C.cast(v, t) if (v is not None and _is_pointer(t) and t is not C.c_void_p) else v for v, t in zip(args, types)]
    rv = fn(*args)
    if res is None:
        bits = 0
    elif res is C.c_char_p:
        bits = len(rv) if rv else 0
    elif res is C.c_double:
        bits = struct.unpack("<Q", struct.pack("<d", rv))[0]
    elif res is C.c_float:
        bits = struct.unpack("<I", struct.pack("<f", rv))[0]
    else:
        bits = int(rv) & 0xffffffffffffffff
    return bits, [b.raw[:n] for b, n in keep]


def encode(calls):
    parts = [struct.pack("<I", len(calls))]
    for c in calls:
        name = c.name.encode()
        parts.append(struct.pack("<H", len(name)) + name + struct.pack("<I", len(c.args)))
        for a in c.args:
            if a[0] == "i":
                v = a[1]
                parts.append(struct.pack("<Bq", 0, v if v < 1 << 63 else v - (1 << 64)))
            elif a[0] == "d":
                parts.append(struct.pack("<Bd", 1, a[1]))
            elif a[0] == "null":
                parts.append(b"\x02")
            else:
                parts.append(struct.pack("<BQ", 3, len(a[1])))
                parts.append(a[1])
    return b"".join(parts)


def decode(blob, calls):
    """the driver's results -> [(return bits, buffers)]"""
    at, out = 0, []
    for c in calls:
        bits = struct.unpack_from("<Q", blob, at)[0]
        at += 8
        bufs = []
        for a in c.args:
            if a[0] == "buf":
                bufs.append(blob[at:at + len(a[1])])
                at += len(a[1])
        out.append((bits, bufs))
    assert at == len(blob), "the driver wrote %d bytes, the cases account for %d" % (len(blob), at)
    return out


# ---- the build ------------------------------------------------------------------------------------------------------------------

def makefile_hipflags():
    arch = "gfx950"
    for line in open(os.path.join(ROOT, "Makefile")):
        if line.startswith("ARCH"):
            arch = line.split("=", 1)[1].strip()
        if line.startswith("HIPFLAGS"):
            return line.split(":=", 1)[1].replace("$(ARCH)", arch).split()
    raise AssertionError("the Makefile has no HIPFLAGS")


@pytest.fixture(scope="session")
def driver(tmp_path_factory):
    """the library's sources, with the Makefile's HIPFLAGS as they are, and the driver with ASan and UBSan -> the program"""
    hipcc = shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not on PATH")
    if not os.path.exists(gr_fosphor_amd.LIB_PATH):
        gr_fosphor_amd.build()
    work = tmp_path_factory.mktemp("host_sanitized")
    flags = makefile_hipflags() + ["-g"]
    host = [x for f in SANITIZE for x in ("-Xarch_host", f)]
    sources = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")))
    jobs = [([hipcc] + flags + host + ["-x", "hip", "-c", s, "-o", str(work / (os.path.basename(s) + ".o"))], s) for s in sources]
    jobs.append(([hipcc, "-std=c++17", "-O1", "-g", "-pthread"] + SANITIZE + ["-I" + os.path.join(ROOT, "include"), "-c", DRIVER,
                  "-o", str(work / "driver.o")], DRIVER))
    t0 = time.time()

    def compile_one(job):
        cmd, src = job
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=BUILD_TIMEOUT)
        return src, r.returncode, r.stdout

    with concurrent.futures.ThreadPoolExecutor(max_workers=JOBS) as pool:
        done = list(pool.map(compile_one, jobs))
    failed = [(src, out) for src, rc, out in done if rc]
    assert not failed, "\n".join("%s:\n%s" % (src, out[-3000:]) for src, out in failed)
    exe = work / "host_sanitized"
    arch = [f for f in flags if f.startswith("--offload-arch=")]
    link = subprocess.run([hipcc] + arch + ["-pthread"] + SANITIZE + [str(work / (os.path.basename(s) + ".o")) for _, s in jobs[:-1]]
                          + [str(work / "driver.o"), "-ldl", "-o", str(exe)], capture_output=True, text=True, timeout=BUILD_TIMEOUT)
    if link.returncode and ("asan" in link.stderr.lower() or "ubsan" in link.stderr.lower()):
        pytest.skip("sanitizer runtime missing: " + link.stderr.strip()[-300:])
    assert link.returncode == 0, link.stderr[-3000:]
    print("host_sanitized: built in %.1f s" % (time.time() - t0))
    return str(exe), str(work)


def child_env():
    """an environment that shows the child no GPU: the program opens none wherever the suite runs"""
    env = {k: v for k, v in os.environ.items() if k in ("PATH", "HOME", "LD_LIBRARY_PATH", "ROCM_PATH", "TMPDIR")}
    env.update(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ASAN_OPTIONS="detect_leaks=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    assert "LD_PRELOAD" not in env
    return env


def run_driver(driver, calls, tag):
    """the calls in one child process -> [(return bits, buffers)]; fails on a report, printing it"""
    exe, work = driver
    cases, results = os.path.join(work, tag + ".cases"), os.path.join(work, tag + ".results")
    with open(cases, "wb") as f:
        f.write(encode(calls))
    r = subprocess.run([exe, cases, results], env=child_env(), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    lines = r.stderr.splitlines()
    last = [l for l in lines if l.startswith("case ")][-1:] or ["(none)"]
    report = "\n".join(l for l in lines if not l.startswith("case "))
    where = ""
    if last[0] != "(none)":
        where = calls[int(last[0].split()[1])].origin
    bad = r.returncode != 0 or "AddressSanitizer" in r.stderr or "runtime error:" in r.stderr
    if bad:
        print(report[-6000:])
    assert not bad, "%s: exit %d in %s, from %s:\n%s" % (tag, r.returncode, last[0], where, report[:1500])
    assert lines and lines[-1] == "done %d" % len(calls)
    with open(results, "rb") as f:
        return decode(f.read(), calls)


# ---- where the calls come from -----------------------------------------------------------------------------------------------------

# module -> the test functions that call the host side (all parametrisations); None: every test_ function of the module
HARVEST = {
    "test_extract_cpu": ["test_host_function_against_model", "test_design_against_formula", "test_from_burst_by_hand",
                         "test_host_einval_table"],
    "test_measure_cpu": ["test_host_against_model", "test_a_job_cut_in_two_recombines", "test_einval_table",
                         "test_measure_from_extract", "test_derive_degenerate_records_are_zeros", "test_derive_two_pulses"],
    "test_demod_cpu": ["test_atan2_turns_seam_table", "test_host_against_model", "test_the_cut_rule", "test_n_out_and_from_extract",
                       "test_einval_table"],
    "test_correlate_cpu": None, "test_resample_cpu": None, "test_psd_cpu": None, "test_symbols_cpu": None,
    "test_carrier_cpu": None, "test_decide_cpu": None,
    "test_decode_cpu": ["test_host_against_model", "test_einval_table", "test_steps_from_decide_and_derive", "test_call_limit"],
    "test_soft_cpu": ["test_host_against_model", "test_einval_table", "test_numerical_edges", "test_from_decide_and_derive",
                      "test_call_limit"],
    "test_burst_cpu": ["test_host_function_against_model", "test_model_by_hand", "test_host_overflows", "test_host_einval_table"],
    "test_mask_cpu": ["test_row_rule_fixed_cases", "test_row_rule_random_rows", "test_row_host_argument_errors",
                      "test_from_points_bit_for_bit", "test_from_points_random_bit_for_bit", "test_from_points_argument_errors"],
    "test_detect_cpu": ["test_bin_y_table", "test_band_rules_fixed_cases", "test_band_rules_random_cases",
                        "test_bands_host_argument_errors"],
    "test_job_refusals_cpu": None,
    "test_count_plan_cpu": None,
    "test_tile_walk_cases_cpu": None,
    "test_view_cpu": ["test_span_rule", "test_span_argument_errors", "test_view_from_render_defaults_give_the_whole_buffer",
                      "test_view_from_render_zooms", "test_view_from_render_demo_zoom_values", "test_view_from_render_argument_errors"],
    "test_axis": None,
    "test_cmap": None,
}
# of the modules harvested whole: tests that compile kernels, need other fixtures or make a million calls
LEFT_OUT = ("spill", "resources", "without_a_device", "exported_and_bound", "header", "million", "dtype", "estimator_finds", "oracle")


class Unsupported(Exception):
    pass


def _fixture_function(obj):
    get = getattr(obj, "_get_wrapped_function", None)
    if get is not None:
        return get()
    wrapped = getattr(obj, "__pytest_wrapped__", None)
    return wrapped.obj if wrapped is not None else None


def _fixture_params(obj):
    m = getattr(obj, "_fixture_function_marker", None) or getattr(obj, "_pytestfixturefunction", None)
    return getattr(m, "params", None)


def _resolve(mod, name, request_param, cache):
    """the value of fixture `name` of module mod, as pytest would make it (module fixtures without teardown work only)"""
    if name in cache:
        return cache[name]
    obj = getattr(mod, name, None)
    fn = _fixture_function(obj) if obj is not None else None
    if fn is None:
        raise Unsupported(name)
    kw = {}
    for p in inspect.signature(fn).parameters:
        if p == "request":
            kw[p] = type("Request", (), {"param": request_param.get(name)})()
        else:
            kw[p] = _resolve(mod, p, request_param, cache)
    v = fn(**kw)
    if inspect.isgenerator(v):
        v = next(v)
    cache[name] = v
    return v


def _parametrisations(fn):
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
    axes = []
    for m in marks:
        names = [s.strip() for s in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
        values = []
        for v in m.args[1]:
            v = v.values if isinstance(v, type(pytest.param(0))) else v
            values.append(dict(zip(names, v if len(names) > 1 else [v])))
        axes.append(values)
    for combo in itertools.product(*axes):
        kw = {}
        for d in combo:
            kw.update(d)
        yield kw


def harvest(rec):
    """run the suite's own calls through the recorder"""
    import importlib
    for modname, names in HARVEST.items():
        mod = importlib.import_module(modname)
        if names is None:
            names = [n for n, f in vars(mod).items() if n.startswith("test_") and callable(f) and not any(w in n for w in LEFT_OUT)]
        for tname in names:
            fn = getattr(mod, tname)
            if any(m.name in ("gpu", "skip", "skipif") for m in getattr(fn, "pytestmark", [])):
                continue
            for kw in _parametrisations(fn):
                fixtures = [p for p in inspect.signature(fn).parameters if p not in kw]
                # a parametrised fixture: once per parameter
                choices = [{}]
                for p in fixtures:
                    obj = getattr(mod, p, None)
                    params = _fixture_params(obj) if obj is not None else None
                    if params:
                        choices = [dict(c, **{p: q}) for c in choices for q in params]
                for choice in choices:
                    rec.origin = "%s::%s%s" % (modname, tname, "[%s]" % ",".join(str(v)[:24] for v in list(kw.values()) + list(choice.values()))
                                               if kw or choice else "")
                    try:
                        args = dict(kw)
                        cache = {}
                        for p in fixtures:
                            args[p] = _resolve(mod, p, choice, cache)
                    except Unsupported as e:
                        raise AssertionError("%s needs fixture %s, which the harvest cannot make" % (rec.origin, e))
                    except pytest.skip.Exception as e:
                        raise AssertionError("a fixture of %s skipped (%s): its calls are missing from the harvest" % (rec.origin, e))
                    try:
                        fn(**args)
                    except pytest.skip.Exception as e:
                        raise AssertionError("%s skipped (%s): its calls are missing from the harvest" % (rec.origin, e))
                    rec.ran[modname] = rec.ran.get(modname, 0) + 1


def extremes(L, F):
    """the size rules, constructors, designs and derive functions at the ends of their ranges; -> what the models' integer
    arithmetic says of the size rules, as (call index offset, expected) is checked right here against the plain library"""
    import decode_model as dcm
    import demod_model as dm
    import correlate_model as cm
    import job_scale_cases as jc
    import psd_model as pm
    import resample_model as rm
    import symbols_model as sm
    import test_view_cpu as tv
    n = jc.LONG_N

    def fits(want):
        """a count an int cannot hold is refused"""
        return want if want <= 2 ** 31 - 1 else -22
    assert n == 2 ** 31 - 1
    L.fosphor_amd_version()
    # the size rules at n = 2^31 - 1, against the models' integers
    for spec in (jc.PSD_LONG, jc.PSD_LONG_PARTS):
        assert L.fosphor_amd_psd_n_seg(n, spec["fft_len_log"], spec["hop"]) == fits(pm.n_seg(n, spec["fft_len_log"], spec["hop"]))
    for log in pm.LOGS:
        for hop in (1, 1 << log):
            assert L.fosphor_amd_psd_n_seg(n, log, hop) == fits(pm.n_seg(n, log, hop))
    for spec in jc.SYM_LONG.values():
        assert L.fosphor_amd_symbols_max_out(n, spec["sps"]) == fits(sm.max_out(n, spec["sps"]))
    for sps in (sm.MIN_SPS, sm.MAX_SPS):
        assert L.fosphor_amd_symbols_max_out(n, sps) == fits(sm.max_out(n, sps))
    for mode in (dm.POWER, dm.PHASE, dm.FM):
        for avg in (1, 2, dm.MAX_AVG):
            assert L.fosphor_amd_demod_n_out(mode, n, avg) == fits(dm.n_out(mode, n, avg))
    for trace in (cm.NONE, cm.RHO, cm.C):
        for t in (1, jc.TIE_T, cm.MAX_TPL):
            assert L.fosphor_amd_correlate_n_out(trace, n, t) == fits(cm.n_out(trace, n, t))
    for up, down in tuple(rm.RATIOS) + ((jc.RS_UP, jc.RS_TILE[0]), (jc.RS_UP, jc.RS_DIRECT[0]), (rm.MAX_UP, rm.MAX_DOWN)):
        for q in tuple(rm.QS) + (jc.RS_TILE[1], jc.RS_DIRECT[1], rm.MAX_BRANCH):
            for phase0 in (0, up - 1):
                want = fits(rm.max_n_out(n, up, down, q * up, phase0)) if 1 <= q <= rm.MAX_BRANCH else -22
                assert L.fosphor_amd_resample_n_out(n, up, down, q * up, phase0) == want, (up, down, q, phase0)
    # the constructors over an extract job of 2^31 - 1 outputs at an offset of 2^62
    e = L_.ExtractJob(first=0, out_offset=2 ** 62, n_out=n, decim=1, phase_inc=0, phase0=0, taps_offset=0, n_taps=1)
    L.fosphor_amd_measure_from_extract(C.byref(e), 0.5, C.byref(L_.MeasureJob()))
    L.fosphor_amd_demod_from_extract(C.byref(e), dm.FM, dm.MAX_AVG, C.byref(L_.DemodJob()))
    L.fosphor_amd_correlate_from_extract(C.byref(e), 2 ** 62, cm.MAX_TPL, cm.C, 0.5, C.byref(L_.CorrelateJob()))
    L.fosphor_amd_psd_from_extract(C.byref(e), 2 ** 62, 10, 128, 1, 1, 0.99, 0.0025, C.byref(L_.PsdJob()))
    L.fosphor_amd_symbols_from_extract(C.byref(e), 64, sm.ESTIMATE, 0.0, C.byref(L_.SymbolsJob()))
    r = L_.ResampleJob()
    L.fosphor_amd_resample_from_extract(C.byref(e), rm.MAX_UP, 1, rm.MAX_UP * rm.MAX_BRANCH, C.byref(r))
    L.fosphor_amd_resample_from_extract(C.byref(e), 1, rm.MAX_DOWN, rm.MAX_BRANCH, C.byref(r))
    L.fosphor_amd_symbols_from_resample(C.byref(r), 2, sm.FIXED, 0.4, C.byref(L_.SymbolsJob()))
    # decode and soft: rule 2's T at n = 2^31 - 1 and around MAX_STEPS, against the model's integers; the jobs over a decide job
    # of 2^31 - 1 symbols at offsets of 2^62, the word at its start and at its very end
    for order in dcm.ORDERS:
        for period, punct in (dcm.P_NONE, dcm.P_34, dcm.P_78, dcm.P_16, dcm.P3_NONE, dcm.P3_16, (16, (1, 0, 0)), (16, (0xffff, 0xffff, 0xffff))):
            masks = np.array(punct, np.uint16)
            n_poly = 3 if punct[2] else 2
            for count in (0, 1, n - 1, n):
                assert L.fosphor_amd_decode_steps(count, order, n_poly, period, masks.ctypes.data) == fits(dcm.steps_that_fit(count, order, period, punct))
            for T in (dcm.MAX_STEPS, dcm.MAX_STEPS + 1):
                count = dcm.symbols_for(T, order, (period, punct))
                got = L.fosphor_amd_decode_steps(count, order, n_poly, period, masks.ctypes.data)
                assert got == dcm.steps_that_fit(count, order, period, punct) >= T
    from decide_model import GRAY, JOB_DTYPE as DECIDE_JOB, NO_UW, OK as DECIDE_OK, RECORD_DTYPE as DECIDE_RECORD, UW
    for flags in (0, UW, UW | GRAY):
        for order in (2, 4, 8):
            for uw_pos, uw_len, n_payload in ((0, 0, 0), (0, n, 0), (n - 32, 32, 0), (0, 32, n - 32), (n - 1, 1, 1), (n, 2 ** 31 - 1, 2 ** 31 - 1)):
                for status in (DECIDE_OK, NO_UW):
                    d, r = np.zeros(1, DECIDE_JOB), np.zeros(1, DECIDE_RECORD)
                    d["offset"], d["out_offset"], d["n"], d["flags"] = 2 ** 62, 2 ** 62, n, flags
                    r["n"], r["order"], r["status"], r["uw_pos"], r["uw_rot"], r["a"] = n, order, status, uw_pos, order - 1, 1e-30 * n
                    L.fosphor_amd_decode_from_decide(d.ctypes.data, r.ctypes.data, uw_len, n_payload, C.byref(L_.DecodeJob()))
                    L.fosphor_amd_soft_from_decide(d.ctypes.data, r.ctypes.data, uw_len, n_payload, C.byref(L_.SoftJob()))
    # a burst at the far end of a stream: newest_first_sample near 2^62, the largest row_hop an int holds, a ring of 65536 rows
    for hop in (1, 2 ** 31 - 1):
        for newest, oldest in ((0, 0), (0, 65535), (65535, 65535)):
            b = L_.Burst(newest=newest, oldest=oldest, first_col=0, last_col=65535, n_cells=1, peak_row=newest, peak_col=0)
            for nfs in (2 ** 62, 2 ** 62 - 1 + 2 ** 61, 2 ** 63 - 1, oldest * hop):
                for fft_len in (2, 65536, 2 ** 30):
                    L.fosphor_amd_extract_from_burst(C.byref(b), fft_len, nfs, hop, 2 ** 31 - 1, 1.0, C.byref(L_.ExtractJob()),
                                                     C.byref(C.c_int()))
    # the views at 65536 x 65536, at the grid's corners
    lo, hi = C.c_int(), C.c_int()
    for n_src, n_out in set(tv.GRID) | {(65536, 65536), (65536, 1), (1, 65536)}:
        for p in (0, n_out // 2, n_out - 1):
            L.fosphor_amd_view_span(n_src, n_out, p, C.byref(lo), C.byref(hi))
    for center, span, wf_span in tv.ZOOMS:
        r = tv.render(gr_fosphor_amd, center, span, wf_span)
        L.fosphor_amd_view_from_render(65536, 65536, C.byref(r), 65536, 65536, C.byref(L_.View()))
        L.fosphor_amd_view_from_render(65536, 65536, C.byref(r), 1, 1, C.byref(L_.View()))
    # the designs at their limits
    up, down, err = C.c_int(), C.c_int(), C.c_double()
    for rate_in, rate_out in ((1.0, 1.0), (1.0, 256.0), (256.0, 1.0), (1e-300, 1e300), (1e300, 1e-300), (48000.0, 44100.0),
                              (255.0, 256.0), (3.0, 1e9)):
        for max_term in (1, 2, 255, 256, 257, 2 ** 31 - 1):
            L.fosphor_amd_resample_ratio(rate_in, rate_out, max_term, C.byref(up), C.byref(down), C.byref(err))
    for u, d, bt in ((1, 1, 1), (rm.MAX_UP, 1, rm.MAX_BRANCH), (1, rm.MAX_DOWN, rm.MAX_BRANCH), (rm.MAX_UP, rm.MAX_DOWN, 1),
                     (rm.MAX_UP, 1, rm.MAX_BRANCH + 1)):
        out = np.zeros(max(u * bt, 1), np.float32)
        L.fosphor_amd_resample_design(u, d, bt, 1.0, out.ctypes.data)
    for decim, taps in ((1, 1), (1024, 8192), (1024, 1), (1, 8192), (1024, 8193)):
        out = np.zeros(taps, np.float32)
        L.fosphor_amd_extract_design(decim, taps, 1.0, out.ctypes.data)
    for kind in range(-1, 8):
        for log in pm.LOGS:
            out = np.zeros(1 << log, np.float32)
            L.fosphor_amd_psd_window(kind, log, out.ctypes.data)
    for sps in range(sm.MIN_SPS, sm.MAX_SPS + 1):
        out = np.zeros(2 * sps)
        L.fosphor_amd_symbols_twiddles(sps, out.ctypes.data)
    out = np.zeros(1024)
    L.fosphor_amd_psd_twiddles(out.ctypes.data)
    for which in range(-1, 6):
        for count in (1, 2, 256, 65536):
            out = np.zeros(count, np.uint32)
            L.fosphor_amd_cmap_generate(which, out.ctypes.data, count)
    for bins in (16, 512, 65536):
        out = np.zeros(bins + 1)
        L.fosphor_amd_host_thresholds(bins, bins / 10.0, 1.5, out.ctypes.data)
        outf = np.zeros(bins, np.float32)
        L.fosphor_amd_detect_bin_y(bins, bins / 10.0, 1.5, outf.ctypes.data)
    tw = np.zeros(2 * L.fosphor_amd_host_twiddle_count(), np.float32)
    L.fosphor_amd_host_twiddles(tw.ctypes.data)
    # the records as values: all-zero counts, and sums and counts at the ends of their types
    big = {"i": 2 ** 31 - 1, "u": 2 ** 32 - 1, "f": np.finfo(np.float32).max}
    for key, fn, extra in (("measure", L.fosphor_amd_measure_derive, (1e6,)), ("correlate", L.fosphor_amd_correlate_derive, (1e6,)),
                           ("psd", L.fosphor_amd_psd_derive, (1e6,)), ("symbols", L.fosphor_amd_symbols_derive, None),
                           ("carrier", L.fosphor_amd_carrier_derive, (1e6,)), ("decide", L.fosphor_amd_decide_derive, None),
                           ("decode", L.fosphor_amd_decode_derive, ()), ("soft", L.fosphor_amd_soft_derive, ())):
        dtype = getattr(F, key.upper() + "_RECORD_DTYPE")
        values = getattr(L_, key.capitalize() + "Values")
        zero, full, mixed = np.zeros(1, dtype), np.zeros(1, dtype), np.zeros(1, dtype)
        for field in dtype.names:
            kind = dtype[field].kind
            if dtype[field].shape:
                full[field] = big["i"]
                continue
            full[field] = np.finfo(np.float64).max if (kind == "f" and dtype[field].itemsize == 8) else big[kind]
            mixed[field] = (1e300 if dtype[field].itemsize == 8 else 1e30) if kind == "f" else 1
        for rec in (zero, full, mixed):
            v = values()
            if key == "symbols":
                for sps in (2, 64):
                    fn(rec.ctypes.data, sps, 1e6, C.byref(v))
            elif key == "decide":
                for uw_len in (0, 1, 2 ** 31 - 1):
                    fn(rec.ctypes.data, uw_len, C.byref(v))
            else:
                fn(rec.ctypes.data, *extra, C.byref(v))


@pytest.fixture(scope="session")
def recorded():
    real = L_.load()
    rec = Recorder(real)
    L_._lib = rec
    t0 = time.time()
    try:
        harvest(rec)
        rec.origin = "extremes()"
        extremes(rec, gr_fosphor_amd.Fosphor)
    finally:
        L_._lib = real
    print("host_sanitized: %d calls recorded in %.1f s (%d about alignment left out, %d claims above MAX_BYTES)"
          % (len(rec.calls), time.time() - t0, rec.misaligned, rec.oversize))
    return rec


def groups_of(calls):
    by = {}
    for c in calls:
        by.setdefault(c.name, []).append(c)
    return by


def test_every_entry_point_has_cases(recorded):
    """the harvest reaches every entry point of the contract table; prints the number of cases of each"""
    by = groups_of(recorded.calls)
    for name in sorted(CONTRACT):
        print("%6d  %s" % (len(by.get(name, [])), name))
    missing = [n for n in CONTRACT if n not in by]
    assert not missing, missing
    hosts = [n for n in CONTRACT if n.endswith("_host")]
    assert len(hosts) == 14
    # every host statement with accepted calls and with refusals: a harvest that lost a module's refusal table, or a whole module
    # (pytest's fixture and parametrize attributes are read here as they are today), does not pass for complete
    for n in hosts:
        refused = sum(1 for c in by[n] if c.plain_rv != 0)
        assert refused >= MIN_REFUSED and len(by[n]) - refused >= MIN_ACCEPTED, (n, refused, len(by[n]))
    idle = [m for m in HARVEST if not recorded.ran.get(m)]
    assert not idle, "no test function of %s ran in the harvest" % idle


def test_the_program_starts_without_a_gpu(driver):
    """the child's environment hides every device; the program still starts, runs a case and ends"""
    env = child_env()
    assert env["HIP_VISIBLE_DEVICES"] == "" and env["ROCR_VISIBLE_DEVICES"] == "" and "LD_PRELOAD" not in env
    got = run_driver(driver, [Call("fosphor_amd_version", [], "version")], "start")
    assert got[0][0] == len(L_.load().fosphor_amd_version())


@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_sanitized_against_plain(driver, recorded, name):
    """the entry point's cases in one child process under ASan and UBSan: no report, and return value, records, outputs and the
    untouched fills byte for byte what the plain library gives; a refused call leaves every buffer as it was"""
    calls = groups_of(recorded.calls).get(name, [])
    assert calls, "no case"
    # identical calls (the suite repeats some) run once
    seen, unique = set(), []
    for c in calls:
        key = repr([(a[0], a[1]) if a[0] != "null" else a for a in c.args])
        if key not in seen:
            seen.add(key)
            unique.append(c)
    got = run_driver(driver, unique, name)
    refusals = 0
    for c, (bits, bufs) in zip(unique, got):
        want_bits, want_bufs = replay_plain(c)
        assert bits == want_bits, "%s from %s: returns %#x, the plain library %#x" % (name, c.origin, bits, want_bits)
        before = [a[1] for a in c.args if a[0] == "buf"]
        for i, (g, w, b) in enumerate(zip(bufs, want_bufs, before)):
            if g != w:
                at = next(k for k in range(len(g)) if g[k] != w[k])
                raise AssertionError("%s from %s: buffer %d differs from the plain library's at byte %d of %d: %s / %s"
                                     % (name, c.origin, i, at, len(g), g[at:at + 16].hex(), w[at:at + 16].hex()))
        res = L_.SIGNATURES[name][0]
        if getattr(c, "must_refuse", False):
            assert bits != 0, c.origin
        if res is C.c_int and name not in ("fosphor_amd_host_twiddle_count",) and bits >> 63 and (bits - (1 << 64)) == -22:
            refusals += 1
            inputs_and_outputs = [(g, b) for g, b in zip(bufs, before)]
            if name.endswith("_host") or name.endswith("_derive") or "_from_" in name or "_design" in name:
                for g, b in inputs_and_outputs:
                    assert g == b, "%s from %s: a refused call wrote into a buffer" % (name, c.origin)
    print("%s: %d cases (%d of them refusals), %d calls recorded" % (name, len(unique), refusals, len(calls)))
