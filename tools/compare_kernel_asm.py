#!/usr/bin/env python3
"""Compare the device code of two `hipcc -S` listings kernel by kernel, apart from labels and metadata.

    hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -x hip --cuda-device-only -S -o old.s fosphor_kernels.hip   # (old tree)
    hipcc ... -o new.s fosphor_kernels.hip                                                                                    # (new tree)
    python3 tools/compare_kernel_asm.py old.s new.s

Every function of OLD is looked up in NEW by its mangled name; its instructions are compared after the basic-block labels are
renumbered in order of appearance and comments / assembler directives are dropped.  The register counts, LDS and scratch sizes the
compiler reports in the comment block behind each function are compared as well.  One line per function; exit status 1 if any function
of OLD is missing from NEW or differs.  Functions that exist only in NEW (new entry points) are listed, not compared.

    python3 tools/compare_kernel_asm.py --vector old.s new.s

compares less, for a change that only moves kernel arguments: per function the resources, and the multiset of vector instructions
(v_, ds_, global_, buffer_, flat_ lines) with scalar register numbers masked.  Argument offsets, scalar registers and the order of
the instructions may differ.

    python3 tools/compare_kernel_asm.py --rename 'PATTERN=REPLACEMENT' [--rename ...] old.s new.s

follows functions that were renamed on purpose: each PATTERN (a Python regular expression, the renames applied in the order given) is
replaced in the DEMANGLED name of every function of OLD (llvm-cxxfilt of the ROCm toolchain, or c++filt), and the result is looked up
among the demangled names of NEW."""
import collections
import os
import re
import shutil
import subprocess
import sys


def functions(path):
    lines = open(path).read().splitlines()
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_.$][\w.$]*):\s*(;.*)?$", lines[i])
        if m and not m.group(1).startswith(".") and i + 1 < len(lines):
            end = next((j for j in range(i + 1, len(lines)) if lines[j].startswith(".Lfunc_end")), None)
            if end is not None:
                name = m.group(1)
                # the resource summary (NumVgprs, ScratchSize, ...) follows the function's end, before the next function
                tail = next((j for j in range(end + 1, min(end + 200, len(lines))) if re.match(r"^\s*\.globl\s", lines[j])), end + 200)
                out[name] = (lines[i + 1:end], lines[end:tail])
                i = end
                continue
        i += 1
    return out


def normalise(body):
    labels, code = {}, []
    for l in body:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels.setdefault(m.group(1), "L%d" % len(labels))
    for l in body:
        t = l.split(";")[0].rstrip()
        if not t.strip() or t.strip().startswith("."):
            m = re.match(r"^(\.LBB\d+_\d+):", t)
            if m:
                code.append(labels[m.group(1)] + ":")
            continue
        code.append(re.sub(r"\.LBB\d+_\d+", lambda mm: labels.get(mm.group(0), mm.group(0)), t.strip()))
    return code


def resources(tail):
    keys = ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")
    res = {}
    for l in tail:
        for k in keys:
            m = re.search(r";\s*%s:\s*(\d+)" % k, l)
            if m:
                res[k] = int(m.group(1))
    return res


def vector_multiset(code):
    return collections.Counter(re.sub(r"\bs(\d+|\[\d+:\d+\])", "s#", l) for l in code
                               if re.match(r"(v_|ds_|global_|buffer_|flat_)", l))


def demangle(names):
    tool = next((t for t in (shutil.which("llvm-cxxfilt"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-cxxfilt"),
                             shutil.which("c++filt")) if t and os.path.exists(t)), None)
    if tool is None:
        raise SystemExit("--rename needs llvm-cxxfilt or c++filt")
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def main(old_path, new_path, vector=False, renames=()):
    old, new = functions(old_path), functions(new_path)
    # OLD's name -> the name it has in NEW
    target = {name: name for name in old}
    if renames:
        dem_old, by_dem = demangle(list(old)), {d: n for n, d in demangle(list(new)).items()}
        for name in old:
            d = dem_old[name]
            for pat, repl in renames:
                d = re.sub(pat, repl, d)
            target[name] = by_dem.get(d, name if d == dem_old[name] else d)
    bad = 0
    for name in old:
        if target[name] not in new:
            print("MISSING  %s" % (name if target[name] == name else "%s (as %s)" % (name, target[name])))
            bad += 1
            continue
        a, b = normalise(old[name][0]), normalise(new[target[name]][0])
        ra, rb = resources(old[name][1]), resources(new[target[name]][1])
        if target[name] != name:
            name = "%s -> %s" % (name, target[name])
        if vector:
            a, b = vector_multiset(a), vector_multiset(b)
        if a == b and ra == rb:
            print("same     %s (%d %sinstructions)" % (name, sum(1 for l in a if not l.endswith(":")) if not vector else sum(a.values()),
                                                     "vector " if vector else ""))
        else:
            bad += 1
            print("DIFFERS  %s (%d vs %d lines; resources %s vs %s)" % (name, len(a), len(b), ra, rb))
    for name in new:
        if name not in target.values():
            print("new      %s %s" % (name, resources(new[name][1])))
    print("%d of %d functions of %s identical in %s" % (len(old) - bad, len(old), old_path, new_path))
    return 1 if bad else 0


if __name__ == "__main__":
    args, renames = [a for a in sys.argv[1:] if a != "--vector"], []
    while "--rename" in args:
        i = args.index("--rename")
        if i + 1 >= len(args) or "=" not in args[i + 1]:
            raise SystemExit(__doc__)
        renames.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    if len(args) != 2:
        raise SystemExit(__doc__)
    sys.exit(main(args[0], args[1], vector="--vector" in sys.argv, renames=renames))
