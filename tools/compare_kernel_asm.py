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
the instructions may differ."""
import collections
import re
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


def main(old_path, new_path, vector=False):
    old, new = functions(old_path), functions(new_path)
    bad = 0
    for name in old:
        if name not in new:
            print("MISSING  %s" % name)
            bad += 1
            continue
        a, b = normalise(old[name][0]), normalise(new[name][0])
        ra, rb = resources(old[name][1]), resources(new[name][1])
        if vector:
            a, b = vector_multiset(a), vector_multiset(b)
        if a == b and ra == rb:
            print("same     %s (%d %sinstructions)" % (name, sum(1 for l in a if not l.endswith(":")) if not vector else sum(a.values()),
                                                     "vector " if vector else ""))
        else:
            bad += 1
            print("DIFFERS  %s (%d vs %d lines; resources %s vs %s)" % (name, len(a), len(b), ra, rb))
    for name in new:
        if name not in old:
            print("new      %s %s" % (name, resources(new[name][1])))
    print("%d of %d functions of %s identical in %s" % (len(old) - bad, len(old), old_path, new_path))
    return 1 if bad else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--vector"]
    if len(args) != 2:
        raise SystemExit(__doc__)
    sys.exit(main(args[0], args[1], vector="--vector" in sys.argv))
