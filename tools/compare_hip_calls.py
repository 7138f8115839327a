#!/usr/bin/env python3
"""Compare the HIP runtime calls of two traced runs of tools/hip_call_driver.py (rocprofv3 --hip-trace -f csv json -d DIR):

    python3 tools/compare_hip_calls.py PARENT_DIR BRANCH_DIR

Per thread (threads matched in order of their first call) the calls are put in time order and cut at the driver's marks
(hipMemGetInfo): mark, fosphor_amd_init, mark, the entry points, mark, fosphor_release, mark, once per instance.  Between the
marks around the entry points the two runs must make the same calls in the same order, on the same streams where the trace
carries the arguments (the JSON output; stream handles are numbered in order of first appearance, so that two runs compare);
inside fosphor_amd_init and fosphor_release the branch must not create or destroy more streams or events than the parent.
Calls whose names start with "__hip" (compiler-generated: kernel argument set-up) are left out.  Exit status 1 on a difference."""
import collections
import csv
import glob
import json
import os
import re
import sys

MARK = "hipMemGetInfo"
LIFETIME = ("hipStreamCreate", "hipStreamCreateWithFlags", "hipStreamCreateWithPriority", "hipStreamDestroy",
            "hipEventCreate", "hipEventCreateWithFlags", "hipEventDestroy")


def find(d, pattern):
    hits = sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True))
    return hits[0] if hits else None


def calls_from_json(path):
    """[(thread, start, name, stream or None)] from the tool's JSON, or None when it carries no HIP records"""
    top = json.load(open(path))["rocprofiler-sdk-tool"]
    top = top[0] if isinstance(top, list) else top
    names = {}
    for ent in top.get("strings", {}).get("buffer_records", []):
        if "HIP" in str(ent.get("kind", "")):
            names[ent["kind"]] = ent["operations"]
    kinds = top.get("strings", {}).get("buffer_records", [])
    by_index = {i: ent for i, ent in enumerate(kinds)}
    out = []
    for r in top.get("buffer_records", {}).get("hip_api", []):
        kind = r.get("kind")
        ops = names.get(kind) if kind in names else (by_index.get(kind, {}).get("operations") if isinstance(kind, int) else None)
        name = ops[r["operation"]] if ops else str(r.get("operation"))
        stream = None
        for a in r.get("args", []) or []:
            if a.get("name") in ("stream", "hStream"):
                stream = a.get("value")
        out.append((r["thread_id"], r["start_timestamp"], name, stream))
    return out or None


def calls_from_csv(path):
    out = []
    for row in csv.DictReader(open(path)):
        out.append((int(row["Thread_Id"]), int(row["Start_Timestamp"]), row["Function"], None))
    return out


def load(d):
    js, cs = find(d, "*results.json"), find(d, "*hip_api_trace.csv")
    try:
        calls = calls_from_json(js) if js else None
    except (KeyError, IndexError, TypeError, ValueError) as e:
        print("%s: not read (%s: %s); using the CSV" % (js, type(e).__name__, e))
        calls = None
    if calls is None:
        if not cs:
            raise SystemExit("%s: no HIP trace found" % d)
        calls = calls_from_csv(cs)
    threads = collections.OrderedDict()
    for t, ts, name, stream in sorted(calls, key=lambda c: c[1]):
        if not name.startswith("__hip"):
            threads.setdefault(t, []).append((name, stream))
    return list(threads.values())


def segments(seq):
    """the thread's calls cut at the marks: [before, init, region, release, between, init, region, release, ...]"""
    segs, cur = [], []
    for c in seq:
        if c[0] == MARK:
            segs.append(cur)
            cur = []
        else:
            cur.append(c)
    segs.append(cur)
    return segs


def numbered(seg):
    """stream handles -> s0, s1, ... in order of first appearance in the segment"""
    ids, out = {}, []
    for name, stream in seg:
        if stream is not None and not re.fullmatch(r"(0x)?0+|nullptr|null", str(stream)):
            stream = "s%d" % ids.setdefault(stream, len(ids))
        out.append((name, stream))
    return out


def main(a_dir, b_dir):
    a, b = load(a_dir), load(b_dir)
    bad = 0
    with_streams = any(s is not None for seq in a for _, s in seq)
    print("threads with HIP calls: %d and %d; stream arguments %s" % (len(a), len(b), "compared" if with_streams else "NOT in the trace: names only"))
    if len(a) != len(b):
        bad += 1
    for t, (sa, sb) in enumerate(zip(a, b)):
        ga, gb = segments(sa), segments(sb)
        if len(ga) != len(gb):
            print("thread %d: %d and %d marks" % (t, len(ga) - 1, len(gb) - 1))
            bad += 1
            continue
        if len(ga) == 1:
            same = numbered(ga[0]) == numbered(gb[0])
            print("thread %d (no marks): %d and %d calls, %s" % (t, len(ga[0]), len(gb[0]), "same" if same else "DIFFERENT"))
            bad += 0 if same else 1
            continue
        for i in range(1, len(ga) - 1, 4):
            inst = i // 4
            for what, k in (("fosphor_amd_init", i), ("fosphor_release", i + 2)):
                ca = collections.Counter(n for n, _ in ga[k] if n in LIFETIME)
                cb = collections.Counter(n for n, _ in gb[k] if n in LIFETIME)
                grew = {n: (ca[n], cb[n]) for n in cb if cb[n] > ca[n]}
                print("thread %d instance %d %s: %s -> %s%s" % (t, inst, what, dict(ca), dict(cb), "  GREW" if grew else ""))
                bad += 1 if grew else 0
            ra, rb = numbered(ga[i + 1]), numbered(gb[i + 1])
            if ra == rb:
                print("thread %d instance %d, between init and release: %d calls, same names%s in the same order"
                      % (t, inst, len(ra), " and streams" if with_streams else ""))
                print("    " + ", ".join("%s x%d" % kv for kv in sorted(collections.Counter(n for n, _ in ra).items())))
            else:
                bad += 1
                at = next((j for j, (x, y) in enumerate(zip(ra, rb)) if x != y), min(len(ra), len(rb)))
                print("thread %d instance %d: DIFFERENT at call %d of %d / %d: %s | %s" % (t, inst, at, len(ra), len(rb), ra[at - 2:at + 3], rb[at - 2:at + 3]))
    print("identical" if not bad else "%d differences" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
