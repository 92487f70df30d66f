#!/usr/bin/env python3
"""The SW rerank's dispatches in a rocprofv3 kernel trace: per rerank call (the last N of the run) each
dispatch's start and end relative to the call's first dispatch, its queue, and for every top-k / flagged
dispatch whether it starts inside the span of a scoring dispatch (the overlap DESIGN.md sec. 4.4 "Round 8" reads).
Usage: rerank_tail_trace.py <dir with *_kernel_trace.csv> [calls to print, default 1]"""
import csv
import glob
import os
import sys

d = sys.argv[1]
ncalls = int(sys.argv[2]) if len(sys.argv) > 2 else 1
f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
rows = []
for r in csv.DictReader(open(f)):
    n = r["Kernel_Name"]
    if "sw_score" in n or "sw_topk" in n:
        kind = "topk" if "sw_topk" in n else "flagged" if ("true>" in n.replace(" ", "") and "sw_score_kernel" in n) \
            else "score"
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, n[:40], r.get("Queue_Id", "?"),
                     r.get("Grid_Size_X", r.get("Grid_Size", "?"))))
rows.sort()
# a rerank call: dispatches closer than 20 ms to the previous one's end (the search between two calls takes > 80 ms
# at C5, > 5 ms at C3)
calls, cur = [], []
for x in rows:
    if cur and x[0] - max(e for _, e, *_ in cur) > 3_000_000:
        calls.append(cur)
        cur = []
    cur.append(x)
if cur:
    calls.append(cur)
print(f"{os.path.basename(f)}: {len(rows)} rerank dispatches in {len(calls)} calls")
for c in calls[-ncalls:]:
    t0 = c[0][0]
    score = [(s, e) for s, e, k, *_ in c if k == "score"]
    span = (max(e for _, e, *_ in c) - t0) / 1e6
    tot = {k: sum(e - s for s, e, kk, *_ in c if kk == k) / 1e6 for k in ("score", "flagged", "topk")}
    print(f"call: span {span:.3f} ms; summed score {tot['score']:.3f} flagged {tot['flagged']:.3f} topk {tot['topk']:.3f} ms; "
          f"last score end -> call end {(max(e for _, e, *_ in c) - max(e for _, e in score)) / 1e6 if score else 0:.3f} ms")
    for s, e, k, n, qid, g in c:
        inside = ""
        if k != "score":
            inside = " [starts inside a scoring dispatch]" if any(a < s < b for a, b in score) else " [exposed]"
        print(f"  {k:8s} q{qid} grid {g:>9s} start {(s - t0) / 1e6:9.3f} end {(e - t0) / 1e6:9.3f} dur {(e - s) / 1e6:8.3f}{inside}")
