#!/usr/bin/env python3
"""Summary of a rocprofv3 --memory-copy-trace CSV of bench.py (config 2, wire
packing): per step, how long the link carried no H2D copy between the step's
first and last copy, in how many gaps, and the first copies' start and
duration (the trace has no sizes: a raw 64 MiB strip takes 1.18 ms alone, a
packed one about 0.9; two copies on two streams run at the same time, each
about twice as long).

  python tools/copy_trace_summary.py TRACE.csv [--steps 3] [--first 40]
"""
import argparse
import csv
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--steps", type=int, default=3, help="the last N steps of the trace are summarised")
    ap.add_argument("--step-gap-us", type=float, default=1000.0, help="idle time that separates two steps")
    ap.add_argument("--first", type=int, default=40, help="list this many first copies of each step")
    a = ap.parse_args()
    rows = []
    with open(a.csv) as f:
        for r in csv.DictReader(f):
            if r["Direction"] == "MEMORY_COPY_HOST_TO_DEVICE":
                rows.append((int(r["Start_Timestamp"]) / 1e3, int(r["End_Timestamp"]) / 1e3, r["Stream_Id"]))
    rows.sort()
    steps, cur, end = [], [], 0.0
    for r in rows:
        if cur and r[0] - end > a.step_gap_us:
            steps.append(cur)
            cur = []
        end = max(end, r[1]) if cur else r[1]
        cur.append(r)
    if cur:
        steps.append(cur)
    out = []
    for s in [x for x in steps if len(x) >= 20][-a.steps:]:
        t0, end, gaps = s[0][0], s[0][1], []
        for b, e, _ in s[1:]:
            if b > end:
                gaps.append(b - end)
            end = max(end, e)
        out.append({
            "copies": len(s), "streams": len({st for _, _, st in s}),
            "first_to_last_copy_ms": round((end - t0) / 1e3, 3),
            "link_idle_ms": round(sum(gaps) / 1e3, 3), "gaps": len(gaps),
            "gap_median_us": round(statistics.median(gaps), 2) if gaps else None,
            "gap_max_us": round(max(gaps), 1) if gaps else None,
            "first_copies_start_ms_duration_us": [[round((b - t0) / 1e3, 3), round(e - b, 1)] for b, e, _ in s[:a.first]],
        })
    print(json.dumps(out))


if __name__ == "__main__":
    main()
