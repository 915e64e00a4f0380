#!/usr/bin/env python3
"""tools/sets_probe.py -- GPU box: many query sets in one call (Database.search_sets) against the ways a user had before.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Set k = synth.make_queries(n,
seed=1000 + k).  One JSON line per case (K sets x n queries):
  sets_ms       search_sets wall time, median of --reps calls
  loop_ms       a Python loop of K Database.search calls, one per set (median of --loop-reps loops)
  concat_ms     one Database.search over the concatenation (the same overlaps, one row), median of --reps
  rows_equal    every row of search_sets equals the per-set search
The slice kernel's own time (igd_sets_count) comes from a run of one case under `rocprofv3 --kernel-trace --stats`
(profiles/sets/): this tool prints host wall times only.
Usage: tools/sets_probe.py [--case K,n ...] [--out profiles/sets/probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from igd_amd import Database, synth  # noqa: E402

CASES = [(1000, 1000), (10000, 100), (100, 10000), (1, 1000000)]


def med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/igdb")
    ap.add_argument("--case", action="append", help="K,n (default: the four cases of the issue)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    cases = [tuple(int(x) for x in c.split(",")) for c in a.case] if a.case else CASES
    for K, n in cases:
        sets = [synth.make_queries(n, seed=1000 + k) for k in range(K)]
        ichr, qs, qe = (np.concatenate([s[i] for s in sets]) for i in range(3))
        off = np.arange(K + 1, dtype=np.int64) * n
        hits, totals = db.search_sets(ichr, qs, qe, off)           # warm-up (workspaces)
        rows = [db.search(*s) for s in sets]
        rows_equal = all(np.array_equal(hits[k], rows[k][0]) and totals[k] == rows[k][1] for k in range(K))
        sets_ms = med(lambda: db.search_sets(ichr, qs, qe, off), a.reps)
        loop_ms = med(lambda: [db.search(*s) for s in sets], a.loop_reps)
        db.search(ichr, qs, qe)
        concat_ms = med(lambda: db.search(ichr, qs, qe), a.reps)
        line = dict(case="%d x %d" % (K, n), sets=K, queries_per_set=n, sets_ms=round(sets_ms, 3), loop_ms=round(loop_ms, 3),
                    concat_ms=round(concat_ms, 3), loop_over_sets=round(loop_ms / sets_ms, 2),
                    sets_over_concat=round(sets_ms / concat_ms, 3), overlaps=int(totals.sum()), rows_equal=bool(rows_equal),
                    big_min=os.environ.get("IGD_SETS_BIG_MIN", "default"))
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
