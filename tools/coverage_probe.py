#!/usr/bin/env python3
"""tools/coverage_probe.py -- GPU box: covered base pairs of many query sets in one call (Database.coverage_sets) beside the
support counts and the pair counts of the same sets (Database.support_sets, Database.search_sets: the yardsticks) and beside
the only route to the same answer without igd_sets_coverage: Database.enumerate plus an interval union per (query, file) in
numpy, per set.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Set k = synth.make_queries(n,
seed=1000 + k).  One JSON line per case (K sets x n queries):
  coverage_ms   coverage_sets wall time, median of --reps calls after one warm-up call
  support_ms    support_sets wall time on the same input, the same way
  sets_ms       search_sets wall time on the same input, the same way
  enum_ms       enumerate + clip + sort + sweep per (query, file), wall time (--enum-reps runs, median)
  enum_equal    the coverage matrix and covered[] made from the enumeration equal coverage_sets exactly
  same_support  coverage > 0 exactly where support > 0
  ordered_share (a build with -DIGD_COVERAGE_PROBE only) iterations with a hit that took the ordered path / all of them
The kernel's own time (igd_sets_coverage) comes from a run of one case under `rocprofv3 --kernel-trace --stats`
(profiles/coverage/): this tool prints host wall times only.
Usage: tools/coverage_probe.py [--case K,n ...] [--no-enum] [--out profiles/coverage/probe.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from igd_amd import Database, synth  # noqa: E402
from igd_amd import _native as N  # noqa: E402

CASES = [(1000, 1000), (100, 10000), (1, 1000000)]


def med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def union_by_group(g, lo, hi, ngroups):
    """per group the length of the union of its intervals [lo, hi): sort by (group, lo), running maximum of hi, sweep"""
    out = np.zeros(ngroups, np.int64)
    if len(g) == 0:
        return out
    o = np.lexsort((lo, g))
    g, lo, hi = g[o], lo[o], hi[o]
    first = np.ones(len(g), bool)
    first[1:] = g[1:] != g[:-1]
    rank = np.cumsum(first) - 1                               # dense group numbers keep the offsets below 2^63
    big = np.int64(1) << 34
    run = np.maximum.accumulate(hi + rank * big)
    prev = np.empty_like(run)
    prev[0] = 0
    prev[1:] = run[:-1]
    prev = np.where(first, lo, prev - rank * big)
    np.add.at(out, g, np.maximum(0, hi - np.maximum(lo, prev)))
    return out


def coverage_from_enumeration(db, ichr, qs, qe, K, n):
    """the route without the coverage kernel: every overlap to the host, clipped to its query, united per (query, file)"""
    nF = db.nfiles
    _, rec = db.enumerate(ichr, qs, qe)
    q = rec[:, 0].astype(np.int64)
    lo = np.maximum(rec[:, 2], qs[q]).astype(np.int64)
    hi = np.minimum(rec[:, 3], qe[q]).astype(np.int64)
    per = union_by_group(q * nF + rec[:, 1], lo, hi, K * n * nF) if K * n * nF <= (1 << 31) else None
    if per is None:                                           # (a set at a time: the per-(query, file) table of all sets is too large)
        cov = np.zeros((K, nF), np.int64)
        cut = np.searchsorted(q, np.arange(K + 1, dtype=np.int64) * n)
        for k in range(K):
            a, b = cut[k], cut[k + 1]
            cov[k] = union_by_group((q[a:b] - k * n) * nF + rec[a:b, 1], lo[a:b], hi[a:b], n * nF).reshape(n, nF).sum(axis=0)
    else:
        cov = per.reshape(K, n, nF).sum(axis=1)
    covered = union_by_group(q, lo, hi, K * n).reshape(K, n).sum(axis=1)
    return cov, covered


def ordered_share():
    """iterations with a hit and those of them on the ordered path since the last call, or None (the shipped build)"""
    H = N.hip()
    if not hasattr(H, "igd_hip_coverage_probe"):
        return None
    out = (C.c_ulonglong * 2)()
    H.igd_hip_coverage_probe(out)
    return int(out[0]), int(out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/igdb")
    ap.add_argument("--case", action="append", help="K,n (default: the three cases of DESIGN 4.6)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--enum-reps", type=int, default=3)
    ap.add_argument("--no-enum", action="store_true", help="skip the enumeration route (profiling runs)")
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
        ordered_share()
        cov, covered = db.coverage_sets(ichr, qs, qe, off)          # warm-up (workspaces)
        share = ordered_share()
        sup, nhit = db.support_sets(ichr, qs, qe, off)
        hits, totals = db.search_sets(ichr, qs, qe, off)
        coverage_ms = med(lambda: db.coverage_sets(ichr, qs, qe, off), a.reps)
        support_ms = med(lambda: db.support_sets(ichr, qs, qe, off), a.reps)
        sets_ms = med(lambda: db.search_sets(ichr, qs, qe, off), a.reps)
        line = dict(case="%d x %d" % (K, n), sets=K, queries_per_set=n, coverage_ms=round(coverage_ms, 3),
                    support_ms=round(support_ms, 3), sets_ms=round(sets_ms, 3), coverage_over_support=round(coverage_ms / support_ms, 3),
                    overlaps=int(totals.sum()), coverage_sum=int(cov.sum()), covered=int(covered.sum()),
                    query_bp=int((qe.astype(np.int64) - qs)[qe > qs].sum()), same_support=bool(np.array_equal(cov > 0, sup > 0)))
        if share is not None:
            line.update(steps_with_hit=share[0], steps_ordered=share[1], ordered_share=round(share[1] / max(share[0], 1), 5))
        if not a.no_enum:
            e_cov, e_covered = coverage_from_enumeration(db, ichr, qs, qe, K, n)
            enum_ms = med(lambda: coverage_from_enumeration(db, ichr, qs, qe, K, n), a.enum_reps)
            line.update(enum_ms=round(enum_ms, 1), enum_reps=a.enum_reps, enum_over_coverage=round(enum_ms / coverage_ms, 1),
                        enum_equal=bool(np.array_equal(e_cov, cov) and np.array_equal(e_covered, covered)))
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
