#!/usr/bin/env python3
"""tools/support_probe.py -- GPU box: support counts of many query sets in one call (Database.support_sets) beside the pair
counts of the same sets (Database.search_sets) and beside the only route to the same answer without igd_sets_support:
Database.enumerate plus numpy.unique over (query, idx), per set.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Set k = synth.make_queries(n,
seed=1000 + k).  One JSON line per case (K sets x n queries):
  support_ms    support_sets wall time, median of --reps calls after one warm-up call
  sets_ms       search_sets wall time on the same input, median of --reps calls after one warm-up call
  enum_ms       enumerate + numpy.unique + bincount, wall time (--enum-reps runs, median; 1 = a single run)
  enum_equal    the support matrix and nhit made from the enumeration equal support_sets exactly
  below         entries of the support matrix that are smaller than the pair count of search_sets
The kernel's own time (igd_sets_support) comes from a run of one case under `rocprofv3 --kernel-trace --stats`
(profiles/support/): this tool prints host wall times only.
Usage: tools/support_probe.py [--case K,n ...] [--no-enum] [--out profiles/support/probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from igd_amd import Database, synth  # noqa: E402

CASES = [(1000, 1000), (100, 10000), (1, 1000000)]


def med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def support_from_enumeration(db, ichr, qs, qe, K, n):
    """the route without the support kernel: every overlap to the host, distinct (query, idx) pairs, counted per set"""
    nF = db.nfiles
    _, rec = db.enumerate(ichr, qs, qe)
    pairs = np.unique(rec[:, 0].astype(np.int64) * nF + rec[:, 1])
    q, f = pairs // nF, pairs % nF
    sup = np.bincount((q // n) * nF + f, minlength=K * nF).reshape(K, nF)
    nhit = np.bincount(np.unique(q) // n, minlength=K)
    return sup, nhit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/igdb")
    ap.add_argument("--case", action="append", help="K,n (default: the three cases of DESIGN 4.5)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--enum-reps", type=int, default=1)
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
        sup, nhit = db.support_sets(ichr, qs, qe, off)             # warm-up (workspaces)
        hits, totals = db.search_sets(ichr, qs, qe, off)
        support_ms = med(lambda: db.support_sets(ichr, qs, qe, off), a.reps)
        sets_ms = med(lambda: db.search_sets(ichr, qs, qe, off), a.reps)
        line = dict(case="%d x %d" % (K, n), sets=K, queries_per_set=n, support_ms=round(support_ms, 3), sets_ms=round(sets_ms, 3),
                    support_over_sets=round(support_ms / sets_ms, 3), overlaps=int(totals.sum()), support_sum=int(sup.sum()),
                    nhit=int(nhit.sum()), le_hits=bool((sup <= hits).all()), below=int((sup < hits).sum()))
        if not a.no_enum:
            e_sup, e_nhit = support_from_enumeration(db, ichr, qs, qe, K, n)
            enum_ms = med(lambda: support_from_enumeration(db, ichr, qs, qe, K, n), a.enum_reps)
            line.update(enum_ms=round(enum_ms, 1), enum_reps=a.enum_reps, enum_over_support=round(enum_ms / support_ms, 1),
                        enum_equal=bool(np.array_equal(e_sup, sup) and np.array_equal(e_nhit, nhit)))
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
