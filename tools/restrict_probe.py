#!/usr/bin/env python3
"""tools/restrict_probe.py -- GPU box: enrichment of query sets restricted to a universe (Database.enrichment_restricted), its
stages timed apart, beside the only other route: an interval join in numpy, explicit region lists, then enrichment_sets.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Set k = synth.make_queries(n,
seed=1000 + k); the universe = synth.make_queries(--universe, seed=999), in the generator's order (not sorted).  One JSON
line per case (K sets x n regions):
  restricted_ms   enrichment_restricted wall time, median of --reps calls (the host sort of the universe included)
  join_ms         restrict_sets alone (sort, upload, igd_restrict_bits, popcounts, rows back to the host)
  sort_ms         join_ms minus restrict_sets on the same universe given sorted: the host sort's cost; sort_share of restricted_ms
  membership_ms   membership of the universe alone (it copies the rows to the host, which the call itself does not: upper bound)
  gather_ms       restricted_ms - join_ms - membership_ms - fisher_ms: what is left for igd_bits_support and its copies
  fisher_ms       Database.fisher on the K x nfiles tables (generic form: an upper bound of the stage inside the call)
  numpy_join_ms   the numpy join (sort, prefix maximum, two searchsorted, candidates filtered) and the explicit lists
  sets_ms         enrichment_sets on the explicit lists
  equal           the two routes agree: supports, tables, clamped == 0, statistics bit for bit
Registers and occupancy: tools/regs.sh (profiles/enrich/regs_restrict.txt).
Usage: tools/restrict_probe.py [--case K,n ...] [--universe 1000000] [--out profiles/enrich/restrict_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from igd_amd import Database, synth  # noqa: E402

CASES = [(1000, 1000)]


def med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def numpy_join(ichr, qs, qe, off, uc, us, ue):
    """explicit lists of R_k: ((ichr, qs, qe), off), the universe's triples in universe order"""
    order = np.lexsort((us, uc))
    order = order[uc[order] >= 0]
    sc, ss, se = uc[order], us[order], ue[order]
    key = sc.astype(np.int64) << 32
    pm = np.empty(len(se), np.int64)                                       # prefix maximum of the ends, per contig
    bounds = np.flatnonzero(np.diff(sc, prepend=-1, append=-2))
    for a, b in zip(bounds[:-1], bounds[1:]):
        pm[a:b] = np.maximum.accumulate(se[a:b])
    skey, pkey = key + ss.astype(np.int64) + (1 << 31), key + pm + (1 << 31)
    qkey = ichr.astype(np.int64) << 32
    hi = np.searchsorted(skey, qkey + qe.astype(np.int64) + (1 << 31), "left")
    lo = np.searchsorted(pkey, qkey + qs.astype(np.int64) + (1 << 31), "right")
    n = np.where(ichr >= 0, np.maximum(hi - lo, 0), 0)
    qi = np.repeat(np.arange(len(qs)), n)
    pos = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(lo, n)
    ok = se[pos] > qs[qi]
    setno = np.searchsorted(off, qi[ok], "right") - 1
    pairs = np.unique(setno.astype(np.int64) * len(us) + order[pos[ok]])
    k, u = pairs // len(us), pairs % len(us)
    xoff = np.searchsorted(k, np.arange(len(off)), "left").astype(np.int64)
    return (uc[u], us[u], ue[u]), xoff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/igdb")
    ap.add_argument("--case", action="append", help="K,n (default: 1000 sets x 1000 regions)")
    ap.add_argument("--universe", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    cases = [tuple(int(x) for x in c.split(",")) for c in a.case] if a.case else CASES
    u = tuple(np.ascontiguousarray(x, np.int32) for x in synth.make_queries(a.universe, seed=999))
    srt = np.lexsort((u[1], u[0]))
    us = tuple(x[srt] for x in u)
    for K, n in cases:
        sets = [synth.make_queries(n, seed=1000 + k) for k in range(K)]
        ichr, qs, qe = (np.concatenate([s[i] for s in sets]).astype(np.int32) for i in range(3))
        off = np.arange(K + 1, dtype=np.int64) * n
        res = db.enrichment_restricted(ichr, qs, qe, off, *u)               # warm-up (workspaces)
        tabs = [np.ascontiguousarray(x.ravel()) for x in (res.support, res.b, res.c, res.d)]
        restricted_ms = med(lambda: db.enrichment_restricted(ichr, qs, qe, off, *u), a.reps)
        join_ms = med(lambda: db.restrict_sets(ichr, qs, qe, off, *u), a.reps)
        join_sorted_ms = med(lambda: db.restrict_sets(ichr, qs, qe, off, *us), a.reps)
        membership_ms = med(lambda: db.membership(*u), a.reps)
        fisher_ms = med(lambda: db.fisher(*tabs), a.reps)
        t0 = time.perf_counter()
        xcat, xoff = numpy_join(ichr, qs, qe, off, *u)
        numpy_join_ms = 1e3 * (time.perf_counter() - t0)
        ex = db.enrichment_sets(*xcat, xoff, *u)
        sets_ms = med(lambda: db.enrichment_sets(*xcat, xoff, *u), a.reps)
        equal = bool(np.array_equal(ex.support, res.support) and np.array_equal(ex.usupport, res.usupport) and
                     np.array_equal(ex.b, res.b) and np.array_equal(ex.c, res.c) and np.array_equal(ex.d, res.d) and
                     not ex.clamped.any() and np.array_equal(np.diff(xoff), res.size) and
                     np.array_equal(ex.pvalue_log.view(np.int64), res.pvalue_log.view(np.int64)) and
                     np.array_equal(ex.odds_ratio.view(np.int64), res.odds_ratio.view(np.int64)))
        sort_ms = join_ms - join_sorted_ms
        line = dict(case="%d x %d" % (K, n), sets=K, regions_per_set=n, universe=int(a.universe), cells=int(len(tabs[0])),
                    restricted_ms=round(restricted_ms, 3), join_ms=round(join_ms, 3), sort_ms=round(sort_ms, 3),
                    sort_share=round(sort_ms / restricted_ms, 3), membership_ms=round(membership_ms, 3),
                    fisher_ms=round(fisher_ms, 3), gather_ms=round(restricted_ms - join_ms - membership_ms - fisher_ms, 3),
                    numpy_join_ms=round(numpy_join_ms, 1), sets_ms=round(sets_ms, 3),
                    other_over_restricted=round((numpy_join_ms + sets_ms) / restricted_ms, 2), equal=equal,
                    mean_size=float(res.size.mean()), rows_with_support=int((res.support > 0).sum()),
                    max_pvalue_log=float(res.pvalue_log.max()))
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
