#!/usr/bin/env python3
"""tools/nearest_hist_probe.py -- GPU box: the histogram of the signed nearest distances per set and dataset
(Database.nearest_hist) beside Database.nearest_sets, the yardstick, in the same process.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Regions = synth.make_queries(
--sets x --regions, seed=999), cut into --sets sets; window --window.  One JSON line:
  nearest_sets_ms          Database.nearest_sets wall time, median of --reps calls
  nearest_signed_rows_ms   Database.nearest_signed over the first --row-regions regions, median of --reps (rows come back)
  nearest_rows_ms          Database.nearest over the same regions: what the sign costs in the row kernel
  cases                    per ne of --ne (1, 10, 63; edges spread over [-W, W]):
      nearest_hist_ms      Database.nearest_hist wall time, median of --reps calls (regions up, per chunk igd_nearest_rows
                           <., ., true> and igd_nearest_hist, sets x (ne + 1) x (nfiles + 1) words back)
      ratio                nearest_hist_ms / nearest_sets_ms
      sum_is_n_within      hist.sum(axis=1) == nearest_sets().n_within
      equal_host           the host result (igd_amd.nearest_hist_host, first --host-regions regions) equals the device's
  overlap_bin_is_n_overlap with edges (0, 1), bin 1 == nearest_sets().n_overlap
  abs_is_dist              abs(sdist) == dist where dist >= 0, sdist == NO_RECORD where dist == -1 (and sdmin, dmin)
No threshold: the first measurement of the stage.  Registers and occupancy: tools/regs.sh (profiles/enrich/regs_nearest_hist.txt).
Usage: tools/nearest_hist_probe.py [--sets 100] [--regions 10000] [--out profiles/enrich/nearest_hist_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import igd_amd  # noqa: E402
from igd_amd import Database, synth  # noqa: E402


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
    ap.add_argument("--sets", type=int, default=100)
    ap.add_argument("--regions", type=int, default=10000, help="regions per set")
    ap.add_argument("--window", type=int, default=10000)
    ap.add_argument("--ne", default="1,10,63")
    ap.add_argument("--host-regions", type=int, default=10000)
    ap.add_argument("--row-regions", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    nq, W = a.sets * a.regions, a.window
    ichr, qs, qe = (np.ascontiguousarray(x, np.int32) for x in synth.make_queries(nq, seed=999, sorted_=False))
    off = np.arange(a.sets + 1, dtype=np.int64) * a.regions
    nh = min(a.host_regions, nq)
    hoff = np.array([0, nh], np.int64)
    nr = min(a.row_regions, nq)
    ns = db.nearest_sets(ichr, qs, qe, off, W)                               # warm-up (workspaces)
    sets_ms = med(lambda: db.nearest_sets(ichr, qs, qe, off, W), a.reps)
    dist, dmin = db.nearest(ichr[:nr], qs[:nr], qe[:nr], W)
    sdist, sdmin = db.nearest_signed(ichr[:nr], qs[:nr], qe[:nr], W)
    rows_ms = med(lambda: db.nearest(ichr[:nr], qs[:nr], qe[:nr], W, dist=dist), a.reps)
    srows_ms = med(lambda: db.nearest_signed(ichr[:nr], qs[:nr], qe[:nr], W, sdist=sdist), a.reps)
    abs_ok = all(np.array_equal(s == igd_amd.NEAREST_NO_RECORD, d == -1) and np.array_equal(np.abs(s.astype(np.int64))[d >= 0], d[d >= 0])
                 for s, d in ((sdist, dist), (sdmin, dmin)))
    ov = db.nearest_hist(ichr, qs, qe, off, W, (0, 1))
    line = dict(sets=a.sets, regions_per_set=a.regions, nfiles=int(db.nfiles), window=W, host_regions=int(nh), row_regions=int(nr),
                nearest_sets_ms=round(sets_ms, 3), nearest_rows_ms=round(rows_ms, 3), nearest_signed_rows_ms=round(srows_ms, 3),
                abs_is_dist=bool(abs_ok), overlap_bin_is_n_overlap=bool(np.array_equal(ov.hist[:, 1], ns.n_overlap)),
                upstream_any=int(ov.hist[:, 0, -1].sum()), overlap_any=int(ov.hist[:, 1, -1].sum()), downstream_any=int(ov.hist[:, 2, -1].sum()),
                cases=[])
    equal = line["abs_is_dist"] and line["overlap_bin_is_n_overlap"]
    for ne in (int(x) for x in a.ne.split(",")):
        edges = np.unique(np.linspace(-W, W + 1, ne).astype(np.int64)) if ne > 1 else np.array([0])
        h = db.nearest_hist(ichr, qs, qe, off, W, edges)                     # warm-up (workspaces)
        hist_ms = med(lambda: db.nearest_hist(ichr, qs, qe, off, W, edges, hist=h.hist), a.reps)
        hh = igd_amd.nearest_hist_host(path, ichr[:nh], qs[:nh], qe[:nh], hoff, W, edges)
        dh = db.nearest_hist(ichr[:nh], qs[:nh], qe[:nh], hoff, W, edges)
        case = dict(ne=int(len(edges)), nearest_hist_ms=round(hist_ms, 3), ratio=round(hist_ms / sets_ms, 2),
                    sum_is_n_within=bool(np.array_equal(h.hist.sum(axis=1), ns.n_within)), equal_host=bool(np.array_equal(hh.hist, dh.hist)))
        equal = equal and case["sum_is_n_within"] and case["equal_host"]
        line["cases"].append(case)
    line["equal"] = bool(equal)
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
