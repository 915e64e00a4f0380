#!/usr/bin/env python3
"""tools/flank_probe.py -- GPU box: the flanking records per dataset (Database.flanks) and the relative-distance histogram per set
and dataset (Database.flank_reldist) beside their yardsticks, Database.nearest_signed and Database.nearest_hist with 10 edges, in
the same process.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Regions = synth.make_queries(
--sets x --regions, seed=999), cut into --sets sets; window --window; --bins bins.  One JSON line:
  nearest_hist_ms          Database.nearest_hist (10 edges spread over [-W, W]) wall time, median of --reps calls
  nearest_signed_rows_ms   Database.nearest_signed over the first --row-regions regions, median of --reps (rows come back)
  cases                    per measure (edges, midpoints):
      flank_reldist_ms     Database.flank_reldist wall time, median of --reps calls (regions up, per chunk igd_flank_rows and
                           igd_flank_reldist, sets x bins x (nfiles + 1) words back)
      ratio                flank_reldist_ms / nearest_hist_ms
      flank_rows_ms        Database.flanks over the first --row-regions regions, median of --reps (two rows come back)
      rows_ratio           flank_rows_ms / nearest_signed_rows_ms
      sum_is_flanked       flank_reldist(first --host-regions regions).hist.sum(axis=1) == the flanked pairs counted from flanks()
      equal_host           the host results (igd_amd.flanks_host / flank_reldist_host, first --host-regions regions) equal the device's
      flanked_any          flanked regions in the any-dataset column, all sets
No threshold: the first measurement of the stage.  Registers and occupancy: tools/regs.sh (profiles/enrich/regs_flank.txt).
Usage: tools/flank_probe.py [--sets 100] [--regions 10000] [--out profiles/enrich/flank_probe.jsonl]"""
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
    ap.add_argument("--bins", type=int, default=50)
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
    nq, W, B = a.sets * a.regions, a.window, a.bins
    ichr, qs, qe = (np.ascontiguousarray(x, np.int32) for x in synth.make_queries(nq, seed=999, sorted_=False))
    off = np.arange(a.sets + 1, dtype=np.int64) * a.regions
    nh = min(a.host_regions, nq)
    hoff = np.array([0, nh], np.int64)
    nr = min(a.row_regions, nq)
    edges = np.unique(np.linspace(-W, W + 1, 10).astype(np.int64))
    h = db.nearest_hist(ichr, qs, qe, off, W, edges)                         # warm-up (workspaces)
    hist_ms = med(lambda: db.nearest_hist(ichr, qs, qe, off, W, edges, hist=h.hist), a.reps)
    sdist, _ = db.nearest_signed(ichr[:nr], qs[:nr], qe[:nr], W)
    srows_ms = med(lambda: db.nearest_signed(ichr[:nr], qs[:nr], qe[:nr], W, sdist=sdist), a.reps)
    line = dict(sets=a.sets, regions_per_set=a.regions, nfiles=int(db.nfiles), window=W, bins=B, host_regions=int(nh), row_regions=int(nr),
                nearest_hist_ms=round(hist_ms, 3), nearest_signed_rows_ms=round(srows_ms, 3), cases=[])
    equal = True
    for ms in ("edges", "midpoints"):
        fr = db.flank_reldist(ichr, qs, qe, off, W, B, measure=ms)          # warm-up (workspaces)
        rel_ms = med(lambda: db.flank_reldist(ichr, qs, qe, off, W, B, measure=ms, hist=fr.hist), a.reps)
        up, down, _, _ = db.flanks(ichr[:nr], qs[:nr], qe[:nr], W, measure=ms)
        rows_ms = med(lambda: db.flanks(ichr[:nr], qs[:nr], qe[:nr], W, measure=ms, up=up, down=down), a.reps)
        du, dd, dum, ddm = db.flanks(ichr[:nh], qs[:nh], qe[:nh], W, measure=ms)
        dh = db.flank_reldist(ichr[:nh], qs[:nh], qe[:nh], hoff, W, B, measure=ms)
        hu, hd, hum, hdm = igd_amd.flanks_host(path, ichr[:nh], qs[:nh], qe[:nh], W, measure=ms)
        hh = igd_amd.flank_reldist_host(path, ichr[:nh], qs[:nh], qe[:nh], hoff, W, B, measure=ms)
        u = np.concatenate([du, dum[:, None]], axis=1).astype(np.int64)
        d = np.concatenate([dd, ddm[:, None]], axis=1).astype(np.int64)
        flanked = ((u >= 0) & (d >= 0) & (u + d > 0)).sum(axis=0)
        case = dict(measure=ms, flank_reldist_ms=round(rel_ms, 3), ratio=round(rel_ms / hist_ms, 2), flank_rows_ms=round(rows_ms, 3),
                    rows_ratio=round(rows_ms / srows_ms, 2), sum_is_flanked=bool(np.array_equal(dh.hist.sum(axis=1)[0], flanked)),
                    equal_host=bool(np.array_equal(hh.hist, dh.hist) and all(np.array_equal(x, y) for x, y in zip((hu, hd, hum, hdm), (du, dd, dum, ddm)))),
                    flanked_any=int(fr.hist[:, :, -1].sum()))
        equal = equal and case["sum_is_flanked"] and case["equal_host"]
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
