#!/usr/bin/env python3
"""tools/map_probe.py -- GPU box: the values of the overlapping records per region set and dataset (Database.map_sets) beside
Database.nearest_sets at W = 0, the call that does the same walk and writes rows of the same volume as op count.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Regions = synth.make_queries(
--sets x --regions, seed=999), cut into --sets sets.  One JSON line:
  nearest_sets_w0_ms       Database.nearest_sets at W = 0, median of --reps calls
  map_sets_ms              {count, max, sum}: Database.map_sets, median of --reps calls (regions up, per chunk igd_map_rows and
                           igd_map_reduce, 3 x sets x nfiles words back), with the form the op took (lds / wide) and the ratio to
                           nearest_sets_w0_ms
  map_values_max_ms        Database.map_values (op max: count and agg rows back to the host) over the first --values-regions
                           regions, median of --reps (12 nfiles bytes per region come back: 22.8 GB for 10^6 regions of 1 900 files,
                           hence a part of them)
  host_1thread_ms          igd_amd.map_sets_host (op sum) on ONE thread over the first --host-regions regions, median of --reps
  equal                    n_hit equals nearest_sets' n_overlap without its last column for every op, pairs is the same under
                           every op, AND the host result equals the device result on the host's regions
No threshold: the first measurement of the stage.  Registers and occupancy: tools/regs.sh (profiles/enrich/regs_map.txt).
Usage: tools/map_probe.py [--sets 100] [--regions 10000] [--out profiles/enrich/map_probe.jsonl]"""
import argparse
import json
import os
import re
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


def lds_limits():
    src = open(os.path.join(ROOT, "igd_amd", "csrc", "engine", "map_dev.hpp")).read()
    wave = int(re.search(r"^#define\s+IGD_MAP_LDS_WAVE_BYTES\s+(\d+)", src, re.M).group(1))
    return {"count": wave // 4, "max": wave // 8, "sum": wave // 12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/igdb")
    ap.add_argument("--sets", type=int, default=100)
    ap.add_argument("--regions", type=int, default=10000, help="regions per set")
    ap.add_argument("--values-regions", type=int, default=100000)
    ap.add_argument("--host-regions", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    nq = a.sets * a.regions
    ichr, qs, qe = (np.ascontiguousarray(x, np.int32) for x in synth.make_queries(nq, seed=999, sorted_=False))
    off = np.arange(a.sets + 1, dtype=np.int64) * a.regions
    nh, nv = min(a.host_regions, nq), min(a.values_regions, nq)
    hoff = np.array([0, nh], np.int64)
    os.environ["IGD_HOST_THREADS"] = "1"
    ns = db.nearest_sets(ichr, qs, qe, off, 0)                                # warm-up (workspaces)
    near_ms = med(lambda: db.nearest_sets(ichr, qs, qe, off, 0), a.reps)
    line = dict(sets=a.sets, regions_per_set=a.regions, nfiles=int(db.nfiles), host_regions=int(nh), values_regions=int(nv),
                nearest_sets_w0_ms=round(near_ms, 3), map_sets_ms={})
    equal, lim, pairs = True, lds_limits(), None
    for op in ("count", "max", "sum"):
        ms = db.map_sets(ichr, qs, qe, off, op)                               # warm-up
        t = med(lambda: db.map_sets(ichr, qs, qe, off, op), a.reps)
        equal = equal and bool(np.array_equal(ms.n_hit, ns.n_overlap[:, :-1])) and (pairs is None or bool(np.array_equal(ms.pairs, pairs)))
        pairs = ms.pairs
        line["map_sets_ms"][op] = dict(ms=round(t, 3), form="lds" if db.nfiles <= lim[op] else "wide", ratio_to_nearest=round(t / near_ms, 2))
    count = np.empty((nv, db.nfiles), np.int32)
    agg = np.empty((nv, db.nfiles), np.int64)
    values = lambda: db.map_values(ichr[:nv], qs[:nv], qe[:nv], "max", count=count, agg=agg)
    values()
    line["map_values_max_ms"] = round(med(values, a.reps), 3)
    hs = [None]

    def host():
        hs[0] = igd_amd.map_sets_host(path, ichr[:nh], qs[:nh], qe[:nh], hoff, "sum")
    line["host_1thread_ms"] = round(med(host, a.reps), 3)
    dm = db.map_sets(ichr[:nh], qs[:nh], qe[:nh], hoff, "sum")
    equal = equal and all(np.array_equal(g, w) for g, w in zip(hs[0][:3], dm[:3]))
    line["pairs"] = int(pairs.sum())
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
