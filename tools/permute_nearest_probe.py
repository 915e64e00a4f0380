#!/usr/bin/env python3
"""tools/permute_nearest_probe.py -- GPU box: the permutation null of the nearest-record distances (Database.permutation_nearest,
kernel igd_nearest_slices) beside what there was before it, and the fused set statistics beside the rows route.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  One JSON line:
  null       --regions regions (synth.make_queries, seed=999), --perms circular permutations at W = --window; contig lengths = the
             database's tiles, stretched to the farthest region.  Medians of --reps calls of
    permutation_nearest_ms   Database.permutation_nearest: regions up once, per chunk igd_permute_regions, a memset, ONE
                             igd_nearest_slices launch and a copy; 3 x (perms + 1) x (nfiles + 1) words back
    composition_ms           Database.permute_regions (the explicit lists come back to the host), Database.nearest_sets on them
                             and on the set as given, numpy for the rest (nothing is left to it here: the matrices ARE the result)
    composition_permute_ms / composition_nearest_sets_ms   its two parts
    equal                    every integer of the two routes
  sets       --sets x --set-regions regions (seed=999) cut into --sets sets, per window of --windows: medians of --reps calls of
             Database.nearest_sets_fused and Database.nearest_sets, their ratio, and equality of every integer
No threshold: the first measurements of the stage.  Registers: profiles/enrich/regs_nearest_fused.txt.
Usage: tools/permute_nearest_probe.py [--out profiles/enrich/permute_nearest_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

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
    ap.add_argument("--regions", type=int, default=10000)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--window", type=int, default=10000)
    ap.add_argument("--sets", type=int, default=100)
    ap.add_argument("--set-regions", type=int, default=10000)
    ap.add_argument("--windows", default="0,10000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)

    # ---- the null
    ichr, qs, qe = (np.ascontiguousarray(x, np.int32) for x in synth.make_queries(a.regions, seed=999))
    ctg_len = np.array(db.ntile, np.int64) * db.nbp
    np.maximum.at(ctg_len, ichr, qe.astype(np.int64))
    ctg_len = ctg_len.astype(np.int32)
    nq, P, W = a.regions, a.perms, a.window
    off = np.arange(P + 2, dtype=np.int64) * nq
    pn = db.permutation_nearest(ichr, qs, qe, ctg_len, P, W)                  # warm-up (workspaces)
    null_ms = med(lambda: db.permutation_nearest(ichr, qs, qe, ctg_len, P, W), a.reps)
    st = {}

    def composition():
        t0 = time.perf_counter()
        s, e = db.permute_regions(ichr, qs, qe, ctg_len, 0, P)
        t1 = time.perf_counter()
        c = np.tile(ichr, P + 1)
        ns = db.nearest_sets(c, np.concatenate([qs, s.ravel()]), np.concatenate([qe, e.ravel()]), off, W)
        t2 = time.perf_counter()
        st.setdefault("perm", []).append(t1 - t0)
        st.setdefault("near", []).append(t2 - t1)
        st["last"] = ns
    composition()                                                             # warm-up
    st = {}
    comp_ms = med(composition, a.reps)
    equal_null = all(np.array_equal(g, w) for g, w in zip(pn[:3], st["last"][:3]))
    nw = pn.n_within
    line = dict(nfiles=int(db.nfiles),
                null=dict(regions=int(nq), perms=int(P), window=int(W), mode="circular", permutation_nearest_ms=round(null_ms, 3),
                          composition_ms=round(comp_ms, 3), composition_permute_ms=round(1e3 * float(np.median(st["perm"])), 3),
                          composition_nearest_sets_ms=round(1e3 * float(np.median(st["near"])), 3), ratio=round(comp_ms / null_ms, 2),
                          equal=bool(equal_null), n_within_any_observed=int(nw[0, -1]),
                          n_within_any_mean=round(float(nw[1:, -1].mean()), 3)),
                sets=dict(sets=a.sets, regions_per_set=a.set_regions, windows=[]))

    # ---- the fused set statistics beside the rows route
    n = a.sets * a.set_regions
    ichr, qs, qe = (np.ascontiguousarray(x, np.int32) for x in synth.make_queries(n, seed=999, sorted_=False))
    soff = np.arange(a.sets + 1, dtype=np.int64) * a.set_regions
    equal = bool(equal_null)
    for w in (int(x) for x in a.windows.split(",")):
        fu = db.nearest_sets_fused(ichr, qs, qe, soff, w)                     # warm-up
        ro = db.nearest_sets(ichr, qs, qe, soff, w)
        fused_ms = med(lambda: db.nearest_sets_fused(ichr, qs, qe, soff, w), a.reps)
        rows_ms = med(lambda: db.nearest_sets(ichr, qs, qe, soff, w), a.reps)
        eq = all(np.array_equal(g, x) for g, x in zip(fu[:3], ro[:3]))
        equal = equal and eq
        line["sets"]["windows"].append(dict(window=w, nearest_sets_fused_ms=round(fused_ms, 3), nearest_sets_ms=round(rows_ms, 3),
                                            ratio=round(rows_ms / fused_ms, 2), equal=bool(eq)))
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
