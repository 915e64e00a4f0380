#!/usr/bin/env python3
"""tools/permute_bp_probe.py -- GPU box: the permutation null of the base-pair overlap (Database.permutation_bp: the merged runs are
handed to the coverage kernel on the device, kernels igd_merge_slices and igd_merge_row_bp) beside the same table through the
calls there were before it.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  One JSON line, per case of --cases
(regions, synth.make_queries with seed=999; --perms circular permutations; contig lengths = the database's tiles, stretched to
the farthest region).  Medians of --reps calls after a warm-up of
  permutation_bp_ms        Database.permutation_bp: regions up once; per chunk igd_permute_regions, the merge launches,
                           igd_merge_slices, igd_sets_coverage, igd_merge_row_bp and the copies, no wait in between
  composition_ms           Database.permute_regions (the explicit lists come back to the host), then Database.jaccard_sets with
                           the set as given and the permuted sets: merge, runs back to the host, slices cut there, coverage
  composition_permute_ms / composition_jaccard_ms   its two parts
  ratio                    composition_ms / permutation_bp_ms
  equal                    every integer of the two tables
No threshold: the first measurement of the stage.  Registers: profiles/enrich/regs_permute_bp.txt.
Usage: tools/permute_bp_probe.py [--out profiles/enrich/permute_bp_probe.jsonl]"""
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
    ap.add_argument("--cases", default="10000,100000", help="regions of the set, one case each")
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    db.dataset_bp()                                                               # (kept in the handle: not part of either side)
    P = a.perms
    line = dict(nfiles=int(db.nfiles), perms=int(P), mode="circular", cases=[])
    equal = True
    for nq in (int(x) for x in a.cases.split(",")):
        ichr, qs, qe = (np.ascontiguousarray(x, np.int32) for x in synth.make_queries(nq, seed=999))
        ctg_len = np.array(db.ntile, np.int64) * db.nbp
        np.maximum.at(ctg_len, ichr, qe.astype(np.int64))
        ctg_len = ctg_len.astype(np.int32)
        off = np.arange(P + 2, dtype=np.int64) * nq
        pb = db.permutation_bp(ichr, qs, qe, ctg_len, P)                          # warm-up (workspaces)
        null_ms = med(lambda: db.permutation_bp(ichr, qs, qe, ctg_len, P), a.reps)
        st = {}

        def composition():
            t0 = time.perf_counter()
            s, e = db.permute_regions(ichr, qs, qe, ctg_len, 0, P)
            t1 = time.perf_counter()
            js = db.jaccard_sets(np.tile(ichr, P + 1), np.concatenate([qs, s.ravel()]), np.concatenate([qe, e.ravel()]), off)
            t2 = time.perf_counter()
            st.setdefault("perm", []).append(t1 - t0)
            st.setdefault("jac", []).append(t2 - t1)
            st["last"] = js
        composition()                                                             # warm-up
        st = {}
        comp_ms = med(composition, a.reps)
        js = st["last"]
        eq = bool(np.array_equal(pb.inter, js.inter) and np.array_equal(pb.set_bp, js.set_bp) and np.array_equal(pb.n_merged, js.n_merged) and
                  (js.n_dropped == pb.n_dropped).all() and np.array_equal(pb.file_bp, js.file_bp))
        equal = equal and eq
        line["cases"].append(dict(regions=int(nq), permutation_bp_ms=round(null_ms, 3), composition_ms=round(comp_ms, 3),
                                  composition_permute_ms=round(1e3 * float(np.median(st["perm"])), 3),
                                  composition_jaccard_ms=round(1e3 * float(np.median(st["jac"])), 3), ratio=round(comp_ms / null_ms, 2), equal=eq,
                                  any_bp_observed=int(pb.inter[0, -1]), any_bp_mean=round(float(pb.inter[1:, -1].mean()), 1),
                                  set_bp_observed=int(pb.set_bp[0]), set_bp_min=int(pb.set_bp.min())))
        del js, st, pb
    line["equal"] = equal
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
