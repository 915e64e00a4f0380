#!/usr/bin/env python3
"""tools/permute_probe.py -- GPU box: the permutation null of region-set support (Database.permutation_support) beside the only
route there was before it: the permuted lists generated in numpy, counted by Database.support_sets, the statistics in numpy.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Regions = synth.make_queries(
--regions, seed=999); contig lengths = the database's tiles, stretched to the farthest region.  One JSON line:
  permutation_support_ms   Database.permutation_support wall time, median of --reps calls (regions up, per chunk the permute,
                           support and statistics kernels, 7 x (nfiles + 1) words back)
  explicit_ms              the explicit route, median of --reps: explicit_generate_ms (tests/permute_ref.permute in numpy) +
                           explicit_support_sets_ms (H2D of the lists, the same support kernel, the rows back) +
                           explicit_stats_ms (numpy over the rows)
  ratio                    explicit_ms / permutation_support_ms
  equal                    the two routes agree on every integer
  permute_regions_ms       the generic entry of igd_permute_regions on the same shape (it copies the lists to the host, which
                           the call itself does not: an upper bound of the stage)
  perm_stats_ms            the generic entry of igd_perm_stats on the explicit route's rows (rows up: an upper bound)
No threshold: the first measurement of the stage.  Registers and occupancy: tools/regs.sh (profiles/enrich/regs_permute.txt).
Usage: tools/permute_probe.py [--regions 10000] [--perms 1000] [--mode circular] [--out profiles/enrich/permute_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import permute_ref as PR  # noqa: E402
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
    ap.add_argument("--mode", default="circular")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    ichr, qs, qe = (np.ascontiguousarray(x, np.int32) for x in synth.make_queries(a.regions, seed=999))
    ctg_len = np.array(db.ntile, np.int64) * db.nbp
    np.maximum.at(ctg_len, ichr, qe.astype(np.int64))
    ctg_len = ctg_len.astype(np.int32)
    nq, P = a.regions, a.perms
    off = np.arange(P + 1, dtype=np.int64) * nq

    ps = db.permutation_support(ichr, qs, qe, ctg_len, P, mode=a.mode)        # warm-up (workspaces)
    dev_ms = med(lambda: db.permutation_support(ichr, qs, qe, ctg_len, P, mode=a.mode), a.reps)

    st = {}

    def explicit():
        t0 = time.perf_counter()
        s, e = PR.permute(ichr, qs, qe, ctg_len, 0, P, 0, a.mode)
        c = np.tile(ichr, P)
        t1 = time.perf_counter()
        sup, nhit = db.support_sets(c, s.ravel(), e.ravel(), off)
        osup, onhit = db.support_sets(ichr, qs, qe, off[:2])
        t2 = time.perf_counter()
        rows = np.concatenate([sup, nhit[:, None]], axis=1)
        obs = np.concatenate([osup[0], onhit])
        res = PR.stats(rows, obs)
        t3 = time.perf_counter()
        st.setdefault("gen", []).append(t1 - t0)
        st.setdefault("sup", []).append(t2 - t1)
        st.setdefault("stat", []).append(t3 - t2)
        st["last"] = (obs, rows, res)
    explicit()                                                                # warm-up
    st = {}
    exp_ms = med(explicit, a.reps)
    obs, rows, res = st["last"]
    equal = bool(np.array_equal(ps.observed, obs) and all(np.array_equal(g, w) for g, w in zip(ps[1:7], res)))

    permute_ms = med(lambda: db.permute_regions(ichr, qs, qe, ctg_len, 0, P, 0, a.mode), a.reps)
    out6 = [np.empty(rows.shape[1], np.int64) for _ in range(6)]
    stats_ms = med(lambda: db.perm_stats(rows, obs, out=out6), a.reps)

    line = dict(regions=int(nq), perms=int(P), mode=a.mode, nfiles=int(db.nfiles), permutation_support_ms=round(dev_ms, 3),
                explicit_ms=round(exp_ms, 3), explicit_generate_ms=round(1e3 * float(np.median(st["gen"])), 3),
                explicit_support_sets_ms=round(1e3 * float(np.median(st["sup"])), 3),
                explicit_stats_ms=round(1e3 * float(np.median(st["stat"])), 3), ratio=round(exp_ms / dev_ms, 2), equal=equal,
                permute_regions_ms=round(permute_ms, 3), perm_stats_ms=round(stats_ms, 3),
                observed_any=int(ps.observed[-1]), mean_any=round(float(ps.sum[-1]) / P, 3))
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
