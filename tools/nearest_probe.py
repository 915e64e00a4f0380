#!/usr/bin/env python3
"""tools/nearest_probe.py -- GPU box: the nearest record per dataset within a window (Database.nearest_sets) beside the only
device route there was before it: Database.support_sets on the same regions padded by W, which yields n_within only.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Regions = synth.make_queries(
--sets x --regions, seed=999), cut into --sets sets.  One JSON line; per window W of --windows (0, 10^4, 10^6):
  nearest_sets_ms          Database.nearest_sets wall time, median of --reps calls (regions up, per chunk igd_nearest_rows and
                           igd_nearest_reduce, 3 x sets x (nfiles + 1) words back)
  padded_support_ms        Database.support_sets (rule FLAT) over the padded regions, median of --reps
  ratio                    padded_support_ms / nearest_sets_ms
  host_1thread_ms          igd_amd.nearest_sets_host on ONE thread over the first --host-regions regions, median of --reps
  equal                    n_within from the padded regions equals the call's n_within (over the regions whose padding does not
                           clamp at 0), AND the host result equals the device result on the host's regions
No threshold: the first measurement of the stage.  Registers and occupancy: tools/regs.sh (profiles/enrich/regs_nearest.txt).
Usage: tools/nearest_probe.py [--sets 100] [--regions 10000] [--out profiles/enrich/nearest_probe.jsonl]"""
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
from igd_amd import _native as N  # noqa: E402


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
    ap.add_argument("--windows", default="0,10000,1000000")
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
    nh = min(a.host_regions, nq)
    hoff = np.array([0, nh], np.int64)
    os.environ["IGD_HOST_THREADS"] = "1"
    line = dict(sets=a.sets, regions_per_set=a.regions, nfiles=int(db.nfiles), host_regions=int(nh), windows=[])
    equal = True
    for W in (int(w) for w in a.windows.split(",")):
        ns = db.nearest_sets(ichr, qs, qe, off, W)                            # warm-up (workspaces)
        dev_ms = med(lambda: db.nearest_sets(ichr, qs, qe, off, W), a.reps)
        ps, pe = (qs.astype(np.int64) - W).clip(-2 ** 31, None).astype(np.int32), (qe.astype(np.int64) + W).clip(None, 2 ** 31 - 1).astype(np.int32)
        pad = lambda: db.support_sets(ichr, ps, pe, off, rule=N.IGD_HIP_RULE_FLAT, value_filter=N.IGD_HIP_NO_VALUE_FILTER)
        pad()
        pad_ms = med(pad, a.reps)
        # the padded route where padding does not clamp at 0: those regions alone, through both routes
        keep = qs.astype(np.int64) - W >= 0
        koff = np.concatenate([[0], np.cumsum(keep)])[off].astype(np.int64)
        kn = db.nearest_sets(ichr[keep], qs[keep], qe[keep], koff, W)
        sup, nhit = db.support_sets(ichr[keep], ps[keep], pe[keep], koff, rule=N.IGD_HIP_RULE_FLAT, value_filter=N.IGD_HIP_NO_VALUE_FILTER)
        eq_pad = bool(np.array_equal(kn.n_within[:, :-1], sup) and np.array_equal(kn.n_within[:, -1], nhit))
        hs = [None]

        def host():
            hs[0] = igd_amd.nearest_sets_host(path, ichr[:nh], qs[:nh], qe[:nh], hoff, W)
        host_ms = med(host, a.reps)
        dn = db.nearest_sets(ichr[:nh], qs[:nh], qe[:nh], hoff, W)
        eq_host = all(np.array_equal(g, w) for g, w in zip(hs[0][:3], dn[:3]))
        equal = equal and eq_pad and eq_host
        nw_any = int(ns.n_within[:, -1].sum())
        line["windows"].append(dict(window=W, nearest_sets_ms=round(dev_ms, 3), padded_support_ms=round(pad_ms, 3),
                                    ratio=round(pad_ms / dev_ms, 2), host_1thread_ms=round(host_ms, 3), equal_padded=eq_pad,
                                    equal_host=bool(eq_host), regions_unclamped=int(keep.sum()), n_within_any=nw_any,
                                    n_overlap_any=int(ns.n_overlap[:, -1].sum()),
                                    mean_dist_any=round(float(ns.sum_dist[:, -1].sum()) / nw_any, 2) if nw_any else None))
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
