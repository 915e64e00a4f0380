#!/usr/bin/env python3
"""tools/jaccard_probe.py -- GPU box: the device merge (Database.merge_sets_dev), the base-pair Jaccard table
(Database.jaccard_sets) and the merged base pairs per dataset (Database.dataset_bp, first and second call) beside their
yardsticks in the same process: Database.coverage_sets on the unmerged sets, and a numpy lexsort-and-sweep merge on the host.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Two inputs, as the coverage probe's:
100 sets x 10^4 regions and 1 set x 10^6 (synth.make_queries, seed=999).  One JSON line, per input:
  merge_dev_ms        merge_sets_dev on resident sets, stream synchronised, median of --reps calls after a warm-up
  jaccard_ms          jaccard_sets (merge, runs back, coverage of the runs), median of --reps
  coverage_ms         coverage_sets on the unmerged sets, median of --reps;  ratio = jaccard_ms / coverage_ms
  numpy_merge_ms      lexsort by (set, ichr, qs, qe) and a sweep with maximum.accumulate per (set, contig), median of --reps
  equal               the host route (igd_amd.jaccard_host, merge_host) equals the device on the first --host-regions regions
and dataset_bp_first_ms / dataset_bp_second_ms (one call each).  No threshold: the first measurement of the stage.
Usage: tools/jaccard_probe.py [--out profiles/enrich/jaccard_probe.jsonl]"""
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


def numpy_merge(ichr, qs, qe, off):
    """gap 0, the regions that take part only; returns the number of runs"""
    sets = np.repeat(np.arange(len(off) - 1), np.diff(off))
    keep = (ichr >= 0) & (qe > qs)
    k, c, s, e = sets[keep], ichr[keep], qs[keep].astype(np.int64), qe[keep].astype(np.int64)
    o = np.lexsort((e, s, c, k))
    k, c, s, e = k[o], c[o], s[o], e[o]
    seg = np.ones(len(s), bool)
    seg[1:] = (k[1:] != k[:-1]) | (c[1:] != c[:-1])
    # running maximum per segment: lift every segment above the one before it, then one maximum.accumulate
    lift = np.cumsum(seg).astype(np.int64) << 32
    run = np.maximum.accumulate(e + lift) - lift
    head = seg.copy()
    head[1:] |= s[1:] > run[:-1]
    return int(head.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/igdb")
    ap.add_argument("--host-regions", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    a = ap.parse_args()
    import torch
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    t = time.perf_counter()
    bp1 = db.dataset_bp()
    first_ms = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    bp2 = db.dataset_bp()
    second_ms = 1e3 * (time.perf_counter() - t)
    line = dict(nfiles=int(db.nfiles), dataset_bp_first_ms=round(first_ms, 3), dataset_bp_second_ms=round(second_ms, 3),
                dataset_bp_computed=db.dataset_bp_computed(), cases=[])
    equal = bool(np.array_equal(bp1, bp2))
    dev = torch.device("cuda", 0)
    for nsets, per in ((100, 10000), (1, 1000000)):
        n = nsets * per
        ichr, qs, qe = (np.ascontiguousarray(x, np.int32) for x in synth.make_queries(n, seed=999, sorted_=False))
        off = np.arange(nsets + 1, dtype=np.int64) * per
        d = [torch.from_numpy(x).to(dev) for x in (ichr, qs, qe, off)]
        o32 = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
        o64 = [torch.empty(k, dtype=torch.int64, device=dev) for k in (nsets + 1, nsets)]

        def merge_dev():
            db.merge_sets_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), nsets, n, o32[0].data_ptr(), o32[1].data_ptr(),
                              o32[2].data_ptr(), o64[0].data_ptr(), o64[1].data_ptr(), d_m_count=o32[3].data_ptr())
            db.sync()
        merge_dev()
        merge_ms = med(merge_dev, a.reps)
        js = db.jaccard_sets(ichr, qs, qe, off)
        jac_ms = med(lambda: db.jaccard_sets(ichr, qs, qe, off), a.reps)
        cov, _ = db.coverage_sets(ichr, qs, qe, off)
        cov_ms = med(lambda: db.coverage_sets(ichr, qs, qe, off), a.reps)
        runs = numpy_merge(ichr, qs, qe, off)
        np_ms = med(lambda: numpy_merge(ichr, qs, qe, off), a.reps)
        nh = min(a.host_regions, per)
        hoff = np.array([0, nh], np.int64)
        dj, hj = db.jaccard_sets(ichr[:nh], qs[:nh], qe[:nh], hoff), igd_amd.jaccard_host(path, ichr[:nh], qs[:nh], qe[:nh], hoff)
        dm, hm = db.merge_sets(ichr[:nh], qs[:nh], qe[:nh], hoff), igd_amd.merge_host(path, ichr[:nh], qs[:nh], qe[:nh], hoff)
        eq = all(np.array_equal(x, y) for x, y in zip(dj, hj)) and all(np.array_equal(x, y) for x, y in zip(dm, hm))
        eq = eq and int(o64[0][-1].item()) == runs == int(js.n_merged.sum())
        equal = equal and bool(eq)
        line["cases"].append(dict(sets=nsets, regions_per_set=per, merge_dev_ms=round(merge_ms, 3), jaccard_ms=round(jac_ms, 3),
                                  coverage_ms=round(cov_ms, 3), ratio=round(jac_ms / cov_ms, 2), numpy_merge_ms=round(np_ms, 3), runs=runs,
                                  equal=bool(eq)))
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
