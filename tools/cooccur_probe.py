#!/usr/bin/env python3
"""tools/cooccur_probe.py -- GPU box: dataset co-occurrence over a region list (Database.cooccurrence), its stages timed
apart, beside the host route on one thread.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Regions = synth.make_queries(
--regions, seed=999), in the generator's order.  One JSON line:
  cooccurrence_ms   Database.cooccurrence wall time, median of --reps calls (upload, membership, transpose, Gram, the matrix back)
  membership_ms     membership alone (it copies the rows to the host, which the call itself does not: an upper bound)
  transpose_ms      transpose_bits on those rows (rows up, columns back: an upper bound)
  gram_ms           bitrows_gram, symmetric form, on the first nfiles columns (columns up, the matrix back: an upper bound)
  host_ms           igd_amd.cooccur_host on ONE thread on the first --host-regions regions
  equal             the device and host routes agree on that subset: the matrix and nhit
  pairs, nhit       pairs of datasets a < b with a common region; regions with any dataset
Registers and occupancy: tools/regs.sh (profiles/enrich/regs_cooccur.txt).
Usage: tools/cooccur_probe.py [--regions 1000000] [--host-regions 100000] [--out profiles/enrich/cooccur_probe.jsonl]"""
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
    ap.add_argument("--regions", type=int, default=1000000)
    ap.add_argument("--host-regions", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    q = tuple(np.ascontiguousarray(x, np.int32) for x in synth.make_queries(a.regions, seed=999))
    cooc, nhit = db.cooccurrence(*q)                                        # warm-up (workspaces)
    cooccurrence_ms = med(lambda: db.cooccurrence(*q), a.reps)
    bits, _, _ = db.membership(*q)
    membership_ms = med(lambda: db.membership(*q, bits=bits), a.reps)
    cols = db.transpose_bits(bits)
    transpose_ms = med(lambda: db.transpose_bits(bits, cols=cols), a.reps)
    colw = np.ascontiguousarray(cols[:db.nfiles]).view(np.uint32)
    gram = db.bitrows_gram(colw)
    gram_ms = med(lambda: db.bitrows_gram(colw, out=gram), a.reps)
    stages_equal = bool(np.array_equal(gram, cooc))
    h = min(a.host_regions, a.regions)
    sub = tuple(x[:h] for x in q)
    os.environ["IGD_HOST_THREADS"] = "1"
    t0 = time.perf_counter()
    hc, hn = igd_amd.cooccur_host(path, *sub)
    host_ms = 1e3 * (time.perf_counter() - t0)
    dc, dn = db.cooccurrence(*sub)
    line = dict(regions=int(a.regions), nfiles=int(db.nfiles), cooccurrence_ms=round(cooccurrence_ms, 3),
                membership_ms=round(membership_ms, 3), transpose_ms=round(transpose_ms, 3), gram_ms=round(gram_ms, 3),
                stages_equal=stages_equal, host_regions=int(h), host_ms=round(host_ms, 1),
                equal=bool(np.array_equal(hc, dc) and hn == dn), pairs=int((np.triu(cooc, 1) > 0).sum()), nhit=int(nhit),
                slices=int(igd_amd._native.hip().igd_hip_gram_slices(db.nfiles, 0, 2 * ((a.regions + 63) // 64))))
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
