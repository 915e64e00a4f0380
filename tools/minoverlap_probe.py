#!/usr/bin/env python3
"""tools/minoverlap_probe.py -- GPU box: what the minimum overlap per pair costs.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Timed, each as the median of --reps
calls after one warm-up call, with their run-to-run spread (min .. max):
  support_ms / sets_ms   Database.support_sets / search_sets, 100 sets x 10^4 regions (set k = synth.make_queries(n, seed=1000 + k))
  permute_ms             Database.permutation_support, 1 000 permutations x 10^4 regions, circular
three ways: without a threshold (`inactive`), `-O 50` and `-A 0.5 -B 0.5`.  One JSON line holds the three rows; --out appends it
(profiles/enrich/minoverlap_probe.jsonl).  On a tree without `min_overlap=` (a parent commit) only the inactive row is timed, so
the same file measures both sides of a comparison.  Host wall times; the kernels' own times come from rocprofv3 --kernel-trace.
Usage: tools/minoverlap_probe.py [--reps 7] [--sets 100] [--n 10000] [--perms 1000] [--label TEXT] [--out FILE]"""
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


def timed(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(1e3 * (time.perf_counter() - t))
    return dict(median=round(float(np.median(ts)), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/igdb")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sets", type=int, default=100)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None, help="also append the line to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    K, n = a.sets, a.n
    sets = [synth.make_queries(n, seed=1000 + k) for k in range(K)]
    ichr, qs, qe = (np.concatenate([s[i] for s in sets]) for i in range(3))
    off = np.arange(K + 1, dtype=np.int64) * n
    # the permutation null wants regions inside their contigs: lengths that hold every region of the first set
    p_ichr, p_qs, p_qe = sets[0]
    ctg_len = np.full(db.nctg, 1, np.int64)
    np.maximum.at(ctg_len, p_ichr, p_qe.astype(np.int64) + 1000)
    ctg_len = np.minimum(ctg_len, 2 ** 31 - 1).astype(np.int32)
    ok = (p_ichr >= 0) & (p_qs >= 0) & (p_qe >= p_qs)
    p_ichr, p_qs, p_qe = p_ichr[ok], p_qs[ok], p_qe[ok]
    ways = [("inactive", {})]
    if hasattr(igd_amd, "MinOverlap") or "MinOverlap" in getattr(igd_amd, "__all__", ()):
        from igd_amd import MinOverlap
        ways += [("-O 50", dict(min_overlap=MinOverlap(bp=50))), ("-A 0.5 -B 0.5", dict(min_overlap=MinOverlap.from_fractions(0, 0.5, 0.5)))]
    rows = []
    for name, kw in ways:
        sup, nhit = db.support_sets(ichr, qs, qe, off, **kw)
        hits, tot = db.search_sets(ichr, qs, qe, off, **kw)
        r = dict(way=name, pairs=int(tot.sum()), support_sum=int(sup.sum()), nhit=int(nhit.sum()),
                 support_ms=timed(lambda: db.support_sets(ichr, qs, qe, off, **kw), a.reps),
                 sets_ms=timed(lambda: db.search_sets(ichr, qs, qe, off, **kw), a.reps),
                 permute_ms=timed(lambda: db.permutation_support(p_ichr, p_qs, p_qe, ctg_len, a.perms, seed=1, **kw), max(3, a.reps // 2)))
        rows.append(r)
        print(json.dumps(r), flush=True)
    line = json.dumps(dict(tool="minoverlap_probe", label=a.label, sets=K, regions_per_set=n, perms=a.perms, perm_regions=int(len(p_qs)),
                           reps=a.reps, rows=rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    db.close()


if __name__ == "__main__":
    main()
