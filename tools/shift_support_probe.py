#!/usr/bin/env python3
"""tools/shift_support_probe.py -- GPU box: the shift profile of the support in one call (Database.shift_support: the regions
uploaded once, kernel igd_shift_regions per chunk of shifts) beside what a user could do before it: the set shifted on the host
and handed to Database.support_sets as nshift copies, in as many calls as igd_hip_max_batch() forces.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Regions = synth.make_queries(--regions,
seed=999); contig lengths as permute_probe.py; offsets = shift_offsets(--window, --step) (41 by default).  ONE run of each side,
nothing repeated, no warm-up of either: both pay their workspaces.  One JSON line:
  shift_support_ms   the wall time of the one shift_support call
  support_sets_ms    the wall time of shifting on the host (numpy) plus the support_sets calls, calls = their number
  equal              every integer of the two matrices agrees (asserted)
No threshold and no ratio promised: nobody has measured this.
Usage: tools/shift_support_probe.py [--regions 100000] [--window 2000] [--step 100] [--out profiles/enrich/shift_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import igd_amd  # noqa: E402
from igd_amd import Database, _native, synth  # noqa: E402


def host_shift(qs, qe, L, d):
    """THE SHIFT of include/igd_hip.h on valid regions of known contigs (L: the length of each region's contig)"""
    ln = qe.astype(np.int64) - qs
    s = np.minimum(np.maximum(qs.astype(np.int64) + d, 0), L - ln)
    return s.astype(np.int32), (s + ln).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/igdb")
    ap.add_argument("--regions", type=int, default=100000)
    ap.add_argument("--window", type=int, default=2000)
    ap.add_argument("--step", type=int, default=100)
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
    offsets = igd_amd.shift_offsets(a.window, a.step)
    nq, n = len(qs), len(offsets)

    t = time.perf_counter()
    ss = db.shift_support(ichr, qs, qe, ctg_len, offsets)
    shift_ms = 1e3 * (time.perf_counter() - t)

    per_call = max(int(_native.hip().igd_hip_max_batch()) // nq, 1)
    L = ctg_len.astype(np.int64)[ichr]
    rows, calls = [], 0
    t = time.perf_counter()
    for j0 in range(0, n, per_call):
        k = min(per_call, n - j0)
        cs, ce = zip(*[host_shift(qs, qe, L, int(d)) for d in offsets[j0:j0 + k]])
        sup, nhit = db.support_sets(np.tile(ichr, k), np.concatenate(cs), np.concatenate(ce), np.arange(k + 1, dtype=np.int64) * nq)
        rows.append(np.concatenate([sup, nhit[:, None]], axis=1))
        calls += 1
    sets_ms = 1e3 * (time.perf_counter() - t)
    equal = bool(np.array_equal(np.concatenate(rows), ss.shifted))
    assert equal, "shift_support and support_sets over the host-shifted copies differ"

    line = dict(regions=int(nq), shifts=int(n), window=a.window, step=a.step, nfiles=int(db.nfiles), shift_support_ms=round(shift_ms, 3),
                support_sets_ms=round(sets_ms, 3), calls=calls, equal=equal, any_at_0=int(ss.shifted[n // 2, -1]),
                any_at_window=int(ss.shifted[-1, -1]))
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
