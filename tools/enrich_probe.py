#!/usr/bin/env python3
"""tools/enrich_probe.py -- GPU box: region-set enrichment of many query sets against a universe (Database.enrichment_sets),
its two stages timed apart, beside the Fisher tests of the same tables on one host thread (igd_amd.fisher_host).

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Set k = synth.make_queries(n,
seed=1000 + k); the universe = the --universe-sets first sets together (so most set regions are universe regions and some
tables are clamped).  One JSON line per case (K sets x n queries):
  enrich_ms      enrichment_sets wall time (support of the K + 1 sets, then the cell kernel), median of --reps calls
  support_ms     support_sets on the same K + 1 sets: the support stage alone
  fisher_ms      Database.fisher on the K x nfiles tables of the result: the Fisher stage alone in its generic form (it
                 uploads four arrays where enrichment_sets uploads one: an upper bound of the stage inside enrich_ms)
  fisher_share   (enrich_ms - support_ms) / enrich_ms: the Fisher stage's share of the whole call
  host_ms        igd_amd.fisher_host on the same tables, one thread, one run (--host-cells of them when given, scaled)
  host_over_gpu  host_ms / (enrich_ms - support_ms)
  equal          enrichment_sets' statistics equal Database.fisher's bit for bit; max |GPU - host| of pvalue_log
The kernel's registers and occupancy come from tools/regs.sh (profiles/enrich/regs.txt).
Usage: tools/enrich_probe.py [--case K,n ...] [--out profiles/enrich/probe.jsonl]"""
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

CASES = [(1000, 1000)]


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
    ap.add_argument("--case", action="append", help="K,n (default: 1000 sets x 1000 queries)")
    ap.add_argument("--universe-sets", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-cells", type=int, default=0, help="time the host on this many of the tables and scale (0: all)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    cases = [tuple(int(x) for x in c.split(",")) for c in a.case] if a.case else CASES
    for K, n in cases:
        sets = [synth.make_queries(n, seed=1000 + k) for k in range(K)]
        ichr, qs, qe = (np.concatenate([s[i] for s in sets]) for i in range(3))
        off = np.arange(K + 1, dtype=np.int64) * n
        nu = min(a.universe_sets, K) * n
        u = (ichr[:nu], qs[:nu], qe[:nu])
        all_c, all_s, all_e = (np.concatenate([x, y]) for x, y in zip((ichr, qs, qe), u))
        all_off = np.concatenate([off, [off[-1] + nu]])
        res = db.enrichment_sets(ichr, qs, qe, off, *u)                      # warm-up (workspaces)
        tabs = [np.ascontiguousarray(x.ravel()) for x in (res.support, res.b, res.c, res.d)]
        p, o = db.fisher(*tabs)
        enrich_ms = med(lambda: db.enrichment_sets(ichr, qs, qe, off, *u), a.reps)
        support_ms = med(lambda: db.support_sets(all_c, all_s, all_e, all_off), a.reps)
        fisher_ms = med(lambda: db.fisher(*tabs), a.reps)
        m = a.host_cells if 0 < a.host_cells < len(tabs[0]) else len(tabs[0])
        pick = np.linspace(0, len(tabs[0]) - 1, m).astype(np.int64)
        sub = [t[pick] for t in tabs]
        t0 = time.perf_counter()
        hp, _ = igd_amd.fisher_host(*sub)
        host_ms = 1e3 * (time.perf_counter() - t0) * len(tabs[0]) / m
        stage = enrich_ms - support_ms
        line = dict(case="%d x %d" % (K, n), sets=K, queries_per_set=n, universe=nu, cells=int(len(tabs[0])),
                    enrich_ms=round(enrich_ms, 3), support_ms=round(support_ms, 3), fisher_ms=round(fisher_ms, 3),
                    fisher_share=round(stage / enrich_ms, 3), host_ms=round(host_ms, 1), host_cells=int(m),
                    host_over_gpu=round(host_ms / stage, 1) if stage > 0 else None,
                    equal=bool(np.array_equal(p, res.pvalue_log.ravel()) and np.array_equal(o, res.odds_ratio.ravel(), equal_nan=True)),
                    max_gpu_minus_host=float(np.abs(p[pick] - hp).max()), clamped=int(res.clamped.sum()),
                    rows_with_support=int((res.support > 0).sum()), max_pvalue_log=float(res.pvalue_log.max()))
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
