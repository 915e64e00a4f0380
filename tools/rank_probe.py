#!/usr/bin/env python3
"""tools/rank_probe.py -- GPU box: the rank columns and q-values of an enrichment table (Database.enrichment_ranks) beside
the host route on one thread (igd_amd.rank_host) and numpy's argsort on the same matrices.

The table is 1 000 sets x 1 900 columns, the width of the roadmap-scale database.  The rank call takes its width from the
caller and never looks at the database, so the matrices are drawn here (ties, zeros, huge pvalue_log, inf and NaN odds
ratios, as an enrichment table has them) and the handle is any small database (--db).  One JSON line:
  gpu_ms           enrichment_ranks wall time (three uploads, the kernel, six downloads), median of --reps calls
  gpu_q_only_ms    the same asking for qvalue_log alone through the C entry point (one upload, one column sorted)
  host_ms          igd_amd.rank_host, one thread, median of --host-reps runs
  argsort_ms       np.argsort along the rows of the three matrices (kind="stable"): the sort a caller's own loop starts with,
                   without the tie handling or the q-values
  host_over_gpu, argsort_over_gpu
  equal_ranks      the GPU's four integer columns and mean_rnk equal the host route's; max |GPU - host| of qvalue_log
The kernel's registers and occupancy come from tools/regs.sh (profiles/enrich/regs.txt).
Usage: tools/rank_probe.py [--sets 1000] [--cols 1900] [--out profiles/enrich/rank_probe.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import igd_amd  # noqa: E402
from igd_amd import Database  # noqa: E402


def med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def table(nsets, ncols, seed=11):
    rng = np.random.default_rng(seed)
    sup = rng.poisson(3.0, (nsets, ncols)).astype(np.int64)
    pv = np.where(sup == 0, 0.0, rng.exponential(2.0, (nsets, ncols)) * np.where(rng.random((nsets, ncols)) < 0.01, 500.0, 1.0))
    kind = rng.random((nsets, ncols))
    odds = np.where(sup == 0, np.where(kind < 0.1, np.nan, 0.0), np.where(kind < 0.02, np.inf, np.exp(rng.normal(0.0, 1.0, (nsets, ncols)))))
    return sup, pv, odds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", default=os.path.join(ROOT, "tests", "golden", "branch", "db.igd"))
    ap.add_argument("--sets", type=int, default=1000)
    ap.add_argument("--cols", type=int, default=1900)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    a = ap.parse_args()
    sup, pv, odds = table(a.sets, a.cols)
    db = Database(a.db)
    got = db.enrichment_ranks(sup, pv, odds)                                 # warm-up (workspace, LDS attribute)
    gpu_ms = med(lambda: db.enrichment_ranks(sup, pv, odds), a.reps)
    q = np.empty(sup.shape)

    def q_only():
        rc = db._H.igd_hip_enrich_ranks(db.dev, None, C.c_void_p(pv.ctypes.data), None, sup.shape[0], sup.shape[1],
                                        C.c_void_p(q.ctypes.data), None, None, None, None, None)
        assert rc == 0
    q_only()
    q_ms = med(q_only, a.reps)
    host = igd_amd.rank_host(sup, pv, odds)
    host_ms = med(lambda: igd_amd.rank_host(sup, pv, odds), a.host_reps)
    argsort_ms = med(lambda: [np.argsort(x, axis=1, kind="stable") for x in (sup, pv, odds)], a.host_reps)
    line = dict(sets=a.sets, cols=a.cols, cells=int(sup.size), gpu_ms=round(gpu_ms, 3), gpu_q_only_ms=round(q_ms, 3),
                host_ms=round(host_ms, 1), argsort_ms=round(argsort_ms, 1), host_over_gpu=round(host_ms / gpu_ms, 1),
                argsort_over_gpu=round(argsort_ms / gpu_ms, 1),
                equal_ranks=bool(all(np.array_equal(x, y) for x, y in zip(got[1:], host[1:]))),
                q_only_equal=bool(np.array_equal(q, got.qvalue_log)),
                max_gpu_minus_host_q=float(np.abs(got.qvalue_log - host.qvalue_log).max()),
                max_qvalue_log=float(got.qvalue_log.max()), lds_cols=int(db._H.igd_hip_rank_lds_cols()),
                grid=int(db._H.igd_hip_rank_grid(a.sets)))
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
