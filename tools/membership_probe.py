#!/usr/bin/env python3
"""tools/membership_probe.py -- GPU box: per-query dataset membership (Database.membership) beside the only route to the
same rows without igd_member_rows: Database.enumerate_stream8 (8 bytes per overlap over PCIe) plus a numpy reduction of each
chunk to the same bit rows, on the same database and queries.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Queries: synth.make_queries(n,
seed=1000).  One JSON line per case (n queries):
  member_ms     membership wall time (H2D + kernel + D2H of the rows), median of --reps calls after one warm-up call
  enum_ms       enumerate_stream8 + per chunk np.bitwise_or.at into the rows, wall time (--enum-reps runs, median)
  equal         the rows, nfiles_hit and nhit made from the enumeration equal membership's exactly
  row_bytes     bytes of one row; overlaps_per_query the records `-f` ships per query (8 bytes each)
  nhit_support  nhit equals what Database.support returns for the same queries
The kernel's own time comes from a run of one case under `rocprofv3 --kernel-trace --stats`: this tool prints host wall
times only.
Usage: tools/membership_probe.py [--n N ...] [--out profiles/membership/probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from igd_amd import Database, synth  # noqa: E402

CASES = [100000, 1000000]


def med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def rows_from_enumeration(db, ichr, qs, qe):
    """the route without the membership kernel: every overlap to the host, OR-ed into the query's row chunk by chunk"""
    nW = db.member_words
    bits = np.zeros(len(qs) * nW, np.uint32)

    def on_chunk(q0, q1, qoff, rec, b):
        if not len(rec):
            return
        idx = rec[:, 1] & np.uint32((1 << b) - 1)
        qno = np.repeat(np.arange(q0, q1, dtype=np.int64), np.diff(qoff[q0:q1 + 1]))
        np.bitwise_or.at(bits, qno * nW + (idx >> np.uint32(5)), np.uint32(1) << (idx & np.uint32(31)))

    _, total = db.enumerate_stream8(ichr, qs, qe, on_chunk)
    bits = bits.reshape(len(qs), nW)
    nfh = db.unpack_membership(bits, db.nfiles).sum(axis=1).astype(np.int32)
    return bits, nfh, int((nfh > 0).sum()), total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/igdb")
    ap.add_argument("--n", action="append", type=int, help="queries of a case (default: 10^5 and 10^6)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--enum-reps", type=int, default=1)
    ap.add_argument("--no-enum", action="store_true", help="skip the enumeration route (profiling runs)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    if db.hit8_idx_bits() < 0:
        sys.exit("the packed -f record does not fit this database")
    for n in (a.n or CASES):
        ichr, qs, qe = synth.make_queries(n, seed=1000)
        bits, nfh, nhit = db.membership(ichr, qs, qe)                 # warm-up (workspaces)
        buf = np.empty_like(bits)
        member_ms = med(lambda: db.membership(ichr, qs, qe, bits=buf), a.reps)
        _, snhit = db.support(ichr, qs, qe)
        line = dict(case="%d queries" % n, queries=n, files=db.nfiles, row_bytes=4 * db.member_words, member_ms=round(member_ms, 3),
                    nhit=int(nhit), nhit_support=bool(snhit == nhit), files_per_query=round(float(nfh.mean()), 2),
                    row_mbytes=round(bits.nbytes / 1e6, 1))
        if not a.no_enum:
            e_bits, e_nfh, e_nhit, total = rows_from_enumeration(db, ichr, qs, qe)
            enum_ms = med(lambda: rows_from_enumeration(db, ichr, qs, qe), a.enum_reps)
            line.update(enum_ms=round(enum_ms, 1), enum_reps=a.enum_reps, enum_over_member=round(enum_ms / member_ms, 1),
                        overlaps=int(total), overlaps_per_query=round(total / n, 2), enum_mbytes=round(8 * total / 1e6, 1),
                        equal=bool(np.array_equal(e_bits, bits) and np.array_equal(e_nfh, nfh) and e_nhit == nhit))
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
