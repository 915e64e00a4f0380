#!/usr/bin/env python3
"""tools/group_support_probe.py [--regions N] [--sets K] [--host] -- support per group of datasets against the route it replaces.

On the roadmap-scale synthetic database (1 900 files; bench.py's, generated on first use) with a three-facet grouping (cell type,
antibody, collection: about three labels per dataset) it times Database.group_support_files against the route a caller had
before: Database.membership in chunks, a numpy `any` per group over the unpacked rows and a sum per set.  It ASSERTS that the two
give equal integers and prints one JSON line with both times.  No threshold: the line is a measurement, not a test.
--host runs the same comparison without a GPU on a small synthetic database: igd_amd.group_support_host against
igdc_membership_host folded the same way (equality only; the times are the host's)."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import igd_amd                                                     # noqa: E402
from igd_amd import _native as N                                   # noqa: E402

CHUNK = 1 << 16                                                    # regions per membership call of the old route


def three_facets(nfiles):
    """cell type (f mod 127), antibody (f // 25) and collection (f // 400); every 97th dataset unlabelled"""
    labels = [[] if f % 97 == 96 else ["cell%d" % (f % 127), "ab%d" % (f // 25), "coll%d" % (f // 400)] for f in range(nfiles)]
    return igd_amd.build_groups(labels, nfiles)


def fold(member, dense, set_off):
    """any per group, sum per set: (gsupport, gnhit) of a bool[nq, nfiles] member matrix"""
    gm = (member.astype(np.float32) @ dense.astype(np.float32)) > 0
    k = len(set_off) - 1
    return (np.array([gm[set_off[i]:set_off[i + 1]].sum(axis=0) for i in range(k)], np.int64).reshape(k, dense.shape[1]),
            np.array([gm[set_off[i]:set_off[i + 1]].any(axis=1).sum() for i in range(k)], np.int64))


def old_route(member_rows, nfiles, q, set_off, dense):
    """membership in chunks of CHUNK regions, folded chunk by chunk"""
    k = len(set_off) - 1
    gsup, gnhit = np.zeros((k, dense.shape[1]), np.int64), np.zeros(k, np.int64)
    n = len(q[1])
    for c0 in range(0, n, CHUNK):
        c1 = min(n, c0 + CHUNK)
        member = member_rows(q[0][c0:c1], q[1][c0:c1], q[2][c0:c1])
        off = np.clip(set_off, c0, c1) - c0
        s, h = fold(member, dense, off)
        gsup += s
        gnhit += h
    return gsup, gnhit


def write_sets(d, q, set_off, contig_name):
    paths = []
    for i in range(len(set_off) - 1):
        p = os.path.join(d, "set%d.bed" % i)
        with open(p, "w") as fh:
            for j in range(set_off[i], set_off[i + 1]):
                fh.write("%s\t%d\t%d\n" % (contig_name(int(q[0][j])), q[1][j], q[2][j]))
        paths.append(p)
    return paths


def synth(d, nfiles, per_file, nq, genome, seed=7):
    """(database path, regions) from libigd_synth (genome 0: the hg38 contigs of the benchmark database, 1: the small genome):
    gType 1, tiles of 2^14 bp, regions of 100 .. 1999 bp in position order"""
    S = N.synth()
    path = os.path.join(d, "probe_%dx%d.igd" % (nfiles, per_file))
    if S.igd_synth_db(path.encode(), nfiles, per_file, seed, 14, genome, 0, 100, 1999, 0, 1) != 0:
        raise SystemExit("igd_synth_db failed")
    q = [np.zeros(nq, np.int32) for _ in range(3)]
    got = S.igd_synth_queries(nq, seed + 1, genome, 100, 1999, 1, 0, 0, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data)
    return path, [a[:got] for a in q]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=1000000)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        if a.host:
            nfiles, nq = 260, min(a.regions, 4000)
            path, q = synth(d, nfiles, 400, nq, 1)
        else:
            nfiles, nq = 1900, a.regions
            path, q = synth(d, nfiles, 26316, nq, 0)
        nq = len(q[1])
        set_off = (np.arange(a.sets + 1, dtype=np.int64) * nq) // a.sets
        g = three_facets(nfiles)
        dense = g.dense()
        out = dict(regions=nq, sets=a.sets, nfiles=nfiles, ngroups=g.ngroups, route="host" if a.host else "engine")
        if a.host:
            L = N.cli()
            h = igd_amd.database._HostDb(path, "probe")
            nW = (nfiles + 31) // 32

            def rows(ichr, qs, qe):
                bits = np.zeros((len(qs), nW), np.uint32)
                assert L.igdc_membership_host(h.core, h.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), N.IGD_HIP_NO_VALUE_FILTER,
                                              N.IGD_HIP_RULE_NEST, bits.ctypes.data, None, C.byref(C.c_int64(0))) == 0
                return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :nfiles].astype(bool)
            t0 = time.perf_counter()
            want = old_route(rows, nfiles, q, set_off, dense)
            out["membership_numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
            h.close()
            t0 = time.perf_counter()
            parts = [igd_amd.group_support_host(path, *(x[set_off[i]:set_off[i + 1]] for x in q), g) for i in range(a.sets)]
            out["group_support_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
            got = (np.array([p[0] for p in parts]), np.array([p[1] for p in parts]))
        else:
            with igd_amd.Database(path) as db:
                paths = write_sets(d, q, set_off, lambda c: db.contig_names[c])
                db.group_support_files(paths[:1], g)                                       # (first launch, workspaces)
                t0 = time.perf_counter()
                got = db.group_support_files(paths, g)
                out["group_support_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                sets = db._read_sets(paths)
                t0 = time.perf_counter()
                want = old_route(lambda c, s, e: db.unpack_membership(db.membership(c, s, e)[0], nfiles), nfiles, sets[:3], sets[3], dense)
                out["membership_numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "the two routes differ"
        assert want[0].any(), "nothing was counted"
        out["equal"] = True
        out["group_regions"] = int(want[0].sum())
        print(json.dumps(out))


if __name__ == "__main__":
    main()
