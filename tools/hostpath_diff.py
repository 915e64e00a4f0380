#!/usr/bin/env python3
"""Differential record of the host route (igd_amd/csrc/igd_hostpath.c) between two builds.

    python tools/hostpath_diff.py OTHER/igd_amd/lib/libigd.so [THIS/igd_amd/lib/libigd.so]

Every exported igdc_*_host* entry, igdc_merge_host, igdc_bitrows_gram_host and igdc_permute_regions_host(_ws) is driven through
both libraries with the same inputs; every return code and every output array (filled with the same pattern before the call, one
word longer than the entry may write) is compared byte for byte.  Inputs: the eight random databases of tests/test_gpu_parity.py
and one without files; 13 000 random regions (short, many-tile, inverted, zero-length, out of range, unknown contigs: enough for
seven threads); IGD_HOST_THREADS 1, 2 and 7; both rules, a value filter, an active minimum overlap, windows 0 and > 0, both
flank measures, the four map ops, the three placements with and without a workspace, empty sets at the start, in the middle and
at the end, nsets = 0, nq = 0, refused arguments, and the set entries once more under a lowered IGD_HOST_ROW_BYTES (a library
that does not know the variable runs its usual one chunk: the answers must not depend on the seams).  Prints the number of calls
compared and of differences; exit status 1 if there is a difference.  Needs no GPU."""
import ctypes as C
import os
import random
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import short_tmpdir, write_igd_numpy  # noqa: E402
from test_gpu_parity import CASES, _random_db, _random_queries  # noqa: E402

NOV = -2 ** 31
DB, MAP, WS = "db", "map", "ws"
i32, i64, u64 = C.c_int32, C.c_int64, C.c_uint64


class Out:
    """an output array: n words of dtype the entry may write, + 1 it may not; filled with 3 (some entries ADD to theirs)"""
    def __init__(self, dtype, n):
        self.dtype, self.n = dtype, int(n) + 1


class Side:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        for f in ("igdc_open", "igdc_map_open", "igdc_index_path"):
            getattr(self.lib, f).restype = C.c_void_p
        self.h = {}

    def open(self, path):
        L = self.lib
        db = L.igdc_open(path.encode())
        assert db, path
        tsv = L.igdc_index_path(path.encode())
        L.igdc_load_index(C.c_void_p(db), C.c_void_p(tsv))
        fd = os.open(path, os.O_RDONLY)
        m = L.igdc_map_open(C.c_void_p(db), fd)
        os.close(fd)
        assert m, path
        self.h = {DB: db, MAP: m, WS: None}

    def workspace(self, ichr, a, b, ctg_len):
        ws = C.c_void_p()
        rc = self.lib.igdc_workspace_build(ptr(ichr), ptr(a), ptr(b), i64(len(a)), ptr(ctg_len), i32(len(ctg_len)), C.byref(ws))
        assert rc == 0
        self.h[WS] = ws.value

    def close(self):
        if self.h.get(WS):
            self.lib.igdc_workspace_free(C.c_void_p(self.h[WS]))
        self.lib.igdc_map_close(C.c_void_p(self.h[MAP]))
        self.lib.igdc_close(C.c_void_p(self.h[DB]))


def ptr(a):
    return C.c_void_p(None if a is None else a.ctypes.data)


class Record:
    def __init__(self, sides):
        self.sides, self.calls, self.answered, self.diffs, self.tally = sides, 0, 0, [], {}

    def call(self, tag, name, *args):
        res = []
        for s in self.sides:
            argv, outs = [], []
            for a in args:
                if isinstance(a, str):
                    argv.append(C.c_void_p(s.h[a]))
                elif isinstance(a, Out):
                    outs.append(np.full(a.n, 3, a.dtype))
                    argv.append(ptr(outs[-1]))
                elif a is None or isinstance(a, np.ndarray):
                    argv.append(ptr(a))
                else:
                    argv.append(a)
            rc = getattr(s.lib, name)(*argv)
            res.append((rc, [o.tobytes() for o in outs]))
        self.calls += 1
        self.answered += res[0][0] == 0
        t = self.tally.setdefault(name, [0, 0])
        t[0] += res[0][0] == 0
        t[1] += 1
        if res[0] != res[1]:
            self.diffs.append("%s %s: rc %d / %d%s" % (tag, name, res[0][0], res[1][0], ", outputs differ" if res[0][1] != res[1][1] else ""))

    def enumerate(self, tag, ichr, qs, qe):
        """igdc_enumerate_host allocates its list: offsets, total and the list's bytes are compared"""
        res = []
        for s in self.sides:
            qoff = np.full(len(qs) + 2, 3, np.int64)
            out, tot = C.c_void_p(), i64(3)
            rc = s.lib.igdc_enumerate_host(C.c_void_p(s.h[DB]), C.c_void_p(s.h[MAP]), ptr(ichr), ptr(qs), ptr(qe), i64(len(qs)), ptr(qoff),
                                           C.byref(out), C.byref(tot))
            rec = C.string_at(out.value, 16 * tot.value) if rc == 0 and out.value else b""
            if out.value:
                libc.free(out)
            res.append((rc, tot.value, qoff.tobytes(), rec))
        self.calls += 1
        self.answered += res[0][0] == 0
        if res[0] != res[1]:
            self.diffs.append("%s igdc_enumerate_host" % tag)


libc = C.CDLL(None)
libc.free.argtypes = [C.c_void_p]


def drive(R, rng, nctg, nf, nbp, span, gtype, row_bytes_case):
    tag = "nf%d nbp%d T%s" % (nf, nbp, os.environ["IGD_HOST_THREADS"])
    nC, nW = nf + 1, (nf + 31) // 32
    ichr, qs, qe = _random_queries(rng, list(range(nctg)), nbp, span, 13000)
    u_ichr, u_qs, u_qe = _random_queries(rng, list(range(nctg)), nbp, span, 13000)
    nq = len(qs)
    set_off = np.array([0, 0, 4000, 4000, 4000, 9000, 13000, 13000], np.int64)      # empty sets: first, two in the middle, last
    nsets = len(set_off) - 1
    q3, e3 = (ichr, qs, qe), (None, None, None)
    mo = np.array([10, 200000, 100000], np.int32)
    mo_off = np.zeros(3, np.int32)
    rules = [(NOV, 0), (NOV, 1), (500, 1), (500, 0)]

    for v, rule in rules:
        a = (DB, MAP) + q3 + (i64(nq), i32(v), i32(rule))
        R.call(tag, "igdc_search_host", *a, Out(np.int64, nf), Out(np.int64, 1))
        R.call(tag, "igdc_support_host", *a, Out(np.int64, nf), Out(np.int64, 1))
        R.call(tag, "igdc_coverage_host", *a, Out(np.int64, nf), Out(np.int64, 1))
        R.call(tag, "igdc_membership_host", *a, Out(np.uint32, nq * nW), Out(np.int32, nq), Out(np.int64, 1))
        R.call(tag, "igdc_cooccur_host", *a, Out(np.int64, nf * nf), Out(np.int64, 1))
        for o in (mo, mo_off, None):
            R.call(tag, "igdc_search_host_ov", *a, Out(np.int64, nf), Out(np.int64, 1), o)
            R.call(tag, "igdc_support_host_ov", *a, Out(np.int64, nf), Out(np.int64, 1), o)
        R.call(tag, "igdc_dataset_bp_host", DB, MAP, i32(v), i32(rule), Out(np.int64, nC))
        R.call(tag, "igdc_jaccard_host", DB, MAP, *q3, set_off, i32(nsets), i32(v), i32(rule), Out(np.int64, nsets * nC), Out(np.int64, nsets),
               Out(np.int64, nC), Out(np.int64, nsets), Out(np.int64, nsets))
        R.call(tag, "igdc_enrich_restricted_host", DB, MAP, *q3, set_off, i32(nsets), u_ichr, u_qs, u_qe, i64(nq), i32(v), i32(rule),
               Out(np.int64, nsets * nf), Out(np.int64, nf), Out(np.int64, nsets), Out(np.float64, nsets * nf), Out(np.float64, nsets * nf),
               Out(np.uint32, nsets * ((nq + 31) // 32)), Out(np.int64, nsets), Out(np.int64, 1))
    R.enumerate(tag, *q3)
    R.call(tag, "igdc_search_host", DB, MAP, *q3, i64(nq), i32(NOV), i32(0), None, Out(np.int64, 1))           # refused: no hits[]
    R.call(tag, "igdc_search_host_ov", DB, MAP, *q3, i64(nq), i32(NOV), i32(0), Out(np.int64, nf), Out(np.int64, 1), np.array([-1, 0, 0], np.int32))
    R.call(tag, "igdc_search_host", DB, MAP, *e3, i64(0), i32(NOV), i32(0), Out(np.int64, nf), Out(np.int64, 1))
    R.call(tag, "igdc_membership_host", DB, MAP, *e3, i64(0), i32(NOV), i32(0), None, None, Out(np.int64, 1))
    R.call(tag, "igdc_restrict_host", *q3, set_off, i32(nsets), u_ichr, u_qs, u_qe, i64(nq), Out(np.uint32, nsets * ((nq + 31) // 32)), Out(np.int64, nsets))

    # rows per region and their per-set statistics; the set entries again under the lowered row budget
    edges = np.array([-5000, -100, 0, 1, 250, 9000], np.int32)
    bad_off = [np.array([1, 2, 3, 4, 5, 6, 7, 13000], np.int64), np.array([0, 5, 4, 4000, 4000, 9000, 13000, 13000], np.int64)]
    for window in (0, 3 * nbp + 11):
        for v in (NOV, 500):
            a = (DB, MAP) + q3 + (i64(nq), i32(window))
            s = (DB, MAP) + q3 + (set_off, i32(nsets), i32(window))
            R.call(tag, "igdc_nearest_host", *a, i32(v), Out(np.int32, nq * nf), Out(np.int32, nq))
            R.call(tag, "igdc_nearest_signed_host", *a, i32(v), Out(np.int32, nq * nf), Out(np.int32, nq))
            for measure in (0, 1):
                R.call(tag, "igdc_flank_host", *a, i32(measure), i32(v), Out(np.int32, nq * nf), Out(np.int32, nq * nf), Out(np.int32, nq), Out(np.int32, nq))
            for budget in (None, row_bytes_case):
                if budget:
                    os.environ["IGD_HOST_ROW_BYTES"] = str(budget)
                R.call(tag, "igdc_nearest_sets_host", *s, i32(v), Out(np.int64, nsets * nC), Out(np.int64, nsets * nC), Out(np.int64, nsets * nC))
                R.call(tag, "igdc_nearest_hist_host", *s, i32(v), edges, i32(len(edges)), Out(np.int64, nsets * (len(edges) + 1) * nC))
                for measure in (0, 1):
                    R.call(tag, "igdc_flank_reldist_host", *s, i32(measure), i32(v), i32(10), Out(np.int64, nsets * 10 * nC))
                os.environ.pop("IGD_HOST_ROW_BYTES", None)
    for op in (0, 1, 2, 3, 4):
        for v in (NOV, 500):
            R.call(tag, "igdc_map_host", DB, MAP, *q3, i64(nq), i32(op), i32(v), Out(np.int32, nq * nf), Out(np.int64, nq * nf))
            for budget in (None, row_bytes_case):
                if budget:
                    os.environ["IGD_HOST_ROW_BYTES"] = str(budget)
                R.call(tag, "igdc_map_sets_host", DB, MAP, *q3, set_off, i32(nsets), i32(op), i32(v), Out(np.int64, nsets * nf), Out(np.int64, nsets * nf),
                       Out(np.int64, nsets * nf))
                os.environ.pop("IGD_HOST_ROW_BYTES", None)
    for off, n in [(set_off, 0), (None, 0), (None, 3)] + [(b, nsets) for b in bad_off]:      # nsets = 0 and refused offsets
        R.call(tag, "igdc_nearest_sets_host", DB, MAP, *q3, off, i32(n), i32(5), i32(NOV), Out(np.int64, nsets * nC), None, Out(np.int64, nsets * nC))
        R.call(tag, "igdc_nearest_hist_host", DB, MAP, *q3, off, i32(n), i32(5), i32(NOV), edges, i32(len(edges)), Out(np.int64, nsets * (len(edges) + 1) * nC))
        R.call(tag, "igdc_flank_reldist_host", DB, MAP, *q3, off, i32(n), i32(5), i32(0), i32(NOV), i32(10), Out(np.int64, nsets * 10 * nC))
        R.call(tag, "igdc_map_sets_host", DB, MAP, *q3, off, i32(n), i32(0), i32(NOV), Out(np.int64, nsets * nf), Out(np.int64, nsets * nf), None)
        R.call(tag, "igdc_merge_host", DB, *q3, off, i32(n), i64(0), Out(np.int32, nq), Out(np.int32, nq), Out(np.int32, nq), Out(np.int64, nsets + 1),
               Out(np.int32, nq), Out(np.int64, nsets))
        R.call(tag, "igdc_jaccard_host", DB, MAP, *q3, off, i32(n), i32(NOV), i32(0), Out(np.int64, nsets * nC), Out(np.int64, nsets),
               Out(np.int64, nC), Out(np.int64, nsets), Out(np.int64, nsets))
        R.call(tag, "igdc_restrict_host", *q3, off, i32(n), u_ichr, u_qs, u_qe, i64(nq), Out(np.uint32, nsets * ((nq + 31) // 32)), Out(np.int64, nsets))
    R.call(tag, "igdc_nearest_host", DB, MAP, *q3, i64(nq), i32(-1), i32(NOV), Out(np.int32, nq * nf), Out(np.int32, nq))       # refused window
    R.call(tag, "igdc_nearest_sets_host", DB, MAP, *e3, set_off, i32(nsets), i32(0), i32(NOV), Out(np.int64, nsets * nC), None, None)  # regions missing
    for gap in (0, 1000, -1):
        R.call(tag, "igdc_merge_host", DB, *q3, set_off, i32(nsets), i64(gap), Out(np.int32, nq), Out(np.int32, nq), Out(np.int32, nq), Out(np.int64, nsets + 1),
               Out(np.int32, nq), Out(np.int64, nsets))

    # permutations: regions inside 0 <= s <= e <= L on the known contigs (unknown contigs stay as they are)
    L = span + 3 * nbp
    ctg_len = np.full(nctg, L, np.int32)
    n = 600
    p_ichr = ichr[:n].copy()
    p_qs = np.minimum(np.maximum(qs[:n], 0), L - 1).astype(np.int32)
    p_qe = np.minimum(p_qs + np.minimum(np.abs(qe[:n] - qs[:n]), nbp), L).astype(np.int32)
    seg_c = np.repeat(np.arange(nctg, dtype=np.int32), 2)
    seg_a = np.tile(np.array([0, L // 2 + 10], np.int32), nctg)
    seg_b = np.tile(np.array([L // 2, L], np.int32), nctg)
    inside = (p_ichr < 0) | (p_ichr >= nctg) | (p_qe <= L // 2) | (p_qs >= L // 2 + 10)
    w3 = (p_ichr[inside].copy(), p_qs[inside].copy(), p_qe[inside].copy())
    for s in R.sides:
        s.workspace(seg_c, seg_a, seg_b, ctg_len)
    nperm = 24
    Rr = nperm + 1
    for mode, ws, (a_c, a_s, a_e) in [(0, None, (p_ichr, p_qs, p_qe)), (1, None, (p_ichr, p_qs, p_qe)), (2, WS, w3), (2, None, w3), (1, WS, w3),
                                     (2, WS, (p_ichr, p_qs, p_qe)), (3, None, (p_ichr, p_qs, p_qe))]:
        k = len(a_s)
        g = (DB, MAP, a_c, a_s, a_e, i64(k), ctg_len, i32(mode), u64(0x9E3779B97F4A7C15))
        R.call(tag, "igdc_permute_regions_host_ws", a_c, a_s, a_e, i64(k), ctg_len, i32(nctg), i32(mode), u64(77), i64(3), i64(4), Out(np.int32, 4 * k),
               Out(np.int32, 4 * k), ws)
        if ws is None:
            R.call(tag, "igdc_permute_regions_host", a_c, a_s, a_e, i64(k), ctg_len, i32(nctg), i32(mode), u64(77), i64(0), i64(2), Out(np.int32, 2 * k),
                   Out(np.int32, 2 * k))
        for v, rule in ((NOV, 0), (500, 1), (NOV, 2)):
            seven = [Out(np.int64, nC) for _ in range(7)]
            R.call(tag, "igdc_permute_host_ws", *g, i64(nperm), i32(v), i32(rule), *seven, mo if rule else None, ws)
            R.call(tag, "igdc_permute_bp_host_ws", *g, i64(nperm), i32(v), i32(rule), Out(np.int64, Rr * nC), Out(np.int64, Rr), Out(np.int64, Rr),
                   Out(np.int64, 1), ws)
            if ws is None:
                R.call(tag, "igdc_permute_host", *g, i64(nperm), i32(v), i32(rule), *[Out(np.int64, nC) for _ in range(7)])
                R.call(tag, "igdc_permute_host_ov", *g, i64(nperm), i32(v), i32(rule), *[Out(np.int64, nC) for _ in range(7)], mo)
                R.call(tag, "igdc_permute_bp_host", *g, i64(nperm), i32(v), i32(rule), Out(np.int64, Rr * nC), Out(np.int64, Rr), Out(np.int64, Rr),
                       Out(np.int64, 1))
        for window in (0, 2 * nbp):
            R.call(tag, "igdc_permute_nearest_host_ws", *g, i64(nperm), i32(window), i32(NOV), Out(np.int64, Rr * nC), Out(np.int64, Rr * nC),
                   Out(np.int64, Rr * nC), ws)
            if ws is None:
                R.call(tag, "igdc_permute_nearest_host", *g, i64(nperm), i32(window), i32(500), Out(np.int64, Rr * nC), None, Out(np.int64, Rr * nC))
    g0 = (DB, MAP, p_ichr, p_qs, p_qe)
    for k, np_ in ((0, nperm), (n, 0), (n, (1 << 20) + 1)):                                  # nq = 0; refused numbers of permutations
        R.call(tag, "igdc_permute_host", *g0, i64(k), ctg_len, i32(0), u64(1), i64(np_), i32(NOV), i32(0), *[Out(np.int64, nC) for _ in range(7)])
        R.call(tag, "igdc_permute_nearest_host", *g0, i64(k), ctg_len, i32(1), u64(1), i64(np_), i32(9), i32(NOV), Out(np.int64, Rr * nC), Out(np.int64, Rr * nC),
               Out(np.int64, Rr * nC))
        R.call(tag, "igdc_permute_bp_host", *g0, i64(k), ctg_len, i32(1), u64(1), i64(np_), i32(NOV), i32(0), Out(np.int64, Rr * nC), Out(np.int64, Rr),
               Out(np.int64, Rr), Out(np.int64, 1))
    R.call(tag, "igdc_permute_host", DB, MAP, *q3, i64(nq), ctg_len, i32(0), u64(1), i64(3), i32(NOV), i32(0), *[Out(np.int64, nC) for _ in range(7)])  # regions outside L


def tables(R, rng):
    """the entries that take no database"""
    tag = "tables T%s" % os.environ["IGD_HOST_THREADS"]
    nr = np.random.RandomState(rng.randrange(1 << 30))
    for m, n, nw in ((600, 600, 64), (37, 5, 3), (0, 4, 2), (5, 7, 0)):
        a = nr.randint(0, 1 << 32, size=max(1, m * nw), dtype=np.uint64).astype(np.uint32)
        b = nr.randint(0, 1 << 32, size=max(1, n * nw), dtype=np.uint64).astype(np.uint32)
        R.call(tag, "igdc_bitrows_gram_host", a, i64(m), b, i64(n), i64(nw), Out(np.int64, m * n))
        R.call(tag, "igdc_bitrows_gram_host", a, i64(m), None, i64(0), i64(nw), Out(np.int64, m * m))
    cells = [nr.randint(0, 5000, size=400).astype(np.int64) for _ in range(4)]
    R.call(tag, "igdc_fisher_host", *cells, i64(400), Out(np.float64, 400), Out(np.float64, 400))
    sup = nr.randint(0, 50, size=20 * 30).astype(np.int64)
    pv = np.round(nr.rand(20 * 30) * 8, 1)
    orr = np.round(nr.rand(20 * 30) * 4, 1)
    R.call(tag, "igdc_rank_host", sup, pv, orr, i64(20), i64(30), Out(np.float64, 600), Out(np.int32, 600), Out(np.int32, 600), Out(np.int32, 600),
           Out(np.int32, 600), Out(np.float64, 600))


def main():
    other = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "igd_amd", "lib", "libigd.so")
    R = Record([Side(other), Side(this)])
    d = short_tmpdir("ighd")
    try:
        for threads in ("1", "2", "7"):
            os.environ["IGD_HOST_THREADS"] = threads
            for case in range(len(CASES) + 1):
                rng = random.Random(9100 + case)
                if case < len(CASES):
                    nbp, gtype, nfiles, nctg, span_tiles, dens, hot = CASES[case]
                    path, _, span = _random_db(rng, d, "h%d" % case, nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
                else:                                                       # a database without files
                    nbp, gtype, nfiles, nctg, span = 4096, 1, 0, 0, 4096 * 10
                    path = os.path.join(d, "empty.igd")
                    write_igd_numpy(path, [], nbp=nbp, gtype=gtype)
                for s in R.sides:
                    s.open(path)
                drive(R, rng, nctg, nfiles, nbp, span, gtype, 4 * max(1, nfiles) * 1000)
                for s in R.sides:
                    s.close()
            tables(R, random.Random(5))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    for name in sorted(R.tally):
        print("%-34s %5d calls, %5d answered with 0" % (name, R.tally[name][1], R.tally[name][0]))
    for line in R.diffs[:40]:
        print("DIFFERENT", line)
    print("hostpath_diff: %d calls compared (%d answered with 0, the rest refused), %d differences" % (R.calls, R.answered, len(R.diffs)))
    return 1 if R.diffs else 0


if __name__ == "__main__":
    sys.exit(main())
