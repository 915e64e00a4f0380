"""The literal reference of the minimum overlap per pair (include/igd_hip.h: igd_hip_min_overlap), and the fixtures its tests share.

Reference.  Oracle.enumerate lists, per query, the (idx, start, end) of every record the plain search counts under rule NEST
without a value filter.  `pairs()` keeps those lists; `counts()` applies

    ov = min(qe, end) - max(qs, start)
    ov >= max(bp, 1)  and  ov * 10^6 >= (qe - qs) * query_ppm  and  ov * 10^6 >= (end - start) * record_ppm

in integers (int64: every product is below 2^31 * 10^6 < 2^63; `qualifies()` is the same test in Python integers and
test_minoverlap_host.py holds the two against each other) and counts pairs, regions per file and regions with any pair, per
set.  For a value filter the values are looked up from the fixture's own records: every record of a file has a distinct
(start, end) (`Fixture.values`), so (idx, start, end) names one record.  Nothing here comes from the code under test.

Fixtures.  Each is a small .igd written by helpers.write_igd_numpy, a query list and a threshold that CUTS: `assert_cuts`
demands, on the reference alone, that among the unthresholded pairs at least a fifth qualify and at least a fifth do not, and
the same for the (region, file) incidences."""
import os

import numpy as np

from helpers import write_igd_numpy

PPM = 1000000


def qualifies(t, qs, qe, start, end):
    """the predicate in Python integers; t = (bp, query_ppm, record_ppm), all zero = inactive (every listed pair counts)"""
    bp, pq, pr = (int(x) for x in t)
    if not (bp or pq or pr):
        return True
    qs, qe, start, end = int(qs), int(qe), int(start), int(end)
    ov = min(qe, end) - max(qs, start)
    return ov >= max(bp, 1) and ov * PPM >= (qe - qs) * pq and ov * PPM >= (end - start) * pr


def pairs(orc, ichr, qs, qe):
    """(qno, idx, start, end) int64 arrays: the plain search's pairs under rule NEST, idx within the database's files"""
    qoff, rec = orc.enumerate(ichr, qs, qe)
    qno = np.repeat(np.arange(len(qs), dtype=np.int64), np.diff(qoff))
    rec = rec.astype(np.int64)
    ok = (rec[:, 0] >= 0) & (rec[:, 0] < orc.nfiles)
    return qno[ok], rec[ok, 0], rec[ok, 1], rec[ok, 2]


def keep(t, p, qs, qe, v=None, values=None):
    """bool per pair of `p`: passes the threshold t and, for v, the value filter (values: {(idx, start, end): value})"""
    qno, idx, s, e = p
    a, b = np.asarray(qs, np.int64)[qno], np.asarray(qe, np.int64)[qno]
    k = np.ones(len(qno), bool)
    bp, pq, pr = (int(x) for x in t)
    if bp or pq or pr:
        ov = np.minimum(b, e) - np.maximum(a, s)
        k = (ov >= max(bp, 1)) & (ov * PPM >= (b - a) * pq) & (ov * PPM >= (e - s) * pr)
    if v is not None:
        k &= np.array([values[(int(i), int(x), int(y))] >= v for i, x, y in zip(idx, s, e)], bool).reshape(len(idx))
    return k


def counts(nfiles, p, k, off):
    """(hits [nsets, nfiles], totals, support [nsets, nfiles], nhit) of the pairs p[k]; set j = queries [off[j], off[j + 1])"""
    off = np.asarray(off, np.int64)
    nsets = len(off) - 1
    qno, idx = p[0][k], p[1][k]
    st = np.searchsorted(off, qno, side="right") - 1
    hits = np.bincount(st * nfiles + idx, minlength=nsets * nfiles).reshape(nsets, nfiles).astype(np.int64)
    inc = np.unique(qno * nfiles + idx)                                   # (region, file) incidences
    iq = inc // nfiles
    sup = np.bincount((np.searchsorted(off, iq, side="right") - 1) * nfiles + inc % nfiles,
                      minlength=nsets * nfiles).reshape(nsets, nfiles).astype(np.int64)
    hq = np.unique(qno)
    nhit = np.bincount(np.searchsorted(off, hq, side="right") - 1, minlength=nsets).astype(np.int64)
    return hits, hits.sum(axis=1), sup, nhit


def assert_cuts(nfiles, p, k):
    """the threshold cuts: of the plain pairs, and of the plain (region, file) incidences, >= 1/5 stay and >= 1/5 go"""
    n, m = len(k), int(k.sum())
    assert n >= 20 and 5 * m >= n and 5 * (n - m) >= n, "pairs: %d of %d qualify" % (m, n)
    a = len(np.unique(p[0] * nfiles + p[1]))
    b = len(np.unique(p[0][k] * nfiles + p[1][k]))
    assert 5 * b >= a and 5 * (a - b) >= a, "incidences: %d of %d stay" % (b, a)
    return m, n, b, a


class Fixture:
    """path of the .igd, its records per file, the queries, the sets and the thresholds that cut on it"""

    def __init__(self, d, name, nbp, gtype, files, queries, off, thresholds, ctgs=None):
        self.path = os.path.join(d, name + ".igd")
        self.name, self.nbp, self.gtype, self.nfiles = name, nbp, gtype, len(files)
        for f, recs in enumerate(files):
            seen = set((c, s, e) for c, s, e, _ in recs)
            assert len(seen) == len(recs), "file %d of %s repeats a (start, end)" % (f, name)
        self.ctgs = write_igd_numpy(self.path, files, nbp=nbp, gtype=gtype, contig_order=ctgs)
        # (idx, start, end) -> value; no two records of a file share (start, end), on whichever contig they lie
        self.values = {}
        for f, recs in enumerate(files):
            for _, s, e, v in recs:
                assert (f, s, e) not in self.values, "value lookup ambiguous in " + name
                self.values[(f, s, e)] = v
        self.ichr, self.qs, self.qe = (np.asarray(a, np.int32) for a in queries)
        self.off = np.asarray(off, np.int64)
        self.thresholds = thresholds


def _short_records(rng, nfiles, ctg, base, width, n, used, lo=20, hi=600):
    """n records of one tile, none crossing its end, (start, end) distinct within a file and across the fixture"""
    out = []
    while len(out) < n:
        s = base + rng.randrange(0, width - hi - 1)
        e = s + rng.randint(lo, hi)
        f = rng.randrange(nfiles) if rng.random() < 0.8 else rng.choice([0, nfiles - 1])
        if (s, e) in used:
            continue
        used.add((s, e))
        out.append((f, (ctg, s, e, rng.randint(0, 1000))))
    return out


def _queries_from(rng, recs, ctg_id, n):
    """queries built around records: equal, inside, around, shifted by a part of the length, plus short strays"""
    ic, qs, qe = [], [], []
    for _ in range(n):
        _, (_, s, e, _) = rng.choice(recs)
        L = e - s
        kind = rng.randrange(6)
        if kind == 0:
            a, b = s, e
        elif kind == 1:
            a = s + rng.randint(0, L // 3)
            b = e - rng.randint(0, L // 3)
        elif kind == 2:
            a, b = s - rng.randint(0, L // 2), e + rng.randint(0, L // 2)
        elif kind == 3:
            sh = rng.randint(1, L)
            a, b = s + sh, e + sh
        elif kind == 4:
            sh = rng.randint(1, L)
            a, b = s - sh, e - sh
        else:
            a = s + rng.randint(-40, L)
            b = a + rng.randint(1, 120)
        a = max(a, 0)
        ic.append(ctg_id); qs.append(a); qe.append(max(b, a + 1))
    return ic, qs, qe


T_BP = (120, 0, 0)
T_HALF = (0, 500000, 500000)
T_QUERY = (0, 500000, 0)
T_RECORD = (0, 0, 500000)
T_MIX = (30, 250000, 400000)
T_Q_INSIDE = (0, PPM, 0)
T_R_INSIDE = (0, 0, PPM)


def tiles_fixture(rng, d, name="tl", gtype=1, nfiles=5, set_sizes=(0, 1, 700, 64)):
    """chr1: tiles of 1, 127, 128, 129 and 257 records (none crossing a tile's end) -- one step of 64 x 2 with a tail, exactly
    one iteration, one iteration and one record, two iterations and one record; chr2: long records over three and more tiles,
    each copied into every tile it touches, under queries over three tiles.  Queries are built around the records."""
    nbp = 1 << 14
    used = set()
    recs = []
    for t, n in enumerate((1, 127, 128, 129, 257)):
        recs += _short_records(rng, nfiles, "chr1", t * nbp, nbp, n, used)
    longs = []
    for i in range(8):                                            # chr2: records of 2.2 to 4 tiles, staggered
        s = 3000 + i * 6100 + rng.randrange(0, 500)
        e = s + rng.randint(2 * nbp + 3000, 4 * nbp)
        if (s, e) in used:
            continue
        used.add((s, e))
        longs.append((rng.randrange(nfiles), ("chr2", s, e, rng.randint(0, 1000))))
    longs += [(f, ("chr2",) + r[1:]) for f, r in _short_records(rng, nfiles, "chr2", 2 * nbp, nbp, 40, used)]
    files = [[] for _ in range(nfiles)]
    for f, r in recs + longs:
        files[f].append(r)
    nq = sum(set_sizes)
    n1 = nq * 7 // 8
    q1 = _queries_from(rng, recs, 0, n1)
    ic, qs, qe = list(q1[0]), list(q1[1]), list(q1[2])
    for _ in range(nq - n1):                                      # chr2: queries over three tiles and more
        a = rng.randrange(0, 3 * nbp)
        ic.append(1); qs.append(a); qe.append(a + rng.randint(2 * nbp + 1, 5 * nbp))
    order = list(range(nq))
    rng.shuffle(order)
    q = [np.array(x)[order] for x in (ic, qs, qe)]
    off = np.concatenate([[0], np.cumsum(set_sizes)])
    return Fixture(d, name, nbp, gtype, files, q, off, [T_BP, T_HALF, T_QUERY, T_MIX], ctgs=["chr1", "chr2"])


def wide_fixture(rng, d, nfiles, name=None, n_records=500, nq=600):
    """few records over many files (the first and the last file among them), two tiles: the counters' and bitmaps' edges"""
    nbp = 1 << 14
    used = set()
    n_records = min(n_records, 60 * nfiles)                       # (one file: few records, or nearly every region keeps some pair)
    recs = _short_records(rng, nfiles, "chr1", 0, nbp, n_records // 2, used) + _short_records(rng, nfiles, "chr1", nbp, nbp, n_records // 2, used)
    files = [[] for _ in range(nfiles)]
    for f, r in recs:
        files[f].append(r)
    q = _queries_from(rng, recs, 0, nq)
    return Fixture(d, name or "w%d" % nfiles, nbp, 1, files, q, [0, nq // 3, nq], [T_BP, T_HALF], ctgs=["chr1"])


def big_fixture(d, name="big"):
    """coordinates and record lengths near 2^31 - 1 (tiles of 2^15 bp): (end - start) * record_ppm and ov * 10^6 pass 2^32 many
    times over, and the decisions turn on the high bits of the products.  One query spans half the contig (ov up to 2^30); the
    others are at most 64 tiles long, so that a walk stays short, and lie at the contig's ends and at the long records' ends."""
    nbp = 1 << 15
    M = 2 ** 31 - 1
    G, H = 2 ** 30, 2 ** 29
    files = [[("chr1", 1000, M - 647, 10), ("chr1", G, M - 7, 600), ("chr1", M - 5000, M - 1000, 900)],
             [("chr1", 5, G + 5, 700), ("chr1", M - 3000, M, 20), ("chr1", 4096, 4096 + G + H, 450)]]
    qs, qe = [G], [M]
    for s, e in ((M - 6000, M - 1), (M - 2999, M), (G - 10, G + 10), (G - 2 ** 20, G + 2 ** 20), (0, 2 ** 20), (4096, 4096 + 2 ** 21),
                 (M - 2 ** 21, M - 1000), (G + H - 2 ** 20, G + H + 2 ** 20 + 4096), (M - 4000, M - 2000), (G + 5 - 300000, G + 5 + 300000),
                 (M - 900000, M - 7), (1000, 1000 + 2 ** 21)):
        for da, db in ((0, 0), (1, 0), (0, -1), (7, -9)):
            qs.append(s + da); qe.append(e + db)
    q = (np.zeros(len(qs), np.int32), qs, qe)
    return Fixture(d, name, nbp, 1, files, q, [0, len(qs)], [(0, 0, 1000), (0, 500000, 300), (0, 0, 2000)], ctgs=["chr1"])


def boundary_fixture(d, name="bd"):
    """isolated records of 1 000 bp, 100 000 bp apart, and hand-made queries: `cases` lists (query number, threshold, counted)
    for the pairs whose  ov * 10^6 == len * ppm  exactly, the same pairs one bp short, and ppm = 10^6 per term and for both"""
    nbp = 1 << 14
    S = [100000 * (i + 1) for i in range(12)]
    files = [[("chr1", s, s + 1000, 300 + 400 * (i % 2)) for i, s in enumerate(S[0::2])],
             [("chr1", s, s + 1000, 300 + 400 * (i % 2)) for i, s in enumerate(S[1::2])]]
    Q = []
    cases = []

    def q(a, b):
        Q.append((a, b))
        return len(Q) - 1
    s = S[0]
    k = q(s + 900, s + 1100)                                      # ov 100 of a query of 200: exactly one half
    cases += [(k, (0, 500000, 0), 1), (k, (0, 500001, 0), 0), (k, (0, 0, 100000), 1), (k, (0, 0, 100001), 0), (k, (100, 0, 0), 1),
              (k, (101, 0, 0), 0)]
    k = q(s + 901, s + 1101)                                      # one bp less
    cases += [(k, (0, 500000, 0), 0), (k, (0, 0, 100000), 0), (k, (99, 495000, 99000), 1), (k, (0, 495001, 0), 0)]
    s = S[1]
    k = q(s + 998, s + 1001)                                      # ov 2 of 3: 666 666 ppm qualifies, 666 667 does not
    cases += [(k, (0, 666666, 0), 1), (k, (0, 666667, 0), 0), (k, (0, 0, 2000), 1), (k, (0, 0, 2001), 0)]
    k = q(s + 999, s + 1002)                                      # ov 1 of 3: ceil(3 * 333 334 / 10^6) = 2
    cases += [(k, (0, 333333, 0), 1), (k, (0, 333334, 0), 0), (k, (1, 0, 0), 1), (k, (2, 0, 0), 0)]
    s = S[2]
    inside, equal, around, left = q(s + 10, s + 990), q(s, s + 1000), q(s - 10, s + 1010), q(s - 1, s + 999)
    for k, a, b, c in ((inside, 1, 0, 0), (equal, 1, 1, 1), (around, 0, 1, 0), (left, 0, 0, 0)):
        cases += [(k, T_Q_INSIDE, a), (k, T_R_INSIDE, b), (k, (0, PPM, PPM), c), (k, (0, 0, 0), 1)]
    s = S[3]
    zero, inverted = q(s + 500, s + 500), q(s + 600, s + 400)     # counted by the plain predicate, never under a threshold
    for k in (zero, inverted):
        cases += [(k, (0, 0, 0), 1), (k, (1, 0, 0), 0), (k, (0, 1, 0), 0), (k, (0, 0, 1), 0)]
    for s in S[4:]:                                               # filler so that the thresholds of `thresholds` cut
        for a, b in ((s, s + 1000), (s + 100, s + 900), (s - 300, s + 200), (s + 800, s + 1300), (s + 960, s + 1400), (s - 50, s + 30)):
            q(a, b)
    qs, qe = [a for a, _ in Q], [b for _, b in Q]
    fx = Fixture(d, name, nbp, 1, files, (np.zeros(len(Q), np.int32), qs, qe), [0, len(Q)], [(100, 0, 0), (0, 400000, 0), (0, 0, 150000)],
                 ctgs=["chr1"])
    fx.cases = cases
    return fx
