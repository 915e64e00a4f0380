"""The nearest record per dataset within a window, restated in numpy (include/igd_hip.h has the definitions), and the fixtures
of tests/test_nearest_host.py, tests/test_nearest_cli.py and tests/test_gpu_nearest.py.  A plain module: no pytest hooks.

    d = 0 if s < qe and e > qs else max(s - qe, qs - e) + 1          within the window iff d <= W
    dist[q][f] = min d over the records of file f within the window [with value >= v], -1 when there is none
    dmin[q]    = min over the files of the dist[q][f] that are not -1, else -1

The reference is a broadcast over the INTERVAL LISTS THE TEST ITSELF WROTE with write_igd_numpy -- never over anything read
back from the .igd, so tiles, copies of records and the prefix skip do not exist here."""
import os

import numpy as np

from helpers import write_igd_numpy

MAX_WINDOW = 1 << 30
NOV = -2 ** 31                      # IGD_HIP_NO_VALUE_FILTER
NONE = np.int64(1) << 40            # "no record" while minimising


def windows(nbp):
    """the W list of the issue"""
    return [0, 1, nbp - 1, nbp, 3 * nbp + 5, MAX_WINDOW]


# ---- databases that keep their lists ---------------------------------------------------------------------------------------
class ListDb:
    """path of the .igd, its interval lists (one per file: (chrom, start, end, value)), contig names in the file's order"""

    def __init__(self, d, name, files, nbp, gtype, contig_order=None):
        self.path = os.path.join(d, name + ".igd")
        self.files, self.nbp, self.gtype = files, nbp, gtype
        self.ctgs = write_igd_numpy(self.path, files, nbp=nbp, gtype=gtype, contig_order=contig_order)
        self.nfiles = len(files)
        self.names = ["f%04d.bed" % i for i in range(self.nfiles)]
        self._by_ctg = None

    def by_contig(self):
        """per contig number: (idx, start, end, value) int64 arrays of the records the writer kept (start < end), ordered by file"""
        if self._by_ctg is None:
            rows = [(self.ctgs.index(c), f, s, e, v) for f, recs in enumerate(self.files) for (c, s, e, v) in recs if s < e]
            a = np.array(rows, np.int64).reshape(-1, 5)
            self._by_ctg = {}
            for c in range(len(self.ctgs)):
                r = a[a[:, 0] == c]
                r = r[np.argsort(r[:, 1], kind="stable")]
                self._by_ctg[c] = (r[:, 1], r[:, 2], r[:, 3], r[:, 4])
        return self._by_ctg


def clustered_lists(rng, nbp, nfiles, nctg, span_tiles, min_value=0):
    """the shape of test_support_host.clustered_db: clusters of neighbouring records, long records over four and six tiles, two
    long ones that overlap each other, scattered short ones -- as lists"""
    ctgs = ["chr%d" % (i + 1) for i in range(nctg)]
    span = nbp * span_tiles
    files = []
    for f in range(nfiles):
        rows = []
        for c in ctgs:
            for _ in range(3):
                s = rng.randrange(0, span - 2000)
                for k in range(rng.randint(2, 5)):
                    rows.append((c, s + 90 * k, s + 90 * k + rng.randint(20, 400), rng.randint(min_value, 1000)))
            for L in (3 * nbp + 7, 5 * nbp + 1):
                s = rng.randrange(0, span)
                rows.append((c, s, s + L, rng.randint(min_value, 1000)))
            s = rng.randrange(nbp, span)
            rows.append((c, s, s + 3 * nbp, rng.randint(min_value, 1000)))
            rows.append((c, s + nbp // 2, s + 4 * nbp, rng.randint(min_value, 1000)))
            for _ in range(6):
                s = rng.randrange(0, span)
                rows.append((c, s, s + rng.choice([1, 5, nbp // 3]), rng.randint(min_value, 1000)))
        files.append(rows)
    return files, span


def sparse_lists(rng, nbp, nfiles, per_file, span):
    """one contig, `per_file` short records per file scattered over `span`: databases of many files stay small"""
    return [[("chr1", s, s + rng.randint(1, 300), rng.choice([0, 400, 1000]))
             for s in (rng.randrange(0, span) for _ in range(per_file))] for _ in range(nfiles)]


def mixed_regions(rng, nctg, nbp, span, n):
    """the style of test_support_host.mixed_queries -- unknown contigs, zero-length and inverted regions, short and many-tile
    ones, every fifth one repeated -- and regions that start past the contig's last tile or at negative starts"""
    ichr = np.array([rng.choice(list(range(nctg)) + [-1, 99]) for _ in range(n)], np.int32)
    qs = np.array([rng.choice([rng.randrange(0, span + 3 * nbp), rng.randrange(0, span + 3 * nbp), span + rng.randrange(7 * nbp, 40 * nbp),
                               -rng.randrange(1, 3 * nbp)]) for _ in range(n)], np.int64)
    ln = np.array([rng.choice([0, 1, 200, 700, nbp, 2 * nbp + 5, 7 * nbp + 3, rng.randint(1, 3 * nbp), -rng.randint(1, 50)])
                   for _ in range(n)], np.int64)
    qe = qs + ln
    for i in range(5, n, 5):
        ichr[i], qs[i], qe[i] = ichr[i - 1], qs[i - 1], qe[i - 1]
    return ichr, qs.astype(np.int32), qe.astype(np.int32)


# ---- the definition ---------------------------------------------------------------------------------------------------------
def pair_dist(qs, qe, s, e):
    """d of every (region, record) pair: int64[nq, nrec]"""
    qs, qe = np.asarray(qs, np.int64)[:, None], np.asarray(qe, np.int64)[:, None]
    s, e = np.asarray(s, np.int64)[None, :], np.asarray(e, np.int64)[None, :]
    return np.where((s < qe) & (e > qs), 0, np.maximum(s - qe, qs - e) + 1)


def ref_rows(db, ichr, qs, qe, window, v=None, block=256):
    """(dist int32[nq, nfiles], dmin int32[nq]) from db's lists.  v: a value filter (None: none); it counts on gType 1 only."""
    ichr = np.asarray(ichr)
    nq, nf = len(qs), db.nfiles
    dist = np.full((nq, nf), -1, np.int32)
    use_v = v is not None and v != NOV and db.gtype == 1
    for c, (idx, s, e, val) in db.by_contig().items():
        if use_v:
            keep = val >= v
            idx, s, e = idx[keep], s[keep], e[keep]
        if len(idx) == 0:
            continue
        order = np.argsort(idx, kind="stable")
        idx, s, e = idx[order], s[order], e[order]
        present, starts = np.unique(idx, return_index=True)
        sel = np.flatnonzero(ichr == c)
        for b0 in range(0, len(sel), block):
            q = sel[b0:b0 + block]
            d = pair_dist(qs[q], qe[q], s, e)
            d = np.where(d <= window, d, NONE)
            m = np.minimum.reduceat(d, starts, axis=1)
            out = np.full((len(q), nf), -1, np.int64)
            out[:, present] = np.where(m < NONE, m, -1)
            dist[q] = out
    return dist, row_min(dist)


def row_min(dist):
    big = np.where(dist >= 0, dist.astype(np.int64), NONE)
    m = big.min(axis=1, initial=NONE)
    return np.where(m < NONE, m, -1).astype(np.int32)


def ref_sets(dist, dmin, set_off):
    """(n_within, n_overlap, sum_dist), each int64[nsets, nfiles + 1]: sums over the rows, the last column from dmin"""
    full = np.concatenate([dist.astype(np.int64), dmin.astype(np.int64)[:, None]], axis=1)
    nsets = len(set_off) - 1
    out = [np.zeros((nsets, full.shape[1]), np.int64) for _ in range(3)]
    for k in range(nsets):
        r = full[int(set_off[k]):int(set_off[k + 1])]
        out[0][k] = (r >= 0).sum(axis=0)
        out[1][k] = (r == 0).sum(axis=0)
        out[2][k] = np.where(r >= 0, r, 0).sum(axis=0)
    return out


def mean_text(n_within, sum_dist):
    return "%.2f" % (float(sum_dist) / float(n_within)) if n_within > 0 else "NA"


def table_text(names, n_within, n_overlap, sum_dist, window, nq):
    """the block `igd search db -q F -N window` prints for one set, from its three rows"""
    nf = len(names)
    out = ["index\tn_within\tn_overlap\tmean_dist\tFile\n"]
    for i in range(nf):
        out.append("%d\t%d\t%d\t%s\t%s\n" % (i, n_within[i], n_overlap[i], mean_text(n_within[i], sum_dist[i]), names[i]))
    out.append("Regions with a dataset within %d bp: %d of %d; overlapping: %d; mean distance %s\n"
               % (window, n_within[nf], nq, n_overlap[nf], mean_text(n_within[nf], sum_dist[nf])))
    return "".join(out)


# ---- placed cases -----------------------------------------------------------------------------------------------------------
TOP = 2 ** 31 - 1


def placed_db(d, nbp=1 << 14, name="placed"):
    """One database for the placed cases of the issue; chrE holds the coordinates at 2^31 - 1 (its tiles run up there)."""
    files = [
        # f0: a book-ended pair (region [1000, 2000) in placed_regions), and a record over five tiles from 0
        [("chrA", 2000, 2500, 900), ("chrB", 0, 5 * nbp, 900)],
        # f1: two records on either side of region [50000, 50100): the nearer one fails -v 500, the farther one passes
        [("chrA", 49900, 49990, 100), ("chrA", 50400, 50500, 800)],
        # f2: ties -- two records at the same distance on both sides of [70000, 70010), and two equal records
        [("chrA", 69900, 69950, 700), ("chrA", 70060, 70100, 700), ("chrA", 90000, 90010, 1), ("chrA", 90000, 90010, 1000)],
        # f3: the contig's first and last record: windows that reach before 0 and past the last tile
        [("chrA", 5, 10, 600), ("chrA", 8 * nbp - 30, 8 * nbp - 20, 600)],
        # f4: the top of int32
        [("chrE", TOP - 100, TOP, 900), ("chrE", TOP - 5 * nbp, TOP - 5 * nbp + 10, 900)],
    ]
    return ListDb(d, name, files, nbp, 1, contig_order=["chrA", "chrB", "chrE"])


def placed_regions(nbp=1 << 14):
    """((ichr, qs, qe), notes): every region with what it is there for"""
    rows = [
        (0, 1000, 2000, "book-ended with f0's [2000, 2500): d = 1"),
        (0, 2500, 2600, "book-ended on the other side: d = 1"),
        (1, 6 * nbp, 6 * nbp + 10, "f0's [0, 5 nbp) reached only as an earlier tile's copy at W = 2 nbp"),
        (0, 50000, 50100, "f1: -v picks the farther record"),
        (0, 70000, 70010, "f2: a tie on both sides"),
        (0, 90020, 90030, "f2: two equal records"),
        (0, 20, 30, "f3: the window reaches before 0"),
        (0, 8 * nbp - 10, 8 * nbp + 50, "f3: the window reaches past the contig's last tile"),
        (0, 9 * nbp, 9 * nbp + 5, "starts past the last tile"),
        (0, -3 * nbp, -3 * nbp + 40, "a negative start"),
        (0, -2 ** 31, -2 ** 31 + 7, "the bottom of int32"),
        (2, TOP - 10, TOP, "inside the record at the top of int32"),
        (2, TOP, TOP, "zero length at 2^31 - 1"),
        (2, TOP - 3 * nbp, TOP - 3 * nbp + 1, "between the two records of chrE"),
        (2, 5, 6, "far below chrE's records: within reach at W = 2^30 only where 2^31 - 5 nbp - 6 + 1 <= 2^30 -- it is not"),
        (2, TOP - 2 ** 30, TOP - 2 ** 30 + 50, "2^30 below the top"),
        (0, 50100, 50000, "inverted around f1's gap"),
        (0, 49950, 49950, "zero length inside f1's record"),
        (-1, 100, 200, "unknown contig"), (3, 100, 200, "contig number = nCtg"),
    ]
    a = np.array([r[:3] for r in rows], np.int64)
    return (a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32)), [r[3] for r in rows]
