"""The values of the overlapping records per region and dataset, restated in numpy (include/igd_hip.h has the definitions), and
the fixtures of tests/test_map_host.py, tests/test_map_cli.py and tests/test_gpu_map.py.  A plain module: no pytest hooks.

    counted       a record (f, s, e, val) on the region's contig with s < qe and e > qs [and val >= v on a database with values]
    count[q][f]   the number of counted records of file f
    agg[q][f]     their sum, minimum or maximum of val (op "count": the count), 0 where count is 0
    sets          n_hit = #{q: count > 0}, pairs = sum of count, agg_sum = sum of agg, per set and file

The reference is a broadcast over the INTERVAL LISTS THE TEST ITSELF WROTE with write_igd_numpy (nearest_ref.ListDb) -- never
over anything read back from the .igd, so tiles, copies of records and the prefix skip do not exist here."""
import numpy as np

from nearest_ref import NOV, TOP, ListDb, clustered_lists, mixed_regions, sparse_lists  # noqa: F401  (the tests' fixtures)

OPS = ("count", "sum", "min", "max")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def ref_rows(db, ichr, qs, qe, op, v=None, block=256):
    """(count int32[nq, nfiles], agg int64[nq, nfiles]) from db's lists.  v: a value filter (None: none); it counts on gType 1
    only."""
    assert op in OPS
    ichr = np.asarray(ichr)
    nq, nf = len(qs), db.nfiles
    count = np.zeros((nq, nf), np.int64)
    agg = np.zeros((nq, nf), np.int64)
    use_v = v is not None and v != NOV and db.gtype == 1
    for c, (idx, s, e, val) in db.by_contig().items():
        if use_v:
            keep = val >= v
            idx, s, e, val = idx[keep], s[keep], e[keep], val[keep]
        if len(idx) == 0:
            continue
        order = np.argsort(idx, kind="stable")
        idx, s, e, val = idx[order], s[order], e[order], val[order]
        present, starts = np.unique(idx, return_index=True)
        sel = np.flatnonzero(ichr == c)
        for b0 in range(0, len(sel), block):
            q = sel[b0:b0 + block]
            a, b = np.asarray(qs, np.int64)[q][:, None], np.asarray(qe, np.int64)[q][:, None]
            hit = (s[None, :] < b) & (e[None, :] > a)
            cnt = np.add.reduceat(hit.astype(np.int64), starts, axis=1)
            count[np.ix_(q, present)] = cnt
            if op == "sum":
                g = np.add.reduceat(np.where(hit, val[None, :], 0), starts, axis=1)
            elif op == "min":
                g = np.minimum.reduceat(np.where(hit, val[None, :], np.int64(1) << 40), starts, axis=1)
            elif op == "max":
                g = np.maximum.reduceat(np.where(hit, val[None, :], -(np.int64(1) << 40)), starts, axis=1)
            else:
                g = cnt
            agg[np.ix_(q, present)] = np.where(cnt > 0, g, 0)
    return count.astype(np.int32), agg


def ref_sets(count, agg, set_off):
    """(n_hit, pairs, agg_sum), each int64[nsets, nfiles]: sums over the rows of each set"""
    nsets = len(set_off) - 1
    out = [np.zeros((nsets, count.shape[1]), np.int64) for _ in range(3)]
    for k in range(nsets):
        a, b = int(set_off[k]), int(set_off[k + 1])
        out[0][k] = (count[a:b] > 0).sum(axis=0)
        out[1][k] = count[a:b].astype(np.int64).sum(axis=0)
        out[2][k] = agg[a:b].sum(axis=0)
    return out


def mean_text(num, den):
    return "%.2f" % (float(num) / float(den)) if den > 0 else "NA"


def table_text(names, n_hit, pairs, agg_sum, op):
    """the block `igd search db -q F -V op` prints for one set, from its three rows; op "mean": the rows of op "sum", the mean over
    the pairs instead of over the regions with a hit"""
    out = ["index\tn_hit\tpairs\tmean_%s\tFile\n" % op]
    for i in range(len(names)):
        out.append("%d\t%d\t%d\t%s\t%s\n" % (i, n_hit[i], pairs[i], mean_text(agg_sum[i], pairs[i] if op == "mean" else n_hit[i]), names[i]))
    out.append("Pairs: %d; datasets with a hit: %d of %d\n" % (int(np.sum(pairs)), int(np.count_nonzero(n_hit)), len(names)))
    return "".join(out)


# ---- placed cases -----------------------------------------------------------------------------------------------------------
CROWD_VALUES = (I32_MAX, I32_MIN, -7, I32_MAX, I32_MAX)
CROWD_RECORDS = 300


def crowd_base(nbp=1 << 14):
    """where the crowd file's records start: inside tile 7 of chrA, two tiles past every other record of the contig"""
    return 7 * nbp + 100


def crowd_file(nbp=1 << 14):
    """300 records of one file in one tile, record k starting at base + k: sorted by start, every 64 consecutive records -- one
    load of a wave -- belong to this file, and under a region over all of them every lane folds into the same (region, file)
    cell.  The values cycle through CROWD_VALUES; a record of value INT32_MAX ends 50 bp behind its start, one of INT32_MIN at
    base + 1000 + k and one of -7 at base + 2000 + k, so that regions behind the starts select records by value."""
    base = crowd_base(nbp)
    tail = {I32_MAX: lambda k: base + k + 50, I32_MIN: lambda k: base + 1000 + k, -7: lambda k: base + 2000 + k}
    recs = [("chrA", base + k, tail[CROWD_VALUES[k % 5]](k), CROWD_VALUES[k % 5]) for k in range(CROWD_RECORDS)]
    assert (base + 2000 + CROWD_RECORDS) // nbp == base // nbp
    return recs


def crowd_regions(nbp=1 << 14):
    """((ichr, qs, qe), counts): all 300 records; the first 128; the records of -7 alone; those of INT32_MIN and -7 (a sum far
    below -2^32).  counts: the records each region overlaps, without a value filter."""
    base = crowd_base(nbp)
    rows = [(0, base - 10, base + 400), (0, base - 10, base + 128), (0, base + 1500, base + 1600), (0, base + 600, base + 700)]
    a = np.array(rows, np.int64)
    n7 = sum(1 for k in range(CROWD_RECORDS) if CROWD_VALUES[k % 5] == -7)
    nmin = sum(1 for k in range(CROWD_RECORDS) if CROWD_VALUES[k % 5] == I32_MIN)
    return (a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32)), [CROWD_RECORDS, 128, n7, n7 + nmin]


def pad_file(i, nbp=1 << 14):
    """file i of a padded placed_db: one short record on chrB with a negative value, somewhere in the contig's first twelve
    tiles -- under placed_regions' seven-tile region when it starts below 7 nbp + 3, clear of every other region"""
    s = (i * 2654435761) % (12 * nbp)
    return [("chrB", s, s + 1 + i % 50, -1 - i % 1000)]


def placed_db(d, nbp=1 << 14, name="mplaced", pad_to=None, crowd=False):
    """One database for the placed cases of the issue; chrE holds the coordinates at 2^31 - 1 (its tiles run up there).
    crowd: crowd_file() follows as file 6.  pad_to = n: pad_file()s follow until there are n files (the wide forms)."""
    files = [
        # f0: a record over five tiles (under a region over seven), and a book-ended pair around region [1000, 2000)
        [("chrB", nbp + 5, 6 * nbp - 5, 321), ("chrA", 2000, 2500, 900), ("chrA", 500, 1000, 900)],
        # f1: two equal records
        [("chrA", 90000, 90010, 77), ("chrA", 90000, 90010, 77)],
        # f2: negative values, and the ends of int32
        [("chrA", 70000, 70100, -5), ("chrA", 70050, 70200, -900), ("chrA", 70090, 70300, 3),
         ("chrA", 40000, 40100, I32_MIN), ("chrA", 40050, 40200, I32_MAX)],
        # f3: three records of INT32_MAX under one region: the sum needs 64 bits
        [("chrA", 50000, 50100, I32_MAX), ("chrA", 50010, 50100, I32_MAX), ("chrA", 50020, 50400, I32_MAX)],
        # f4: -v 500 removes the maximum's rivals or the maximum itself: values 100, 499, 500, 800 under one region
        [("chrA", 60000, 60010, 100), ("chrA", 60005, 60020, 499), ("chrA", 60008, 60030, 500), ("chrA", 60009, 60040, 800),
         ("chrA", 61000, 61010, 400)],
        # f5: the top of int32
        [("chrE", TOP - 100, TOP, 900), ("chrE", TOP - 5 * nbp, TOP - 5 * nbp + 10, -1)],
    ]
    if crowd:
        files.append(crowd_file(nbp))
    while pad_to is not None and len(files) < pad_to:
        files.append(pad_file(len(files), nbp))
    return ListDb(d, name, files, nbp, 1, contig_order=["chrA", "chrB", "chrE"])


def placed_regions(nbp=1 << 14):
    """((ichr, qs, qe), notes): every region with what it is there for"""
    rows = [
        (1, 10, 7 * nbp + 3, "seven tiles over f0's record of five: counted once, its value taken once"),
        (0, 1000, 2000, "book-ended on both sides with f0's records: not counted"),
        (0, 90005, 90006, "f1: two equal records, both counted"),
        (0, 70000, 70400, "f2: negative values"),
        (0, 40000, 40300, "f2: INT32_MIN and INT32_MAX under one region"),
        (0, 40000, 40050, "f2: INT32_MIN alone"),
        (0, 50000, 50500, "f3: three times INT32_MAX"),
        (0, 60000, 60100, "f4: -v 500 keeps 500 and 800"),
        (0, 60000, 60008, "f4: -v 500 removes every record (and the maximum 499)"),
        (0, 61000, 61010, "f4: one record below -v 500"),
        (0, 9 * nbp, 9 * nbp + 5, "starts past the last tile"),
        (0, -3 * nbp, -3 * nbp + 40, "a negative start"),
        (0, -3 * nbp, 1200, "a negative start that reaches f0's first record"),
        (0, -2 ** 31, -2 ** 31 + 7, "the bottom of int32"),
        (0, -2 ** 31, TOP, "all of int32"),
        (2, TOP - 10, TOP, "inside the record at the top of int32"),
        (2, TOP, TOP, "zero length at 2^31 - 1"),
        (2, TOP - 6 * nbp, TOP, "both records of chrE"),
        (0, 70095, 70060, "inverted inside two of f2's records"),
        (0, 70095, 70095, "zero length inside f2's three records"),
        (0, 3000, 3000, "zero length in a gap: an empty row between two that are not"),
        (0, 70000, 70400, "f2 again"),
        (-1, 100, 200, "unknown contig"), (3, 100, 200, "contig number = nCtg"),
    ]
    a = np.array([r[:3] for r in rows], np.int64)
    return (a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32)), [r[3] for r in rows]
