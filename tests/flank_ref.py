"""Flanking records per dataset and the relative-distance histogram, restated in numpy (include/igd_hip.h has the definitions), for
tests/test_flank_host.py, tests/test_flank_cli.py and tests/test_gpu_flank.py.  A plain module: no pytest hooks.  Built on
tests/nearest_ref.py's ListDb, lists and regions.

    d = 0 if s < qe and e > qs else max(s - qe, qs - e) + 1          a record is counted iff d <= W [and value >= v]
    edges:      a = s - qe, b = qs - e; d > 0 and a >= b: downstream at d; d > 0 and a < b: upstream at d; d == 0: neither
    midpoints:  D = ((s + e) >> 1) - ((qs + qe) >> 1); takes part iff |D| <= W; D < 0: upstream at -D; D >= 0: downstream at D
    up[q][f], down[q][f] = the minimum over the side's records of file f, -1 when there is none; upmin, downmin over the files
    flanked:    up >= 0 and down >= 0 and up + down > 0;  bin = min(B - 1, 2 B min(up, down) // (up + down))
    hist[k][b][f] = #{q in set k : (q, f) flanked and in bin b}; column nfiles from upmin / downmin

The reference is a broadcast over the INTERVAL LISTS THE TEST ITSELF WROTE, as nearest_ref.ref_rows is."""
import numpy as np

from nearest_ref import NONE, NOV, pair_dist, row_min

EDGES, MIDPOINTS = 0, 1             # IGD_HIP_FLANK_EDGES, IGD_HIP_FLANK_MIDPOINTS
MAX_BINS = 64                       # IGD_HIP_FLANK_MAX_BINS


def pair_sides(qs, qe, s, e, window, measure):
    """(up, down) int64[nq, nrec]: the distance of every (region, record) pair on its side, NONE elsewhere"""
    d = pair_dist(qs, qe, s, e)
    qs, qe = np.asarray(qs, np.int64)[:, None], np.asarray(qe, np.int64)[:, None]
    s, e = np.asarray(s, np.int64)[None, :], np.asarray(e, np.int64)[None, :]
    counted = d <= window
    if measure == EDGES:
        dn = s - qe >= qs - e
        return np.where(counted & (d > 0) & ~dn, d, NONE), np.where(counted & (d > 0) & dn, d, NONE)
    D = ((s + e) >> 1) - ((qs + qe) >> 1)
    part = counted & (np.abs(D) <= window)
    return np.where(part & (D < 0), -D, NONE), np.where(part & (D >= 0), D, NONE)


def ref_flanks(db, ichr, qs, qe, window, measure, v=None, block=256):
    """(up, down int32[nq, nfiles], upmin, downmin int32[nq]) from db's lists.  v: a value filter (None: none; gType 1 only)."""
    ichr = np.asarray(ichr)
    nq, nf = len(qs), db.nfiles
    out = [np.full((nq, nf), -1, np.int32), np.full((nq, nf), -1, np.int32)]
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
            for side, x in enumerate(pair_sides(qs[q], qe[q], s, e, window, measure)):
                m = np.minimum.reduceat(x, starts, axis=1)
                row = np.full((len(q), nf), -1, np.int64)
                row[:, present] = np.where(m < NONE, m, -1)
                out[side][q] = row
    return out[0], out[1], row_min(out[0]), row_min(out[1])


def flanked(up, down):
    up, down = np.asarray(up, np.int64), np.asarray(down, np.int64)
    return (up >= 0) & (down >= 0) & (up + down > 0)


def bins(up, down, nbins):
    """the bin of every pair (anything where the pair is not flanked)"""
    up, down = np.asarray(up, np.int64), np.asarray(down, np.int64)
    t = np.where(flanked(up, down), up + down, 1)
    return np.minimum(nbins - 1, 2 * nbins * np.minimum(up, down) // t)


def ref_hist(up, down, upmin, downmin, set_off, nbins):
    """hist int64[nsets, nbins, nfiles + 1]: the last column from upmin / downmin"""
    u = np.concatenate([up.astype(np.int64), upmin.astype(np.int64)[:, None]], axis=1)
    d = np.concatenate([down.astype(np.int64), downmin.astype(np.int64)[:, None]], axis=1)
    nsets = len(set_off) - 1
    hist = np.zeros((nsets, nbins, u.shape[1]), np.int64)
    for k in range(nsets):
        a, b = int(set_off[k]), int(set_off[k + 1])
        ok, bn = flanked(u[a:b], d[a:b]), bins(u[a:b], d[a:b], nbins)
        for j in range(nbins):
            hist[k, j] = (ok & (bn == j)).sum(axis=0)
    return hist


def table_text(names, hist_k, window, nq):
    """the block `igd search db -q F -N window -L nbins` prints for one set, from its histogram int64[nbins, nfiles + 1]"""
    nf, nb = len(names), hist_k.shape[0]
    out = ["index\tn_flanked\t" + "\t".join("%.4f" % (k / (2.0 * nb)) for k in range(nb)) + "\tFile\n"]
    for i in range(nf):
        out.append("%d\t%d\t%s\t%s\n" % (i, hist_k[:, i].sum(), "\t".join("%d" % x for x in hist_k[:, i]), names[i]))
    out.append("Any dataset within %d bp: %d of %d\t%s\n" % (window, hist_k[:, nf].sum(), nq, "\t".join("%d" % x for x in hist_k[:, nf])))
    return "".join(out)
