"""Signed nearest distances and their histogram per set and dataset, restated in numpy (include/igd_hip.h has the definitions),
for tests/test_nearest_signed_host.py, tests/test_nearest_signed_cli.py and tests/test_gpu_nearest_signed.py.  A plain module: no
pytest hooks.  Built on tests/nearest_ref.py's ListDb, lists and regions.

    a = s - qe, b = qs - e                                           (64 bits)
    key = 0 if s < qe and e > qs else 2 (a + 1) + 1 if a >= b else 2 (b + 1)       d = key >> 1, within the window iff d <= W
    sdist[q][f] = decode(min key over the records of file f within the window [with value >= v]), NO_RECORD when there is none
    decode(key) = -(key >> 1) for an even key, +(key >> 1) for an odd one
    sdmin[q]    = decode(min over the files of those minimum keys), else NO_RECORD
    bin(x)      = #{k : edges[k] <= x};  hist[k][b][f] = #{q in set k : sdist[q][f] != NO_RECORD and bin(sdist[q][f]) == b}

The reference is a broadcast over the INTERVAL LISTS THE TEST ITSELF WROTE, as nearest_ref.ref_rows is."""
import numpy as np

from nearest_ref import NONE, NOV

NO_RECORD = -2 ** 31                # IGD_HIP_NEAREST_NO_RECORD
MAX_EDGES = 63                      # IGD_HIP_NEAREST_MAX_EDGES


def pair_key(qs, qe, s, e):
    """key of every (region, record) pair: int64[nq, nrec]"""
    qs, qe = np.asarray(qs, np.int64)[:, None], np.asarray(qe, np.int64)[:, None]
    s, e = np.asarray(s, np.int64)[None, :], np.asarray(e, np.int64)[None, :]
    a, b = s - qe, qs - e
    return np.where((s < qe) & (e > qs), 0, np.where(a >= b, 2 * (a + 1) + 1, 2 * (b + 1)))


def decode(key):
    """int64 keys (NONE: no record) -> int32 signed distances"""
    key = np.asarray(key, np.int64)
    d = key >> 1
    return np.where(key >= NONE, NO_RECORD, np.where(key & 1 == 1, d, -d)).astype(np.int32)


def ref_signed_rows(db, ichr, qs, qe, window, v=None, block=256):
    """(sdist int32[nq, nfiles], sdmin int32[nq]) from db's lists.  v: a value filter (None: none); it counts on gType 1 only."""
    ichr = np.asarray(ichr)
    nq, nf = len(qs), db.nfiles
    keys = np.full((nq, nf), NONE, np.int64)
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
            k = pair_key(qs[q], qe[q], s, e)
            k = np.where((k >> 1) <= window, k, NONE)
            out = np.full((len(q), nf), NONE, np.int64)
            out[:, present] = np.minimum.reduceat(k, starts, axis=1)
            keys[q] = out
    return decode(keys), decode(keys.min(axis=1, initial=NONE))


def bins(x, edges):
    """bin(x) of every element: the number of edges <= x"""
    return (np.asarray(edges, np.int64)[None, :] <= np.asarray(x, np.int64).reshape(-1, 1)).sum(axis=1).reshape(np.shape(x))


def ref_hist(sdist, sdmin, set_off, edges):
    """hist int64[nsets, ne + 1, nfiles + 1]: the last column from sdmin"""
    full = np.concatenate([sdist.astype(np.int64), sdmin.astype(np.int64)[:, None]], axis=1)
    nsets, nb = len(set_off) - 1, len(edges) + 1
    hist = np.zeros((nsets, nb, full.shape[1]), np.int64)
    for k in range(nsets):
        r = full[int(set_off[k]):int(set_off[k + 1])]
        b = bins(r, edges)
        for j in range(nb):
            hist[k, j] = ((b == j) & (r != NO_RECORD)).sum(axis=0)
    return hist


def bin_labels(edges):
    e = [int(x) for x in edges]
    return ["<%d" % e[0]] + ["[%d,%d)" % (e[i - 1], e[i]) for i in range(1, len(e))] + [">=%d" % e[-1]]


def table_text(names, hist_k, edges, window, nq):
    """the block `igd search db -q F -N window -H edges` prints for one set, from its histogram int64[ne + 1, nfiles + 1]"""
    nf = len(names)
    out = ["index\tn_within\t" + "\t".join(bin_labels(edges)) + "\tFile\n"]
    for i in range(nf):
        out.append("%d\t%d\t%s\t%s\n" % (i, hist_k[:, i].sum(), "\t".join("%d" % x for x in hist_k[:, i]), names[i]))
    out.append("Any dataset within %d bp: %d of %d\t%s\n" % (window, hist_k[:, nf].sum(), nq, "\t".join("%d" % x for x in hist_k[:, nf])))
    return "".join(out)


# ---- edge lists of the issue ------------------------------------------------------------------------------------------------
def edge_lists(W):
    """(0,), (0, 1), (-W, 0, 1, W + 1) -- ascending only for W > 0 --, 63 consecutive edges around 0, the ends of int32"""
    return [(0,), (0, 1)] + ([(-W, 0, 1, W + 1)] if W > 0 else []) + [tuple(range(-31, 32)), (-2 ** 31 + 1, 0, 2 ** 31 - 1)]
