"""Merged region sets and the base-pair Jaccard per set and dataset, restated in plain Python and numpy (include/igd_hip.h has the
definitions), for tests/test_jaccard_host.py, tests/test_jaccard_cli.py and tests/test_gpu_jaccard.py.  A plain module: no pytest
hooks.  Built on tests/nearest_ref.py's ListDb.

    takes part:  0 <= ichr < nctg and qe > qs; the others are dropped and counted
    merge:       per set, sort by (ichr, qs, qe); a region opens a run iff it is the first of its contig or qs > E + gap, E the
                 largest end so far on that contig; a run is (ichr, first qs, largest qe, regions joined)
    inter, file_bp, set_bp: one boolean array per contig -- the set's runs, the counted records of a file -- and-ed and summed
    rule NEST (the command line's without -v, and gType 0): a region whose first tile holds no record, or lies past the contig's
                 tiles, counts nothing -- the search's own rule, restated from the lists (a record lies in the tiles it overlaps)

The reference works on the INTERVAL LISTS THE TEST ITSELF WROTE."""
import numpy as np

from nearest_ref import NOV

MAX_GAP = 1 << 30
NEST, FLAT = 0, 1


def ref_merge(nctg, ichr, qs, qe, set_off, gap=0):
    """(m_ichr, m_qs, m_qe int32, m_off int64[nsets + 1], m_count int32, n_dropped int64[nsets]): a Python sort and sweep"""
    runs, off, dropped = [], [0], []
    for k in range(len(set_off) - 1):
        a, b = int(set_off[k]), int(set_off[k + 1])
        regs = sorted((int(ichr[i]), int(qs[i]), int(qe[i])) for i in range(a, b) if 0 <= ichr[i] < nctg and qe[i] > qs[i])
        dropped.append(b - a - len(regs))
        cur = None
        for c, s, e in regs:
            if cur is None or c != cur[0] or s > cur[2] + gap:
                cur = [c, s, e, 1]
                runs.append(cur)
            else:
                cur[2] = max(cur[2], e)
                cur[3] += 1
        off.append(len(runs))
    r = np.array(runs, np.int64).reshape(-1, 4)
    return (r[:, 0].astype(np.int32), r[:, 1].astype(np.int32), r[:, 2].astype(np.int32), np.array(off, np.int64), r[:, 3].astype(np.int32),
            np.array(dropped, np.int64))


def ref_merge_np(nctg, ichr, qs, qe, set_off, gap=0):
    """ref_merge's six arrays, vectorised for millions of regions: a lexsort by (set, contig, qs, qe); the largest end so far
    of every (set, contig) segment as ONE running maximum over end + (segment << 32) in int64, the ends moved to 0 .. 2^32 - 1
    so that a later segment's smallest value is above an earlier one's largest; run heads, counts, dropped regions"""
    ichr, qs, qe = (np.asarray(a).astype(np.int64) for a in (ichr, qs, qe))
    set_off = np.asarray(set_off, np.int64)
    nsets = len(set_off) - 1
    setof = np.repeat(np.arange(nsets, dtype=np.int64), np.diff(set_off))
    part = (ichr >= 0) & (ichr < nctg) & (qe > qs)
    dropped = np.bincount(setof[~part], minlength=nsets).astype(np.int64)
    s, c, a, b = setof[part], ichr[part], qs[part], qe[part]
    order = np.lexsort((b, a, c, s))
    s, c, a, b = s[order], c[order], a[order], b[order]
    m = len(s)
    seg_head = np.ones(m, bool)
    seg_head[1:] = (s[1:] != s[:-1]) | (c[1:] != c[:-1])
    seg = (np.cumsum(seg_head) - 1) << 32
    inc = np.maximum.accumulate(b + (1 << 31) + seg) - seg - (1 << 31)
    opens = seg_head.copy()
    opens[1:] |= a[1:] > inc[:-1] + gap
    heads = np.flatnonzero(opens)
    ends = np.append(heads[1:], m)[:len(heads)]          # (no region takes part: no run)
    m_off = np.concatenate([[0], np.cumsum(np.bincount(s[heads], minlength=nsets))]).astype(np.int64)
    return (c[heads].astype(np.int32), a[heads].astype(np.int32), inc[ends - 1].astype(np.int32), m_off, (ends - heads).astype(np.int32), dropped)


def _masks(db, span, v):
    """per contig: bool[nfiles + 1, span], row f the bp under the counted records of file f, the last row under any file's"""
    use_v = v is not None and v != NOV and db.gtype == 1
    out = {}
    for c, (idx, s, e, val) in db.by_contig().items():
        m = np.zeros((db.nfiles + 1, span), bool)
        for f, a, b, x in zip(idx, s, e, val):
            if not use_v or x >= v:
                m[f, a:b] = True
        m[db.nfiles] = m[:db.nfiles].any(axis=0)
        out[c] = m
    return out


def _span(db):
    return max([int(e.max()) for (_, _, e, _) in db.by_contig().values() if len(e)] + [1])


def ref_dataset_bp(db, v=None):
    """file_bp int64[nfiles + 1]"""
    bp = np.zeros(db.nfiles + 1, np.int64)
    for m in _masks(db, _span(db), v).values():
        bp += m.sum(axis=1)
    return bp


def _tile_used(db):
    """per contig: bool[ntiles], the tile holds a record (a record lies in every tile it overlaps)"""
    out = {}
    for c, (_, s, e, _) in db.by_contig().items():
        used = np.zeros(int((e.max() - 1) // db.nbp) + 1 if len(e) else 0, bool)
        for a, b in zip(s, e):
            used[a // db.nbp:(b - 1) // db.nbp + 1] = True
        out[c] = used
    return out


def ref_jaccard(db, ichr, qs, qe, set_off, v=None, rule=FLAT):
    """(inter int64[nsets, nfiles + 1], set_bp, file_bp, n_merged, n_dropped) from db's lists; regions need 0 <= qs"""
    nsets, nf = len(set_off) - 1, db.nfiles
    mc, ms, me, moff, _, dropped = ref_merge(len(db.ctgs), ichr, qs, qe, set_off, 0)
    span = max(_span(db), int(me.max()) if len(me) else 1)
    masks, used = _masks(db, span, v), _tile_used(db)
    inter, set_bp = np.zeros((nsets, nf + 1), np.int64), np.zeros(nsets, np.int64)
    for k in range(nsets):
        mine = {c: np.zeros(span, bool) for c in masks}
        for r in range(int(moff[k]), int(moff[k + 1])):
            c, a, b = int(mc[r]), int(ms[r]), int(me[r])
            set_bp[k] += b - a
            t = a // db.nbp
            if rule == NEST and (t >= len(used[c]) or not used[c][t]):
                continue
            mine[c][a:b] = True
        for c, m in masks.items():
            inter[k] += (m & mine[c][None, :]).sum(axis=1)
    return inter, set_bp, ref_dataset_bp(db, v), np.diff(moff), dropped


def ratio_text(num, den):
    return "%.6f" % (float(num) / float(den)) if den != 0 else "NA"


def table_text(names, inter_k, set_bp, file_bp, n_merged, n_dropped):
    """the block `igd search db -q F -J` prints for one set"""
    nf = len(names)
    out = ["index\tintersection\tunion\tjaccard\tset_fraction\tfile_bp\tFile\n"]
    for i in range(nf):
        u = set_bp + file_bp[i] - inter_k[i]
        out.append("%d\t%d\t%d\t%s\t%s\t%d\t%s\n" % (i, inter_k[i], u, ratio_text(inter_k[i], u), ratio_text(inter_k[i], set_bp), file_bp[i], names[i]))
    out.append("Any dataset: %d of %d bp in %d merged regions (%d dropped); jaccard %s\n"
               % (inter_k[nf], set_bp, n_merged, n_dropped, ratio_text(inter_k[nf], set_bp + file_bp[nf] - inter_k[nf])))
    return "".join(out)


def jaccard_regions(rng, nctg, nbp, span, n):
    """regions with 0 <= qs: unknown contigs, zero-length and inverted ones, short, nested, book-ended and many-tile ones, every
    fifth one repeated, some that start past the contig's last tile"""
    ichr = np.array([rng.choice(list(range(nctg)) + [-1, 99]) for _ in range(n)], np.int64)
    qs = np.array([rng.choice([rng.randrange(0, span), rng.randrange(0, span), span + rng.randrange(7 * nbp, 9 * nbp)]) for _ in range(n)], np.int64)
    ln = np.array([rng.choice([0, 1, 200, 700, nbp, 2 * nbp + 5, rng.randint(1, 3 * nbp), -rng.randint(1, 50)]) for _ in range(n)], np.int64)
    qe = qs + ln
    for i in range(5, n, 5):
        ichr[i], qs[i], qe[i] = ichr[i - 1], qs[i - 1], qe[i - 1]
    for i in range(7, n, 7):                             # book-ended with the one before
        ichr[i], qs[i], qe[i] = ichr[i - 1], max(qe[i - 1], 0), max(qe[i - 1], 0) + 50
    return ichr.astype(np.int32), qs.astype(np.int32), qe.astype(np.int32)
