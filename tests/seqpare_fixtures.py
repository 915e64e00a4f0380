"""Databases and query files of the Seqpare tests (tests/test_seqpare_ref.py without a GPU, tests/test_gpu_seqpare_scale.py
with one), written with the independent numpy writer.  Every builder takes a directory and returns a dict with `igd` and `q`
(paths) and what its conditions need.  The building block: k records of one dataset that all overlap each other inside ONE
tile, under j queries of that tile's contig that overlap them all -- a (query contig, dataset) group of exactly j * k
candidates, which the tests assert on the reference's diagnostics, not on this construction."""
import os
import random
from fractions import Fraction

from helpers import write_igd_numpy

NBP = 16384
# (queries j, records k): 1, 63, 64, 65 around the kernel's batch of 64; 128, 129; 1023, 1024, 1025 around SQ_CAP (LDS -> HBM hash
# sets); 2048 and 2049, where the HBM table's power of two (the smallest >= 2n) steps from 4096 to 8192
EDGE_SHAPES = [(1, 1), (7, 9), (8, 8), (5, 13), (8, 16), (3, 43), (31, 33), (32, 32), (25, 41), (32, 64), (3, 683)]
EDGE_SIZES = [j * k for j, k in EDGE_SHAPES]


def _write_q(path, rows):
    with open(path, "w") as f:
        f.write("".join("%s\t%d\t%d\n" % r for r in rows))


def _pile(rng, base, j, k, identical, lens=None):
    """(records, queries) as (start, end): all k records overlap all j queries and each other; max start < base + 2 100 and
    min end >= base + 3 000, everything below base + 6 000.  `lens`: draw the free part of the ends from this short list
    (many repeated scores) instead of from 0 .. 2 999."""
    if identical:
        return [(base, base + 100)] * k, [(base, base + 100)] * j
    tail = (lambda: rng.choice(lens)) if lens else (lambda: rng.randrange(0, 3000))
    head = (lambda: rng.choice(lens)) if lens else (lambda: rng.randrange(0, 2100))
    recs = [(base + (3 * r if not lens else head()), base + 3000 + tail()) for r in range(k)]
    qrys = [(base + head(), base + 3000 + tail()) for _ in range(j)]
    return recs, qrys


def edges(d, identical):
    """11 datasets, dataset i alone on contig chr(i+1) with EDGE_SHAPES[i]; chr12 is known to the database (one far record) and
    its queries overlap nothing.  The query file names the contigs in another order than the database."""
    rng = random.Random(11 + identical)
    files, qrows = [], {}
    base = 3 * NBP + 50
    for i, (j, k) in enumerate(EDGE_SHAPES):
        c = "chr%d" % (i + 1)
        recs, qrys = _pile(rng, base, j, k, identical)
        files.append([(c, s, e, 1) for s, e in recs])
        qrows[c] = [(c, s, e) for s, e in qrys]
    files[0].append(("chr12", 40 * NBP, 40 * NBP + 10, 1))
    qrows["chr12"] = [("chr12", 100 + 7 * i, 400 + 9 * i) for i in range(5)]
    names = ["chr%d" % (i + 1) for i in range(11)]
    order = names[:5:-1] + ["chr12"] + names[5::-1] if not identical else names[:4] + ["chr12"] + names[4:]
    tag = "ei" if identical else "em"
    out = dict(igd=os.path.join(d, tag + ".igd"), q=os.path.join(d, tag + ".bed"), empty_group=order.index("chr12"))
    write_igd_numpy(out["igd"], files, nbp=NBP, contig_order=names + ["chr12"])
    _write_q(out["q"], [r for c in order for r in qrows[c]])
    return out


def chains(d):
    """2 datasets x 2 contigs, 12 queries over 12 records each (144 candidates = 3 runs of 64), ends and starts from four values:
    many equal scores, so rows and columns are contested inside a run and across runs."""
    rng = random.Random(21)
    lens = [0, 50, 100, 150]
    files, q = [[], []], []
    for ci, c in enumerate(("chr1", "chr2")):
        base = (2 + ci) * NBP + 10
        for m in range(2):
            recs, qrys = _pile(rng, base, 12, 12, False, lens)
            files[m] += [(c, s, e, 1) for s, e in recs]
        q += [(c, s, e) for s, e in qrys]
    out = dict(igd=os.path.join(d, "ch.igd"), q=os.path.join(d, "ch.bed"))
    write_igd_numpy(out["igd"], files, nbp=NBP)
    _write_q(out["q"], q)
    return out


def near_ties(d):
    """Tiles of 2^21 bp; dataset m has 12 records of L, L + 1, .. bp (L = 10^4, 10^5, 10^6 for m = 0, 1, 2) from two starts one
    base apart, under 10 queries of L, L + 2, .. bp: quotients a / b and (a + 1) / (b + 1) whose float32 values differ in the last
    bits or not at all.  `exact[m]`: the distinct exact quotients overlap / (|q| + |r| - overlap) of dataset m's pairs."""
    nbp = 1 << 21
    files, q, exact = [], [], {}
    for m, L in enumerate((10 ** 4, 10 ** 5, 10 ** 6)):
        c = "chr%d" % (m + 1)
        recs = [(1000 + (r & 1), 1000 + (r & 1) + L + r) for r in range(12)]
        qrys = [(1000 + (i % 3), 1000 + (i % 3) + L + 2 * i) for i in range(10)]
        files.append([(c, s, e, 1) for s, e in recs])
        q += [(c, s, e) for s, e in qrys]
        ex = set()
        for qs, qe in qrys:
            for rs, re in recs:
                st = min(qe, re) - max(qs, rs)
                assert st > 0
                ex.add(Fraction(st, (qe - qs) + (re - rs) - st))
        exact[m] = ex
    out = dict(igd=os.path.join(d, "nt.igd"), q=os.path.join(d, "nt.bed"), exact=exact)
    write_igd_numpy(out["igd"], files, nbp=nbp)
    _write_q(out["q"], q)
    return out


WAVES_FILES, WAVES_LEAD, WAVES_CONTIGS, WAVES_J = 40, 20, 28, 25


def waves(d):
    """40 datasets x 28 contigs = 1 120 groups of 25 queries each.  Groups are handed out in order, one per wave at first, so
    the first 20 contigs (800 groups) are all of the largest class: every wave starts with a group above 1 024 candidates and
    what it takes next comes from the last 8 contigs, where the class of group (c, m) is (c + m) % 4 -- no record, 1 or 2
    records (below 64 candidates), 3 .. 39 (75 .. 975), 41 .. 43 (1 025 .. 1 075) -- and cycles in group order."""
    rng = random.Random(31)
    files = [[] for _ in range(WAVES_FILES)]
    q = []
    for ci in range(WAVES_CONTIGS):
        c = "chr%d" % (ci + 1)
        base = (1 + ci % 5) * NBP + 20
        qrys = None
        for m in range(WAVES_FILES):
            cls = (ci + m) % 4 if ci >= WAVES_LEAD else 3
            k = (0, 1 + (ci + m) % 2, 3 + (7 * ci + m) % 37, 41 + (ci + m) % 3)[cls]
            recs, qr = _pile(rng, base, WAVES_J, k, False, [0, 40, 80, 120, 160, 200, 240] if m % 3 == 0 else None)
            qrys = qrys or qr
            files[m] += [(c, s, e, 1) for s, e in recs]
        q += [(c, s, e) for s, e in qrys]
    out = dict(igd=os.path.join(d, "wv.igd"), q=os.path.join(d, "wv.bed"))
    write_igd_numpy(out["igd"], files, nbp=NBP, contig_order=["chr%d" % (i + 1) for i in range(WAVES_CONTIGS)])
    _write_q(out["q"], q)
    return out


def waves_classes(ref):
    """class (0 empty, 1 below 64, 2 from 65 to 1 024, 3 above) of every group of the waves fixture, in group order"""
    cls = lambda n: 0 if n == 0 else 1 if n < 64 else 2 if 65 <= n <= 1024 else 3 if n > 1024 else None
    return [cls(ref.diag[(c, m)].size if (c, m) in ref.diag else 0) for c in range(ref.args[4]) for m in range(WAVES_FILES)]


def few(d, nfiles, nctg):
    """nfiles x nctg groups; group g = c * nfiles + m has 1 + g % 9 queries (per contig: 1 + c % 9) over (5 * g + 3) % 17 records
    (one query contig: 9 queries; one group: 9 x 15)."""
    rng = random.Random(41 + nfiles + nctg)
    files = [[] for _ in range(nfiles)]
    q = []
    for ci in range(nctg):
        c = "chr%d" % (ci + 1)
        base = 2 * NBP + 5
        j = 1 + ci % 9 if nctg > 1 else 9
        qrys = None
        for m in range(nfiles):
            g = ci * nfiles + m
            k = (5 * g + 3) % 17 if nfiles * nctg > 1 else 15
            recs, qr = _pile(rng, base, j, k, False, [0, 30, 60, 90] if g % 2 else None)
            qrys = qrys or qr
            files[m] += [(c, s, e, 1) for s, e in recs]
        q += [(c, s, e) for s, e in qrys]
    tag = "fw%dx%d" % (nfiles, nctg)
    out = dict(igd=os.path.join(d, tag + ".igd"), q=os.path.join(d, tag + ".bed"))
    write_igd_numpy(out["igd"], files, nbp=NBP, contig_order=["chr%d" % (i + 1) for i in range(nctg)])
    _write_q(out["q"], q)
    return out


def awkward(d):
    """Tiles of 4 096 bp, 6 datasets, 3 contigs: 1-bp records, records over up to 5 tiles, piles of identical records; queries of
    length 0, over several tiles, past the last tile, duplicated, on a contig the database does not have, on a name that is no
    `chr`, with start > end."""
    rng = random.Random(51)
    nbp = 4096
    files = []
    for m in range(6):
        recs = []
        for c in ("chr1", "chr2", "chrX"):
            for _ in range(150):
                kind = rng.random()
                if kind < 0.25:
                    s = rng.randrange(0, 30 * nbp); e = s + 1
                elif kind < 0.6:
                    s = rng.randrange(0, 30 * nbp); e = s + rng.randrange(1, 5 * nbp)
                elif kind < 0.8:
                    s = 5 * nbp + 256 * rng.randrange(0, 4); e = s + rng.choice([100, 100, 250])
                else:
                    s = 7 * nbp - rng.randrange(1, 300); e = s + rng.choice([300, 300, nbp + 7])
                recs.append((c, s, e, rng.randrange(0, 1000)))
        files.append(recs)
    rows = []
    for _ in range(700):
        if rows and rng.random() < 0.2:
            rows.append(rng.choice(rows))
            continue
        c = rng.choice(["chr1", "chr2", "chrX", "chr10", "chr1", "1"])
        kind = rng.random()
        if kind < 0.4:
            s = rng.randrange(0, 40 * nbp)
        elif kind < 0.7:
            s = 5 * nbp + 256 * rng.randrange(0, 4) + rng.randrange(0, 3)
        else:
            s = 7 * nbp - rng.randrange(0, 400)
        L = rng.choice([0, 0, 1, 7, 100, 300, nbp // 2, nbp, 3 * nbp + 5, rng.randrange(1, 2 * nbp), -20])
        rows.append((c, s, s + L))
    out = dict(igd=os.path.join(d, "aw.igd"), q=os.path.join(d, "aw.bed"))
    write_igd_numpy(out["igd"], files, nbp=nbp)
    _write_q(out["q"], rows)
    return out


BUILDERS = {
    "edges_mixed": lambda d: edges(d, False),
    "edges_identical": lambda d: edges(d, True),
    "chains": chains,
    "near_ties": near_ties,
    "waves": waves,
    "few_1x1": lambda d: few(d, 1, 1),
    "few_2x1": lambda d: few(d, 2, 1),
    "few_257x1": lambda d: few(d, 257, 1),
    "few_1x257": lambda d: few(d, 1, 257),
    "awkward": awkward,
}
