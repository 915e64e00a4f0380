"""Fixtures for the sets / support / coverage kernels (igd_sets_count, igd_sets_support, igd_sets_coverage) beyond one slice
per workgroup.  A plain module: no pytest hooks.  tests/test_sets_fixtures.py checks it without a GPU;
tests/test_gpu_sets_scale.py and tests/test_gpu_coverage_scale.py use it on one.

    consts()         the constants of the work decomposition, read out of the sources
    plan()           the host's chunk and slice arithmetic (run_set_chunks, host_common.hpp, and its three callers), restated:
                     every test asserts through it that its fixture is in the regime it claims
    wide_db()        a database of many files whose boundary files (bit 0 and bit 31 of the first, 64th, 65th and last
                     bitmap word) lie inside a window that a known share of the queries covers
    scale_queries()  the query kinds of test_gpu_sets._queries, drawn with numpy (cases of 10^6 and more queries)
    expected_rows()  per set (hits, total, support, nhit), none of it from the kernels under test
    Witness          the non-vacuity conditions, asserted on the expectation alone
    expected_cov_rows()  per set (coverage, covered, pair sums), none of it from the kernel under test
    CovWitness       the same for covered base pairs
    bigbp_db(), bigbp_sets()  more than 2^32 bp under one file in one slice"""
import os
import random
import re

import numpy as np

from helpers import ROOT, write_igd_numpy
from test_coverage_host import coverage_brute, coverage_from_enumeration, read_rows
from test_support_host import cli_rule, oracle_support, oracle_support_enum

ENGINE = os.path.join(ROOT, "igd_amd", "csrc", "engine")
NBP = 1 << 14
ANCHOR_MAX = 1500          # sets of at most this many queries: igdc_support_host is held against the oracle in place
COV_ANCHORS = 40           # igdc_coverage_host is held in place against the brute force on this many non-empty sets at least


# ---- the constants and the host's arithmetic --------------------------------------------------------------------------------
def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, text, re.M)
    assert m, "no #define %s" % name
    val = m.group(1).strip()
    m2 = re.fullmatch(r"\(\(int64_t\)(\d+)\s*<<\s*(\d+)\)", val)
    if m2:
        return int(m2.group(1)) << int(m2.group(2))
    assert re.fullmatch(r"\d+", val), "%s = %r: neither a number nor ((int64_t)a << b)" % (name, val)
    return int(val)


def consts():
    src = {n: open(p).read() for n, p in (
        ("sets_dev", os.path.join(ENGINE, "sets_dev.hpp")), ("support_dev", os.path.join(ENGINE, "support_dev.hpp")),
        ("host_sets", os.path.join(ENGINE, "host_sets.hpp")), ("host_support", os.path.join(ENGINE, "host_support.hpp")),
        ("coverage_dev", os.path.join(ENGINE, "coverage_dev.hpp")), ("host_coverage", os.path.join(ENGINE, "host_coverage.hpp")),
        ("member_dev", os.path.join(ENGINE, "member_dev.hpp")),
        ("hip", os.path.join(ROOT, "igd_amd", "csrc", "igd_hip.hip")), ("api", os.path.join(ROOT, "include", "igd_hip.h")))}
    c = {}
    for name, where in (("IGD_SETS_SLICES", "host_sets"), ("IGD_SETS_SLICE_MIN", "host_sets"), ("IGD_SETS_SLICE_MAX", "host_sets"),
                        ("IGD_SETS_ROW_BYTES", "host_sets"), ("IGD_SETS_BIG_MIN_DEFAULT", "host_sets"),
                        ("IGD_SETS_GRID", "sets_dev"), ("IGD_SETS_LDS_FILES", "sets_dev"), ("IGD_SETS_WG", "sets_dev"),
                        ("IGD_SUPPORT_LDS_FILES", "support_dev"), ("IGD_SUPPORT_BITS_BYTES", "host_support"),
                        ("IGD_COVERAGE_LDS_FILES", "coverage_dev"), ("IGD_COVERAGE_FRONT_BYTES", "host_coverage"),
                        ("IGD_MEMBER_LDS_FILES", "member_dev"),
                        ("IGD_WAVE", "hip"), ("IGD_HIP_MAX_BATCH_DEFAULT", "api")):
        c[name] = _define(src[where], name)
    return c


def _clamp(x, lo, hi):
    return lo if x < lo else hi if x > hi else x


def plan(set_sizes, nfiles, big_min=None, max_batch=None, row_bytes=None):
    """What igd_hip_search_sets ("search"), igd_hip_support_sets ("support") and igd_hip_coverage_sets ("coverage") make of
    these sets: sliceLen, and per chunk its first set, rows, queries, slices, sets on the batch pipeline (search only) and the
    grid of the slice kernel.  big_min, max_batch, row_bytes: what IGD_SETS_BIG_MIN, IGD_HIP_MAX_BATCH and
    IGD_HIP_SETS_ROW_BYTES are set to (None: the engine's defaults)."""
    c = consts()
    big_min = c["IGD_SETS_BIG_MIN_DEFAULT"] if big_min is None else big_min
    step = c["IGD_HIP_MAX_BATCH_DEFAULT"] if max_batch is None else max_batch
    sizes = [int(n) for n in set_sizes]
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    row_cap = max((c["IGD_SETS_ROW_BYTES"] if row_bytes is None else row_bytes) // (nfiles * 8), 1)
    waves = c["IGD_SETS_WG"] // c["IGD_WAVE"]
    nw = (nfiles + 31) // 32

    def slice_len(n):
        return _clamp(-(-n // c["IGD_SETS_SLICES"]), c["IGD_SETS_SLICE_MIN"], c["IGD_SETS_SLICE_MAX"])

    def chunks(slen, max_grid, with_bigs):
        out, k, pos = [], 0, 0
        while k < len(sizes):
            k0, c0, rows, slices, bigs = k, pos, 0, 0, 0
            while k < len(sizes) and k - k0 < row_cap:
                end = min(off[k + 1], c0 + step)
                rows = k - k0 + 1
                if end > pos:
                    if with_bigs and sizes[k] >= big_min:
                        bigs += 1
                    else:
                        slices += -(-(end - pos) // slen)
                pos = end
                if pos < off[k + 1]:
                    break
                k += 1
            if pos > c0:
                out.append(dict(first=k0, rows=rows, nq=pos - c0, slices=slices, bigs=bigs, grid=min(slices, max_grid)))
        return out

    max_grid = c["IGD_SETS_GRID"]
    if nfiles > c["IGD_SUPPORT_LDS_FILES"]:
        max_grid = _clamp(c["IGD_SUPPORT_BITS_BYTES"] // (nw * 4 * waves), 1, c["IGD_SETS_GRID"])
    cov_lds = nfiles <= c["IGD_COVERAGE_LDS_FILES"]          # (one stripe of nfiles 64-bit words per wave otherwise)
    cov_grid = c["IGD_SETS_GRID"] if cov_lds else _clamp(c["IGD_COVERAGE_FRONT_BYTES"] // (nfiles * 8 * waves), 1, c["IGD_SETS_GRID"])
    s_len = slice_len(sum(n for n in sizes if n < big_min))
    u_len = slice_len(off[-1])
    return dict(rowCap=row_cap, nW=nw,
                search=dict(sliceLen=s_len, lds=nfiles <= c["IGD_SETS_LDS_FILES"], maxGrid=c["IGD_SETS_GRID"],
                            chunks=chunks(s_len, c["IGD_SETS_GRID"], True)),
                support=dict(sliceLen=u_len, lds=nfiles <= c["IGD_SUPPORT_LDS_FILES"], maxGrid=max_grid,
                             chunks=chunks(u_len, max_grid, False)),
                coverage=dict(sliceLen=u_len, lds=cov_lds, maxGrid=cov_grid, chunks=chunks(u_len, cov_grid, False)))


# ---- databases and queries --------------------------------------------------------------------------------------------------
def boundary_files(nfiles):
    """bit 0 and bit 31 of the first, 64th, 65th and last bitmap word, and the files around the last full word"""
    return sorted({f for f in (0, 31, 32, 63, 64, 2047, 2048, nfiles - 33, nfiles - 32, nfiles - 1) if 0 <= f < nfiles})


def wide_db(rng, d, name, nfiles, nbp, span_tiles, gtype=1):
    """One contig.  Per file: one cluster of 2-3 neighbouring records (several records of one file under one query) and one
    record over 3 tiles.  The boundary files also get two records (values 1000 and 900: they pass -v 500) inside `window`.
    Returns (path, span, window, boundary files)."""
    span = nbp * span_tiles
    window = (2 * nbp + 1000, 2 * nbp + 2000)
    edge = set(boundary_files(nfiles))
    files = []
    for f in range(nfiles):
        rows = []
        s = rng.randrange(0, span - 2000)
        for k in range(rng.randint(2, 3)):
            rows.append(("chr1", s + 90 * k, s + 90 * k + rng.randint(20, 400), rng.randint(0, 1000)))
        s = rng.randrange(0, span - 3 * nbp)
        rows.append(("chr1", s, s + 2 * nbp + rng.randint(1, nbp - 1), rng.randint(0, 1000)))
        if f in edge:
            for val in (1000, 900):
                s = window[0] + rng.randrange(0, 400)
                rows.append(("chr1", s, s + rng.randint(50, 500), val))
        files.append(rows)
    path = os.path.join(d, name + ".igd")
    write_igd_numpy(path, files, nbp=nbp, gtype=gtype)
    return path, span, window, sorted(edge)


def scale_queries(rs, nctg, nbp, span, n, window=None, share=8):
    """The kinds of test_gpu_sets._queries -- unknown contigs (-1, 99), inverted, zero-length, one base, multi-tile -- in
    random order, drawn with numpy (rs: numpy Generator).  With a window, about one query in `share` lies on contig 0 and
    covers the whole window."""
    ichr = rs.choice(np.array(list(range(nctg)) + [-1, 99], np.int32), n).astype(np.int32)
    qs = rs.integers(0, span + 3 * nbp, n).astype(np.int64)
    kind = rs.integers(0, 8, n)
    ln = np.choose(kind, [np.zeros(n, np.int64), np.ones(n, np.int64), np.full(n, 200), np.full(n, nbp), np.full(n, 5 * nbp),
                          np.full(n, 9 * nbp + 3), rs.integers(1, 3 * nbp + 1, n), -rs.integers(1, 51, n)])
    qe = qs + ln
    if window is not None:
        pin = rs.integers(0, share, n) == 0
        m = int(pin.sum())
        ichr[pin] = 0
        qs[pin] = window[0] - rs.integers(1, 500, m)
        qe[pin] = window[1] + rs.integers(0, 2000, m)
    return ichr, qs.astype(np.int32), qe.astype(np.int32)


def make_sets(rs, nctg, nbp, span, sizes, window=None, share=8):
    """((ichr, qs, qe) concatenated, off int64[nsets + 1])"""
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    return scale_queries(rs, nctg, nbp, span, int(off[-1]), window, share), off


# ---- case f: 300 000 files (the cut grid of the wide support form) ------------------------------------------------------------
F_FILES = 300000
F_WINDOW = (5 * NBP + 3000, 5 * NBP + 33000)


def f_db(d, nfiles=F_FILES):
    """one short record per file, 100 bp apart; the first and the last file lie in the query window too, with a neighbour
    each (two records of one file under one query: support < hits)"""
    rng = random.Random(16)
    files = []
    for f in range(nfiles):
        s = 100 * f + rng.randrange(0, 60)
        if f == 0 or f == nfiles - 1:
            s = F_WINDOW[0] + 10000 + (f > 0) * 50
        files.append([("chr1", s, s + rng.randint(1, 80), rng.choice([0, 1000]) if 0 < f < nfiles - 1 else 1000)])
        if f == 0 or f == nfiles - 1:
            files[-1].append(("chr1", s + 30, s + 30 + rng.randint(1, 80), 1000))
    path = os.path.join(d, "f.igd")
    write_igd_numpy(path, files, nbp=NBP, gtype=1)
    return path


def f_queries(rs, n):
    """inside the fixed window (which meets about 300 files), a few before and behind it; some inverted or empty"""
    qs = rs.integers(F_WINDOW[0] - 2000, F_WINDOW[1], n)
    ln = np.choose(rs.integers(0, 6, n), [np.zeros(n, np.int64), np.ones(n, np.int64), np.full(n, 200), rs.integers(1, 3000, n),
                                          np.full(n, NBP), -rs.integers(1, 51, n)])
    ichr = rs.choice(np.array([0, 0, 0, 0, 0, 0, -1, 99], np.int32), n).astype(np.int32)
    return ichr, qs.astype(np.int32), (qs + ln).astype(np.int32)


def f_sets():
    # 40 sets of 4 096 queries and one small one: sliceLen = 64, 2 563 slices.  (30 such sets would be 1 920 slices, fewer
    # than the 2 048 workgroups of the full grid: the regime needs more than 32.)
    sizes = [4096] * 40 + [150]
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    return sizes, f_queries(np.random.default_rng(17), int(off[-1])), off


# ---- the expectation --------------------------------------------------------------------------------------------------------
def expected_rows(orc, host, ichr, qs, qe, off, v):
    """Yields per set (hits int64[nfiles], total, support int64[nfiles], nhit), set by set (memory: one set's enumeration).
    hits, total: one Oracle.search call per set.  support, nhit: at v = 0 the oracle's enumeration (distinct (query, idx)
    pairs); at v > 0 igdc_support_host with the command line's rule -- product host code, not the kernels under test, held
    against the oracle in tests/test_support_host.py -- which for sets of at most ANCHOR_MAX queries is checked here, in
    place, against the oracle one query at a time."""
    rule, ev = cli_rule(orc.gtype, v)
    for k in range(len(off) - 1):
        a, b = int(off[k]), int(off[k + 1])
        c, s, e = ichr[a:b], qs[a:b], qe[a:b]
        hits, total = orc.search(c, s, e, v)
        if v == 0:
            sup, nhit = oracle_support_enum(orc, c, s, e)
        else:
            sup, nhit = host.support(c, s, e, ev, rule)
            if b - a <= ANCHOR_MAX:
                w_sup, w_nhit, w_hits = oracle_support(orc, c, s, e, v)
                assert np.array_equal(sup, w_sup) and nhit == w_nhit and np.array_equal(hits, w_hits), (v, k, b - a)
        yield hits, int(total), sup, int(nhit)


class Witness:
    """Non-vacuity, from the expectation alone: support <= hits everywhere and < hits somewhere (a kernel that counted
    pairs would fail); every boundary file has support in at least two sets; some set has 0 < nhit < |set|; some set of at
    most ANCHOR_MAX queries exists (the in-place anchor of expected_rows ran)."""

    def __init__(self, boundary=()):
        self.below = self.partial = self.anchored = False
        self.sets_with = {int(f): 0 for f in boundary}

    def add(self, size, hits, total, sup, nhit):
        assert (sup <= hits).all() and (sup <= size).all() and nhit <= size and total == hits.sum()
        assert (sup > 0).any() == (nhit > 0) and nhit >= (sup.max() if len(sup) else 0)
        self.below |= bool((sup < hits).any())
        self.partial |= 0 < nhit < size
        self.anchored |= 0 < size <= ANCHOR_MAX
        for f in self.sets_with:
            self.sets_with[f] += int(sup[f] > 0)

    def check(self):
        assert self.below, "fixture is vacuous: support equals the pair counts in every set"
        assert self.partial, "fixture is vacuous: no set has 0 < nhit < |set|"
        assert self.anchored, "no set of at most %d queries: igdc_support_host was not held against the oracle" % ANCHOR_MAX
        few = {f: n for f, n in self.sets_with.items() if n < 2}
        assert not few, "boundary files with support in fewer than two sets: %r" % few


# ---- covered base pairs: the expectation --------------------------------------------------------------------------------------
_rows_cache = {}


def cached_rows(path):
    """(read_rows(path), the same per contig sorted by start with its longest record): read once per database file"""
    st = os.stat(path)
    key = (path, st.st_mtime_ns, st.st_size)
    if key not in _rows_cache:
        rows = {c: np.asfortranarray(r) for c, r in read_rows(path).items()}     # (column slices are contiguous)
        srt = {}
        for c, r in rows.items():
            r = r[np.argsort(r[:, 1], kind="stable")]
            srt[c] = (r, int((r[:, 2] - r[:, 1]).max(initial=0)))
        _rows_cache[key] = (rows, srt)
    return _rows_cache[key]


def pair_sums(path, orc, ichr, qs, qe, v):
    """int64[nfiles]: the clipped lengths of all counted (query, record) pairs under rule FLAT with `value >= v`, summed per
    file -- what a kernel that added every record's overlap would return.  The candidates of a query are the records that
    start in [qs - longest record, qe), found by bisection; as in coverage_brute the result is only trusted where the
    same pairs reproduce the oracle's hits."""
    _, srt = cached_rows(path)
    ichr = np.asarray(ichr)
    qs, qe = np.asarray(qs, np.int64), np.asarray(qe, np.int64)
    pairs = np.zeros(orc.nfiles, np.int64)
    hits = np.zeros(orc.nfiles, np.int64)
    use = (ichr >= 0) & (ichr < orc.nctg) & (qs > -orc.nbp) & (qe > qs)
    for c in np.unique(ichr[use]):
        r, longest = srt[int(c)]
        s, e = qs[use & (ichr == c)], qe[use & (ichr == c)]
        a = np.searchsorted(r[:, 1], s - longest, "left")
        n = np.maximum(np.searchsorted(r[:, 1], e, "left") - a, 0)
        qi = np.repeat(np.arange(len(n)), n)
        ri = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(a, n)
        rr = r[ri]
        ok = (rr[:, 2] > s[qi]) & (rr[:, 3] >= v) & (rr[:, 0] >= 0) & (rr[:, 0] < orc.nfiles)
        rr, qi = rr[ok], qi[ok]
        np.add.at(pairs, rr[:, 0], np.minimum(rr[:, 2], e[qi]) - np.maximum(rr[:, 1], s[qi]))
        hits += np.bincount(rr[:, 0], minlength=orc.nfiles)
    want, _ = orc.search(ichr[use], qs[use], qe[use], v)
    assert np.array_equal(hits, want), "INVALID TEST: the pair sums do not reproduce the oracle's hits at v = %d" % v
    return pairs


def expected_cov_rows(path, orc, hostcov, ichr, qs, qe, off, v, named=(), tally=None):
    """Yields per set (coverage int64[nfiles], covered, pair sums int64[nfiles]), one set at a time: the numpy union of
    test_coverage_host allocates queries x files words, so a whole call's queries never go in at once.
    v = 0 (or gType 0): the oracle's enumeration, clipped and united in numpy (coverage_from_enumeration).
    v > 0: igdc_coverage_host (`hostcov`, a test_coverage_host.HostCov) with the command line's rule -- product host code,
    not the kernel under test -- held IN PLACE against coverage_brute on the first COV_ANCHORS non-empty sets, on the first
    set of every distinct size and on every set in `named`; the pair sums come from pair_sums() and, on the anchored sets,
    must equal the brute force's.  tally (a dict) counts the non-empty and the anchored sets for CovWitness.check()."""
    rule, ev = cli_rule(orc.gtype, v)
    flat = orc.gtype != 0 and v > 0
    rows = cached_rows(path)[0] if flat else None
    sizes_seen, anchored, nonempty = set(), 0, 0
    for k in range(len(off) - 1):
        a, b = int(off[k]), int(off[k + 1])
        c, s, e = ichr[a:b], qs[a:b], qe[a:b]
        if not flat:
            cov, covered, pairs = coverage_from_enumeration(orc, c, s, e)
        else:
            cov, covered = hostcov.coverage(c, s, e, ev, rule)
            pairs = pair_sums(path, orc, c, s, e, v)
            nonempty += b > a
            if b > a and (anchored < COV_ANCHORS or (b - a) not in sizes_seen or k in named):
                w_cov, w_covered, w_pairs = coverage_brute(path, orc, c, s, e, v, rows=rows)
                assert np.array_equal(cov, w_cov) and covered == w_covered and np.array_equal(pairs, w_pairs), (v, k, b - a)
                anchored += 1
            sizes_seen.add(b - a)
        yield cov, int(covered), pairs
    if tally is not None and flat:
        tally["nonempty"] = tally.get("nonempty", 0) + nonempty
        tally["anchored"] = tally.get("anchored", 0) + anchored


class CovWitness:
    """Non-vacuity of a coverage fixture, from the expectation alone.  Everywhere: coverage <= the pair sum and <= the set's
    bp, max coverage <= covered <= sum of coverage.  Somewhere: coverage < pair sum (a kernel that summed pairs fails),
    covered > the largest file's coverage (one that took the best file fails), covered < the sum over the files,
    0 < covered < the set's bp; every boundary file has coverage in at least two sets.  With a tally of
    expected_cov_rows (v > 0): at least COV_ANCHORS sets -- or every non-empty set of a fixture that has fewer -- were
    held against the brute force; this is a condition of the test's validity, not a figure."""

    def __init__(self, boundary=()):
        self.below = self.above = self.under = self.partial = False
        self.sets_with = {int(f): 0 for f in boundary}

    def add(self, cov, covered, pairs, bp):
        assert (cov >= 0).all() and (cov <= pairs).all() and (cov <= bp).all()
        assert cov.max(initial=0) <= covered <= min(int(cov.sum()), bp)
        self.below |= bool((cov < pairs).any())
        self.above |= covered > cov.max(initial=0)
        self.under |= covered < cov.sum()
        self.partial |= 0 < covered < bp
        for f in self.sets_with:
            self.sets_with[f] += int(cov[f] > 0)

    def check(self, tally=None):
        assert self.below, "fixture is vacuous: coverage equals the pair sum in every set"
        assert self.above, "fixture is vacuous: covered equals the largest file's coverage in every set"
        assert self.under, "fixture is vacuous: covered equals the sum over the files in every set"
        assert self.partial, "fixture is vacuous: no set has 0 < covered < its bp"
        few = {f: n for f, n in self.sets_with.items() if n < 2}
        assert not few, "boundary files with coverage in fewer than two sets: %r" % few
        if tally is not None:
            need = min(COV_ANCHORS, tally["nonempty"])
            assert need > 0 and tally["anchored"] >= need, \
                "INVALID TEST: igdc_coverage_host was held against the brute force on %d sets, not %d" % (tally["anchored"], need)


# ---- case g: more than 2^32 bp under one file in one slice ------------------------------------------------------------------
BIGBP_Q = (0, 69000000)
BIGBP_HAND = 64 * (69000000 - 1000)            # coverage[0][0] = covered[0] = 4 415 936 000 > 2^32


def bigbp_db(d):
    """One contig, nbp = 2^14, three files.  File 0: one record over [1000, 70 000 000).  File 1: a short record inside it
    and one that starts behind the long query.  File 2: one record behind everything asked."""
    files = [[("chr1", 1000, 70000000, 1000)],
             [("chr1", 10000000, 10000500, 1000), ("chr1", 69500000, 71000000, 1000)],
             [("chr1", 72000000, 72000100, 1000)]]
    path = os.path.join(d, "bigbp.igd")
    write_igd_numpy(path, files, nbp=NBP, gtype=1)
    return path


def bigbp_sets():
    """64 copies of [0, 69 000 000) -- one slice of sliceLen = 64, so one LDS counter gathers 64 x 68 999 000 bp --, then
    one copy, then 64 copies of a 100 bp query: ((ichr, qs, qe), off)"""
    short = (20000000, 20000100)
    qs = np.array([BIGBP_Q[0]] * 65 + [short[0]] * 64, np.int32)
    qe = np.array([BIGBP_Q[1]] * 65 + [short[1]] * 64, np.int32)
    assert BIGBP_HAND == 4415936000 > 1 << 32
    return (np.zeros(129, np.int32), qs, qe), np.array([0, 64, 65, 129], np.int64)
