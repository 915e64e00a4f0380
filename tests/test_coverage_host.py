"""Covered base pairs without a GPU: igdc_coverage_host (igd_hostpath.c) and `igd search -q F -b` / `-Q list -b` on the host route.

    coverage[f] = sum over the queries of | [qs, qe) n union of the records of file f that the query counts |     (bp)
    covered     = the same with the union taken over the records of all files

The expected values never come from the code under test.  Two independent sources:
  1. v = 0 (the command line's rule NEST) and gType 0: the CPU oracle's enumeration (helpers.Oracle.enumerate) gives the
     counted records per query; they are clipped to the query and united per file, and over all files, by sorting and
     sweeping in numpy (union_by_group).
  2. v > 0 on gType 1 (the command line's rule FLAT): brute force `start < qe && end > qs && value >= v` over the database's
     rows, read back from the .igd by this file's own reader (each record once, from the tile it starts in), for the queries
     with a known contig, qs >= 0 and qe > qs (the others cover nothing).  One more kind of query is taken in because the
     golden family "edge" holds one: -nbp < qs < 0, whose first tile is tile 0 by the reference's C division, so it counts
     like any other (qs <= -nbp counts nothing).  Before it is trusted the same brute force must reproduce Oracle.search's
     hits of the same queries at that v -- otherwise the test fails as invalid.
Non-vacuity: coverage <= the pair sum of clipped lengths everywhere and below it somewhere, so a build that summed pairs
fails; covered above the largest row entry somewhere, so one that took the best file fails."""
import ctypes as C
import os
import random
import shutil

import numpy as np
import pytest

from helpers import GOLDEN, Oracle
from test_golden_oracle import CASES, materialize
from test_sets_cli import _case_files, _write_list
from test_support_host import (FLAT, HOST, NEST, NOV, NUMPY_DBS, HostDb, _index, _run, cli_rule, clustered_db, host_threads,  # noqa: F401
                               mixed_queries, sparse_db, tmp)


# ---- expected values ------------------------------------------------------------------------------------------------------
def union_by_group(g, lo, hi, ngroups):
    """int64[ngroups]: per group the length of the union of its intervals [lo, hi) (those with hi <= lo are empty)"""
    g, lo, hi = (np.asarray(a, np.int64) for a in (g, lo, hi))
    keep = hi > lo
    g, lo, hi = g[keep], lo[keep], hi[keep]
    out = np.zeros(ngroups, np.int64)
    if len(g) == 0:
        return out
    o = np.lexsort((lo, g))
    g, lo, hi = g[o], lo[o], hi[o]
    big = np.int64(1) << 34                                   # coordinates are 32-bit: groups cannot meet
    run = np.maximum.accumulate(hi + g * big)                 # running maximum of hi inside each group ...
    prev = np.empty_like(run)
    prev[0] = np.iinfo(np.int64).min
    prev[1:] = run[:-1]
    first = np.ones(len(g), bool)
    first[1:] = g[1:] != g[:-1]
    prev = np.where(first, lo, prev - g * big)                # ... before this interval (a group's first: nothing yet)
    np.add.at(out, g, np.maximum(0, hi - np.maximum(lo, prev)))
    return out


def _reduce(nfiles, qno, idx, lo, hi, nq):
    """(coverage[nfiles], covered, pair sum[nfiles]) from one clipped interval per counted (query, record)"""
    qno, idx, lo, hi = (np.asarray(a, np.int64) for a in (qno, idx, lo, hi))
    ok = (idx >= 0) & (idx < nfiles)
    qno, idx, lo, hi = qno[ok], idx[ok], lo[ok], hi[ok]
    per = union_by_group(qno * nfiles + idx, lo, hi, max(nq, 1) * nfiles).reshape(-1, nfiles).sum(axis=0)
    covered = int(union_by_group(qno, lo, hi, max(nq, 1)).sum())
    pairs = np.zeros(nfiles, np.int64)
    np.add.at(pairs, idx, np.maximum(0, hi - lo))
    return per, covered, pairs


def coverage_from_enumeration(orc, ichr, qs, qe):
    """source 1: rule NEST, no filter"""
    qs, qe = np.asarray(qs, np.int64), np.asarray(qe, np.int64)
    qoff, rec = orc.enumerate(ichr, qs, qe)
    qno = np.repeat(np.arange(len(qs), dtype=np.int64), np.diff(qoff))
    rec = rec.astype(np.int64)
    return _reduce(orc.nfiles, qno, rec[:, 0], np.maximum(rec[:, 1], qs[qno]), np.minimum(rec[:, 2], qe[qno]), len(qs))


def read_rows(path):
    """{contig number: int64[n, 4] (idx, start, end, value)}: every record of the .igd once, from the tile it starts in"""
    raw = np.fromfile(path, np.int32)
    nbp, gtype, nctg = (int(x) for x in raw[:3])
    ntile = raw[3:3 + nctg].astype(np.int64)
    p = 3 + nctg
    cnt = raw[p:p + ntile.sum()].astype(np.int64)
    p += int(ntile.sum()) + 10 * nctg                          # (40 bytes of name per contig)
    w = 4 if gtype == 1 else 3
    rows, t = {}, 0
    for c in range(nctg):
        parts = []
        for j in range(int(ntile[c])):
            n = int(cnt[t])
            t += 1
            if n:
                r = raw[p:p + n * w].reshape(n, w).astype(np.int64)
                p += n * w
                parts.append(r[r[:, 1] // nbp == j])
        r = np.concatenate(parts) if parts else np.zeros((0, w), np.int64)
        if w == 3:
            r = np.concatenate([r, np.zeros((len(r), 1), np.int64)], axis=1)
        rows[c] = r
    return rows


def coverage_brute(path, orc, ichr, qs, qe, v, rows=None):
    """source 2: rule FLAT with the filter `value >= v` on gType 1  (rows: read_rows(path), for callers that keep it)"""
    rows = read_rows(path) if rows is None else rows
    qs, qe = np.asarray(qs, np.int64), np.asarray(qe, np.int64)
    use = [i for i in range(len(qs)) if 0 <= ichr[i] < orc.nctg and qs[i] > -orc.nbp and qe[i] > qs[i]]
    qno, idx, lo, hi = [], [], [], []
    for i in use:
        r = rows[int(ichr[i])]
        r = r[(r[:, 1] < qe[i]) & (r[:, 2] > qs[i]) & (r[:, 3] >= v)]
        qno.append(np.full(len(r), i, np.int64))
        idx.append(r[:, 0])
        lo.append(np.maximum(r[:, 1], qs[i]))
        hi.append(np.minimum(r[:, 2], qe[i]))
    cat = [np.concatenate(a) if a else np.zeros(0, np.int64) for a in (qno, idx, lo, hi)]
    # the brute force is only trusted where it reproduces the oracle's counts of the same queries at this v
    hits = np.bincount(cat[1][(cat[1] >= 0) & (cat[1] < orc.nfiles)], minlength=orc.nfiles)
    u = np.array(use, np.int64)
    want, _ = orc.search(np.asarray(ichr)[u], qs[u], qe[u], v)
    assert np.array_equal(hits, want), "INVALID TEST: the brute force does not reproduce the oracle's hits at v = %d" % v
    return _reduce(orc.nfiles, *cat, len(qs))


def expected_coverage(path, orc, ichr, qs, qe, v):
    """what `-q ... -b -v V` must give: (coverage, covered, pair sum)"""
    if orc.gtype != 0 and v > 0:
        return coverage_brute(path, orc, ichr, qs, qe, v)
    return coverage_from_enumeration(orc, ichr, qs, qe)


def query_bp(qs, qe):
    d = np.asarray(qe, np.int64) - np.asarray(qs, np.int64)
    return int(d[d > 0].sum())


class HostCov(HostDb):
    def coverage(self, ichr, qs, qe, v, rule, coverage=None, covered0=0):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        cov = np.zeros(self.nfiles, np.int64) if coverage is None else coverage
        covered = C.c_int64(covered0)
        rc = self.L.igdc_coverage_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), v, rule,
                                       cov.ctypes.data, C.byref(covered))
        assert rc == 0
        return cov, covered.value


def check_bounds(cov, covered, pairs, qs, qe):
    assert (cov <= pairs).all() and (cov <= query_bp(qs, qe)).all()
    assert cov.max(initial=0) <= covered <= cov.sum()


# ---- the helper itself, by hand -------------------------------------------------------------------------------------------
def test_union_by_group_by_hand():
    #        group 0: [0,10) [5,8) [8,20) -> 20; [30,30) empty; group 2: [1,2) [1,2) [2,3) -> 2; group 1: nothing
    g = [0, 2, 0, 2, 0, 0, 2]
    lo = [5, 1, 0, 1, 8, 30, 2]
    hi = [8, 2, 10, 2, 20, 30, 3]
    assert union_by_group(g, lo, hi, 3).tolist() == [20, 0, 2]
    assert union_by_group([1], [100], [1000], 2).tolist() == [0, 900]
    assert union_by_group([0, 0], [200, 100], [300, 1000], 1).tolist() == [900]          # a later container loses nothing
    assert union_by_group([], [], [], 2).tolist() == [0, 0]


# ---- igdc_coverage_host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_host_coverage_equals_the_helper_on_the_golden_families(case, host_threads):
    d, dst, man = materialize(case)
    try:
        path = os.path.join(dst, "db.igd")
        orc = Oracle(path)
        ichr, qs, qe = orc.read_queries(os.path.join(dst, "q.bed"))
        if len(qs) > 3000:
            ichr, qs, qe = ichr[:3000], qs[:3000], qe[:3000]
        H = HostCov(path)
        for v in (0, 500):
            want, wcovered, pairs = expected_coverage(path, orc, ichr, qs, qe, v)
            print(case, "v", v, "coverage", int(want.sum()), "pairs", int(pairs.sum()), "covered", wcovered, "of", query_bp(qs, qe))
            check_bounds(want, wcovered, pairs, qs, qe)
            rule, ev = cli_rule(orc.gtype, v)
            for threads in ("1", "3", "7"):
                host_threads(threads)
                got, covered = H.coverage(ichr, qs, qe, ev, rule)
                assert np.array_equal(got, want), (case, v, threads)
                assert covered == wcovered
        H.close()
        orc.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_coverage_equals_the_helper_on_clustered_databases(case, tmp, host_threads):
    rng = random.Random(4100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    path, span = clustered_db(rng, tmp, "c%d" % case, nbp, gtype, nfiles, nctg, span_tiles)
    ichr, qs, qe = mixed_queries(rng, nctg, nbp, span, 1500)
    orc = Oracle(path)
    H = HostCov(path)
    try:
        for v in (0, 500):
            want, wcovered, pairs = expected_coverage(path, orc, ichr, qs, qe, v)
            check_bounds(want, wcovered, pairs, qs, qe)
            assert (want < pairs).any(), "fixture is vacuous: no two counted records of a file overlap under a query"
            assert want.max() < wcovered < want.sum()
            rule, ev = cli_rule(gtype, v)
            for threads in ("1", "3", "7"):
                host_threads(threads)
                got, covered = H.coverage(ichr, qs, qe, ev, rule)
                assert np.array_equal(got, want) and covered == wcovered, (case, v, threads)
        # ADDED to the caller's vector and counter; the empty call
        base = np.arange(nfiles, dtype=np.int64) * 100
        rule, ev = cli_rule(gtype, 0)
        want, wcovered, _ = expected_coverage(path, orc, ichr, qs, qe, 0)
        got, covered = H.coverage(ichr, qs, qe, ev, rule, coverage=base.copy(), covered0=11)
        assert np.array_equal(got, base + want) and covered == 11 + wcovered
        got, covered = H.coverage(ichr[:0], qs[:0], qe[:0], ev, rule)
        assert not got.any() and covered == 0
    finally:
        H.close()
        orc.close()


def test_explicit_rules_on_a_sparse_database(tmp, host_threads):
    rng = random.Random(4200)
    path, span, nbp = sparse_db(rng, tmp)
    ichr, qs, qe = mixed_queries(rng, 2, nbp, span, 2000)
    orc = Oracle(path)
    H = HostCov(path)
    try:
        nest, nest_c, _ = coverage_from_enumeration(orc, ichr, qs, qe)
        flat, flat_c, _ = coverage_brute(path, orc, ichr, qs, qe, 1)            # values >= 1: rule FLAT, every record passes
        flat5, flat5_c, _ = coverage_brute(path, orc, ichr, qs, qe, 500)
        assert not np.array_equal(nest, flat) and nest_c < flat_c, "the two rules do not differ on this fixture"
        for threads in ("1", "3", "7"):
            host_threads(threads)
            for v, rule, want, wc in ((NOV, NEST, nest, nest_c), (NOV, FLAT, flat, flat_c), (1, FLAT, flat, flat_c),
                                      (500, FLAT, flat5, flat5_c)):
                got, covered = H.coverage(ichr, qs, qe, v, rule)
                assert np.array_equal(got, want) and covered == wc, (threads, v, rule)
    finally:
        H.close()
        orc.close()


# ---- command line ---------------------------------------------------------------------------------------------------------
def expected_table(db, orc, qfile, v):
    """the text of `igd search db -q qfile -b [-v v]`, from the helper"""
    try:
        ichr, qs, qe = orc.read_queries(qfile)
    except IOError:
        ichr = qs = qe = np.zeros(0, np.int32)
    cov, covered, _ = expected_coverage(db, orc, ichr, qs, qe, v)
    out = "index\t number of regions\t covered bp\t File_name\n"
    for i, (nr, name) in enumerate(_index(db)):
        if cov[i] > 0:
            out += "%d\t%d\t%d\t%s\n" % (i, nr, cov[i], name)
    return out + "Query bp with a hit: %d of %d\n" % (covered, query_bp(qs, qe))


CLI_CASES = [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("gtype0", ["-v", "500"]), ("edge", []), ("edge", ["-v", "500"])]


@pytest.mark.parametrize("case,extra", CLI_CASES)
def test_cli_b_prints_the_helpers_coverage_on_the_host_route(case, extra, tmp):
    db = os.path.join(GOLDEN, case, "db.igd")
    v = int(extra[1]) if extra else 0
    orc = Oracle(db)
    try:
        files = _case_files(case)
        q = files[0]
        for args in (["-q", q, "-b"] + extra, ["-b"] + extra + ["-q", q]):
            got = _run(["search", db] + args, HOST)
            assert got.returncode == 0, got.stderr
            assert got.stdout.decode() == expected_table(db, orc, q, v), args
        files = files + [os.path.join(tmp, "missing.bed")]
        lst = _write_list(tmp, files, crlf=True)
        got = _run(["search", db, "-Q", lst, "-b"] + extra, HOST)
        assert got.returncode == 0, got.stderr
        want = "".join("Query set %d: %s\n" % (k, p) + expected_table(db, orc, p, v) for k, p in enumerate(files))
        assert got.stdout.decode() == want
        assert "Total:" not in want and want.count("Query bp with a hit:") == len(files) and "\t covered bp\t" in want
    finally:
        orc.close()


@pytest.mark.parametrize("other", [["-q", "Q", "-f"], ["-r", "chr1", "1000", "90000"], ["-r", "chr1", "1000", "90000", "-f"],
                                   ["-r", "chr1", "1000", "90000", "-v", "300"], ["-f"], ["-c"], ["-r", "chr1", "1000", "90000", "-u"]])
def test_b_has_no_effect_on_the_other_command_lines(other, tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    other = [q if a == "Q" else a for a in other]
    want = _run(["search", db] + other, HOST)
    for args in (["-b"] + other, other + ["-b"]):
        got = _run(["search", db] + args, HOST)
        assert (got.returncode, got.stdout) == (want.returncode, want.stdout), args


def test_b_together_with_u_is_refused(tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    lst = _write_list(tmp, _case_files("branch"))
    for args in (["-q", q, "-b", "-u"], ["-u", "-b", "-q", q, "-v", "500"], ["-Q", lst, "-u", "-b"]):
        got = _run(["search", db] + args, HOST)
        assert got.returncode == 0
        out = got.stdout.decode()
        assert out.count("\n") == 1 and "-b" in out and "-u" in out and "index\t" not in out, args
    # each of them alone still prints its table
    u = _run(["search", db, "-q", q, "-u"], HOST).stdout.decode()
    b = _run(["search", db, "-q", q, "-b"], HOST).stdout.decode()
    assert "\t number of query regions\t" in u and u.splitlines()[-1].startswith("Query regions with a hit: ")
    assert "\t covered bp\t" in b and b.splitlines()[-1].startswith("Query bp with a hit: ")


def test_engine_route_without_a_device_fails_loudly(tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    nodev = {"IGD_HOST_MAX_QUERIES": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
    lst = _write_list(tmp, _case_files("branch"))
    for args in (["-q", q, "-b"], ["-q", q, "-b", "-v", "500"], ["-Q", lst, "-b"]):
        got = _run(["search", db] + args, nodev)
        assert got.returncode == 69 and b"no CPU search path" in got.stderr, args
        assert b"index\t" not in got.stdout and b"Query bp" not in got.stdout and b"Query set" not in got.stdout
