"""GPU: igd_sets_coverage (Database.coverage_sets / coverage) beyond one slice per workgroup and at the edges of its LDS form.

tests/test_gpu_coverage.py holds every row against the two sources of tests/test_coverage_host.py on every awkward query
kind, but its fixtures have sliceLen = 64, fewer slices than workgroups, and at most 40 files or 20 000.  This kernel keeps
more between a workgroup's slices than any other: per-wave frontier words that are valid only under a tag that must keep
rising from slice to slice (and, in the wide form, from launch to launch), 64-bit LDS counters and the lcov[0] word, flushed
and cleared per slice, and more than 64 KiB of dynamic LDS from 1 639 files up.  The cases:

    a  several slices per workgroup: the persistent loop, the counter and lcov[0] clear after a flush, the tag carried on
    b  sliceLen strictly between its bounds, shorter last slices, more slices than workgroups
    d  file counts around 64 KiB of dynamic LDS (1 638 / 1 639), the benchmark's 1 900, IGD_COVERAGE_LDS_FILES (2 039,
       2 040) and the first wide form (2 041)
    e  the row cap ends a chunk (20 000 files)
    w  the cut grid of the wide form: more slices than workgroups, so a wave reuses its global stripe within one launch,
       between launches of other grids and other tags on the same handle
    g  more than 2^32 bp gathered by one LDS counter in one slice

Every case asserts through sets_fixtures.plan()["coverage"] that it is in the regime it claims, checks coverage_sets row by
row, and covered[], against sets_fixtures.expected_cov_rows() for v = 0 and v = 500 -- no expectation comes from the kernel
-- asserts the fixture's non-vacuity on the expectation alone (sets_fixtures.CovWitness; case g's witness is its hand
values: one record per file under a query leaves nothing for a union to merge), checks coverage > 0 exactly where
support_sets > 0 over the queries with qe > qs, and repeats the call: the second one must return the same matrices.

Not covered, on purpose.  The tag wrap of coverage_fronts (host_coverage.hpp) needs 2^32 queries on one handle, and a hook
that started the tags high could not show a missing reset either: a stale tag only collides with a live one a full 2^32
queries later.  sliceLen at its cap needs 1.7 x 10^7 queries and reaches nothing in this kernel that case b does not: its
counters are 64-bit (case g is the test of that), so the slice length bounds nothing here."""
import os
import random
import shutil

import numpy as np
import pytest

import sets_fixtures as F
from helpers import Oracle, short_tmpdir
from test_coverage_host import HostCov, query_bp
from test_gpu_sets import DBS, SIZES, _db

pytestmark = pytest.mark.gpu

NBP = F.NBP


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igy")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(autouse=True)
def _default_seams():
    assert "IGD_HIP_MAX_BATCH" not in os.environ        # (read once per process: the seams of plan() are the default ones)


_wide = {}


def wide(workdir, nfiles):
    """the wide_db of `nfiles` files, written once per module: (path, span, window, boundary files)"""
    if nfiles not in _wide:
        _wide[nfiles] = F.wide_db(random.Random(7000 + nfiles), workdir, "w%d" % nfiles, nfiles, NBP, max(40, nfiles * 3 // 10))
    return _wide[nfiles]


def check(path, ichr, qs, qe, off, boundary=(), vs=(0, 500), prefill=False, must_hit=(), witness=True, db=None, between=None):
    """coverage_sets against expected_cov_rows, row by row, and covered[]; CovWitness on the expectation; coverage > 0 exactly
    where support_sets > 0 over the queries with qe > qs; the second call (into a pre-filled matrix when `prefill`) must add
    the same numbers.  must_hit: sets that are anchored by name and whose expected rows must be non-zero.  db: an open
    Database to use (and leave open).  between(db, v): called before a third call, which must again return the same."""
    from igd_amd import Database
    nsets = len(off) - 1
    orc, H = Oracle(path), HostCov(path)
    own = db is None
    db = Database(path) if own else db
    try:
        keep = qe > qs
        koff = np.concatenate([[0], np.cumsum([int(keep[off[k]:off[k + 1]].sum()) for k in range(nsets)])]).astype(np.int64)
        for v in vs:
            cov, covered = db.coverage_sets(ichr, qs, qe, off, v)
            assert cov.shape == (nsets, orc.nfiles) and covered.shape == (nsets,) and cov.dtype == covered.dtype == np.int64
            W, tally = F.CovWitness(boundary), {}
            for k, (e_cov, e_covered, pairs) in enumerate(F.expected_cov_rows(path, orc, H, ichr, qs, qe, off, v, must_hit, tally)):
                a, b = int(off[k]), int(off[k + 1])
                assert np.array_equal(cov[k], e_cov), ("coverage_sets", v, k, b - a)
                assert covered[k] == e_covered, ("covered", v, k, b - a, int(covered[k]), e_covered)
                W.add(e_cov, e_covered, pairs, query_bp(qs[a:b], qe[a:b]))
                if k in must_hit:
                    assert e_cov.any() and e_covered > 0, "set %d should have a non-zero expected row" % k
            if witness:
                W.check(tally if v else None)
            # an inverted or empty query can count a record that contains both of its ends; it covers nothing
            c2, n2 = db.coverage_sets(ichr[keep], qs[keep], qe[keep], koff, v)
            s2, _ = db.support_sets(ichr[keep], qs[keep], qe[keep], koff, v)
            assert np.array_equal(c2, cov) and np.array_equal(n2, covered), ("queries with qe <= qs cover something", v)
            assert np.array_equal(c2 > 0, s2 > 0), ("coverage > 0 where support > 0", v)
            del c2, s2
            if prefill:
                base = (np.arange(nsets, dtype=np.int64)[:, None] * 7 + np.arange(orc.nfiles, dtype=np.int64)[None, :] % 5)
                again, n2 = db.coverage_sets(ichr, qs, qe, off, v, coverage=base.copy())
                again -= base
            else:
                again, n2 = db.coverage_sets(ichr, qs, qe, off, v)
            assert np.array_equal(again, cov) and np.array_equal(n2, covered), ("coverage_sets, second call", v)
            if between is not None:
                between(db, v)
                again, n2 = db.coverage_sets(ichr, qs, qe, off, v)
                assert np.array_equal(again, cov) and np.array_equal(n2, covered), ("coverage_sets, after other launches", v)
            del again, cov
    finally:
        H.close()
        if own:
            db.close()
        orc.close()


# ---- a ----------------------------------------------------------------------------------------------------------------------
A_SIZES = [0, 1, 63, 64, 65, 70, 130] * 300             # 2 100 sets, 117 900 queries, 3 000 slices


@pytest.mark.parametrize("which", ["d0", "w1900", "w2040"])
def test_a_several_slices_per_workgroup(which, workdir):
    """sliceLen = 64 and 3 000 slices against 2 048 workgroups in one chunk: 952 workgroups take a second slice, with the
    frontier words, counters and lcov[0] their first slice left.  On the hot tile of DBS[0], whose same-file collisions fill
    the ordered path; on 1 900 files, the benchmark's LDS size; and on 2 040 files, the largest LDS launch."""
    c = F.consts()
    if which == "d0":
        nbp, gtype, nfiles, nctg, span_tiles, dens, hot = DBS[0]
        assert hot > 512
        path, span = _db(random.Random(900), workdir, "a_d0", nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
        window, boundary = None, ()
    else:
        nfiles, nctg, nbp = int(which[1:]), 1, NBP
        path, span, window, boundary = wide(workdir, nfiles)
    p = F.plan(A_SIZES, nfiles)["coverage"]
    assert p["sliceLen"] == c["IGD_SETS_SLICE_MIN"] == 64 and p["lds"] and nfiles <= c["IGD_COVERAGE_LDS_FILES"]
    (ch,) = p["chunks"]
    assert ch["slices"] == 3000 > ch["grid"] == c["IGD_SETS_GRID"] == 2048 and ch["nq"] == 117900
    (ichr, qs, qe), off = F.make_sets(np.random.default_rng(21), nctg, nbp, span, A_SIZES, window)
    check(path, ichr, qs, qe, off, boundary)


# ---- b ----------------------------------------------------------------------------------------------------------------------
def test_b_slice_len_between_the_bounds(workdir):
    """120 sets of 2 400-2 600 queries (3 x 10^5 in all) on 1 900 files, plus three small sets: 64 < sliceLen < 4096, the last
    slice of a set shorter than the others, more slices than workgroups."""
    c = F.consts()
    rs = np.random.default_rng(22)
    sizes = [int(n) for n in rs.integers(2400, 2601, 120)] + [0, 300, 1500]
    path, span, window, boundary = wide(workdir, 1900)
    p = F.plan(sizes, 1900)["coverage"]
    slen = p["sliceLen"]
    assert c["IGD_SETS_SLICE_MIN"] < slen == 74 < c["IGD_SETS_SLICE_MAX"] and p["lds"]
    (ch,) = p["chunks"]
    assert ch["slices"] > ch["grid"] == c["IGD_SETS_GRID"] == 2048
    assert sum(1 for n in sizes[:120] if n % slen) >= 108               # a shorter last slice
    (ichr, qs, qe), off = F.make_sets(rs, 1, NBP, span, sizes, window)
    check(path, ichr, qs, qe, off, boundary)


# ---- d ----------------------------------------------------------------------------------------------------------------------
def lds_bytes(nfiles, c):
    """the dynamic LDS of an LDS-form launch: lcov[2], then a counter and one frontier word per wave for every file"""
    return (2 + nfiles * (1 + c["IGD_SETS_WG"] // c["IGD_WAVE"])) * 8


@pytest.mark.parametrize("nfiles", [1638, 1639, 1900, 2039, 2040, 2041])
def test_d_file_count_edges(nfiles, workdir):
    """1 638 files ask for exactly 65 536 B of dynamic LDS, the last launch that gets it unasked; 1 639 is the first that
    needs hipFuncSetAttribute, whose result the host does not look at: a clean launch and exact rows are the assertion.
    1 900 is the benchmark's size, 2 040 (81 616 B) the largest LDS launch, 2 041 the first wide form."""
    c = F.consts()
    sizes = SIZES + [4097]
    p = F.plan(sizes, nfiles)["coverage"]
    assert c["IGD_COVERAGE_LDS_FILES"] == 2040 and p["lds"] == (nfiles <= 2040) and len(p["chunks"]) == 1
    assert lds_bytes(1638, c) == 65536 and lds_bytes(1639, c) > 65536
    assert lds_bytes(1900, c) == 76016 and lds_bytes(c["IGD_COVERAGE_LDS_FILES"], c) == 81616
    path, span, window, boundary = wide(workdir, nfiles)
    (ichr, qs, qe), off = F.make_sets(np.random.default_rng(24), 1, NBP, span, sizes, window)
    check(path, ichr, qs, qe, off, boundary)


# ---- e ----------------------------------------------------------------------------------------------------------------------
def test_e_row_cap_ends_a_chunk(workdir):
    """20 000 files, rowCap + 40 sets of 0-3 queries and three of 300: the device rows of one chunk are full before its
    queries are.  The sets on either side of the border cover the window (non-zero rows, anchored by name), and a
    pre-filled matrix is added to across the border."""
    nfiles = 20000
    cap = F.plan([1], nfiles)["rowCap"]
    rs = np.random.default_rng(25)
    sizes = [int(n) for n in rs.integers(0, 4, cap + 40)]
    for k in (5, cap - 7, cap + 20):
        sizes[k] = 300
    sizes[cap - 1] = sizes[cap] = 3
    p = F.plan(sizes, nfiles)["coverage"]
    assert [(ch["first"], ch["rows"]) for ch in p["chunks"]] == [(0, cap), (cap, 40)] and not p["lds"]
    path, span, window, boundary = wide(workdir, nfiles)
    (ichr, qs, qe), off = F.make_sets(rs, 1, NBP, span, sizes, window)
    a, b = int(off[cap - 1]), int(off[cap + 1])                         # the border sets: every query covers the window
    ichr[a:b], qs[a:b], qe[a:b] = F.scale_queries(rs, 1, NBP, span, b - a, window, share=1)
    check(path, ichr, qs, qe, off, boundary, prefill=True, must_hit=(cap - 1, cap))


# ---- w ----------------------------------------------------------------------------------------------------------------------
W_SIZES = [0, 1, 63, 64, 65, 70, 130] * 90              # 630 sets, 35 370 queries, 900 slices


def test_w_cut_grid_of_the_wide_form(workdir):
    """20 000 files: the stripes of a full grid would pass IGD_COVERAGE_FRONT_BYTES, so 419 workgroups take 900 slices and
    every wave reuses its global stripe for a second slice in one launch.  A launch of 10 slices on the same handle comes
    first and a launch of other queries comes before the third call, so the stripes hold stale words of launches with
    other grids and other tags.  The three results must be equal and exact."""
    from igd_amd import Database
    c = F.consts()
    nfiles = 20000
    p = F.plan(W_SIZES, nfiles)["coverage"]
    (ch,) = p["chunks"]
    assert not p["lds"] and p["sliceLen"] == 64 and p["maxGrid"] == 419 < c["IGD_SETS_GRID"]
    assert ch["slices"] == 900 > 2 * ch["grid"] == 838 and ch["nq"] == 35370
    assert p["maxGrid"] * 4 * nfiles * 8 <= c["IGD_COVERAGE_FRONT_BYTES"] < (p["maxGrid"] + 1) * 4 * nfiles * 8
    path, span, window, boundary = wide(workdir, nfiles)
    (ichr, qs, qe), off = F.make_sets(np.random.default_rng(26), 1, NBP, span, W_SIZES, window)
    small = [0, 1, 64, 65, 300, 33]
    (s_ichr, s_qs, s_qe), s_off = F.make_sets(np.random.default_rng(27), 1, NBP, span, small, window)
    (ch,) = F.plan(small, nfiles)["coverage"]["chunks"]
    assert ch["slices"] == ch["grid"] == 10
    (o_ichr, o_qs, o_qe), o_off = F.make_sets(np.random.default_rng(28), 1, NBP, span, [500, 129, 2], window)

    def other_queries(db, v):
        got, _ = db.coverage_sets(o_ichr, o_qs, o_qe, o_off, v)
        assert got.any()

    db = Database(path)
    try:
        first, _ = db.coverage_sets(s_ichr, s_qs, s_qe, s_off, 0)
        assert first.any()
        check(path, ichr, qs, qe, off, boundary, db=db, between=other_queries)
    finally:
        db.close()


# ---- g ----------------------------------------------------------------------------------------------------------------------
def test_g_more_than_2_32_bp_in_one_slice(workdir):
    """64 copies of a 69 Mbp query under one 70 Mbp record are one slice, and its LDS counter of file 0 gathers
    64 x 68 999 000 = 4 415 936 000 bp: a 32-bit counter would return 120 968 704.  covered[0] is the same number."""
    from igd_amd import Database
    path = F.bigbp_db(workdir)
    (ichr, qs, qe), off = F.bigbp_sets()
    p = F.plan(np.diff(off), 3)["coverage"]
    assert p["sliceLen"] == 64 and p["lds"] and p["chunks"][0]["slices"] == 3 and off[1] == 64
    check(path, ichr, qs, qe, off, witness=False)
    db = Database(path)
    try:
        for v in (0, 500):
            cov, covered = db.coverage_sets(ichr, qs, qe, off, v)
            assert cov[0].tolist() == [F.BIGBP_HAND, 64 * 500, 0] and covered[0] == F.BIGBP_HAND > 1 << 32
            assert cov[1].tolist() == [68999000, 500, 0] and cov[2].tolist() == [6400, 0, 0]
            one, n = db.coverage(ichr, qs, qe, v)
            assert one.tolist() == [65 * 68999000 + 6400, 65 * 500, 0] and n == 65 * 68999000 + 6400
    finally:
        db.close()
