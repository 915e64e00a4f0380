"""GPU: igd_sets_count and igd_sets_support (Database.search_sets / support_sets) beyond one slice per workgroup.

tests/test_gpu_sets.py and tests/test_gpu_support.py hold every row against the oracle on every awkward query kind, but all
their fixtures have sliceLen = 64 and as many workgroups as slices.  The cases here reach the rest of the work decomposition:

    a  several slices per workgroup (the persistent loop, the counter clear after a flush, lhit, the bitmaps between slices)
    b  sliceLen strictly between its bounds, slices and batch-pipeline sets in one chunk
    c  sliceLen at its cap (the 32-bit LDS counters of igd_sets_support) and the default batch seam of 2^24 queries
    d  file counts at the edges of the LDS forms: 1 900, 2 081 (66 bitmap words), 8 191, 8 192 (64 KiB of LDS), 8 193
    e  the row cap ends a chunk
    f  the cut grid of the wide support form (300 000 files)

Every case asserts through sets_fixtures.plan() that it is in the regime it claims, checks both entry points row by row
against sets_fixtures.expected_rows() for v = 0 and v = 500 -- no expectation comes from the kernels -- asserts the
fixture's non-vacuity on the expectation alone (sets_fixtures.Witness), and repeats each call: the second one must return
the same matrices (counters, lhit, bitmaps and stripes were left clear)."""
import hashlib
import os
import random
import shutil

import numpy as np
import pytest

import sets_fixtures as F
from helpers import Oracle, short_tmpdir
from test_gpu_sets import DBS, SIZES, _db
from test_support_host import HostDb

pytestmark = pytest.mark.gpu

NBP = F.NBP


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igx")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(autouse=True)
def _default_routes(monkeypatch):
    monkeypatch.delenv("IGD_SETS_BIG_MIN", raising=False)
    assert "IGD_HIP_MAX_BATCH" not in os.environ        # (read once per process: the seams of plan() are the default ones)


_wide = {}


def wide(workdir, nfiles, span_tiles=None):
    """the wide_db of `nfiles` files, written once per module: (path, span, window, boundary files)"""
    if nfiles not in _wide:
        _wide[nfiles] = F.wide_db(random.Random(7000 + nfiles), workdir, "w%d" % nfiles, nfiles, NBP,
                                  span_tiles or max(40, nfiles * 3 // 10))
    return _wide[nfiles]


def _digest(path, ichr, qs, qe, off):
    h = hashlib.sha256(open(path, "rb").read())
    for a in (ichr, qs, qe, off):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def check(path, ichr, qs, qe, off, boundary=(), vs=(0, 500), prefill=False, must_hit=(), expect_cache=None):
    """Both entry points against expected_rows, row by row; the second call (into a pre-filled matrix when `prefill`) must
    add the same numbers.  must_hit: sets whose expected hits and support rows must be non-zero.  expect_cache: a dict
    that keeps the expected rows per v for a later call -- with a digest of the database and the queries, which that call
    must present again."""
    from igd_amd import Database
    nsets = len(off) - 1
    orc, H, db = Oracle(path), HostDb(path), Database(path)
    try:
        for v in vs:
            hits, tot = db.search_sets(ichr, qs, qe, off, v)
            sup, nhit = db.support_sets(ichr, qs, qe, off, v)
            assert hits.shape == sup.shape == (nsets, orc.nfiles) and tot.shape == nhit.shape == (nsets,)
            if expect_cache is not None and v in expect_cache:
                digest, rows = expect_cache[v]
                assert digest == _digest(path, ichr, qs, qe, off), "cached expectation of other queries or another database"
            else:
                rows = F.expected_rows(orc, H, ichr, qs, qe, off, v)
                if expect_cache is not None:
                    rows = list(rows)
                    expect_cache[v] = (_digest(path, ichr, qs, qe, off), rows)
            W = F.Witness(boundary)
            for k, (e_hits, e_tot, e_sup, e_nhit) in enumerate(rows):
                size = int(off[k + 1] - off[k])
                assert np.array_equal(hits[k], e_hits), ("search_sets", v, k, size)
                assert tot[k] == e_tot, ("search_sets totals", v, k, size)
                assert np.array_equal(sup[k], e_sup), ("support_sets", v, k, size)
                assert nhit[k] == e_nhit, ("support_sets nhit", v, k, size)
                W.add(size, e_hits, e_tot, e_sup, e_nhit)
                if k in must_hit:
                    assert e_hits.any() and e_sup.any(), "set %d should have non-zero expected rows" % k
            W.check()
            if prefill:
                base = (np.arange(nsets, dtype=np.int64)[:, None] * 7 + np.arange(orc.nfiles, dtype=np.int64)[None, :] % 5)
                again, tot2 = db.search_sets(ichr, qs, qe, off, v, hits=base.copy())
                again -= base
                assert np.array_equal(again, hits) and np.array_equal(tot2, tot), ("search_sets into a pre-filled matrix", v)
                again, nhit2 = db.support_sets(ichr, qs, qe, off, v, support=base.copy())
                again -= base
                assert np.array_equal(again, sup) and np.array_equal(nhit2, nhit), ("support_sets into a pre-filled matrix", v)
            else:
                again, tot2 = db.search_sets(ichr, qs, qe, off, v)
                assert np.array_equal(again, hits) and np.array_equal(tot2, tot), ("search_sets, second call", v)
                again, nhit2 = db.support_sets(ichr, qs, qe, off, v)
                assert np.array_equal(again, sup) and np.array_equal(nhit2, nhit), ("support_sets, second call", v)
            del again, hits, sup
    finally:
        H.close()
        db.close()
        orc.close()


# ---- a ----------------------------------------------------------------------------------------------------------------------
A_SIZES = [0, 1, 63, 64, 65, 70, 200] * 429            # 3 003 sets, 198 627 queries


@pytest.mark.parametrize("which", ["d0", "w1900", "w20000"])
def test_a_several_slices_per_workgroup(which, workdir):
    """sliceLen = 64 and more slices than workgroups in every chunk: a workgroup takes a second and a third slice.  On the hot
    tile of DBS[0], on 1 900 files (the benchmark's count) and on the wide form, where 20 000 files also cut the call into
    two chunks."""
    c = F.consts()
    if which == "d0":
        nbp, gtype, nfiles, nctg, span_tiles, dens, hot = DBS[0]
        assert hot > 512
        path, span = _db(random.Random(900), workdir, "a_d0", nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
        window, boundary = None, ()
    else:
        nfiles, nctg, nbp = int(which[1:]), 1, NBP
        path, span, window, boundary = wide(workdir, nfiles)
    p = F.plan(A_SIZES, nfiles)
    assert sum(A_SIZES) < 262144 and len(A_SIZES) >= 3000
    for e in ("search", "support"):
        assert p[e]["sliceLen"] == c["IGD_SETS_SLICE_MIN"] == 64 and p[e]["lds"] == (nfiles <= 8192)
        assert p[e]["chunks"] and all(ch["slices"] > ch["grid"] == c["IGD_SETS_GRID"] for ch in p[e]["chunks"])
        assert len(p[e]["chunks"]) == (2 if nfiles == 20000 else 1)
    (ichr, qs, qe), off = F.make_sets(np.random.default_rng(11), nctg, nbp, span, A_SIZES, window)
    check(path, ichr, qs, qe, off, boundary)


# ---- b ----------------------------------------------------------------------------------------------------------------------
_b_expect = {}


@pytest.mark.parametrize("big", [None, "2500"])
def test_b_slice_len_between_the_bounds(big, workdir, monkeypatch):
    """400 sets of 2 400-2 600 queries (10^6 in all) on 1 900 files, plus three small sets for the in-place anchor:
    64 < sliceLen < 4096, the last slice of a set shorter than the others, more slices than workgroups.  With
    IGD_SETS_BIG_MIN = 2500 about half of the sets take the batch pipeline in the same chunk as the others' slices."""
    c = F.consts()
    rs = np.random.default_rng(12)
    sizes = [int(n) for n in rs.integers(2400, 2601, 400)] + [0, 300, 1500]
    path, span, window, boundary = wide(workdir, 1900)
    p = F.plan(sizes, 1900, big_min=int(big) if big else None)
    for e in ("search", "support"):
        slen = p[e]["sliceLen"]
        assert c["IGD_SETS_SLICE_MIN"] < slen < c["IGD_SETS_SLICE_MAX"] and p[e]["lds"]
        (ch,) = p[e]["chunks"]
        assert ch["slices"] > ch["grid"] == c["IGD_SETS_GRID"]
        assert sum(1 for n in sizes[:400] if n % slen) >= 360           # a shorter last slice
    if big:
        monkeypatch.setenv("IGD_SETS_BIG_MIN", big)
        (ch,) = p["search"]["chunks"]
        assert ch["bigs"] >= 100 and ch["slices"] > ch["grid"] and p["search"]["sliceLen"] < p["support"]["sliceLen"]
    else:
        assert p["search"]["chunks"][0]["bigs"] == 0
    (ichr, qs, qe), off = F.make_sets(rs, 1, NBP, span, sizes, window)
    check(path, ichr, qs, qe, off, boundary, expect_cache=_b_expect)


# ---- c ----------------------------------------------------------------------------------------------------------------------
def test_c_cap_and_default_batch_seam(workdir):
    """140 sets of 120 001 queries (each below 2^17: the slice kernel), then small sets for the in-place anchor: sliceLen
    clamps to 4 096 -- the bound the 32-bit LDS counters of igd_sets_support are argued from -- and the default batch seam
    of 2^24 queries falls inside the last large set.  A sparse database of 9 files: under 2 records per query."""
    c = F.consts()
    sizes = [120001] * 140 + [0, 1, 64, 700, 1500]
    assert all(n < c["IGD_SETS_BIG_MIN_DEFAULT"] for n in sizes)
    p = F.plan(sizes, 9)
    for e in ("search", "support"):
        assert p[e]["sliceLen"] == c["IGD_SETS_SLICE_MAX"] == 4096 and p[e]["lds"]
        first, second = p[e]["chunks"]
        assert first["nq"] == c["IGD_HIP_MAX_BATCH_DEFAULT"] and first["slices"] > first["grid"] == c["IGD_SETS_GRID"]
        assert second["first"] == 139 and first["rows"] == 140          # the seam cuts the last large set
    path, span, window, boundary = wide(workdir, 9, span_tiles=96)
    (ichr, qs, qe), off = F.make_sets(np.random.default_rng(13), 1, NBP, span, sizes, window)
    orc = Oracle(path)
    try:
        _, total = orc.search(ichr[:120001], qs[:120001], qe[:120001], 0)
        assert 0 < total < 2 * 120001, "the database is not sparse: %d records under 120 001 queries" % total
    finally:
        orc.close()
    check(path, ichr, qs, qe, off, boundary)


# ---- d ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfiles", [1900, 2081, 8191, 8192, 8193])
def test_d_file_count_edges(nfiles, workdir):
    """The LDS forms at the benchmark's 1 900 files, at 2 081 (66 bitmap words: two steps of the per-query clear, and
    nfiles % 32 = 1), on both sides of and at IGD_SETS_LDS_FILES = IGD_SUPPORT_LDS_FILES = 8 192 -- where igd_sets_count
    asks for exactly 64 KiB of dynamic LDS: a clean launch is itself the assertion -- and the first wide form, 8 193."""
    c = F.consts()
    sizes = SIZES + [4097]
    p = F.plan(sizes, nfiles)
    assert c["IGD_SETS_LDS_FILES"] == c["IGD_SUPPORT_LDS_FILES"] == 8192
    assert p["search"]["lds"] == p["support"]["lds"] == (nfiles <= 8192) and p["nW"] == (nfiles + 31) // 32
    if nfiles == 2081:
        assert p["nW"] == 66 > c["IGD_WAVE"] and nfiles % 32 == 1
    if nfiles == 8192:
        assert nfiles * 8 == 64 << 10
    path, span, window, boundary = wide(workdir, nfiles)
    (ichr, qs, qe), off = F.make_sets(np.random.default_rng(14), 1, NBP, span, sizes, window)
    check(path, ichr, qs, qe, off, boundary)


# ---- e ----------------------------------------------------------------------------------------------------------------------
def test_e_row_cap_ends_a_chunk(workdir):
    """20 000 files, rowCap + 40 sets of 0-3 queries and a few of 300: the device rows of one chunk are full before its
    queries are.  The sets on either side of the border cover the window (non-zero rows), and a pre-filled matrix is added
    to across the border."""
    nfiles = 20000
    cap = F.plan([1], nfiles)["rowCap"]
    rs = np.random.default_rng(15)
    sizes = [int(n) for n in rs.integers(0, 4, cap + 40)]
    for k in (5, cap - 7, cap + 20):
        sizes[k] = 300
    sizes[cap - 1] = sizes[cap] = 3
    p = F.plan(sizes, nfiles)
    for e in ("search", "support"):
        assert [(ch["first"], ch["rows"]) for ch in p[e]["chunks"]] == [(0, cap), (cap, 40)] and not p[e]["lds"]
    path, span, window, boundary = wide(workdir, nfiles)
    (ichr, qs, qe), off = F.make_sets(rs, 1, NBP, span, sizes, window)
    a, b = int(off[cap - 1]), int(off[cap + 1])                         # the border sets: every query covers the window
    ichr[a:b], qs[a:b], qe[a:b] = F.scale_queries(rs, 1, NBP, span, b - a, window, share=1)
    check(path, ichr, qs, qe, off, boundary, prefill=True, must_hit=(cap - 1, cap))


# ---- f ----------------------------------------------------------------------------------------------------------------------
def test_f_cut_grid_of_the_wide_support_form(workdir):
    """300 000 files: the bitmap stripes of a full grid would pass IGD_SUPPORT_BITS_BYTES, so igd_hip_support_sets launches
    fewer workgroups than IGD_SETS_GRID, each with more than one slice; a miscounted stripe would be a write outside the
    stripes.  The first and the last file (bit 0 of the first word, bit 31 of the last) have support."""
    c = F.consts()
    sizes, (ichr, qs, qe), off = F.f_sets()
    p = F.plan(sizes, F.F_FILES)
    (ch,) = p["support"]["chunks"]
    assert p["support"]["maxGrid"] < c["IGD_SETS_GRID"] < ch["slices"] and ch["grid"] == p["support"]["maxGrid"]
    assert p["support"]["maxGrid"] * 4 * p["nW"] * 4 <= c["IGD_SUPPORT_BITS_BYTES"] and not p["support"]["lds"]
    assert (F.F_FILES - 1) % 32 == 31
    path = F.f_db(workdir)
    check(path, ichr, qs, qe, off, boundary=(0, F.F_FILES - 1))
