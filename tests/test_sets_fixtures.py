"""No GPU: the fixtures of tests/test_gpu_sets_scale.py are sound (tests/sets_fixtures.py).

igdc_support_host -- the expectation of the scale tests at v > 0 -- is held against the oracle at file counts that are new for
it (2 081 and 8 193: its stamp array has nFiles entries), the non-vacuity conditions hold on such a database, and plan()
gives the hand-computed decomposition of known shapes, two of them the measured shapes of DESIGN section 4.4.  The numpy
writer, the oracle and igdc_support_host take the 300 000-file database of case f.

The same for tests/test_gpu_coverage_scale.py: igdc_coverage_host -- its expectation at v > 0 -- is held against both sources of
tests/test_coverage_host.py at 2 041 and 8 193 files (its front[] and last[] arrays have nFiles entries), CovWitness passes
there, plan()["coverage"] gives the hand-computed shapes, and the oracle and igdc_coverage_host take the fixture of more than
2^32 bp in one slice, whose hand values hold."""
import random
import shutil

import numpy as np
import pytest

import sets_fixtures as F
from helpers import Oracle, short_tmpdir
from test_coverage_host import HostCov, coverage_brute, coverage_from_enumeration, query_bp
from test_support_host import HostDb, cli_rule, oracle_support, oracle_support_enum


@pytest.fixture
def tmp():
    d = short_tmpdir("isf")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("nfiles", [2081, 8193])
def test_host_support_and_the_fixture_on_wide_databases(nfiles, tmp, monkeypatch):
    nbp = 1 << 14
    path, span, window, edge = F.wide_db(random.Random(nfiles), tmp, "w", nfiles, nbp, max(40, nfiles * 3 // 10))
    assert edge == F.boundary_files(nfiles) and {0, 31, 32, 63, 64, 2047, 2048, nfiles - 1} <= set(edge)
    sizes = [0, 1, 65, 700, 1500, 734]
    (ichr, qs, qe), off = F.make_sets(np.random.default_rng(nfiles), 1, nbp, span, sizes, window)
    assert off[-1] == 3000
    orc, H = Oracle(path), HostDb(path)
    try:
        assert H.nfiles == orc.nfiles == nfiles
        for v in (0, 500):
            rule, ev = cli_rule(orc.gtype, v)
            W = F.Witness(edge)
            rows = F.expected_rows(orc, H, ichr, qs, qe, off, v)
            for k, (hits, total, sup, nhit) in enumerate(rows):
                a, b = off[k], off[k + 1]
                want, wnhit, whits = oracle_support(orc, ichr[a:b], qs[a:b], qe[a:b], v)
                assert np.array_equal(sup, want) and nhit == wnhit and np.array_equal(hits, whits), (v, k)
                if v == 0:
                    e_sup, e_nhit = oracle_support_enum(orc, ichr[a:b], qs[a:b], qe[a:b])
                    assert np.array_equal(e_sup, want) and e_nhit == wnhit
                for threads in ("1", "3"):
                    monkeypatch.setenv("IGD_HOST_THREADS", threads)
                    got, gnhit = H.support(ichr[a:b], qs[a:b], qe[a:b], ev, rule)
                    assert np.array_equal(got, want) and gnhit == wnhit, (v, k, threads)
                W.add(b - a, hits, total, sup, nhit)
            W.check()
    finally:
        H.close()
        orc.close()


def test_consts_are_the_values_the_cases_were_sized_for():
    c = F.consts()
    assert (c["IGD_SETS_SLICES"], c["IGD_SETS_SLICE_MIN"], c["IGD_SETS_SLICE_MAX"], c["IGD_SETS_GRID"]) == (4096, 64, 4096, 2048)
    assert c["IGD_SETS_LDS_FILES"] == c["IGD_SUPPORT_LDS_FILES"] == 8192
    assert c["IGD_SETS_ROW_BYTES"] == c["IGD_SUPPORT_BITS_BYTES"] == 256 << 20
    assert c["IGD_SETS_BIG_MIN_DEFAULT"] == 1 << 17 and c["IGD_HIP_MAX_BATCH_DEFAULT"] == 1 << 24
    assert c["IGD_SETS_WG"] // c["IGD_WAVE"] == 4
    assert c["IGD_COVERAGE_LDS_FILES"] == 2040 and c["IGD_COVERAGE_FRONT_BYTES"] == 256 << 20 and c["IGD_MEMBER_LDS_FILES"] == 16384


def test_plan_gives_the_hand_computed_decomposition():
    # DESIGN 4.4, 1 000 sets of 1 000 queries at 1 900 files: ceil(10^6 / 4096) = 245, ceil(1000 / 245) = 5 slices per set
    p = F.plan([1000] * 1000, 1900)
    for e in ("search", "support"):
        assert p[e]["sliceLen"] == 245 and p[e]["lds"]
        assert p[e]["chunks"] == [dict(first=0, rows=1000, nq=1000000, slices=5000, bigs=0, grid=2048)]
    # DESIGN 4.4, 10 000 sets of 100: the same sliceLen, one slice per set
    p = F.plan([100] * 10000, 1900)
    for e in ("search", "support"):
        assert p[e]["sliceLen"] == 245
        assert p[e]["chunks"] == [dict(first=0, rows=10000, nq=1000000, slices=10000, bigs=0, grid=2048)]
    # the suite's small shapes: sliceLen at its lower bound, as many workgroups as slices (1 + 0 + ceil(400 / 64) + 1)
    p = F.plan([10, 0, 400, 3], 6)
    assert p["search"]["sliceLen"] == 64 and p["search"]["chunks"] == [dict(first=0, rows=4, nq=413, slices=9, bigs=0, grid=9)]
    assert p["support"]["chunks"] == p["search"]["chunks"]
    # a set on the batch pipeline: search slices the small one only (and sizes its slices by the small queries alone);
    # support slices every set: ceil(5010 / 4096) = 2 -> 64, ceil(5000 / 64) + 1 = 80
    p = F.plan([5000, 10], 9, big_min=64)
    assert p["search"]["chunks"] == [dict(first=0, rows=2, nq=5010, slices=1, bigs=1, grid=1)]
    assert p["support"]["sliceLen"] == 64 and p["support"]["chunks"] == [dict(first=0, rows=2, nq=5010, slices=80, bigs=0, grid=80)]
    # the row cap: 2^28 / (20 000 * 8) = 1 677 rows per chunk
    p = F.plan([1] * 1717, 20000)
    assert p["rowCap"] == 1677 and not p["search"]["lds"] and not p["support"]["lds"]
    assert [(c["first"], c["rows"]) for c in p["support"]["chunks"]] == [(0, 1677), (1677, 40)]
    assert p["support"]["maxGrid"] == 2048                 # 625 words x 4 waves x 4 bytes x 2 048 = 20 MB of stripes
    # the batch seam: 140 sets of 120 001; 2^24 = 139 * 120 001 + 97 077; ceil(120001 / 4096) = 30, ceil(97077 / 4096) = 24,
    # the rest of set 139 (22 924 queries) opens the second chunk with ceil(22924 / 4096) = 6 slices
    p = F.plan([120001] * 140, 9)
    for e in ("search", "support"):
        assert p[e]["sliceLen"] == 4096
        assert p[e]["chunks"] == [dict(first=0, rows=140, nq=1 << 24, slices=139 * 30 + 24, bigs=0, grid=2048),
                                  dict(first=139, rows=1, nq=22924, slices=6, bigs=0, grid=6)]
    # a lowered seam as in test_sets_straddle_engine_batches (a chunk that is full when a set begins still holds its empty row)
    p = F.plan([0, 1, 96, 97, 98], 9, max_batch=97)
    assert [(c["first"], c["rows"], c["nq"]) for c in p["support"]["chunks"]] == [(0, 4, 97), (3, 2, 97), (4, 1, 97), (4, 1, 1)]
    # the cut grid: 300 000 files are 9 375 words; 2^28 / (9 375 * 16) = 1 789.57
    p = F.plan([4096] * 40, 300000)
    assert p["nW"] == 9375 and p["support"]["maxGrid"] == 1789 and p["search"]["maxGrid"] == 2048
    assert p["rowCap"] == 111 and p["support"]["chunks"] == [dict(first=0, rows=40, nq=163840, slices=2560, bigs=0, grid=1789)]
    # 8 192 files are still the LDS forms, 8 193 are not
    assert F.plan([1], 8192)["search"]["lds"] and F.plan([1], 8192)["support"]["lds"]
    assert not F.plan([1], 8193)["search"]["lds"] and not F.plan([1], 8193)["support"]["lds"]


def test_writer_and_oracle_take_the_300000_file_database(tmp):
    """Case f's database and sets (sets_fixtures.f_db, f_sets) before any GPU sees them: the numpy writer writes 300 000 files,
    the oracle and igdc_support_host open them, and the expectation of a 4 096-query set and of the small set (anchored
    per query against the oracle) is non-vacuous: the first and the last file have support, below their pair counts."""
    path = F.f_db(tmp)
    sizes, (ichr, qs, qe), off = F.f_sets()
    assert sizes[0] == 4096 and 0 < sizes[-1] <= F.ANCHOR_MAX
    keep = np.r_[off[0]:off[1], off[-2]:off[-1]]                        # the first large set and the small one
    sub = np.array([0, sizes[0], sizes[0] + sizes[-1]], np.int64)
    assert len(keep) == sub[-1]
    orc, H = Oracle(path), HostDb(path)
    try:
        assert H.nfiles == orc.nfiles == F.F_FILES
        for v in (0, 500):
            W = F.Witness((0, F.F_FILES - 1))
            for k, (hits, total, sup, nhit) in enumerate(F.expected_rows(orc, H, ichr[keep], qs[keep], qe[keep], sub, v)):
                W.add(int(sub[k + 1] - sub[k]), hits, total, sup, nhit)
                assert 100 < np.count_nonzero(sup) < 1000, "the window should meet a few hundred files"
                assert 0 < sup[0] < hits[0] and 0 < sup[-1] < hits[-1]
            W.check()
    finally:
        H.close()
        orc.close()


# ---- covered base pairs -----------------------------------------------------------------------------------------------------
def test_plan_gives_the_hand_computed_decomposition_of_coverage():
    # DESIGN 4.6's measured shape, 1 000 sets of 1 000 queries at 1 900 files: as support, in the LDS form
    p = F.plan([1000] * 1000, 1900)["coverage"]
    assert p["sliceLen"] == 245 and p["lds"] and p["maxGrid"] == 2048
    assert p["chunks"] == [dict(first=0, rows=1000, nq=1000000, slices=5000, bigs=0, grid=2048)]
    # 2 040 files are the LDS form, 2 041 are not; the cut grid: 2^28 / (2 041 * 32) = 4 110 -> 2 048,
    # 2^28 / (20 000 * 32) = 419.4, 2^28 / (10^6 * 32) = 8.4
    assert F.plan([1], 2040)["coverage"]["lds"] and not F.plan([1], 2041)["coverage"]["lds"]
    assert F.plan([1], 2040)["coverage"]["maxGrid"] == F.plan([1], 2041)["coverage"]["maxGrid"] == 2048
    assert F.plan([1], 20000)["coverage"]["maxGrid"] == 419 and F.plan([1], 1000000)["coverage"]["maxGrid"] == 8
    # the row cap: 1 677 rows per chunk at 20 000 files
    p = F.plan([1] * 1717, 20000)
    assert [(c["first"], c["rows"]) for c in p["coverage"]["chunks"]] == [(0, 1677), (1677, 40)]
    # case a of test_gpu_coverage_scale: (1 + 1 + 1 + 2 + 2 + 3) * 300 = 3 000 slices of 117 900 queries, one chunk
    sizes = [0, 1, 63, 64, 65, 70, 130] * 300
    for nfiles in (9, 1900, 2040):
        p = F.plan(sizes, nfiles)["coverage"]
        assert p["sliceLen"] == 64 and p["lds"]
        assert p["chunks"] == [dict(first=0, rows=2100, nq=117900, slices=3000, bigs=0, grid=2048)]
    # case w: 90 repeats are 900 slices against the 419 workgroups of 20 000 files
    p = F.plan([0, 1, 63, 64, 65, 70, 130] * 90, 20000)["coverage"]
    assert p["sliceLen"] == 64 and not p["lds"]
    assert p["chunks"] == [dict(first=0, rows=630, nq=35370, slices=900, bigs=0, grid=419)]


@pytest.mark.parametrize("nfiles", [2041, 8193])
def test_host_coverage_and_the_fixture_on_wide_databases(nfiles, tmp, monkeypatch):
    nbp = 1 << 14
    path, span, window, edge = F.wide_db(random.Random(nfiles), tmp, "w", nfiles, nbp, max(40, nfiles * 3 // 10))
    sizes = [0, 1, 65, 700, 1500, 734]
    (ichr, qs, qe), off = F.make_sets(np.random.default_rng(nfiles), 1, nbp, span, sizes, window)
    orc, H = Oracle(path), HostCov(path)
    try:
        assert H.nfiles == orc.nfiles == nfiles
        for v in (0, 500):
            rule, ev = cli_rule(orc.gtype, v)
            W, tally = F.CovWitness(edge), {}
            for k, (cov, covered, pairs) in enumerate(F.expected_cov_rows(path, orc, H, ichr, qs, qe, off, v, tally=tally)):
                a, b = off[k], off[k + 1]
                c, s, e = ichr[a:b], qs[a:b], qe[a:b]
                # the two sources of test_coverage_host, each where it applies: the enumeration at v = 0 (rule NEST), the
                # brute force at v > 0 (rule FLAT) -- here for every set, not only the ones expected_cov_rows anchors
                want =coverage_brute(path, orc, c, s, e, v) if v else coverage_from_enumeration(orc, c, s, e)
                assert np.array_equal(cov, want[0]) and covered == want[1] and np.array_equal(pairs, want[2]), (v, k)
                for threads in ("1", "3"):
                    monkeypatch.setenv("IGD_HOST_THREADS", threads)
                    got, gcovered = H.coverage(c, s, e, ev, rule)
                    assert np.array_equal(got, want[0]) and gcovered == want[1], (v, k, threads)
                W.add(cov, covered, pairs, query_bp(s, e))
            W.check(tally if v else None)
            if v:
                assert tally == dict(nonempty=5, anchored=5)
    finally:
        H.close()
        orc.close()


def test_oracle_and_host_take_more_than_2_32_bp_in_one_slice(tmp):
    path = F.bigbp_db(tmp)
    (ichr, qs, qe), off = F.bigbp_sets()
    p = F.plan(np.diff(off), 3)["coverage"]
    assert p["sliceLen"] == 64 and p["lds"] and p["chunks"][0]["slices"] == 3       # set 0 is one slice: one LDS counter
    orc, H = Oracle(path), HostCov(path)
    try:
        assert orc.nfiles == 3 and orc.gtype == 1
        for v in (0, 500):
            tally = {}
            rows = list(F.expected_cov_rows(path, orc, H, ichr, qs, qe, off, v, tally=tally))
            assert not v or tally == dict(nonempty=3, anchored=3)
            assert rows[0][0].tolist() == [F.BIGBP_HAND, 64 * 500, 0] and rows[0][1] == F.BIGBP_HAND > 1 << 32
            assert rows[1][0].tolist() == [68999000, 500, 0] and rows[1][1] == 68999000
            assert rows[2][0].tolist() == [6400, 0, 0] and rows[2][1] == 6400
            rule, ev = cli_rule(orc.gtype, v)
            for k, (cov, covered, pairs) in enumerate(rows):
                got, gcovered = H.coverage(ichr[off[k]:off[k + 1]], qs[off[k]:off[k + 1]], qe[off[k]:off[k + 1]], ev, rule)
                assert np.array_equal(got, cov) and gcovered == covered and np.array_equal(pairs, cov), (v, k)
            got, gcovered = H.coverage(ichr, qs, qe, ev, rule)
            assert got.tolist() == [65 * 68999000 + 6400, 65 * 500, 0] and gcovered == 65 * 68999000 + 6400
    finally:
        H.close()
        orc.close()
