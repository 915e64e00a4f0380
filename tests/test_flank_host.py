"""Flanking records per dataset and the relative-distance histogram without a GPU: igdc_flank_host and igdc_flank_reldist_host
(igd_hostpath.c) through igd_amd.flanks_host / flank_reldist_host and through ctypes.

The expected values never come from the code under test: tests/flank_ref.py restates the definition as a numpy broadcast over the
interval lists this test wrote itself, and the placed cases are written out by hand.  Every integer must be equal.  The
identities are held against igdc_nearest_signed_host."""
import os
import random
import shutil

import numpy as np
import pytest

import igd_amd
from flank_ref import EDGES, MAX_BINS, MIDPOINTS, bins, flanked, ref_flanks, ref_hist
from helpers import short_tmpdir
from nearest_ref import MAX_WINDOW, NOV, TOP, ListDb, clustered_lists, mixed_regions, windows
from nearest_signed_ref import NO_RECORD
from test_nearest_host import set_offsets, tiled
from test_nearest_signed_host import SignedHost, top_db, top_regions
from test_support_host import NUMPY_DBS

GARBAGE = 0x5a5a5a5a
MEASURES = (EDGES, MIDPOINTS)


@pytest.fixture
def tmp():
    d = short_tmpdir("ifl")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", str(t))
    os.environ.pop("IGD_HOST_THREADS", None)


class FlankHost(SignedHost):
    """igdc_flank_host / igdc_flank_reldist_host through ctypes; every output is handed over full of garbage"""

    def flanks(self, ichr, qs, qe, window, measure, v=NOV, want_min=True):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        up, down = (np.full((len(qs), self.nfiles), GARBAGE, np.int32) for _ in range(2))
        upmin, downmin = (np.full(len(qs), GARBAGE, np.int32) for _ in range(2))
        rc = self.L.igdc_flank_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), window, measure, v,
                                    up.ctypes.data if up.size else None, down.ctypes.data if down.size else None,
                                    upmin.ctypes.data if want_min else None, downmin.ctypes.data if want_min else None)
        return rc, up, down, upmin, downmin

    def reldist(self, ichr, qs, qe, off, window, measure, nbins, v=NOV):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        off = np.ascontiguousarray(off, dtype=np.int64)
        h = np.full((len(off) - 1, min(max(nbins, 1), 64), self.nfiles + 1), -77, np.int64)
        rc = self.L.igdc_flank_reldist_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, off.ctypes.data,
                                            len(off) - 1, window, measure, v, nbins, h.ctypes.data)
        return rc, h


def flank_identities(up, down, sdist):
    """the edges measure against nearest_signed"""
    pos, neg, none = sdist > 0, (sdist < 0) & (sdist != NO_RECORD), sdist == NO_RECORD
    s = sdist.astype(np.int64)
    assert np.array_equal(down[pos], s[pos]) and ((up[pos] == -1) | (up[pos] > s[pos])).all()
    assert np.array_equal(up[neg], -s[neg]) and ((down[neg] == -1) | (down[neg] >= up[neg])).all()
    assert (up[none] == -1).all() and (down[none] == -1).all()


# ---- the placed cases of the issue ------------------------------------------------------------------------------------------
def placed_flank_db(d, nbp=1 << 14, name="fplaced"):
    files = [
        [("chrA", 900, 1000, 900), ("chrA", 2000, 2500, 900)],              # f0: book-ended on both sides of [1000, 2000)
        [("chrA", 10050, 10300, 900)],                                      # f1: overlaps [10000, 10100), its midpoint lies above
        [("chrA", 20040, 20060, 900)],                                      # f2: the midpoint of [20000, 20100)
        [("chrA", 30100, 31100, 900)],                                      # f3: d = 91 but D = 595 from [30000, 30010)
        [("chrA", 49900, 49990, 100), ("chrA", 49000, 49100, 800), ("chrA", 50400, 50500, 800)],   # f4: -v removes the nearer one
        [("chrA", 59990, 60000, 900), ("chrA", 60102, 60110, 900)],         # f5: up 1, down 3 around [60000, 60100)
    ]
    return ListDb(d, name, files, nbp, 1)


def placed_flank_regions():
    a = np.array([(0, 1000, 2000), (0, 10000, 10100), (0, 20000, 20100), (0, 30000, 30010), (0, 50000, 50100), (0, 60000, 60100),
                  (0, 50100, 50000), (0, 49950, 49950), (-1, 100, 200), (1, 100, 200)], np.int64)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32)


def wide_db(d, nbp=1 << 14, name="fwide"):
    """one file on one contig: records [0, 1) and [2^31 - 2, 2^31 - 1): 2^30 on either side of the inverted region
    (2^30, 2^30 - 1), up + down = 2^31"""
    return ListDb(d, name, [[("chrE", 0, 1, 900), ("chrE", TOP - 1, TOP, 900)]], nbp, 1)


def test_the_reference_restates_the_bins():
    assert bins([1, 1, 2 ** 30, 0, 3, 49], [1, 3, 2 ** 30, 7, 1, 51], 2).tolist() == [1, 1, 1, 0, 1, 1]
    assert bins([1, 1, 49, 1], [1, 3, 51, 99], 50).tolist() == [49, 25, 49, 1]
    assert flanked([-1, 0, 0, 5, 2 ** 30], [3, 0, 1, -1, 2 ** 30]).tolist() == [False, False, True, False, True]


def test_placed_cases(tmp, host_threads):
    nbp = 1 << 14
    db = placed_flank_db(tmp, nbp)
    ichr, qs, qe = placed_flank_regions()
    H = FlankHost(db.path)
    try:
        host_threads(1)
        for W in windows(nbp) + [500, 1000]:
            for v in (None, 500):
                for ms in MEASURES:
                    want = ref_flanks(db, ichr, qs, qe, W, ms, v)
                    got = H.flanks(ichr, qs, qe, W, ms, NOV if v is None else v)
                    assert got[0] == 0 and all(np.array_equal(g, w) for g, w in zip(got[1:], want)), (W, v, ms)
        _, eu, ed, eum, edm = H.flanks(ichr, qs, qe, 1000, EDGES)
        _, mu, md, mum, mdm = H.flanks(ichr, qs, qe, 1000, MIDPOINTS)
        assert eu[0, 0] == 1 and ed[0, 0] == 1                             # book-ended on each side
        assert mu[0, 0] == 550 and md[0, 0] == 750                         # 1500 against 950 and 2250
        assert eu[1, 1] == -1 and ed[1, 1] == -1 and mu[1, 1] == -1 and md[1, 1] == 125    # overlapping: neither side / downstream
        assert eu[2, 2] == -1 and ed[2, 2] == -1 and mu[2, 2] == -1 and md[2, 2] == 0      # equal midpoints are "right"
        assert ed[3, 3] == 91 and md[3, 3] == 595
        _, _, ed5, _, _ = H.flanks(ichr, qs, qe, 500, EDGES)
        _, _, md5, _, _ = H.flanks(ichr, qs, qe, 500, MIDPOINTS)
        assert ed5[3, 3] == 91 and md5[3, 3] == -1                         # d <= W but |D| > W: does not take part
        assert eu[4, 4] == 11 and ed[4, 4] == 301
        _, vu, vd, vum, _ = H.flanks(ichr, qs, qe, 1000, EDGES, 500)
        assert vu[4, 4] == 901 and vd[4, 4] == 301 and vum[4] == 901       # -v 500 removes the nearer upstream record
        assert eu[5, 5] == 1 and ed[5, 5] == 3
        assert eum[0] == 1 and edm[0] == 1 and mum[1] == -1 and mdm[1] == 125
        assert (eu[8:] == -1).all() and (ed[8:] == -1).all() and (eum[8:] == -1).all() and (mdm[8:] == -1).all()     # unknown contigs
        assert eu[6, 4] == 111 and ed[6, 4] == 401 and eu[7, 4] == 851 and ed[7, 4] == 451 and mu[7, 4] == 5 and md[7, 4] == 500      # inverted, zero length: the formula, literally
        # bins by hand: min == max is ratio 0.5, the last bin; 1 / (1 + 3) is exactly the edge 0.25
        off = np.array([0, len(qs)], np.int64)
        for B, b0, b5 in ((1, 0, 0), (2, 1, 1), (50, 49, 25), (64, 63, 32)):
            rc, h = H.reldist(ichr, qs, qe, off, 1000, EDGES, B)
            assert rc == 0 and np.array_equal(h, ref_hist(eu, ed, eum, edm, off, B)), B
            assert h[0, b0, 0] == 1 and h[0, :, 0].sum() == 1 and h[0, b5, 5] == 1 and h[0, :, 5].sum() == 1, B
            assert np.array_equal(h.sum(axis=1)[0], flanked(np.c_[eu, eum], np.c_[ed, edm]).sum(axis=0))
    finally:
        H.close()


def test_a_distance_of_2_to_the_30_and_a_sum_of_2_to_the_31(tmp, host_threads):
    nbp = 1 << 14
    host_threads(1)
    H = FlankHost(top_db(tmp, nbp).path)
    try:
        ichr, qs, qe = top_regions()
        _, up, down, _, _ = H.flanks(ichr, qs, qe, MAX_WINDOW, EDGES)
        assert down[0, 0] == 2 ** 30 and up[1, 1] == 2 ** 30
        _, up, down, _, _ = H.flanks(ichr, qs, qe, MAX_WINDOW - 1, EDGES)
        assert down[0, 0] == -1 and up[1, 1] == -1
    finally:
        H.close()
    wdb = wide_db(tmp, nbp)
    H = FlankHost(wdb.path)
    try:
        ichr, qs, qe = np.array([0], np.int32), np.array([2 ** 30], np.int32), np.array([2 ** 30 - 1], np.int32)
        rc, up, down, upmin, downmin = H.flanks(ichr, qs, qe, MAX_WINDOW, EDGES)
        assert rc == 0 and up[0, 0] == 2 ** 30 and down[0, 0] == 2 ** 30 and upmin[0] == 2 ** 30 and downmin[0] == 2 ** 30
        assert all(np.array_equal(g, w) for g, w in zip((up, down, upmin, downmin), ref_flanks(wdb, ichr, qs, qe, MAX_WINDOW, EDGES)))
        for B in (1, 2, 50, 64):
            rc, h = H.reldist(ichr, qs, qe, [0, 1], MAX_WINDOW, EDGES, B)
            assert rc == 0 and h[0, B - 1].tolist() == [1, 1] and h.sum() == 2, B
        rc, mu, md, _, _ = H.flanks(ichr, qs, qe, MAX_WINDOW, MIDPOINTS)
        assert rc == 0 and mu[0, 0] == 2 ** 30 - 1 and md[0, 0] == 2 ** 30 - 1
    finally:
        H.close()


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_route_equals_the_definition_on_the_four_database_shapes(case, tmp, host_threads):
    rng = random.Random(11100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    db = ListDb(tmp, "c%d" % case, files, nbp, gtype)
    ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 600)
    off = set_offsets(rng, len(qs))
    H = FlankHost(db.path)
    try:
        seen = 0
        for W in windows(nbp):
            for v in (None, 500):
                nv = NOV if v is None else v
                host_threads(1)
                for ms in MEASURES:
                    want = ref_flanks(db, ichr, qs, qe, W, ms, v)
                    got = H.flanks(ichr, qs, qe, W, ms, nv)
                    assert got[0] == 0 and all(np.array_equal(g, w) for g, w in zip(got[1:], want)), (W, v, ms)
                    if ms == EDGES:
                        rc, sdist, _ = H.signed(ichr, qs, qe, W, nv)
                        assert rc == 0
                        flank_identities(want[0], want[1], sdist)
                    for B in (1, 2, 50, 64):
                        rc, h = H.reldist(ichr, qs, qe, off, W, ms, B, nv)
                        assert rc == 0 and np.array_equal(h, ref_hist(*want, off, B)), (W, v, ms, B)
                    seen += int(flanked(want[0], want[1]).sum())
        assert seen > 1000, "fixture is vacuous: hardly a flanked pair"
        # thread counts 1, 2 and 7 agree (on enough regions for seven threads to start)
        W = 3 * nbp + 5
        for ms in MEASURES:
            want = ref_flanks(db, ichr, qs, qe, W, ms, 500)
            tc, ts, te, tu = tiled(ichr, qs, qe, want[0])
            reps = len(ts) // len(qs)
            td, tum, tdm = np.tile(want[1], (reps, 1)), np.tile(want[2], reps), np.tile(want[3], reps)
            toff = np.array([0, 1, 2049, len(ts)], np.int64)
            hwant = ref_hist(tu, td, tum, tdm, toff, 50)
            for threads in (1, 2, 7):
                host_threads(threads)
                got = H.flanks(tc, ts, te, W, ms, 500)
                assert got[0] == 0 and all(np.array_equal(g, w) for g, w in zip(got[1:], (tu, td, tum, tdm))), (ms, threads)
                rc, h = H.reldist(tc, ts, te, toff, W, ms, 50, 500)
                assert rc == 0 and np.array_equal(h, hwant), (ms, threads)
    finally:
        H.close()


def test_outputs_are_defined_and_bad_arguments_write_nothing(tmp):
    rng = random.Random(11300)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 3, 1, 6)
    db = ListDb(tmp, "a", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 40)
    H = FlankHost(db.path)
    try:
        rc, up, down, upmin, downmin = H.flanks(ichr, qs, qe, nbp, MIDPOINTS, want_min=False)
        want = ref_flanks(db, ichr, qs, qe, nbp, MIDPOINTS)
        assert rc == 0 and np.array_equal(up, want[0]) and np.array_equal(down, want[1]) and (upmin == GARBAGE).all() and (downmin == GARBAGE).all()
        rc, up, _, _, _ = H.flanks(ichr[:0], qs[:0], qe[:0], nbp, EDGES)
        assert rc == 0 and up.shape == (0, 3)
        for W, ms, B in ((-1, EDGES, 50), (MAX_WINDOW + 1, MIDPOINTS, 50), (-2 ** 31, EDGES, 50), (100, 2, 50), (100, -1, 50),
                         (100, EDGES, 0), (100, EDGES, 65), (100, MIDPOINTS, -3)):
            if B == 50:
                got = H.flanks(ichr, qs, qe, W, ms)
                assert got[0] == -1 and all((g == GARBAGE).all() for g in got[1:]), (W, ms)
            rc, h = H.reldist(ichr, qs, qe, [0, 40], W, ms, B)
            assert rc == -1 and (h == -77).all(), (W, ms, B)
        for off in ([1, 40], [0, 30, 20, 40]):
            rc, h = H.reldist(ichr, qs, qe, off, nbp, EDGES, 50)
            assert rc == -1 and (h == -77).all(), off
        rc, h = H.reldist(ichr, qs, qe, [0, 40], nbp, EDGES, MAX_BINS)
        assert rc == 0 and h.shape == (1, 64, 4) and h.sum() > 0
        # only empty sets: every word is written, all zero; no set at all: nothing to write
        rc, h = H.reldist(ichr[:0], qs[:0], qe[:0], [0, 0, 0], nbp, MIDPOINTS, 5)
        assert rc == 0 and h.shape == (2, 5, 4) and not h.any()
        rc, h = H.reldist(ichr[:0], qs[:0], qe[:0], [0], nbp, MIDPOINTS, 5)
        assert rc == 0 and h.shape == (0, 5, 4)
        rc, h = H.reldist(ichr, qs, qe, [0, 0, 40, 40], nbp, MIDPOINTS, 5)
        assert rc == 0 and not h[0].any() and not h[2].any() and h[1].any()
    finally:
        H.close()


def test_python_entry_points(tmp):
    rng = random.Random(11400)
    nbp = 1 << 11
    files, span = clustered_lists(rng, nbp, 4, 2, 12)
    db = ListDb(tmp, "p", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 2, nbp, span, 200)
    off = np.array([0, 0, 150, 200], np.int64)
    assert (igd_amd.FLANK_EDGES, igd_amd.FLANK_MIDPOINTS, igd_amd.FLANK_MAX_BINS) == (EDGES, MIDPOINTS, MAX_BINS)
    for name, ms in (("edges", EDGES), ("midpoints", MIDPOINTS)):
        want = ref_flanks(db, ichr, qs, qe, 700, ms, 500)
        got = igd_amd.flanks_host(db.path, ichr, qs, qe, 700, measure=name, value_filter=500)
        assert all(g.dtype == np.int32 and np.array_equal(g, w) for g, w in zip(got, want))
        fr = igd_amd.flank_reldist_host(db.path, ichr, qs, qe, off, 700, 50, measure=ms, value_filter=500)
        assert isinstance(fr, igd_amd.FlankReldist) and (fr.nbins, fr.window, fr.measure) == (50, 700, ms)
        assert fr.hist.dtype == np.int64 and np.array_equal(fr.hist, ref_hist(*want, off, 50)) and fr.hist.any()
        n, frac = igd_amd.reldist_summary(fr)
        assert np.array_equal(n, fr.hist.sum(axis=1)) and frac.shape == fr.hist.shape
        assert np.isnan(frac[0]).all() and np.isnan(frac[1][:, n[1] == 0]).all()
        assert np.allclose(frac[1][:, n[1] > 0].sum(axis=0), 1.0) and np.array_equal(frac[1][:, n[1] > 0] * n[1][n[1] > 0], fr.hist[1][:, n[1] > 0])
    assert np.array_equal(igd_amd.flank_reldist_host(db.path, ichr, qs, qe, off, 700).hist,
                          igd_amd.flank_reldist_host(db.path, ichr, qs, qe, off, 700, 50, "midpoints").hist)
    err = igd_amd.database.IgdError
    for bad in (0, 65, -1, 2.0, "50", True):
        with pytest.raises(err):
            igd_amd.flank_reldist_host(db.path, ichr, qs, qe, off, 700, bad)
    for bad in ("edge", 2, None, True):
        with pytest.raises(err):
            igd_amd.flanks_host(db.path, ichr, qs, qe, 700, measure=bad)
    with pytest.raises(err):
        igd_amd.flanks_host(db.path, ichr, qs, qe, MAX_WINDOW + 1)
    with pytest.raises(err):
        igd_amd.flank_reldist_host(db.path, ichr, qs, qe, [0, 5], 700)
