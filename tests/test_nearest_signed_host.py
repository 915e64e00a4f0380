"""Signed nearest distances and their histogram without a GPU: igdc_nearest_signed_host and igdc_nearest_hist_host
(igd_hostpath.c) through igd_amd.nearest_signed_host / nearest_hist_host and through ctypes.

The expected values never come from the code under test: tests/nearest_signed_ref.py restates the definition as a numpy
broadcast over the interval lists this test wrote itself, and the placed cases are written out by hand.  Every integer must be
equal.  The identities are held against igdc_nearest_host / igdc_nearest_sets_host."""
import os
import random
import shutil

import numpy as np
import pytest

import igd_amd
from helpers import short_tmpdir
from nearest_ref import MAX_WINDOW, NOV, TOP, ListDb, clustered_lists, mixed_regions, placed_db, placed_regions, windows
from nearest_signed_ref import MAX_EDGES, NO_RECORD, decode, edge_lists, pair_key, ref_hist, ref_signed_rows
from test_nearest_host import NearestHost, set_offsets, tiled
from test_support_host import NUMPY_DBS

GARBAGE = 0x5a5a5a5a


@pytest.fixture
def tmp():
    d = short_tmpdir("ins")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", str(t))
    os.environ.pop("IGD_HOST_THREADS", None)


def top_db(d, nbp, name="top"):
    """two files on one contig: f0 a record at the top of int32, f1 one that ends at 1000"""
    return ListDb(d, name, [[("chrE", TOP - 100, TOP, 900)], [("chrE", 900, 1000, 900)]], nbp, 1)


def top_regions():
    """region 0 ends 2^30 - 1 below f0's record at the top: d = 2^30, downstream; region 1 starts 2^30 - 1 above the end of f1's
    record: d = 2^30, upstream (each is nearer to the other file's record)"""
    qe0, qs1 = TOP - 100 + 1 - 2 ** 30, 1000 - 1 + 2 ** 30
    return np.array([0, 0], np.int32), np.array([qe0 - 50, qs1], np.int32), np.array([qe0, qs1 + 50], np.int32)


class SignedHost(NearestHost):
    """igdc_nearest_signed_host / igdc_nearest_hist_host through ctypes; every output is handed over full of garbage"""

    def signed(self, ichr, qs, qe, window, v=NOV, want_min=True):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        sdist = np.full((len(qs), self.nfiles), GARBAGE, np.int32)
        sdmin = np.full(len(qs), GARBAGE, np.int32)
        rc = self.L.igdc_nearest_signed_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), window, v,
                                             sdist.ctypes.data if sdist.size else None, sdmin.ctypes.data if want_min else None)
        return rc, sdist, sdmin

    def hist(self, ichr, qs, qe, off, window, edges, v=NOV, ne=None):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        off = np.ascontiguousarray(off, dtype=np.int64)
        edges = np.ascontiguousarray(edges, dtype=np.int32)
        ne = len(edges) if ne is None else ne
        h = np.full((len(off) - 1, max(ne, 0) + 1, self.nfiles + 1), -77, np.int64)
        rc = self.L.igdc_nearest_hist_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, off.ctypes.data,
                                           len(off) - 1, window, v, edges.ctypes.data if edges.size else None, ne, h.ctypes.data)
        return rc, h


def identities(sdist, sdmin, dist, dmin):
    for s, d in ((sdist, dist), (sdmin, dmin)):
        assert np.array_equal(s == NO_RECORD, d == -1)
        assert np.array_equal(np.abs(s.astype(np.int64))[d >= 0], d[d >= 0])


def test_the_reference_restates_the_key():
    """the key by hand: overlap 0; book-ended downstream 2 * 1 + 1, upstream 2 * 1; the largest key 2^31 + 1"""
    k = pair_key([1000, 2500, 2100, TOP - 100 - 2 ** 30], [2000, 2600, 2200, TOP - 100 + 1 - 2 ** 30], [2000, TOP - 100], [2500, TOP])
    assert k[0, 0] == 3 and k[1, 0] == 2 and k[2, 0] == 0 and k[3, 1] == 2 ** 31 + 1
    assert decode([0, 2, 3, 2 ** 31 + 1, 2 ** 31, 1 << 40]).tolist() == [0, -1, 1, 2 ** 30, -2 ** 30, NO_RECORD]


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_route_equals_the_definition_on_the_four_database_shapes(case, tmp, host_threads):
    rng = random.Random(8100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    db = ListDb(tmp, "c%d" % case, files, nbp, gtype)
    ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 600)
    off = set_offsets(rng, len(qs))
    H = SignedHost(db.path)
    try:
        up = down = False
        for W in windows(nbp):
            for v in (None, 500):
                nv = NOV if v is None else v
                want, wmin = ref_signed_rows(db, ichr, qs, qe, W, v)
                host_threads(1)
                rc, sdist, sdmin = H.signed(ichr, qs, qe, W, nv)
                assert rc == 0 and np.array_equal(sdist, want) and np.array_equal(sdmin, wmin), (W, v)
                rc, dist, dmin = H.nearest(ichr, qs, qe, W, nv)
                assert rc == 0
                identities(sdist, sdmin, dist, dmin)
                rc, (nw, no, _) = H.nearest_sets(ichr, qs, qe, off, W, nv)
                assert rc == 0
                for edges in edge_lists(W):
                    rc, h = H.hist(ichr, qs, qe, off, W, edges, nv)
                    assert rc == 0 and np.array_equal(h, ref_hist(want, wmin, off, edges)), (W, v, edges)
                    assert np.array_equal(h.sum(axis=1), nw)
                    if edges == (0, 1):
                        assert np.array_equal(h[:, 1], no)
                up |= bool(((want < 0) & (want != NO_RECORD)).any())
                down |= bool((want > 0).any())
        assert up and down, "fixture is vacuous: no upstream or no downstream record"
        # thread counts 1, 2 and 7 agree (on enough regions for seven threads to start)
        W = 3 * nbp + 5
        want, wmin = ref_signed_rows(db, ichr, qs, qe, W, 500)
        tc, ts, te, td = tiled(ichr, qs, qe, want)
        tmin = np.tile(wmin, len(ts) // len(qs))
        toff = np.array([0, 1, 2049, len(ts)], np.int64)
        hwant = ref_hist(td, tmin, toff, (-W, 0, 1, W + 1))
        for threads in (1, 2, 7):
            host_threads(threads)
            rc, sdist, sdmin = H.signed(tc, ts, te, W, 500)
            assert rc == 0 and np.array_equal(sdist, td) and np.array_equal(sdmin, tmin), threads
            rc, h = H.hist(tc, ts, te, toff, W, (-W, 0, 1, W + 1), 500)
            assert rc == 0 and np.array_equal(h, hwant), threads
    finally:
        H.close()


def test_placed_cases(tmp, host_threads):
    nbp = 1 << 14
    db = placed_db(tmp, nbp)
    (ichr, qs, qe), notes = placed_regions(nbp)
    H = SignedHost(db.path)
    try:
        host_threads(1)
        for W in windows(nbp) + [2 * nbp, 500]:
            for v in (None, 500):
                want, wmin = ref_signed_rows(db, ichr, qs, qe, W, v)
                rc, sdist, sdmin = H.signed(ichr, qs, qe, W, NOV if v is None else v)
                bad = np.flatnonzero((sdist != want).any(axis=1) | (sdmin != wmin))
                assert rc == 0 and len(bad) == 0, (W, v, [(notes[i], sdist[i].tolist(), want[i].tolist()) for i in bad])
                rc, dist, dmin = H.nearest(ichr, qs, qe, W, NOV if v is None else v)
                identities(sdist, sdmin, dist, dmin)
        # the expected values by hand (W = 500 serves the first four)
        rc, a, amin = H.signed(ichr, qs, qe, 500)
        rc2, b, _ = H.signed(ichr, qs, qe, 500, 500)
        assert rc == 0 and rc2 == 0
        assert a[0, 0] == 1                                               # [1000, 2000) against f0's [2000, 2500): downstream
        assert a[1, 0] == -1                                              # [2500, 2600): upstream
        assert a[4, 2] == -51                                             # f2's tie, d = 51 on both sides: upstream wins
        assert a[3, 1] == -11 and b[3, 1] == 301                          # f1: the filter flips the side
        assert amin[3] == -11 and amin[4] == -51
        for W in (1, 51, 301):
            rc, s, _ = H.signed(ichr, qs, qe, W)
            assert s[0, 0] == 1 and s[1, 0] == -1
            assert s[4, 2] == (-51 if W >= 51 else NO_RECORD)
            assert s[3, 1] == (-11 if W >= 11 else NO_RECORD)
            assert H.signed(ichr, qs, qe, W, 500)[1][3, 1] == (301 if W >= 301 else NO_RECORD)
        rc, big, bmin = H.signed(ichr, qs, qe, MAX_WINDOW)
        assert big[11, 4] == 0 and big[12, 4] == -1                       # inside the top record; zero length at 2^31 - 1: upstream
        assert (big[18:20] == NO_RECORD).all() and (bmin[18:20] == NO_RECORD).all()       # unknown contigs
        assert big[9, 3] == 3 * nbp - 40 + 5 + 1                          # a negative start: f3's first record is downstream
        assert a[16, 1] != NO_RECORD and a[17, 1] == 0                    # inverted and zero-length regions: the formula, literally
        # the histogram of the placed regions, edges at the ends of int32
        off = np.array([0, 5, 5, len(qs)], np.int64)
        for edges in edge_lists(MAX_WINDOW):
            rc, h = H.hist(ichr, qs, qe, off, MAX_WINDOW, edges)
            assert rc == 0 and np.array_equal(h, ref_hist(big, bmin, off, edges)), edges
        rc, h = H.hist(ichr, qs, qe, off, MAX_WINDOW, (-2 ** 31 + 1, 0, 2 ** 31 - 1))
        assert not h[:, 0].any() and not h[:, 3].any() and h[:, 1].any() and h[:, 2].any() and not h[1].any()
    finally:
        H.close()


def test_the_largest_key_survives(tmp, host_threads):
    """a region that ends 2^30 - 1 below a record at the top of int32: d = 2^30 downstream, key 2^31 + 1; and its mirror image,
    a record that ends 2^30 - 1 below a region: key 2^31"""
    nbp = 1 << 14
    db = top_db(tmp, nbp)
    ichr, qs, qe = top_regions()
    H = SignedHost(db.path)
    try:
        host_threads(1)
        rc, s, smin = H.signed(ichr, qs, qe, MAX_WINDOW)
        want, wmin = ref_signed_rows(db, ichr, qs, qe, MAX_WINDOW)
        assert rc == 0 and s[0, 0] == 2 ** 30 and s[1, 1] == -2 ** 30
        assert s[0, 1] == -(2 ** 30 - 1149) and s[1, 0] == 2 ** 30 - 1149          # qs - 1000 + 1; TOP - 100 - qe + 1
        assert np.array_equal(s, want) and np.array_equal(smin, wmin) and smin.tolist() == [-(2 ** 30 - 1149), 2 ** 30 - 1149]
        rc, s, smin = H.signed(ichr, qs, qe, MAX_WINDOW - 1)
        assert rc == 0 and s[0, 0] == NO_RECORD and s[1, 1] == NO_RECORD and s[0, 1] == want[0, 1] and s[1, 0] == want[1, 0]
        rc, h = H.hist(ichr, qs, qe, [0, 2], MAX_WINDOW, (-2 ** 30, 0, 2 ** 30))
        assert rc == 0 and h[0, :, 0].tolist() == [0, 0, 1, 1] and h[0, :, 1].tolist() == [0, 2, 0, 0] and h[0, :, 2].tolist() == [0, 1, 1, 0]
    finally:
        H.close()


def test_outputs_are_defined_and_bad_arguments_write_nothing(tmp):
    rng = random.Random(8300)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 3, 1, 6)
    db = ListDb(tmp, "a", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 40)
    H = SignedHost(db.path)
    try:
        rc, sdist, sdmin = H.signed(ichr, qs, qe, nbp, want_min=False)
        assert rc == 0 and np.array_equal(sdist, ref_signed_rows(db, ichr, qs, qe, nbp)[0]) and (sdmin == GARBAGE).all()
        rc, sdist, _ = H.signed(ichr[:0], qs[:0], qe[:0], nbp)
        assert rc == 0 and sdist.shape == (0, 3)
        for W in (-1, MAX_WINDOW + 1, -2 ** 31):
            rc, sdist, sdmin = H.signed(ichr, qs, qe, W)
            assert rc == -1 and (sdist == GARBAGE).all() and (sdmin == GARBAGE).all(), W
            rc, h = H.hist(ichr, qs, qe, [0, 40], W, (0, 1))
            assert rc == -1 and (h == -77).all(), W
        for off in ([1, 40], [0, 30, 20, 40]):
            rc, h = H.hist(ichr, qs, qe, off, nbp, (0, 1))
            assert rc == -1 and (h == -77).all(), off
        # edges: empty, not ascending, equal neighbours, more than 63
        for edges, ne in (((), 0), ((1, 0), 2), ((0, 0), 2), ((0, 5, 5), 3), (tuple(range(64)), 64), ((0,), -1)):
            rc, h = H.hist(ichr, qs, qe, [0, 40], nbp, edges, ne=ne)
            assert rc == -1 and (h == -77).all(), edges
        rc, h = H.hist(ichr, qs, qe, [0, 40], nbp, tuple(range(MAX_EDGES)))
        assert rc == 0 and h.shape == (1, 64, 4) and h.sum() > 0
        # only empty sets: every word is written, all zero; no set at all: nothing to write
        rc, h = H.hist(ichr[:0], qs[:0], qe[:0], [0, 0, 0], nbp, (0, 1))
        assert rc == 0 and h.shape == (2, 3, 4) and not h.any()
        rc, h = H.hist(ichr[:0], qs[:0], qe[:0], [0], nbp, (0, 1))
        assert rc == 0 and h.shape == (0, 3, 4)
    finally:
        H.close()


def test_python_entry_points(tmp):
    rng = random.Random(8400)
    nbp = 1 << 11
    files, span = clustered_lists(rng, nbp, 4, 2, 12)
    db = ListDb(tmp, "p", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 2, nbp, span, 200)
    off = np.array([0, 0, 150, 200], np.int64)
    assert igd_amd.NEAREST_NO_RECORD == NO_RECORD
    want, wmin = ref_signed_rows(db, ichr, qs, qe, 700, 500)
    sdist, sdmin = igd_amd.nearest_signed_host(db.path, ichr, qs, qe, 700, value_filter=500)
    assert sdist.dtype == np.int32 and np.array_equal(sdist, want) and np.array_equal(sdmin, wmin)
    identities(sdist, sdmin, *igd_amd.nearest_host(db.path, ichr, qs, qe, 700, value_filter=500))
    nh = igd_amd.nearest_hist_host(db.path, ichr, qs, qe, off, 700, [-700, 0, 1, 701], value_filter=500)
    assert isinstance(nh, igd_amd.NearestHist) and nh.window == 700 and nh.edges.tolist() == [-700, 0, 1, 701]
    assert nh.hist.dtype == np.int64 and np.array_equal(nh.hist, ref_hist(want, wmin, off, (-700, 0, 1, 701)))
    ns = igd_amd.nearest_sets_host(db.path, ichr, qs, qe, off, 700, value_filter=500)
    assert np.array_equal(nh.hist.sum(axis=1), ns.n_within) and np.array_equal(nh.hist[:, 2], ns.n_overlap)
    assert not nh.hist[:, 0].any() and not nh.hist[:, 4].any() and nh.hist[:, 1].any() and nh.hist[:, 3].any()
    err = igd_amd.database.IgdError
    for bad in ([], [1, 0], [0, 0], list(range(64)), [2 ** 31], [0.5], [[0, 1]]):
        with pytest.raises(err):
            igd_amd.nearest_hist_host(db.path, ichr, qs, qe, off, 700, bad)
    with pytest.raises(err):
        igd_amd.nearest_signed_host(db.path, ichr, qs, qe, MAX_WINDOW + 1)
    with pytest.raises(err):
        igd_amd.nearest_hist_host(db.path, ichr, qs, qe, off, -1, [0])
