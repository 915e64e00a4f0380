"""Nearest record per dataset within a window without a GPU: igdc_nearest_host, igdc_nearest_sets_host and
igdc_nearest_summary (igd_hostpath.c) through igd_amd.nearest_host / nearest_sets_host / nearest_summary and through ctypes.

The expected values never come from the code under test: tests/nearest_ref.py restates the definition as a numpy broadcast
over the interval lists this test wrote itself.  Every integer must be equal.  The identities with the support counts are
held against igdc_support_host (rule FLAT), product code of another walk that tests/test_support_host.py holds against the
oracle."""
import ctypes as C
import os
import random
import shutil

import numpy as np
import pytest

import igd_amd
from helpers import short_tmpdir
from nearest_ref import (MAX_WINDOW, NOV, ListDb, clustered_lists, mixed_regions, placed_db, placed_regions, ref_rows, ref_sets,
                         row_min, windows)
from test_support_host import FLAT, NUMPY_DBS, HostDb


@pytest.fixture
def tmp():
    d = short_tmpdir("inr")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", str(t))
    os.environ.pop("IGD_HOST_THREADS", None)


class NearestHost(HostDb):
    """igdc_nearest_host / igdc_nearest_sets_host through ctypes; every output is handed over full of garbage"""

    def nearest(self, ichr, qs, qe, window, v=NOV, want_dmin=True):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        dist = np.full((len(qs), self.nfiles), 0x5a5a5a5a, np.int32)
        dmin = np.full(len(qs), 0x5a5a5a5a, np.int32)
        rc = self.L.igdc_nearest_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), window, v,
                                      dist.ctypes.data if dist.size else None, dmin.ctypes.data if want_dmin else None)
        return rc, dist, dmin

    def nearest_sets(self, ichr, qs, qe, off, window, v=NOV):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        off = np.ascontiguousarray(off, dtype=np.int64)
        out = [np.full((len(off) - 1, self.nfiles + 1), -77, np.int64) for _ in range(3)]
        rc = self.L.igdc_nearest_sets_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, off.ctypes.data,
                                           len(off) - 1, window, v, *[a.ctypes.data for a in out])
        return rc, out


def tiled(ichr, qs, qe, dist, n=7 * 2048 + 5):
    """the regions repeated until seven host threads are worth starting (one per 2048 regions), and their rows"""
    reps = -(-n // len(qs))
    return np.tile(ichr, reps), np.tile(qs, reps), np.tile(qe, reps), np.tile(dist, (reps, 1))


def set_offsets(rng, nq):
    """sets of 0, 1, 5 and more regions that fill [0, nq)"""
    sizes = [0, 1, 5, 0, 300]
    while sum(sizes) < nq:
        sizes.append(min(rng.choice([0, 1, 5, 64, 700]), nq - sum(sizes)))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_route_equals_the_definition_on_the_four_database_shapes(case, tmp, host_threads):
    rng = random.Random(5100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    db = ListDb(tmp, "c%d" % case, files, nbp, gtype)
    ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 600)
    off = set_offsets(rng, len(qs))
    H = NearestHost(db.path)
    try:
        assert H.nfiles == nfiles
        seen_far = seen_none = False
        for W in windows(nbp):
            for v in (None, 500):
                want, wmin = ref_rows(db, ichr, qs, qe, W, v)
                host_threads(1)
                rc, dist, dmin = H.nearest(ichr, qs, qe, W, NOV if v is None else v)
                assert rc == 0 and np.array_equal(dist, want) and np.array_equal(dmin, wmin), (W, v)
                rc, sets = H.nearest_sets(ichr, qs, qe, off, W, NOV if v is None else v)
                assert rc == 0
                for got, ref in zip(sets, ref_sets(want, wmin, off)):
                    assert np.array_equal(got, ref), (W, v)
                seen_far |= bool((want > 0).any())
                seen_none |= bool(((want == -1).any(axis=1) & (want >= 0).any(axis=1)).any())
                if W == 0:
                    assert np.array_equal(sets[0], sets[1]) and not (want > 0).any()
        assert seen_far and seen_none, "fixture is vacuous: no positive distance, or no row that mixes -1 with distances"
        # the value filter changes something on gType 1 and nothing on gType 0
        a, b = ref_rows(db, ichr, qs, qe, nbp, None)[0], ref_rows(db, ichr, qs, qe, nbp, 500)[0]
        assert np.array_equal(a, b) == (gtype == 0)
        # thread counts 1, 2 and 7 agree (on enough regions for seven threads to start)
        W = 3 * nbp + 5
        want, _ = ref_rows(db, ichr, qs, qe, W, 500)
        tc, ts, te, td = tiled(ichr, qs, qe, want)
        for threads in (1, 2, 7):
            host_threads(threads)
            rc, dist, dmin = H.nearest(tc, ts, te, W, 500)
            assert rc == 0 and np.array_equal(dist, td) and np.array_equal(dmin, row_min(td)), threads
    finally:
        H.close()


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_n_overlap_is_the_support_under_rule_flat(case, tmp, host_threads):
    rng = random.Random(5200 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    db = ListDb(tmp, "s%d" % case, files, nbp, gtype)
    ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 500)
    # (rule FLAT counts nothing for a region that starts before 0 or past the last tile; the distance knows no such rule --
    # the identity is stated on the regions that start inside the contig's tiles)
    ntile = {c: max((e - 1) // nbp + 1 for recs in files for (cc, s, e, _) in recs if cc == "chr%d" % (c + 1)) for c in range(nctg)}
    ok = np.array([0 <= int(ichr[i]) < nctg and 0 <= int(qs[i]) < ntile[int(ichr[i])] * nbp for i in range(len(qs))])
    ichr, qs, qe = ichr[ok], qs[ok], qe[ok]
    off = np.array([0, 1, 6, 6, len(qs)], np.int64)
    H = NearestHost(db.path)
    try:
        for v in (NOV, 500):
            sup = np.zeros((4, nfiles + 1), np.int64)
            for k in range(4):
                a, b = int(off[k]), int(off[k + 1])
                s, nhit = H.support(ichr[a:b], qs[a:b], qe[a:b], v, FLAT)
                sup[k, :nfiles], sup[k, nfiles] = s, nhit
            assert sup.any()
            for W in (0, 1, nbp):
                rc, (nw, no, sd) = H.nearest_sets(ichr, qs, qe, off, W, v)
                assert rc == 0 and np.array_equal(no, sup), (v, W)
                assert (nw >= no).all() and (sd >= nw - no).all()
                if W == 0:
                    assert np.array_equal(nw, no) and not sd.any()
    finally:
        H.close()


def test_placed_cases(tmp, host_threads):
    nbp = 1 << 14
    db = placed_db(tmp, nbp)
    (ichr, qs, qe), notes = placed_regions(nbp)
    H = NearestHost(db.path)
    try:
        host_threads(1)
        for W in windows(nbp) + [2 * nbp, 500]:
            for v in (None, 500):
                want, wmin = ref_rows(db, ichr, qs, qe, W, v)
                rc, dist, dmin = H.nearest(ichr, qs, qe, W, NOV if v is None else v)
                bad = np.flatnonzero((dist != want).any(axis=1) | (dmin != wmin))
                assert rc == 0 and len(bad) == 0, (W, v, [(notes[i], dist[i].tolist(), want[i].tolist()) for i in bad])
        # what the placed cases are there for, read off the reference
        d1, _ = ref_rows(db, ichr, qs, qe, 1)
        assert d1[0, 0] == 1 and d1[1, 0] == 1                            # book-ended: 1 bp apart
        d0, _ = ref_rows(db, ichr, qs, qe, 0)
        assert d0[0, 0] == -1 and d0[1, 0] == -1                          # ... and not overlapping
        d2, _ = ref_rows(db, ichr, qs, qe, 2 * nbp)
        assert d2[2, 0] == nbp + 1                                        # the copy in an earlier tile
        assert ref_rows(db, ichr, qs, qe, nbp - 1)[0][2, 0] == -1
        a, b = ref_rows(db, ichr, qs, qe, 500)[0], ref_rows(db, ichr, qs, qe, 500, 500)[0]
        assert a[3, 1] == 11 and b[3, 1] == 301                           # -v picks the farther, passing record
        assert a[4, 2] == 51                                              # a tie: 70000 - 69950 + 1 = 70060 - 70010 + 1
        big, bmin = ref_rows(db, ichr, qs, qe, MAX_WINDOW)
        assert big[11, 4] == 0 and big[12, 4] == 1 and big[14, 4] == -1 and big[15, 4] > 0
        assert (big[18:] == -1).all() and (bmin[18:] == -1).all()         # unknown contigs
        assert big[9, 3] == 3 * nbp - 40 + 5 + 1 and big[10, 3] == -1     # negative starts: 5 - qe + 1; 2^31 - 2 is out of reach
    finally:
        H.close()


def test_outputs_are_defined_and_bad_arguments_write_nothing(tmp):
    rng = random.Random(5300)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 3, 1, 6)
    db = ListDb(tmp, "a", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 40)
    H = NearestHost(db.path)
    try:
        # dmin may be NULL; an empty call is fine
        rc, dist, dmin = H.nearest(ichr, qs, qe, nbp, want_dmin=False)
        assert rc == 0 and np.array_equal(dist, ref_rows(db, ichr, qs, qe, nbp)[0]) and (dmin == 0x5a5a5a5a).all()
        rc, dist, _ = H.nearest(ichr[:0], qs[:0], qe[:0], nbp)
        assert rc == 0 and dist.shape == (0, 3)
        # a window out of range and a bad set_off are refused before anything is written
        for W in (-1, MAX_WINDOW + 1, -2 ** 31):
            rc, dist, dmin = H.nearest(ichr, qs, qe, W)
            assert rc == -1 and (dist == 0x5a5a5a5a).all() and (dmin == 0x5a5a5a5a).all(), W
            rc, out = H.nearest_sets(ichr, qs, qe, [0, 40], W)
            assert rc == -1 and all((a == -77).all() for a in out), W
        for off in ([1, 40], [0, 30, 20, 40]):
            rc, out = H.nearest_sets(ichr, qs, qe, off, nbp)
            assert rc == -1 and all((a == -77).all() for a in out), off
        # only empty sets: every word is written, all zero
        rc, out = H.nearest_sets(ichr[:0], qs[:0], qe[:0], [0, 0, 0], nbp)
        assert rc == 0 and all(a.shape == (2, 4) and not a.any() for a in out)
    finally:
        H.close()


def test_python_entry_points_and_summary(tmp):
    rng = random.Random(5400)
    nbp = 1 << 11
    files, span = clustered_lists(rng, nbp, 4, 2, 12)
    db = ListDb(tmp, "p", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 2, nbp, span, 200)
    off = np.array([0, 0, 150, 200], np.int64)
    want, wmin = ref_rows(db, ichr, qs, qe, 700, 500)
    dist, dmin = igd_amd.nearest_host(db.path, ichr, qs, qe, 700, value_filter=500)
    assert dist.dtype == np.int32 and np.array_equal(dist, want) and np.array_equal(dmin, wmin)
    ns = igd_amd.nearest_sets_host(db.path, ichr, qs, qe, off, 700, value_filter=500)
    assert isinstance(ns, igd_amd.NearestSets) and ns.window == 700
    for got, ref in zip(ns[:3], ref_sets(want, wmin, off)):
        assert got.dtype == np.int64 and np.array_equal(got, ref)
    mean = igd_amd.nearest_summary(ns)
    assert mean.shape == ns.n_within.shape and np.isnan(mean[0]).all()
    nz = ns.n_within > 0
    assert nz.any() and np.array_equal(mean[nz], ns.sum_dist[nz] / ns.n_within[nz]) and np.isnan(mean[~nz]).all()
    with pytest.raises(igd_amd.database.IgdError):
        igd_amd.nearest_host(db.path, ichr, qs, qe, MAX_WINDOW + 1)
    with pytest.raises(igd_amd.database.IgdError):
        igd_amd.nearest_sets_host(db.path, ichr, qs, qe, off, -1)
    with pytest.raises(igd_amd.database.IgdError):
        igd_amd.nearest_host(db.path, ichr, qs, qe, 2 ** 40)
