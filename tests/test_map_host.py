"""Values of the overlapping records per region and dataset without a GPU: igdc_map_host, igdc_map_sets_host and
igdc_map_summary (igd_hostpath.c) through ctypes and through igd_amd.map_host / map_sets_host / map_summary.

The expected values never come from the code under test: tests/map_ref.py restates the definition as a numpy broadcast over
the interval lists this test wrote itself.  Every integer must be equal.  The identities are held against igdc_nearest_host
at W = 0 and igdc_search_host under rule FLAT, product code of other walks that their own tests hold against the definition
and the oracle."""
import os
import random
import shutil

import numpy as np
import pytest

import igd_amd
from helpers import short_tmpdir
from map_ref import (I32_MAX, I32_MIN, NOV, OPS, ListDb, clustered_lists, mixed_regions, placed_db, placed_regions, ref_rows, ref_sets)
from test_nearest_host import NearestHost, set_offsets, tiled
from test_support_host import FLAT, NUMPY_DBS

GARBAGE32, GARBAGE64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a
OP_NO = {"count": 0, "sum": 1, "min": 2, "max": 3}


@pytest.fixture
def tmp():
    d = short_tmpdir("imp")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", str(t))
    os.environ.pop("IGD_HOST_THREADS", None)


class MapHost(NearestHost):
    """igdc_map_host / igdc_map_sets_host through ctypes; every output is handed over full of garbage"""

    def map(self, ichr, qs, qe, op, v=NOV, want_agg=True):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        count = np.full((len(qs), self.nfiles), GARBAGE32, np.int32)
        agg = np.full((len(qs), self.nfiles), GARBAGE64, np.int64)
        rc = self.L.igdc_map_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), OP_NO.get(op, op), v,
                                  count.ctypes.data if count.size else None, agg.ctypes.data if want_agg and agg.size else None)
        return rc, count, agg

    def map_sets(self, ichr, qs, qe, off, op, v=NOV):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        off = np.ascontiguousarray(off, dtype=np.int64)
        out = [np.full((len(off) - 1, self.nfiles), -77, np.int64) for _ in range(3)]
        rc = self.L.igdc_map_sets_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, off.ctypes.data,
                                       len(off) - 1, OP_NO.get(op, op), v, *[a.ctypes.data for a in out])
        return rc, out


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_route_equals_the_definition_on_the_four_database_shapes(case, tmp, host_threads):
    rng = random.Random(8100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles, min_value=-300)
    db = ListDb(tmp, "c%d" % case, files, nbp, gtype)
    ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 600)
    off = set_offsets(rng, len(qs))
    H = MapHost(db.path)
    try:
        assert H.nfiles == nfiles
        host_threads(1)
        for op in OPS:
            for v in (None, 500):
                if gtype == 0 and op != "count":                          # no values: refused, nothing written
                    rc, count, agg = H.map(ichr, qs, qe, op, NOV if v is None else v)
                    assert rc == -1 and (count == GARBAGE32).all() and (agg == GARBAGE64).all()
                    rc, out = H.map_sets(ichr, qs, qe, off, op)
                    assert rc == -1 and all((a == -77).all() for a in out)
                    continue
                want, wagg = ref_rows(db, ichr, qs, qe, op, v)
                rc, count, agg = H.map(ichr, qs, qe, op, NOV if v is None else v)
                assert rc == 0 and np.array_equal(count, want) and np.array_equal(agg, wagg), (op, v)
                rc, sets = H.map_sets(ichr, qs, qe, off, op, NOV if v is None else v)
                assert rc == 0
                for got, ref in zip(sets, ref_sets(want, wagg, off)):
                    assert np.array_equal(got, ref), (op, v)
                if op == "count":
                    assert np.array_equal(sets[1], sets[2])
                    assert (want > 1).any() and ((want == 0).any(axis=1) & (want > 0).any(axis=1)).any(), "fixture is vacuous"
        # the value filter changes something on gType 1 and nothing on gType 0
        a, b = ref_rows(db, ichr, qs, qe, "count", None)[0], ref_rows(db, ichr, qs, qe, "count", 500)[0]
        assert np.array_equal(a, b) == (gtype == 0)
        # thread counts 1, 2 and 7 agree (on enough regions for seven threads to start)
        op = "count" if gtype == 0 else "sum"
        want, wagg = ref_rows(db, ichr, qs, qe, op, 500)
        tc, ts, te, tw = tiled(ichr, qs, qe, want)
        ta = np.tile(wagg, (len(tw) // len(wagg), 1))
        for threads in (1, 2, 7):
            host_threads(threads)
            rc, count, agg = H.map(tc, ts, te, op, 500)
            assert rc == 0 and np.array_equal(count, tw) and np.array_equal(agg, ta), threads
    finally:
        H.close()


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_identities_with_nearest_and_search(case, tmp, host_threads):
    """count > 0 iff nearest(W = 0).dist == 0; n_hit == nearest_sets(W = 0).n_overlap[:, :nFiles]; over regions with 0 <= qs that
    start inside the contig's tiles the column sums of count are the hits of a search under rule FLAT"""
    rng = random.Random(8200 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    db = ListDb(tmp, "s%d" % case, files, nbp, gtype)
    ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 500)
    off = np.array([0, 1, 6, 6, len(qs)], np.int64)
    ntile = {c: max((e - 1) // nbp + 1 for recs in files for (cc, s, e, _) in recs if cc == "chr%d" % (c + 1)) for c in range(nctg)}
    ok = np.array([0 <= int(ichr[i]) < nctg and 0 <= int(qs[i]) < ntile[int(ichr[i])] * nbp for i in range(len(qs))])
    H = MapHost(db.path)
    try:
        host_threads(1)
        for v in (NOV, 500):
            rc, count, _ = H.map(ichr, qs, qe, "count", v, want_agg=False)
            assert rc == 0 and count.any()
            rc, dist, _ = H.nearest(ichr, qs, qe, 0, v)
            assert rc == 0 and np.array_equal(count > 0, dist == 0)
            rc, (nh, _, _) = H.map_sets(ichr, qs, qe, off, "count", v)
            rc2, (_, no, _) = H.nearest_sets(ichr, qs, qe, off, 0, v)
            assert rc == 0 and rc2 == 0 and np.array_equal(nh, no[:, :nfiles])
            hits, total = igd_amd.search_host(db.path, ichr[ok], qs[ok], qe[ok], value_filter=v, rule=FLAT)
            assert np.array_equal(count[ok].sum(axis=0), hits) and total == count[ok].sum()
    finally:
        H.close()


def test_placed_cases(tmp, host_threads):
    nbp = 1 << 14
    db = placed_db(tmp, nbp)
    (ichr, qs, qe), notes = placed_regions(nbp)
    H = MapHost(db.path)
    try:
        host_threads(1)
        ref = {}
        for op in OPS:
            for v in (None, 500):
                want, wagg = ref[op, v] = ref_rows(db, ichr, qs, qe, op, v)
                rc, count, agg = H.map(ichr, qs, qe, op, NOV if v is None else v)
                bad = np.flatnonzero((count != want).any(axis=1) | (agg != wagg).any(axis=1))
                assert rc == 0 and len(bad) == 0, (op, v, [(notes[i], count[i].tolist(), want[i].tolist(), agg[i].tolist(), wagg[i].tolist()) for i in bad])
        # what the placed cases are there for, read off the reference
        c, s = ref["sum", None]
        assert c[0, 0] == 1 and s[0, 0] == 321                            # five tiles under seven: once
        assert c[1, 0] == 0 and s[1, 0] == 0                              # book-ended: not counted
        assert c[2, 1] == 2 and s[2, 1] == 154                            # two equal records
        assert c[3, 2] == 3 and s[3, 2] == -902 and ref["min", None][1][3, 2] == -900 and ref["max", None][1][3, 2] == 3
        assert c[4, 2] == 2 and s[4, 2] == -1 and ref["min", None][1][4, 2] == I32_MIN and ref["max", None][1][4, 2] == I32_MAX
        assert ref["max", None][1][5, 2] == I32_MIN and ref["sum", None][1][5, 2] == I32_MIN
        assert c[6, 3] == 3 and s[6, 3] == 3 * I32_MAX > 2 ** 32          # the sum needs 64 bits
        assert ref["max", None][1][7, 4] == 800 and ref["min", None][1][7, 4] == 100 and ref["min", 500][1][7, 4] == 500
        assert ref["max", None][1][8, 4] == 499 and ref["count", 500][0][8, 4] == 0 and ref["max", 500][1][8, 4] == 0   # -v removes the maximum
        assert not c[10].any() and not c[11].any() and c[12, 0] == 1 and not c[13].any()
        assert c[14].tolist() == [2, 2, 5, 3, 5, 0]                       # all of int32: every record of chrA once
        assert c[15, 5] == 1 and not c[16].any() and c[17, 5] == 2 and s[17, 5] == 899
        assert c[18, 2] == 2 and c[19, 2] == 3                            # inverted and zero-length regions: the predicate decides
        assert not c[20].any() and np.array_equal(c[21], c[3]) and not c[22:].any()
    finally:
        H.close()


def test_outputs_are_defined_and_bad_arguments_write_nothing(tmp):
    rng = random.Random(8300)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 3, 1, 6)
    db = ListDb(tmp, "a", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 40)
    H = MapHost(db.path)
    try:
        # agg may be NULL under COUNT only; an empty call is fine
        rc, count, agg = H.map(ichr, qs, qe, "count", want_agg=False)
        assert rc == 0 and np.array_equal(count, ref_rows(db, ichr, qs, qe, "count")[0]) and (agg == GARBAGE64).all()
        rc, count, agg = H.map(ichr, qs, qe, "count")
        assert rc == 0 and np.array_equal(agg, count)
        for op in ("sum", "min", "max"):
            rc, count, agg = H.map(ichr, qs, qe, op, want_agg=False)
            assert rc == -1 and (count == GARBAGE32).all()
        rc, count, _ = H.map(ichr[:0], qs[:0], qe[:0], "sum")
        assert rc == 0 and count.shape == (0, 3)
        # an unknown op and a bad set_off are refused before anything is written
        for op in (-1, 4, 99):
            rc, count, agg = H.map(ichr, qs, qe, op)
            assert rc == -1 and (count == GARBAGE32).all() and (agg == GARBAGE64).all(), op
            rc, out = H.map_sets(ichr, qs, qe, [0, 40], op)
            assert rc == -1 and all((a == -77).all() for a in out), op
        for off in ([1, 40], [0, 30, 20, 40]):
            rc, out = H.map_sets(ichr, qs, qe, off, "sum")
            assert rc == -1 and all((a == -77).all() for a in out), off
        # only empty sets, and no set at all: every word is written, all zero
        rc, out = H.map_sets(ichr[:0], qs[:0], qe[:0], [0, 0, 0], "max")
        assert rc == 0 and all(a.shape == (2, 3) and not a.any() for a in out)
        rc, out = H.map_sets(ichr[:0], qs[:0], qe[:0], [0], "max")
        assert rc == 0 and all(a.shape == (0, 3) for a in out)
    finally:
        H.close()


def test_python_entry_points_and_summary(tmp):
    rng = random.Random(8400)
    nbp = 1 << 11
    files, span = clustered_lists(rng, nbp, 4, 2, 12, min_value=-200)
    db = ListDb(tmp, "p", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 2, nbp, span, 200)
    off = np.array([0, 0, 150, 200], np.int64)
    for op in OPS:
        want, wagg = ref_rows(db, ichr, qs, qe, op, 500 if op == "min" else None)
        count, agg = igd_amd.map_host(db.path, ichr, qs, qe, op, value_filter=500 if op == "min" else None)
        assert count.dtype == np.int32 and agg.dtype == np.int64 and np.array_equal(count, want) and np.array_equal(agg, wagg)
        ms = igd_amd.map_sets_host(db.path, ichr, qs, qe, off, op, value_filter=500 if op == "min" else None)
        assert isinstance(ms, igd_amd.MapSets) and ms.op == op
        for got, ref in zip(ms[:3], ref_sets(want, wagg, off)):
            assert got.dtype == np.int64 and np.array_equal(got, ref)
        mean_region, mean_pair = igd_amd.map_summary(ms)
        assert mean_region.shape == ms.n_hit.shape and np.isnan(mean_region[0]).all() and np.isnan(mean_pair[0]).all()
        nz = ms.n_hit > 0
        assert nz.any() and np.array_equal(mean_region[nz], ms.agg_sum[nz] / ms.n_hit[nz]) and np.isnan(mean_region[~nz]).all()
        if op == "sum":
            assert np.array_equal(mean_pair[nz], ms.agg_sum[nz] / ms.pairs[nz]) and np.isnan(mean_pair[~nz]).all()
        else:
            assert np.isnan(mean_pair).all()
    with pytest.raises(igd_amd.database.IgdError):
        igd_amd.map_host(db.path, ichr, qs, qe, "median")
    with pytest.raises(igd_amd.database.IgdError):
        igd_amd.map_sets_host(db.path, ichr, qs, qe, [0, 10, 5, 200], "sum")
    # a database without values: count works, the value ops raise
    g0 = ListDb(tmp, "g0", files, nbp, 0)
    count, agg = igd_amd.map_host(g0.path, ichr, qs, qe, "count", value_filter=500)
    assert np.array_equal(count, ref_rows(g0, ichr, qs, qe, "count")[0]) and np.array_equal(agg, count)
    with pytest.raises(igd_amd.database.IgdError):
        igd_amd.map_host(g0.path, ichr, qs, qe, "sum")
    with pytest.raises(igd_amd.database.IgdError):
        igd_amd.map_sets_host(g0.path, ichr, qs, qe, off, "max")
