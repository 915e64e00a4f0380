"""GPU: minimum overlap per pair -- igd_sets_count_ov / igd_sets_support_ov through Database.search_sets / support_sets /
enrichment_sets / permutation_support with `min_overlap=`.

Device, reference and host route are compared as integers.  The reference is tests/minoverlap_ref.py (the oracle's enumeration,
rule NEST, the predicate in integers; values for a filter looked up from the fixture); the host route is igdc_*_host_ov, which
tests/test_minoverlap_host.py holds against the same reference, and stands in for rule FLAT, which the enumeration does not
restate.  Every fixture is cut by its thresholds (minoverlap_ref.assert_cuts, asserted on the reference alone).

Shapes: tiles of 1, 127, 128, 129 and 257 records (the two steps of 64 per iteration, their tail, the early exit); queries over
three tiles with long records copied into each; pairs on the boundary ov * 10^6 == len * ppm and one bp short of it; ppm = 10^6
per term and for both; record lengths near 2^31; 1, 33 and 8 192 files (LDS form) and 8 193 (wide form); gType 0 and gType 1
with a value filter; both rules; sets of 0, 1, 4 096 and 4 097 queries; more slices than the grid has workgroups (the grid of
these kernels is a constant of 2 048 workgroups, which IGD_HIP_WG_PER_CU does not change: about 2 450 slices of 64 queries).
No number below comes from the kernels."""
import random
import shutil

import numpy as np
import pytest

import minoverlap_ref as R
import permute_ref as PR
from helpers import Oracle, short_tmpdir
from test_enrich_host import tables_from_supports

pytestmark = pytest.mark.gpu

NEST, FLAT = 0, 1
GARBAGE = 0x0123456789


@pytest.fixture(scope="module")
def tmp():
    d = short_tmpdir("igm")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def mo(t):
    from igd_amd import MinOverlap
    return MinOverlap(*t)


class Case:
    """a fixture with its database on the device, the oracle's pairs (computed once) and the host answers"""

    def __init__(self, fx):
        from igd_amd import Database
        self.fx, self.db = fx, Database(fx.path)
        orc = Oracle(fx.path)
        try:
            self.p = R.pairs(orc, fx.ichr, fx.qs, fx.qe)
        finally:
            orc.close()

    def ref(self, t, v=None):
        fx = self.fx
        k = R.keep(t, self.p, fx.qs, fx.qe, v, fx.values)
        if any(t) and v is None:
            print(fx.name, t, "pairs %d of %d, incidences %d of %d" % R.assert_cuts(fx.nfiles, self.p, R.keep(t, self.p, fx.qs, fx.qe)))
        return R.counts(fx.nfiles, self.p, k, fx.off)

    def dev(self, t, rule=NEST, vf=None):
        fx = self.fx
        m = None if t is None else mo(t)
        hits, tot = self.db.search_sets(fx.ichr, fx.qs, fx.qe, fx.off, rule=rule, value_filter=vf, min_overlap=m)
        sup, nhit = self.db.support_sets(fx.ichr, fx.qs, fx.qe, fx.off, rule=rule, value_filter=vf, min_overlap=m)
        return hits, tot, sup, nhit

    def host(self, t, rule, vf=None):
        import igd_amd
        fx = self.fx
        n = len(fx.off) - 1
        out = np.zeros((n, fx.nfiles), np.int64), np.zeros(n, np.int64), np.zeros((n, fx.nfiles), np.int64), np.zeros(n, np.int64)
        for k in range(n):
            a, b = fx.off[k], fx.off[k + 1]
            kw = dict(rule=rule, value_filter=vf, min_overlap=None if t is None else mo(t))
            out[0][k], out[1][k] = igd_amd.search_host(fx.path, fx.ichr[a:b], fx.qs[a:b], fx.qe[a:b], **kw)
            out[2][k], out[3][k] = igd_amd.support_host(fx.path, fx.ichr[a:b], fx.qs[a:b], fx.qe[a:b], **kw)
        return out

    def close(self):
        self.db.close()


def same(got, want, what):
    for g, w, name in zip(got, want, ("hits", "totals", "support", "nhit")):
        assert np.array_equal(g, w), (what, name)


def check(c, with_v, rules=True):
    """inactive = the plain entry points = the reference; every threshold of the fixture: device = reference (rule NEST) and
    device = host (both rules), with a value filter where the records have values"""
    fx = c.fx
    plain = c.ref((0, 0, 0))
    same(c.dev(None), plain, (fx.name, "no threshold"))
    same(c.dev((0, 0, 0)), plain, (fx.name, "inactive threshold"))
    for t in fx.thresholds:
        want = c.ref(t)
        same(c.dev(t), want, (fx.name, t))
        if rules:
            same(c.dev(t, NEST), c.host(t, NEST), (fx.name, t, "rule NEST"))
            same(c.dev(t, FLAT), c.host(t, FLAT), (fx.name, t, "rule FLAT"))
        if with_v:
            wv = c.ref(t, 500)
            assert 0 < wv[1].sum() < want[1].sum()
            same(c.dev(t, NEST, 500), wv, (fx.name, t, "v = 500"))
            if rules:
                same(c.dev(t, FLAT, 500), c.host(t, FLAT, 500), (fx.name, t, "rule FLAT, v = 500"))


@pytest.fixture(scope="module")
def tiles(tmp):
    c = Case(R.tiles_fixture(random.Random(11), tmp, set_sizes=(0, 1, 4096, 4097, 64)))
    yield c
    c.close()


def test_tile_sizes_long_records_and_sets_that_span_slices(tiles):
    """gType 1 with a value filter; sets of 0, 1, 4 096 and 4 097 queries (slices of 64: the larger sets span 64 and 65)"""
    assert list(np.diff(tiles.fx.off)) == [0, 1, 4096, 4097, 64]
    check(tiles, with_v=True)
    long_q = (tiles.fx.ichr == 1) & (tiles.fx.qe - tiles.fx.qs > 2 * tiles.fx.nbp)
    assert long_q.sum() > 100                                     # queries over three tiles, records copied into each of them


def test_gtype0(tmp):
    c = Case(R.tiles_fixture(random.Random(12), tmp, "tl0", gtype=0))
    try:
        check(c, with_v=False)
        # a value filter is ignored on a database without values, threshold or not
        same(c.dev(R.T_HALF, NEST, 500), c.ref(R.T_HALF), "gType 0, v ignored")
    finally:
        c.close()


@pytest.mark.parametrize("nfiles", [1, 33, 8192, 8193])
def test_file_counts_at_the_edges_of_the_lds_and_wide_forms(nfiles, tmp):
    c = Case(R.wide_fixture(random.Random(100 + nfiles), tmp, nfiles))
    try:
        if nfiles > 1:
            inc = np.unique(c.p[1])
            assert inc[0] == 0 and inc[-1] == nfiles - 1          # the first and the last counter and bitmap bit are used
        check(c, with_v=True, rules=nfiles <= 33)
    finally:
        c.close()


def test_boundaries_full_containment_and_degenerate_queries(tmp):
    c = Case(R.boundary_fixture(tmp))
    fx = c.fx
    try:
        check(c, with_v=True)
        for q, t, counted in fx.cases:
            sl = slice(q, q + 1)
            m = mo(t) if any(t) else None
            hits, tot = c.db.search_sets(fx.ichr[sl], fx.qs[sl], fx.qe[sl], [0, 1], rule=NEST, min_overlap=m)
            sup, nhit = c.db.support_sets(fx.ichr[sl], fx.qs[sl], fx.qe[sl], [0, 1], rule=NEST, min_overlap=m)
            assert tot[0] == hits.sum() == sup.sum() == nhit[0] == counted, (q, t, counted)
        z = fx.qe <= fx.qs                                        # zero-length and inverted: counted without, never with
        assert z.sum() == 2
        one = np.arange(z.sum() + 1, dtype=np.int64)
        assert list(c.db.support_sets(fx.ichr[z], fx.qs[z], fx.qe[z], one, rule=NEST)[1]) == [1, 1]
        assert list(c.db.search_sets(fx.ichr[z], fx.qs[z], fx.qe[z], one, rule=NEST, min_overlap=mo((0, 0, 0)))[1]) == [1, 1]
        for t in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            assert not c.db.search_sets(fx.ichr[z], fx.qs[z], fx.qe[z], one, rule=NEST, min_overlap=mo(t))[0].any()
            assert not c.db.support_sets(fx.ichr[z], fx.qs[z], fx.qe[z], one, rule=NEST, min_overlap=mo(t))[1].any()
    finally:
        c.close()


def test_lengths_near_2_31_need_the_64_bit_products(tmp):
    """few launches: one query walks 32 768 tiles"""
    c = Case(R.big_fixture(tmp))
    try:
        fx = c.fx
        lenr = c.p[3] - c.p[2]
        ov = np.minimum(fx.qe.astype(np.int64)[c.p[0]], c.p[3]) - np.maximum(fx.qs.astype(np.int64)[c.p[0]], c.p[2])
        assert ov.max() >= 2 ** 30 - 8 and lenr.max() > 2 ** 31 - 2000 and fx.qe.max() == 2 ** 31 - 1
        for t in fx.thresholds:                                   # a 32-bit product would decide some pair the other way
            wrapped = ((ov * R.PPM) & 0xffffffff) >= ((lenr * t[2]) & 0xffffffff)
            assert (wrapped != (ov * R.PPM >= lenr * t[2])).any()
            same(c.dev(t), c.ref(t), (fx.name, t))
        t = fx.thresholds[1]
        same(c.dev(t, FLAT, 500), c.host(t, FLAT, 500), (fx.name, t, "rule FLAT, v = 500"))
        same(c.dev(t, NEST, 500), c.ref(t, 500), (fx.name, t, "v = 500"))
    finally:
        c.close()


def test_more_slices_than_workgroups(tiles):
    """the tiles fixture's queries 19 times over in three sets: about 2 450 slices of 64 queries on a grid of 2 048 workgroups,
    so some 400 workgroups take a second slice; the expected rows are the one-set reference times the repeats (counts add up)"""
    fx = tiles.fx
    nq = len(fx.qs)
    reps = (3, 7, 9)
    assert sum(reps) * nq // 64 > 2048 and sum(reps) * nq <= 4096 * 64
    ichr, qs, qe = (np.tile(a, sum(reps)) for a in (fx.ichr, fx.qs, fx.qe))
    off = np.concatenate([[0], np.cumsum(reps)]) * nq
    for t in (R.T_HALF, R.T_BP):
        k = R.keep(t, tiles.p, fx.qs, fx.qe)
        base = R.counts(fx.nfiles, tiles.p, k, [0, nq])
        hits, tot = tiles.db.search_sets(ichr, qs, qe, off, rule=NEST, min_overlap=mo(t))
        sup, nhit = tiles.db.support_sets(ichr, qs, qe, off, rule=NEST, min_overlap=mo(t))
        for j, r in enumerate(reps):
            same((hits[j], tot[j], sup[j], nhit[j]), [r * x[0] for x in base], (t, j))


def test_enrichment_tables_are_built_from_thresholded_supports(tiles):
    fx = tiles.fx
    off = fx.off[:4]                                              # sets 0..2 (0, 1 and 4 096 regions); the universe: set 3
    a, b = fx.off[3], fx.off[4]
    n = off[-1]
    for t in (R.T_HALF, R.T_BP):
        _, _, sup, _ = tiles.ref(t)
        e = tiles.db.enrichment_sets(fx.ichr[:n], fx.qs[:n], fx.qe[:n], off, fx.ichr[a:b], fx.qs[a:b], fx.qe[a:b], rule=NEST, min_overlap=mo(t))
        plain = tiles.db.enrichment_sets(fx.ichr[:n], fx.qs[:n], fx.qe[:n], off, fx.ichr[a:b], fx.qs[a:b], fx.qe[a:b], rule=NEST)
        assert np.array_equal(e.support, sup[:3]) and np.array_equal(e.usupport, sup[3]) and (e.usupport < plain.usupport).any()
        for k in range(3):
            tb, tc, td, cl = tables_from_supports(sup[k], sup[3], int(off[k + 1] - off[k]), int(b - a))
            assert np.array_equal(e.b[k], tb) and np.array_equal(e.c[k], tc) and np.array_equal(e.d[k], td) and e.clamped[k] == cl
        p, o = tiles.db.fisher(e.support.ravel(), e.b.ravel(), e.c.ravel(), e.d.ravel())
        assert np.array_equal(p, e.pvalue_log.ravel()) and np.array_equal(o, e.odds_ratio.ravel(), equal_nan=True)


@pytest.mark.parametrize("mode", ["circular", "shuffle"])
def test_permutation_null_counts_every_row_under_the_threshold(tiles, mode):
    fx, db = tiles.fx, tiles.db
    ctg_len = np.array([6 * fx.nbp, 8 * fx.nbp], np.int32)
    ok = fx.qe <= ctg_len[fx.ichr]
    ichr, qs, qe = fx.ichr[ok][:700], fx.qs[ok][:700], fx.qe[ok][:700]
    nq, nperm = len(qs), 8
    for t in (R.T_BP, R.T_HALF):
        got = db.permutation_support(ichr, qs, qe, ctg_len, nperm, seed=9, mode=mode, rule=NEST, min_overlap=mo(t))
        plain = db.permutation_support(ichr, qs, qe, ctg_len, nperm, seed=9, mode=mode, rule=NEST)
        ps, pe = db.permute_regions(ichr, qs, qe, ctg_len, 0, nperm, seed=9, mode=mode)
        rs, re_ = PR.permute(ichr, qs, qe, ctg_len, 0, nperm, 9, PR.SHUFFLE if mode == "shuffle" else PR.CIRCULAR)
        assert np.array_equal(ps, rs) and np.array_equal(pe, re_)
        sup, nhit = db.support_sets(np.tile(ichr, nperm), ps.ravel(), pe.ravel(), np.arange(nperm + 1, dtype=np.int64) * nq, rule=NEST,
                                    min_overlap=mo(t))
        rows = np.concatenate([sup, nhit[:, None]], axis=1)
        osup, onhit = db.support_sets(ichr, qs, qe, [0, nq], rule=NEST, min_overlap=mo(t))
        obs = np.concatenate([osup[0], onhit])
        assert np.array_equal(got.observed, obs) and (got.observed < plain.observed).any() and got.sum.sum() < plain.sum.sum()
        st = db.perm_stats(rows, obs)
        for g, w, r, name in zip(got[1:7], st, PR.stats(rows, obs), ("sum", "sumsq", "n_ge", "n_le", "min", "max")):
            assert np.array_equal(g, w) and np.array_equal(g, r), (t, name)
        # and the rows themselves are the reference's: the oracle's pairs of the permuted regions under the predicate
        orc = Oracle(fx.path)
        try:
            p = R.pairs(orc, np.tile(ichr, nperm), ps.ravel(), pe.ravel())
        finally:
            orc.close()
        _, _, rsup, rnhit = R.counts(fx.nfiles, p, R.keep(t, p, ps.ravel(), pe.ravel()), np.arange(nperm + 1) * nq)
        assert np.array_equal(sup, rsup) and np.array_equal(nhit, rnhit)


def test_existing_entry_points_still_add_into_the_callers_arrays(tiles):
    """igd_hip_search_sets / igd_hip_support_sets (no threshold argument) and their `_ov` forms with NULL and with a threshold,
    into matrices pre-filled with known values: all of them ADD"""
    import ctypes as C
    from igd_amd import _native as N
    fx, db = tiles.fx, tiles.db
    H = N.hip()
    n = len(fx.off) - 1
    q = [np.ascontiguousarray(a, np.int32) for a in (fx.ichr, fx.qs, fx.qe)]
    args = [db.dev] + [a.ctypes.data for a in q] + [fx.off.ctypes.data, n, -2 ** 31, NEST]
    plain, thr = tiles.ref((0, 0, 0)), tiles.ref(R.T_HALF)
    m = mo(R.T_HALF)
    base = (np.arange(n * fx.nfiles, dtype=np.int64).reshape(n, fx.nfiles) * 1000 + GARBAGE)
    tb = np.arange(n, dtype=np.int64) * 77 + 5
    for call, extra, want in ((H.igd_hip_search_sets, (), plain), (H.igd_hip_search_sets_ov, (None,), plain), (H.igd_hip_search_sets_ov, (C.byref(m),), thr)):
        rows, tot = base.copy(), tb.copy()
        assert call(*args, 0, rows.ctypes.data, tot.ctypes.data, *extra) == 0
        assert np.array_equal(rows - base, want[0]) and np.array_equal(tot - tb, want[1])
    for call, extra, want in ((H.igd_hip_support_sets, (), plain), (H.igd_hip_support_sets_ov, (None,), plain), (H.igd_hip_support_sets_ov, (C.byref(m),), thr)):
        rows, tot = base.copy(), tb.copy()
        assert call(*args, rows.ctypes.data, tot.ctypes.data, *extra) == 0
        assert np.array_equal(rows - base, want[2]) and np.array_equal(tot - tb, want[3])
    # a field out of range is refused before anything is written
    bad = (C.c_int32 * 3)(0, 0, 1000001)
    rows, tot = base.copy(), tb.copy()
    assert H.igd_hip_support_sets_ov(*args, rows.ctypes.data, tot.ctypes.data, C.byref(bad)) == -2
    assert H.igd_hip_search_sets_ov(*args, 0, rows.ctypes.data, tot.ctypes.data, C.byref(bad)) == -2
    assert np.array_equal(rows, base) and np.array_equal(tot, tb)


def test_large_set_route_is_not_taken_under_a_threshold(tiles, monkeypatch):
    """IGD_SETS_BIG_MIN = 1 sends every set of the plain call through the batch pipeline; with a threshold every set is cut into
    slices all the same, and the plain call's rows do not depend on the route"""
    want, plain = tiles.ref(R.T_MIX), tiles.ref((0, 0, 0))
    monkeypatch.setenv("IGD_SETS_BIG_MIN", "1")
    same(tiles.dev(R.T_MIX), want, "threshold, IGD_SETS_BIG_MIN = 1")
    same(tiles.dev(None), plain, "plain, IGD_SETS_BIG_MIN = 1")
