"""Minimum overlap per pair without a GPU: igdc_search_host_ov / igdc_support_host_ov / igdc_permute_host_ov (igd_hostpath.c)
through igd_amd.search_host / support_host / permute_host, and igd_amd.MinOverlap.

Expected values come from tests/minoverlap_ref.py: the oracle's enumeration, the predicate in integers, counted.  Every fixture
is first shown to be cut by its thresholds (minoverlap_ref.assert_cuts, on the reference alone)."""
import random
import shutil

import numpy as np
import pytest

import minoverlap_ref as R
from helpers import Oracle, short_tmpdir

NEST, FLAT = 0, 1


@pytest.fixture(scope="module")
def tmp():
    d = short_tmpdir("imo")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def fixtures(tmp):
    return {"tiles": R.tiles_fixture(random.Random(11), tmp), "tiles0": R.tiles_fixture(random.Random(12), tmp, "tl0", gtype=0),
            "w33": R.wide_fixture(random.Random(13), tmp, 33), "big": R.big_fixture(tmp), "bd": R.boundary_fixture(tmp)}


def mo(t):
    from igd_amd import MinOverlap
    return MinOverlap(*t)


def host_rows(fx, t, rule=None, vf=None, v=0):
    """search_host and support_host per set: (hits, totals, support, nhit) as minoverlap_ref.counts returns them"""
    import igd_amd
    n = len(fx.off) - 1
    hits, sup = np.zeros((n, fx.nfiles), np.int64), np.zeros((n, fx.nfiles), np.int64)
    tot, nhit = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for k in range(n):
        a, b = fx.off[k], fx.off[k + 1]
        kw = dict(v=v, rule=rule, value_filter=vf, min_overlap=None if t is None else mo(t))
        hits[k], tot[k] = igd_amd.search_host(fx.path, fx.ichr[a:b], fx.qs[a:b], fx.qe[a:b], **kw)
        sup[k], nhit[k] = igd_amd.support_host(fx.path, fx.ichr[a:b], fx.qs[a:b], fx.qe[a:b], **kw)
    return hits, tot, sup, nhit


def same(got, want, what):
    for g, w, name in zip(got, want, ("hits", "totals", "support", "nhit")):
        assert np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("name", ["tiles", "tiles0", "w33", "big", "bd"])
def test_host_twins_equal_the_reference(name, fixtures):
    fx = fixtures[name]
    orc = Oracle(fx.path)
    try:
        p = R.pairs(orc, fx.ichr, fx.qs, fx.qe)
        plain = R.counts(fx.nfiles, p, R.keep((0, 0, 0), p, fx.qs, fx.qe), fx.off)
        same(host_rows(fx, None, NEST), plain, (name, "no threshold"))
        same(host_rows(fx, (0, 0, 0), NEST), plain, (name, "inactive threshold"))
        for t in fx.thresholds:
            k = R.keep(t, p, fx.qs, fx.qe)
            print(name, t, "pairs %d of %d, incidences %d of %d" % R.assert_cuts(fx.nfiles, p, k))
            same(host_rows(fx, t, NEST), R.counts(fx.nfiles, p, k, fx.off), (name, t))
            if fx.gtype == 1:                                     # a value filter on top, values looked up from the fixture
                kv = R.keep(t, p, fx.qs, fx.qe, 500, fx.values)
                assert 0 < kv.sum() < k.sum()
                same(host_rows(fx, t, NEST, 500), R.counts(fx.nfiles, p, kv, fx.off), (name, t, "v"))
    finally:
        orc.close()


def test_numpy_predicate_is_the_python_integer_predicate(fixtures):
    for name in ("tiles", "big", "bd"):
        fx = fixtures[name]
        orc = Oracle(fx.path)
        try:
            p = R.pairs(orc, fx.ichr, fx.qs, fx.qe)
        finally:
            orc.close()
        for t in fx.thresholds + [R.T_Q_INSIDE, R.T_R_INSIDE, (0, R.PPM, R.PPM), (0, 0, 0)]:
            k = R.keep(t, p, fx.qs, fx.qe)
            lit = [R.qualifies(t, fx.qs[q], fx.qe[q], s, e) for q, s, e in zip(p[0], p[2], p[3])]
            assert k.tolist() == lit, (name, t)


def test_boundaries_equality_qualifies_one_bp_less_does_not(fixtures):
    import igd_amd
    fx = fixtures["bd"]
    orc = Oracle(fx.path)
    try:
        for q, t, counted in fx.cases:
            sl = slice(q, q + 1)
            p = R.pairs(orc, fx.ichr[sl], fx.qs[sl], fx.qe[sl])
            assert len(p[0]) == 1, "query %d of the boundary fixture meets %d records, not 1" % (q, len(p[0]))
            assert int(R.keep(t, p, fx.qs[sl], fx.qe[sl]).sum()) == counted, (q, t)
            hits, tot = igd_amd.search_host(fx.path, fx.ichr[sl], fx.qs[sl], fx.qe[sl], rule=NEST, min_overlap=mo(t))
            sup, nhit = igd_amd.support_host(fx.path, fx.ichr[sl], fx.qs[sl], fx.qe[sl], rule=NEST, min_overlap=mo(t))
            assert tot == hits.sum() == sup.sum() == nhit == counted, (q, t, counted)
    finally:
        orc.close()


def test_min_bp_1_equals_the_plain_search_on_well_formed_queries(fixtures):
    for name in ("tiles", "tiles0", "w33", "big"):
        fx = fixtures[name]
        assert (fx.qe > fx.qs).all()
        for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300)):
            same(host_rows(fx, (1, 0, 0), rule, vf), host_rows(fx, None, rule, vf), (name, rule, vf))


def test_both_rules_and_the_cli_dispatch_differ_only_where_the_plain_search_does(tmp):
    """rule FLAT against rule NEST on a database with empty tiles: the thresholded counts are the plain ones filtered -- the
    host walks the tiles of either rule and then applies the one predicate (the reference restates rule NEST only)"""
    import igd_amd
    rng = random.Random(21)
    nbp = 1 << 12
    files = [[("chr1", s, s + rng.randint(50, 3 * nbp), rng.randint(1, 1000)) for s in rng.sample(range(0, 100 * nbp, 7), 60)] for _ in range(3)]
    ic, qs = np.zeros(800, np.int32), np.array([rng.randrange(0, 100 * nbp) for _ in range(800)], np.int32)
    fx = R.Fixture(tmp, "sparse", nbp, 1, files, (ic, qs, qs + np.array([rng.randint(1, 4 * nbp) for _ in range(800)], np.int32)),
                   [0, 800], [R.T_BP])
    nest, flat = host_rows(fx, None, NEST), host_rows(fx, None, FLAT)
    assert nest[1][0] < flat[1][0], "the two rules do not differ on this fixture"
    t = (400, 300000, 0)
    tn, tf = host_rows(fx, t, NEST), host_rows(fx, t, FLAT)
    assert 0 < tn[1][0] < nest[1][0] and tn[1][0] < tf[1][0] < flat[1][0]
    orc = Oracle(fx.path)
    try:
        p = R.pairs(orc, fx.ichr, fx.qs, fx.qe)
        same(tn, R.counts(fx.nfiles, p, R.keep(t, p, fx.qs, fx.qe), fx.off), "rule NEST")
    finally:
        orc.close()
    # the dispatch of `-v`: v = 1 is rule FLAT with a filter that every record passes
    got = igd_amd.support_host(fx.path, fx.ichr, fx.qs, fx.qe, v=1, min_overlap=mo(t))
    assert np.array_equal(got[0], tf[2][0]) and got[1] == tf[3][0]


def test_permute_host_counts_every_row_under_the_threshold(fixtures):
    import igd_amd
    fx = fixtures["tiles"]
    ctg_len = np.array([6 * fx.nbp, 8 * fx.nbp], np.int32)
    ok = fx.qe <= ctg_len[fx.ichr]
    ichr, qs, qe = fx.ichr[ok][:300], fx.qs[ok][:300], fx.qe[ok][:300]
    t = R.T_BP
    for mode in ("circular", "shuffle"):
        got = igd_amd.permute_host(fx.path, ichr, qs, qe, ctg_len, 8, seed=5, mode=mode, rule=NEST, min_overlap=mo(t))
        plain = igd_amd.permute_host(fx.path, ichr, qs, qe, ctg_len, 8, seed=5, mode=mode, rule=NEST)
        none = igd_amd.permute_host(fx.path, ichr, qs, qe, ctg_len, 8, seed=5, mode=mode, rule=NEST, min_overlap=mo((0, 0, 0)))
        assert all(np.array_equal(a, b) for a, b in zip(plain[:7], none[:7]))
        ps, pe = igd_amd.permute_regions_host(ichr, qs, qe, ctg_len, 0, 8, seed=5, mode=mode)
        rows = np.zeros((8, fx.nfiles + 1), np.int64)
        for r in range(8):
            rows[r, :fx.nfiles], rows[r, fx.nfiles] = igd_amd.support_host(fx.path, ichr, ps[r], pe[r], rule=NEST, min_overlap=mo(t))
        obs = np.concatenate(igd_amd.support_host(fx.path, ichr, qs, qe, rule=NEST, min_overlap=mo(t))[:1] + (
            [igd_amd.support_host(fx.path, ichr, qs, qe, rule=NEST, min_overlap=mo(t))[1]],))
        assert np.array_equal(got.observed, obs) and (got.observed < plain.observed).any()
        assert np.array_equal(got.sum, rows.sum(axis=0)) and np.array_equal(got.sumsq, (rows * rows).sum(axis=0))
        assert np.array_equal(got.n_ge, (rows >= obs).sum(axis=0)) and np.array_equal(got.n_le, (rows <= obs).sum(axis=0))
        assert np.array_equal(got.min, rows.min(axis=0)) and np.array_equal(got.max, rows.max(axis=0))
        assert got.sum.sum() < plain.sum.sum()


def test_min_overlap_objects_and_refusals(fixtures):
    import igd_amd
    from igd_amd import MinOverlap
    from igd_amd.database import IgdError
    fx = fixtures["tiles"]
    m = MinOverlap.from_fractions(10, 0.5, 0.000001)
    assert (m.bp, m.query_ppm, m.record_ppm) == (10, 500000, 1) and m.active and not MinOverlap().active
    assert MinOverlap.from_fractions(0, 1, 1).query_ppm == 1000000 and MinOverlap.from_fractions(0, 0.3333335, 0).query_ppm == 333334
    for bad in (dict(query=1.5), dict(record=-0.1), dict(query=float("nan"))):
        with pytest.raises(IgdError):
            MinOverlap.from_fractions(0, **bad)
    for bad in (dict(bp=-1), dict(query_ppm=1000001), dict(record_ppm=-1), dict(bp=2 ** 31), dict(bp=1.5)):
        with pytest.raises(IgdError):
            MinOverlap(**bad)
    with pytest.raises(IgdError):
        igd_amd.support_host(fx.path, fx.ichr, fx.qs, fx.qe, min_overlap="50")
    a = igd_amd.support_host(fx.path, fx.ichr, fx.qs, fx.qe, min_overlap=50)          # a bare int is base pairs
    b = igd_amd.support_host(fx.path, fx.ichr, fx.qs, fx.qe, min_overlap=MinOverlap(bp=50))
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    # a field out of range reaches the C functions only around the class: they refuse it and write nothing
    import ctypes as C
    from igd_amd import _native as N
    from test_support_host import HostDb
    H = HostDb(fx.path)
    try:
        raw = (C.c_int32 * 3)(0, 1000001, 0)
        sup = np.full(fx.nfiles, 7, np.int64)
        nh = C.c_int64(3)
        q = [np.ascontiguousarray(x, np.int32) for x in (fx.ichr, fx.qs, fx.qe)]
        assert N.cli().igdc_support_host_ov(H.core, H.m, *[x.ctypes.data for x in q], len(q[0]), -2 ** 31, NEST, sup.ctypes.data, C.byref(nh),
                                            C.byref(raw)) == -1
        assert (sup == 7).all() and nh.value == 3
    finally:
        H.close()
