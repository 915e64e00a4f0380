"""igd_hip_enrich_ranks / Database.enrichment_ranks (kernel igd_rank_rows): rank columns and Benjamini-Hochberg q-values of
an enrichment table on the GPU, against rank_ref.py (bounds there) and within twice its bound of the host route.  The number
of columns is the caller's, so a tiny database drives every width.  Outputs are pre-filled with a sentinel: every requested
cell must be stored.  (tests/test_gpu_rank.py is the merge join's rank method, another thing.)"""
import os
import shutil

import numpy as np
import pytest

import rank_ref as R
from helpers import GOLDEN
from test_rank_host import FIELDS, call_abi, host_fn, untouched

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def db():
    from igd_amd import Database
    d = Database(os.path.join(GOLDEN, "branch", "db.igd"))
    yield d
    d.close()


def gpu(db, sup, pv, odds, ask=FIELDS, shape=None):
    return call_abi(db._H.igd_hip_enrich_ranks, (db.dev,), sup, pv, odds, ask, shape)


def run_case(db, name, table, host=True):
    sup, pv, odds = table
    rc, got = gpu(db, sup, pv, odds)
    assert rc == 0, db._H.igd_hip_last_error()
    want = R.want_of(name, table)
    R.check(sup, pv, odds, got, want, name)
    if host:                                           # the GPU within twice the bound of the host route; the rest equal
        rc, h = call_abi(host_fn(), (), sup, pv, odds)
        assert rc == 0
        R.check(sup, pv, odds, got, h, name + " against the host route", scale=2.0)
    return got


@pytest.mark.parametrize("m", R.WIDTHS)
def test_widths_at_the_lane_workgroup_and_padding_edges(db, m):
    run_case(db, "width%d" % m, R.widths_case(m))


def test_both_sides_of_the_lds_limit(db):
    L = int(db._H.igd_hip_rank_lds_cols())
    assert 1024 < L <= 1 << 19
    for m in R.seam_widths(L):
        run_case(db, "seam%d" % m, R.seam_case(m), host=False)
    a, b = R.seam_padded_case(L)                       # the same data in the LDS form and, one lowest column wider, in the global form
    ga, gb = gpu(db, *a)[1], gpu(db, *b)[1]
    for f in ("rnk_sup", "rnk_pv", "rnk_or", "max_rnk"):
        np.testing.assert_array_equal(getattr(ga, f), getattr(gb, f)[:, :-1], err_msg=f)
    R.check(*a, ga, R.want_of("seam_padded", a), "seam_padded")


@pytest.mark.parametrize("m", [5, 70])
def test_workgroups_take_a_second_row(db, m):
    grid = int(db._H.igd_hip_rank_grid(10**9))
    assert 0 < grid <= 1 << 16 and int(db._H.igd_hip_rank_grid(3)) == 3
    run_case(db, "second_rows%d_%d" % (m, grid), R.second_rows_case(grid, m))


def test_two_launches_with_the_seam_between_rows(db):
    run_case(db, "two_launches", R.two_launches_case(), host=False)


def test_ties(db):
    cases = R.ties_cases()
    got = {name: run_case(db, name, cases[name]) for name in cases}
    g = got["all_equal"]
    assert all((a == 1).all() for a in g[1:5]) and (g.mean_rnk == 1.0).all()
    for name in ("all_equal", "all_zero_p"):
        assert (got[name].rnk_pv == 1).all()
        assert (got[name].qvalue_log.view(np.int64) == np.ascontiguousarray(cases[name][1], np.float64).view(np.int64)).all()


def test_odds_column_with_inf_and_nan(db):
    cases = R.odds_cases()
    got = {name: run_case(db, name, cases[name]) for name in cases}
    r = got["odds9"].rnk_or
    assert (r[0] == 1).all()                           # only NaN: all tie, no number above them
    # 3.5 inf nan 0 1e-300 .25 nan 0 7: inf, the finite values, the zeros, the NaN
    np.testing.assert_array_equal(r[1], [3, 1, 8, 6, 5, 4, 8, 6, 2])
    np.testing.assert_array_equal(r[2], [1, 5, 1, 1, 8, 9, 7, 1, 5])


def test_supports_are_compared_as_64_bit_values(db):
    got = run_case(db, "keys64", R.keys64_case())
    np.testing.assert_array_equal(got.rnk_sup, [[5, 4, 3, 2, 1], [1, 2, 3, 4, 5], [2, 5, 1, 3, 4]])


def test_benjamini_hochberg_shapes(db):
    cases = R.bh_cases()
    got = {name: run_case(db, name, cases[name]) for name in cases}
    q = got["suffix"].qvalue_log[0]
    assert q[2] == q[1] and abs(q[1] - 1.3979400086720377) < 1e-12          # .03 takes .04 from the less significant cell
    q = got["clamp"].qvalue_log
    assert (q[0] == 0.02).all() and q[1, 1] == 0.0 and not np.signbit(q[1, 1])
    q = got["huge"].qvalue_log
    assert np.isfinite(q).all() and abs(q[0, 0] - (4609.06 - np.log10(2))) < 1e-8 and q[0, 1] == 1e-9


def test_null_outputs_and_inputs(db):
    sup, pv, odds = R.widths_case(257)
    want = R.want_of("width257", (sup, pv, odds))
    rc, got = gpu(db, None, pv, None, ask=("qvalue_log",))
    assert rc == 0 and untouched(got[1:])
    R.check(sup, pv, odds, got, want, "q only", only=("qvalue_log",))
    rc, got = gpu(db, sup, None, None, ask=("rnk_sup",))
    assert rc == 0 and untouched((got.qvalue_log,) + got[2:])
    R.check(sup, pv, odds, got, want, "rnk_sup only", only=("rnk_sup",))
    rc, got = gpu(db, sup, pv, odds, ask=("max_rnk",))
    assert rc == 0 and untouched(got[:4] + got[5:])
    R.check(sup, pv, odds, got, want, "max only", only=("max_rnk",))
    for missing in range(3):
        args = [sup, pv, odds]
        args[missing] = None
        rc, got = gpu(db, *args, ask=("max_rnk",))
        assert rc != 0 and untouched(got), missing


def test_refusals_leave_the_outputs_at_the_sentinel(db):
    sup, pv, odds = R.widths_case(65)
    for bad in (-1e-300, np.nan):
        p2 = pv.copy()
        p2[6, 64] = bad
        rc, got = gpu(db, sup, p2, odds)
        assert rc != 0 and untouched(got), bad
        assert b"pvalue_log" in db._H.igd_hip_last_error()
    z = np.zeros((1, 4))
    rc, got = gpu(db, z, z, z, shape=(1, (1 << 20) + 1))                      # refused from the shape alone
    assert rc != 0 and untouched(got)
    for shape in ((0, 4), (1, 0)):
        rc, got = gpu(db, z, z, z, shape=shape)
        assert rc == 0 and untouched(got)


def test_end_to_end_on_the_enrichment_fixture():
    """enrichment_sets on the 40-file fixture of test_gpu_enrich.py, then enrichment_ranks of its result"""
    from igd_amd import Database
    from igd_amd.database import EnrichmentRanks
    from helpers import Oracle, short_tmpdir
    from test_enrich_host import enrich_fixture
    d = short_tmpdir("igk")
    try:
        path, upath, sets, _ = enrich_fixture(d, nfiles=40, name="ge")
        orc = Oracle(path)
        q = [orc.read_queries(p) for p in sets]
        uni = orc.read_queries(upath)
        orc.close()
        off = np.zeros(len(q) + 1, np.int64)
        off[1:] = np.cumsum([len(s[1]) for s in q])
        cat = [np.concatenate([s[i] for s in q]).astype(np.int32) for i in range(3)]
        with_db = Database(path)
        try:
            e = with_db.enrichment_sets(cat[0], cat[1], cat[2], off, uni[0], uni[1], uni[2])
            got = with_db.enrichment_ranks(e)
            again = with_db.enrichment_ranks(e.support, e.pvalue_log, e.odds_ratio)
        finally:
            with_db.close()
        assert isinstance(got, EnrichmentRanks) and got.rnk_pv.shape == (3, 40)
        assert (e.pvalue_log > 2).any() and (e.support == 0).any()
        R.check(e.support, e.pvalue_log, e.odds_ratio, got, R.reference(e.support, e.pvalue_log, e.odds_ratio), "end to end")
        assert all((a.view(np.int64) == b.view(np.int64)).all() if a.dtype == np.float64 else (a == b).all() for a, b in zip(got, again))
    finally:
        shutil.rmtree(d, ignore_errors=True)
