"""igdc_rank_host / igd_amd.rank_host: the rank columns and Benjamini-Hochberg q-values of an enrichment table on the host
route, against rank_ref.py on every row the GPU tests (test_gpu_enrich_rank.py) name, through the C entry point with all
outputs pre-filled with a sentinel; the argument refusals, which leave the sentinel; and the Python face."""
import ctypes as C

import numpy as np
import pytest

import rank_ref as R

SENT_I, SENT_D = -7, -1.5
FIELDS = R.Ranks._fields


def sentinel_outputs(shape):
    return R.Ranks(np.full(shape, SENT_D), *(np.full(shape, SENT_I, np.int32) for _ in range(4)), np.full(shape, SENT_D))


def untouched(out):
    return all((a == (SENT_D if a.dtype == np.float64 else SENT_I)).all() for a in out if a is not None)


def call_abi(fn, head, sup, pv, odds, ask=FIELDS, shape=None):
    """fn(*head, support, pvalue_log, odds_ratio, nrows, ncols, six outputs): inputs may be None (NULL), only the outputs
    named in `ask` are passed; returns (rc, Ranks of sentinel-filled arrays)"""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in zip((sup, pv, odds), (np.int64, np.float64, np.float64))]
    if shape is None:
        shape = next(a.shape for a in arrs if a is not None)
    out = sentinel_outputs(shape)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = fn(*head, *(ptr(a) for a in arrs), shape[0], shape[1], *(ptr(getattr(out, f)) if f in ask else None for f in FIELDS))
    return rc, out


def host_fn():
    from igd_amd import _native as N
    return N.cli().igdc_rank_host


CASES = R.all_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_row_of_the_gpu_tests_through_the_host_route(name):
    sup, pv, odds = CASES[name]
    rc, got = call_abi(host_fn(), (), sup, pv, odds)
    assert rc == 0
    R.check(sup, pv, odds, got, R.want_of(name, CASES[name]), name)


def test_all_equal_rows_rank_one_and_keep_p_bit_for_bit():
    for name in ("all_equal", "all_zero_p"):
        sup, pv, odds = CASES[name]
        rc, got = call_abi(host_fn(), (), sup, pv, odds)
        assert rc == 0 and (got.rnk_pv == 1).all()
        assert (got.qvalue_log.view(np.int64) == np.ascontiguousarray(pv, np.float64).view(np.int64)).all()
    rc, got = call_abi(host_fn(), (), *CASES["all_equal"])
    assert all((a == 1).all() for a in got[1:5]) and (got.mean_rnk == 1.0).all()


def test_lowest_extra_column_leaves_the_other_ranks():
    a, b = R.seam_padded_case(R.LDS_COLS)
    ga, gb = call_abi(host_fn(), (), *a)[1], call_abi(host_fn(), (), *b)[1]
    for f in ("rnk_sup", "rnk_pv", "rnk_or", "max_rnk"):
        np.testing.assert_array_equal(getattr(ga, f), getattr(gb, f)[:, :-1])


def test_null_outputs_and_inputs():
    sup, pv, odds = R.widths_case(65)
    want = R.want_of("width65", (sup, pv, odds))
    rc, got = call_abi(host_fn(), (), None, pv, None, ask=("qvalue_log",))
    assert rc == 0 and untouched(got[1:])
    R.check(sup, pv, odds, got, want, "q only", only=("qvalue_log",))
    rc, got = call_abi(host_fn(), (), sup, None, None, ask=("rnk_sup",))
    assert rc == 0 and untouched((got.qvalue_log,) + got[2:])
    R.check(sup, pv, odds, got, want, "rnk_sup only", only=("rnk_sup",))
    rc, got = call_abi(host_fn(), (), sup, pv, odds, ask=("mean_rnk",))
    assert rc == 0 and untouched(got[:5])
    R.check(sup, pv, odds, got, want, "mean only", only=("mean_rnk",))


def test_refusals_leave_the_outputs_at_the_sentinel():
    sup, pv, odds = R.widths_case(65)
    for missing in range(3):                           # max_rnk / mean_rnk need all three inputs
        args = [sup, pv, odds]
        args[missing] = None
        for ask in (("max_rnk",), ("mean_rnk",), FIELDS):
            rc, got = call_abi(host_fn(), (), *args, ask=ask)
            assert rc != 0 and untouched(got), (missing, ask)
    rc, got = call_abi(host_fn(), (), sup, None, odds, ask=("qvalue_log",))
    assert rc != 0 and untouched(got)
    for bad in (-1e-300, -3.0, np.nan, -np.inf):
        p2 = pv.copy()
        p2[6, 64] = bad                                # the very last cell: everything before it is in order
        rc, got = call_abi(host_fn(), (), sup, p2, odds)
        assert rc != 0 and untouched(got), bad
    # more than 2^20 columns: refused from the shape alone (the arrays are never read)
    one = np.zeros((1, 1))
    rc, got = call_abi(host_fn(), (), one.astype(np.int64), one, one, shape=(1, 1))
    assert rc == 0
    out = sentinel_outputs((1, 1))
    big = (1 << 20) + 1
    z = np.zeros(big)
    rc = host_fn()(C.c_void_p(z.ctypes.data), C.c_void_p(z.ctypes.data), C.c_void_p(z.ctypes.data), 1, big,
                   *(C.c_void_p(a.ctypes.data) for a in out))
    assert rc != 0 and untouched(out)
    # no rows or no columns: fine, nothing written
    for shape in ((0, 5), (5, 0)):
        out = sentinel_outputs((1, 1))
        rc = host_fn()(None, None, None, shape[0], shape[1], *(C.c_void_p(a.ctypes.data) for a in out))
        assert rc == 0 and untouched(out)


def test_python_face():
    import igd_amd
    from igd_amd.database import Enrichment, EnrichmentRanks, IgdError
    sup, pv, odds = R.widths_case(257)
    want = R.want_of("width257", (sup, pv, odds))
    got = igd_amd.rank_host(sup, pv, odds)
    assert isinstance(got, EnrichmentRanks) and EnrichmentRanks._fields == FIELDS
    assert got.rnk_sup.dtype == np.int32 and got.mean_rnk.dtype == np.float64 and got.qvalue_log.shape == sup.shape
    R.check(sup, pv, odds, got, want, "rank_host")
    e = Enrichment(sup, None, None, None, None, pv, odds, None)
    again = igd_amd.rank_host(e)
    assert all((a == b).all() for a, b in zip(got, again))
    with pytest.raises(IgdError):
        igd_amd.rank_host(sup, pv)
    with pytest.raises(IgdError):
        igd_amd.rank_host(sup, pv[:, :-1], odds)
    with pytest.raises(IgdError):
        igd_amd.rank_host(sup, -1.0 - pv, odds)
