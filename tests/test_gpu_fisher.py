"""GPU: Fisher's exact test of 2x2 tables (igd_hip_fisher_tables / igd_fisher_cells, Database.fisher).

Expected values are exact arithmetic (fisher_ref.py), never the code under test; the bound is the issue's
    |x - y| <= 64 * 2^-53 * lgamma(N + 2) / ln 10 + 1e-12 * |y| + 1e-13
odds ratios within 4 ulp with inf and NaN exact, and the GPU within twice the bound of igd_amd.fisher_host."""
import math
import os
import random
import shutil

import numpy as np
import pytest

import fisher_ref as R
from helpers import short_tmpdir, write_igd_numpy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def db():
    """any database will do: the tables do not come from it"""
    from igd_amd import Database
    d = short_tmpdir("igf")
    path = os.path.join(d, "t.igd")
    write_igd_numpy(path, [[("chr1", 10, 500, 1)], [("chr1", 400, 900, 2)]], nbp=1 << 12)
    h = Database(path)
    yield h
    h.close()
    shutil.rmtree(d, ignore_errors=True)


def both(db, tables, what, want):
    import igd_amd
    a, b, c, d = (np.array(x, np.int64) for x in zip(*tables))
    n = len(tables)
    p, o = db.fisher(a, b, c, d, pvalue_log=np.full(n, -7.0), odds_ratio=np.full(n, -7.0))       # outputs are DEFINED
    worst = R.check(tables, want, p, o, what)
    hp, ho = igd_amd.fisher_host(a, b, c, d)
    for t, y, x, z in zip(tables, want, p, hp):
        assert abs(x - z) <= 2 * R.tol(*t, y), (what, t, x, z)
    assert np.array_equal(np.isnan(o), np.isnan(ho)) and np.array_equal(np.isinf(o), np.isinf(ho))
    print("%s: worst |x - y| / bound = %.3g" % (what, worst))
    return p, o


def test_golden_tables(db):
    G = R.golden()
    tables = [g[:4] for g in G]
    p, _ = both(db, tables, "golden", [g[4] for g in G])
    assert abs(p[tables.index((2000, 1000, 1000, 996000))] - 4609.0606) < 1e-3


def test_random_tables_and_the_flat_case(db):
    flat = [g for g in R.golden() if g[5] == "flat"]          # several 64-term steps in one wave: the stop must not fire early
    assert len(flat) == 2
    tables = R.random_tables() + [g[:4] for g in flat]
    both(db, tables, "random + flat", R.random_expected() + [g[4] for g in flat])


def test_waves_take_a_second_cell_and_the_last_workgroup_is_partly_empty(db):
    from igd_amd import _native as N
    H = N.hip()
    grid = lambda n: int(H.igd_hip_fisher_grid(n))
    assert grid(0) == 1 and grid(1) == 1 and grid(4) == 1 and grid(5) == 2
    big = grid(10 ** 9)                                        # the persistent grid: more cells do not widen it
    assert grid(4 * big) == big and grid(4 * big + 5) == big
    n = 4 * big + 5                                            # every wave one cell, five waves a second one
    rng = random.Random(77)
    base = [(3, 10, 10, 50), (10, 5, 3, 20), (0, 5, 5, 5), (5, 0, 0, 5), (1, 1, 1, 1), (12, 30, 25, 200), (7, 0, 3, 0), (0, 0, 0, 0)]
    tables = []
    for i in range(n):                                         # copies with variation: neighbours differ, the values stay small
        a, b, c, d = base[i % len(base)]
        tables.append((a + i % 3, b + (i // 3) % 4, c + (i // 12) % 5, d + rng.randint(0, 40)))
    memo = {}
    want = [memo[t] if t in memo else memo.setdefault(t, R.exact_plog(*t)) for t in tables]
    p, o = both(db, tables, "batch of %d" % n, want)
    # the cells a wave takes second (index >= 4 * grid) and the last ones carry their own values
    for i in list(range(4 * big, n)) + [0, 1, 4 * big - 1]:
        assert abs(p[i] - want[i]) <= R.tol(*tables[i], want[i])


def test_no_cell_and_one_cell(db):
    p, o = db.fisher([], [], [], [])
    assert len(p) == 0 and len(o) == 0
    p, o = db.fisher([5], [0], [0], [5])
    assert abs(p[0] - math.log10(252)) < 1e-13 and o[0] == math.inf
    from igd_amd import _native as N
    a = np.array([10], np.int64); b = np.array([5], np.int64); c = np.array([3], np.int64); d = np.array([20], np.int64)
    p = np.full(1, -1.0)                                       # odds_ratio may be NULL
    assert N.hip().igd_hip_fisher_tables(db.dev, a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, 1, p.ctypes.data, None) == 0
    assert abs(p[0] - R.exact_plog(10, 5, 3, 20)) <= R.tol(10, 5, 3, 20, p[0])


def test_bad_tables_raise_and_leave_the_outputs_untouched(db):
    from igd_amd.database import IgdError
    for bad in [(-1, 2, 3, 4), (4, 3, -2, 1), (2 ** 31 - 3, 1, 1, 1), (0, 2 ** 31, 0, 0), (2 ** 62, 2 ** 62, 0, 0)]:
        a, b, c, d = (np.array(x, np.int64) for x in zip((1, 2, 3, 4), bad, (5, 6, 7, 8)))
        p, o = np.full(3, 7.5), np.full(3, -3.25)
        with pytest.raises(IgdError):
            db.fisher(a, b, c, d, pvalue_log=p, odds_ratio=o)
        assert (p == 7.5).all() and (o == -3.25).all()
    p, o = db.fisher([2 ** 31 - 4], [1], [1], [1])             # N = 2^31 - 1 is the largest accepted
    assert p[0] >= 0 and o[0] == float(2 ** 31 - 4)


def test_wide_tables_run_for_hundreds_of_steps(db):
    """tails of 27 to about 1 700 steps of 64 terms in one wave each, lgamma arguments near 2^30 (test_fisher_host.py)"""
    import time
    from test_fisher_host import wide_golden
    G = wide_golden()
    t0 = time.perf_counter()
    both(db, [g[:4] for g in G], "wide", [g[4] for g in G])
    print("wide: %.3f s for the device and the host call together" % (time.perf_counter() - t0))


def test_support_end_edges(db):
    """1, 2, 63, 64, 65, 127, 128, 129 and 192 summed terms in both directions: the lanes past the end of the support
    compute a term and must not add it (test_fisher_host.py holds the fixture's condition in exact arithmetic)"""
    E = R.edge_tables()
    tables = [t for _, _, t in E]
    both(db, tables, "edges", [R.exact_plog(*t) for t in tables])


def test_generic_form_across_the_chunk_seam(db):
    """2^20 + 77 cells: two launches, the second with cell0 = 2^20, 77 cells and a grid of 20 workgroups, its inputs taken
    from a + 2^20 .. and its results copied to pvalue_log + 2^20 / odds_ratio + 2^20.  The tables cycle fisher_ref's pool
    of 1 009 distinct ones (all four branches), so what belongs at 2^20 + j differs from what belongs at j."""
    import time
    import igd_amd
    from igd_amd import _native as N
    chunk = R.chunk_cells()
    T, want = R.pool_expected()
    n = chunk + 77
    grid = int(N.hip().igd_hip_fisher_grid(chunk))
    assert R.POOL % 2 == 1 and math.gcd(R.POOL, 4 * grid) == 1 and 4 * grid < chunk
    idx = np.arange(n) % R.POOL
    a, b, c, d = (np.ascontiguousarray(np.array(x, np.int64)[idx]) for x in zip(*T))
    y = np.array(want)[idx]
    ways = np.array([R.branch(*t) for t in T])[idx]
    # the two sides of the seam hold different values, and no cell behind it expects what the cell 2^20 before it does
    assert y[chunk - 1] != y[chunk] and y[chunk] != y[0] and y[n - 1] != y[76] and y[chunk - 1] > 0 and y[chunk] > 0 and y[n - 1] > 0
    assert (y[chunk:] != y[:77]).sum() >= 60 and {"lo", "up", "down"} <= set(ways[chunk:])
    t0 = time.perf_counter()
    p, o = db.fisher(a, b, c, d, pvalue_log=np.full(n, -7.0), odds_ratio=np.full(n, -7.0))
    t1 = time.perf_counter()
    worst = R.check_many(T, want, idx, p, o, "seam")
    for i in (0, chunk - 1, chunk, n - 1):
        t = T[idx[i]]
        assert abs(p[i] - want[idx[i]]) <= R.tol(*t, want[idx[i]]) and R.ulps(float(o[i]), R.odds(*t)) <= 4, (i, t, p[i], o[i])
    hp, ho = igd_amd.fisher_host(a, b, c, d)
    t2 = time.perf_counter()
    bound2 = np.array([2 * R.tol(*t, w) for t, w in zip(T, want)])[idx]
    assert (np.abs(p - hp) <= bound2).all()
    assert np.array_equal(np.isnan(o), np.isnan(ho)) and np.array_equal(np.isinf(o), np.isinf(ho))
    print("seam: %d cells, worst |x - y| / bound = %.3g; GPU call %.3f s, host call %.3f s" % (n, worst, t1 - t0, t2 - t1))
