"""Fisher's exact test on the host: igd_amd.fisher_host over igdc_fisher_host (igd_hostpath.c), no GPU.

    pvalue_log = -log10 P(X >= a),  X ~ Hypergeometric(a+b+c+d, a+b, a+c)          odds_ratio = (a d) / (b c)

Expected values are exact arithmetic (fisher_ref.py): recorded for the golden tables, computed here for the random ones.
The bound is the issue's, derived from the rounding of nine log-factorials:
    |x - y| <= 64 * 2^-53 * lgamma(N + 2) / ln 10 + 1e-12 * |y| + 1e-13
Odds ratios: 4 ulp, inf and NaN exactly."""
import math

import numpy as np
import pytest

import fisher_ref as R


def host(tables):
    import igd_amd
    a, b, c, d = (np.array(x, np.int64) for x in zip(*tables))
    return igd_amd.fisher_host(a, b, c, d)


def test_golden_tables():
    G = R.golden()
    names = [g[5] for g in G]
    assert len(G) >= 40 and {"edge", "min", "max", "mode", "mode+1", "deep", "large", "flat"} <= set(names)
    tables = [g[:4] for g in G]
    assert (2000, 1000, 1000, 996000) in tables and (30, 999970, 20, 2 * 10 ** 9) in tables
    assert any(sum(t) == 2 ** 31 - 2 for t in tables)
    p, o = host(tables)
    worst = R.check(tables, [g[4] for g in G], p, o, "golden")
    print("golden: worst |x - y| / bound = %.3g" % worst)
    deep = p[tables.index((2000, 1000, 1000, 996000))]
    assert abs(deep - 4609.0606) < 1e-3                       # where a double p underflows: computed in log space
    # the edge tables by hand
    e = dict(zip(tables, zip(p, o)))
    assert e[(0, 0, 0, 0)][0] == 0.0 and math.isnan(e[(0, 0, 0, 0)][1])
    assert e[(1, 0, 0, 0)][0] == 0.0 and math.isnan(e[(1, 0, 0, 0)][1])
    assert e[(0, 5, 5, 5)] == (0.0, 0.0)
    assert e[(5, 0, 0, 5)][1] == math.inf and abs(e[(5, 0, 0, 5)][0] - math.log10(252)) < 1e-13
    assert e[(3, 0, 7, 0)][0] == 0.0 and math.isnan(e[(3, 0, 7, 0)][1])
    assert e[(1, 1, 1, 1)][1] == 1.0 and abs(e[(1, 1, 1, 1)][0] + math.log10(5 / 6)) < 1e-13


def test_random_tables_against_the_exact_sum():
    tables = R.random_tables()
    want = R.random_expected()
    assert len(tables) == 300 and max(sum(t) for t in tables) <= 3000
    assert sum(1 for y in want if y == 0.0) >= 20 and sum(1 for y in want if y > 10) >= 20     # both ends of the range
    p, o = host(tables)
    print("random: worst |x - y| / bound = %.3g" % R.check(tables, want, p, o, "random"))


def test_flat_case_runs_past_256_terms():
    """K = N/2, n = 3000: the terms fall slowly, the tail has more than 256 terms above e^-45 of the first -- a stop that
    fired after one or two steps of 64 would miss the bound more than ten times over"""
    G = [g for g in R.golden() if g[5] == "flat"]
    assert len(G) == 2
    for a, b, c, d, y, _ in G:
        N, K, n, lo, hi = R.params(a, b, c, d)
        assert K * 2 == N and n == 3000
        k0 = a if a > (n + 1) * (K + 1) // (N + 2) else a - 1
        step = 1 if k0 == a else -1
        lt = lambda k: (math.lgamma(K + 1) - math.lgamma(k + 1) - math.lgamma(K - k + 1) + math.lgamma(N - K + 1)
                        - math.lgamma(n - k + 1) - math.lgamma(N - K - n + k + 1))
        assert lt(k0 + 256 * step) > lt(k0) - 45               # term 256 is still above the stop
        cut = sum(math.exp(lt(k0 + j * step) - lt(k0)) for j in range(128))
        full = sum(math.exp(lt(k0 + j * step) - lt(k0)) for j in range(400))
        assert abs(math.log10(cut / full)) > 10 * R.tol(a, b, c, d, y)       # an early stop would be seen
    tables = [g[:4] for g in G]
    p, o = host(tables)
    R.check(tables, [g[4] for g in G], p, o, "flat")


def test_bad_tables_are_refused_and_outputs_untouched():
    import igd_amd
    from igd_amd import _native as N
    from igd_amd.database import IgdError
    for bad in [(-1, 2, 3, 4), (1, 2, 3, -4), (2 ** 31 - 3, 1, 1, 1), (2 ** 31, 0, 0, 0), (2 ** 62, 2 ** 62, 0, 0)]:
        tabs = [(1, 2, 3, 4), bad]
        with pytest.raises(IgdError):
            host(tabs)
        a, b, c, d = (np.array(x, np.int64) for x in zip(*tabs))
        p, o = np.full(2, 7.5), np.full(2, -3.25)
        assert N.cli().igdc_fisher_host(a.ctypes.data, b.ctypes.data, c.ctypes.data, d.ctypes.data, 2, p.ctypes.data, o.ctypes.data) == -1
        assert (p == 7.5).all() and (o == -3.25).all()
    p, o = igd_amd.fisher_host([2 ** 31 - 4], [1], [1], [1])             # N = 2^31 - 1 is the largest accepted
    assert p[0] >= 0 and o[0] == float(2 ** 31 - 4)
    p, o = igd_amd.fisher_host([], [], [], [])
    assert len(p) == 0 and len(o) == 0
    # odds_ratio may be NULL
    a = np.array([5], np.int64)
    z = np.array([0], np.int64)
    p = np.zeros(1)
    assert N.cli().igdc_fisher_host(a.ctypes.data, z.ctypes.data, z.ctypes.data, a.ctypes.data, 1, p.ctypes.data, None) == 0
    assert abs(p[0] - math.log10(252)) < 1e-13


def wide_golden():
    G = [g for g in R.golden() if g[5] == "wide"]
    assert len(G) == 20
    margins = {(sum(g[:4]), g[0] + g[1], g[0] + g[2]) for g in G}
    assert margins == {(2 ** 31 - 2, 2 ** 30, 2 ** 30), (2 ** 31 - 2, 2 ** 30, 10 ** 6), (10 ** 8, 5 * 10 ** 7, 10 ** 7),
                       (4 * 10 ** 6, 2 * 10 ** 6, 2 * 10 ** 6)}
    ways = [R.branch(*g[:4]) for g in G]
    assert ways.count("down") == 8 and ways.count("up") == 12      # a = mode and mode - 3 sd are summed downward
    return G


def test_wide_tables_run_for_hundreds_of_steps():
    """N up to 2^31 - 2 with a standard deviation of up to 16 384: the tail is summed over 27 to about 1 700 steps of 64
    terms, with lgamma arguments near 2^30, where 1e-6 is one ulp of a log-factorial.  The recorded values come from mpmath
    (tools/make_fisher_golden.py); the bound is the same as everywhere."""
    G = wide_golden()
    tables = [g[:4] for g in G]
    p, o = host(tables)
    worst = R.check(tables, [g[4] for g in G], p, o, "wide")
    print("wide: worst |x - y| / bound = %.3g" % worst)
    assert max(g[4] for g in G) > 30 and min(g[4] for g in G) < 1e-3     # 12 sd above the mode, 3 sd below it


def test_support_end_edges():
    """The number of summed terms at 1, 2, 63, 64, 65, 127, 128, 129 and 192 in both directions (fisher_ref.edge_tables).
    The fixture's condition, in exact arithmetic: wherever the last step of 64 is not full, one more copy of the first
    term -- what an unmasked lane past the end would add -- moves the exact value by more than ten times the bound."""
    E = R.edge_tables()
    assert sorted((w, T) for w, T, _ in E) == sorted((w, T) for w in ("up", "down") for T in R.EDGE_COUNTS)
    tables = [t for _, _, t in E]
    want = [R.exact_plog(*t) for t in tables]
    for (way, T, t), y in zip(E, want):
        assert sum(t) <= 2000
        if T % 64:
            moved = abs(R.one_more_first_term(*t) - y)
            assert moved > 10 * R.tol(*t, y), (way, T, t, moved)
    p, o = host(tables)
    print("edges: worst |x - y| / bound = %.3g" % R.check(tables, want, p, o, "edges"))


def test_pool_tables_cover_the_four_branches():
    T, want = R.pool_expected()
    assert len(T) == len(set(T)) == R.POOL == 1009 and max(sum(t) for t in T) <= 300
    ways = [R.branch(*t) for t in T]
    assert ways.count("zero") == 1 and min(ways.count(w) for w in ("lo", "up", "down")) >= 100
    assert all(T[i] != T[i + 1] for i in range(len(T) - 1))
    idx = np.arange(3 * R.POOL + 5) % R.POOL
    a, b, c, d = (np.array(x, np.int64)[idx] for x in zip(*T))
    import igd_amd
    p, o = igd_amd.fisher_host(a, b, c, d)
    print("pool: worst |x - y| / bound = %.3g" % R.check_many(T, want, idx, p, o, "pool"))
    bad = p.copy()
    bad[R.POOL + 1] += 1e-9                                      # the vectorised check sees one wrong cell
    with pytest.raises(AssertionError):
        R.check_many(T, want, idx, bad, o, "pool")
