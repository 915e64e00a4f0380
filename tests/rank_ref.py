"""Reference for the rank columns and Benjamini-Hochberg q-values of an enrichment table (igd_hip_enrich_ranks,
igdc_rank_host), written from the definitions and never calling the code under test.

Per row (the m cells of one query set):
    rank[f] = 1 + #{g : x[g] > x[f]}            ties take the minimum rank; for the odds ratio +inf is the largest value, NaN
                                                 ranks below every number and all NaN tie
    r[f]    = #{g : p[g] >= p[f]}                p = pvalue_log
    adj[f]  = p[f] + (log10 r[f] - log10 m)
    q[f]    = max(+0.0, max{adj[g] : p[g] <= p[f]})

Ranks come two ways -- literally, O(m^2), and by np.sort + searchsorted -- which must agree on small rows; q comes in Python
floats with math.log10, and on small rows also from mpmath as -log10 min(1, min over j >= i of m p_(j) / j) with p = 10^-p_log
at 60 digits.

Bounds: ranks and max_rnk exact; mean_rnk within 1 ulp; q within tol(y) = 1e-12 (1 + |y|): the value is one correctly
rounded log10 difference of magnitude <= ~6 added to pvalue_log and then an exact maximum, a few units of 2^-53 relative,
and the bound leaves two orders over that.  Exactly: q >= +0.0 with the sign bit clear; q <= p + tol; equal p in a row give
bit-equal q; p[f] >= p[g] implies q[f] >= q[g]."""
import collections
import math

import numpy as np

Ranks = collections.namedtuple("Ranks", "qvalue_log rnk_sup rnk_pv rnk_or max_rnk mean_rnk")
SMALL = 300            # rows up to this width are also ranked literally
LDS_COLS = 8192        # the engine's values (igd_hip_rank_lds_cols(), igd_hip_rank_grid(10**9)) for tests that cannot ask it
GRID = 2048
_cache = {}


def tol(y):
    return 1e-12 * (1.0 + np.abs(y))


# ---- ranks ---------------------------------------------------------------------------------------------------------------
def ranks_literal(x, nan_low=False):
    """1 + #{g : x[g] > x[f]} by the double loop (numpy does the inner one)"""
    x = np.asarray(x)
    if nan_low:
        nan = np.isnan(x)
        with np.errstate(invalid="ignore"):
            gt = (~nan)[None, :] & (nan[:, None] | (x[None, :] > x[:, None]))       # gt[f, g]: x[g] above x[f]
    else:
        gt = x[None, :] > x[:, None]
    return (1 + gt.sum(axis=1)).astype(np.int32)


def ranks_sorted(x, nan_low=False):
    x = np.asarray(x)
    nan = np.isnan(x) if nan_low else np.zeros(len(x), bool)
    s = np.sort(x[~nan])
    out = np.empty(len(x), np.int32)
    out[~nan] = 1 + len(s) - np.searchsorted(s, x[~nan], side="right")
    out[nan] = 1 + len(s)
    return out


def ranks(x, nan_low=False):
    r = ranks_sorted(x, nan_low)
    if len(x) <= SMALL:
        np.testing.assert_array_equal(r, ranks_literal(x, nan_low))
    return r


# ---- q-values ------------------------------------------------------------------------------------------------------------
def q_row(p):
    """q of one row in Python floats: one adj per distinct value, a running maximum from the small end"""
    p = [float(v) for v in p]
    m = len(p)
    sp = sorted(p)
    lm = math.log10(m)
    logr = {}
    best = -math.inf
    q = {}
    i = 0
    while i < m:                                       # distinct values, ascending; r = cells at or above the value = m - i
        v = sp[i]
        r = m - i
        if r not in logr:
            logr[r] = math.log10(r)
        adj = v + (logr[r] - lm)
        if adj > best:
            best = adj
        q[v] = best if best > 0.0 else 0.0
        while i < m and sp[i] == v:
            i += 1
    return np.array([q[v] for v in p], np.float64)


def q_row_literal(p):
    """the definition, cell by cell (small rows)"""
    p = [float(v) for v in p]
    m = len(p)
    adj = [p[f] + (math.log10(sum(1 for g in range(m) if p[g] >= p[f])) - math.log10(m)) for f in range(m)]
    return np.array([max(0.0, max(adj[g] for g in range(m) if p[g] <= p[f])) for f in range(m)], np.float64)


def q_row_mpmath(p):
    """-log10 of the Benjamini-Hochberg adjusted p, min(1, min over j >= i of m p_(j) / j), from p = 10^-p_log at 60 digits"""
    import mpmath as mp
    with mp.workdps(60):
        m = len(p)
        order = sorted(range(m), key=lambda f: -float(p[f]))            # ascending p = descending p_log
        pp = [mp.power(10, -mp.mpf(float(p[f]))) for f in order]
        out = [None] * m
        run = mp.mpf(1)
        for j in range(m, 0, -1):
            run = min(run, m * pp[j - 1] / j)
            out[order[j - 1]] = float(-mp.log10(run))
        return np.array([v if v > 0 else 0.0 for v in out], np.float64)


def reference(sup, pv, odds):
    """Ranks of three [nrows, m] arrays, by the definitions"""
    sup, pv, odds = np.asarray(sup, np.int64), np.asarray(pv, np.float64), np.asarray(odds, np.float64)
    nrows, m = sup.shape
    out = Ranks(np.empty((nrows, m)), *(np.empty((nrows, m), np.int32) for _ in range(4)), np.empty((nrows, m)))
    for k in range(nrows):
        out.rnk_sup[k] = ranks(sup[k])
        out.rnk_pv[k] = ranks(pv[k])
        out.rnk_or[k] = ranks(odds[k], nan_low=True)
        out.qvalue_log[k] = q_row(pv[k])
        if m <= SMALL and k < 4:
            lit = q_row_literal(pv[k])
            assert (lit.view(np.int64) == out.qvalue_log[k].view(np.int64)).all()
            mpq = q_row_mpmath(pv[k])
            assert (np.abs(mpq - out.qvalue_log[k]) <= 0.01 * tol(mpq)).all(), (pv[k], mpq, out.qvalue_log[k])
    out.max_rnk[:] = np.maximum(np.maximum(out.rnk_sup, out.rnk_pv), out.rnk_or)
    # the exact mean: the integer sum is exact, one correctly rounded division
    out.mean_rnk[:] = (out.rnk_sup.astype(np.int64) + out.rnk_pv + out.rnk_or) / 3.0
    return out


def check(sup, pv, odds, got, want, what, scale=1.0, only=None):
    """got (Ranks; fields not asked for may be None) against want within the bounds, and the exact properties of q"""
    pv = np.asarray(pv, np.float64)
    for name in ("rnk_sup", "rnk_pv", "rnk_or", "max_rnk"):
        g = getattr(got, name)
        if g is not None and (only is None or name in only):
            np.testing.assert_array_equal(g, getattr(want, name), err_msg="%s: %s" % (what, name))
    if got.mean_rnk is not None and (only is None or "mean_rnk" in only):
        err = np.abs(got.mean_rnk - want.mean_rnk)
        assert (err <= np.spacing(want.mean_rnk)).all(), (what, "mean_rnk", err.max())
    q = got.qvalue_log
    if q is not None and (only is None or "qvalue_log" in only):
        err = np.abs(q - want.qvalue_log)
        bound = scale * tol(want.qvalue_log)
        assert (err <= bound).all(), (what, "qvalue_log", float((err / bound).max()))
        assert (q >= 0.0).all() and not np.signbit(q).any(), (what, "q below +0.0")
        assert (q <= pv + tol(pv)).all(), (what, "q above p")
        order = np.argsort(pv, axis=1, kind="stable")
        ps, qs = np.take_along_axis(pv, order, 1), np.take_along_axis(q, order, 1)
        same = ps[:, 1:] == ps[:, :-1]
        assert (qs.view(np.int64)[:, 1:][same] == qs.view(np.int64)[:, :-1][same]).all(), (what, "equal p, different q")
        assert (qs[:, 1:] >= qs[:, :-1]).all(), (what, "q not monotone in p")


# ---- the rows of the tests -----------------------------------------------------------------------------------------------
def random_table(seed, nrows, m):
    """ties in every column, zeros and huge values among pvalue_log, inf / NaN / 0 among the odds ratios"""
    rng = np.random.default_rng(seed)
    sup = rng.integers(0, max(3, m // 2), (nrows, m)).astype(np.int64)
    kind = rng.random((nrows, m))
    pv = np.where(kind < 0.1, 0.0, np.where(kind < 0.5, np.round(rng.exponential(3.0, (nrows, m)), 1), rng.exponential(50.0, (nrows, m))))
    kind = rng.random((nrows, m))
    odds = np.where(kind < 0.05, np.inf, np.where(kind < 0.1, np.nan, np.where(kind < 0.2, 0.0, np.where(
        kind < 0.5, np.round(rng.exponential(2.0, (nrows, m)), 1), np.exp(rng.normal(0.0, 2.0, (nrows, m)))))))
    return sup, pv, odds


WIDTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def widths_case(m):
    return random_table(1000 + m, 7, m)


def seam_widths(L):
    return (L - 1, L, L + 1, 2 * L + 3)


def seam_case(m):
    return random_table(2000 + m, 3, m)


def seam_padded_case(L):
    """one table of L columns, and the same with an (L+1)-th column of lowest keys: the first L columns' ranks are equal"""
    sup, pv, odds = random_table(2500, 2, L)
    lo = (np.zeros((2, 1), np.int64), np.zeros((2, 1)), np.full((2, 1), np.nan))
    return (sup, pv, odds), tuple(np.ascontiguousarray(np.concatenate([a, b], axis=1)) for a, b in zip((sup, pv, odds), lo))


def second_rows_case(grid, m):
    t = random_table(3000 + m, grid + 5, m)
    assert all((a[grid:] != a[:5]).any() for a in t[:2])             # the last rows differ from the first
    return t


def two_launches_case():
    t = random_table(4000, 505, 2081)
    assert 505 * 2081 > 1 << 20 and (1 << 20) % 2081 != 0
    return t


def ties_cases():
    out = {}
    m = 300
    out["all_equal"] = (np.full((2, m), 7, np.int64), np.full((2, m), 3.25), np.full((2, m), 1.5))
    rows = []
    for k in range(4):                                 # tie runs of 2, 64, 65 and 300 among 100 singles, in shuffled columns
        rng = np.random.default_rng(5000 + k)
        vals = rng.permutation(104)
        col = np.concatenate([np.repeat(vals[:4], (2, 64, 65, 300)), vals[4:]])
        assert len(col) == 531
        rows.append(col[rng.permutation(len(col))])
    c = np.array(rows)
    out["runs"] = (c.astype(np.int64), c * 0.75, np.where(c % 7 == 0, np.inf, c / 8.0))
    m = 70                                             # the lowest value ten times, with the padding's key (p = +0.0, NaN), beside the padding
    rng = np.random.default_rng(5100)
    c = np.concatenate([np.zeros(10), 1 + rng.permutation(60)])[rng.permutation(70)][None, :]
    out["beside_padding"] = (c.astype(np.int64), c * 1.5, np.where(c == 0, np.nan, c))
    out["all_zero_p"] = (np.arange(65, dtype=np.int64)[None, :], np.zeros((1, 65)), np.ones((1, 65)))
    return out


def odds_cases():
    nan, inf = np.nan, np.inf
    rows = [[nan] * 9,
            [3.5, inf, nan, 0.0, 1e-300, 0.25, nan, 0.0, 7.0],
            [inf, 2.0, inf, inf, 0.0, nan, 1.0, inf, 2.0]]
    odds = np.array(rows)
    wide = np.resize(np.array(rows[1] + rows[2]), (1, 130))
    sup9 = np.arange(27, dtype=np.int64).reshape(3, 9) % 5
    return {"odds9": (sup9, np.abs(sup9 - 2.0), odds),
            "odds130": (np.arange(130, dtype=np.int64)[None, :] % 9, (np.arange(130.0) % 11)[None, :], wide)}


def keys64_case():
    vals = [0, 1, 2**31 - 2, 2**32 + 1, 2**40]
    sup = np.array([vals, vals[::-1], [vals[i] for i in (3, 0, 4, 2, 1)]], np.int64)
    return sup, np.ones(sup.shape), np.ones(sup.shape)


def bh_cases():
    """suffix: p = .01, .04, .03 -- the cell with p = .03 has m p / j = .045 and takes .04 from the less significant one.
    clamp: every adj but the last cell's is negative; the last cell's is its own p (r = m: the logarithms cancel exactly)
    and lies in every cell's maximum, so q = the smallest p everywhere -- min(1, .) of the adjusted p is reached, q never
    goes below the row's smallest p.  The second row holds a p of -0.0, whose q must come out as +0.0.
    huge: 4609.06 beside 1e-9."""
    lg = lambda x: -math.log10(x)
    suffix = np.array([[lg(0.01), lg(0.04), lg(0.03)]])
    clamp = np.array([[0.1, 0.05, 0.02], [0.3, -0.0, 0.1]])
    huge = np.array([[4609.06, 1e-9], [1e-9, 4609.06]])
    huge7 = np.array([[4609.06, 1e-9, 3.0, 4609.06, 0.0, 1e-9, 250.5]])
    one = lambda p: (np.arange(p.size, dtype=np.int64).reshape(p.shape), p, np.ones(p.shape))
    want = reference(*one(suffix))
    assert want.qvalue_log[0, 2] == want.qvalue_log[0, 1] > suffix[0, 2] + (math.log10(2) - math.log10(3))
    return {"suffix": one(suffix), "clamp": one(clamp), "huge": one(huge), "huge7": one(huge7)}


def all_cases(L=LDS_COLS, grid=GRID, wide=True):
    """name -> (support, pvalue_log, odds_ratio): every row the GPU tests name"""
    out = {}
    for m in WIDTHS:
        out["width%d" % m] = widths_case(m)
    if wide:
        for m in seam_widths(L):
            out["seam%d" % m] = seam_case(m)
        out["two_launches"] = two_launches_case()
    for m in (5, 70):
        out["second_rows%d" % m] = second_rows_case(grid, m)
    out.update(ties_cases())
    out.update(odds_cases())
    out["keys64"] = keys64_case()
    out.update(bh_cases())
    return out


def want_of(name, table):
    """the reference of a named case, computed once per session"""
    if name not in _cache:
        _cache[name] = reference(*table)
    return _cache[name]
