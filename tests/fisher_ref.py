"""Yardsticks of the Fisher tests (test_fisher_host.py, test_enrich_host.py, test_gpu_fisher.py, test_gpu_enrich.py).

Expected values never come from the code under test: -log10 P(X >= a) is the exact tail sum in Python integers
(math.comb), whose logarithm is taken from a 120-bit quotient; tests/golden/fisher_tables.json holds tables whose exact
value was recorded with mpmath at 60 digits (tools/make_fisher_golden.py).  The "wide" tables of that file (N up to
2^31 - 2, tails of hundreds to thousands of 64-term steps) are beyond math.comb; the tool sums them in mpmath by the exact
ratio of neighbouring terms and holds that method against math.comb on every other table of the file.

    edge_tables()   the number of summed terms pinned at 1, 2, 63, 64, 65, 127, 128, 129, 192 in each direction
    pool_tables()   1 009 distinct small tables of all four branches, cycled by the tests that cross a chunk seam
    chunk_cells()   IGD_FISHER_CHUNK, read out of the source
    check_many()    check() for a million cells: numpy, per-cell bounds taken from the distinct tables"""
import json
import math
import os
import random

import numpy as np

GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fisher_tables.json")


def params(a, b, c, d):
    N, K, n = a + b + c + d, a + b, a + c
    return N, K, n, max(0, n - (N - K)), min(n, K)


def exact_tail(a, b, c, d):
    """(numerator, denominator) of P(X >= a), X ~ Hypergeometric(N, K, n), as integers; the shorter side is summed"""
    N, K, n, lo, hi = params(a, b, c, d)
    den = math.comb(N, n)
    if a - lo <= hi - a:
        return den - sum(math.comb(K, k) * math.comb(N - K, n - k) for k in range(lo, a)), den
    return sum(math.comb(K, k) * math.comb(N - K, n - k) for k in range(a, hi + 1)), den


def plog_of(num, den):
    """-log10(num / den) of two integers, exact to a few 1e-16 relative: the quotient is kept to 120 bits before the logarithm"""
    if num == den:
        return 0.0
    shift = den.bit_length() - num.bit_length() + 120
    q = (num << shift) // den
    return -(math.log2(q) - shift) * math.log10(2.0) if shift > 1000 else -math.log10(q / 2.0 ** shift)


def exact_plog(a, b, c, d):
    """-log10 P(X >= a), exact to a few 1e-16 relative"""
    return plog_of(*exact_tail(a, b, c, d))


def tol(a, b, c, d, y):
    """the issue's bound: nine log-factorials of magnitude <= lgamma(N + 2) at a few ulp each, the final log, a floor"""
    N = a + b + c + d
    return 64 * 2.0 ** -53 * math.lgamma(N + 2) / math.log(10) + 1e-12 * abs(y) + 1e-13


def odds(a, b, c, d):
    """(a d) / (b c) in double; inf when b c = 0 < a d, NaN when both are 0"""
    ad, bc = float(a) * float(d), float(b) * float(c)
    if bc == 0.0:
        return math.inf if ad > 0.0 else math.nan
    return ad / bc


def ulps(x, y):
    if math.isnan(x) or math.isnan(y) or math.isinf(x) or math.isinf(y):
        return 0 if (x == y or (math.isnan(x) and math.isnan(y))) else 1 << 62
    return abs(x - y) / math.ulp(y) if y else abs(x - y) / 5e-324


def golden():
    """[(a, b, c, d, exact pvalue_log, name)]"""
    return [(t["a"], t["b"], t["c"], t["d"], float(t["pvalue_log"]), t["name"]) for t in json.load(open(GOLDEN_JSON))["tables"]]


_cache = {}


def branch(a, b, c, d):
    """which way the scheme takes: "zero" (N == 0), "lo" (a == lo: p = 1 without a term), "up" (a > mode: k = a .. hi is
    summed) or "down" (k = a - 1 .. lo is summed and p = 1 - L)"""
    N, K, n, lo, hi = params(a, b, c, d)
    if N == 0:
        return "zero"
    if a <= lo:
        return "lo"
    return "up" if a > (n + 1) * (K + 1) // (N + 2) else "down"


def summed_terms(a, b, c, d):
    """the number of support points on the side that is summed: hi - a + 1 upward, a - lo downward"""
    N, K, n, lo, hi = params(a, b, c, d)
    return {"zero": 0, "lo": 0, "up": hi - a + 1, "down": a - lo}[branch(a, b, c, d)]


EDGE_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 192)


def edge_tables():
    """[(direction, T, (a, b, c, d))]: the summed side has exactly T terms, T in EDGE_COUNTS, and a lies next to the mode,
    where the first term is a large share of the whole tail -- one term too many or too few moves the value far beyond
    the bound (test_fisher_host.py checks that in exact arithmetic).
    up:    N = 2000, K = 1000, n = 2 T: mode = T, a = T + 1, hi = 2 T.
    down:  N = 1900, K = 950,  n = 1900 - 2 T: lo = 950 - 2 T > 0, mode = a = 950 - T."""
    out = []
    for T in EDGE_COUNTS:
        out.append(("up", T, (T + 1, 1000 - (T + 1), T - 1, 1000 - (T - 1))))
        n, a = 1900 - 2 * T, 950 - T
        out.append(("down", T, (a, 950 - a, n - a, 950 - (n - a))))
    for way, T, t in out:
        assert min(t) >= 0 and sum(t) <= 2000 and branch(*t) == way and summed_terms(*t) == T, (way, T, t)
        assert way == "up" or params(*t)[3] > 0, t
    return out


def one_more_first_term(a, b, c, d):
    """the exact value of a sum that holds the first term of the summed side twice: what a lane past the end of the support
    adds when it is not masked (it computes the term k0)"""
    N, K, n, lo, hi = params(a, b, c, d)
    way = branch(a, b, c, d)
    assert way in ("up", "down")
    k0 = a if way == "up" else a - 1
    first = math.comb(K, k0) * math.comb(N - K, n - k0)
    num, den = exact_tail(a, b, c, d)
    return plog_of(num + first if way == "up" else num - first, den)


def chunk_cells():
    """IGD_FISHER_CHUNK, read out of engine/host_enrich.hpp: the cells of one launch of either form"""
    import re
    src = os.path.join(os.path.dirname(GOLDEN_JSON), "..", "..", "igd_amd", "csrc", "engine", "host_enrich.hpp")
    m = re.search(r"^#define\s+IGD_FISHER_CHUNK\s+\(\(int64_t\)1\s*<<\s*(\d+)\)", open(src).read(), re.M)
    assert m and int(m.group(1)) == 20, "IGD_FISHER_CHUNK is no longer 2^20: the seam fixtures need resizing"
    return 1 << int(m.group(1))


POOL = 1009                 # a prime: coprime to 64 and to the wave count of any grid


def pool_tables(seed=1016, nmax=300):
    """POOL distinct tables with N <= nmax, (0, 0, 0, 0) among them, a drawn over the whole support; neighbours differ.
    (The seed is one for which the cells 2^20 - 1, 2^20 and 2^20 + 76 of the cycle expect three different positive values.)"""
    rng = random.Random(seed)
    out, seen = [(0, 0, 0, 0)], {(0, 0, 0, 0)}
    while len(out) < POOL:
        N = rng.choice([rng.randint(1, 12), rng.randint(1, 80), rng.randint(1, nmax)])
        K, n = rng.randint(0, N), rng.randint(0, N)
        lo, hi = max(0, n - (N - K)), min(n, K)
        mode = (n + 1) * (K + 1) // (N + 2)
        a = rng.choice([lo, min(max(mode, lo), hi), min(mode + 1, hi), rng.randint(lo, hi), rng.randint(lo, hi), rng.randint(lo, hi)])
        t = (a, K - a, n - a, N - K - n + a)
        if t not in seen:
            seen.add(t)
            out.append(t)
    rng.shuffle(out)
    return out


def pool_expected():
    """(tables, exact values): computed once"""
    if "p" not in _cache:
        T = pool_tables()
        _cache["p"] = (T, [exact_plog(*t) for t in T])
    return _cache["p"]


def random_tables(seed=20261018, count=300, nmax=3000):
    """seeded tables with N <= nmax: margins of every size, a drawn over the whole support, boundaries included"""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        N = rng.choice([rng.randint(1, 40), rng.randint(1, 400), rng.randint(1, nmax)])
        K, n = rng.randint(0, N), rng.randint(0, N)
        lo, hi = max(0, n - (N - K)), min(n, K)
        mode = (n + 1) * (K + 1) // (N + 2)
        a = rng.choice([lo, hi, min(max(mode, lo), hi), min(mode + 1, hi), rng.randint(lo, hi), rng.randint(lo, hi)])
        out.append((a, K - a, n - a, N - K - n + a))
    return out


def random_expected():
    if "r" not in _cache:
        _cache["r"] = [exact_plog(*t) for t in random_tables()]
    return _cache["r"]


def check(tables, want, got_p, got_o, what, scale=1.0, extra=0.0):
    """every table within scale * tol + extra of the exact value, >= 0, and odds ratios within 4 ulp (inf / NaN exact)"""
    worst = 0.0
    for t, y, p, o in zip(tables, want, got_p, got_o):
        bound = scale * tol(*t, y) + extra
        assert p >= 0.0 and not math.isnan(p) and math.isfinite(p), (what, t, p)
        assert abs(p - y) <= bound, (what, t, p, y, abs(p - y), bound)
        worst = max(worst, abs(p - y) / bound)
        if o is not None:
            assert ulps(float(o), odds(*t)) <= 4, (what, t, o, odds(*t))
        N, K, n, lo, hi = params(*t)
        if N == 0 or t[0] == lo:
            assert p == 0.0 and not np.signbit(p), (what, t, p)
    return worst


def check_many(tables, want, idx, got_p, got_o, what, scale=1.0):
    """check() over the cells i whose table is tables[idx[i]]: the same conditions, in numpy.  Returns the worst ratio."""
    got_p = np.asarray(got_p)
    assert got_p.shape == idx.shape
    y = np.array(want)[idx]
    bound = np.array([scale * tol(*t, w) for t, w in zip(tables, want)])[idx]
    assert np.isfinite(got_p).all() and (got_p >= 0.0).all(), what
    err = np.abs(got_p - y)
    bad = np.flatnonzero(~(err <= bound))
    assert len(bad) == 0, (what, len(bad), [(int(i), tables[idx[i]], float(got_p[i]), float(y[i])) for i in bad[:5]])
    one = np.array([branch(*t) in ("zero", "lo") for t in tables])[idx]
    assert not got_p[one].any() and not np.signbit(got_p[one]).any(), what                  # +0.0 exactly
    if got_o is not None:
        got_o = np.asarray(got_o)
        o = np.array([odds(*t) for t in tables])[idx]
        assert np.array_equal(np.isnan(got_o), np.isnan(o)) and np.array_equal(np.isinf(got_o), np.isinf(o)), what
        fin = np.isfinite(o)
        assert (got_o[~fin & ~np.isnan(o)] > 0).all(), what
        with np.errstate(invalid="ignore"):
            ok = np.abs(got_o[fin] - o[fin]) <= 4 * np.spacing(np.abs(o[fin]))
        assert ok.all(), (what, "odds ratio")
    return float((err / bound).max(initial=0.0))
