"""Yardsticks of the Fisher tests (test_fisher_host.py, test_enrich_host.py, test_gpu_fisher.py, test_gpu_enrich.py).

Expected values never come from the code under test: -log10 P(X >= a) is the exact tail sum in Python integers
(math.comb), whose logarithm is taken from a 120-bit quotient; tests/golden/fisher_tables.json holds tables whose exact
value was recorded with mpmath at 60 digits (tools/make_fisher_golden.py)."""
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


def exact_plog(a, b, c, d):
    """-log10 P(X >= a), exact to a few 1e-16 relative: the quotient is kept to 120 bits before the logarithm"""
    num, den = exact_tail(a, b, c, d)
    if num == den:
        return 0.0
    shift = den.bit_length() - num.bit_length() + 120
    q = (num << shift) // den
    return -(math.log2(q) - shift) * math.log10(2.0) if shift > 1000 else -math.log10(q / 2.0 ** shift)


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


_cache = {}


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
