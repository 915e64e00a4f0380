#!/usr/bin/env python3
"""Writes tests/golden/fisher_tables.json: 2x2 tables with their exact -log10 P(X >= a), X ~ Hypergeometric(a+b+c+d, a+b,
a+c) -- the one-sided Fisher test of igd_hip_fisher_tables / igdc_fisher_host.  The tail is summed in Python integers
(math.comb) and its logarithm taken with mpmath at 60 digits; no GPU and nothing of the project is used.

The "wide" tables (N up to 2^31 - 2, tails of thousands of terms) are out of math.comb's reach.  wide_plog() sums them in
mpmath at 60 digits: the first term from loggamma, every following one from the exact ratio of neighbouring terms, until a
term is below 10^-45 of the first or the support ends.  main() holds wide_plog() against the math.comb method on every
other table of the file (1e-14 relative) before it writes anything.

    python tools/make_fisher_golden.py
"""
import json
import math
import os

from mpmath import exp, log10, loggamma, mp, mpf

mp.dps = 60
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_plog(a, b, c, d):
    N, K, n = a + b + c + d, a + b, a + c
    lo, hi = max(0, n - (N - K)), min(n, K)
    den = math.comb(N, n)
    if a - lo <= hi - a:
        num = den - sum(math.comb(K, k) * math.comb(N - K, n - k) for k in range(lo, a))
    else:
        num = sum(math.comb(K, k) * math.comb(N - K, n - k) for k in range(a, hi + 1))
    if num == den:
        return 0.0
    return float(-log10(mpf(num) / mpf(den)))


def wide_plog(a, b, c, d):
    """the same value without math.comb: the side of the mode on which the terms decay is summed by the ratio recurrence
    t(k+1) / t(k) = (K-k)(n-k) / ((k+1)(N-K-n+k+1)) upward, its inverse downward"""
    N, K, n = a + b + c + d, a + b, a + c
    lo, hi = max(0, n - (N - K)), min(n, K)
    if N == 0 or a <= lo:
        return 0.0
    lf = lambda x: loggamma(mpf(x) + 1)
    up = a > (n + 1) * (K + 1) // (N + 2)
    k = a if up else a - 1
    t = exp(lf(K) + lf(N - K) + lf(n) + lf(N - n) - lf(N) - lf(k) - lf(K - k) - lf(n - k) - lf(N - K - n + k))
    floor, s = t * mpf(10) ** -45, mpf(0)
    while (k <= hi if up else k >= lo) and t >= floor:
        s += t
        if up:
            t = t * (K - k) * (n - k) / (mpf(k + 1) * (N - K - n + k + 1))
            k += 1
        else:
            t = t * k * (N - K - n + k) / (mpf(K - k + 1) * (n - k + 1))
            k -= 1
    y = float(-log10(s if up else 1 - s))
    return y if y > 0.0 else 0.0


# margins of the wide tables: at each, a = mode, mode + 1, mode +- floor(3 sd), mode + floor(12 sd)
WIDE = [(2 ** 31 - 2, 2 ** 30, 2 ** 30), (2 ** 31 - 2, 2 ** 30, 10 ** 6), (10 ** 8, 5 * 10 ** 7, 10 ** 7),
        (4 * 10 ** 6, 2 * 10 ** 6, 2 * 10 ** 6)]


def table(N, K, n, a):
    return a, K - a, n - a, N - K - n + a


def main():
    T = [("edge", t) for t in [(0, 0, 0, 0), (1, 0, 0, 0), (0, 5, 5, 5), (5, 0, 0, 5), (3, 0, 7, 0), (1, 1, 1, 1)]]
    # a at the support minimum, at the maximum, at the mode and one above it
    for N, K, n in [(30, 12, 9), (30, 25, 20), (1000, 300, 120), (1000, 900, 700), (50000, 20000, 400), (10 ** 6, 3000, 3000),
                    (10 ** 6, 999000, 2000)]:
        lo, hi = max(0, n - (N - K)), min(n, K)
        mode = (n + 1) * (K + 1) // (N + 2)
        for name, a in (("min", lo), ("max", hi), ("mode", mode), ("mode+1", mode + 1)):
            T.append((name, table(N, K, n, a)))
    T.append(("deep", (2000, 1000, 1000, 996000)))
    T.append(("large", (30, 999970, 20, 2 * 10 ** 9)))
    T.append(("large", table(2 ** 31 - 2, 10 ** 9, 40, 35)))
    T.append(("large", table(2 ** 31 - 2, 2 ** 30, 60, 31)))
    T.append(("flat", table(10 ** 6, 500000, 3000, 1501)))      # K = N/2, n = 3000: more than 256 terms before the stop
    T.append(("flat", table(10 ** 6, 500000, 3000, 1500)))      # the same at the mode: the lower side is summed
    out = []
    for name, (a, b, c, d) in T:
        assert min(a, b, c, d) >= 0, (name, a, b, c, d)
        y = exact_plog(a, b, c, d)
        w = wide_plog(a, b, c, d)                             # the second method, on every table the first one reaches
        assert (w == 0.0 if y == 0.0 else abs(w - y) <= 1e-14 * y), (name, a, b, c, d, y, w)
        out.append({"name": name, "a": a, "b": b, "c": c, "d": d, "pvalue_log": repr(y)})
        print(name, a, b, c, d, y)
    for N, K, n in WIDE:
        mode = (n + 1) * (K + 1) // (N + 2)
        sd = math.sqrt(n * (K / N) * (1 - K / N) * (N - n) / (N - 1))
        for a in (mode, mode + 1, mode + int(3 * sd), mode - int(3 * sd), mode + int(12 * sd)):
            a, b, c, d = table(N, K, n, a)
            assert min(a, b, c, d) >= 0, (N, K, n, a)
            y = wide_plog(a, b, c, d)
            out.append({"name": "wide", "a": a, "b": b, "c": c, "d": d, "pvalue_log": repr(y)})
            print("wide", a, b, c, d, y)
    dst = os.path.join(ROOT, "tests", "golden", "fisher_tables.json")
    with open(dst, "w") as f:
        json.dump({"what": "exact -log10 P(X >= a) of 2x2 tables a b / c d (tools/make_fisher_golden.py)", "tables": out}, f, indent=0)
        f.write("\n")
    print(len(out), "tables ->", dst)


if __name__ == "__main__":
    main()
