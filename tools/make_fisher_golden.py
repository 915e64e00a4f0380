#!/usr/bin/env python3
"""Writes tests/golden/fisher_tables.json: 2x2 tables with their exact -log10 P(X >= a), X ~ Hypergeometric(a+b+c+d, a+b,
a+c) -- the one-sided Fisher test of igd_hip_fisher_tables / igdc_fisher_host.  The tail is summed in Python integers
(math.comb) and its logarithm taken with mpmath at 60 digits; no GPU and nothing of the project is used.

    python tools/make_fisher_golden.py
"""
import json
import math
import os

from mpmath import log10, mp, mpf

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
        out.append({"name": name, "a": a, "b": b, "c": c, "d": d, "pvalue_log": repr(y)})
        print(name, a, b, c, d, y)
    dst = os.path.join(ROOT, "tests", "golden", "fisher_tables.json")
    with open(dst, "w") as f:
        json.dump({"what": "exact -log10 P(X >= a) of 2x2 tables a b / c d (tools/make_fisher_golden.py)", "tables": out}, f, indent=0)
        f.write("\n")
    print(len(out), "tables ->", dst)


if __name__ == "__main__":
    main()
