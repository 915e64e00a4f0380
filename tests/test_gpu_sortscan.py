"""The two device primitives of igd_sortscan.hpp, directly: exclusive_scan<uint32_t, int64_t> and radix_sort_pairs through the
TEST-ONLY entries igd_hip_test_exclusive_scan / igd_hip_test_radix_sort_pairs (include/igd_hip.h).  `igd create`, Seqpare and the
merge behind -J / -G are built on them, and reach them only at small sizes and with small counts.

The scan is compared with np.cumsum in int64, the sort with np.argsort(kind="stable") of the keys; every integer must be equal
and outputs are handed over full of 0x5a.  The constants are read from the source, and every large case first asserts from them
that the tile sums take ss_scan_of_sums past one round of its workgroup (or two): with a changed constant it fails there.  The
entries put guard bytes behind every device array, sized as the comment above radix_sort_pairs promises: a kernel that writes
past such a size fails the call with -1."""
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from igd_amd import _native

pytestmark = pytest.mark.gpu

G64 = 0x5a5a5a5a5a5a5a5a
FULL = 0xffffffff


def constants():
    """(SCAN_TILE, RS_BLOCK, the tile sums one round of ss_scan_of_sums takes) from igd_sortscan.hpp"""
    src = open(os.path.join(ROOT, "igd_amd", "csrc", "igd_sortscan.hpp")).read()
    g = lambda name: int(re.search(r"^#define\s+%s\s+(\d+)" % name, src, re.M).group(1))       # noqa: E731
    bound = int(re.search(r"__launch_bounds__\((\d+)\)\s+ss_scan_of_sums\(", src).group(1))
    step = int(re.search(r"base < nb; base \+= (\d+)\)", src).group(1))
    launch = int(re.search(r"ss_scan_of_sums<<<1, (\d+),", src).group(1))
    last = int(re.search(r"threadIdx\.x == (\d+)\) carry = pre", src).group(1))
    assert bound == step == launch == last + 1, (bound, step, launch, last)
    return g("SCAN_WG") * g("SCAN_PER"), g("RS_WG") * g("RS_STRIPS"), step


SCAN_TILE, RS_BLOCK, SUMS_WG = constants()
ROUND = SUMS_WG * SCAN_TILE                      # elements of one round of the sums workgroup
LARGEST = 2 * ROUND + SCAN_TILE + 5              # a third round and a ragged last tile


def tiles(n):
    return -(-n // SCAN_TILE)


def scan(a, n=None, null=()):
    """igd_hip_test_exclusive_scan on a uint32 array -> (rc, out, total); out and total go in full of 0x5a"""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    n = len(a) if n is None else n
    out, total = np.full(len(a), G64, np.int64), np.full(1, G64, np.int64)
    p = [None if k in null else x.ctypes.data for k, x in enumerate((a, out, total))]
    rc = _native.hip().igd_hip_test_exclusive_scan(0, p[0], n, p[1], p[2])
    return rc, out, int(total[0])


def check_scan(a, what):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    inc = np.cumsum(a, dtype=np.int64)
    rc, out, total = scan(a)
    assert rc == 0, (what, _native.hip().igd_hip_last_error())
    assert total == (int(inc[-1]) if len(a) else 0), (what, total)
    bad = np.flatnonzero(out != inc - a)
    assert len(bad) == 0, (what, len(bad), int(bad[0]), int(out[bad[0]]), int((inc - a)[bad[0]]))
    return total


def full_range(rng, n):
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    a[rng.integers(0, n, max(1, n // 97))] = FULL
    return a


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_scan_small_sizes(n):
    rng = np.random.default_rng(4100 + n)
    assert check_scan(np.ones(n, np.uint32), "ones") == n
    if n:
        check_scan(full_range(rng, n), "full range")
        check_scan(np.full(n, FULL, np.uint32), "all 0xffffffff")


def singles(n):
    """positions of the one 0xffffffff: either side of the first round seam, the first element of the last tile sum of the
    first round, the last element"""
    return sorted({p for p in (ROUND - 1, ROUND, (SUMS_WG - 1) * SCAN_TILE, n - 1) if p < n})


@pytest.mark.parametrize("n,rounds", [(ROUND - 1, 1), (ROUND, 1), (ROUND + 1, 2), (LARGEST, 3)])
def test_scan_around_a_round_of_the_sums_workgroup(n, rounds):
    assert -(-tiles(n) // SUMS_WG) == rounds, "%d elements are %d tile sums: not %d rounds of %d" % (n, tiles(n), rounds, SUMS_WG)
    assert n == LARGEST or abs(tiles(n) - SUMS_WG) <= 1
    assert n != LARGEST or (tiles(n) > 2 * SUMS_WG and n % SCAN_TILE not in (0, 1, SCAN_TILE - 1))
    rng = np.random.default_rng(4200 + rounds)
    assert check_scan(np.ones(n, np.uint32), "ones") == n           # out[i] == i: a misplaced carry reads off directly
    total = check_scan(full_range(rng, n), "full range")
    assert n != LARGEST or total > 1 << 53                          # (beyond what a double holds: integers are compared)
    for p in singles(n):
        a = np.zeros(n, np.uint32)
        a[p] = FULL
        assert check_scan(a, ("single", p)) == FULL


def test_scan_refusals_write_nothing():
    a = np.arange(10, dtype=np.uint32)
    for n, null in ((-1, ()), (10, (0,)), (10, (1,)), (10, (2,)), (0, (2,)), ((1 << 31) + 1, ())):
        rc, out, total = scan(a, n, null)
        assert rc == -2 and (out == G64).all() and total == G64, (n, null)
    rc, out, total = scan(a, 0)                                     # n == 0: the total alone
    assert rc == 0 and (out == G64).all() and total == 0


# ---- the sort ---------------------------------------------------------------------------------------------------------------
def sort(keys, vals, bits, n=None, null=()):
    """igd_hip_test_radix_sort_pairs on copies -> (rc, keys, vals)"""
    k, v = np.array(keys, dtype=np.uint32), np.array(vals, dtype=np.uint32)
    n = len(k) if n is None else n
    p = [None if i in null else x.ctypes.data for i, x in enumerate((k, v))]
    rc = _native.hip().igd_hip_test_radix_sort_pairs(0, p[0], p[1], n, bits)
    return rc, k, v


def stable_order(keys, bits):
    """np.argsort(kind="stable"); keys that fit 8 or 16 bits are cast down, where numpy sorts by radix"""
    small = keys.astype(np.uint8 if bits <= 8 else np.uint16 if bits <= 16 else np.uint32)
    assert np.array_equal(small, keys)
    return np.argsort(small, kind="stable")


def check_sort(rng, keys, bits, what):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    n = len(keys)
    assert bits == 32 or bits == 0 or int(keys.max()) < 1 << bits          # (as every caller: keys below 2^bits)
    ref = stable_order(keys, bits) if bits else np.arange(n)               # (0 bits: both arrays as given)
    for payload in ("arange", "random"):
        vals = np.arange(n, dtype=np.uint32) if payload == "arange" else rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        rc, k, v = sort(keys, vals, bits)
        assert rc == 0, (what, payload, _native.hip().igd_hip_last_error())
        assert np.array_equal(k, keys[ref]), (what, payload, "keys")
        bad = np.flatnonzero(v != vals[ref])
        assert len(bad) == 0, (what, payload, "vals", len(bad), int(bad[0]))


def skewed(rng, n, top):
    """about 90 % one value, the rest uniform"""
    keys = rng.integers(0, top + 1, n, dtype=np.uint64)
    keys[rng.random(n) < 0.9] = rng.integers(0, top + 1)
    return keys


def key_shapes(rng, n, bits):
    top = (1 << (bits if bits else 32)) - 1                                 # (0 bits: nothing is ordered, any key will do)
    uniform = rng.integers(0, top + 1, n, dtype=np.uint64)
    yield "uniform", uniform
    yield "all 0", np.zeros(n, np.uint64)
    yield "all 2^bits - 1", np.full(n, top, np.uint64)                      # (32 bits: the padding value of a ragged last strip)
    yield "two values", np.where(np.arange(n) & 1, top, top >> 1).astype(np.uint64)
    yield "skewed", skewed(rng, n, top)
    yield "sorted", np.sort(uniform)
    yield "reverse sorted", np.sort(uniform)[::-1]


SORT_SIZES = [1, 63, 64, 65, 511, 512, 513, RS_BLOCK - 1, RS_BLOCK, RS_BLOCK + 1, 3 * RS_BLOCK + 77]


@pytest.mark.parametrize("bits", [0, 1, 8, 9, 16, 24, 32])
def test_sort_is_the_stable_sort(bits):
    rng = np.random.default_rng(4300 + bits)
    for n in SORT_SIZES:
        for what, keys in key_shapes(rng, n, bits):
            check_sort(rng, keys, bits, (n, what))


@pytest.mark.parametrize("bits,shape", [(8, "uniform"), (16, "uniform"), (8, "skewed")])
def test_sort_past_one_round_of_the_histogram_scan(bits, shape):
    n = 8192 * RS_BLOCK + RS_BLOCK + 7
    hist = -(-n // RS_BLOCK) * 256                                          # entries of the digit histogram, scanned per pass
    assert tiles(hist) > SUMS_WG, "%d histogram entries are %d tile sums: one round of %d" % (hist, tiles(hist), SUMS_WG)
    assert n % RS_BLOCK not in (0, 1, RS_BLOCK - 1)
    rng = np.random.default_rng(4400 + bits)
    top = (1 << bits) - 1
    keys = rng.integers(0, top + 1, n, dtype=np.uint64) if shape == "uniform" else skewed(rng, n, top)
    check_sort(rng, keys, bits, (n, shape))


def test_sort_refusals_write_nothing():
    keys, vals = np.array([3, 1, 2, 0], np.uint32), np.array([9, 8, 7, 6], np.uint32)
    for n, bits, null in ((-1, 8, ()), (4, 33, ()), (4, -1, ()), (4, 8, (0,)), (4, 8, (1,)), ((1 << 31) + 1, 8, ())):
        rc, k, v = sort(keys, vals, bits, n, null)
        assert rc == -2 and np.array_equal(k, keys) and np.array_equal(v, vals), (n, bits, null)
    rc, k, v = sort(keys, vals, 8, 0)
    assert rc == 0 and np.array_equal(k, keys) and np.array_equal(v, vals)
