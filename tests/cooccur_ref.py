"""References for the co-occurrence tests (tests/test_cooccur_host.py, test_cooccur_cli.py, test_gpu_cooccur.py).  A plain
module: no pytest hooks.  Nothing here calls the code under test.

    cooc(member)            member.T @ member on an unpacked bool matrix, int64
    jaccard(cooc)           cooc[f, g] / (cooc[f, f] + cooc[g, g] - cooc[f, g]) in float64, NaN where the denominator is 0
    unpack(bits, nbits)     uint32 rows -> bool[nrows, nbits], bit b = bit b & 31 of word b >> 5 (np.unpackbits)
    transpose(bits)         the expected output of the transpose: uint64[32 * nW, ceil(nrows / 64)]
    gram(a, b)              popcount(a_i & b_j) from unpacked rows, int64[m, n]
    random_rows(...)        bit rows of a given density"""
import numpy as np


def cooc(member):
    m = np.asarray(member).astype(np.int64)
    return m.T @ m


def jaccard(c):
    c = np.asarray(c, np.int64)
    d = np.diagonal(c)
    den = d[:, None] + d[None, :] - c
    out = np.full(c.shape, np.nan, np.float64)
    ok = den != 0
    out[ok] = c[ok].astype(np.float64) / den[ok].astype(np.float64)
    return out


def unpack(bits, nbits=None):
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    n, nw = bits.shape
    if n == 0 or nw == 0:
        return np.zeros((n, 32 * nw if nbits is None else nbits), bool)
    b = np.unpackbits(bits.astype("<u4").view(np.uint8).reshape(n, -1), axis=1, bitorder="little").astype(bool)
    return b if nbits is None else b[:, :nbits]


def transpose(bits):
    """column c of the result holds, for every row r, bit c of the row at bit r & 63 of word r >> 6; the tail is 0"""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    n, nw = bits.shape
    cw = (n + 63) // 64
    wide = np.zeros((32 * nw, cw * 64), np.uint8)
    wide[:, :n] = unpack(bits).T
    return np.packbits(wide, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(32 * nw, cw)


def gram(a, b=None):
    ua = unpack(a).astype(np.int64)
    ub = ua if b is None else unpack(b).astype(np.int64)
    return ua @ ub.T


def random_rows(rs, n, nwords, kind):
    """kind: "half" (density 0.5), "sparse" (one bit in 64), "ones" """
    if kind == "ones":
        return np.full((n, nwords), 0xffffffff, np.uint32)
    x = rs.integers(0, 1 << 32, (n, nwords), dtype=np.uint64).astype(np.uint32)
    if kind == "sparse":
        for _ in range(5):
            x &= rs.integers(0, 1 << 32, (n, nwords), dtype=np.uint64).astype(np.uint32)
    return x
