"""THE DRAW of include/igd_hip.h in numpy uint64, written from its definition: the keyed bijection on [0, n) -- a four-round
Feistel network on 2^(2h) >= n points with cycle walking -- and the explicit region lists of a resampling null."""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
U = np.uint64


def mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U(30))) * M1
        z = (z ^ (z >> U(27))) * M2
        return z ^ (z >> U(31))


def perm_base(seed, p):
    with np.errstate(over="ignore"):
        a = mix64(U(seed & (2 ** 64 - 1)) + G)
        return mix64(a + U(p + 1) * G)


def bits(n):
    h = 1
    while 4 ** h < n:
        h += 1
    return h


def step(base, x, h):
    mask = U((1 << h) - 1)
    L, R = x >> U(h), x & mask
    with np.errstate(over="ignore"):
        for j in range(4):
            f = mix64(base + ((U(j + 1) << U(32)) + R + U(1)) * G) & mask
            L, R = R, L ^ f
    return (L << U(h)) | R


def resample_indices(seed, p, nq, n, steps=None):
    """int64[nq]: igd_hip_resample_index(base(seed, p), i, n) for i = 0 .. nq - 1 (nq <= n); steps, a list, receives the longest walk"""
    assert 1 <= n < 2 ** 31 and 0 <= nq <= n
    h, base = bits(n), perm_base(seed, p)
    y = step(base, np.arange(nq, dtype=np.uint64), h)
    walks = 1
    while True:
        out = y >= U(n)
        if not out.any():
            break
        y[out] = step(base, y[out], h)
        walks += 1
    if steps is not None:
        steps.append(walks)
    return y.astype(np.int64)


def resample_regions(pool, nq, p0, np_, seed):
    """(ichr, qs, qe) int32[np_, nq]: draws p0 .. p0 + np_ - 1 of nq regions from the pool (ichr, qs, qe)"""
    pc, ps, pe = (np.asarray(a, dtype=np.int32) for a in pool)
    idx = np.stack([resample_indices(seed, p0 + k, nq, len(ps)) for k in range(np_)]) if np_ else np.zeros((0, nq), np.int64)
    return pc[idx], ps[idx], pe[idx]


def resample_sets(q, pool, nperm, seed):
    """the nperm + 1 rows of a resampling null as concatenated sets (ichr, qs, qe, set_off): row 0 the set q as given, row p + 1
    draw p of len(q[1]) regions from the pool"""
    nq = len(q[1])
    dc, ds, de = resample_regions(pool, nq, 0, nperm, seed)
    cat = [np.concatenate([np.asarray(a, dtype=np.int32), d.ravel()]) for a, d in zip(q, (dc, ds, de))]
    return (*cat, np.arange(nperm + 2, dtype=np.int64) * nq)
