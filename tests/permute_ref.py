"""Reference for the permutation null of region-set support, in numpy.  A plain module: no pytest hooks.

The generator is the definition of include/igd_hip.h written out once more in numpy uint64 (arithmetic modulo 2^64):

    G = 0x9E3779B97F4A7C15
    mix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31
    r(p, k) = mix64(mix64(mix64(seed + G) + (p + 1) * G) + (k + 1) * G)

    permute(...)   the explicit permuted lists, int32[np, nq] each
    stats(...)     sum, sumsq, n_ge, n_le, min, max of a row matrix, column by column, in Python integers where they may be large
    summary(...)   mean, sd (ddof = 1), z and -log10 p from the rows themselves"""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
CIRCULAR, SHUFFLE = "circular", "shuffle"


def mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def r(seed, p, k):
    """r(p, k) for arrays p and k (broadcast), uint64"""
    p, k = np.asarray(p, np.uint64), np.asarray(k, np.uint64)
    with np.errstate(over="ignore"):
        base = mix64(mix64(np.uint64(seed & (2 ** 64 - 1)) + G) + (p + np.uint64(1)) * G)
        return mix64(base + (k + np.uint64(1)) * G)


def permute(ichr, qs, qe, ctg_len, p0, np_, seed=0, mode=CIRCULAR):
    """(qs', qe') int32[np_, nq]: permutations p0 .. p0 + np_ - 1 of the regions.  Valid regions on known contigs only are
    moved; a region with ichr outside [0, len(ctg_len)) passes through unchanged."""
    ichr = np.asarray(ichr, np.int64)
    s, e = np.asarray(qs, np.int64), np.asarray(qe, np.int64)
    ctg_len = np.asarray(ctg_len, np.int64)
    nq, nctg = len(s), len(ctg_len)
    known = (ichr >= 0) & (ichr < nctg)
    c = np.where(known, ichr, 0)
    L = ctg_len[c] if nctg else np.ones(nq, np.int64)
    ln = e - s
    assert (~known | ((L >= 1) & (s >= 0) & (ln >= 0) & (e <= L))).all(), "permute_ref.permute: an invalid region on a known contig"
    L = np.where(known, L, 1)
    ln = np.where(known, ln, 0)
    p = (np.arange(np_, dtype=np.uint64) + np.uint64(p0))[:, None]
    key = (np.arange(nq, dtype=np.uint64) if mode == SHUFFLE else c.astype(np.uint64))[None, :]
    rr = r(seed, p, key)                                                      # uint64[np_, nq]
    Lu, lnu = L.astype(np.uint64)[None, :], ln.astype(np.uint64)[None, :]
    if mode == SHUFFLE:
        t = (rr % (Lu - lnu + np.uint64(1))).astype(np.int64)
    else:
        t = ((np.where(known, s, 0).astype(np.uint64)[None, :] + rr % Lu) % Lu).astype(np.int64)
        t = np.where(ln[None, :] == L[None, :], 0, np.where(t + ln[None, :] > L[None, :], L[None, :] - ln[None, :], t))
    out_s = np.where(known[None, :], t, s[None, :])
    out_e = np.where(known[None, :], t + ln[None, :], e[None, :])
    return out_s.astype(np.int32), out_e.astype(np.int32)


def stats(rows, observed):
    """(sum, sumsq, n_ge, n_le, min, max), int64[ncols] each; sums modulo 2^64 as two's complement"""
    rows = np.asarray(rows, np.int64)
    observed = np.asarray(observed, np.int64)
    assert rows.ndim == 2 and rows.shape[0] >= 1 and observed.shape == (rows.shape[1],)
    u = rows.astype(np.uint64)
    with np.errstate(over="ignore"):
        sm = u.sum(axis=0, dtype=np.uint64).view(np.int64)
        sq = (u * u).sum(axis=0, dtype=np.uint64).view(np.int64)
    return (sm, sq, (rows >= observed[None, :]).sum(axis=0).astype(np.int64), (rows <= observed[None, :]).sum(axis=0).astype(np.int64),
            rows.min(axis=0), rows.max(axis=0))


def summary(rows, observed):
    """(mean, sd, z, nlog10_p_upper, nlog10_p_lower) float64[ncols] from the rows: numpy's mean and std(ddof=1)"""
    rows = np.asarray(rows, np.float64)
    observed = np.asarray(observed, np.float64)
    P = rows.shape[0]
    mean = rows.mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = rows.std(axis=0, ddof=1) if P > 1 else np.full(rows.shape[1], np.nan)
        z = np.where((sd == 0) | np.isnan(sd), np.nan, (observed - mean) / sd)
    pu = 0.0 - np.log10(((rows >= observed[None, :]).sum(axis=0) + 1) / (P + 1))
    pl = 0.0 - np.log10(((rows <= observed[None, :]).sum(axis=0) + 1) / (P + 1))
    return mean, sd, z, pu, pl


def random_regions(rng, ctg_len, n, unknown=(-1, 99)):
    """n valid regions (rng: random.Random): contigs drawn from the known ones and `unknown`; on a known contig of length L
    a start in [0, L] and a width from a few kinds clipped to the contig (0, 1, short, long, the rest of the contig); on an
    unknown one any coordinates.  Every fifth region repeats its predecessor."""
    nctg = len(ctg_len)
    ichr, qs, qe = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        c = rng.choice(list(range(nctg)) + list(unknown))
        if 0 <= c < nctg:
            L = int(ctg_len[c])
            s = rng.randrange(0, L + 1)
            ln = min(rng.choice([0, 1, 200, 700, L // 7, L // 2, L, rng.randint(1, max(1, L // 20))]), L - s)
        else:
            s, ln = rng.randrange(0, 1 << 20), rng.choice([0, 5, 3000, -7])
        ichr[i], qs[i], qe[i] = c, s, s + ln
    for i in range(5, n, 5):
        ichr[i], qs[i], qe[i] = ichr[i - 1], qs[i - 1], qe[i - 1]
    return ichr, qs, qe
