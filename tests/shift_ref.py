"""numpy restatement of THE SHIFT of include/igd_hip.h (igd_hip_shift_place) and of the local z-score.

A region (c, s, e) on a known contig of length L >= 1 with 0 <= s <= e <= L, len = e - s, under offset d becomes
s' = min(max(s + d, 0), L - len), e' = s' + len, in 64-bit arithmetic.  Regions on unknown contigs and invalid regions pass
through unchanged.  Nothing here calls the code under test."""
import numpy as np


def shift(ichr, qs, qe, ctg_len, offsets, clamp=True):
    """(qs', qe') int32[nshift, nq].  clamp=False: the regions moved without the two clamps, as int64 -- what a generator that
    forgets them would produce (for the fixtures' own sanity checks)."""
    ichr, qs, qe = (np.asarray(a, np.int64) for a in (ichr, qs, qe))
    ctg_len, offsets = np.asarray(ctg_len, np.int64), np.asarray(offsets, np.int64)
    known = (ichr >= 0) & (ichr < len(ctg_len))
    L = np.where(known, ctg_len[np.where(known, ichr, 0)] if len(ctg_len) else 0, 0)
    ln = qe - qs
    valid = known & (L >= 1) & (qs >= 0) & (ln >= 0) & (qs + ln <= L)
    t = qs[None, :] + offsets[:, None]
    if clamp:
        t = np.minimum(np.maximum(t, 0), (L - ln)[None, :])
    s = np.where(valid[None, :], t, qs[None, :])
    e = np.where(valid[None, :], t + ln[None, :], qe[None, :])
    if not clamp:
        return s, e
    return s.astype(np.int32), e.astype(np.int32)


def offsets(window, step):
    k = window // step
    return np.array([j * step for j in range(-k, k + 1)], np.int32)


def zscore(shifted, rows):
    """z[j, f] = (shifted[j, f] - mean_f) / sd_f from the permuted rows int64[nperm, ncols]: numpy's mean and std(ddof=1); NaN
    where sd is 0 or undefined"""
    rows = np.asarray(rows, np.float64)
    mean = rows.mean(axis=0)
    sd = rows.std(axis=0, ddof=1) if len(rows) > 1 else np.full(rows.shape[1], np.nan)
    sd = np.where(sd == 0, np.nan, sd)
    return (np.asarray(shifted, np.float64) - mean[None, :]) / sd[None, :]
