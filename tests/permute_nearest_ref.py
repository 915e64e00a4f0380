"""Reference for the permutation null of the nearest-record distances, in numpy.  A plain module: no pytest hooks.

Nothing here calls the code under test: the generator is tests/permute_ref.py's, the distances and the set statistics are
tests/nearest_ref.py's broadcast over the interval lists the test itself wrote, and the summary is numpy float64 with Python
integers where the comparison has to be exact.

    null(...)          (n_within, n_overlap, sum_dist), int64[nperm + 1, nfiles + 1]: row 0 the set as given, row p + 1 permutation p
    summary(nw, sd)    the twelve columns of igdc_perm_nearest_summary (igd_core.h has the formulas)
    table_text(...)    what `igd search db -q F -P N -g G -D W` prints"""
import numpy as np

import permute_ref as PR
from nearest_ref import mean_text, ref_rows, ref_sets

HEADER = ("index\tn_within\tmean_dist\twithin_mean\twithin_sd\twithin_z\tnlog10_p_within_upper\tdist_mean\tdist_sd\tdist_z\tn_def\t"
          "dist_n_le\tnlog10_p_dist_lower\tFile\n")
FIELDS = ("within_mean", "within_sd", "within_z", "within_n_ge", "nlog10_p_within_upper", "mean_dist", "dist_mean", "dist_sd", "dist_z",
          "n_def", "dist_n_le", "nlog10_p_dist_lower")
INT_FIELDS = ("within_n_ge", "n_def", "dist_n_le")


def null(ldb, ichr, qs, qe, ctg_len, nperm, window, seed=0, mode=PR.CIRCULAR, v=None):
    ichr, qs, qe = np.asarray(ichr, np.int32), np.asarray(qs, np.int32), np.asarray(qe, np.int32)
    nq = len(qs)
    ps, pe = PR.permute(ichr, qs, qe, ctg_len, 0, nperm, seed, mode)
    c = np.tile(ichr, nperm + 1)
    s = np.concatenate([qs, ps.reshape(-1)])
    e = np.concatenate([qe, pe.reshape(-1)])
    dist, dmin = ref_rows(ldb, c, s, e, window, v)
    return ref_sets(dist, dmin, np.arange(nperm + 2, dtype=np.int64) * nq)


def summary(nw, sd):
    """dict of the twelve columns from int64[nperm + 1, ncols] matrices"""
    nw, sd = np.asarray(nw, np.int64), np.asarray(sd, np.int64)
    P, n = nw.shape[0] - 1, nw.shape[1]
    nan = np.full(n, np.nan)
    out = {}
    perm = nw[1:].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["within_mean"] = perm.mean(axis=0)
        out["within_sd"] = perm.std(axis=0, ddof=1) if P > 1 else nan.copy()
        wsd = out["within_sd"]
        out["within_z"] = np.where((wsd == 0) | np.isnan(wsd), np.nan, (nw[0] - out["within_mean"]) / wsd)
        out["within_n_ge"] = (nw[1:] >= nw[0][None, :]).sum(axis=0).astype(np.int64)
        out["nlog10_p_within_upper"] = 0.0 - np.log10((out["within_n_ge"] + 1) / (P + 1))
        out["mean_dist"] = np.where(nw[0] > 0, sd[0].astype(np.float64) / nw[0].astype(np.float64), np.nan)
        dm, ds, ndef, nle = nan.copy(), nan.copy(), np.zeros(n, np.int64), np.zeros(n, np.int64)
        for f in range(n):
            keep = nw[1:, f] > 0
            m = sd[1:, f][keep].astype(np.float64) / nw[1:, f][keep].astype(np.float64)
            ndef[f] = keep.sum()
            if len(m) > 0:
                dm[f] = m.mean()
            if len(m) > 1:
                ds[f] = m.std(ddof=1)
            if nw[0, f] > 0:                                               # exact: Python integers
                nle[f] = sum(1 for p in range(1, P + 1)
                             if nw[p, f] > 0 and int(sd[p, f]) * int(nw[0, f]) <= int(sd[0, f]) * int(nw[p, f]))
        out["dist_mean"], out["dist_sd"], out["n_def"], out["dist_n_le"] = dm, ds, ndef, nle
        out["dist_z"] = np.where((nw[0] <= 0) | (ds == 0) | np.isnan(ds), np.nan, (out["mean_dist"] - dm) / ds)
        out["nlog10_p_dist_lower"] = 0.0 - np.log10((nle + 1) / (P + 1))
    return out


def _f(x, fmt="%.6f"):
    return "NA" if np.isnan(x) else fmt % x


def table_text(names, nw, no, sd, window, nq):
    """the table of the command line from the three reference matrices"""
    s = summary(nw, sd)
    nf = len(names)

    def tail(i):
        return "\t".join([_f(s["within_mean"][i]), _f(s["within_sd"][i]), _f(s["within_z"][i]), _f(s["nlog10_p_within_upper"][i]),
                          _f(s["dist_mean"][i], "%.2f"), _f(s["dist_sd"][i]), _f(s["dist_z"][i]), "%d" % s["n_def"][i],
                          "%d" % s["dist_n_le"][i], _f(s["nlog10_p_dist_lower"][i])])
    out = [HEADER]
    for i in range(nf):
        out.append("%d\t%d\t%s\t%s\t%s\n" % (i, nw[0, i], mean_text(nw[0, i], sd[0, i]), tail(i), names[i]))
    out.append("Regions with a dataset within %d bp: %d of %d; overlapping: %d; mean distance %s\t%s\n"
               % (window, nw[0, nf], nq, no[0, nf], mean_text(nw[0, nf], sd[0, nf]), tail(nf)))
    return "".join(out)
