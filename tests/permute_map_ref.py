"""Reference for the permutation null of the overlapping records' values, in numpy.  A plain module: no pytest hooks.

Nothing here calls the code under test: the permuted sets are tests/permute_ref.py's generator (workspace_ref's placement,
resample_ref's draw), the counts and aggregates are tests/map_ref.py's broadcast over the interval lists the test itself wrote,
and the summary is numpy float64 with Python integers where the comparison has to be exact.

    rows_of(...)       the nperm + 1 region sets of a null, concatenated: (ichr, qs, qe, set_off)
    null(...)          (n_hit, pairs, agg_sum), int64[nperm + 1, nfiles]: row 0 the set as given, row p + 1 permutation p
    summary(...)       the columns of igdc_perm_map_summary (igd_core.h has the formulas), observed_n_hit in front
    table_text(...)    what `igd search db -q F -P N -g G -I op` prints"""
import numpy as np

import permute_ref as PR
import resample_ref as RR
import workspace_ref as WR
from map_ref import ref_rows, ref_sets

FIELDS = ("observed_n_hit", "observed", "n_def", "mean", "sd", "z", "n_ge", "n_le", "nlog10_p_upper", "nlog10_p_lower", "nhit_mean", "nhit_sd",
          "nhit_z")
INT_FIELDS = ("observed_n_hit", "n_def", "n_ge", "n_le")
HEADER = "index\tobserved_n_hit\tobserved_mean_%s\tn_def\tmean\tsd\tz\tn_ge\tn_le\tmlog10p_ge\tmlog10p_le\tnhit_mean\tnhit_sd\tnhit_z\tFile\n"


def rows_of(ichr, qs, qe, ctg_len, nperm, seed=0, mode=PR.CIRCULAR, tab=None, pool=None):
    """mode "workspace" takes workspace_ref's table, mode "resample" the pool (ichr, qs, qe); ctg_len is not read then"""
    ichr, qs, qe = np.asarray(ichr, np.int32), np.asarray(qs, np.int32), np.asarray(qe, np.int32)
    nq = len(qs)
    if mode == "resample":
        return RR.resample_sets((ichr, qs, qe), pool, nperm, seed)
    if mode == "workspace":
        ps, pe = WR.place(ichr, qs, qe, ctg_len, tab, 0, nperm, seed)
    else:
        ps, pe = PR.permute(ichr, qs, qe, ctg_len, 0, nperm, seed, mode)
    return (np.tile(ichr, nperm + 1), np.concatenate([qs, ps.reshape(-1)]), np.concatenate([qe, pe.reshape(-1)]),
            np.arange(nperm + 2, dtype=np.int64) * nq)


def run_op(op):
    """op "mean" runs the rows of op sum"""
    return "sum" if op == "mean" else op


def null(ldb, ichr, qs, qe, ctg_len, nperm, op, seed=0, mode=PR.CIRCULAR, v=None, tab=None, pool=None):
    c, s, e, off = rows_of(ichr, qs, qe, ctg_len, nperm, seed, mode, tab, pool)
    return ref_sets(*ref_rows(ldb, c, s, e, run_op(op), v), off)


def summary(n_hit, pairs, agg_sum, op):
    """dict of FIELDS from int64[nperm + 1, ncols] matrices.  The statistic of a row is agg_sum / n_hit, for op "mean" agg_sum /
    pairs, undefined where the divisor is 0; two ratios are compared by cross-multiplying Python integers."""
    nh, den, sa = np.asarray(n_hit, np.int64), np.asarray(pairs if op == "mean" else n_hit, np.int64), np.asarray(agg_sum, np.int64)
    P, n = nh.shape[0] - 1, nh.shape[1]
    out = {k: (np.zeros(n, np.int64) if k in INT_FIELDS else np.full(n, np.nan)) for k in FIELDS}
    out["observed_n_hit"] = nh[0].copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        perm = nh[1:].astype(np.float64)
        out["nhit_mean"] = perm.mean(axis=0)
        if P > 1:
            out["nhit_sd"] = perm.std(axis=0, ddof=1)
        hs = out["nhit_sd"]
        out["nhit_z"] = np.where((hs == 0) | np.isnan(hs), np.nan, (nh[0] - out["nhit_mean"]) / hs)
    for f in range(n):
        a0, d0 = int(sa[0, f]), int(den[0, f])
        keep = [p for p in range(1, P + 1) if den[p, f] > 0]
        m = np.array([float(sa[p, f]) / float(den[p, f]) for p in keep], np.float64)
        out["n_def"][f] = len(keep)
        if len(m) > 0:
            out["mean"][f] = m.mean()
        if len(m) > 1:
            out["sd"][f] = m.std(ddof=1)
        if d0 <= 0:
            continue                                                       # observed, z and both p stay NaN; n_ge = n_le = 0
        out["observed"][f] = float(a0) / float(d0)
        out["n_ge"][f] = sum(1 for p in keep if int(sa[p, f]) * d0 >= a0 * int(den[p, f]))
        out["n_le"][f] = sum(1 for p in keep if int(sa[p, f]) * d0 <= a0 * int(den[p, f]))
        sd = out["sd"][f]
        if not np.isnan(sd) and sd != 0:
            out["z"][f] = (out["observed"][f] - out["mean"][f]) / sd
        out["nlog10_p_upper"][f] = 0.0 - np.log10((out["n_ge"][f] + 1) / (len(keep) + 1))
        out["nlog10_p_lower"][f] = 0.0 - np.log10((out["n_le"][f] + 1) / (len(keep) + 1))
    return out


def _f(x):
    return "NA" if np.isnan(x) else "%.6f" % x


def table_text(names, n_hit, pairs, agg_sum, op):
    """the table of the command line from the three reference matrices"""
    s = summary(n_hit, pairs, agg_sum, op)
    out = [HEADER % op]
    for i, name in enumerate(names):
        out.append("\t".join(["%d" % i, "%d" % s["observed_n_hit"][i], _f(s["observed"][i]), "%d" % s["n_def"][i], _f(s["mean"][i]), _f(s["sd"][i]),
                              _f(s["z"][i]), "%d" % s["n_ge"][i], "%d" % s["n_le"][i], _f(s["nlog10_p_upper"][i]), _f(s["nlog10_p_lower"][i]),
                              _f(s["nhit_mean"][i]), _f(s["nhit_sd"][i]), _f(s["nhit_z"][i]), name]) + "\n")
    return "".join(out)
