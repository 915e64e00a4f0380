"""Reference for the permutation null of the base-pair overlap (include/igd_hip.h has the definitions), for
tests/test_permute_bp_host.py, tests/test_permute_bp_cli.py and tests/test_gpu_permute_bp.py.  A plain module: no pytest hooks.

    null(...)      tests/permute_ref.py's generator gives the explicit permuted lists; row 0 (the set as given) and every
                   permuted list go through tests/jaccard_ref.py as one set each: a Python sort and sweep merges them at gap 0,
                   boolean arrays over the interval lists the test wrote give the intersections
    summary(...)   igdc_perm_bp_summary restated: Python integers for the sums, fractions.Fraction for the comparison of the
                   Jaccards, floats only where the definition says double
    table_text()   the block `igd search db -q F -P N -g G -G` prints"""
import math
from fractions import Fraction

import numpy as np

import permute_ref as PR
from jaccard_ref import FLAT, ref_jaccard

FIELDS = ("observed", "mean", "sd", "z", "fold", "n_ge", "n_le", "nlog10_p_upper", "nlog10_p_lower", "jaccard", "jaccard_mean", "jaccard_sd",
          "jaccard_n_def", "jaccard_n_ge")
INT_FIELDS = ("observed", "n_ge", "n_le", "jaccard_n_def", "jaccard_n_ge")


def rows_of(ichr, qs, qe, ctg_len, nperm, seed=0, mode=PR.CIRCULAR):
    """(ichr, qs, qe, set_off) of the nperm + 1 rows as sets: row 0 the regions as given, row p + 1 permutation p"""
    ichr, qs, qe = (np.asarray(a, np.int32) for a in (ichr, qs, qe))
    ps, pe = PR.permute(ichr, qs, qe, ctg_len, 0, nperm, seed, mode)
    nq = len(qs)
    return (np.tile(ichr, nperm + 1), np.concatenate([qs, ps.reshape(-1)]).astype(np.int32), np.concatenate([qe, pe.reshape(-1)]).astype(np.int32),
            np.arange(nperm + 2, dtype=np.int64) * nq)


def null(db, ichr, qs, qe, ctg_len, nperm, seed=0, mode=PR.CIRCULAR, v=None, rule=FLAT):
    """(inter int64[nperm + 1, nfiles + 1], set_bp, n_merged int64[nperm + 1], n_dropped, file_bp int64[nfiles + 1])"""
    inter, set_bp, file_bp, n_merged, dropped = ref_jaccard(db, *rows_of(ichr, qs, qe, ctg_len, nperm, seed, mode), v, rule)
    assert len(set(dropped.tolist())) == 1, "a permutation changed the regions that take part"
    return inter, set_bp, n_merged.astype(np.int64), int(dropped[0]), file_bp


def summary(inter, set_bp, file_bp):
    """dict of arrays [ncols], the names of FIELDS"""
    inter = [[int(x) for x in row] for row in np.asarray(inter)]
    set_bp, file_bp = [int(x) for x in set_bp], [int(x) for x in file_bp]
    P, nc = len(inter) - 1, len(file_bp)
    nan = float("nan")
    out = {k: [] for k in FIELDS}
    for f in range(nc):
        x0 = inter[0][f]
        xs = [inter[p][f] for p in range(1, P + 1)]
        us = [set_bp[p] + file_bp[f] - inter[p][f] for p in range(P + 1)]
        sm, sq = sum(xs), sum(x * x for x in xs)
        mu = float(sm) / float(P)
        sd = math.sqrt(float(P * sq - sm * sm) / (float(P) * (float(P) - 1.0))) if P > 1 else nan
        nge, nle = sum(x >= x0 for x in xs), sum(x <= x0 for x in xs)
        out["observed"].append(x0)
        out["mean"].append(mu)
        out["sd"].append(sd)
        out["z"].append(nan if sd != sd or sd == 0.0 else (float(x0) - mu) / sd)
        out["fold"].append(float(x0) / mu if mu != 0.0 else nan)
        out["n_ge"].append(nge)
        out["n_le"].append(nle)
        out["nlog10_p_upper"].append(0.0 - math.log10(float(nge + 1) / (float(P) + 1.0)))
        out["nlog10_p_lower"].append(0.0 - math.log10(float(nle + 1) / (float(P) + 1.0)))
        js = [float(x) / float(u) for x, u in zip(xs, us[1:]) if u != 0]
        acc = 0.0
        for j in js:
            acc += j
        jmu = acc / float(len(js)) if js else nan
        ss = 0.0
        for j in js:
            ss += (j - jmu) * (j - jmu)
        out["jaccard"].append(float(x0) / float(us[0]) if us[0] != 0 else nan)
        out["jaccard_mean"].append(jmu)
        out["jaccard_sd"].append(math.sqrt(ss / float(len(js) - 1)) if len(js) > 1 else nan)
        out["jaccard_n_def"].append(len(js))
        out["jaccard_n_ge"].append(sum(Fraction(x, u) >= Fraction(x0, us[0]) for x, u in zip(xs, us[1:]) if u != 0) if us[0] != 0 else 0)
    return {k: np.array(a, np.int64 if k in INT_FIELDS else np.float64) for k, a in out.items()}


def _na(x, fmt="%.6f"):
    return "NA" if x != x else fmt % x


def table_text(names, inter, set_bp, n_merged, n_dropped, file_bp):
    s = summary(inter, set_bp, file_bp)
    nf = len(names)
    out = ["index\tobserved_bp\tmean\tsd\tz\tfold\tn_ge\tn_le\tnlog10_p_upper\tnlog10_p_lower\tjaccard\tjaccard_mean\tFile\n"]
    for i in range(nf + 1):
        head = "%d\t%d" % (i, s["observed"][i]) if i < nf else ("Any dataset: %d of %d bp in %d merged regions (%d dropped)"
                                                               % (s["observed"][i], set_bp[0], n_merged[0], n_dropped))
        cols = [_na(s[k][i]) for k in ("mean", "sd", "z", "fold")] + ["%d" % s["n_ge"][i], "%d" % s["n_le"][i]]
        cols += [_na(s[k][i]) for k in ("nlog10_p_upper", "nlog10_p_lower", "jaccard", "jaccard_mean")]
        out.append(head + "\t" + "\t".join(cols) + ("\t%s\n" % names[i] if i < nf else "\n"))
    return "".join(out)
