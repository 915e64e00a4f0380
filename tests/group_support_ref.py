"""Reference for support per GROUP of datasets (igd_hip_group_support_sets, igdc_group_support_host_ov), in plain Python.

    gmember_q[g]       = 1 iff the datasets region q overlaps (F_q) hold a dataset of group g
    group_support_S[g] = the regions q of S with gmember_q[g] = 1
    group_nhit_S       = the regions q of S that meet any dataset with at least one group

F_q comes from outside the code under test: from the CPU oracle one region at a time (oracle_member; under a minimum overlap
from its enumeration, oracle_member_ov), or from the unpacked rows of a membership function that has tests of its own.
region_groups() turns ONE region's file set into its group set; expected() sums that over the regions of each set, in loops.
fold() is the same number a second way, as a numpy product over a whole member matrix.  nonvacuous() states, on expected
values only, the three conditions every fixture has to meet."""
import numpy as np


def region_groups(files, labels):
    """the groups of one region: files = the datasets it overlaps, labels[f] = the group numbers of dataset f"""
    out = set()
    for f in files:
        out.update(labels[f])
    return out


def oracle_member(orc, ichr, qs, qe, v=0):
    """bool[nq, nfiles] from Oracle.search on one region at a time (the dispatch of `-v v`)"""
    m = np.zeros((len(qs), orc.nfiles), bool)
    for i in range(len(qs)):
        h, _ = orc.search(ichr[i:i + 1], qs[i:i + 1], qe[i:i + 1], v)
        m[i] = h > 0
    return m


def oracle_member_ov(orc, ichr, qs, qe, min_bp=0, ppm_query=0, ppm_record=0):
    """bool[nq, nfiles] under a minimum overlap per pair (rule NEST, no filter), from the oracle's enumeration: the pair test of
    include/igd_hip.h in Python integers"""
    qoff, rec = orc.enumerate(ichr, qs, qe)
    m = np.zeros((len(qs), orc.nfiles), bool)
    for i in range(len(qs)):
        lenq = int(qe[i]) - int(qs[i])
        if lenq <= 0:
            continue
        need = max(int(min_bp), 1, -((-lenq * int(ppm_query)) // 1000000))
        for idx, s, e in rec[qoff[i]:qoff[i + 1]].tolist():
            ov = min(int(qe[i]), e) - max(int(qs[i]), s)
            if 0 <= idx < orc.nfiles and ov >= need and ov * 1000000 >= (e - s) * int(ppm_record):
                m[i, idx] = True
    return m


def labels_of(groups):
    """[[group numbers of dataset f]] of a DatasetGroups"""
    return [[int(g) for g in groups.idx[groups.off[f]:groups.off[f + 1]]] for f in range(groups.nfiles)]


def expected(member, groups, set_off):
    """(gsupport int64[nsets, ngroups], gnhit int64[nsets]) region by region"""
    labels = labels_of(groups)
    nsets = len(set_off) - 1
    gsup, gnhit = np.zeros((nsets, groups.ngroups), np.int64), np.zeros(nsets, np.int64)
    for k in range(nsets):
        for q in range(int(set_off[k]), int(set_off[k + 1])):
            gs = region_groups(np.flatnonzero(member[q]).tolist(), labels)
            for g in gs:
                gsup[k, g] += 1
            gnhit[k] += bool(gs)
    return gsup, gnhit


def fold(member, groups, set_off):
    """the same from a whole member matrix in numpy: any per group, sum per set"""
    gm = (member.astype(np.int64) @ groups.dense().astype(np.int64)) > 0
    nsets = len(set_off) - 1
    gsup = np.array([gm[set_off[k]:set_off[k + 1]].sum(axis=0) for k in range(nsets)], np.int64).reshape(nsets, groups.ngroups)
    gnhit = np.array([gm[set_off[k]:set_off[k + 1]].any(axis=1).sum() for k in range(nsets)], np.int64)
    return gsup, gnhit


def bounds(member, groups, set_off):
    """(lo, hi int64[nsets, ngroups]): max and min(sum, |S|) of the per-dataset supports over each group's datasets"""
    dense = groups.dense()
    nsets = len(set_off) - 1
    lo, hi = np.zeros((nsets, groups.ngroups), np.int64), np.zeros((nsets, groups.ngroups), np.int64)
    for k in range(nsets):
        sup = member[set_off[k]:set_off[k + 1]].sum(axis=0).astype(np.int64)
        for g in range(groups.ngroups):
            col = sup[dense[:, g]]
            lo[k, g] = col.max() if len(col) else 0
            hi[k, g] = min(col.sum(), set_off[k + 1] - set_off[k])
    return lo, hi


def nonvacuous(member, groups, set_off, gsup):
    """the three conditions of a fixture, on EXPECTED values: some (set, group) strictly below the sum of its datasets' supports
    (a kernel that adds them fails), some strictly above their maximum (one that takes the maximum fails), some dataset in two
    groups with both columns non-zero"""
    dense = groups.dense()
    lo, hi = bounds(member, groups, set_off)
    assert ((lo <= gsup) & (gsup <= hi)).all()
    sums = np.array([member[set_off[k]:set_off[k + 1]].sum(axis=0).astype(np.int64) @ dense for k in range(len(set_off) - 1)])
    assert (gsup < sums).any(), "fixture is vacuous: group support equals the sum of the datasets' supports"
    assert (gsup > lo).any(), "fixture is vacuous: group support equals the maximum of the datasets' supports"
    two = False
    for f in np.flatnonzero(dense.sum(axis=1) >= 2):
        gs = np.flatnonzero(dense[f])
        two |= bool(((gsup[:, gs] > 0).sum(axis=1) >= 2).any())
    assert two, "fixture is vacuous: no dataset in two groups with both columns non-zero"


def three_facets(nfiles, extra_empty=2):
    """labels of a LOLA-like database: a cell type (f mod 3), an antibody (f // 4) and a collection (all but the last two
    datasets); the last dataset has no label at all; extra_empty groups without a dataset are appended.  Returns (off, idx,
    names) for DatasetGroups."""
    number, off, idx = {}, [0], []
    for f in range(nfiles):
        names = [] if f == nfiles - 1 else ["cell%d" % (f % 3), "ab%d" % (f // 4)] + (["coll"] if f < nfiles - 2 else [])
        idx += sorted({number.setdefault(n, len(number)) for n in names})
        off.append(len(idx))
    names = list(number) + ["empty%d" % i for i in range(extra_empty)]
    return np.array(off, np.int32), np.array(idx, np.int32), names
