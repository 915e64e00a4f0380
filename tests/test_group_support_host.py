"""Support per group of datasets without a GPU: igdc_group_support_host_ov (igd_hostpath.c) through igd_amd.group_support_host,
and the grouping itself (DatasetGroups, build_groups, Database.read_groups' parser).

    gsupport[g] = the query regions that overlap a record of AT LEAST ONE dataset of group g     (a union over the datasets)
    gnhit       = the query regions that overlap a dataset with at least one group

Expected values never come from the code under test.  Two independent sources (tests/group_support_ref.py): the CPU oracle one
region at a time, folded into groups in plain Python, and the unpacked rows of igdc_membership_host (held against the oracle by
tests/test_membership_host.py) folded in numpy.  Every fixture is checked, on the expected values, not to be vacuous: a group
column strictly below the sum and one strictly above the maximum of its datasets' supports, and a dataset in two groups with
both columns non-zero."""
import ctypes as C
import os
import random
import shutil

import numpy as np
import pytest

import group_support_ref as G
from helpers import Oracle, short_tmpdir
from test_support_host import FLAT, NEST, NOV, NUMPY_DBS, HostDb, cli_rule, clustered_db, mixed_queries, sparse_db

NQ = 600


@pytest.fixture(scope="module")
def tmp():
    d = short_tmpdir("igk")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", t)
    os.environ.pop("IGD_HOST_THREADS", None)


def facets(nfiles):
    from igd_amd import DatasetGroups
    return DatasetGroups(*G.three_facets(nfiles))


def member_host(path, ichr, qs, qe, v, rule):
    """bool[nq, nfiles] from igdc_membership_host"""
    H = HostDb(path)
    try:
        nW = (H.nfiles + 31) // 32
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        bits = np.zeros((len(qs), nW), np.uint32)
        nhit = C.c_int64(0)
        assert H.L.igdc_membership_host(H.core, H.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), v, rule,
                                        bits.ctypes.data, None, C.byref(nhit)) == 0
        return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :H.nfiles].astype(bool)
    finally:
        H.close()


@pytest.fixture(scope="module")
def dbs(tmp):
    """the clustered databases of tests/test_support_host.py, their regions and the oracle's member matrices for v = 0 and 500"""
    out = []
    for case, (nbp, gtype, nfiles, nctg, span_tiles) in enumerate(NUMPY_DBS):
        rng = random.Random(7100 + case)
        path, span = clustered_db(rng, tmp, "k%d" % case, nbp, gtype, nfiles, nctg, span_tiles)
        ichr, qs, qe = mixed_queries(rng, nctg, nbp, span, NQ)
        orc = Oracle(path)
        try:
            member = {v: G.oracle_member(orc, ichr, qs, qe, v) for v in (0, 500)}
            member["ov"] = G.oracle_member_ov(orc, ichr, qs, qe, 150, 0, 250000)
        finally:
            orc.close()
        out.append(dict(path=path, gtype=gtype, nfiles=nfiles, q=(ichr, qs, qe), member=member, off=np.array([0, NQ], np.int64)))
    return out


@pytest.mark.parametrize("v", [0, 500])
@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_equals_the_oracle_fold_and_the_membership_fold(case, v, dbs, host_threads):
    import igd_amd
    d = dbs[case]
    g = facets(d["nfiles"])
    want, wnhit = G.expected(d["member"][v], g, d["off"])
    G.nonvacuous(d["member"][v], g, d["off"], want)
    rule, ev = cli_rule(d["gtype"], v)
    w2, n2 = G.fold(member_host(d["path"], *d["q"], ev, rule), g, d["off"])
    assert np.array_equal(w2, want) and np.array_equal(n2, wnhit)
    assert not want[0, -2:].any(), "the empty groups have zero columns"
    for threads in ("1", "3"):
        host_threads(threads)
        got, nhit = igd_amd.group_support_host(d["path"], *d["q"], g, v)
        assert got.dtype == np.int64 and np.array_equal(got, want[0]) and nhit == wnhit[0], (case, v, threads)
    # two identical query lines count twice: mixed_queries repeats every fifth region
    ichr, qs, qe = d["q"]
    got2, nhit2 = igd_amd.group_support_host(d["path"], np.tile(ichr, 2), np.tile(qs, 2), np.tile(qe, 2), g, v)
    assert np.array_equal(got2, 2 * want[0]) and nhit2 == 2 * wnhit[0]


@pytest.mark.parametrize("case", [0, 2])
def test_host_explicit_rules_and_a_minimum_overlap(case, dbs):
    import igd_amd
    d = dbs[case]
    g = facets(d["nfiles"])
    for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300), (NEST, 300)):
        hv = NOV if (vf is None or d["gtype"] == 0) else vf
        want, wnhit = G.fold(member_host(d["path"], *d["q"], hv, rule), g, d["off"])
        got, nhit = igd_amd.group_support_host(d["path"], *d["q"], g, rule=rule, value_filter=vf)
        assert np.array_equal(got, want[0]) and nhit == wnhit[0], (rule, vf)
    # 150 bp and a quarter of the record: fewer pairs than the plain predicate, from the oracle's enumeration
    m = d["member"]["ov"]
    assert m.sum() < d["member"][0].sum() and m.any()
    want, wnhit = G.expected(m, g, d["off"])
    G.nonvacuous(m, g, d["off"], want)
    got, nhit = igd_amd.group_support_host(d["path"], *d["q"], g, min_overlap=igd_amd.MinOverlap(150, 0, 250000))
    assert np.array_equal(got, want[0]) and nhit == wnhit[0]
    with pytest.raises(igd_amd.database.IgdError):
        igd_amd.group_support_host(d["path"], *d["q"], g, min_overlap=igd_amd.MinOverlap(-1, 0, 0))


def test_rules_differ_on_a_sparse_database(tmp):
    import igd_amd
    rng = random.Random(7200)
    path, span, nbp = sparse_db(rng, tmp, "ksp")
    ichr, qs, qe = mixed_queries(rng, 2, nbp, span, 1200)
    off = np.array([0, len(qs)], np.int64)
    g = igd_amd.build_groups([["a", "b"], ["a"], ["b", "c"], []], 4)
    orc = Oracle(path)
    try:
        nest = G.expected(G.oracle_member(orc, ichr, qs, qe, 0), g, off)
        flat = G.expected(G.oracle_member(orc, ichr, qs, qe, 1), g, off)      # values >= 1: rule FLAT, every record passes
    finally:
        orc.close()
    assert not np.array_equal(nest[0], flat[0]), "the two rules do not differ on this fixture"
    for rule, want in ((NEST, nest), (FLAT, flat)):
        got, nhit = igd_amd.group_support_host(path, ichr, qs, qe, g, rule=rule)
        assert np.array_equal(got, want[0][0]) and nhit == want[1][0]


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_identity_one_group_and_the_inequalities(case, dbs):
    import igd_amd
    d = dbs[case]
    nf = d["nfiles"]
    sup, nhit = igd_amd.support_host(d["path"], *d["q"])
    assert np.array_equal(sup, d["member"][0].sum(axis=0))
    ident = igd_amd.build_groups([["f%d" % f] for f in range(nf)], nf)
    got, gn = igd_amd.group_support_host(d["path"], *d["q"], ident)
    assert np.array_equal(got, sup) and gn == nhit
    one = igd_amd.build_groups([["all"]] * nf, nf)
    got, gn = igd_amd.group_support_host(d["path"], *d["q"], one)
    assert got.shape == (1,) and got[0] == nhit and gn == nhit
    g = facets(nf)
    got, gn = igd_amd.group_support_host(d["path"], *d["q"], g)
    lo, hi = G.bounds(d["member"][0], g, d["off"])
    assert ((lo[0] <= got) & (got <= hi[0])).all() and gn <= nhit
    # an unlabelled dataset changes nothing: the last dataset, labelled or not, leaves every other column as it is
    lab = g.labels()
    lab[-1] = ["only_the_last"]
    g2 = igd_amd.build_groups(lab, nf)
    got2, _ = igd_amd.group_support_host(d["path"], *d["q"], g2)
    for name in g.names:
        if name in g2.names:
            assert got2[g2.names.index(name)] == got[g.names.index(name)]
    assert got2[g2.names.index("only_the_last")] == sup[-1]


def test_groupings_round_trip(tmp):
    import igd_amd
    from igd_amd.database import read_groups_file
    names = ["a.bed.gz", "b.bed.gz", "7", "c.bed.gz", "d.bed.gz"]
    labels = [["liver", "CTCF"], [], ["CTCF", "liver", "CTCF"], ["k562"], ["liver"]]
    g = igd_amd.build_groups(labels, 5)
    assert g.names == ["liver", "CTCF", "k562"] and g.nfiles == 5 and g.ngroups == 3
    assert g.off.tolist() == [0, 2, 2, 4, 5, 6] and g.idx.tolist() == [0, 1, 0, 1, 2, 0]
    assert g.labels() == [["liver", "CTCF"], [], ["liver", "CTCF"], ["k562"], ["liver"]]
    assert g.n_datasets.tolist() == [3, 2, 1] and g.dense().sum() == 6
    g2 = igd_amd.build_groups({0: ["liver", "CTCF"], 2: ["CTCF", "liver"], 3: ["k562"], 4: ["liver"]}, 5)
    assert g2.off.tolist() == g.off.tolist() and g2.idx.tolist() == g.idx.tolist() and g2.names == g.names
    again = igd_amd.DatasetGroups(g.off, g.idx, g.names)
    assert again.labels() == g.labels()
    # the file: names exactly as the index lists them or decimal numbers, `#` and blank lines, CRLF, a dataset on several lines;
    # "7" is a NAME here (dataset 2), "4" a number
    p = os.path.join(tmp, "groups.tsv")
    with open(p, "w") as fh:
        fh.write("# dataset\tgroup\n\na.bed.gz\tliver\r\na.bed.gz\tCTCF\n7\tCTCF\n2\tliver\n   \nc.bed.gz\tk562\n4\tliver\n7\tCTCF\n")
    r = read_groups_file(p, names)
    assert r.names == g.names and r.off.tolist() == g.off.tolist() and r.idx.tolist() == g.idx.tolist()
    # group names may hold blanks and tabs after the first tab
    with open(p, "w") as fh:
        fh.write("0\tcell type\tA\n1\tcell type\tA\n")
    assert read_groups_file(p, names).names == ["cell type\tA"]


def test_refused_groupings(tmp, dbs):
    import igd_amd
    from igd_amd.database import GROUP_MAX, IgdError, read_groups_file
    DG = igd_amd.DatasetGroups
    with pytest.raises(IgdError, match=r"idx\[1\] = 0 does not ascend"):
        DG([0, 2, 3], [1, 0, 2], ["a", "b", "c"])                      # unsorted run
    with pytest.raises(IgdError, match=r"idx\[1\] = 1 does not ascend"):
        DG([0, 2, 3], [1, 1, 2], ["a", "b", "c"])                      # a duplicate
    DG([0, 2, 3], [1, 2, 0], ["a", "b", "c"])                          # (descending across two runs is fine)
    with pytest.raises(IgdError, match=r"idx\[2\] = 3 is not in \[0, 3\)"):
        DG([0, 2, 3], [0, 1, 3], ["a", "b", "c"])
    with pytest.raises(IgdError, match=r"idx\[0\] = -1 is not in"):
        DG([0, 1], [-1], ["a"])
    with pytest.raises(IgdError, match=r"off\[2\] = 1"):
        DG([0, 2, 1], [0, 1], ["a", "b"])
    with pytest.raises(IgdError, match=r"off\[0\] = 1"):
        DG([1, 2], [0, 0], ["a"])
    with pytest.raises(IgdError, match="%d groups given, 1 .. %d" % (GROUP_MAX + 1, GROUP_MAX)):
        DG([0, 1], [0], ["g%d" % i for i in range(GROUP_MAX + 1)])
    with pytest.raises(IgdError, match="0 groups given"):
        DG([0, 0], [], [])
    DG([0, 1], [GROUP_MAX - 1], ["g%d" % i for i in range(GROUP_MAX)])  # the limit itself
    with pytest.raises(IgdError, match="8193 groups"):
        igd_amd.build_groups([["g%d" % i for i in range(GROUP_MAX + 1)]], 1)
    with pytest.raises(IgdError, match="labels for 2 datasets given, the database has 3"):
        igd_amd.build_groups([["a"], ["b"]], 3)
    with pytest.raises(IgdError, match="dataset 3 is not in"):
        igd_amd.build_groups({3: ["a"]}, 3)
    names = ["a.bed", "b.bed"]
    p = os.path.join(tmp, "bad.tsv")
    for text, msg in (("a.bed\tx\nc.bed\ty\n", "line 2: the database has no dataset c.bed"), ("a.bed\tx\n2\ty\n", "line 2: the database has no dataset 2"),
                      ("# only\n\n", "no group given"), ("a.bed\tx\n\nb.bed\n", "line 3: not a dataset, a tab and a group"),
                      ("".join("a.bed\tg%d\n" % i for i in range(GROUP_MAX + 1)), "line %d: more than %d groups" % (GROUP_MAX + 1, GROUP_MAX))):
        with open(p, "w") as fh:
            fh.write(text)
        with pytest.raises(IgdError, match=msg):
            read_groups_file(p, names)
    # the C entry makes the same checks itself: a grouping built without them is refused and nothing is written
    d = dbs[0]
    nf = d["nfiles"]
    H = HostDb(d["path"])
    try:
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in d["q"])
        for off, idx, ng in (([0] + [2] * nf, [1, 0], 3), ([0] + [1] * nf, [3], 3), ([0] + [1] * nf, [0], GROUP_MAX + 1),
                             ([0] + [1] * nf, [0], 0), ([0, 2, 1] + [2] * (nf - 2), [0, 1], 3)):
            off, idx = np.array(off, np.int32), np.array(idx, np.int32)
            sup, nhit = np.full(max(ng, 1), -7, np.int64), C.c_int64(-7)
            rc = H.L.igdc_group_support_host_ov(H.core, H.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), off.ctypes.data,
                                                idx.ctypes.data, ng, NOV, NEST, sup.ctypes.data, C.byref(nhit), None)
            assert rc == -1 and (sup == -7).all() and nhit.value == -7, (off, idx, ng)
    finally:
        H.close()
    with pytest.raises(IgdError, match="the grouping is of 3 datasets, the database has %d" % nf):
        igd_amd.group_support_host(d["path"], *d["q"], igd_amd.build_groups([["a"]] * 3, 3))
    with pytest.raises(IgdError, match="groups must be a DatasetGroups"):
        igd_amd.group_support_host(d["path"], *d["q"], [["a"]] * nf)


def test_counts_are_added_to_the_callers(dbs):
    d = dbs[1]
    g = facets(d["nfiles"])
    want, wnhit = G.expected(d["member"][0], g, d["off"])
    H = HostDb(d["path"])
    try:
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in d["q"])
        sup, nhit = np.arange(g.ngroups, dtype=np.int64) * 100, C.c_int64(11)
        a = (H.core, H.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), g.off.ctypes.data, g.idx.ctypes.data, g.ngroups, NOV, NEST)
        assert H.L.igdc_group_support_host_ov(*a, sup.ctypes.data, C.byref(nhit), None) == 0
        assert np.array_equal(sup, np.arange(g.ngroups) * 100 + want[0]) and nhit.value == 11 + wnhit[0]
        assert H.L.igdc_group_support_host_ov(*a, sup.ctypes.data, None, None) == 0           # gnhit may be NULL
        assert np.array_equal(sup, np.arange(g.ngroups) * 100 + 2 * want[0])
    finally:
        H.close()
