"""GPU: support and enrichment per group of datasets (igd_hip_group_support_sets / igd_sets_group_support<USE_V, OV>,
igd_hip_group_enrich_sets; Database.group_support*, group_enrichment*).

    gsupport[k, g] = the regions of set k that overlap a record of AT LEAST ONE dataset of group g;  gnhit[k] = those that
    overlap a dataset with at least one group

Expected values come from two independent sources (tests/group_support_ref.py): the CPU oracle one region at a time folded into
groups in plain Python, and the unpacked rows of Database.membership (a kernel with tests of its own) folded in numpy.  The
fixtures are checked on the expected values not to be vacuous: a column strictly below the sum and one strictly above the
maximum of its datasets' supports, a dataset in two groups with both columns non-zero.  The shapes are the smallest at which
the kernel can go wrong: one step that meets a group several times, records over four and six tiles, the bitmap's clear
between the regions of one wave, group counts around the bitmap's word and clearing-step edges and at the limit, ragged runs of
the table, two slices of one set, more slices than workgroups, chunk seams with rows that are not nFiles wide."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fisher_ref as R
import group_support_ref as G
import rank_ref as RK
from helpers import ROOT, Oracle, short_tmpdir, write_igd_numpy
from test_database_args_host import BAD, REGIONS, SETS, UNIVERSE
from test_enrich_host import enrich_fixture, tables_from_supports
from sets_fixtures import NBP, wide_db
from test_support_host import FLAT, NEST, NUMPY_DBS, clustered_db, mixed_queries

pytestmark = pytest.mark.gpu
NQ = 600


@pytest.fixture(scope="module")
def fx():
    """the clustered database of 40 files (records over four and six tiles, clusters of one file under one region), 600 regions,
    the oracle's member matrices (computed once, shared, never changed)"""
    from igd_amd import Database
    d = short_tmpdir("igg")
    rng = random.Random(8100)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[2]
    path, span = clustered_db(rng, d, "g40", nbp, gtype, nfiles, nctg, span_tiles)
    ichr, qs, qe = mixed_queries(rng, nctg, nbp, span, NQ)
    orc = Oracle(path)
    member = {0: G.oracle_member(orc, ichr, qs, qe, 0), 500: G.oracle_member(orc, ichr, qs, qe, 500),
              "ov": G.oracle_member_ov(orc, ichr, qs, qe, 150, 0, 250000)}
    orc.close()
    for m in member.values():
        m.setflags(write=False)
    db = Database(path)
    yield dict(d=d, path=path, db=db, nfiles=nfiles, q=(ichr, qs, qe), member=member, off=np.array([0, NQ], np.int64))
    db.close()
    shutil.rmtree(d, ignore_errors=True)


def facets(nfiles):
    from igd_amd import DatasetGroups
    return DatasetGroups(*G.three_facets(nfiles))


def tiled(fx, sizes):
    """sets of the given sizes whose regions repeat the fixture's 600 in order: (ichr, qs, qe, set_off, row numbers)"""
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    rows = np.arange(off[-1]) % NQ
    return tuple(a[rows] for a in fx["q"]) + (off, rows)


def check(fx, groups, sizes, key=0, **kw):
    """group_support_sets on tiled sets against both sources; returns the expected values"""
    db = fx["db"]
    ichr, qs, qe, off, rows = tiled(fx, sizes)
    member = fx["member"][key][rows]
    want, wnhit = G.expected(member, groups, off)
    got, gnhit = db.group_support_sets(ichr, qs, qe, off, groups, **kw)
    assert got.shape == want.shape and got.dtype == np.int64 and gnhit.shape == wnhit.shape
    assert np.array_equal(got, want) and np.array_equal(gnhit, wnhit), (sizes, kw)
    if not kw.get("min_overlap"):
        bits, _, _ = db.membership(ichr, qs, qe, **kw)
        w2, n2 = G.fold(db.unpack_membership(bits, fx["nfiles"]), groups, off)
        assert np.array_equal(w2, want) and np.array_equal(n2, wnhit)
    return member, off, want


@pytest.mark.parametrize("v", [0, 500])
def test_three_facets_across_steps_tiles_and_two_slices_of_one_set(fx, v):
    """sets of 600, 5, 0, 4 097 (two slices of one set: the counters flush twice into one row) and 64 regions; records over four
    and six tiles, so a group met again in a later step or tile still counts 1"""
    g = facets(fx["nfiles"])
    member, off, want = check(fx, g, [600, 5, 0, 4097, 64], key=v, v=v)
    G.nonvacuous(member, g, off, want)
    assert not want[:, -2:].any() and not want[2].any() and want[3].max() > 600


def test_more_slices_than_workgroups(fx):
    """2 100 sets of 3 regions: more slices than persistent workgroups, so a workgroup takes a second slice with the LDS of its
    first to get wrong"""
    g = facets(fx["nfiles"])
    _, _, want = check(fx, g, [3] * 2100)
    assert (want[2048:] > 0).any() and want.max() <= 3


@pytest.fixture(scope="module")
def stacked():
    """40 files on one contig: at P1 the files 0 .. 5 (groups A and B) each have a record -- one region meets six datasets, three
    of one group, within one 128-record step; at P2 only files 3 .. 5 (group B) have one; P3 is empty.  Regions cycle P1, P1, P1,
    P1, P2, P2, P2, P2, P1 .. P3 ..: wave w of a workgroup takes regions w, w + 4, ..: a hit on A and B, then B alone (which the
    clear after the first has to make countable), then A and B again, then nothing."""
    from igd_amd import Database, build_groups
    d = short_tmpdir("igs")
    P1, P2, P3 = 5000, 20000, 40000
    files = []
    for f in range(40):
        rows = [("chr1", 100000 + 50 * f, 100000 + 50 * f + 10, 7)]
        if f < 6:
            rows.append(("chr1", P1 + f, P1 + 300 + f, 600))
        if 3 <= f < 6:
            rows.append(("chr1", P2 + f, P2 + 300 + f, 600))
        files.append(rows)
    path = os.path.join(d, "st.igd")
    write_igd_numpy(path, files, nbp=1 << 14)
    labels = [["A"] if f < 3 else ["B"] if f < 6 else [] for f in range(40)]
    starts = np.array([[P1] * 4 + [P2] * 4 + [P1] * 4 + [P3] * 4] * 9, np.int32).ravel()
    q = (np.zeros(len(starts), np.int32), starts + 100, starts + 200)
    orc = Oracle(path)
    member = G.oracle_member(orc, *q, 0)
    orc.close()
    db = Database(path)
    yield dict(db=db, q=q, member=member, groups=build_groups(labels, 40), off=np.array([0, len(starts)], np.int64))
    db.close()
    shutil.rmtree(d, ignore_errors=True)


def test_one_step_meets_a_group_three_times_and_the_bitmap_is_cleared_between_regions(stacked):
    s = stacked
    want, wnhit = G.expected(s["member"], s["groups"], s["off"])
    n = len(s["q"][1])
    assert want.tolist() == [[n // 2, 3 * n // 4]] and wnhit.tolist() == [3 * n // 4]      # A at P1; B at P1 and P2
    assert s["member"][0].sum() == 6                                                     # six datasets under one region
    got, gnhit = s["db"].group_support_sets(*s["q"], s["off"], s["groups"])
    assert np.array_equal(got, want) and np.array_equal(gnhit, wnhit)


def spread(nfiles, ng):
    """dataset f in group f (ng - 1) // (nfiles - 1) -- the last dataset in the last group -- and every third one also in group
    (7 f) mod ng"""
    from igd_amd import DatasetGroups
    off, idx = [0], []
    for f in range(nfiles):
        gs = {f * (ng - 1) // (nfiles - 1)}
        if f % 3 == 0:
            gs.add((7 * f) % ng)
        idx += sorted(gs)
        off.append(len(idx))
    return DatasetGroups(off, idx, ["g%d" % i for i in range(ng)])


@pytest.mark.parametrize("ng", [1, 31, 32, 33, 64, 65, 2049, 8192])
def test_group_counts_around_the_bitmap_edges_and_at_the_limit(fx, ng):
    """31 / 32 / 33 and 64 / 65 groups: the last bitmap word; 2 049: the first bitmap that needs a second 64-word clearing step;
    8 192: the limit, 36 KiB of LDS"""
    g = spread(fx["nfiles"], ng)
    _, _, want = check(fx, g, [600, 70])
    assert want[0, ng - 1] > 0, "the last group is not hit"


def test_more_groups_than_the_limit_are_refused_before_any_launch(fx):
    from igd_amd import DatasetGroups
    from igd_amd.database import IgdError
    db = fx["db"]
    nf = fx["nfiles"]
    g = DatasetGroups([0] + [1] * nf, [8192], ["g%d" % i for i in range(8193)], check=False)
    out = np.full((1, 8193), -3, np.int64)
    with pytest.raises(IgdError, match="8193 groups given, 1 .. 8192"):
        db.group_support_sets(*fx["q"], fx["off"], g, gsupport=out)
    assert (out == -3).all()
    # the engine names the first bad entry of a grouping it is handed unchecked, and writes nothing
    for off, idx, msg in (([0, 2] + [2] * (nf - 1), [1, 0], r"grp_idx\[1\] = 0 does not ascend"),
                          ([0, 1] + [1] * (nf - 1), [3], r"grp_idx\[0\] = 3 is not in \[0, 3\)"),
                          ([0, 2, 1] + [2] * (nf - 2), [0, 1], r"grp_off\[2\] = 1")):
        out = np.full((1, 3), -3, np.int64)
        with pytest.raises(IgdError, match=msg):
            db.group_support_sets(*fx["q"], fx["off"], DatasetGroups(off, idx, "abc", check=False), gsupport=out)
        assert (out == -3).all()
    with pytest.raises(IgdError, match="set_off decreases"):
        db.group_support_sets(*fx["q"], np.array([0, 400, 300, NQ], np.int64), facets(nf))


def test_fan_out_of_1_2_and_70_groups_with_unlabelled_datasets_and_empty_groups(fx):
    """runs of the table of length 1, 2 and 70 in one wave's step, every other dataset unlabelled, groups 73 .. 79 empty"""
    from igd_amd import DatasetGroups
    nf = fx["nfiles"]
    runs = {3: [72], 17: [0, 71], 29: list(range(1, 71))}
    off, idx = [0], []
    for f in range(nf):
        idx += runs.get(f, [])
        off.append(len(idx))
    g = DatasetGroups(off, idx, ["g%d" % i for i in range(80)])
    member, off, want = check(fx, g, [600])
    sup = member.sum(axis=0)
    assert want[0, 72] == sup[3] and want[0, 0] == sup[17] and want[0, 40] == sup[29] and not want[0, 73:].any()
    assert want[0, 71] == sup[17] and min(sup[3], sup[17], sup[29]) > 0
    assert (member[:, [3, 17, 29]].sum(axis=1) >= 2).any(), "no region meets two of the labelled datasets"


def test_variants_run_all_four_instantiations(fx):
    """USE_V x OV: v = 500, explicit rules, a minimum overlap, and both together"""
    from igd_amd import MinOverlap
    db, nf = fx["db"], fx["nfiles"]
    g = facets(nf)
    mo = MinOverlap(150, 0, 250000)
    check(fx, g, [600], key=500, v=500)                                                   # <true, false>
    member, off, want = check(fx, g, [600, 70], key="ov", min_overlap=mo)                 # <false, true>
    G.nonvacuous(member, g, off, want)
    assert member.sum() < fx["member"][0][np.arange(670) % NQ].sum()
    for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300), (NEST, 300)):
        bits, _, _ = db.membership(*fx["q"], rule=rule, value_filter=vf)
        w, n = G.fold(db.unpack_membership(bits, nf), g, fx["off"])
        got, gn = db.group_support_sets(*fx["q"], fx["off"], g, rule=rule, value_filter=vf)
        assert np.array_equal(got, w) and np.array_equal(gn, n), (rule, vf)
    # <true, true>: the member matrix from igd_sets_support_ov with every region a set of its own
    single = np.arange(NQ + 1, dtype=np.int64)
    rows, _ = db.support_sets(*fx["q"], single, v=500, min_overlap=mo)
    w, n = G.fold(rows > 0, g, fx["off"])
    assert 0 < (rows > 0).sum() < fx["member"][500].sum()
    got, gn = db.group_support_sets(*fx["q"], fx["off"], g, v=500, min_overlap=mo)
    assert np.array_equal(got, w) and np.array_equal(gn, n)
    one, n1 = db.group_support(*fx["q"], g, v=500, min_overlap=mo)
    assert np.array_equal(one, w[0]) and n1 == n[0]


def test_identity_equals_support_sets_and_one_group_equals_nhit(fx):
    from igd_amd import build_groups
    db, nf = fx["db"], fx["nfiles"]
    ichr, qs, qe, off, _ = tiled(fx, [600, 5, 4097, 64])
    for kw in (dict(), dict(v=500)):
        sup, nhit = db.support_sets(ichr, qs, qe, off, **kw)
        got, gn = db.group_support_sets(ichr, qs, qe, off, build_groups([["f%d" % f] for f in range(nf)], nf), **kw)
        assert np.array_equal(got, sup) and np.array_equal(gn, nhit)
        got, gn = db.group_support_sets(ichr, qs, qe, off, build_groups([["all"]] * nf, nf), **kw)
        assert np.array_equal(got[:, 0], nhit) and np.array_equal(gn, nhit) and nhit.min() > 0
    # added to the caller's rows
    g = facets(nf)
    base = np.arange(4 * g.ngroups, dtype=np.int64).reshape(4, g.ngroups)
    first, _ = db.group_support_sets(ichr, qs, qe, off, g)
    got, _ = db.group_support_sets(ichr, qs, qe, off, g, gsupport=base.copy())
    assert np.array_equal(got, base + first)


SEAM = r"""
import random, sys
sys.path[:0] = [%r, %r]
import numpy as np
import group_support_ref as G
from helpers import Oracle, short_tmpdir
from igd_amd import Database
from test_gpu_group_support import spread
from test_support_host import NUMPY_DBS, clustered_db, mixed_queries
import shutil
d = short_tmpdir("igm")
try:
    rng = random.Random(8300)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[2]
    path, span = clustered_db(rng, d, "m40", nbp, gtype, nfiles, nctg, span_tiles)
    q = mixed_queries(rng, nctg, nbp, span, 520)
    off = np.array([0, 150, 155, 155, 455, 519, 520], np.int64)
    orc = Oracle(path)
    member = G.oracle_member(orc, *q, 0)
    orc.close()
    db = Database(path)
    for ng in (33, 7):
        g = spread(nfiles, ng)
        want, wnhit = G.expected(member, g, off)
        assert want[3].any() and want[0].any() and want[5].sum() >= 0
        got, gnhit = db.group_support_sets(*q, off, g)
        assert np.array_equal(got, want) and np.array_equal(gnhit, wnhit), ng
    db.close()
finally:
    shutil.rmtree(d, ignore_errors=True)
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "97"}, {"IGD_HIP_SETS_ROW_BYTES": "600"},
                                 {"IGD_HIP_MAX_BATCH": "97", "IGD_HIP_SETS_ROW_BYTES": "600"}])
def test_calls_straddle_the_chunk_seams(env):
    """chunks of 97 regions (the sets of 150 and 300 are cut by a chunk and their rows folded from two and four chunks) and of
    two rows of 33 x 8 bytes (ten of 7 x 8) within 600 bytes; 33 and 7 columns against 40 files, so a driver that still strides
    by nFiles writes the wrong cells.  The variables are read once per process: a child process each."""
    p = subprocess.run([sys.executable, "-c", SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env), timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def test_group_enrichment_tables_statistics_and_ranks():
    """group_enrichment_files: support, usupport, b, c, d, clamped equal integers formed in numpy from group supports that come
    from the oracle; pvalue_log / odds_ratio within the bound tests/test_gpu_enrich.py holds the dataset table to (fisher_ref.check);
    enrichment_ranks on the result against rank_ref"""
    from igd_amd import Database
    d = short_tmpdir("ign")
    try:
        path, upath, sets, _ = enrich_fixture(d, nfiles=12, name="gn")
        orc, db = Oracle(path), Database(path)
        try:
            g = facets(12)
            uni = orc.read_queries(upath)
            q = [orc.read_queries(p) for p in sets]
            nu = len(uni[1])
            for v in (0, 400):
                um = G.oracle_member(orc, *uni, v)
                usup = G.expected(um, g, np.array([0, nu], np.int64))[0][0]
                res, gnhit, gunhit = db.group_enrichment_sets(*[np.concatenate([s[i] for s in q]) for i in range(3)],
                                                              np.cumsum([0] + [len(s[1]) for s in q]), *uni, g, v=v, with_nhit=True)
                files = db.group_enrichment_files(sets, upath, g, v)
                for x, y in zip(res, files):
                    assert np.array_equal(x, y, equal_nan=True)
                assert np.array_equal(res.usupport, usup) and gunhit == G.fold(um, g, np.array([0, nu]))[1][0]
                for k, (ichr, qs, qe) in enumerate(q):
                    m = G.oracle_member(orc, ichr, qs, qe, v)
                    off = np.array([0, len(qs)], np.int64)
                    sup, nh = G.expected(m, g, off)
                    if v == 0 and k == 0:
                        G.nonvacuous(m, g, off, sup)
                    b, c, dd, clamped = tables_from_supports(sup[0], usup, len(qs), nu)
                    assert np.array_equal(res.support[k], sup[0]) and gnhit[k] == nh[0]
                    assert np.array_equal(res.b[k], b) and np.array_equal(res.c[k], c) and np.array_equal(res.d[k], dd)
                    assert res.clamped[k] == clamped
                    tabs = [(int(sup[0][j]), int(b[j]), int(c[j]), int(dd[j])) for j in range(g.ngroups)]
                    R.check(tabs, [R.exact_plog(*t) for t in tabs], res.pvalue_log[k], res.odds_ratio[k], ("groups", v, k))
                assert res.support.shape == (3, g.ngroups) and res.pvalue_log.max() > 2
                ranks = db.enrichment_ranks(res)
                RK.check(res.support, res.pvalue_log, res.odds_ratio, ranks, RK.reference(res.support, res.pvalue_log, res.odds_ratio),
                         ("group ranks", v))
        finally:
            db.close()
            orc.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


# ---- the arguments: the one checker's refusals under the entry's name, as tests/test_gpu_database_args.py holds the others ----
ENTRIES = {
    "group_support_sets": ("group_support_sets", {**REGIONS, **SETS}, ("qe", "sets", "min_overlap")),
    "group_support": ("group_support_sets", {**REGIONS}, ("qe", "min_overlap")),
    "group_enrichment_sets": ("group_enrichment_sets", {**REGIONS, **SETS, **UNIVERSE}, ("qe", "sets", "universe", "min_overlap")),
}
ARG_CASES = [(name, case, over, text) for name, (_, _, feats) in ENTRIES.items() for f in feats for case, over, text in BAD[f]]


@pytest.fixture(scope="module")
def tiny():
    from igd_amd import Database, build_groups
    d = short_tmpdir("iga")
    path, span, _, _ = wide_db(random.Random(4100), d, "tiny", 3, NBP, 4)
    assert span > max(REGIONS["qe"])
    with Database(path) as handle:
        yield handle, build_groups([["a"], ["a", "b"], []], 3)
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("name,case,over,text", ARG_CASES, ids=["%s-%s" % c[:2] for c in ARG_CASES])
def test_one_bad_argument_is_refused_under_the_entrys_name(tiny, name, case, over, text):
    from igd_amd.database import IgdError
    db, g = tiny
    prefix, kw, _ = ENTRIES[name]
    texts = []
    for _ in range(2):
        with pytest.raises(IgdError) as e:
            getattr(db, name)(**{**kw, **over}, groups=g)
        texts.append(str(e.value))
    assert texts[0].startswith(prefix + ": ") and text in texts[0] and texts[0] == texts[1], texts
    getattr(db, name)(**kw, groups=g)                              # and the handle serves the next good call
    with pytest.raises(IgdError, match="%s: groups must be a DatasetGroups" % prefix):
        getattr(db, name)(**kw, groups=[["a"]] * 3)


def test_a_callers_gsupport_array(tiny):
    from igd_amd.database import IgdError
    db, g = tiny
    text = "group_support_sets: gsupport must be a C-ordered int64[2, 2]"
    for arr in (np.zeros((2, 2), np.int32), np.zeros((2, 2, 1), np.int64), np.asfortranarray(np.zeros((2, 2), np.int64))):
        with pytest.raises(IgdError) as e:
            db.group_support_sets(**REGIONS, **SETS, groups=g, gsupport=arr)
        assert str(e.value) == text


def test_no_regions_and_no_sets(tiny):
    """nsets = 0, sets without regions and no regions at all: shapes and zeros, and the handle serves the next call"""
    db, g = tiny
    none = np.zeros(0, np.int32)
    sup, nhit = db.group_support_sets(none, none, none, [0], g)
    assert sup.shape == (0, 2) and nhit.shape == (0,)
    sup, nhit = db.group_support_sets(none, none, none, [0, 0, 0], g)
    assert sup.shape == (2, 2) and not sup.any() and nhit.tolist() == [0, 0]
    sup, nhit = db.group_support(none, none, none, g)
    assert sup.shape == (2,) and not sup.any() and nhit == 0
    res = db.group_enrichment_sets(none, none, none, [0], **UNIVERSE, groups=g)
    assert res.support.shape == (0, 2) and res.usupport.shape == (2,) and res.clamped.shape == (0,)
    res = db.group_enrichment_sets(**REGIONS, **SETS, u_ichr=none, u_qs=none, u_qe=none, groups=g)
    assert res.support.shape == (2, 2) and not res.usupport.any()
    sup, _ = db.group_support_sets(**REGIONS, set_off=[0, 0, 3, 3], groups=g)
    assert not sup[0].any() and not sup[2].any() and np.array_equal(sup[1], db.group_support(**REGIONS, groups=g)[0])


def test_files_and_the_engine_route_of_the_command_line_equal_the_host_goldens():
    """group_support_files / read_groups on the golden family, and `-K -u`, `-K -U -R` on the engine route (limit 0): -u the host
    golden's bytes; -U -R its lines with integers, names and ranks exact and the %.4f fields within the bound
    tests/test_gpu_enrich.py holds the two routes to (they may round a printed tie differently)"""
    import test_group_cli_host as K
    from igd_amd import Database
    from test_support_host import _run
    ENGINE = {"IGD_HOST_MAX_QUERIES": "0"}
    with Database(K.DB) as db:
        g = db.read_groups(K.GROUPS)
        assert g.names == K.groups_of().names and g.idx.tolist() == K.groups_of().idx.tolist()
        f00 = os.path.join(os.path.dirname(K.DB), "beds", "f00.bed")
        sup, nhit = db.group_support_files([K.Q, f00], g)
        res = db.group_enrichment_files([K.Q], K.UNIVERSE, g)
    golden = open(os.path.join(K.DIR, "K_u.txt"), newline="").read()
    rows = {int(l.split("\t")[0]): int(l.split("\t")[2]) for l in golden.splitlines()[1:-1]}
    assert sup.shape == (2, g.ngroups) and {i: int(x) for i, x in enumerate(sup[0]) if x > 0} == rows
    assert golden.splitlines()[-1] == "Query regions with a hit: %d of 80" % nhit[0] and sup[1].any()
    ur = open(os.path.join(K.DIR, "K_U_R.txt"), newline="").read()
    assert [int(l.split("\t")[2]) for l in ur.splitlines()[1:-1]] == [int(x) for x in res.support[0] if x > 0]
    for v, name in (([], "K_u.txt"), (["-v", "500"], "K_u_v500.txt")):
        got = _run(["search", K.DB, "-q", K.Q, "-u", "-K", K.GROUPS] + v, ENGINE)
        assert got.returncode == 0, got.stderr
        assert got.stdout.decode() == open(os.path.join(K.DIR, name), newline="").read()
    got = _run(["search", K.DB, "-q", K.Q, "-U", K.UNIVERSE, "-R", "-K", K.GROUPS], ENGINE)
    assert got.returncode == 0, got.stderr
    K.same_table(got.stdout.decode(), ur, "engine -U -R -K")
