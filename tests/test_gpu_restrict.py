"""GPU: query sets restricted to the universe (igd_hip_restrict_sets = igd_restrict_bits + igd_member_popc;
igd_hip_enrich_restricted = the join + igd_hip_membership_dev over the universe + igd_bits_support + igd_fisher_cells;
Database.restrict_sets / enrichment_restricted / enrichment_restricted_files, `igd search -U -X` on the engine route).

The join is held against restrict_ref.join, a numpy broadcast of the predicate; the gather against sums over the rows of
Database.unpack_membership(Database.membership(universe)); all integer outputs must be EQUAL.  The statistics must be the
bits that enrichment_sets returns for R_k given as explicit region lists -- the same tables through the same kernel -- and
lie within fisher_ref's bound of exact arithmetic."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fisher_ref as FR
import rank_ref as KR
import restrict_ref as RR
import sets_fixtures as F
from helpers import ROOT, Oracle, short_tmpdir
from test_enrich_host import enrich_fixture
from test_sets_cli import _write_list
from test_support_host import FLAT, HOST, NEST, NOV, _run

pytestmark = pytest.mark.gpu
ENGINE = {"IGD_HOST_MAX_QUERIES": "0"}
NFILES = 40
HEADER = "index\t number of regions\t support\t b\t c\t d\t oddsRatio\t pValueLog\t File_name"
MODES = {"nest": dict(rule=NEST), "flat": dict(rule=FLAT), "v400": dict(v=400)}


def lds_files():
    return F._define(open(os.path.join(F.ENGINE, "restrict_dev.hpp")).read(), "IGD_RESTRICT_LDS_FILES")


@pytest.fixture(scope="module")
def fx():
    """the 40-file enrichment fixture (gType 1): a universe of a few thousand regions, three sets of which the second has
    regions where the universe has none, and a fourth, empty one"""
    from igd_amd import Database
    d = short_tmpdir("igx")
    path, upath, sets, uni = enrich_fixture(d, nfiles=NFILES, name="gx")
    empty = os.path.join(d, "gx_empty.bed")
    open(empty, "w").close()
    files = [sets[0], sets[1], empty, sets[2]]
    orc, db = Oracle(path), Database(path)
    assert db.gtype == 1 and db.nfiles == NFILES
    q = [orc.read_queries(p) for p in files]
    off = np.zeros(len(q) + 1, np.int64)
    off[1:] = np.cumsum([len(s[1]) for s in q])
    cat = tuple(np.concatenate([s[i] for s in q]).astype(np.int32) for i in range(3))
    u = orc.read_queries(upath)
    assert 2000 < len(u[1]) < 10000
    R = RR.join(*cat, off, *u)
    assert (R.sum(axis=1)[[0, 1, 3]] > 0).all() and not R[2].any()
    yield dict(d=d, path=path, upath=upath, files=files, db=db, cat=cat, off=off, uni=u, R=R, member={})
    db.close()
    orc.close()
    shutil.rmtree(d, ignore_errors=True)


def member_of(fx, mode):
    """the universe's membership matrix under the mode's rule and filter (computed once)"""
    if mode not in fx["member"]:
        bits, _, _ = fx["db"].membership(*fx["uni"], **MODES[mode])
        fx["member"][mode] = fx["db"].unpack_membership(bits, NFILES)
    return fx["member"][mode]


def check_restricted(db, res, nhit, unhit, R, member, nu, what, gather=RR.gather):
    """every integer output against the brute force, exactly"""
    sup, usup, wnhit, wunhit = gather(R, member)
    size = R.sum(axis=1)
    print(what, "size", size.tolist(), "support max", int(sup.max(initial=0)), "nhit", wnhit.tolist(), "unhit", wunhit)
    assert np.array_equal(res.bits, RR.pack(R)), what
    assert np.array_equal(res.size, size), what
    assert np.array_equal(res.usupport, usup) and np.array_equal(res.support, sup), what
    assert np.array_equal(nhit, wnhit) and unhit == wunhit, what
    b, c, d = RR.tables(sup, usup, size, nu)
    assert (b >= 0).all() and (c >= 0).all() and (d >= 0).all(), what
    assert np.array_equal(res.b, b) and np.array_equal(res.c, c) and np.array_equal(res.d, d), what
    assert np.array_equal(db.unpack_restricted(res.bits, nu), R), what


def check_equivalence(db, res, R, uni, what, **kw):
    """R_k as explicit region lists through enrichment_sets: the same supports and tables, nothing clamped, the same bits"""
    cat, off = RR.explicit_lists(R, *uni)
    ex = db.enrichment_sets(*cat, off, *uni, **kw)
    assert np.array_equal(ex.support, res.support) and np.array_equal(ex.usupport, res.usupport), what
    assert np.array_equal(ex.b, res.b) and np.array_equal(ex.c, res.c) and np.array_equal(ex.d, res.d), what
    assert not ex.clamped.any(), what
    assert np.array_equal(ex.pvalue_log.view(np.int64), res.pvalue_log.view(np.int64)), what
    assert np.array_equal(ex.odds_ratio.view(np.int64), res.odds_ratio.view(np.int64)), what


# ---- the join ----------------------------------------------------------------------------------------------------------------
CASES = RR.join_cases()


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0].replace(" ", "_") for c in CASES])
def test_join_equals_the_predicate(fx, case):
    """bit edges (nu = 1 .. 2 049: bits >= nu zero, two sets in one universe word, the row stride, an empty set between two
    others), order and contigs, the prefix maximum, touching / empty / inverted regions, no set, no universe"""
    name, (cat, off), uni, cond = CASES[case]
    R = RR.join(*cat, off, *uni)
    if cond:
        cond(R)
    bits, size = fx["db"].restrict_sets(*cat, off, *uni)
    assert bits.dtype == np.uint32 and bits.shape == (len(off) - 1, (len(uni[1]) + 31) // 32) and size.shape == (len(off) - 1,)
    assert np.array_equal(bits, RR.pack(R)), name
    assert np.array_equal(size, R.sum(axis=1)), name


def test_shuffled_universe_comes_back_in_the_callers_order(fx):
    (cat, off), uni, _ = RR.order_and_contigs()
    db = fx["db"]
    order = np.lexsort((uni[1], uni[0]))
    assert not np.array_equal(order, np.arange(len(order)))
    srt = tuple(a[order] for a in uni)
    got = db.unpack_restricted(db.restrict_sets(*cat, off, *uni)[0], len(order))
    got_sorted = db.unpack_restricted(db.restrict_sets(*cat, off, *srt)[0], len(order))
    assert got.any() and np.array_equal(got[:, order], got_sorted)


def test_lanes_take_second_regions(fx):
    """600 000 set regions in 3 sets over a universe of 5 000: more than the 2 048 x 256 lanes of the capped grid"""
    from igd_amd import _native as N
    c = F.consts()
    cat, off, uni = RR.many_regions()
    grid = int(N.hip().igd_hip_restrict_grid(len(cat[1])))
    assert grid == c["IGD_SETS_GRID"] == int(N.hip().igd_hip_restrict_grid(1 << 40)) and len(cat[1]) > grid * c["IGD_SETS_WG"]
    R = RR.join(*cat, off, *uni)
    beyond = np.arange(len(cat[1])) >= grid * c["IGD_SETS_WG"]
    only_late = RR.join(cat[0][beyond], cat[1][beyond], cat[2][beyond], np.array([0, int(beyond.sum())], np.int64), *uni)
    assert only_late.any() and (R.sum(axis=1) > 0).all() and not np.array_equal(R[0], R[1])
    bits, size = fx["db"].restrict_sets(*cat, off, *uni)
    assert np.array_equal(bits, RR.pack(R)) and np.array_equal(size, R.sum(axis=1))


# ---- the enrichment ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_enrichment_restricted_equals_the_definitions_and_enrichment_sets_on_explicit_lists(fx, mode):
    db, kw = fx["db"], MODES[mode]
    res, nhit, unhit = db.enrichment_restricted(*fx["cat"], fx["off"], *fx["uni"], with_nhit=True, **kw)
    nu = len(fx["uni"][1])
    check_restricted(db, res, nhit, unhit, fx["R"], member_of(fx, mode), nu, mode)
    check_equivalence(db, res, fx["R"], fx["uni"], mode, **kw)
    if mode == "v400":
        res2 = db.enrichment_restricted(*fx["cat"], fx["off"], *fx["uni"], rule=FLAT, value_filter=400)
        for x, y in zip(res, res2):
            assert np.array_equal(x, y, equal_nan=True)
        assert not np.array_equal(member_of(fx, "v400"), member_of(fx, "flat"))
    if mode == "nest":
        # not vacuous: set 1 has regions where the universe has none (the unrestricted table clamps there), enrichment shows
        nk = np.diff(fx["off"])
        assert (res.size != nk).any() and res.pvalue_log.max() > 2 and (res.support[2] == 0).all() and res.size[2] == 0
        assert db.enrichment_sets(*fx["cat"], fx["off"], *fx["uni"], **kw).clamped.sum() > 0
        tabs = [(int(res.support[k, f]), int(res.b[k, f]), int(res.c[k, f]), int(res.d[k, f])) for k in (0, 1) for f in range(NFILES)]
        want = [FR.exact_plog(*t) for t in tabs]
        worst = FR.check(tabs, want, res.pvalue_log[:2].ravel(), res.odds_ratio[:2].ravel(), mode)
        print("worst |x - y| / bound = %.3g" % worst)
        # ranks of the restricted table: the engine's equal the host's
        got, host = db.enrichment_ranks(res), __import__("igd_amd").rank_host(res)
        for name in ("rnk_sup", "rnk_pv", "rnk_or", "max_rnk"):
            assert np.array_equal(getattr(got, name), getattr(host, name)), name
        assert np.array_equal(got.mean_rnk, host.mean_rnk)
        assert (np.abs(got.qvalue_log - host.qvalue_log) <= KR.tol(host.qvalue_log)).all()


def test_whole_universe_and_a_set_that_hits_nothing(fx):
    db, u = fx["db"], fx["uni"]
    nu = len(u[1])
    ichr = np.concatenate([u[0], np.array([99, -1], np.int32)])
    qs = np.concatenate([u[1], np.array([0, 0], np.int32)])
    qe = np.concatenate([u[2], np.array([10 ** 6, 10 ** 6], np.int32)])
    off = np.array([0, nu, nu + 2], np.int64)
    res, nhit, unhit = db.enrichment_restricted(ichr, qs, qe, off, *u, with_nhit=True)
    assert res.size[0] == nu and np.array_equal(res.support[0], res.usupport) and res.usupport.any()
    assert not res.b[0].any() and np.array_equal(res.c[0], res.size[0] - res.support[0]) and nhit[0] == unhit > 0
    assert res.size[1] == 0 and not res.support[1].any() and nhit[1] == 0 and not res.bits[1].any()
    assert not res.pvalue_log[1].any() and not np.signbit(res.pvalue_log[1]).any()                  # +0.0
    assert not res.pvalue_log[0].any()                                                               # a == lo: p = 1


@pytest.mark.parametrize("nfiles", [1, 31, 32, 33, 2081, 8192, 8193])
def test_file_counts(nfiles):
    """rows of 1 .. 257 words: 2 081 files are 66 words, so a lane takes a second word; 8 192 files are the last LDS form
    (IGD_RESTRICT_LDS_FILES), 8 193 the first wide one.  (40 files: every other test of this file.)"""
    from igd_amd import Database
    assert lds_files() == 8192
    d = short_tmpdir("igf")
    try:
        path, span, window, edge = F.wide_db(random.Random(8100 + nfiles), d, "r%d" % nfiles, nfiles, F.NBP, max(40, nfiles * 3 // 10))
        uni, _ = F.make_sets(np.random.default_rng(nfiles), 1, F.NBP, span, [330], window)
        nu = len(uni[1])
        rs = np.random.default_rng(nfiles + 1)
        pick = rs.permutation(nu)[:120]
        lists = [[(int(uni[0][i]), int(uni[1][i]), int(uni[2][i])) for i in pick],
                 [(0, window[0], window[1])], [(0, 0, span // 3), (0, span // 2, span // 2 + 5 * F.NBP)], []]
        cat, off = RR.sets_of(lists)
        R = RR.join(*cat, off, *uni)
        db = Database(path)
        try:
            member = db.unpack_membership(db.membership(*uni)[0], nfiles)
            assert member[:, edge].any(axis=0).all() and R[:3].any(axis=1).all() and (uni[0] < 0).any()
            res, nhit, unhit = db.enrichment_restricted(*cat, off, *uni, with_nhit=True)
            check_restricted(db, res, nhit, unhit, R, member, nu, nfiles)
            assert res.support[:, edge].any(axis=0).all(), "a boundary file has no support in any set"
            check_equivalence(db, res, R, uni, nfiles)
        finally:
            db.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


# ---- seams: the budgets are read once per process, so a child process crosses them -----------------------------------------------
CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from igd_amd import Database
z = np.load(sys.argv[3])
db = Database(sys.argv[2])
res, nhit, unhit = db.enrichment_restricted(z["ichr"], z["qs"], z["qe"], z["off"], z["uc"], z["us"], z["ue"], with_nhit=True)
bits, size = db.restrict_sets(z["ichr"], z["qs"], z["qe"], z["off"], z["uc"], z["us"], z["ue"])
np.savez(sys.argv[4], nhit=nhit, unhit=unhit, bits2=bits, size2=size, **res._asdict())
db.close()
"""


@pytest.mark.parametrize("env", [dict(IGD_HIP_MEMBER_ROW_BYTES="8000", IGD_HIP_RESTRICT_ROW_BYTES="700"), dict(IGD_HIP_MAX_BATCH="50")],
                         ids=["row_budgets", "max_batch"])
def test_chunk_seams(fx, env):
    """IGD_HIP_MEMBER_ROW_BYTES = 8 000: rows of 2 words, 1 000 universe regions per membership chunk -- at least 3 chunks whose
    ends are no multiples of 32 -- and IGD_HIP_RESTRICT_ROW_BYTES = 700: 2 sets per set chunk, 2 chunks.  IGD_HIP_MAX_BATCH =
    50: a set's regions reach the join in several batches, the universe in chunks of 50."""
    db, u, R = fx["db"], fx["uni"], fx["R"]
    nu = len(u[1])
    step = 1000 if "IGD_HIP_MEMBER_ROW_BYTES" in env else 50
    with_members = [bool(R[3, a:a + step].any()) for a in range(0, nu, step)]
    assert nu > 2 * step and (all(with_members) if step == 1000 else sum(with_members) >= 3), "set 3 does not span the universe chunks"
    want, wnhit, wunhit = db.enrichment_restricted(*fx["cat"], fx["off"], *u, with_nhit=True)
    check_restricted(db, want, wnhit, wunhit, R, member_of(fx, "nest"), nu, "parent")
    inp, out = os.path.join(fx["d"], "seam_in.npz"), os.path.join(fx["d"], "seam_out.npz")
    np.savez(inp, ichr=fx["cat"][0], qs=fx["cat"][1], qe=fx["cat"][2], off=fx["off"], uc=u[0], us=u[1], ue=u[2])
    e = dict(os.environ)
    e.update(env)
    got = subprocess.run([sys.executable, "-c", CHILD, ROOT, fx["path"], inp, out], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300)
    assert got.returncode == 0, got.stderr.decode()
    z = np.load(out)
    for name in want._fields:
        assert np.array_equal(z[name], getattr(want, name), equal_nan=True), name
    assert np.array_equal(z["nhit"], wnhit) and int(z["unhit"]) == wunhit
    assert np.array_equal(z["bits2"], want.bits) and np.array_equal(z["size2"], want.size)


# ---- defined, not added ------------------------------------------------------------------------------------------------------
def test_outputs_are_defined_and_refusals_leave_the_callers_arrays_untouched(fx):
    from igd_amd import _native as N
    db, u = fx["db"], fx["uni"]
    first = db.enrichment_restricted(*fx["cat"], fx["off"], *u)
    a, b = int(fx["off"][3]), int(fx["off"][4])
    other = db.enrichment_restricted(fx["cat"][0][a:b], fx["cat"][1][a:b], fx["cat"][2][a:b], np.array([0, b - a], np.int64), *u)
    assert np.array_equal(other.support[0], first.support[3]) and np.array_equal(other.bits[0], first.bits[3])
    again = db.enrichment_restricted(*fx["cat"], fx["off"], *u)
    for x, y in zip(first, again):
        assert np.array_equal(x, y, equal_nan=True)
    none = db.enrichment_restricted(u[0][:0], u[1][:0], u[2][:0], np.zeros(1, np.int64), *u)
    assert none.support.shape == (0, NFILES) and np.array_equal(none.usupport, first.usupport)
    H = N.hip()
    ichr, qs, qe = fx["cat"]
    nu, nUW = len(u[1]), (len(u[1]) + 31) // 32
    sup, usup, size = np.full((4, NFILES), -5, np.int64), np.full(NFILES, -5, np.int64), np.full(4, -5, np.int64)
    p, o, nh, unh = np.full((4, NFILES), -5.0), np.full((4, NFILES), -5.0), np.full(4, -5, np.int64), np.full(1, -5, np.int64)
    bits = np.full((4, nUW), 0xa5a5a5a5, np.uint32)

    def untouched():
        return ((sup == -5).all() and (usup == -5).all() and (size == -5).all() and (p == -5.0).all() and (o == -5.0).all() and
                (nh == -5).all() and (unh == -5).all() and (bits == 0xa5a5a5a5).all())
    good = fx["off"]
    for off, rule in ((np.array([1, 2, 3, 4, len(qs)], np.int64), NEST), (np.array([0, 50, 20, 60, len(qs)], np.int64), NEST), (good, 7)):
        rc = H.igd_hip_enrich_restricted(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, off.ctypes.data, 4, u[0].ctypes.data,
                                         u[1].ctypes.data, u[2].ctypes.data, nu, NOV, rule, sup.ctypes.data, usup.ctypes.data,
                                         size.ctypes.data, p.ctypes.data, o.ctypes.data, bits.ctypes.data, nh.ctypes.data, unh.ctypes.data)
        assert rc != 0 and untouched(), (off, rule)
        if rule == NEST:
            rc = H.igd_hip_restrict_sets(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, off.ctypes.data, 4, u[0].ctypes.data,
                                         u[1].ctypes.data, u[2].ctypes.data, nu, bits.ctypes.data, size.ctypes.data)
            assert rc != 0 and untouched(), off
    rc = H.igd_hip_restrict_sets(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, good.ctypes.data, 4, u[0].ctypes.data,
                                 u[1].ctypes.data, u[2].ctypes.data, (1 << 31) - 1, bits.ctypes.data, size.ctypes.data)
    assert rc != 0 and untouched()


# ---- the command line -----------------------------------------------------------------------------------------------------------
def _blocks(text, ranked):
    """[(title, rows, last line)]"""
    out, title, cur = [], None, None
    for line in text.splitlines():
        if line.startswith("Query set "):
            title = line
        elif line.startswith(HEADER):
            assert (line != HEADER) == ranked
            cur = []
        elif line.startswith("Restricted regions with a hit:") or line.startswith("Query regions with a hit:"):
            out.append((title, cur, line))
            title, cur = None, None
        else:
            cur.append(line.split("\t"))
    return out


@pytest.mark.parametrize("ranks", [[], ["-R"]], ids=["plain", "R"])
def test_engine_route_of_the_command_line_prints_the_host_routes_table(fx, ranks):
    path, upath, files, db = fx["path"], fx["upath"], fx["files"], fx["db"]
    lst = _write_list(fx["d"], files)
    res, nhit, unhit = db.enrichment_restricted(*fx["cat"], fx["off"], *fx["uni"], with_nhit=True)
    for args in (["-Q", lst, "-U", upath, "-X"] + ranks, ["-X", "-q", files[1], "-U", upath] + ranks):
        host = _run(["search", path] + args, HOST)
        eng = _run(["search", path] + args, ENGINE)
        assert host.returncode == 0 and eng.returncode == 0, (host.stderr, eng.stderr)
        Hb, Eb = _blocks(host.stdout.decode(), bool(ranks)), _blocks(eng.stdout.decode(), bool(ranks))
        assert len(Hb) == len(Eb) == (4 if args[0] == "-Q" else 1)
        for n, ((ht, hrows, hlast), (et, erows, elast)) in enumerate(zip(Hb, Eb)):
            k = n if args[0] == "-Q" else 1
            assert ht == et and hlast == elast and len(hrows) == len(erows)
            assert elast == "Restricted regions with a hit: %d of %d (from %d query regions); universe regions: %d" % (
                nhit[k], res.size[k], fx["off"][k + 1] - fx["off"][k], len(fx["uni"][1]))
            assert [int(r[0]) for r in erows] == [f for f in range(NFILES) if res.support[k, f] > 0]
            for h, e in zip(hrows, erows):
                f = int(e[0])
                assert h[:6] == e[:6] and h[8] == e[8] and len(e) == (15 if ranks else 9)
                assert [int(x) for x in e[2:6]] == [res.support[k, f], res.b[k, f], res.c[k, f], res.d[k, f]]
                assert abs(float(e[7]) - res.pvalue_log[k, f]) <= 5.01e-5
                for j in (6, 7) + ((13, 14) if ranks else ()):          # %.4f / %.2f fields: the routes may round a tie differently
                    assert h[j] == e[j] or abs(float(h[j]) - float(e[j])) <= 1.01e-4, (h, e)
                if ranks:
                    assert h[9:13] == e[9:13]
    # without -X the engine route prints what it printed: the unrestricted table with its clamp count
    plain_h = _run(["search", path, "-Q", lst, "-U", upath] + ranks, HOST).stdout.decode()
    plain_e = _run(["search", path, "-Q", lst, "-U", upath] + ranks, ENGINE).stdout.decode()
    assert "clamped cells: " in plain_e and "Restricted" not in plain_e
    assert [l.split("\t")[:6] for l in plain_h.splitlines()] == [l.split("\t")[:6] for l in plain_e.splitlines()]
