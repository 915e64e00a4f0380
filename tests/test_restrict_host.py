"""Query sets restricted to the universe without a GPU: igdc_restrict_host and igdc_enrich_restricted_host (igd_hostpath.c)
through igd_amd.restrict_host / igd_amd.enrich_restricted_host.

The join is held against restrict_ref.join, a numpy broadcast of the predicate; the gather against sums over the oracle's
per-query membership (test_membership_host.oracle_member: Oracle.search one universe region at a time); all integer outputs
must be EQUAL.  The statistics must be the bits igd_amd.fisher_host returns for the same tables and lie within fisher_ref's
bound of exact arithmetic.  Every fixture's stated conditions are asserted on the expectation, so none is vacuous."""
import os
import shutil

import numpy as np
import pytest

import fisher_ref as FR
import restrict_ref as RR
import sets_fixtures as F
from helpers import Oracle, short_tmpdir
from test_enrich_host import enrich_fixture
from test_membership_host import oracle_member, oracle_member_enum
from test_support_host import FLAT, NEST

CASES = RR.join_cases()


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0].replace(" ", "_") for c in CASES])
def test_join_equals_the_predicate(case):
    import igd_amd
    name, (cat, off), uni, cond = CASES[case]
    R = RR.join(*cat, off, *uni)
    if cond:
        cond(R)
    bits, size = igd_amd.restrict_host(*cat, off, *uni)
    assert bits.dtype == np.uint32 and bits.shape == (len(off) - 1, (len(uni[1]) + 31) // 32) and size.shape == (len(off) - 1,)
    assert np.array_equal(bits, RR.pack(R)), name
    assert np.array_equal(size, R.sum(axis=1)), name


def test_shuffled_universe_comes_back_in_the_callers_order():
    import igd_amd
    (cat, off), uni, _ = RR.order_and_contigs()
    order = np.lexsort((uni[1], uni[0]))
    assert not np.array_equal(order, np.arange(len(order)))
    srt = tuple(a[order] for a in uni)
    unpack = igd_amd.Database.unpack_restricted
    got = unpack(igd_amd.restrict_host(*cat, off, *uni)[0], len(order))
    got_sorted = unpack(igd_amd.restrict_host(*cat, off, *srt)[0], len(order))
    assert got.any() and np.array_equal(got[:, order], got_sorted)


def test_many_regions_with_duplicates():
    import igd_amd
    cat, off, uni = RR.many_regions(n=60000)
    R = RR.join(*cat, off, *uni)
    assert (R.sum(axis=1) > 0).all() and not np.array_equal(R[0], R[1])
    bits, size = igd_amd.restrict_host(*cat, off, *uni)
    assert np.array_equal(bits, RR.pack(R)) and np.array_equal(size, R.sum(axis=1))


def test_refusals_leave_the_callers_arrays_untouched():
    from igd_amd import _native as N
    L = N.cli()
    (cat, off), uni, _ = RR.bit_edges(65)
    bits, size = np.full((4, 3), 0xa5a5a5a5, np.uint32), np.full(4, -5, np.int64)

    def call(o, nu):
        return L.igdc_restrict_host(cat[0].ctypes.data, cat[1].ctypes.data, cat[2].ctypes.data, o.ctypes.data, 4, uni[0].ctypes.data,
                                    uni[1].ctypes.data, uni[2].ctypes.data, nu, bits.ctypes.data, size.ctypes.data)
    for o, nu in ((np.array([1, 2, 2, 3, 4], np.int64), 65), (np.array([0, 3, 2, 3, 4], np.int64), 65), (off, (1 << 31) - 1), (off, -1)):
        assert call(o, nu) != 0 and (bits == 0xa5a5a5a5).all() and (size == -5).all(), (o, nu)
    assert call(off, 65) == 0 and size.tolist() == [2, 0, 65, 2]


@pytest.fixture(scope="module")
def fx():
    """the engineered 6-file database of test_enrich_host: set 1 has regions where the universe has none"""
    d = short_tmpdir("irh")
    path, upath, sets, _ = enrich_fixture(d)
    orc = Oracle(path)
    q = [orc.read_queries(p) for p in sets]
    off = np.zeros(len(q) + 2, np.int64)
    off[1:4] = np.cumsum([len(s[1]) for s in q])
    off[4] = off[3]                                        # a fourth, empty set
    cat = tuple(np.concatenate([s[i] for s in q]).astype(np.int32) for i in range(3))
    u = orc.read_queries(upath)
    yield dict(path=path, orc=orc, cat=cat, off=off, uni=u, R=RR.join(*cat, off, *u))
    orc.close()
    shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("v", [0, 400])
def test_enrichment_restricted_on_the_host_equals_the_definitions(fx, v):
    import igd_amd
    orc, u, R = fx["orc"], fx["uni"], fx["R"]
    nu = len(u[1])
    member, _ = oracle_member(orc, *u, v)
    sup, usup, wnhit, wunhit = RR.gather(R, member)
    size = R.sum(axis=1)
    res, nhit, unhit = igd_amd.enrich_restricted_host(fx["path"], *fx["cat"], fx["off"], *u, v=v, with_nhit=True)
    assert np.array_equal(res.bits, RR.pack(R)) and np.array_equal(res.size, size)
    assert np.array_equal(res.usupport, usup) and np.array_equal(res.support, sup)
    assert np.array_equal(nhit, wnhit) and unhit == wunhit
    b, c, d = RR.tables(sup, usup, size, nu)
    assert (b >= 0).all() and (c >= 0).all() and (d >= 0).all()
    assert np.array_equal(res.b, b) and np.array_equal(res.c, c) and np.array_equal(res.d, d)
    # not vacuous: the restriction changes set 1, a file has support, a file has none, the last set is empty
    nk = np.diff(fx["off"])
    assert size[1] != nk[1] and (sup[0] > 0).any() and (sup[0] == 0).any() and size[3] == 0 and not sup[3].any()
    if v == 0:
        assert res.pvalue_log.max() > 2
    # the statistics: igdc_fisher_host's bits on these tables, within the bound of exact arithmetic
    p, o = igd_amd.fisher_host(sup.ravel(), b.ravel(), c.ravel(), d.ravel())
    assert np.array_equal(p.view(np.int64), res.pvalue_log.ravel().view(np.int64))
    assert np.array_equal(o.view(np.int64), res.odds_ratio.ravel().view(np.int64))
    tabs = [(int(sup[k, f]), int(b[k, f]), int(c[k, f]), int(d[k, f])) for k in range(4) for f in range(sup.shape[1])]
    FR.check(tabs, [FR.exact_plog(*t) for t in tabs], res.pvalue_log.ravel(), res.odds_ratio.ravel(), v)
    assert not res.pvalue_log[3].any() and not np.signbit(res.pvalue_log[3]).any()
    # explicit rules as the command line's dispatch selects them
    rule, vf = (FLAT, v) if v > 0 else (NEST, None)
    res2 = igd_amd.enrich_restricted_host(fx["path"], *fx["cat"], fx["off"], *u, rule=rule, value_filter=vf)
    for x, y in zip(res, res2):
        assert np.array_equal(x, y, equal_nan=True)
    # ranks of a RestrictedEnrichment as of three arrays
    r1, r2 = igd_amd.rank_host(res), igd_amd.rank_host(res.support, res.pvalue_log, res.odds_ratio)
    for x, y in zip(r1, r2):
        assert np.array_equal(x, y)


def test_whole_universe_and_a_set_that_hits_nothing(fx):
    import igd_amd
    u = fx["uni"]
    nu = len(u[1])
    ichr = np.concatenate([u[0], np.array([99, -1], np.int32)])
    qs = np.concatenate([u[1], np.array([0, 0], np.int32)])
    qe = np.concatenate([u[2], np.array([10 ** 6, 10 ** 6], np.int32)])
    res, nhit, unhit = igd_amd.enrich_restricted_host(fx["path"], ichr, qs, qe, np.array([0, nu, nu + 2], np.int64), *u, with_nhit=True)
    assert res.size[0] == nu and np.array_equal(res.support[0], res.usupport) and res.usupport.any()
    assert not res.b[0].any() and np.array_equal(res.c[0], res.size[0] - res.support[0]) and nhit[0] == unhit > 0
    assert res.size[1] == 0 and not res.support[1].any() and nhit[1] == 0 and not res.bits[1].any()
    assert not res.pvalue_log[1].any() and not np.signbit(res.pvalue_log[1]).any()


# ---- the fixtures of tests/test_gpu_restrict_scale.py, proven without a GPU ----------------------------------------------------
SPAN = (1 << 11) * 200                                     # chr1 of enrich_fixture: 200 tiles of 2 048 bp
SEAM_SETS = (5, 6, 11, 100, 700)                           # of scale_b: the whole of chr1 twice, an empty set, two others


def scale_consts():
    """the work decomposition of igd_bits_support, read out of the sources"""
    c = F.consts()
    text = open(os.path.join(F.ENGINE, "restrict_dev.hpp")).read()
    return dict(grid=c["IGD_SETS_GRID"], wg=c["IGD_SETS_WG"], wave=c["IGD_WAVE"], block_words=F._define(text, "IGD_RESTRICT_BLOCK_WORDS"),
                lds_files=F._define(text, "IGD_RESTRICT_LDS_FILES"))


def scale_fixture_a(orc, uni):
    """restrict_ref.scale_a on the 40-file enrich_fixture: the anchors are the universe regions of the first twentieth of
    chr1 that file 0 meets with a value of at least 400 (the oracle, one region at a time)"""
    head = np.flatnonzero((uni[0] == 0) & (uni[1] < SPAN // 20))
    member, _ = oracle_member(orc, uni[0][head], uni[1][head], uni[2][head], 400)
    return RR.scale_a(uni, head[member[:, 0]], scale_consts()["grid"], SPAN)


@pytest.fixture(scope="module")
def fx40():
    """the 40-file database of tests/test_gpu_restrict.py"""
    d = short_tmpdir("irs")
    path, upath, _, _ = enrich_fixture(d, nfiles=40, name="gx")
    orc = Oracle(path)
    yield dict(path=path, orc=orc, uni=orc.read_queries(upath))
    orc.close()
    shutil.rmtree(d, ignore_errors=True)


def hold_host_route(path, cat, off, uni, R, want, v):
    import igd_amd
    sup, usup, wnhit, wunhit = want
    res, nhit, unhit = igd_amd.enrich_restricted_host(path, *cat, off, *uni, v=v, with_nhit=True)
    size = R.sum(axis=1)
    assert np.array_equal(res.bits, RR.pack(R)) and np.array_equal(res.size, size)
    assert np.array_equal(res.usupport, usup) and np.array_equal(res.support, sup)
    assert np.array_equal(nhit, wnhit) and unhit == wunhit
    b, c, d = RR.tables(sup, usup, size, R.shape[1])
    assert (b >= 0).all() and (c >= 0).all() and (d >= 0).all()
    assert np.array_equal(res.b, b) and np.array_equal(res.c, c) and np.array_equal(res.d, d)
    bits, size2 = igd_amd.restrict_host(*cat, off, *uni)
    assert np.array_equal(bits, res.bits) and np.array_equal(size2, size)


@pytest.mark.parametrize("v", [0, 400])
def test_scale_fixture_a_second_items(fx40, v):
    """case A of tests/test_gpu_restrict_scale.py: IGD_SETS_GRID + 300 sets over one block.  The conditions hold on the brute
    force, the two forms of the gather agree, and the host route returns the brute force."""
    k = scale_consts()
    a = scale_fixture_a(fx40["orc"], fx40["uni"])
    assert len(a["off"]) - 1 == k["grid"] + 300 and (len(a["uni"][1]) + 31) // 32 <= k["block_words"]
    n = np.diff(a["off"])
    assert n.max() <= 30 and n[n > 0].min() >= 3
    R = RR.join(*a["cat"], a["off"], *a["uni"])
    member, _ = oracle_member(fx40["orc"], *a["uni"], v)
    want = RR.gather_rows(R, member)
    for x, y in zip(want, RR.gather(R, member)):
        assert np.array_equal(x, y)
    print(RR.second_item_conditions(R, member, want[0], want[1], k["grid"], "A v=%d" % v))
    hold_host_route(fx40["path"], a["cat"], a["off"], a["uni"], R, want, v)


def test_scale_fixture_b_blocks_and_waves(fx40):
    """cases B and C: a universe of three blocks whose last word lies in wave 1, 900 sets, and the five sets of the seam
    child.  The membership is the oracle's enumeration."""
    k = scale_consts()
    b = RR.scale_b(SPAN, k["block_words"])
    uni = b["uni"]
    assert (uni[0] == 1).sum() == 40 and (uni[0] < 0).sum() == 12 and not np.array_equal(np.lexsort((uni[1], uni[0])), np.arange(len(uni[1])))
    R = RR.join(*b["cat"], b["off"], *uni)
    member = oracle_member_enum(fx40["orc"], *uni)
    reach = int(np.concatenate([fx40["uni"][2], [SPAN + 4 * 2048]]).max())
    assert (uni[1] > reach).sum() == 1500 and not member[uni[1] > reach].any() and not member[uni[0] < 0].any()
    want = RR.gather_rows(R, member)
    for x, y in zip(want, RR.gather(R, member)):
        assert np.array_equal(x, y)
    print(RR.block_conditions(R, member, k["grid"], k["block_words"], k["wg"] // k["wave"], "B"))
    print(RR.seam_conditions(R[list(SEAM_SETS)], member, 9001, k["block_words"], "C"))
    hold_host_route(fx40["path"], b["cat"], b["off"], uni, R, want, 0)
