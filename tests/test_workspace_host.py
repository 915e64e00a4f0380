"""The workspace of the permutation nulls on the host (no GPU): the table builder, igd_hip_workspace_valid, the placement of
igdc_permute_regions_host_ws bit for bit against workspace_ref (numpy, written from the definition in include/igd_hip.h), the
two identities, uniformity, and the three host drivers against "reference lists, then support_host / nearest_sets_host /
jaccard_host".  Refusals leave the caller's arrays as they were."""
import ctypes as C
import os
import random
import shutil

import numpy as np
import pytest

import igd_amd
import permute_ref as PR
import workspace_ref as WR
from helpers import short_tmpdir
from igd_amd import _native as N
from igd_amd.database import IgdError
from test_support_host import FLAT, NEST, clustered_db

BIG = 2 ** 31 - 1
WS = "workspace"


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def same_table(ws, ref):
    assert (ws.nctg, ws.nseg) == (ref["nctg"], ref["nseg"])
    for k in ("w_off", "w_start", "w_len", "w_pre"):
        got = getattr(ws, k)
        assert got.dtype == ref[k].dtype and np.array_equal(got, ref[k]), k


def raw_table(ref):
    """an igd_hip_workspace over the arrays of a reference table (kept alive by the caller)"""
    return N.HipWorkspace(ref["nctg"], ref["nseg"], ref["w_off"].ctypes.data, ref["w_start"].ctypes.data, ref["w_len"].ctypes.data,
                          ref["w_pre"].ctypes.data)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", t)
    os.environ.pop("IGD_HOST_THREADS", None)


# ---- the builder ------------------------------------------------------------------------------------------------------------
def test_builder_equals_the_reference_on_hand_made_segments():
    L = np.array([100, 50, 30, BIG, 0], np.int32)
    rows = [(0, 10, 20), (0, 15, 30), (0, 30, 35), (0, 36, 40), (0, 12, 14),           # overlapping, touching, a gap of 1, nested
            (0, 60, 60), (0, 70, 65), (0, 90, 130), (0, -20, 3), (0, 200, 300),        # empty, inverted, past the end, before 0, beyond
            (0, 50, 54), (0, 80, 84), (0, 44, 48),                                     # ties in length: ordered by start
            (1, 0, 50), (1, 10, 20),                                                   # the whole contig
            (3, 0, BIG),                                                               # 2^31 - 1 bp as one segment (contig 2: none)
            (4, 0, 10), (5, 1, 2), (-1, 1, 2)]                                         # a contig of length 0, unknown contigs
    a = np.array(rows, np.int64)
    ws = igd_amd.build_workspace(a[:, 0], a[:, 1], a[:, 2], L)
    ref = WR.table(a[:, 0], a[:, 1], a[:, 2], L)
    same_table(ws, ref)
    assert ws.w_off.tolist() == [0, 7, 8, 8, 9, 9]
    assert list(zip(ws.w_start[:7].tolist(), ws.w_len[:7].tolist())) == [(10, 25), (90, 10), (36, 4), (44, 4), (50, 4), (80, 4), (0, 3)]
    assert ws.w_start[8] == 0 and ws.w_len[8] == BIG and ws.w_pre[8 + 3 + 1] == BIG
    assert N.cli().igdc_workspace_valid(ws.ptr, ptr(L), len(L)) == 1
    # no segment at all is a table like any other
    e = np.zeros(0, np.int32)
    same_table(igd_amd.build_workspace(e, e, e, L), WR.table(e, e, e, L))
    with pytest.raises(IgdError):
        igd_amd.build_workspace([0], [0], [5], [-1])


@pytest.mark.parametrize("seed", range(4))
def test_builder_equals_the_reference_on_random_segments(seed):
    rng = random.Random(900 + seed)
    L = np.array([rng.choice([1, 2, 50, 1000, 30000]) for _ in range(rng.randint(1, 9))], np.int32)
    seg = WR.random_workspace(rng, L, rng.choice([0, 3, 40, 400]), rng.choice([1, 9, 300]))
    ws = igd_amd.build_workspace(*seg, L)
    same_table(ws, WR.table(*seg, L))
    assert N.cli().igdc_workspace_valid(ws.ptr, ptr(L), len(L)) == 1


def test_valid_refuses_each_way_a_table_can_be_wrong():
    L = np.array([100, 50], np.int32)
    good = WR.table([0, 0, 0, 1], [0, 20, 40, 5], [10, 25, 43, 30], L)
    valid = lambda t, ln=L: N.cli().igdc_workspace_valid(C.byref(raw_table(t)), ptr(ln), len(ln))
    assert valid(good) == 1
    assert good["w_len"].tolist() == [10, 5, 3, 25]

    def broken(key, idx, val, **kw):
        t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        if key:
            t[key][idx] = val
        t.update(kw)
        return t
    bad = [broken("w_off", 0, 1), broken("w_off", 1, 5), broken("w_off", 2, 3), broken("w_off", 1, -1),      # offsets
           broken(None, 0, 0, nseg=5), broken(None, 0, 0, nctg=1),
           broken("w_len", 0, 0), broken("w_len", 2, -3), broken("w_len", 1, 11),                           # lengths >= 1, descending
           broken("w_start", 0, -1), broken("w_start", 0, 91), broken("w_start", 3, 26),                    # on the contig
           broken("w_pre", 0, 1), broken("w_pre", 1, 9), broken("w_pre", 3, 19), broken("w_pre", 4, 1), broken("w_pre", 5, 24)]
    for i, t in enumerate(bad):
        assert valid(t) == 0, i
    assert valid(good, np.array([100, 29], np.int32)) == 0 and valid(good, np.array([100], np.int32)) == 0
    assert N.cli().igdc_workspace_valid(None, ptr(L), 2) == 0
    # the routes refuse such a table, nothing written
    one = (np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones(1, np.int32))
    os_, oe = np.full(3, 0x5a5a5a5a, np.int32), np.full(3, 0x5a5a5a5a, np.int32)
    t = raw_table(bad[8])
    rc = N.cli().igdc_permute_regions_host_ws(ptr(one[0]), ptr(one[1]), ptr(one[2]), 1, ptr(L), 2, 2, 0, 0, 3, ptr(os_), ptr(oe), C.byref(t))
    assert rc == -1 and (os_ == 0x5a5a5a5a).all() and (oe == 0x5a5a5a5a).all()


# ---- the placement ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    ctg_len, seg, reg = WR.segment_cases()
    return dict(ctg_len=ctg_len, seg=seg, reg=reg, tab=WR.table(*seg, ctg_len), ws=igd_amd.build_workspace(*seg, ctg_len))


def test_placement_equals_the_reference_on_every_segment_count(cases):
    ctg_len, reg, tab, ws = cases["ctg_len"], cases["reg"], cases["tab"], cases["ws"]
    same_table(ws, tab)
    assert sorted(set(np.diff(tab["w_off"]).tolist())) == sorted(WR.SEG_COUNTS)
    stuck = WR.unplaceable(*reg, ctg_len, tab)
    assert stuck.any() and not stuck.all()
    for seed, p0, n in ((0, 0, 9), (2 ** 64 - 1, 5, 4), (31337, 2 ** 20 - 2, 2)):
        ws_, we_ = WR.place(*reg, ctg_len, tab, p0, n, seed)
        gs, ge = igd_amd.permute_regions_host(*reg, ctg_len, p0, n, seed, WS, workspace=ws)
        assert gs.dtype == np.int32 and gs.shape == (n, len(reg[1]))
        assert np.array_equal(gs, ws_) and np.array_equal(ge, we_), (seed, p0)
        # a region that fits nowhere, or on an unknown contig, stays; every other one lies inside one segment
        known = (reg[0] >= 0) & (reg[0] < len(ctg_len))
        stay = stuck | ~known
        assert (gs[:, stay] == reg[1][stay]).all() and (ge[:, stay] == reg[2][stay]).all()
        assert WR.inside(reg[0], gs, ge, tab)[:, ~stay].all()
        assert ((ge - gs) == (reg[2] - reg[1])[None, :]).all()
    assert ws.first_unplaceable(*reg) == int(np.flatnonzero(stuck)[0])
    # the longest length has one start per longest segment
    c = len(WR.SEG_COUNTS) + 4                                   # kind "distinct", 63 segments
    kk, F = WR.weights(tab, c, 63)
    assert (kk, int(F[kk])) == (1, 1)
    c = 4                                                        # kind "equal", 63 segments
    kk, F = WR.weights(tab, c, 7)
    assert (kk, int(F[kk])) == (63, 63)


def test_one_segment_per_contig_gives_shuffle(cases):
    from test_permute_host import CTG_LEN, generator_fixture
    ichr, qs, qe = generator_fixture()
    n = len(CTG_LEN)
    full = igd_amd.build_workspace(np.arange(n), np.zeros(n), CTG_LEN, CTG_LEN)
    for seed, p0, k in ((0, 0, 9), (2 ** 64 - 1, 5, 4)):
        a = igd_amd.permute_regions_host(ichr, qs, qe, CTG_LEN, p0, k, seed, WS, workspace=full)
        b = igd_amd.permute_regions_host(ichr, qs, qe, CTG_LEN, p0, k, seed, PR.SHUFFLE)
        w = WR.place(ichr, qs, qe, CTG_LEN, WR.table(np.arange(n), np.zeros(n), CTG_LEN, CTG_LEN), p0, k, seed)
        for x, y, z in zip(a, b, w):
            assert np.array_equal(x, y) and np.array_equal(x, z)
    assert (a[0][:, ichr == 3] != qs[ichr == 3][None, :]).any()


def test_starts_are_uniform_over_two_segments():
    """[0, 3) and [10, 14), len 2: the five starts 0, 1, 10, 11, 12 over 10^5 permutations, each 20 000 +- 760 (six binomial
    standard deviations of sqrt(10^5 x 0.2 x 0.8) = 126); the reference itself stays inside for this seed"""
    L = np.array([20], np.int32)
    seg = ([0, 0], [0, 10], [3, 14])
    ws = igd_amd.build_workspace(*seg, L)
    want = WR.place([0], [5], [7], L, WR.table(*seg, L), 0, 100000, 4)
    got = igd_amd.permute_regions_host([0], [5], [7], L, 0, 100000, 4, WS, workspace=ws)
    for s, e in (want, got):
        cnt = np.bincount(s[:, 0], minlength=20)
        print(cnt.tolist())
        assert set(np.flatnonzero(cnt).tolist()) == {0, 1, 10, 11, 12}
        assert (np.abs(cnt[[0, 1, 10, 11, 12]] - 20000) <= 760).all(), cnt.tolist()
        assert np.array_equal(e, s + 2)
    assert np.array_equal(want[0], got[0])


def test_outside_counts_the_regions_not_inside_one_segment():
    L = np.array([100, 50], np.int32)
    seg = ([0, 0, 1], [10, 40, 0], [20, 60, 50])
    ws = igd_amd.build_workspace(*seg, L)
    reg = (np.array([0, 0, 0, 0, 0, 0, 1, 1, 7, 0], np.int32), np.array([10, 12, 5, 15, 20, 40, 0, 49, 0, 15], np.int32),
           np.array([20, 12, 15, 41, 21, 61, 50, 50, 9, 12], np.int32))
    want = int((~WR.inside(reg[0], reg[1], reg[2], WR.table(*seg, L)) & (reg[0] < 2)).sum())
    assert ws.outside(*reg) == want == 5


# ---- the three drivers --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dbfx():
    d = short_tmpdir("iws")
    rng = random.Random(41)
    nbp = 1 << 12
    db, span = clustered_db(rng, d, "db", nbp, 1, 6, 2, 10)
    ctg_len = np.array([span + 2 * nbp, span + 777], np.int32)
    seg = WR.random_workspace(rng, ctg_len, 60, 2000)
    n = 150
    ichr = np.array([rng.choice([0, 1, 1, -1]) for _ in range(n)], np.int32)
    ln = np.array([rng.choice([0, 1, 50, 300, 700, 1999]) for _ in range(n)], np.int32)
    qs = np.array([rng.randrange(0, 20000) for _ in range(n)], np.int32)
    yield dict(d=d, db=db, ctg_len=ctg_len, seg=seg, tab=WR.table(*seg, ctg_len), ws=igd_amd.build_workspace(*seg, ctg_len), reg=(ichr, qs, qs + ln))
    shutil.rmtree(d, ignore_errors=True)


def lists(fx, nperm, seed):
    return WR.place(*fx["reg"], fx["ctg_len"], fx["tab"], 0, nperm, seed)


@pytest.mark.parametrize("threads", ["1", "2", "7"])
def test_support_driver_equals_its_composition(dbfx, threads, host_threads):
    from test_permute_host import check_result
    ichr, qs, qe = dbfx["reg"]
    host_threads(threads)
    moved = 0
    for nperm, seed, kw in ((1, 0, {}), (7, 3, {}), (5, 9, dict(rule=FLAT, value_filter=300)), (4, 2, dict(rule=NEST, min_overlap=40))):
        ps, pe = lists(dbfx, nperm, seed)
        row = lambda s, e: np.concatenate([(r := igd_amd.support_host(dbfx["db"], ichr, s, e, **kw))[0], [r[1]]]).astype(np.int64)
        obs, rows = row(qs, qe), np.stack([row(ps[p], pe[p]) for p in range(nperm)])
        got = igd_amd.permute_host(dbfx["db"], ichr, qs, qe, dbfx["ctg_len"], nperm, seed, WS, workspace=dbfx["ws"], **kw)
        check_result(got, obs, rows, (nperm, seed, kw))
        moved += int((rows != obs[None, :]).sum())
    assert moved > 0 and obs[:-1].any()


@pytest.mark.parametrize("threads", ["1", "2", "7"])
def test_nearest_driver_equals_its_composition(dbfx, threads, host_threads):
    ichr, qs, qe = dbfx["reg"]
    host_threads(threads)
    off = np.array([0, len(qs)], np.int64)
    for nperm, seed, window, vf in ((1, 0, 0, None), (7, 3, 500, None), (5, 9, 100000, 300)):
        ps, pe = lists(dbfx, nperm, seed)
        rows = [igd_amd.nearest_sets_host(dbfx["db"], ichr, s, e, off, window, vf) for s, e in [(qs, qe)] + [(ps[p], pe[p]) for p in range(nperm)]]
        got = igd_amd.permute_nearest_host(dbfx["db"], ichr, qs, qe, dbfx["ctg_len"], nperm, window, seed, WS, vf, workspace=dbfx["ws"])
        for k in ("n_within", "n_overlap", "sum_dist"):
            assert np.array_equal(getattr(got, k), np.concatenate([getattr(r, k) for r in rows])), (k, nperm, window)
    assert got.n_within.any()


@pytest.mark.parametrize("threads", ["1", "2", "7"])
def test_bp_driver_equals_its_composition(dbfx, threads, host_threads):
    ichr, qs, qe = dbfx["reg"]
    host_threads(threads)
    off = np.array([0, len(qs)], np.int64)
    for nperm, seed, kw in ((1, 0, {}), (7, 3, {}), (5, 9, dict(rule=FLAT, value_filter=300))):
        ps, pe = lists(dbfx, nperm, seed)
        rows = [igd_amd.jaccard_host(dbfx["db"], ichr, s, e, off, **kw) for s, e in [(qs, qe)] + [(ps[p], pe[p]) for p in range(nperm)]]
        got = igd_amd.permute_bp_host(dbfx["db"], ichr, qs, qe, dbfx["ctg_len"], nperm, seed, WS, workspace=dbfx["ws"], **kw)
        assert np.array_equal(got.inter, np.concatenate([r.inter for r in rows]))
        assert np.array_equal(got.set_bp, np.concatenate([r.set_bp for r in rows]))
        assert np.array_equal(got.n_merged, np.concatenate([r.n_merged for r in rows]))
        assert got.n_dropped == int(rows[0].n_dropped[0]) and np.array_equal(got.file_bp, rows[0].file_bp)
    assert got.inter.any() and (got.set_bp[1:] != got.set_bp[0]).any()


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_mode_and_workspace_come_together(dbfx):
    ichr, qs, qe = dbfx["reg"]
    L, ws, db = dbfx["ctg_len"], dbfx["ws"], dbfx["db"]
    for call in (lambda **k: igd_amd.permute_regions_host(ichr, qs, qe, L, 0, 1, **k), lambda **k: igd_amd.permute_host(db, ichr, qs, qe, L, 2, **k),
                 lambda **k: igd_amd.permute_nearest_host(db, ichr, qs, qe, L, 2, 100, **k), lambda **k: igd_amd.permute_bp_host(db, ichr, qs, qe, L, 2, **k)):
        with pytest.raises(ValueError):
            call(mode=WS)
        for mode in ("circular", "shuffle"):
            with pytest.raises(ValueError):
                call(mode=mode, workspace=ws)
        with pytest.raises(ValueError):
            call(mode=WS, workspace=object())


def test_the_old_entries_still_refuse_mode_2_and_the_new_ones_a_mismatch(dbfx):
    L_ = N.cli()
    ichr, qs, qe = (np.ascontiguousarray(x) for x in dbfx["reg"])
    L, ws = dbfx["ctg_len"], dbfx["ws"]
    n = len(qs)
    os_, oe = np.full(n, 0x5a5a5a5a, np.int32), np.full(n, 0x5a5a5a5a, np.int32)
    a = (ptr(ichr), ptr(qs), ptr(qe), n, ptr(L), len(L))
    assert L_.igdc_permute_regions_host(*a, 2, 0, 0, 1, ptr(os_), ptr(oe)) == -1
    assert L_.igdc_permute_regions_host_ws(*a, 2, 0, 0, 1, ptr(os_), ptr(oe), None) == -1
    for mode in (0, 1, 3):
        assert L_.igdc_permute_regions_host_ws(*a, mode, 0, 0, 1, ptr(os_), ptr(oe), ws.ptr) == -1
    assert (os_ == 0x5a5a5a5a).all() and (oe == 0x5a5a5a5a).all()
    assert L_.igdc_permute_regions_host_ws(*a, 2, 0, 0, 1, ptr(os_), ptr(oe), ws.ptr) == 0 and not (os_ == 0x5a5a5a5a).any()


def test_the_drivers_refuse_a_region_that_fits_nowhere_and_write_nothing(dbfx):
    from test_support_host import HostDb
    L_ = N.cli()
    L, ws = dbfx["ctg_len"], dbfx["ws"]
    longest = int(WR.contig(dbfx["tab"], 0)[1][0])
    ichr, qs, qe = np.zeros(3, np.int32), np.array([0, 5, 9], np.int32), np.array([10, 5 + longest + 1, 9], np.int32)
    assert ws.first_unplaceable(ichr, qs, qe) == 1
    # the generic entry passes it through
    gs, ge = igd_amd.permute_regions_host(ichr, qs, qe, L, 0, 2, 0, WS, workspace=ws)
    assert (gs[:, 1] == 5).all() and (ge[:, 1] == 5 + longest + 1).all() and (gs[:, 0] != 0).any()
    H = HostDb(dbfx["db"])
    try:
        nC, R = H.nfiles + 1, 3
        st = [np.full(nC, 0x5a, np.int64) for _ in range(7)]
        mats = [np.full(R * nC, 0x5a, np.int64) for _ in range(3)]
        small = [np.full(R, 0x5a, np.int64), np.full(R, 0x5a, np.int64), np.full(1, 0x5a, np.int64)]
        a = (H.core, H.m, ptr(ichr), ptr(qs), ptr(qe), 3, ptr(L))
        for mode, w in ((2, ws.ptr), (1, ws.ptr), (2, None)):
            assert L_.igdc_permute_host_ws(*a, mode, 0, 2, FLAT_V, NEST, *[ptr(x) for x in st], None, w) == -1
            assert L_.igdc_permute_nearest_host_ws(*a, mode, 0, 2, 100, FLAT_V, *[ptr(x) for x in mats], w) == -1
            assert L_.igdc_permute_bp_host_ws(*a, mode, 0, 2, FLAT_V, NEST, ptr(mats[0]), ptr(small[0]), ptr(small[1]), ptr(small[2]), w) == -1
        for x in st + mats + small:
            assert (x == 0x5a).all()
        # the same call without the long region runs
        assert L_.igdc_permute_host_ws(H.core, H.m, ptr(ichr), ptr(qs), ptr(qs), 3, ptr(L), 2, 0, 2, FLAT_V, NEST, *[ptr(x) for x in st], None, ws.ptr) == 0
        assert not (st[3] == 0x5a).any()
    finally:
        H.close()
    for f in (lambda: igd_amd.permute_host(dbfx["db"], ichr, qs, qe, L, 2, 0, WS, workspace=ws),
              lambda: igd_amd.permute_nearest_host(dbfx["db"], ichr, qs, qe, L, 2, 100, 0, WS, workspace=ws),
              lambda: igd_amd.permute_bp_host(dbfx["db"], ichr, qs, qe, L, 2, 0, WS, workspace=ws)):
        with pytest.raises(IgdError):
            f()


FLAT_V = -2 ** 31                    # IGD_HIP_NO_VALUE_FILTER
