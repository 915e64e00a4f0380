"""The support of a region set under rigid shifts on the host: igd_amd.shift_regions_host (igdc_shift_regions_host),
igd_amd.shift_support_host (igdc_shift_support_host_ov), shift_offsets and local_zscore.

Expected values never come from the code under test: shift_ref (a numpy restatement of THE SHIFT of include/igd_hip.h) moves the
regions, and igd_amd.support_host -- held against the oracle in tests/test_support_host.py -- counts every moved set.  Every
integer must be EQUAL."""
import random
import shutil

import numpy as np
import pytest

import permute_ref as PR
import shift_ref as SR
from helpers import short_tmpdir
from test_support_host import FLAT, NEST, clustered_db

L = 1000
CTG_LEN = np.array([L, 1, 50], np.int32)
OFFSETS = np.array([-2 ** 30, -L, -6, -1, 0, 1, 6, L, 2 ** 30], np.int32)


def generator_fixture():
    """(ichr, qs, qe): a region at its contig's start, one ending at L, one with len == L, a zero-length region at 0 and one at
    L, a region on contig -1 and one on contig nctg, every region of a contig of length 1, two in the middle of a contig"""
    reg = [(0, 0, 10), (0, L - 10, L), (0, 0, L), (0, 0, 0), (0, L, L), (-1, 5, 9), (len(CTG_LEN), 5, 9),
           (1, 0, 1), (1, 0, 0), (1, 1, 1), (0, 500, 520), (2, 3, 47), (0, 3, 4), (0, L - 7, L - 2)]
    c, s, e = (np.array(x, np.int32) for x in zip(*reg))
    return c, s, e


def test_the_reference_itself_on_hand_computed_regions():
    c, s, e = generator_fixture()
    ws, we = SR.shift(c, s, e, CTG_LEN, OFFSETS)
    col = lambda i: list(zip(ws[:, i].tolist(), we[:, i].tolist()))
    assert col(0) == [(0, 10), (0, 10), (0, 10), (0, 10), (0, 10), (1, 11), (6, 16), (990, 1000), (990, 1000)]
    assert col(1) == [(0, 10), (0, 10), (984, 994), (989, 999), (990, 1000), (990, 1000), (990, 1000), (990, 1000), (990, 1000)]
    assert col(2) == [(0, L)] * 9 and col(3) == [(0, 0)] * 5 + [(1, 1), (6, 6), (L, L), (L, L)]
    assert col(4) == [(0, 0), (0, 0), (994, 994), (999, 999)] + [(L, L)] * 5
    assert col(5) == [(5, 9)] * 9 and col(6) == [(5, 9)] * 9 and col(7) == [(0, 1)] * 9
    assert col(8) == [(0, 0)] * 5 + [(1, 1)] * 4 and col(9) == [(0, 0)] * 4 + [(1, 1)] * 5


def test_shift_regions_host_equals_the_reference():
    import igd_amd
    c, s, e = generator_fixture()
    ws, we = SR.shift(c, s, e, CTG_LEN, OFFSETS)
    gs, ge = igd_amd.shift_regions_host(c, s, e, CTG_LEN, OFFSETS)
    assert gs.dtype == np.int32 and gs.shape == (len(OFFSETS), len(s))
    assert np.array_equal(gs, ws) and np.array_equal(ge, we)
    # any order, repeats, one offset, no region
    o = np.array([6, 6, -1, 2 ** 30, 0], np.int32)
    gs, ge = igd_amd.shift_regions_host(c, s, e, CTG_LEN, o)
    assert np.array_equal(gs, SR.shift(c, s, e, CTG_LEN, o)[0]) and np.array_equal(gs[0], gs[1]) and np.array_equal(gs[4], s)
    assert igd_amd.shift_regions_host(c[:0], s[:0], e[:0], CTG_LEN, [5])[0].shape == (1, 0)
    # an invalid region on a known contig passes through the generic entry
    gs, ge = igd_amd.shift_regions_host([0, 0], [10, 990], [5, 1001], CTG_LEN, [7])
    assert gs.tolist() == [[10, 990]] and ge.tolist() == [[5, 1001]]


def test_shift_regions_host_refusals():
    import igd_amd
    from igd_amd.database import IgdError
    c, s, e = generator_fixture()
    for bad, text in (([], "0 shifts, not 1 .. 4096"), (list(range(4097)), "4097 shifts"), ([0, 2 ** 30 + 1], "offset 1 = 1073741825 is beyond"),
                      ([-2 ** 30 - 1], "offset 0 = -1073741825"), ([2 ** 32], "offset 0 = 4294967296"), ([0.5], "whole numbers")):
        with pytest.raises(IgdError, match="shift_regions_host: .*" + text):
            igd_amd.shift_regions_host(c, s, e, CTG_LEN, bad)
    with pytest.raises(IgdError, match="shift_regions_host: 3 / 3 / 2 regions given"):
        igd_amd.shift_regions_host([0, 0, 0], [1, 2, 3], [1, 2], CTG_LEN, [0])
    assert igd_amd.shift_regions_host(c, s, e, CTG_LEN, list(range(4096)))[0].shape == (4096, len(s))


# ---- igdc_shift_support_host_ov -------------------------------------------------------------------------------------------------
STEP = 37
SUP_OFFSETS = np.array([-2 ** 30, -4000, -STEP, 0, STEP, 4000, 2 ** 30, 0, STEP], np.int32)


def support_fixture(d, nregions=200, seed=9100):
    """a fuzzed clustered database of 40 files on 3 contigs, contig lengths well inside the records' span (so that a region pushed
    back against its contig's end still meets records), and regions on them (some on unknown contigs)"""
    rng = random.Random(seed)
    path, span = clustered_db(rng, d, "sh", 1 << 12, 1, 40, 3, 12)
    ctg_len = np.array([span // 2, span // 2 + 1234, span // 3], np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, nregions)
    return dict(path=path, ctg_len=ctg_len, reg=(ichr, qs, qe))


@pytest.fixture(scope="module")
def sfx():
    d = short_tmpdir("ish")
    yield support_fixture(d)
    shutil.rmtree(d, ignore_errors=True)


def reference_rows(path, ichr, qs, qe, ctg_len, offsets, clamp=True, **kw):
    """int64[nshift, nfiles + 1] from igd_amd.support_host on shift_ref's explicit lists"""
    import igd_amd
    ws, we = SR.shift(ichr, qs, qe, ctg_len, offsets, clamp=clamp)
    rows = []
    for j in range(len(offsets)):
        sup, nhit = igd_amd.support_host(path, ichr, ws[j], we[j], **kw)
        rows.append(np.concatenate([sup, [nhit]]))
    return np.array(rows, np.int64)


def test_the_fixture_can_tell_a_generator_that_ignores_d_or_forgets_the_clamp(sfx):
    ichr, qs, qe = sfx["reg"]
    want = reference_rows(sfx["path"], ichr, qs, qe, sfx["ctg_len"], SUP_OFFSETS)
    z = list(SUP_OFFSETS).index(0)
    # a dataset whose support differs between shift 0 and shift +-step
    assert (want[z, :-1] != want[z + 1, :-1]).any() and (want[z, :-1] != want[z - 1, :-1]).any()
    # a region whose clamped position changes a count: moved by 4000 without the clamps, the rows are different
    o = np.array([4000], np.int32)
    free_s, free_e = SR.shift(ichr, qs, qe, sfx["ctg_len"], o, clamp=False)
    assert free_e.max() < 2 ** 31 and (free_e[0] > sfx["ctg_len"][np.clip(ichr, 0, 2)])[(ichr >= 0) & (ichr < 3)].any()
    import igd_amd
    sup, nhit = igd_amd.support_host(sfx["path"], ichr, free_s[0].astype(np.int32), free_e[0].astype(np.int32))
    assert (np.concatenate([sup, [nhit]]) != want[5]).any()
    # at +-2^30 every region on a known contig stands against an end, and still meets records
    assert want[0, :-1].any() and want[6, :-1].any()


@pytest.mark.parametrize("kw", [dict(), dict(v=500), dict(min_overlap=40), dict(min_overlap="query"), dict(min_overlap="record"),
                                dict(rule=FLAT, value_filter=300), dict(rule=NEST)])
def test_shift_support_host_rows_equal_support_host_of_each_shifted_set(sfx, kw):
    import igd_amd
    from igd_amd import MinOverlap
    if kw.get("min_overlap") == "query":
        kw = dict(min_overlap=MinOverlap.from_fractions(query=0.5))
    elif kw.get("min_overlap") == "record":
        kw = dict(v=500, min_overlap=MinOverlap.from_fractions(bp=3, record=0.25))
    ichr, qs, qe = sfx["reg"]
    want = reference_rows(sfx["path"], ichr, qs, qe, sfx["ctg_len"], SUP_OFFSETS, **kw)
    ss = igd_amd.shift_support_host(sfx["path"], ichr, qs, qe, sfx["ctg_len"], SUP_OFFSETS, **kw)
    assert ss.shifted.dtype == np.int64 and ss.shifted.shape == want.shape and np.array_equal(ss.offsets, SUP_OFFSETS)
    assert np.array_equal(ss.shifted, want), kw
    assert want[:, :-1].any()
    # the offset-0 row is support_host of the set as given; equal offsets give equal rows
    sup, nhit = igd_amd.support_host(sfx["path"], ichr, qs, qe, **kw)
    assert np.array_equal(ss.shifted[3, :-1], sup) and ss.shifted[3, -1] == nhit
    assert np.array_equal(ss.shifted[3], ss.shifted[7]) and np.array_equal(ss.shifted[4], ss.shifted[8])


def test_threads_one_shift_no_region_and_unknown_contigs(sfx, monkeypatch):
    import igd_amd
    ichr, qs, qe = sfx["reg"]
    one = igd_amd.shift_support_host(sfx["path"], ichr, qs, qe, sfx["ctg_len"], SUP_OFFSETS).shifted
    for t in ("1", "3"):
        monkeypatch.setenv("IGD_HOST_THREADS", t)
        assert np.array_equal(igd_amd.shift_support_host(sfx["path"], ichr, qs, qe, sfx["ctg_len"], SUP_OFFSETS).shifted, one)
    monkeypatch.delenv("IGD_HOST_THREADS")
    assert np.array_equal(igd_amd.shift_support_host(sfx["path"], ichr, qs, qe, sfx["ctg_len"], [STEP]).shifted, one[4:5])
    e = np.zeros(0, np.int32)
    assert not igd_amd.shift_support_host(sfx["path"], e, e, e, sfx["ctg_len"], [0, 5]).shifted.any()
    u = igd_amd.shift_support_host(sfx["path"], [-1, 3, 99], [0, 5, 7], [100, 50, 70000], sfx["ctg_len"], [0, 5, -5]).shifted
    assert u.shape == (3, 41) and not u.any()


def test_one_region_and_fewer_shifts_than_threads(sfx, monkeypatch):
    """one region under every offset; one shift of 4600 regions on three threads: 4600 region rows are worth three threads, and
    only one row is there to share out"""
    import igd_amd
    monkeypatch.setenv("IGD_HOST_THREADS", "3")
    ichr, qs, qe = sfx["reg"]
    k = int(np.flatnonzero((ichr >= 0) & (ichr < 3))[0])
    for c, s, e, offs in ((ichr[k:k + 1], qs[k:k + 1], qe[k:k + 1], SUP_OFFSETS), (np.tile(ichr, 23), np.tile(qs, 23), np.tile(qe, 23), [STEP])):
        want = reference_rows(sfx["path"], c, s, e, sfx["ctg_len"], np.asarray(offs, np.int32))
        got = igd_amd.shift_support_host(sfx["path"], c, s, e, sfx["ctg_len"], offs).shifted
        assert got.shape == want.shape and np.array_equal(got, want) and want.any()


def test_shift_support_host_refuses_what_the_engine_refuses(sfx):
    import igd_amd
    from igd_amd.database import IgdError
    ichr, qs, qe = sfx["reg"]
    L0 = int(sfx["ctg_len"][0])
    with pytest.raises(IgdError, match="shift_support_host: a refused argument"):
        igd_amd.shift_support_host(sfx["path"], [0], [L0 - 5], [L0 + 1], sfx["ctg_len"], [0])
    with pytest.raises(IgdError, match="shift_support_host: a refused argument"):
        igd_amd.shift_support_host(sfx["path"], [0], [9], [5], sfx["ctg_len"], [0])
    with pytest.raises(IgdError, match="shift_support_host: ctg_len has 2 entries, the database 3 contigs"):
        igd_amd.shift_support_host(sfx["path"], ichr, qs, qe, sfx["ctg_len"][:2], [0])
    with pytest.raises(IgdError, match="shift_support_host: 0 shifts"):
        igd_amd.shift_support_host(sfx["path"], ichr, qs, qe, sfx["ctg_len"], [])
    with pytest.raises(IgdError, match="shift_support_host: offset 1 = -1073741825 is beyond"):
        igd_amd.shift_support_host(sfx["path"], ichr, qs, qe, sfx["ctg_len"], [0, -2 ** 30 - 1])
    with pytest.raises(IgdError, match="shift_support_host: 3 / 3 / 2 regions given"):
        igd_amd.shift_support_host(sfx["path"], [0, 0, 0], [1, 2, 3], [1, 2], sfx["ctg_len"], [0])


# ---- shift_offsets, local_zscore ------------------------------------------------------------------------------------------------
def test_shift_offsets_edges():
    import igd_amd
    from igd_amd.database import IgdError
    assert igd_amd.shift_offsets(100, 25).tolist() == [-100, -75, -50, -25, 0, 25, 50, 75, 100]
    assert igd_amd.shift_offsets(99, 25).tolist() == [-75, -50, -25, 0, 25, 50, 75]
    assert igd_amd.shift_offsets(5, 6).tolist() == [0] and igd_amd.shift_offsets(0, 1).tolist() == [0]          # W < step, W == 0
    assert igd_amd.shift_offsets(2 ** 30, 2 ** 30).tolist() == [-2 ** 30, 0, 2 ** 30]
    assert igd_amd.shift_offsets(2047, 1).dtype == np.int32 and len(igd_amd.shift_offsets(2047, 1)) == 4095
    for w, s in ((2048, 1), (-1, 5), (10, 0), (10, -3), (2 ** 30 + 1, 2 ** 30)):
        with pytest.raises(IgdError, match="shift_offsets: "):
            igd_amd.shift_offsets(w, s)
    for w, s in ((100, 25), (5, 6), (999, 7)):
        assert np.array_equal(igd_amd.shift_offsets(w, s), SR.offsets(w, s))


def test_local_zscore_against_the_literal_formula():
    import igd_amd
    from igd_amd.database import IgdError, PermutationSupport, ShiftSupport
    rng = np.random.RandomState(5)
    rows = rng.randint(0, 50, (11, 6)).astype(np.int64)
    rows[:, 2] = 7                                             # sd == 0
    obs = rows[0] + 3
    ps = PermutationSupport(obs, *PR.stats(rows, obs), 11)
    shifted = rng.randint(0, 60, (5, 6)).astype(np.int64)
    z = igd_amd.local_zscore(ps, ShiftSupport(shifted, np.arange(5, dtype=np.int32)))
    assert z.dtype == np.float64 and z.shape == (5, 6) and np.isnan(z[:, 2]).all() and not np.isnan(np.delete(z, 2, axis=1)).any()
    for j in range(5):
        for f in (0, 1, 3, 4, 5):
            col = [int(x) for x in rows[:, f]]
            mean = sum(col) / 11
            sd = (sum((x - mean) ** 2 for x in col) / 10) ** 0.5
            assert abs(z[j, f] - (int(shifted[j, f]) - mean) / sd) <= 1e-9 * max(1.0, abs(z[j, f]))
    assert np.allclose(np.delete(z, 2, axis=1), np.delete(SR.zscore(shifted, rows), 2, axis=1), rtol=1e-12, atol=0)
    # the summary's own mean and sd, bit for bit
    sm = igd_amd.perm_summary(ps)
    assert np.array_equal(z[:, 0], (shifted[:, 0].astype(np.float64) - sm.mean[0]) / sm.sd[0])
    # one permutation: sd is undefined, every z is NaN
    one = PermutationSupport(obs, *PR.stats(rows[:1], obs), 1)
    assert np.isnan(igd_amd.local_zscore(one, ShiftSupport(shifted, None))).all()
    with pytest.raises(IgdError, match="local_zscore: "):
        igd_amd.local_zscore(ps, ShiftSupport(shifted[:, :5], None))


def test_the_new_host_names_resolve_but_stay_out_of_all():
    import igd_amd
    from igd_amd import database
    for name in ("shift_support_host", "shift_regions_host"):
        assert name not in igd_amd.__all__ and getattr(igd_amd, name) is getattr(database, name)
    for name in ("ShiftSupport", "shift_offsets", "local_zscore"):
        assert name in igd_amd.__all__ and getattr(igd_amd, name) is getattr(database, name)
