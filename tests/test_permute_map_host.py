"""The permutation null of the overlapping records' values on the host (igdc_permute_map_host, _ws, _rs and
igdc_perm_map_summary; igd_amd.permute_map_host / perm_map_summary).  No GPU.

Expected values never come from the code under test: tests/permute_map_ref.py composes permute_ref's generator, workspace_ref's
placement and resample_ref's draw with map_ref's definition over interval lists this test wrote, every integer compared
exactly; the summary against numpy float64 on hand-made matrices, floats to 1e-12 relative -- derived, not measured: 64 sequential
double additions err by at most 64 x 2^-53, about 7e-15, and the rest is margin.  Every output array the caller can hand over is
handed over full of 0x5a5a5a5a5a5a5a5a (the host functions allocate their own)."""
import random
import shutil

import numpy as np
import pytest

import igd_amd
import permute_map_ref as PM
import permute_ref as PR
import workspace_ref as WR
from helpers import short_tmpdir
from map_ref import I32_MAX, I32_MIN, OPS, ListDb, clustered_lists, crowd_regions, placed_db, placed_regions
from test_support_host import host_threads  # noqa: F401  (a fixture)

RTOL = 1e-12
ALL_OPS = OPS + ("mean",)


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("ipm")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def fx(workdir):
    """a clustered database with values, regions on its two contigs (and on unknown ones), a workspace they all fit in, a universe"""
    rng = random.Random(8800)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 9, 2, 12, -1000)
    ldb = ListDb(workdir, "pm", files, nbp, 1)
    ctg_len = np.array([span + 7 * nbp, span + 5 * nbp + 13], np.int32)
    n = 120
    ichr = np.array([rng.choice([0, 1, 0, 1, -1, 99]) for _ in range(n)], np.int32)
    ln = np.array([rng.choice([0, 1, 50, 300, 700, 1999]) for _ in range(n)], np.int32)
    qs = np.array([rng.randrange(0, span) for _ in range(n)], np.int32)
    seg = WR.random_workspace(rng, ctg_len, 40, 2000)
    tab = WR.table(*seg, ctg_len)
    assert not WR.unplaceable(ichr, qs, qs + ln, ctg_len, tab).any()
    pool = PR.random_regions(rng, ctg_len, 400)
    return dict(ldb=ldb, nbp=nbp, ctg_len=ctg_len, reg=(ichr, qs, qs + ln), tab=tab, ws=igd_amd.build_workspace(*seg, ctg_len), pool=pool)


def host_null(fx, ldb, reg, nperm, op, seed, mode, v):
    kw = dict(seed=seed, mode=mode, value_filter=v)
    if mode == "workspace":
        kw["workspace"] = fx["ws"]
    if mode == "resample":
        kw["universe"] = fx["pool"]
    return igd_amd.permute_map_host(ldb.path, *reg, None if mode == "resample" else fx["ctg_len"], nperm, op, **kw)


def check(fx, ldb, reg, nperm, op, seed, mode, v):
    want = PM.null(ldb, *reg, fx["ctg_len"], nperm, op, seed, mode, v, tab=fx["tab"], pool=fx["pool"])
    got = host_null(fx, ldb, reg, nperm, op, seed, mode, v)
    assert got.op == op and got.nperm == nperm
    for name, g, w in zip(("n_hit", "pairs", "agg_sum"), got[:3], want):
        assert g.dtype == np.int64 and g.shape == (nperm + 1, ldb.nfiles) and np.array_equal(g, w), (name, nperm, op, mode, v)
    return got


@pytest.mark.parametrize("mode", ["circular", "shuffle", "workspace", "resample"])
@pytest.mark.parametrize("op", ALL_OPS)
def test_host_equals_the_numpy_composition(op, mode, fx, host_threads):
    moved = hit = False
    for nperm, threads, seed in ((1, "1", 3), (37, "7", 11)):
        host_threads(threads)
        for v in (None, 500):
            got = check(fx, fx["ldb"], fx["reg"], nperm, op, seed, mode, v)
            hit |= bool(got.n_hit.any())
            moved |= bool((got.agg_sum[1:] != got.agg_sum[0]).any())
            # row 0 is the set as given
            ms = igd_amd.map_sets_host(fx["ldb"].path, *fx["reg"], [0, len(fx["reg"][1])], PM.run_op(op), value_filter=v)
            for g, w in zip(got[:3], ms[:3]):
                assert np.array_equal(g[0], w[0])
    assert hit and moved, "fixture is vacuous"


@pytest.mark.parametrize("mode", ["circular", "shuffle", "workspace", "resample"])
def test_one_region_and_fewer_rows_than_threads(mode, fx, host_threads):
    """the shapes at which a driver shared by the nulls goes wrong: one region; two rows (one permutation) of 2160 regions on three
    threads -- 4320 region rows are worth three threads, and only two rows are there to share out; a pool as large as the set"""
    host_threads("3")
    ichr = fx["reg"][0]
    k = int(np.flatnonzero((ichr >= 0) & (ichr < 2))[0])
    check(fx, fx["ldb"], tuple(a[k:k + 1] for a in fx["reg"]), 3, "sum", 5, mode, None)
    many = tuple(np.tile(a, 18) for a in fx["reg"])
    wide = dict(fx, pool=tuple(np.tile(a, 6) for a in fx["pool"]))
    got = check(wide, fx["ldb"], many, 1, "sum", 7, mode, 500)
    assert got.n_hit.any()
    if mode == "resample":
        n = len(ichr)
        check(dict(fx, pool=tuple(a[:n] for a in fx["pool"])), fx["ldb"], fx["reg"], 2, "max", 9, mode, None)


@pytest.mark.parametrize("op", ALL_OPS)
def test_the_placed_database(op, workdir, fx):
    """300 records of one file under one region, INT32_MIN and INT32_MAX under one region, three times INT32_MAX, -v 500 removing
    the maximum, the record over five tiles: as one set, under the set as given (row 0) and under its permutations"""
    nbp = 1 << 14
    ldb = placed_db(workdir, nbp, "pmplaced", crowd=True)
    (pc, ps, pe), _ = placed_regions(nbp)
    (cc, cs, ce), _ = crowd_regions(nbp)
    # the generator wants 0 <= s <= e <= L on known contigs: the placed regions that are, and the crowd's
    c, s, e = np.concatenate([pc, cc]), np.concatenate([ps, cs]), np.concatenate([pe, ce])
    ctg_len = np.array([9 * nbp, 13 * nbp, 2 ** 31 - 1], np.int32)
    ok = (c < 0) | (c > 2) | ((s >= 0) & (e >= s) & (e <= ctg_len[np.clip(c, 0, 2)]))
    reg = (c[ok], s[ok], e[ok])
    assert ok.sum() >= 20
    for v in (None, 500):
        got = check(dict(fx, ctg_len=ctg_len), ldb, reg, 5, op, 2, "circular", v)
        if op == "sum" and v is None:
            assert got.agg_sum[0, 3] == 3 * I32_MAX and got.pairs[0, 6] >= 300
        if op == "min" and v is None:
            assert (got.agg_sum[0] < 0).any() and got.agg_sum[0, 2] < I32_MIN


def test_refused_arguments_and_empty_calls(workdir, fx):
    from igd_amd.database import IgdError
    ldb, ctg_len = fx["ldb"], fx["ctg_len"]
    ichr, qs, qe = fx["reg"]
    for bad in (dict(nperm=0), dict(nperm=(1 << 20) + 1), dict(op="median"), dict(mode="rotate")):
        a = dict(dict(nperm=3, op="sum", mode="circular"), **bad)
        with pytest.raises(IgdError):
            igd_amd.permute_map_host(ldb.path, ichr, qs, qe, ctg_len, a["nperm"], a["op"], mode=a["mode"])
    for kw in (dict(workspace=fx["ws"]), dict(mode="workspace"), dict(universe=fx["pool"]), dict(mode="resample", universe=fx["pool"])):
        with pytest.raises(ValueError):                               # a workspace without its mode and the reverse; a universe beside ctg_len
            igd_amd.permute_map_host(ldb.path, ichr, qs, qe, ctg_len, 3, "sum", **kw)
    known = np.flatnonzero((ichr >= 0) & (ichr < len(ctg_len)))
    e2 = qe.copy()
    e2[known[0]] = ctg_len[ichr[known[0]]] + 1
    with pytest.raises(IgdError):
        igd_amd.permute_map_host(ldb.path, ichr, qs, e2, ctg_len, 3, "sum")
    with pytest.raises(IgdError):
        igd_amd.permute_map_host(ldb.path, ichr, qs, qe, ctg_len[:1], 3, "sum")
    # a value op on a database without values; count works there
    files, span = clustered_lists(random.Random(5), 1 << 12, 3, 2, 6)
    blind = ListDb(workdir, "pm0", files, 1 << 12, 0)
    for op in ("sum", "min", "max", "mean"):
        with pytest.raises(IgdError):
            igd_amd.permute_map_host(blind.path, ichr, qs, qe, ctg_len, 3, op)
    got = igd_amd.permute_map_host(blind.path, ichr, qs, qe, ctg_len, 3, "count")
    want = PM.null(blind, ichr, qs, qe, ctg_len, 3, "count")
    assert all(np.array_equal(g, w) for g, w in zip(got[:3], want)) and np.array_equal(got.pairs, got.agg_sum)
    z = np.zeros(0, np.int32)
    got = igd_amd.permute_map_host(ldb.path, z, z, z, ctg_len, 4, "max")
    assert all(a.shape == (5, ldb.nfiles) and not a.any() for a in got[:3])


# ---- the summary ------------------------------------------------------------------------------------------------------------
def check_summary(nh, npairs, sa, op):
    nh, npairs, sa = (np.asarray(x, np.int64) for x in (nh, npairs, sa))
    got = igd_amd.perm_map_summary(igd_amd.PermutationMap(nh, npairs, sa, op, nh.shape[0] - 1))
    want = PM.summary(nh, npairs, sa, op)
    for name in PM.FIELDS:
        g, w = getattr(got, name), want[name]
        if name in PM.INT_FIELDS:
            assert g.dtype == np.int64 and np.array_equal(g, w), (name, g, w)
        else:
            assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(w)), (name, g, w)
            assert np.allclose(g, w, rtol=RTOL, atol=0, equal_nan=True), (name, g, w)
    return got


def test_summary_on_hand_made_matrices():
    #            observed row, then four permutations; columns:
    #   0  ordinary    1  n_hit_0 = 0 (observed undefined)    2  every permuted n_hit = 0 (n_def 0)    3  n_def = 2 of 4
    #   4  ties with the observed ratio in two permutations   5  negative sums
    nh = [[5, 0, 4, 3, 2, 4],
          [4, 2, 0, 0, 4, 2],
          [6, 0, 0, 7, 1, 4],
          [5, 3, 0, 0, 6, 8],
          [2, 1, 0, 2, 3, 1]]
    sa = [[50, 0, 40, 9, 10, -40],
          [44, 8, 0, 0, 20, -30],
          [30, 0, 0, 21, 7, -40],
          [75, 9, 0, 0, 30, -88],
          [20, 5, 0, 8, 9, -3]]
    npairs = (np.asarray(nh) * 3).tolist()
    for op in ("sum", "min", "count", "mean"):
        got = check_summary(nh, npairs, sa, op)
        assert got.observed_n_hit.tolist() == nh[0] and got.n_def.tolist() == [4, 3, 0, 2, 4, 4]
        # the observed row without a statistic: everything about it NaN, nothing counted
        assert np.isnan(got.observed[1]) and np.isnan(got.z[1]) and np.isnan(got.nlog10_p_upper[1]) and (got.n_ge[1], got.n_le[1]) == (0, 0)
        assert not np.isnan(got.mean[1])
        # no permutation with a statistic: mean, sd and z NaN, p = (0 + 1) / (0 + 1)
        assert np.isnan(got.mean[2]) and np.isnan(got.sd[2]) and np.isnan(got.z[2]) and got.nlog10_p_upper[2] == 0 and got.nlog10_p_lower[2] == 0
        assert got.n_ge[3] == 2 and abs(got.nlog10_p_upper[3]) < 1e-12     # 3 / 3 against 21 / 7 and 8 / 2: (2 + 1) / (2 + 1)
        # ties count on both sides: 10 / 2 = 20 / 4 = 30 / 6
        assert (got.n_ge[4], got.n_le[4]) == (3, 3)
        assert (got.n_ge[5], got.n_le[5]) == (2, 3)                 # -10 against -15, -10, -11, -3
    one = check_summary([[3, 0], [2, 4]], [[6, 0], [5, 9]], [[30, 0], [10, 4]], "mean")
    assert np.isnan(one.sd).all() and np.isnan(one.z).all() and np.isnan(one.nhit_sd).all()
    rng = np.random.RandomState(5)
    for P in (2, 37):
        h = rng.randint(0, 50, size=(P + 1, 9)).astype(np.int64)
        h[:, 0] = rng.randint(0, 2, size=P + 1)
        check_summary(h, h * 2, h * rng.randint(-1000, 1000, size=h.shape), "mean")


def test_summary_compares_the_ratios_exactly():
    """agg_sum / n_hit as doubles is the same number for the observed row and both permutations (2^62 + 1 and 2^62 + 2 round to
    2^62), the integers differ; and agg_sum * n_hit at the ends of int32 times 2^20 regions does not fit 64 bits: only 128-bit
    arithmetic gets either right."""
    big, n = 1 << 62, (1 << 20) + 1
    nh = [[n, n, n], [n, n - 1, n], [n, n, n]]
    sa = [[big + 1, big, I32_MIN * n], [big, big, I32_MIN * n + 1], [big + 2, big + 1, I32_MIN * n]]
    assert float(big + 1) / n == float(big) / n == float(big + 2) / n
    got = check_summary(nh, nh, sa, "sum")
    assert got.n_ge.tolist() == [1, 2, 2] and got.n_le.tolist() == [1, 0, 1]
