"""Permutation nulls by resampling from a universe on the host: igd_amd.resample_regions_host (igdc_resample_regions_host) and
mode="resample" of igd_amd.permute_host / permute_nearest_host / permute_bp_host (the igdc_*_host_rs entries).

Expected values never come from the code under test: resample_ref (a numpy uint64 restatement of THE DRAW of include/igd_hip.h)
draws the explicit lists, and igd_amd.support_host / nearest_sets_host / jaccard_host -- each held against the oracle in its own
test file -- measure every drawn set.  Every integer must be EQUAL; every output is handed over full of garbage."""
import ctypes as C
import random
import shutil

import numpy as np
import pytest

import permute_ref as PR
import resample_ref as RR
from helpers import short_tmpdir
from test_support_host import clustered_db

BIG_SEED = 0xC0FFEE1234567890


def pool_of(n, nctg=150, seed=1):
    """n regions over nctg contigs, unknown contigs (-1, nctg) among them, every region different from the others"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-1, nctg + 1, n).astype(np.int32)
    s = (np.arange(n, dtype=np.int64) * 7 + rng.integers(0, 7, n)).astype(np.int32)
    return c, s, (s + 1 + rng.integers(0, 500, n)).astype(np.int32)


def test_the_reference_itself():
    # h: the smallest h >= 1 with 4^h >= n
    assert [RR.bits(n) for n in (1, 2, 4, 5, 16, 17, 4096, 4097, 65536, 65537, 2 ** 31 - 1)] == [1, 1, 1, 2, 2, 3, 6, 7, 8, 9, 16]
    # the constants: mix64 is splitmix64's finaliser, whose first output for state 0 is well known
    assert int(RR.mix64(RR.G)) == 0xE220A8397B1DCDAF
    # step is a bijection of the whole domain, for every h the tests meet
    for n in (1, 5, 17, 4097):
        h = RR.bits(n)
        y = RR.step(RR.perm_base(7, 3), np.arange(4 ** h, dtype=np.uint64), h)
        assert np.array_equal(np.sort(y), np.arange(4 ** h, dtype=np.uint64))
    # a full draw is a permutation of [0, n), and its prefix is the shorter draw
    for n in (1, 2, 4, 5, 16, 17, 100, 4097):
        full = RR.resample_indices(7, 11, n, n)
        assert np.array_equal(np.sort(full), np.arange(n))
        assert np.array_equal(RR.resample_indices(7, 11, n // 2, n), full[:n // 2])
    assert not np.array_equal(RR.resample_indices(7, 11, 100, 100), RR.resample_indices(7, 12, 100, 100))
    assert not np.array_equal(RR.resample_indices(7, 11, 100, 100), RR.resample_indices(8, 11, 100, 100))
    # and the header's igd_hip_resample_index is this function: a pool whose region k starts at k hands back the indices
    import igd_amd
    k = np.arange(37, dtype=np.int32)
    assert np.array_equal(igd_amd.resample_regions_host(k * 0, k, k + 1, 12, 4, 1, 7)[1][0], RR.resample_indices(7, 4, 12, 37))


@pytest.mark.parametrize("npool", [1, 2, 4, 5, 16, 17, 4096, 4097, 65537])
def test_resample_regions_host_equals_the_reference(npool):
    import igd_amd
    pool = pool_of(npool)
    for seed, p0, nq, np_ in ((0, 0, npool, 3), (2 ** 64 - 1, 5, 1, 4), (BIG_SEED, 2 ** 20 - 2, min(npool, 1000), 2), (7, 1, max(npool // 3, 1), 2)):
        want = RR.resample_regions(pool, nq, p0, np_, seed)
        got = igd_amd.resample_regions_host(*pool, nq, p0, np_, seed)
        assert all(g.dtype == np.int32 and g.shape == (np_, nq) for g in got)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        # each draw holds nq distinct regions of the pool (the fixture's starts are all different)
        for k in range(np_):
            assert len(set(got[1][k].tolist())) == nq and np.isin(got[1][k], pool[1]).all()


def test_resample_regions_host_sizes_and_refusals():
    import igd_amd
    from igd_amd.database import IgdError
    pool = pool_of(10)
    assert igd_amd.resample_regions_host(*pool, 0, 0, 3)[0].shape == (3, 0)
    assert igd_amd.resample_regions_host(*pool, 4, 0, 0)[0].shape == (0, 4)
    with pytest.raises(IgdError, match="resample_regions_host: bad argument \\(11 regions from a universe of 10\\)"):
        igd_amd.resample_regions_host(*pool, 11, 0, 1)
    with pytest.raises(IgdError, match="resample_regions_host"):
        igd_amd.resample_regions_host(*pool, 4, -1, 1)
    with pytest.raises(IgdError, match="resample_regions_host: 10 / 10 / 9 universe regions given"):
        igd_amd.resample_regions_host(pool[0], pool[1], pool[2][:9], 4, 0, 1)
    with pytest.raises(IgdError, match="resample_regions_host"):
        igd_amd.resample_regions_host(pool[0][:0], pool[1][:0], pool[2][:0], 1, 0, 1)


# ---- the three nulls ---------------------------------------------------------------------------------------------------------------
NPERM = 9


def null_fixture(d, npool=300, nq=40, seed=9300):
    """a fuzzed clustered database of 40 files on 3 contigs; a universe of npool regions on them, unknown contigs and zero-length
    regions included; a set of nq regions that is NOT a subset of the universe"""
    rng = random.Random(seed)
    path, span = clustered_db(rng, d, "rs", 1 << 12, 1, 40, 3, 12)
    ctg_len = np.array([span // 2, span // 2 + 1234, span // 3], np.int32)
    return dict(path=path, pool=PR.random_regions(rng, ctg_len, npool), reg=PR.random_regions(rng, ctg_len, nq))


@pytest.fixture(scope="module")
def nfx():
    d = short_tmpdir("irs")
    yield null_fixture(d)
    shutil.rmtree(d, ignore_errors=True)


def support_rows(path, sets, **kw):
    """int64[nsets, nfiles + 1] from igd_amd.support_host on explicit lists"""
    import igd_amd
    c, s, e, off = sets
    rows = []
    for k in range(len(off) - 1):
        sup, nhit = igd_amd.support_host(path, c[off[k]:off[k + 1]], s[off[k]:off[k + 1]], e[off[k]:off[k + 1]], **kw)
        rows.append(np.concatenate([sup, [nhit]]))
    return np.array(rows, np.int64)


def stats_of(rows):
    """observed, sum, sumsq, n_ge, n_le, min, max of rows[0] among rows[1:]"""
    obs, x = rows[0], rows[1:]
    return [obs, x.sum(0), (x * x).sum(0), (x >= obs).sum(0), (x <= obs).sum(0), x.min(0), x.max(0)]


def test_a_draw_is_counted_with_its_own_contigs(nfx):
    """the fixture can tell: its drawn rows differ from each other and from the set's, and a draw counted with the set's contigs
    instead of its own gives another row than the one the host twin counts"""
    import igd_amd
    rows = support_rows(nfx["path"], RR.resample_sets(nfx["reg"], nfx["pool"], NPERM, 7))
    assert (rows[1:].min(0) != rows[1:].max(0)).sum() > 10 and (rows[0] != rows[1]).any()
    c, s, e, off = RR.resample_sets(nfx["reg"], nfx["pool"], NPERM, 7)
    wrong = c.copy()
    wrong[off[1]:off[2]] = nfx["reg"][0]
    wrong_row = support_rows(nfx["path"], (wrong, s, e, off))[1]
    one = igd_amd.permute_host(nfx["path"], *nfx["reg"], None, 1, 7, "resample", universe=nfx["pool"])
    assert np.array_equal(one.min, rows[1]) and np.array_equal(one.max, rows[1]) and (wrong_row != one.min).any()


@pytest.mark.parametrize("kw", [dict(), dict(v=500), dict(min_overlap=40)])
@pytest.mark.parametrize("seed", [0, BIG_SEED])
def test_permute_host_resample_equals_support_host_of_each_drawn_set(nfx, kw, seed):
    import igd_amd
    want = stats_of(support_rows(nfx["path"], RR.resample_sets(nfx["reg"], nfx["pool"], NPERM, seed), **kw))
    got = igd_amd.permute_host(nfx["path"], *nfx["reg"], None, NPERM, seed, "resample", universe=nfx["pool"], **kw)
    assert got.nperm == NPERM
    for name, w in zip("observed sum sumsq n_ge n_le min max".split(), want):
        assert np.array_equal(getattr(got, name), w), name
    assert np.isfinite(igd_amd.perm_summary(got).mean).all()


def test_permute_nearest_host_resample_equals_nearest_sets_host_of_each_drawn_set(nfx):
    import igd_amd
    for window in (0, 3000):
        want = igd_amd.nearest_sets_host(nfx["path"], *RR.resample_sets(nfx["reg"], nfx["pool"], NPERM, 7), window)
        got = igd_amd.permute_nearest_host(nfx["path"], *nfx["reg"], None, NPERM, window, 7, "resample", universe=nfx["pool"])
        for name in ("n_within", "n_overlap", "sum_dist"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), (window, name)
    assert (got.sum_dist[1:].min(0) != got.sum_dist[1:].max(0)).any()
    assert len(igd_amd.perm_nearest_summary(got).within_mean) == got.n_within.shape[1]


def test_permute_bp_host_resample_equals_jaccard_host_of_each_drawn_set(nfx):
    import igd_amd
    want = igd_amd.jaccard_host(nfx["path"], *RR.resample_sets(nfx["reg"], nfx["pool"], NPERM, 7))
    got = igd_amd.permute_bp_host(nfx["path"], *nfx["reg"], None, NPERM, 7, "resample", universe=nfx["pool"])
    assert np.array_equal(got.inter, want.inter) and np.array_equal(got.set_bp, want.set_bp) and np.array_equal(got.n_merged, want.n_merged)
    assert got.n_dropped == want.n_dropped[0] and np.array_equal(got.file_bp, want.file_bp)
    assert len(set(got.set_bp[1:].tolist())) > 1 and len(set(want.n_dropped.tolist())) > 1
    assert len(igd_amd.perm_bp_summary(got).mean) == got.inter.shape[1]


def test_a_draw_of_the_whole_universe_is_the_universe_in_another_order(nfx):
    import igd_amd
    pool = nfx["pool"]
    row = support_rows(nfx["path"], (*pool, np.array([0, len(pool[1])], np.int64)))[0]
    ps = igd_amd.permute_host(nfx["path"], *pool, None, 5, 3, "resample", universe=pool)
    assert np.array_equal(ps.observed, row) and np.array_equal(ps.min, row) and np.array_equal(ps.max, row)
    assert np.array_equal(ps.sum, 5 * row) and (ps.n_ge == 5).all() and (ps.n_le == 5).all()
    pb = igd_amd.permute_bp_host(nfx["path"], *pool, None, 5, 3, "resample", universe=pool)
    assert (pb.inter == pb.inter[0]).all() and (pb.set_bp == pb.set_bp[0]).all() and (pb.n_merged == pb.n_merged[0]).all()
    pn = igd_amd.permute_nearest_host(nfx["path"], *pool, None, 5, 2000, 3, "resample", universe=pool)
    assert (pn.n_within == pn.n_within[0]).all() and (pn.sum_dist == pn.sum_dist[0]).all()


def test_no_region_and_one_permutation(nfx):
    import igd_amd
    none = tuple(a[:0] for a in nfx["reg"])
    ps = igd_amd.permute_host(nfx["path"], *none, None, 4, 0, "resample", universe=nfx["pool"])
    assert not ps.observed.any() and not ps.sum.any() and (ps.n_ge == 4).all() and (ps.n_le == 4).all()
    assert not igd_amd.permute_nearest_host(nfx["path"], *none, None, 4, 100, 0, "resample", universe=nfx["pool"]).n_within.any()
    assert not igd_amd.permute_bp_host(nfx["path"], *none, None, 4, 0, "resample", universe=nfx["pool"]).inter.any()
    # an empty universe serves an empty set
    assert not igd_amd.permute_host(nfx["path"], *none, None, 1, 0, "resample", universe=none).sum.any()


def test_one_region_and_fewer_rows_than_threads(nfx, monkeypatch):
    """one region; one draw of 4500 regions from a universe of exactly 4500 on three threads: the region rows are worth three
    threads, and only one row (support) or two (the others, with the set as given) are there to share out"""
    import igd_amd
    monkeypatch.setenv("IGD_HOST_THREADS", "3")
    pool = tuple(np.tile(a, 15) for a in nfx["pool"])
    for reg, nperm in ((tuple(a[:1] for a in nfx["reg"]), 3), (tuple(np.tile(a, 113)[:4500] for a in nfx["reg"]), 1)):
        assert nperm == 3 or len(reg[0]) == len(pool[0]) == 4500
        sets = RR.resample_sets(reg, pool, nperm, 5)
        got = igd_amd.permute_host(nfx["path"], *reg, None, nperm, 5, "resample", universe=pool)
        for name, w in zip("observed sum sumsq n_ge n_le min max".split(), stats_of(support_rows(nfx["path"], sets))):
            assert np.array_equal(getattr(got, name), w), (nperm, name)
        want = igd_amd.nearest_sets_host(nfx["path"], *sets, 3000)
        got = igd_amd.permute_nearest_host(nfx["path"], *reg, None, nperm, 3000, 5, "resample", universe=pool)
        assert all(np.array_equal(getattr(got, n), getattr(want, n)) for n in ("n_within", "n_overlap", "sum_dist")), nperm
        want = igd_amd.jaccard_host(nfx["path"], *sets)
        got = igd_amd.permute_bp_host(nfx["path"], *reg, None, nperm, 5, "resample", universe=pool)
        assert np.array_equal(got.inter, want.inter) and np.array_equal(got.set_bp, want.set_bp) and np.array_equal(got.n_merged, want.n_merged)
    assert got.inter[1].any()


HOST = [("permute_host", ()), ("permute_nearest_host", (100,)), ("permute_bp_host", ())]


@pytest.mark.parametrize("name,extra", HOST, ids=[h[0] for h in HOST])
def test_the_python_refusals_of_the_host_entries(nfx, name, extra):
    import igd_amd
    from igd_amd.database import IgdError
    f = getattr(igd_amd, name)
    ctg_len = np.array([10 ** 6] * 3, np.int32)
    ws = igd_amd.build_workspace([0], [0], [1000], ctg_len)
    with pytest.raises(ValueError, match=name + ": mode='resample' and universe= go together, not one without the other"):
        f(nfx["path"], *nfx["reg"], None, 3, *extra, 0, "resample")
    for mode in ("circular", "shuffle"):
        with pytest.raises(ValueError, match=name + ": mode='resample' and universe= go together"):
            f(nfx["path"], *nfx["reg"], ctg_len, 3, *extra, 0, mode, universe=nfx["pool"])
    with pytest.raises(ValueError, match=name + ": mode='resample' .* ctg_len \\(genome_path\\) must be None"):
        f(nfx["path"], *nfx["reg"], ctg_len, 3, *extra, 0, "resample", universe=nfx["pool"])
    with pytest.raises(ValueError, match=name + ": mode='resample' .* there is no workspace= with it"):
        f(nfx["path"], *nfx["reg"], None, 3, *extra, 0, "resample", universe=nfx["pool"], workspace=ws)
    with pytest.raises(ValueError, match=name):
        f(nfx["path"], *nfx["reg"], ctg_len, 3, *extra, 0, "workspace", universe=nfx["pool"], workspace=ws)
    with pytest.raises(IgdError, match=name + ": 300 / 300 / 299 universe regions given"):
        f(nfx["path"], *nfx["reg"], None, 3, *extra, 0, "resample", universe=(nfx["pool"][0], nfx["pool"][1], nfx["pool"][2][:-1]))
    # the engine's refusals, said by the host twin: a set larger than the universe, the number of permutations
    small = tuple(a[:39] for a in nfx["pool"])
    with pytest.raises(IgdError, match=name + ": a refused argument .*40 regions from a universe of 39"):
        f(nfx["path"], *nfx["reg"], None, 3, *extra, 0, "resample", universe=small)
    for nperm in (0, 2 ** 20 + 1):
        with pytest.raises(IgdError, match=name + ": a refused argument"):
            f(nfx["path"], *nfx["reg"], None, nperm, *extra, 0, "resample", universe=nfx["pool"])


def test_the_refusals_of_the_engine_said_by_the_host_twin(nfx):
    """an out-of-range min_overlap (the support's own first check), more regions than a batch, and the support's
    nperm * nq^2 >= 2^63: each is a refused argument, and the call beside it that lacks the fault runs"""
    import igd_amd
    from igd_amd import MinOverlap
    from igd_amd.database import IgdError
    path, reg, pool = nfx["path"], nfx["reg"], nfx["pool"]
    for field in ("bp", "query_ppm", "record_ppm"):
        mo = MinOverlap()
        setattr(mo, field, -1)
        with pytest.raises(IgdError, match="permute_host: a refused argument"):
            igd_amd.permute_host(path, *reg, None, 2, 0, "resample", universe=pool, min_overlap=mo)
    mo = MinOverlap()
    mo.query_ppm = 10 ** 6 + 1
    with pytest.raises(IgdError, match="permute_host: a refused argument"):
        igd_amd.permute_host(path, *reg, None, 2, 0, "resample", universe=pool, min_overlap=mo)
    assert igd_amd.permute_host(path, *reg, None, 2, 0, "resample", universe=pool, min_overlap=MinOverlap(query_ppm=10 ** 6)).nperm == 2
    from igd_amd import _native as N
    N.cli().igd_hip_max_batch.restype = C.c_int64
    big = int(N.cli().igd_hip_max_batch()) + 1
    z = np.zeros(big, np.int32)
    for f, extra in ((igd_amd.permute_host, ()), (igd_amd.permute_nearest_host, (10,)), (igd_amd.permute_bp_host, ())):
        with pytest.raises(IgdError, match="a refused argument .*%d regions from a universe of %d" % (big, big)):
            f(path, z, z, z, None, 2, *extra, 0, "resample", universe=(z, z, z))
    with pytest.raises(IgdError, match="resample_regions_host: bad argument"):
        igd_amd.resample_regions_host(z, z, z, big, 0, 1)
    n = 3100000                                                                # 2^20 * n^2 >= 2^63
    assert 2 ** 20 * n * n >= 2 ** 63 and n < big and 2 ** 19 * n * n < 2 ** 63
    with pytest.raises(IgdError, match="permute_host: a refused argument"):
        igd_amd.permute_host(path, z[:n], z[:n], z[:n], None, 2 ** 20, 0, "resample", universe=(z[:n], z[:n], z[:n]))


def test_a_universe_above_the_batch_is_refused_by_the_host_twin(nfx, monkeypatch):
    """IGD_HIP_MAX_BATCH is read once per process by the library: a child process sees the lowered value"""
    import subprocess
    import sys
    code = ("import sys, numpy as np, igd_amd\n"
            "from igd_amd.database import IgdError\n"
            "z = np.zeros(65, np.int32)\n"
            "for f, extra in ((igd_amd.permute_host, ()), (igd_amd.permute_nearest_host, (10,)), (igd_amd.permute_bp_host, ())):\n"
            "    try:\n"
            "        f(sys.argv[1], z[:3], z[:3], z[:3] + 5, None, 2, *extra, 0, 'resample', universe=(z, z, z + 5))\n"
            "    except IgdError as e:\n"
            "        assert 'a refused argument' in str(e), e\n"
            "    else:\n"
            "        raise SystemExit('a universe of 65 regions passed a batch of 64')\n"
            "    f(sys.argv[1], z[:3], z[:3], z[:3] + 5, None, 2, *extra, 0, 'resample', universe=(z[:64], z[:64], z[:64] + 5))\n"
            "try:\n"
            "    igd_amd.resample_regions_host(z, z, z, 3, 0, 1)\n"
            "except IgdError:\n"
            "    pass\n"
            "else:\n"
            "    raise SystemExit('resample_regions_host took a universe above the batch')\n")
    monkeypatch.setenv("IGD_HIP_MAX_BATCH", "64")
    r = subprocess.run([sys.executable, "-c", code, nfx["path"]], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the statistical condition of the support null -----------------------------------------------------------------------------------
def hypergeometric_fixture(d):
    """npool = 1000 universe regions and a set of the first nq = 100 of them on a clustered database of 40 files"""
    rng = random.Random(9400)
    path, span = clustered_db(rng, d, "hg", 1 << 12, 1, 40, 3, 12)
    ctg_len = np.array([span // 2, span // 2 + 1234, span // 3], np.int32)
    pool = PR.random_regions(rng, ctg_len, 1000, unknown=())
    return dict(path=path, pool=pool, reg=tuple(a[:100] for a in pool))


def hypergeometric_deviations(K, ps, npool, nq):
    """|sum_f - nperm nq K_f / npool| in standard deviations of a sum of nperm independent hypergeometric draws, on every file
    with 0 < K_f < npool"""
    K = np.asarray(K, np.float64)
    live = (K > 0) & (K < npool)
    var = ps.nperm * nq * (K / npool) * (1 - K / npool) * (npool - nq) / (npool - 1)
    return (np.abs(ps.sum - ps.nperm * nq * K / npool) / np.sqrt(var))[live]


def test_the_support_null_is_hypergeometric_within_six_standard_deviations():
    """The largest deviation over the 41 columns of this input is 2.538 standard deviations (seed 7, 2000 draws)."""
    import igd_amd
    d = short_tmpdir("ihg")
    try:
        fx = hypergeometric_fixture(d)
        sup, nhit = igd_amd.support_host(fx["path"], *fx["pool"])
        ps = igd_amd.permute_host(fx["path"], *fx["reg"], None, 2000, 7, "resample", universe=fx["pool"])
        dev = hypergeometric_deviations(np.concatenate([sup, [nhit]]), ps, 1000, 100)
        print("hypergeometric deviations: %d columns, largest %.3f sd" % (len(dev), dev.max()))
        assert len(dev) >= 30 and (dev <= 6).all()
    finally:
        shutil.rmtree(d, ignore_errors=True)
