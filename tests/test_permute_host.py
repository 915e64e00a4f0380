"""Permutation null of region-set support without a GPU: igdc_permute_regions_host, igdc_permute_host and igdc_perm_summary
(igd_hostpath.c) through igd_amd.permute_regions_host / permute_host / perm_summary.

The generator is held bit for bit against permute_ref (numpy uint64); the counts against permute_ref.stats of the rows that
igdc_support_host -- which tests/test_support_host.py holds against the oracle -- gives for permute_ref's explicit lists.  All
integers must be EQUAL.  The summary is held against numpy (ddof = 1) within relative 1e-12: its numerator is exact, then one
division and one square root are a few units of 1.1e-16."""
import os
import random
import shutil

import numpy as np
import pytest

import permute_ref as PR
from helpers import short_tmpdir
from test_support_host import FLAT, NEST, NOV, NUMPY_DBS, HostDb, cli_rule, clustered_db

BIG = 2 ** 31 - 1
CTG_LEN = np.array([1, 2, 1000, BIG, 1000], np.int32)         # (contigs 2 and 4: the same length under two keys)
MODES = (PR.CIRCULAR, PR.SHUFFLE)


@pytest.fixture
def tmp():
    d = short_tmpdir("iph")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", t)
    os.environ.pop("IGD_HOST_THREADS", None)


def generator_fixture():
    """per contig: width 0 at the start and at the end, the whole contig, all but one base at either side, one that ends at
    L, random ones; on the long contig starts near 2^31, where s + offset passes 32 bits; ichr = -1 and ichr = nctg"""
    rows = []
    for c, L in enumerate(int(x) for x in CTG_LEN):
        rows += [(c, 0, 0), (c, L, L), (c, 0, L), (c, 0, L - 1), (c, 1, L), (c, L - L // 3, L), (c, L // 2, L // 2 + L // 4)]
        rows += [(c, L - 1, L), (c, L - 1, L - 1)]
    rng = random.Random(5)
    for _ in range(40):
        s = rng.randrange(BIG - 1000, BIG)
        rows.append((3, s, rng.randrange(s, BIG + 1)))
        s = rng.randrange(0, 1001)
        rows.append((rng.choice([2, 4]), s, rng.randrange(s, 1001)))
    rows += [(-1, 5, 900), (len(CTG_LEN), 7, 3), (-1, -4, -9), (len(CTG_LEN), BIG, BIG)]
    a = np.array(rows, np.int64)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32)


def check_permuted(ichr, qs, qe, ctg_len, ps, pe):
    """0 <= s', e' <= L, e' - s' == len on known contigs; the others unchanged"""
    known = (ichr >= 0) & (ichr < len(ctg_len))
    L = ctg_len.astype(np.int64)[np.where(known, ichr, 0)]
    ps, pe = ps.astype(np.int64), pe.astype(np.int64)
    assert (ps[:, known] >= 0).all() and (pe[:, known] <= L[known][None, :]).all()
    assert ((pe - ps)[:, known] == (qe.astype(np.int64) - qs)[known][None, :]).all()
    assert (ps[:, ~known] == qs[~known][None, :]).all() and (pe[:, ~known] == qe[~known][None, :]).all()


@pytest.mark.parametrize("mode", MODES)
def test_generator_equals_the_reference(mode):
    import igd_amd
    ichr, qs, qe = generator_fixture()
    for seed, p0, n in ((0, 0, 9), (1, 0, 3), (2 ** 64 - 1, 5, 4), (12345678901234567, 2 ** 20 - 2, 2)):
        ws, we = PR.permute(ichr, qs, qe, CTG_LEN, p0, n, seed, mode)
        gs, ge = igd_amd.permute_regions_host(ichr, qs, qe, CTG_LEN, p0, n, seed, mode)
        assert gs.dtype == np.int32 and gs.shape == (n, len(qs))
        assert np.array_equal(gs, ws) and np.array_equal(ge, we), (seed, p0)
        check_permuted(ichr, qs, qe, CTG_LEN, gs, ge)
    # on the long contig the sum s + offset passes 2^32 somewhere, and wraps are pushed back somewhere (circular)
    big = ichr == 3
    off = PR.r(0, np.arange(9, dtype=np.uint64), 3) % np.uint64(BIG)
    assert (qs[big].astype(np.int64)[None, :] + off.astype(np.int64)[:, None] >= 2 ** 31).any()
    gs, ge = igd_amd.permute_regions_host(ichr, qs, qe, CTG_LEN, 0, 9, 0, mode)
    assert (gs[:, big] != qs[big][None, :]).any()
    if mode == PR.CIRCULAR:
        assert (ge[:, (qe > qs) & (ichr >= 0) & (ichr < 5)] == CTG_LEN[ichr[(qe > qs) & (ichr >= 0) & (ichr < 5)]][None, :]).any()
    # no region, no permutation
    e = np.zeros(0, np.int32)
    assert igd_amd.permute_regions_host(e, e, e, CTG_LEN, 0, 3, 0, mode)[0].shape == (3, 0)
    assert igd_amd.permute_regions_host(ichr, qs, qe, CTG_LEN, 0, 0, 0, mode)[0].shape == (0, len(qs))


def test_seed_permutation_and_key_each_change_the_offset():
    import igd_amd
    one = lambda c, n=1: (np.full(n, c, np.int32), np.zeros(n, np.int32), np.ones(n, np.int32))
    f = lambda reg, mode, seed, p: igd_amd.permute_regions_host(*reg, CTG_LEN, p, 1, seed, mode)[0][0]
    for mode in MODES:
        base = f(one(3), mode, 0, 0)[0]
        assert base != f(one(3), mode, 1, 0)[0] and base != f(one(3), mode, 0, 1)[0]
        assert base == f(one(3), mode, 0, 0)[0]
    # the key: the contig under the rigid shift (two contigs of one length), the position under the shuffle
    assert f(one(2), PR.CIRCULAR, 0, 0)[0] != f(one(4), PR.CIRCULAR, 0, 0)[0]
    both = f(one(3, 2), PR.CIRCULAR, 0, 0)
    assert both[0] == both[1]                                    # rigid: two identical regions stay together
    both = f(one(3, 2), PR.SHUFFLE, 0, 0)
    assert both[0] != both[1]


@pytest.mark.parametrize("mode", MODES)
def test_offsets_are_uniform_on_a_contig_of_ten(mode):
    """10^5 permutations of one base on L = 10: each of the 10 starts occurs 10 000 +- 570 times (six binomial standard
    deviations of 95)"""
    import igd_amd
    gs, ge = igd_amd.permute_regions_host([0], [0], [1], [10], 0, 100000, 0, mode)
    cnt = np.bincount(gs[:, 0], minlength=10)
    print(mode, cnt.tolist())
    assert len(cnt) == 10 and (np.abs(cnt - 10000) <= 570).all(), cnt.tolist()
    assert np.array_equal(ge, gs + 1)


def reference_rows(H, ichr, qs, qe, ctg_len, nperm, seed, mode, v, rule):
    """(observed int64[nF + 1], rows int64[nperm, nF + 1]) from igdc_support_host on permute_ref's explicit lists"""
    def row(s, e):
        sup, nhit = H.support(ichr, s, e, v, rule)
        return np.concatenate([sup, [nhit]]).astype(np.int64)
    ps, pe = PR.permute(ichr, qs, qe, ctg_len, 0, nperm, seed, mode)
    return row(qs, qe), np.stack([row(ps[p], pe[p]) for p in range(nperm)])


def check_result(ps, observed, rows, what=None):
    want = PR.stats(rows, observed)
    assert np.array_equal(ps.observed, observed), what
    for got, w, name in zip((ps.sum, ps.sumsq, ps.n_ge, ps.n_le, ps.min, ps.max), want, ("sum", "sumsq", "n_ge", "n_le", "min", "max")):
        assert got.dtype == np.int64 and np.array_equal(got, w), (what, name)
    assert ps.nperm == rows.shape[0]


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_permute_host_equals_the_reference_statistics(case, tmp, host_threads):
    import igd_amd
    rng = random.Random(5100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    path, span = clustered_db(rng, tmp, "p%d" % case, nbp, gtype, nfiles, nctg, span_tiles)
    ctg_len = np.full(nctg, span + 2 * nbp, np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 1300)
    H = HostDb(path)
    try:
        moved = 0
        for mode in MODES:
            for nperm in (1, 2, 7):
                for v in (0, 500):
                    rule, ev = cli_rule(gtype, v)
                    obs, rows = reference_rows(H, ichr, qs, qe, ctg_len, nperm, 3, mode, ev, rule)
                    moved += int((rows != obs[None, :]).sum())
                    for threads in ("1", "3"):
                        host_threads(threads)
                        ps = igd_amd.permute_host(path, ichr, qs, qe, ctg_len, nperm, 3, mode, v)
                        check_result(ps, obs, rows, (mode, nperm, v, threads))
            # both explicit rules, with and without a filter
            for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300)):
                obs, rows = reference_rows(H, ichr, qs, qe, ctg_len, 7, 11, mode, NOV if vf is None else vf, rule)
                ps = igd_amd.permute_host(path, ichr, qs, qe, ctg_len, 7, 11, mode, rule=rule, value_filter=vf)
                check_result(ps, obs, rows, (mode, rule, vf))
                assert obs[:-1].any() and obs[-1] >= obs[:-1].max()
        assert moved > 0, "no permuted count differs from the observed one: the fixture is vacuous"
        # no region: every permuted value is 0 against observed 0
        e = np.zeros(0, np.int32)
        ps = igd_amd.permute_host(path, e, e, e, ctg_len, 4)
        assert not ps.observed.any() and not ps.sum.any() and not ps.sumsq.any() and not ps.min.any() and not ps.max.any()
        assert (ps.n_ge == 4).all() and (ps.n_le == 4).all() and len(ps.observed) == nfiles + 1
    finally:
        H.close()


def test_one_region_and_fewer_rows_than_threads(tmp, host_threads):
    """one region; one permutation of 4500 regions on three threads: 4500 region rows are worth three threads, and only one row
    is there to share out"""
    import igd_amd
    rng = random.Random(77)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[1]
    path, span = clustered_db(rng, tmp, "few", nbp, gtype, nfiles, nctg, span_tiles)
    ctg_len = np.full(nctg, span + 2 * nbp, np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 4500)
    k = int(np.flatnonzero((ichr >= 0) & (ichr < nctg))[0])
    host_threads("3")
    H = HostDb(path)
    try:
        for mode in MODES:
            for c, s, e, nperm in ((ichr[k:k + 1], qs[k:k + 1], qe[k:k + 1], 3), (ichr, qs, qe, 1)):
                obs, rows = reference_rows(H, c, s, e, ctg_len, nperm, 8, mode, NOV, FLAT)
                check_result(igd_amd.permute_host(path, c, s, e, ctg_len, nperm, 8, mode, rule=FLAT), obs, rows, (mode, nperm))
            assert obs[:-1].any() and rows.any()
    finally:
        H.close()


def test_permute_host_refuses_what_the_engine_refuses(tmp):
    import igd_amd
    from igd_amd.database import IgdError
    path, span = clustered_db(random.Random(1), tmp, "r", 1 << 12, 1, 4, 2, 8)
    L = np.array([5000, 0], np.int32)
    ok = (np.zeros(3, np.int32), np.array([0, 10, 4999], np.int32), np.array([5, 10, 5000], np.int32))
    assert igd_amd.permute_host(path, *ok, L, 2).nperm == 2
    for ichr, qs, qe in (([0], [10], [9]), ([0], [-1], [5]), ([0], [4000], [5001]), ([1], [0], [0])):
        with pytest.raises(IgdError):
            igd_amd.permute_host(path, ichr, qs, qe, L, 2)
    for nperm in (0, -3, 2 ** 20 + 1):
        with pytest.raises(IgdError):
            igd_amd.permute_host(path, *ok, L, nperm)
    with pytest.raises(IgdError):
        igd_amd.permute_host(path, *ok, L, 2, mode="rigid")
    with pytest.raises(IgdError):
        igd_amd.permute_host(path, *ok, L[:1], 2)
    # a region on an unknown contig is not validated
    assert igd_amd.permute_host(path, [-1, 7], [9, -5], [3, -50], L, 2).nperm == 2


def test_summary_equals_numpy():
    import igd_amd
    from igd_amd.database import PermutationSupport
    rs = np.random.default_rng(3)
    for P, hi in ((2, 10), (7, 1000), (1000, 100000), (64, 2 ** 24)):
        rows = rs.integers(0, hi, (P, 40)).astype(np.int64)
        rows[:, 5] = 17                                           # all rows equal: sd = 0, z = NaN
        obs = rows[rs.integers(0, P, 40), np.arange(40)].copy()
        obs[::3] += 5
        st = PR.stats(rows, obs)
        got = igd_amd.perm_summary(PermutationSupport(obs, *st, P))
        want = PR.summary(rows, obs)
        for g, w, name in zip(got, want, got._fields):
            assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(w)), name
            ok = ~np.isnan(w)
            rel = np.abs(g[ok] - w[ok]) / np.maximum(np.abs(w[ok]), 1e-300)
            print(P, name, "largest relative difference", rel.max(initial=0))
            assert (g[ok][w[ok] == 0] == 0).all() and (rel[w[ok] != 0] <= 1e-12).all(), name
        flat = (rows == rows[0]).all(axis=0)
        assert flat[5] and got.sd[5] == 0 and np.isnan(got.z[5]) and np.array_equal(np.isnan(got.z), flat) and not flat.all()
    # one permutation: no standard deviation
    rows = rs.integers(0, 50, (1, 6)).astype(np.int64)
    got = igd_amd.perm_summary(PermutationSupport(rows[0], *PR.stats(rows, rows[0]), 1))
    assert np.isnan(got.sd).all() and np.isnan(got.z).all() and np.array_equal(got.mean, rows[0].astype(np.float64))
    assert np.allclose(got.nlog10_p_upper, 0) and np.allclose(got.nlog10_p_lower, 0)
    for name in ("perm_summary", "permute_regions_host", "permute_host"):
        assert name in igd_amd.__all__
