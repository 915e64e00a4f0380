"""The permutation null of the nearest-record distances on the host (igdc_permute_nearest_host, igdc_perm_nearest_summary;
igd_amd.permute_nearest_host / perm_nearest_summary).  No GPU.

Expected values never come from the code under test: tests/permute_ref.py's generator composed with tests/nearest_ref.py's
definition over interval lists this test wrote (tests/permute_nearest_ref.py), every integer compared exactly; the summary
against numpy float64 on hand-made matrices, floats to 1e-12 relative -- derived, not measured: 64 sequential double additions
err by at most 64 x 2^-53, about 7e-15, and the rest is margin."""
import random
import shutil

import numpy as np
import pytest

import igd_amd
import permute_nearest_ref as PN
import permute_ref as PR
from helpers import short_tmpdir
from nearest_ref import MAX_WINDOW, ListDb, clustered_lists
from test_support_host import FLAT, NUMPY_DBS, host_threads  # noqa: F401  (host_threads is a fixture)

RTOL = 1e-12


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("ipn")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def fixture_db(workdir, case, nq):
    rng = random.Random(8100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    ldb = ListDb(workdir, "c%d_%d" % (case, nq), files, nbp, gtype)
    ctg_len = np.array([span + 7 * nbp + 13 * c for c in range(nctg)], np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, nq)
    return ldb, nbp, ctg_len, ichr, qs, qe


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_equals_the_numpy_composition(case, workdir, host_threads):
    """both modes, the filter on and off, W in {0, 1, nbp, 2^30}, 1, 5 and 64 permutations on 1, 2 and 7 threads (7 threads want
    more than 6 x 2048 regions x rows: 200 regions x 65 rows)"""
    ldb, nbp, ctg_len, ichr, qs, qe = fixture_db(workdir, case, 200)
    far = False
    for nperm, threads, n in ((1, "1", 200), (5, "2", 200), (64, "7", 200), (5, "7", 3)):
        host_threads(threads)
        for mode in (PR.CIRCULAR, PR.SHUFFLE):
            for v in (None, 500):
                for W in (0, 1, nbp, MAX_WINDOW):
                    if nperm == 64 and (W == 1) != (mode == PR.SHUFFLE):       # (64 permutations: half of the combinations)
                        continue
                    seed = 17 * nperm + W % 5
                    want = PN.null(ldb, ichr[:n], qs[:n], qe[:n], ctg_len, nperm, W, seed, mode, v)
                    got = igd_amd.permute_nearest_host(ldb.path, ichr[:n], qs[:n], qe[:n], ctg_len, nperm, W, seed=seed, mode=mode,
                                                       value_filter=v)
                    assert got.nperm == nperm and got.window == W
                    for g, w in zip(got[:3], want):
                        assert g.dtype == np.int64 and g.shape == (nperm + 1, ldb.nfiles + 1) and np.array_equal(g, w), (nperm, mode, v, W)
                    far |= bool((got.sum_dist[1:] > 0).any())
                    # row 0 is the set as given
                    ns = igd_amd.nearest_sets_host(ldb.path, ichr[:n], qs[:n], qe[:n], [0, n], W, value_filter=v)
                    for g, w in zip(got[:3], ns[:3]):
                        assert np.array_equal(g[0], w[0])
                    if W == 0:
                        # n_within at W = 0 is the support under rule FLAT: the permuted rows against permute_host's statistics
                        assert np.array_equal(got.n_within, got.n_overlap) and not got.sum_dist.any()
                        vf = igd_amd._native.IGD_HIP_NO_VALUE_FILTER if v is None else v
                        ps = igd_amd.permute_host(ldb.path, ichr[:n], qs[:n], qe[:n], ctg_len, nperm, seed=seed, mode=mode, rule=FLAT,
                                                  value_filter=vf)
                        rows = got.n_within[1:]
                        assert np.array_equal(ps.observed, got.n_within[0]) and np.array_equal(ps.sum, rows.sum(axis=0))
                        assert np.array_equal(ps.min, rows.min(axis=0)) and np.array_equal(ps.max, rows.max(axis=0))
                        assert np.array_equal(ps.sumsq, (rows * rows).sum(axis=0))
    assert far, "fixture is vacuous: no permuted region lies at a distance"


def test_one_region_and_fewer_rows_than_threads(workdir, host_threads):
    """one region; two rows (one permutation) of 2100 regions on three threads: 4200 region rows are worth three threads, and only
    two rows are there to share out"""
    ldb, nbp, ctg_len, ichr, qs, qe = fixture_db(workdir, 1, 2100)
    host_threads("3")
    k = int(np.flatnonzero((ichr >= 0) & (ichr < len(ctg_len)))[0])
    for mode in (PR.CIRCULAR, PR.SHUFFLE):
        for c, s, e, nperm in ((ichr[k:k + 1], qs[k:k + 1], qe[k:k + 1], 3), (ichr, qs, qe, 1)):
            want = PN.null(ldb, c, s, e, ctg_len, nperm, nbp, 9, mode, None)
            got = igd_amd.permute_nearest_host(ldb.path, c, s, e, ctg_len, nperm, nbp, seed=9, mode=mode)
            for g, w in zip(got[:3], want):
                assert g.shape == (nperm + 1, ldb.nfiles + 1) and np.array_equal(g, w), (mode, nperm)
        assert got.n_within[1].any()


def test_refused_arguments_and_empty_calls(workdir):
    from igd_amd.database import IgdError
    ldb, nbp, ctg_len, ichr, qs, qe = fixture_db(workdir, 0, 20)
    ok = dict(nperm=3, window=100)
    for bad in (dict(nperm=0), dict(nperm=(1 << 20) + 1), dict(window=-1), dict(window=MAX_WINDOW + 1), dict(mode="rotate")):
        a = dict(ok, **bad)
        with pytest.raises(IgdError):
            igd_amd.permute_nearest_host(ldb.path, ichr, qs, qe, ctg_len, a["nperm"], a["window"], mode=a.get("mode", "circular"))
    known = np.flatnonzero((ichr >= 0) & (ichr < len(ctg_len)))
    e2 = qe.copy()
    e2[known[0]] = ctg_len[ichr[known[0]]] + 1
    with pytest.raises(IgdError):
        igd_amd.permute_nearest_host(ldb.path, ichr, qs, e2, ctg_len, 3, 100)
    with pytest.raises(IgdError):
        igd_amd.permute_nearest_host(ldb.path, ichr, qs, qe, ctg_len[:1], 3, 100)
    z = np.zeros(0, np.int32)
    got = igd_amd.permute_nearest_host(ldb.path, z, z, z, ctg_len, 4, 100)
    assert all(a.shape == (5, ldb.nfiles + 1) and not a.any() for a in got[:3])


# ---- the summary ------------------------------------------------------------------------------------------------------------
def check_summary(nw, sd):
    nw, sd = np.asarray(nw, np.int64), np.asarray(sd, np.int64)
    got = igd_amd.perm_nearest_summary(igd_amd.PermutationNearest(nw, None, sd, 0, nw.shape[0] - 1))
    want = PN.summary(nw, sd)
    for name in PN.FIELDS:
        g, w = getattr(got, name), want[name]
        if name in PN.INT_FIELDS:
            assert g.dtype == np.int64 and np.array_equal(g, w), (name, g, w)
        else:
            assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(w)), (name, g, w)
            assert np.allclose(g, w, rtol=RTOL, atol=0, equal_nan=True), (name, g, w)
    return got


def test_summary_on_hand_made_matrices():
    #            observed row, then four permutations; columns:
    #   0  ordinary               1  nw_0 = 0               2  all nw_p = 0 (n_def 0)    3  n_def = 1
    #   4  n_def = 2              5  ties everywhere        6  all permuted means equal (sd 0)
    nw = [[5, 0, 4, 3, 3, 2, 6],
          [4, 2, 0, 0, 0, 2, 3],
          [6, 0, 0, 7, 5, 2, 3],
          [5, 3, 0, 0, 0, 2, 6],
          [2, 1, 0, 0, 2, 2, 9]]
    sd = [[50, 0, 40, 9, 9, 10, 60],
          [44, 8, 0, 0, 0, 10, 15],
          [30, 0, 0, 21, 25, 10, 15],
          [75, 9, 0, 0, 0, 10, 30],
          [20, 5, 0, 0, 6, 10, 45]]
    got = check_summary(nw, sd)
    assert got.n_def.tolist() == [4, 3, 0, 1, 2, 4, 4]
    assert np.isnan(got.mean_dist[1]) and np.isnan(got.dist_z[1]) and got.dist_n_le[1] == 0
    assert np.isnan(got.dist_mean[2]) and np.isnan(got.dist_sd[2]) and got.dist_n_le[2] == 0 and got.within_n_ge[2] == 0
    assert not np.isnan(got.dist_mean[3]) and np.isnan(got.dist_sd[3]) and np.isnan(got.dist_z[3])
    assert not np.isnan(got.dist_sd[4]) and got.dist_n_le[5] == 4 and got.within_n_ge[5] == 4 and np.isnan(got.within_z[5])
    assert got.dist_sd[6] == 0 and np.isnan(got.dist_z[6]) and got.dist_n_le[0] == 2


def test_summary_with_one_permutation_and_random_matrices():
    got = check_summary([[3, 0], [2, 4]], [[30, 0], [10, 4]])
    assert np.isnan(got.within_sd).all() and np.isnan(got.within_z).all() and np.isnan(got.dist_sd).all()
    rng = np.random.RandomState(5)
    for P in (2, 5, 64):
        nw = rng.randint(0, 50, size=(P + 1, 9)).astype(np.int64)
        nw[:, 0] = rng.randint(0, 2, size=P + 1)
        sd = nw * rng.randint(0, 1000, size=nw.shape)
        check_summary(nw, sd)


def test_summary_compares_the_ratios_exactly():
    """sd / nw as doubles is the same number for the observed row and both permutations (2^62 + 1 and 2^62 + 2 round to 2^62), the
    integers differ: sd_p nw_0 <= sd_0 nw_p holds for the first permutation only.  The products are near 2^82: only 128-bit
    arithmetic gets it right."""
    big, n = 1 << 62, (1 << 20) + 1
    nw = [[n, n], [n, n - 1], [n, n]]
    sd = [[big + 1, big], [big, big], [big + 2, big + 1]]
    assert float(big + 1) / n == float(big) / n == float(big + 2) / n
    got = check_summary(nw, sd)
    # column 1: (2^62) n <= (2^62)(n - 1) is false; (2^62 + 1) n <= 2^62 n is false
    assert got.dist_n_le.tolist() == [1, 0]
