"""The permutation null of the base-pair overlap on the host (igdc_permute_bp_host, igdc_perm_bp_summary;
igd_amd.permute_bp_host / perm_bp_summary).  No GPU.

Expected values never come from the code under test: tests/permute_ref.py's generator composed with tests/jaccard_ref.py's sort,
sweep and boolean arrays over interval lists this test wrote (tests/permute_bp_ref.py), every integer compared exactly; the
placed cases are worked out by hand from the permuted lists; the summary against Python integers, fractions.Fraction and
floats on hand-made matrices, floats to 1e-12 relative -- derived, not measured: the doubles are sums of at most 64 terms, each
addition errs by at most 2^-53 relative, about 7e-15 in all, and the rest is margin.  Outputs are handed over full of 0x5a."""
import random
import shutil

import numpy as np
import pytest

import igd_amd
import igd_amd.database
import permute_bp_ref as PB
import permute_ref as PR
from helpers import short_tmpdir
from jaccard_ref import FLAT, NEST
from nearest_ref import NOV, ListDb, clustered_lists
from test_jaccard_host import cli_rule
from test_support_host import NUMPY_DBS, host_threads  # noqa: F401  (host_threads is a fixture)

RTOL = 1e-12
G64 = 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("ipb")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def fixture_db(workdir, case, nq):
    rng = random.Random(8100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    ldb = ListDb(workdir, "c%d_%d" % (case, nq), files, nbp, gtype)
    ctg_len = np.array([span + 7 * nbp + 13 * c for c in range(nctg)], np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, nq)
    return ldb, ctg_len, ichr, qs, qe


def equal_null(got, want):
    inter, set_bp, n_merged, n_dropped, file_bp = want
    return (got.inter.dtype == np.int64 and np.array_equal(got.inter, inter) and np.array_equal(got.set_bp, set_bp) and
            np.array_equal(got.n_merged, n_merged) and got.n_dropped == n_dropped and np.array_equal(got.file_bp, file_bp))


# ---- placed cases -----------------------------------------------------------------------------------------------------------
def small_db(d, name):
    """two contigs, three records on chrA in two files, one on chrB"""
    return ListDb(d, name, [[("chrA", 100, 200, 900), ("chrA", 5000, 5100, 100)], [("chrB", 10, 20, 900), ("chrA", 150, 300, 900)]], 1 << 14, 1)


def test_a_shift_pushes_two_regions_onto_each_other_at_the_contigs_end(workdir):
    """chrA is 25 bp long; [5, 15) and [15, 25) are book-ended: one run of 20 bp.  A circular shift t moves both; the one that
    would cross the end is pushed back against it and lands on the other: the row's set_bp is 20 minus their overlap."""
    db = small_db(workdir, "push")
    ctg_len = np.array([25, 1000], np.int32)
    ichr, qs, qe = np.array([0, 0], np.int32), np.array([5, 15], np.int32), np.array([15, 25], np.int32)
    nperm = 40
    got = igd_amd.permute_bp_host(db.path, ichr, qs, qe, ctg_len, nperm, seed=3, mode="circular")
    ps, pe = PR.permute(ichr, qs, qe, ctg_len, 0, nperm, 3, PR.CIRCULAR)
    over = np.maximum(0, np.minimum(pe[:, 0], pe[:, 1]).astype(np.int64) - np.maximum(ps[:, 0], ps[:, 1]))
    apart = (np.maximum(ps[:, 0], ps[:, 1]) > np.minimum(pe[:, 0], pe[:, 1]))            # a gap between them: two runs
    assert got.set_bp[0] == 20 and got.n_merged[0] == 1 and got.n_dropped == 0
    assert np.array_equal(got.set_bp[1:], 20 - over) and np.array_equal(got.n_merged[1:], 1 + apart)
    assert (over > 0).any() and (got.set_bp[1:] < got.set_bp[0]).any(), "fixture is vacuous: no shift pushed a region onto the other"
    assert not got.inter.any() or got.inter.max() <= 20


def test_a_zero_length_region_and_an_unknown_contig_are_dropped(workdir):
    db = small_db(workdir, "drop")
    ctg_len = np.array([6000, 1000], np.int32)
    ichr, qs, qe = np.array([0, 0, 7, 0], np.int32), np.array([100, 40, 0, 5000], np.int32), np.array([300, 40, 10, 5100], np.int32)
    for mode in ("circular", "shuffle"):
        got = igd_amd.permute_bp_host(db.path, ichr, qs, qe, ctg_len, 9, seed=1, mode=mode, rule=FLAT)
        assert got.n_dropped == 2 and got.n_merged[0] == 2 and got.set_bp[0] == 300
        # file 0 holds chrA [100, 200) and [5000, 5100); file 1 chrA [150, 300): the set as given covers all of them
        assert got.inter[0].tolist() == [200, 150, 300] and got.file_bp.tolist() == [200, 160, 310]
        assert (got.n_merged[1:] >= 1).all() and (got.n_merged[1:] <= 2).all() and (got.set_bp[1:] <= 300).all() and (got.set_bp[1:] >= 200).all()
        assert equal_null(got, PB.null(db, ichr, qs, qe, ctg_len, 9, 1, mode, None, FLAT))


# ---- the four database shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_equals_the_reference_on_the_four_database_shapes(case, workdir, host_threads):
    ldb, ctg_len, ichr, qs, qe = fixture_db(workdir, case, 120)
    varied = False
    for nperm, threads, n in ((1, "1", 120), (6, "2", 120), (104, "7", 120), (5, "7", 3)):
        host_threads(threads)
        for mode in (PR.CIRCULAR, PR.SHUFFLE):
            for v in (0, 500):
                for rule, ev in (cli_rule(ldb.gtype, v), (FLAT if v == 0 else NEST, NOV)):
                    if nperm == 104 and (v == 0) != (mode == PR.SHUFFLE):             # (104 permutations -- 7 threads want more than 6 x 2048 regions x rows -- on half of the combinations)
                        continue
                    seed = 31 * nperm + v
                    want = PB.null(ldb, ichr[:n], qs[:n], qe[:n], ctg_len, nperm, seed, mode, ev, rule)
                    got = igd_amd.permute_bp_host(ldb.path, ichr[:n], qs[:n], qe[:n], ctg_len, nperm, seed=seed, mode=mode, rule=rule, value_filter=ev)
                    assert got.nperm == nperm and got.inter.shape == (nperm + 1, ldb.nfiles + 1)
                    assert equal_null(got, want), (nperm, threads, mode, v, rule)
                    varied |= len(set(got.set_bp.tolist())) > 1
                    # row 0 is the set as given, row p + 1 the permuted set, each as jaccard_host treats a set
                    js = igd_amd.jaccard_host(ldb.path, ichr[:n], qs[:n], qe[:n], [0, n], rule=rule, value_filter=ev)
                    assert np.array_equal(js.inter[0], got.inter[0]) and js.set_bp[0] == got.set_bp[0] and js.n_merged[0] == got.n_merged[0]
                    assert js.n_dropped[0] == got.n_dropped and np.array_equal(js.file_bp, got.file_bp)
                    ps, pe = igd_amd.permute_regions_host(ichr[:n], qs[:n], qe[:n], ctg_len, 0, nperm, seed=seed, mode=mode)
                    jp = igd_amd.jaccard_host(ldb.path, np.tile(ichr[:n], nperm), ps.reshape(-1), pe.reshape(-1), np.arange(nperm + 1) * n, rule=rule,
                                              value_filter=ev)
                    assert np.array_equal(jp.inter, got.inter[1:]) and np.array_equal(jp.set_bp, got.set_bp[1:])
                    assert np.array_equal(jp.n_merged, got.n_merged[1:]) and (jp.n_dropped == got.n_dropped).all()
                    # the identities
                    assert (got.inter <= np.minimum(got.set_bp[:, None], got.file_bp[None, :])).all()
                    nf = ldb.nfiles
                    assert (got.inter[:, :nf].max(axis=1) <= got.inter[:, nf]).all() and (got.inter[:, nf] <= got.set_bp).all()
    # the CLI's dispatch through v alone
    got = igd_amd.permute_bp_host(ldb.path, ichr, qs, qe, ctg_len, 3, seed=5, v=500)
    rule, ev = cli_rule(ldb.gtype, 500)
    assert equal_null(got, PB.null(ldb, ichr, qs, qe, ctg_len, 3, 5, PR.CIRCULAR, ev, rule))
    assert varied and got.inter.sum() > 0 and got.n_dropped > 0, "fixture is vacuous"


def test_one_region_and_fewer_rows_than_threads(workdir, host_threads):
    """one region; two rows (one permutation) of 2100 regions on three threads: 4200 region rows are worth three threads, and only
    two rows are there to share out"""
    ldb, ctg_len, ichr, qs, qe = fixture_db(workdir, 1, 2100)
    host_threads("3")
    k = int(np.flatnonzero((ichr >= 0) & (ichr < len(ctg_len)) & (qe > qs))[0])
    for mode in (PR.CIRCULAR, PR.SHUFFLE):
        got = igd_amd.permute_bp_host(ldb.path, ichr[k:k + 1], qs[k:k + 1], qe[k:k + 1], ctg_len, 3, seed=4, mode=mode, rule=FLAT)
        assert equal_null(got, PB.null(ldb, ichr[k:k + 1], qs[k:k + 1], qe[k:k + 1], ctg_len, 3, 4, mode, NOV, FLAT)) and got.n_merged.tolist() == [1] * 4
        got = igd_amd.permute_bp_host(ldb.path, ichr, qs, qe, ctg_len, 1, seed=6, mode=mode, rule=FLAT)
        assert equal_null(got, PB.null(ldb, ichr, qs, qe, ctg_len, 1, 6, mode, NOV, FLAT)) and got.inter.all(axis=1).any()


# ---- refusals and empty calls -----------------------------------------------------------------------------------------------
def test_refused_arguments_leave_the_outputs_as_they_were(workdir):
    ldb, ctg_len, ichr, qs, qe = fixture_db(workdir, 0, 20)
    h = igd_amd.database._HostDb(ldb.path, "test")
    try:
        known = np.flatnonzero((ichr >= 0) & (ichr < len(ctg_len)))
        e2 = qe.copy()
        e2[known[0]] = ctg_len[ichr[known[0]]] + 1
        ok = dict(qe=qe, mode=0, nperm=3, rule=FLAT)
        for bad in (dict(nperm=0), dict(nperm=(1 << 20) + 1), dict(mode=2), dict(rule=7), dict(qe=e2)):
            a = dict(ok, **bad)
            inter, sbp, nm, nd = (np.full((4, ldb.nfiles + 1), G64, np.int64), np.full(4, G64, np.int64), np.full(4, G64, np.int64),
                                  np.full(1, G64, np.int64))
            rc = h.L.igdc_permute_bp_host(h.core, h.m, ichr.ctypes.data, qs.ctypes.data, a["qe"].ctypes.data, len(qs), ctg_len.ctypes.data, a["mode"], 0,
                                          a["nperm"], NOV, a["rule"], inter.ctypes.data, sbp.ctypes.data, nm.ctypes.data, nd.ctypes.data)
            assert rc == -1 and all((x == G64).all() for x in (inter, sbp, nm, nd)), bad
    finally:
        h.close()
    from igd_amd.database import IgdError
    for kw in (dict(nperm=0), dict(nperm=(1 << 20) + 1), dict(mode="rotate")):
        with pytest.raises(IgdError):
            igd_amd.permute_bp_host(ldb.path, ichr, qs, qe, ctg_len, kw.get("nperm", 3), mode=kw.get("mode", "circular"))
    with pytest.raises(IgdError):
        igd_amd.permute_bp_host(ldb.path, ichr, qs, e2, ctg_len, 3)
    with pytest.raises(IgdError):
        igd_amd.permute_bp_host(ldb.path, ichr, qs, qe, ctg_len[:1], 3)
    z = np.zeros(0, np.int32)
    got = igd_amd.permute_bp_host(ldb.path, z, z, z, ctg_len, 4)
    assert got.inter.shape == (5, ldb.nfiles + 1) and not got.inter.any() and not got.set_bp.any() and not got.n_merged.any() and got.n_dropped == 0
    assert got.file_bp.sum() > 0
    # every region dropped: rows of nothing
    got = igd_amd.permute_bp_host(ldb.path, [-1, 0], [0, 7], [10, 7], ctg_len, 4)
    assert not got.inter.any() and not got.set_bp.any() and not got.n_merged.any() and got.n_dropped == 2


# ---- the summary ------------------------------------------------------------------------------------------------------------
def check_summary(inter, set_bp, file_bp):
    inter, set_bp, file_bp = np.asarray(inter, np.int64), np.asarray(set_bp, np.int64), np.asarray(file_bp, np.int64)
    got = igd_amd.perm_bp_summary(igd_amd.PermutationBp(inter, set_bp, None, 0, file_bp, inter.shape[0] - 1))
    want = PB.summary(inter, set_bp, file_bp)
    for name in PB.FIELDS:
        g, w = getattr(got, name), want[name]
        if name in PB.INT_FIELDS:
            assert g.dtype == np.int64 and np.array_equal(g, w), (name, g, w)
        else:
            assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(w)), (name, g, w)
            assert np.allclose(g, w, rtol=RTOL, atol=0, equal_nan=True), (name, g, w)
    return got


def test_summary_by_hand():
    # column 0: observed 6 among 2, 6, 10; column 1: all zeros; column 2: a tie of the Jaccards with different integers
    inter = [[6, 0, 2], [2, 0, 4], [6, 0, 1], [10, 0, 3]]
    set_bp, file_bp = [10, 20, 5, 12], [20, 0, 2]
    s = check_summary(inter, set_bp, file_bp)
    assert s.observed.tolist() == [6, 0, 2] and s.mean[0] == 6.0 and s.sd[0] == 4.0 and s.z[0] == 0.0 and s.fold[0] == 1.0
    assert s.n_ge.tolist() == [2, 3, 2] and s.n_le.tolist() == [2, 3, 1]
    assert abs(s.nlog10_p_upper[0] + np.log10(3 / 4)) < 1e-15 and s.nlog10_p_lower[1] == 0.0
    # a column of zeros: the mean is 0, fold is not defined, nor is z; the Jaccard is 0 / set_bp
    assert s.mean[1] == 0 and np.isnan(s.fold[1]) and np.isnan(s.z[1]) and s.jaccard[1] == 0 and s.jaccard_n_ge[1] == 3
    # column 2: observed 2 / (10 + 2 - 2) = 1/5; permuted 4 / 18 = 2/9, 1 / 6, 3 / 11: 2/9 and 3/11 are at least 1/5
    assert s.jaccard[2] == 0.2 and s.jaccard_n_def[2] == 3 and s.jaccard_n_ge[2] == 2
    # column 0: observed 6 / 24 = 1/4; permuted 2 / 38, 6 / 19, 10 / 22
    assert s.jaccard[0] == 0.25 and s.jaccard_n_ge[0] == 2


def test_summary_of_one_permutation_and_ties_and_undefined_ratios():
    s = check_summary([[3, 0], [5, 0]], [9, 9], [4, 0])
    assert np.isnan(s.sd).all() and np.isnan(s.z).all() and s.mean[0] == 5.0 and s.n_ge.tolist() == [1, 1] and s.n_le.tolist() == [0, 1]
    assert np.isnan(s.jaccard_sd).all() and s.jaccard_n_def.tolist() == [1, 1]
    # an observed Jaccard tied with a permuted one -- 2 / 8 and 3 / 12 -- counts; a union of 0 counts on neither side
    s = check_summary([[2, 0], [3, 0], [0, 0], [1, 0]], [6, 9, 0, 4], [4, 0])
    assert s.jaccard[0] == 0.25 and s.jaccard_n_ge[0] == 1 and s.jaccard_n_def.tolist() == [3, 2]
    assert s.jaccard_n_ge[1] == 2 and s.jaccard[1] == 0.0                    # 0 / 6 against 0 / 9 and 0 / 4: ties; 0 / 0 is left out
    # the observed union is 0: nothing is compared
    s = check_summary([[0], [0], [0]], [0, 5, 0], [0])
    assert np.isnan(s.jaccard[0]) and s.jaccard_n_ge[0] == 0 and s.jaccard_n_def[0] == 1 and s.jaccard_mean[0] == 0.0


def test_summary_with_cross_products_beyond_64_bits():
    """x about 3 x 10^9 bp and unions about 10^13: x_p u_0 is about 3 x 10^22 > 2^64, and x^2 alone passes 2^63.  Two permuted
    rows whose Jaccards differ from the observed one by one part in 10^13 on either side: exactly one counts."""
    a, b = 3_000_000_001, 10_000_000_000_003
    up = (a + 1) * b // a                                # (a + 1) / up >= a / b > (a + 1) / (up + 1)
    assert (a + 1) * b >= a * up and (a + 1) * b < a * (up + 1) and (a + 1) * b > 1 << 64
    fbp = 4_000_000_000
    xs, us = [a, a + 1, a + 1, a - 7], [b, up, up + 1, b]
    inter = [[x] for x in xs]
    set_bp = [u - fbp + x for x, u in zip(xs, us)]
    s = check_summary(inter, set_bp, [fbp])
    assert s.jaccard_n_ge[0] == 1 and s.jaccard_n_def[0] == 3 and s.n_ge[0] == 2 and s.n_le[0] == 1
    assert s.sd[0] > 0 and abs(s.mean[0] - (3 * a - 5) / 3) < 1e-3


def test_summary_refuses_bad_shapes():
    from igd_amd.database import IgdError
    with pytest.raises(IgdError):
        igd_amd.perm_bp_summary(igd_amd.PermutationBp(np.zeros((3, 2), np.int64), np.zeros(2, np.int64), None, 0, np.zeros(2, np.int64), 2))
    with pytest.raises(IgdError):
        igd_amd.perm_bp_summary(igd_amd.PermutationBp(np.zeros((3, 2), np.int64), np.zeros(3, np.int64), None, 0, np.zeros(2, np.int64), 0))
