"""Merged region sets and the base-pair Jaccard without a GPU: igdc_merge_host, igdc_dataset_bp_host and igdc_jaccard_host
(igd_hostpath.c) through ctypes and through igd_amd.merge_host / dataset_bp_host / jaccard_host / jaccard_summary.

The expected values never come from the code under test: tests/jaccard_ref.py restates the definitions as a Python sort and
sweep and as boolean arrays over the interval lists this test wrote itself, and the placed cases are written out by hand.  Every
integer must be equal.  Outputs are handed over full of 0x5a."""
import os
import random
import shutil

import numpy as np
import pytest

import igd_amd
import igd_amd.database
from helpers import short_tmpdir
from jaccard_ref import FLAT, MAX_GAP, NEST, jaccard_regions, ref_dataset_bp, ref_jaccard, ref_merge, ref_merge_np
from nearest_ref import NOV, TOP, ListDb, clustered_lists
from test_nearest_host import set_offsets
from test_support_host import NUMPY_DBS

G32, G64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a


@pytest.fixture
def tmp():
    d = short_tmpdir("ijc")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", str(t))
    os.environ.pop("IGD_HOST_THREADS", None)


def _p(a):
    return a.ctypes.data if a.size else None


def cut_merge(out):
    """(rc, the six arrays with the runs cut at m_off[-1], the words behind the last run)"""
    rc, mc, ms, me, moff, cnt, dropped = out
    r = int(moff[-1]) if rc == 0 and len(moff) else 0
    return rc, (mc[:r], ms[:r], me[:r], moff, cnt[:r], dropped), np.concatenate([mc[r:], ms[r:], me[r:], cnt[r:]])


def merge_equal(got, want):
    return all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))


def cli_rule(gtype, v):
    return (FLAT, v) if gtype != 0 and v > 0 else (NEST, NOV)


class JaccardHost:
    """the three host functions through ctypes; every output is handed over full of 0x5a"""

    def __init__(self, path):
        self.h = igd_amd.database._HostDb(path, "test")
        self.L, self.nfiles = self.h.L, self.h.nfiles

    def close(self):
        self.h.close()

    def merge(self, ichr, qs, qe, off, gap=0, want_count=True):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        off = np.ascontiguousarray(off, dtype=np.int64)
        n, nsets = len(qs), len(off) - 1
        mc, ms, me, cnt = (np.full(n, G32, np.int32) for _ in range(4))
        moff, dropped = np.full(nsets + 1, G64, np.int64), np.full(nsets, G64, np.int64)
        rc = self.L.igdc_merge_host(self.h.core, _p(ichr), _p(qs), _p(qe), off.ctypes.data, nsets, gap, _p(mc), _p(ms), _p(me), moff.ctypes.data,
                                    _p(cnt) if want_count else None, _p(dropped))
        return rc, mc, ms, me, moff, cnt, dropped

    def dataset_bp(self, v, rule):
        bp = np.full(self.nfiles + 1, G64, np.int64)
        return self.L.igdc_dataset_bp_host(self.h.core, self.h.m, v, rule, bp.ctypes.data), bp

    def jaccard(self, ichr, qs, qe, off, v, rule):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        off = np.ascontiguousarray(off, dtype=np.int64)
        nsets = len(off) - 1
        inter, fbp = np.full((nsets, self.nfiles + 1), G64, np.int64), np.full(self.nfiles + 1, G64, np.int64)
        sbp, nm, nd = (np.full(nsets, G64, np.int64) for _ in range(3))
        rc = self.L.igdc_jaccard_host(self.h.core, self.h.m, _p(ichr), _p(qs), _p(qe), off.ctypes.data, nsets, v, rule, _p(inter), _p(sbp),
                                      fbp.ctypes.data, _p(nm), _p(nd))
        return rc, (inter, sbp, fbp, nm, nd)


def shape_case(case, tmp, nreg=500):
    rng = random.Random(8100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    db = ListDb(tmp, "j%d" % case, files, nbp, gtype)
    ichr, qs, qe = jaccard_regions(rng, nctg, nbp, span, nreg)
    return db, ichr, qs, qe, set_offsets(rng, nreg)


# ---- the placed cases -------------------------------------------------------------------------------------------------------
def two_contig_db(d, name="jplaced"):
    """two contigs; chrB's tiles run up to 2^31 - 1"""
    return ListDb(d, name, [[("chrA", 100, 200, 900), ("chrA", 5000, 5100, 100)], [("chrB", TOP - 10, TOP, 900), ("chrA", 150, 300, 900)]], 1 << 14, 1)


PLACED = [
    # (what, regions (ichr, qs, qe), set_off, gap, runs (ichr, qs, qe, count), m_off, n_dropped)
    ("book-ended regions join at gap 0", [(0, 0, 10), (0, 10, 20)], [0, 2], 0, [(0, 0, 20, 2)], [0, 1], [0]),
    ("[0,10) and [11,20) stay apart at gap 0", [(0, 0, 10), (0, 11, 20)], [0, 2], 0, [(0, 0, 10, 1), (0, 11, 20, 1)], [0, 2], [0]),
    ("[0,10) and [11,20) join at gap 1", [(0, 0, 10), (0, 11, 20)], [0, 2], 1, [(0, 0, 20, 2)], [0, 1], [0]),
    ("a nested region leaves the end unchanged", [(0, 0, 100), (0, 10, 20), (0, 100, 101)], [0, 3], 0, [(0, 0, 101, 3)], [0, 1], [0]),
    ("a nested region does not shorten the reach", [(0, 0, 100), (0, 10, 20), (0, 50, 60), (0, 101, 110)], [0, 4], 0,
     [(0, 0, 100, 3), (0, 101, 110, 1)], [0, 2], [0]),
    ("identical regions count 2", [(0, 5, 9), (0, 5, 9)], [0, 2], 0, [(0, 5, 9, 2)], [0, 1], [0]),
    ("equal starts with different ends", [(0, 5, 30), (0, 5, 9), (0, 20, 25)], [0, 3], 0, [(0, 5, 30, 3)], [0, 1], [0]),
    ("neighbours in two sets do not join", [(0, 0, 10), (0, 5, 20)], [0, 1, 2], 0, [(0, 0, 10, 1), (0, 5, 20, 1)], [0, 1, 2], [0, 0]),
    ("neighbours on two contigs do not join", [(0, 0, 10), (1, 5, 20)], [0, 2], 0, [(0, 0, 10, 1), (1, 5, 20, 1)], [0, 2], [0]),
    ("an end at INT32_MAX under gap 2^30 does not wrap", [(1, 5, TOP), (1, TOP - 1, TOP), (0, 0, 1), (0, MAX_GAP + 1, MAX_GAP + 2), (0, MAX_GAP + 2, TOP)],
     [0, 5], MAX_GAP, [(0, 0, TOP, 3), (1, 5, TOP, 2)], [0, 2], [0]),
    ("one past gap 2^30 opens a run", [(0, 0, 1), (0, MAX_GAP + 2, MAX_GAP + 3)], [0, 2], MAX_GAP, [(0, 0, 1, 1), (0, MAX_GAP + 2, MAX_GAP + 3, 1)], [0, 2], [0]),
    ("dropped regions are counted", [(-1, 0, 10), (0, 7, 7), (0, 9, 3), (2, 0, 10), (99, 0, 10), (0, 1, 2)], [0, 6], 0, [(0, 1, 2, 1)], [0, 1], [5]),
    ("a set that merges to nothing, between two that do not", [(0, 0, 5), (-1, 0, 10), (0, 7, 7), (1, 3, 4)], [0, 1, 3, 3, 4], 0,
     [(0, 0, 5, 1), (1, 3, 4, 1)], [0, 1, 1, 1, 2], [0, 2, 0, 0]),
    ("unordered input", [(1, 50, 60), (0, 30, 40), (1, 10, 55), (0, 35, 36), (0, 0, 1)], [0, 5], 0, [(0, 0, 1, 1), (0, 30, 40, 2), (1, 10, 60, 2)], [0, 3], [0]),
]


def placed_arrays(case):
    _, regs, off, gap, runs, moff, dropped = case
    a, r = np.array(regs, np.int64).reshape(-1, 3), np.array(runs, np.int64).reshape(-1, 4)
    want = (r[:, 0].astype(np.int32), r[:, 1].astype(np.int32), r[:, 2].astype(np.int32), np.array(moff, np.int64), r[:, 3].astype(np.int32),
            np.array(dropped, np.int64))
    return (a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32), np.array(off, np.int64), gap), want


@pytest.mark.parametrize("case", PLACED, ids=[c[0] for c in PLACED])
def test_the_reference_gives_the_placed_cases(case):
    (ichr, qs, qe, off, gap), want = placed_arrays(case)
    assert merge_equal(ref_merge(2, ichr, qs, qe, off, gap), want)


def test_the_numpy_reference_equals_the_python_reference(tmp):
    """ref_merge_np (the vectorised form the production-size device cases are checked against) gives ref_merge's six arrays, types
    included: on the placed cases, which it must also give as written out by hand, and on the four database shapes under four gaps"""
    for case in PLACED:
        (ichr, qs, qe, off, gap), want = placed_arrays(case)
        got = ref_merge_np(2, ichr, qs, qe, off, gap)
        assert merge_equal(got, want) and merge_equal(got, ref_merge(2, ichr, qs, qe, off, gap)), case[0]
    for case in range(len(NUMPY_DBS)):
        db, ichr, qs, qe, off = shape_case(case, tmp)
        for gap in (0, 1, 300, MAX_GAP):
            want = ref_merge(len(db.ctgs), ichr, qs, qe, off, gap)
            assert len(want[0]) > 0 and want[5].sum() > 0 and want[4].max() > 1          # (the inputs have runs, joined regions and dropped ones)
            assert merge_equal(ref_merge_np(len(db.ctgs), ichr, qs, qe, off, gap), want), (case, gap)
    none = ref_merge_np(2, [5, 0], [1, 9], [2, 9], [0, 0, 2, 2], 0)
    assert merge_equal(none, ref_merge(2, [5, 0], [1, 9], [2, 9], [0, 0, 2, 2], 0)) and none[3].tolist() == [0, 0, 0, 0] and none[5].tolist() == [0, 2, 0]


def test_placed_cases_on_the_host_route(tmp, host_threads):
    H = JaccardHost(two_contig_db(tmp).path)
    try:
        for threads in (1, 2):
            host_threads(threads)
            for case in PLACED:
                (ichr, qs, qe, off, gap), want = placed_arrays(case)
                rc, got, rest = cut_merge(H.merge(ichr, qs, qe, off, gap))
                assert rc == 0 and merge_equal(got, want), case[0]
                assert (rest == 0).all(), case[0]
        rc, got, _ = cut_merge(H.merge(*placed_arrays(PLACED[0])[0], want_count=False))
        assert rc == 0 and (got[4] == G32).all() and got[3].tolist() == [0, 1]
    finally:
        H.close()


def test_refused_arguments_write_nothing(tmp):
    path = two_contig_db(tmp).path
    H = JaccardHost(path)
    try:
        c, s, e = [0, 0], [0, 5], [10, 20]
        for off, gap in (([0, 2], -1), ([0, 2], MAX_GAP + 1), ([1, 2], 0), ([0, 2, 1], 0)):
            out = H.merge(c, s, e, off, gap)
            assert out[0] == -1
            assert all((a == G32).all() for a in (out[1], out[2], out[3], out[5])) and (out[4] == G64).all() and (out[6] == G64).all()
        rc, js = H.jaccard(c, s, e, [1, 2], NOV, NEST)
        assert rc == -1 and all((a == G64).all() for a in js)
        assert H.jaccard(c, s, e, [0, 2], NOV, 7)[0] == -1 and H.dataset_bp(NOV, 7)[0] == -1
        for bad in (-1, 1.5, True, MAX_GAP + 1):
            with pytest.raises(igd_amd.database.IgdError):
                igd_amd.merge_host(path, c, s, e, [0, 2], gap=bad)
    finally:
        H.close()


# ---- the four database shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_route_equals_the_reference_on_the_four_database_shapes(case, tmp, host_threads):
    db, ichr, qs, qe, off = shape_case(case, tmp)
    nctg = len(db.ctgs)
    H = JaccardHost(db.path)
    try:
        for threads in (1, 2, 7):
            host_threads(threads)
            for gap in (0, 1, 300, MAX_GAP):
                rc, got, rest = cut_merge(H.merge(ichr, qs, qe, off, gap))
                assert rc == 0 and merge_equal(got, ref_merge(nctg, ichr, qs, qe, off, gap)) and (rest == 0).all(), (threads, gap)
            for v in (0, 500):
                rule, ev = cli_rule(db.gtype, v)
                want = ref_jaccard(db, ichr, qs, qe, off, ev, rule)
                rc, got = H.jaccard(ichr, qs, qe, off, ev, rule)
                assert rc == 0 and all(np.array_equal(g, w) for g, w in zip(got, want)), (threads, v)
                rc, bp = H.dataset_bp(ev, rule)
                assert rc == 0 and np.array_equal(bp, ref_dataset_bp(db, ev))
        inter, set_bp, file_bp = got[0], got[1], got[2]
        assert inter.sum() > 0 and (got[4] > 0).any() and (got[3] > 0).any()
        # through the public functions, and the identities
        m = igd_amd.merge_host(db.path, ichr, qs, qe, off, gap=0)
        assert merge_equal(m, ref_merge(nctg, ichr, qs, qe, off, 0))
        js = igd_amd.jaccard_host(db.path, ichr, qs, qe, off, v=500)
        assert all(np.array_equal(g, w) for g, w in zip(js, got))
        assert np.array_equal(igd_amd.dataset_bp_host(db.path, v=500), file_bp)
        assert (inter <= np.minimum(set_bp[:, None], file_bp[None, :])).all()
        nf = db.nfiles
        assert file_bp[:nf].max() <= file_bp[nf] <= file_bp[:nf].sum()
        again = igd_amd.merge_host(db.path, m[0], m[1], m[2], m[3], gap=0)          # merging a merged set is the identity
        assert merge_equal(again[:4], m[:4]) and (again[4] == 1).all() and (again[5] == 0).all()
        rule, ev = cli_rule(db.gtype, 500)
        cov = np.zeros((len(off) - 1, nf), np.int64)
        for k in range(len(off) - 1):
            a, b = int(m[3][k]), int(m[3][k + 1])
            assert H.L.igdc_coverage_host(H.h.core, H.h.m, _p(m[0][a:b]), _p(m[1][a:b]), _p(m[2][a:b]), b - a, ev, rule, cov[k].ctypes.data, None) == 0
        assert np.array_equal(cov, inter[:, :nf])
        # a permuted input gives the same output
        perm = np.concatenate([int(off[k]) + np.random.RandomState(k).permutation(int(off[k + 1] - off[k])) for k in range(len(off) - 1)]).astype(np.int64)
        assert merge_equal(igd_amd.merge_host(db.path, ichr[perm], qs[perm], qe[perm], off, gap=0), m)
    finally:
        H.close()


def test_no_sets_and_empty_sets(tmp):
    db = two_contig_db(tmp)
    H = JaccardHost(db.path)
    try:
        rc, js = H.jaccard([], [], [], [0], NOV, NEST)
        assert rc == 0 and np.array_equal(js[2], ref_dataset_bp(db)) and js[2].tolist() == [200, 160, 310]
        rc, js = H.jaccard([], [], [], [0, 0, 0], NOV, NEST)
        assert rc == 0 and not js[0].any() and not js[1].any() and not js[3].any() and not js[4].any()
        rc, got, _ = cut_merge(H.merge([], [], [], [0, 0]))
        assert rc == 0 and got[3].tolist() == [0, 0] and got[5].tolist() == [0]
        rc, bp = H.dataset_bp(500, FLAT)
        assert rc == 0 and bp.tolist() == [100, 160, 210]
    finally:
        H.close()


def test_jaccard_summary_by_hand():
    js = igd_amd.JaccardSets(np.array([[5, 0, 0], [0, 0, 0]], np.int64), np.array([10, 0], np.int64), np.array([20, 0, 7], np.int64), None, None)
    j, sf, ff = igd_amd.jaccard_summary(js)
    assert j[0, 0] == 5 / 25 and j[0, 1] == 0 and np.isnan(j[1, 1]) and j[1, 2] == 0
    assert sf[0, 0] == 0.5 and np.isnan(sf[1]).all() and ff[0, 0] == 0.25 and np.isnan(ff[:, 1]).all()
    assert igd_amd.jaccard is not igd_amd.jaccard_summary
