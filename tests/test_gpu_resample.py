"""GPU: permutation nulls by resampling from a universe (kernel igd_resample_regions; igd_hip_resample_regions and the three
igd_hip_permute_*_rs drivers; Database.resample_regions and mode="resample" of permutation_support / _nearest / _bp; `igd search
-P -M resample -U` on the engine route).

The kernel is held against resample_ref (THE DRAW of include/igd_hip.h in numpy uint64) through its generic entry; each null
against the statistics that Database.support_sets / nearest_sets / jaccard_sets give for resample_ref's explicit lists, and against
the host twin.  Every integer must be EQUAL.  Every output is handed to the engine full of garbage."""
import ctypes as C
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import permute_ref as PR
import resample_ref as RR
from helpers import ROOT, short_tmpdir
from test_permute_host import check_result
from test_resample_cli import rfx  # noqa: F401  (the command line fixture: database, set file, universe file)
from test_resample_host import BIG_SEED, hypergeometric_deviations, hypergeometric_fixture, pool_of
from test_support_host import FLAT, HOST, NEST, NOV, _run, clustered_db

pytestmark = pytest.mark.gpu
ENGINE = {"IGD_HOST_MAX_QUERIES": "0"}
G32, G64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a


def H():
    from igd_amd import _native as N
    return N.hip()


def ptr(a):
    return a.ctypes.data if a.size else None


def make_db(d, name="r", npool=300, nq=100, seed=47):
    """a clustered database of 40 files on 3 contigs, a universe on them (unknown contigs and zero-length regions included) and a
    set that is not a subset of it"""
    from igd_amd import Database
    rng = random.Random(seed)
    path, span = clustered_db(rng, d, name, 1 << 12, 1, 40, 3, 12)
    ctg_len = np.array([span // 2, span // 2 + 1234, span // 3], np.int32)
    return dict(path=path, db=Database(path), pool=PR.random_regions(rng, ctg_len, npool), reg=PR.random_regions(rng, ctg_len, nq))


@pytest.fixture(scope="module")
def dbfx():
    d = short_tmpdir("igr")
    fx = make_db(d)
    yield fx
    fx["db"].close()
    shutil.rmtree(d, ignore_errors=True)


# ---- igd_resample_regions -----------------------------------------------------------------------------------------------------
def raw_resample(db, pool, nq, p0, n, seed):
    """igd_hip_resample_regions into arrays full of garbage: (rc, ichr, qs, qe)"""
    pool = [np.ascontiguousarray(a, np.int32) for a in pool]
    out = [np.full((n, nq), G32, np.int32) for _ in range(3)]
    rc = H().igd_hip_resample_regions(db.dev, *[ptr(a) for a in pool], len(pool[1]), nq, seed, p0, n, *[ptr(a) for a in out])
    return (rc, *out)


def check_draws(db, pool, nq, p0, n, seed):
    want = RR.resample_regions(pool, nq, p0, n, seed)
    rc, *got = raw_resample(db, pool, nq, p0, n, seed)
    assert rc == 0, H().igd_hip_last_error()
    for g, w in zip(got, want):
        assert np.array_equal(g, w), (len(pool[1]), nq, p0, n, seed)
    return got


@pytest.mark.parametrize("npool", [1, 2, 4, 5, 16, 17, 4096, 4097, 65537])
def test_resample_regions_equals_the_reference(dbfx, npool):
    """pools on each side of a change of h, at domains exactly n and almost 4 n; nq == npool and nq == 1; seeds 0, 2^64 - 1 and a
    large one; p0 > 0 up to 2^20 - 2"""
    pool = pool_of(npool)
    for seed, p0, nq, n in ((0, 0, npool, 3), (2 ** 64 - 1, 5, 1, 4), (BIG_SEED, 2 ** 20 - 2, npool, 2), (7, 1, max(npool // 3, 1), 2)):
        got = check_draws(dbfx["db"], pool, nq, p0, n, seed)
        for k in range(n):                                  # (the fixture's starts are all different)
            assert len(set(got[1][k].tolist())) == nq
    got = dbfx["db"].resample_regions(*pool, 1, 5, 4, 2 ** 64 - 1)
    assert got[0].shape == (4, 1) and np.array_equal(got[1], RR.resample_regions(pool, 1, 5, 4, 2 ** 64 - 1)[1])


def test_resample_regions_sizes_and_many_contigs(dbfx):
    """np * nq of 1, 255, 256, 257 -- one lane, a workgroup less one, exactly one, a second one -- and one above
    256 * igd_hip_permute_grid(n): a lane's second output, with a change of permutation between a lane's outputs.  A pool over 150
    contigs with unknown contigs (-1, 150) in it."""
    pool = pool_of(1500)
    assert len(set(pool[0].tolist())) > 100 and -1 in pool[0] and 150 in pool[0]
    grid = int(H().igd_hip_permute_grid(1 << 30))
    big = 256 * grid // 1021 + 1
    assert big * 1021 > 256 * grid and int(H().igd_hip_permute_grid(big * 1021)) == grid and int(H().igd_hip_permute_grid(257)) == 2
    for nq, n, p0 in ((1, 1, 0), (255, 1, 3), (51, 5, 1000), (256, 1, 7), (64, 4, 2), (257, 1, 1), (1021, big, 9)):
        check_draws(dbfx["db"], pool, nq, p0, n, 42)
    assert dbfx["db"].resample_regions(*pool, 0, 0, 3)[0].shape == (3, 0)
    assert dbfx["db"].resample_regions(*pool, 5, 0, 0)[0].shape == (0, 5)


def test_resample_regions_equals_the_host_twin(dbfx):
    import igd_amd
    pool = pool_of(4097)
    a, b = dbfx["db"].resample_regions(*pool, 4097, 3, 2, BIG_SEED), igd_amd.resample_regions_host(*pool, 4097, 3, 2, BIG_SEED)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the three drivers against their compositions ---------------------------------------------------------------------------
def as_sets(fx, nperm, seed):
    """the nperm + 1 rows as concatenated sets from resample_ref; Database.resample_regions draws the same lists"""
    sets = RR.resample_sets(fx["reg"], fx["pool"], nperm, seed)
    nq = len(fx["reg"][1])
    got = fx["db"].resample_regions(*fx["pool"], nq, 0, nperm, seed)
    for g, w in zip(got, sets[:3]):
        assert np.array_equal(g.reshape(-1), w[nq:])
    return sets


@pytest.mark.parametrize("nperm", [1, 5, 64])
def test_support_driver_equals_its_composition(dbfx, nperm):
    db, reg, pool = dbfx["db"], dbfx["reg"], dbfx["pool"]
    sets = as_sets(dbfx, nperm, 3)
    for kw in ({}, dict(rule=NEST), dict(rule=FLAT, value_filter=300), dict(rule=FLAT, min_overlap=40)):
        sup, nhit = db.support_sets(*sets, **kw)
        rows = np.concatenate([sup, nhit[:, None]], axis=1).astype(np.int64)
        got = db.permutation_support(*reg, None, nperm, 3, "resample", universe=pool, **kw)
        check_result(got, rows[0], rows[1:], (nperm, kw))
    assert rows[0][:-1].any() and (rows[1:] != rows[0][None, :]).any()


@pytest.mark.parametrize("nperm", [1, 5, 64])
def test_nearest_driver_equals_its_composition(dbfx, nperm):
    db, reg, pool = dbfx["db"], dbfx["reg"], dbfx["pool"]
    sets = as_sets(dbfx, nperm, 3)
    for window, vf in ((0, None), (500, None), (100000, 300)):
        want = db.nearest_sets(*sets, window, vf)
        out = [np.full((nperm + 1, db.nfiles + 1), G64, np.int64) for _ in range(3)]
        got = db.permutation_nearest(*reg, None, nperm, window, 3, "resample", vf, out=out, universe=pool)
        for k in ("n_within", "n_overlap", "sum_dist"):
            assert np.array_equal(getattr(got, k), getattr(want, k)), (k, nperm, window)
    assert got.n_within.any()


@pytest.mark.parametrize("nperm", [1, 5, 64])
def test_bp_driver_equals_its_composition(dbfx, nperm):
    db, reg, pool = dbfx["db"], dbfx["reg"], dbfx["pool"]
    sets = as_sets(dbfx, nperm, 3)
    for kw in ({}, dict(rule=NEST), dict(rule=FLAT, value_filter=300)):
        want = db.jaccard_sets(*sets, **kw)
        got = db.permutation_bp(*reg, None, nperm, 3, "resample", universe=pool, **kw)
        assert np.array_equal(got.inter, want.inter) and np.array_equal(got.set_bp, want.set_bp) and np.array_equal(got.n_merged, want.n_merged)
        assert got.n_dropped == int(want.n_dropped[0]) and np.array_equal(got.file_bp, want.file_bp)
    assert got.inter.any() and (nperm == 1 or len(set(want.n_dropped.tolist())) > 1)


def test_the_drivers_equal_the_host_route(dbfx):
    import igd_amd
    db, reg, pool, path = dbfx["db"], dbfx["reg"], dbfx["pool"], dbfx["path"]
    kw = dict(universe=pool)
    a, b = db.permutation_support(*reg, None, 5, 9, "resample", **kw), igd_amd.permute_host(path, *reg, None, 5, 9, "resample", **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a[:7], b[:7]))
    a, b = db.permutation_nearest(*reg, None, 5, 500, 9, "resample", **kw), igd_amd.permute_nearest_host(path, *reg, None, 5, 500, 9, "resample", **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    a, b = db.permutation_bp(*reg, None, 5, 9, "resample", **kw), igd_amd.permute_bp_host(path, *reg, None, 5, 9, "resample", **kw)
    assert all(np.array_equal(x, y) for x, y in zip((a.inter, a.set_bp, a.n_merged, a.file_bp), (b.inter, b.set_bp, b.n_merged, b.file_bp)))
    assert a.n_dropped == b.n_dropped


def test_a_draw_of_the_whole_universe_is_the_universe_in_another_order(dbfx):
    """nq == npool: every permuted row equals the pool's own row, with no reference at all"""
    db, pool = dbfx["db"], dbfx["pool"]
    nperm = 6
    ps = db.permutation_support(*pool, None, nperm, 11, "resample", universe=pool)
    assert ps.observed[:-1].any() and np.array_equal(ps.min, ps.observed) and np.array_equal(ps.max, ps.observed)
    assert np.array_equal(ps.sum, nperm * ps.observed) and np.array_equal(ps.sumsq, nperm * ps.observed ** 2)
    assert (ps.n_ge == nperm).all() and (ps.n_le == nperm).all()
    pb = db.permutation_bp(*pool, None, nperm, 11, "resample", universe=pool)
    assert pb.inter.any() and (pb.inter == pb.inter[0]).all() and (pb.set_bp == pb.set_bp[0]).all() and (pb.n_merged == pb.n_merged[0]).all()
    pn = db.permutation_nearest(*pool, None, nperm, 2000, 11, "resample", universe=pool)
    assert pn.sum_dist.any() and all((x == x[0]).all() for x in pn[:3])


def test_the_support_null_is_hypergeometric_within_six_standard_deviations():
    """npool = 1000, nq = 100, 2000 draws, seed 7: each permuted support of file f is hypergeometric with K_f the pool's support.
    The engine's sums are the host twin's, whose largest deviation on this input is 2.538 standard deviations."""
    import igd_amd
    d = short_tmpdir("igh")
    try:
        fx = hypergeometric_fixture(d)
        db = igd_amd.Database(fx["path"])
        try:
            sup, nhit = db.support(*fx["pool"])
            ps = db.permutation_support(*fx["reg"], None, 2000, 7, "resample", universe=fx["pool"])
        finally:
            db.close()
        dev = hypergeometric_deviations(np.concatenate([sup, [nhit]]), ps, 1000, 100)
        print("hypergeometric deviations: %d columns, largest %.3f sd" % (len(dev), dev.max()))
        assert len(dev) >= 30 and (dev <= 6).all()
        host = igd_amd.permute_host(fx["path"], *fx["reg"], None, 2000, 7, "resample", universe=fx["pool"])
        assert all(np.array_equal(x, y) for x, y in zip(ps[:7], host[:7]))
    finally:
        shutil.rmtree(d, ignore_errors=True)


# ---- chunks of permutations -------------------------------------------------------------------------------------------------
CHUNKS = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_resample as T
from helpers import short_tmpdir
import shutil
d = short_tmpdir("igy")
try:
    fx = T.make_db(d, "c", 300, 100, 47)
    db, reg, pool = fx["db"], fx["reg"], fx["pool"]
    assert len(reg[1]) == 100
    sets = T.as_sets(fx, 7, 6)
    h = hashlib.sha256()
    sup, nhit = db.support_sets(*sets)
    rows = np.concatenate([sup, nhit[:, None]], axis=1).astype(np.int64)
    got = db.permutation_support(*reg, None, 7, 6, "resample", universe=pool)
    T.check_result(got, rows[0], rows[1:], "support")
    for x in got[:7]: h.update(x.tobytes())
    want = db.nearest_sets(*sets, 500)
    got = db.permutation_nearest(*reg, None, 7, 500, 6, "resample", universe=pool)
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])), "nearest"
    for x in got[:3]: h.update(x.tobytes())
    want = db.jaccard_sets(*sets)
    got = db.permutation_bp(*reg, None, 7, 6, "resample", universe=pool)
    assert np.array_equal(got.inter, want.inter) and np.array_equal(got.set_bp, want.set_bp) and np.array_equal(got.n_merged, want.n_merged), "bp"
    for x in (got.inter, got.set_bp, got.n_merged): h.update(x.tobytes())
    db.close()
    print("ok", h.hexdigest())
finally:
    shutil.rmtree(d, ignore_errors=True)
""" % (os.path.join(ROOT, "tests"), ROOT)


def run_chunks(env):
    assert not any(k in os.environ for k in ("IGD_HIP_MAX_BATCH", "IGD_HIP_PERM_ROW_BYTES"))
    p = subprocess.run([sys.executable, "-c", CHUNKS], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env), timeout=600)
    assert p.returncode == 0 and p.stdout.split()[-2:-1] == [b"ok"], p.stderr.decode()[-2000:]
    return p.stdout.split()[-1]


@pytest.fixture(scope="module")
def one_chunk():
    return run_chunks({})


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "300"}, {"IGD_HIP_PERM_ROW_BYTES": str(3 * 40 * 8)}])
def test_chunks_of_permutations(env, one_chunk):
    """100 regions from a universe of 300, 40 files, 7 permutations.  The batch lowered to 300 (the universe still fits): 3 + 3 + 1
    permutations.  The row budget lowered to 3 rows of 40 files: the same cut for the support and the base pairs, one permutation
    per chunk for the distances.  Equal to the one-chunk result (both variables are read once per process)."""
    assert run_chunks(env) == one_chunk


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_callers_arrays_untouched(dbfx):
    import igd_amd
    from igd_amd.database import IgdError
    L_ = H()
    db = dbfx["db"]
    nC, R = db.nfiles + 1, 3
    reg = tuple(np.ascontiguousarray(a[:3], np.int32) for a in dbfx["reg"])
    pool = tuple(np.ascontiguousarray(a[:10], np.int32) for a in dbfx["pool"])
    st = [np.full(nC, G64, np.int64) for _ in range(7)]
    mats = [np.full(R * nC, G64, np.int64) for _ in range(3)]
    small = [np.full(R, G64, np.int64), np.full(R, G64, np.int64), np.full(1, G64, np.int64)]

    def three(reg, nq, pool, npool, nperm=2, window=100, rule=NEST, mo=None):
        a = (db.dev, ptr(reg[0]), ptr(reg[1]), ptr(reg[2]), nq, ptr(pool[0]), ptr(pool[1]), ptr(pool[2]), npool, 0, nperm)
        rcs, msgs = [], []
        for name, call in (("igd_hip_permute_support_rs", lambda: L_.igd_hip_permute_support_rs(*a, NOV, rule, *[ptr(x) for x in st], mo)),
                           ("igd_hip_permute_nearest_rs", lambda: L_.igd_hip_permute_nearest_rs(*a, window, NOV, *[ptr(x) for x in mats])),
                           ("igd_hip_permute_bp_rs", lambda: L_.igd_hip_permute_bp_rs(*a, NOV, rule, ptr(mats[0]), ptr(small[0]), ptr(small[1]),
                                                                                      ptr(small[2])))):
            rcs.append(call())
            msgs.append(L_.igd_hip_last_error())
            assert rcs[-1] == 0 or msgs[-1].startswith(name.encode() + b":"), msgs[-1]
        return tuple(rcs), msgs
    untouched = lambda: all((x == G64).all() for x in st + mats + small)          # noqa: E731
    # nq > npool: the message names both numbers
    rcs, msgs = three(reg, 3, pool, 2)
    assert rcs == (-2, -2, -2) and all(b"3 regions" in m and b"pool of 2" in m for m in msgs) and untouched()
    # the number of permutations comes before the pool
    for nperm in (0, (1 << 20) + 1):
        rcs, msgs = three(reg, 3, pool, 2, nperm=nperm)
        assert rcs == (-2, -2, -2) and all(b"permutations" in m for m in msgs) and untouched()
    # a missing array; the entry's own first check in front of everything
    rcs, msgs = three((reg[0], reg[1], np.zeros(0, np.int32)), 3, pool, 10)
    assert rcs == (-2, -2, -2) and all(b"bad argument" in m for m in msgs) and untouched()
    rcs, msgs = three(reg, 3, (pool[0], np.zeros(0, np.int32), pool[2]), 10)
    assert rcs == (-2, -2, -2) and all(b"bad argument" in m for m in msgs) and untouched()
    rcs, msgs = three(reg, 3, pool, 2, window=-1, rule=77)
    assert rcs == (-2, -2, -2) and b"bad argument" in msgs[0] and b"window -1 outside" in msgs[1] and b"bad argument" in msgs[2] and untouched()
    # the generator alone
    rc, *out = raw_resample(db, pool, 11, 0, 2, 0)
    assert rc == -2 and b"11 regions" in L_.igd_hip_last_error() and b"pool of 10" in L_.igd_hip_last_error() and all((x == G32).all() for x in out)
    rc, *out = raw_resample(db, pool, 3, -1, 2, 0)
    assert rc == -2 and all((x == G32).all() for x in out)
    # mode 4 is no mode of the placing entries, with a workspace or without: there is no pool to draw from
    L = np.array([10 ** 6] * db.nctg, np.int32)
    ws = igd_amd.build_workspace([0], [0], [1000], L)
    r3 = (np.zeros(3, np.int32), np.array([0, 5, 9], np.int32), np.array([10, 50, 19], np.int32))
    for w in (None, ws.ptr):
        a = (db.dev, ptr(r3[0]), ptr(r3[1]), ptr(r3[2]), 3, ptr(L), 4, 0, 2)
        assert L_.igd_hip_permute_support_ws(*a, NOV, NEST, *[ptr(x) for x in st], None, w) == -2
        assert L_.igd_hip_permute_nearest_ws(*a, 100, NOV, *[ptr(x) for x in mats], w) == -2
        assert L_.igd_hip_permute_bp_ws(*a, NOV, NEST, ptr(mats[0]), ptr(small[0]), ptr(small[1]), ptr(small[2]), w) == -2
        os_, oe = np.full((2, 3), G32, np.int32), np.full((2, 3), G32, np.int32)
        assert L_.igd_hip_permute_regions_ws(db.dev, ptr(r3[0]), ptr(r3[1]), ptr(r3[2]), 3, ptr(L), len(L), 4, 0, 0, 2, ptr(os_), ptr(oe), w) == -2
        assert untouched() and (os_ == G32).all() and (oe == G32).all()
    # the calls that are not refused run, and define every word
    rcs, msgs = three(reg, 3, pool, 10)
    assert rcs == (0, 0, 0) and not any((x == G64).any() for x in st + mats + small)
    # the binding: a workspace with the mode, one without the other, contig lengths beside the universe
    for call in (lambda **k: db.permutation_support(*reg, k.pop("L", None), 2, **k), lambda **k: db.permutation_nearest(*reg, k.pop("L", None), 2, 100, **k),
                 lambda **k: db.permutation_bp(*reg, k.pop("L", None), 2, **k)):
        with pytest.raises(ValueError):
            call(mode="resample")
        with pytest.raises(ValueError):
            call(mode="shuffle", universe=pool, L=L)
        with pytest.raises(ValueError):
            call(mode="resample", universe=pool, workspace=ws)
        with pytest.raises(ValueError):
            call(mode="resample", universe=pool, L=L)
        with pytest.raises(IgdError, match="cannot be drawn without replacement from a pool of 2"):
            call(mode="resample", universe=tuple(a[:2] for a in pool))
    with pytest.raises(IgdError, match="igd_hip_resample_regions"):
        db.resample_regions(*pool, 11, 0, 1)


def test_the_refusals_of_the_entries_in_their_order(dbfx):
    """The refusals that need large or odd arguments, each with the outputs' garbage left intact: the support's own first check (an
    out-of-range min_overlap), nq above the batch, the support's nperm * nq^2 >= 2^63.  And the order: the entry's own check before a
    missing argument, nperm before the batch, the batch before npool < nq, npool < nq before 2^63."""
    from igd_amd import MinOverlap
    L_ = H()
    db = dbfx["db"]
    nC, R = db.nfiles + 1, 3
    big = int(L_.igd_hip_max_batch()) + 1
    z = np.zeros(big, np.int32)
    zp = z.ctypes.data
    st = [np.full(nC, G64, np.int64) for _ in range(7)]
    mats = [np.full(R * nC, G64, np.int64) for _ in range(3)]
    small = [np.full(R, G64, np.int64), np.full(R, G64, np.int64), np.full(1, G64, np.int64)]

    def three(nq, npool, nperm, mo=None, rule=NEST):
        a = (db.dev, zp, zp, zp, nq, zp, zp, zp, npool, 0, nperm)
        got = []
        for name, call in (("igd_hip_permute_support_rs", lambda: L_.igd_hip_permute_support_rs(*a, NOV, rule, *[ptr(x) for x in st], mo)),
                           ("igd_hip_permute_nearest_rs", lambda: L_.igd_hip_permute_nearest_rs(*a, 100, NOV, *[ptr(x) for x in mats])),
                           ("igd_hip_permute_bp_rs", lambda: L_.igd_hip_permute_bp_rs(*a, NOV, rule, ptr(mats[0]), ptr(small[0]), ptr(small[1]),
                                                                                      ptr(small[2])))):
            rc = call()
            msg = L_.igd_hip_last_error()
            assert rc == -2 and msg.startswith(name.encode() + b":"), (name, rc, msg)
            got.append(msg)
        assert all((x == G64).all() for x in st + mats + small)
        return got
    # the support's own first check, in front of a missing argument (no such rule), of nperm and of everything behind
    for field, value in (("bp", -1), ("query_ppm", -1), ("record_ppm", -1), ("query_ppm", 10 ** 6 + 1)):
        mo = MinOverlap()
        setattr(mo, field, value)
        for nq, npool, nperm, rule in ((3, 10, 2, NEST), (3, 10, 2, 77), (big, 2, 0, NEST)):
            a = (db.dev, zp, zp, zp, nq, zp, zp, zp, npool, 0, nperm)
            assert L_.igd_hip_permute_support_rs(*a, NOV, rule, *[ptr(x) for x in st], C.byref(mo)) == -2
            msg = L_.igd_hip_last_error()
            assert msg.startswith(b"igd_hip_permute_support_rs: min_overlap") and b"out of range" in msg, msg
            assert all((x == G64).all() for x in st)
    # a missing argument before nperm
    assert all(b"bad argument" in m for m in (three(3, 10, 0, rule=77)[0], three(3, 10, 0, rule=77)[2]))
    # nperm before the batch
    for nperm in (0, 2 ** 20 + 1):
        assert all(b"permutations" in m for m in three(big, 2, nperm))
    # nq above the batch, before npool < nq; npool above the batch before npool < nq too
    assert all(b"%d regions, more than %d" % (big, big - 1) in m and b"pool" not in m for m in three(big, 2, 2))
    assert all(b"%d regions, more than %d" % (big, big - 1) in m for m in three(big, big, 2))
    # npool < nq before the support's 2^63, which stands last and is the support's alone
    n = 3100000                                                                # 2^20 * n^2 >= 2^63
    assert 2 ** 20 * n * n >= 2 ** 63 and n < big
    assert all(b"%d regions cannot be drawn without replacement from a pool of 2" % n in m for m in three(n, 2, 2 ** 20))
    a = (db.dev, zp, zp, zp, n, zp, zp, zp, n, 0, 2 ** 20)
    assert L_.igd_hip_permute_support_rs(*a, NOV, NEST, *[ptr(x) for x in st], None) == -2
    msg = L_.igd_hip_last_error()
    assert msg.startswith(b"igd_hip_permute_support_rs:") and b"2^63" in msg and all((x == G64).all() for x in st), msg
    # the generator alone: nq above the batch, and more than 2^31 - 1 outputs
    for nq, npool, n_ in ((big, big, 1), (big, 2, 1), (3, big, 1), (65536, 65536, 32768)):
        out = [np.full(4, G32, np.int32) for _ in range(3)]
        assert L_.igd_hip_resample_regions(db.dev, zp, zp, zp, npool, nq, 0, 0, n_, *[ptr(x) for x in out]) == -2
        assert L_.igd_hip_last_error().startswith(b"igd_hip_resample_regions:") and all((x == G32).all() for x in out)


REFUSED_ABOVE_THE_BATCH = r"""
import sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_resample as T
import igd_amd
L_ = T.H()
db = igd_amd.Database(sys.argv[1])
z = np.zeros(65, np.int32)
e = z + 5
G = T.G64
nC = db.nfiles + 1
st = [np.full(nC, G, np.int64) for _ in range(7)]
mats = [np.full(3 * nC, G, np.int64) for _ in range(3)]
small = [np.full(3, G, np.int64), np.full(3, G, np.int64), np.full(1, G, np.int64)]
for npool, want in ((65, -2), (64, 0)):
    a = (db.dev, z.ctypes.data, z.ctypes.data, e.ctypes.data, 3, z.ctypes.data, z.ctypes.data, e.ctypes.data, npool, 0, 2)
    rcs = (L_.igd_hip_permute_support_rs(*a, T.NOV, T.NEST, *[x.ctypes.data for x in st], None),
           L_.igd_hip_permute_nearest_rs(*a, 100, T.NOV, *[x.ctypes.data for x in mats]),
           L_.igd_hip_permute_bp_rs(*a, T.NOV, T.NEST, mats[0].ctypes.data, small[0].ctypes.data, small[1].ctypes.data, small[2].ctypes.data))
    assert rcs == (want,) * 3, (npool, rcs, L_.igd_hip_last_error())
    if want:
        assert b"pool of 65 regions, more than 64" in L_.igd_hip_last_error(), L_.igd_hip_last_error()
        assert all((x == G).all() for x in st + mats + small)
    rc, *out = T.raw_resample(db, (z[:npool], z[:npool], e[:npool]), 3, 0, 2, 0)
    assert rc == want and (want == 0 or all((x == T.G32).all() for x in out))
db.close()
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


def test_a_universe_above_the_batch_is_refused(dbfx):
    """IGD_HIP_MAX_BATCH is read once per process: a child with the batch lowered to 64 regions"""
    p = subprocess.run([sys.executable, "-c", REFUSED_ABOVE_THE_BATCH, dbfx["path"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, IGD_HIP_MAX_BATCH="64"), timeout=600)
    assert p.returncode == 0 and p.stdout.split()[-1:] == [b"ok"], p.stderr.decode()[-2000:]


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_cli_M_resample_on_the_engine_route_equals_the_host_route(rfx):  # noqa: F811
    import igd_amd
    for stat in ([], ["-D", "700"], ["-G"], ["-v", "500"], ["-O", "40"]):
        args = ["search", rfx["db"], "-q", rfx["q"], "-P", "7", "-M", "resample", "-U", rfx["u"], "-S", "5"] + stat
        host, eng = _run(args, HOST), _run(args, ENGINE)
        assert host.returncode == 0 and eng.returncode == 0, eng.stderr
        assert eng.stdout == host.stdout and eng.stdout.count(b"\n") >= 9, stat
    files = igd_amd.Database(rfx["db"])
    try:
        a = files.permutation_support_files(rfx["q"], None, 7, 5, "resample", universe_path=rfx["u"])
        b = files.permutation_support(*rfx["regions"], None, 7, 5, "resample", universe=rfx["pool"])
        assert all(np.array_equal(x, y) for x, y in zip(a[:7], b[:7]))
        assert files.permutation_nearest_files(rfx["q"], None, 3, 700, 5, "resample", universe_path=rfx["u"]).n_within.shape == (4, files.nfiles + 1)
        assert files.permutation_bp_files(rfx["q"], None, 3, 5, "resample", universe_path=rfx["u"]).inter.shape == (4, files.nfiles + 1)
        with pytest.raises(ValueError):
            files.permutation_support_files(rfx["q"], None, 7, 5, "shuffle", universe_path=rfx["u"])
    finally:
        files.close()
