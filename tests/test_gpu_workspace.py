"""GPU: the permutation nulls inside a workspace (kernel igd_permute_workspace; igd_hip_permute_regions_ws and the three _ws
drivers; Database.permute_regions / permutation_support / permutation_nearest / permutation_bp with workspace=; `igd search -P
-W` on the engine route).

The kernel is held bit for bit against workspace_ref (numpy, written from the definition) and the host route through its
generic entry, into arrays full of 0x5a.  The drivers are held against their compositions: the generic entry's lists through
support_sets / nearest_sets / jaccard_sets.  Every integer must be EQUAL."""
import ctypes as C
import hashlib
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import igd_amd
import permute_ref as PR
import workspace_ref as WR
from helpers import ROOT, short_tmpdir
from test_support_host import FLAT, HOST, NEST, NOV, _run, clustered_db
from test_workspace_cli import wfx  # noqa: F401  (the command line fixture: database, BED file, genome file, workspace file)

pytestmark = pytest.mark.gpu
ENGINE = {"IGD_HOST_MAX_QUERIES": "0"}
WS = "workspace"
G32 = 0x5a5a5a5a
G64 = 0x5a5a5a5a5a5a5a5a


def H():
    from igd_amd import _native as N
    return N.hip()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igw")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def make_db(workdir, name, nfiles, nctg, seed):
    """a clustered database, a workspace on its contigs and regions that all fit somewhere (some on unknown contigs)"""
    from igd_amd import Database
    rng = random.Random(seed)
    nbp = 1 << 12
    path, span = clustered_db(rng, workdir, name, nbp, 1, nfiles, nctg, 10)
    ctg_len = np.array([span + 2 * nbp + 111 * c for c in range(nctg)], np.int32)
    seg = WR.random_workspace(rng, ctg_len, 60, 2000)
    n = 100
    ichr = np.array([rng.choice(list(range(nctg)) + [-1]) for _ in range(n)], np.int32)
    ln = np.array([rng.choice([0, 1, 50, 300, 700, 1999, 3500]) for _ in range(n)], np.int32)
    qs = np.array([rng.randrange(0, 20000) for _ in range(n)], np.int32)
    tab = WR.table(*seg, ctg_len)
    assert not WR.unplaceable(ichr, qs, qs + ln, ctg_len, tab).any()
    return dict(path=path, db=Database(path), ctg_len=ctg_len, seg=seg, tab=tab, ws=igd_amd.build_workspace(*seg, ctg_len), reg=(ichr, qs, qs + ln))


@pytest.fixture(scope="module", params=[(6, 2, 41), (40, 1, 43)], ids=["6files", "40files"])
def dbfx(request, workdir):
    nfiles, nctg, seed = request.param
    fx = make_db(workdir, "w%d" % nfiles, nfiles, nctg, seed)
    yield fx
    fx["db"].close()


# ---- igd_permute_workspace --------------------------------------------------------------------------------------------------
def raw_permute(db, ichr, qs, qe, ctg_len, p0, n, seed, ws, mode=2):
    """igd_hip_permute_regions_ws into arrays full of 0x5a: (rc, qs', qe')"""
    ichr, qs, qe, ctg_len = (np.ascontiguousarray(a, np.int32) for a in (ichr, qs, qe, ctg_len))
    os_, oe = np.full((n, len(qs)), G32, np.int32), np.full((n, len(qs)), G32, np.int32)
    rc = H().igd_hip_permute_regions_ws(db.dev, ptr(ichr), ptr(qs), ptr(qe), len(qs), ptr(ctg_len), len(ctg_len), mode, seed, p0, n, ptr(os_),
                                        ptr(oe), None if ws is None else ws.ptr)
    return rc, os_, oe


@pytest.fixture(scope="module")
def anydb(workdir):
    from igd_amd import Database
    path, _ = clustered_db(random.Random(3), workdir, "any", 1 << 12, 1, 6, 2, 8)
    db = Database(path)
    yield db
    db.close()


@pytest.fixture(scope="module")
def cases():
    ctg_len, seg, reg = WR.segment_cases()
    return dict(ctg_len=ctg_len, reg=reg, tab=WR.table(*seg, ctg_len), ws=igd_amd.build_workspace(*seg, ctg_len))


def test_kernel_equals_the_reference_and_the_host_on_every_segment_count(anydb, cases):
    ctg_len, reg, tab, ws = cases["ctg_len"], cases["reg"], cases["tab"], cases["ws"]
    nq = len(reg[1])
    assert nq > 257 and sorted(set(np.diff(tab["w_off"]).tolist())) == sorted(WR.SEG_COUNTS)
    stuck = WR.unplaceable(*reg, ctg_len, tab) | (reg[0] < 0) | (reg[0] >= len(ctg_len))
    for seed, p0, n in ((0, 0, 5), (2 ** 64 - 1, 5, 3), (31337, 2 ** 20 - 2, 2)):
        rc, gs, ge = raw_permute(anydb, *reg, ctg_len, p0, n, seed, ws)
        assert rc == 0
        want = WR.place(*reg, ctg_len, tab, p0, n, seed)
        host = igd_amd.permute_regions_host(*reg, ctg_len, p0, n, seed, WS, workspace=ws)
        assert np.array_equal(gs, want[0]) and np.array_equal(ge, want[1]), (seed, p0)
        assert np.array_equal(gs, host[0]) and np.array_equal(ge, host[1])
        assert WR.inside(reg[0], gs, ge, tab)[:, ~stuck].all()                       # containment
        assert (gs[:, stuck] == reg[1][stuck]).all() and (ge[:, stuck] == reg[2][stuck]).all()
    # the keyword route of the binding
    a = anydb.permute_regions(*reg, ctg_len, 5, 3, 2 ** 64 - 1, WS, workspace=ws)
    assert np.array_equal(a[0], WR.place(*reg, ctg_len, tab, 5, 3, 2 ** 64 - 1)[0])


@pytest.mark.parametrize("nq", [1, 2, 63, 64, 65, 255, 256, 257])
def test_one_to_257_outputs_and_p0_above_zero(anydb, cases, nq):
    ctg_len, tab, ws = cases["ctg_len"], cases["tab"], cases["ws"]
    pick = np.linspace(0, len(cases["reg"][1]) - 1, nq).astype(int)
    reg = tuple(a[pick] for a in cases["reg"])
    rc, gs, ge = raw_permute(anydb, *reg, ctg_len, 7, 1, 11, ws)
    want = WR.place(*reg, ctg_len, tab, 7, 1, 11)
    assert rc == 0 and np.array_equal(gs, want[0]) and np.array_equal(ge, want[1])


def test_a_lanes_second_output(anydb, cases):
    """more outputs than the grid has lanes: 300 regions x enough permutations to pass 256 x igd_hip_permute_grid"""
    ctg_len, tab, ws = cases["ctg_len"], cases["tab"], cases["ws"]
    reg = tuple(a[:300] for a in cases["reg"])
    grid = int(H().igd_hip_permute_grid(1 << 30))
    n = 256 * grid // 300 + 1
    assert n * 300 > 256 * grid and int(H().igd_hip_permute_grid(n * 300)) == grid
    rc, gs, ge = raw_permute(anydb, *reg, ctg_len, 3, n, 5, ws)
    want = WR.place(*reg, ctg_len, tab, 3, n, 5)
    assert rc == 0 and np.array_equal(gs, want[0]) and np.array_equal(ge, want[1])


def test_150_contigs(anydb):
    rng = random.Random(8)
    ctg_len = np.array([rng.choice([1, 2, 999, 50000, 2 ** 31 - 1]) for _ in range(150)], np.int32)
    seg = WR.random_workspace(rng, ctg_len, 5, 400)
    tab, ws = WR.table(*seg, ctg_len), igd_amd.build_workspace(*seg, ctg_len)
    ichr = np.array([rng.randrange(-1, 151) for _ in range(400)], np.int32)
    L = ctg_len[np.clip(ichr, 0, 149)].astype(np.int64)
    qs = np.array([rng.randrange(0, int(x) + 1) for x in L], np.int64)
    qe = np.minimum(qs + np.array([rng.choice([0, 1, 7, 399, 801]) for _ in range(400)]), L)
    rc, gs, ge = raw_permute(anydb, ichr, qs, qe, ctg_len, 0, 4, 9, ws)
    want = WR.place(ichr, qs, qe, ctg_len, tab, 0, 4, 9)
    assert rc == 0 and np.array_equal(gs, want[0]) and np.array_equal(ge, want[1])
    assert (gs != qs[None, :]).any()


def test_one_segment_per_contig_gives_shuffle(anydb):
    from test_permute_host import CTG_LEN, generator_fixture
    ichr, qs, qe = generator_fixture()
    n = len(CTG_LEN)
    full = igd_amd.build_workspace(np.arange(n), np.zeros(n), CTG_LEN, CTG_LEN)
    for seed, p0, k in ((0, 0, 9), (2 ** 64 - 1, 5, 4)):
        rc, gs, ge = raw_permute(anydb, ichr, qs, qe, CTG_LEN, p0, k, seed, full)
        bs, be = anydb.permute_regions(ichr, qs, qe, CTG_LEN, p0, k, seed, PR.SHUFFLE)
        ws_, we_ = PR.permute(ichr, qs, qe, CTG_LEN, p0, k, seed, PR.SHUFFLE)
        assert rc == 0 and np.array_equal(gs, bs) and np.array_equal(ge, be) and np.array_equal(gs, ws_) and np.array_equal(ge, we_)


# ---- the three drivers against their compositions ---------------------------------------------------------------------------
def as_sets(fx, nperm, seed):
    """(ichr, qs, qe, set_off) of the nperm + 1 rows: row 0 as given, row p + 1 from Database.permute_regions"""
    ichr, qs, qe = fx["reg"]
    ps, pe = fx["db"].permute_regions(ichr, qs, qe, fx["ctg_len"], 0, nperm, seed, WS, workspace=fx["ws"])
    want = WR.place(ichr, qs, qe, fx["ctg_len"], fx["tab"], 0, nperm, seed)
    assert np.array_equal(ps, want[0]) and np.array_equal(pe, want[1])
    n = len(qs)
    return (np.tile(ichr, nperm + 1), np.concatenate([qs, ps.reshape(-1)]), np.concatenate([qe, pe.reshape(-1)]), np.arange(nperm + 2, dtype=np.int64) * n)


@pytest.mark.parametrize("nperm", [1, 5, 64])
def test_support_driver_equals_its_composition(dbfx, nperm):
    from test_permute_host import check_result
    db, (ichr, qs, qe) = dbfx["db"], dbfx["reg"]
    sets = as_sets(dbfx, nperm, 3)
    for kw in ({}, dict(rule=NEST), dict(rule=FLAT, value_filter=300), dict(rule=FLAT, min_overlap=40)):
        sup, nhit = db.support_sets(*sets, **kw)
        rows = np.concatenate([sup, nhit[:, None]], axis=1).astype(np.int64)
        got = db.permutation_support(ichr, qs, qe, dbfx["ctg_len"], nperm, 3, WS, workspace=dbfx["ws"], **kw)
        check_result(got, rows[0], rows[1:], (nperm, kw))
    assert rows[0][:-1].any() and (rows[1:] != rows[0][None, :]).any()


@pytest.mark.parametrize("nperm", [1, 5, 64])
def test_nearest_driver_equals_its_composition(dbfx, nperm):
    db, (ichr, qs, qe) = dbfx["db"], dbfx["reg"]
    sets = as_sets(dbfx, nperm, 3)
    for window, vf in ((0, None), (500, None), (100000, 300)):
        want = db.nearest_sets(*sets, window, vf)
        out = [np.full((nperm + 1, db.nfiles + 1), G64, np.int64) for _ in range(3)]
        got = db.permutation_nearest(ichr, qs, qe, dbfx["ctg_len"], nperm, window, 3, WS, vf, out=out, workspace=dbfx["ws"])
        for k in ("n_within", "n_overlap", "sum_dist"):
            assert np.array_equal(getattr(got, k), getattr(want, k)), (k, nperm, window)
    assert got.n_within.any()


@pytest.mark.parametrize("nperm", [1, 5, 64])
def test_bp_driver_equals_its_composition(dbfx, nperm):
    db, (ichr, qs, qe) = dbfx["db"], dbfx["reg"]
    sets = as_sets(dbfx, nperm, 3)
    for kw in ({}, dict(rule=NEST), dict(rule=FLAT, value_filter=300)):
        want = db.jaccard_sets(*sets, **kw)
        got = db.permutation_bp(ichr, qs, qe, dbfx["ctg_len"], nperm, 3, WS, workspace=dbfx["ws"], **kw)
        assert np.array_equal(got.inter, want.inter) and np.array_equal(got.set_bp, want.set_bp) and np.array_equal(got.n_merged, want.n_merged)
        assert got.n_dropped == int(want.n_dropped[0]) and np.array_equal(got.file_bp, want.file_bp)
    assert got.inter.any()


def test_the_drivers_equal_the_host_route(dbfx):
    db, (ichr, qs, qe), L, ws, path = dbfx["db"], dbfx["reg"], dbfx["ctg_len"], dbfx["ws"], dbfx["path"]
    a, b = db.permutation_support(ichr, qs, qe, L, 5, 9, WS, workspace=ws), igd_amd.permute_host(path, ichr, qs, qe, L, 5, 9, WS, workspace=ws)
    assert all(np.array_equal(x, y) for x, y in zip(a[:7], b[:7]))
    a, b = db.permutation_nearest(ichr, qs, qe, L, 5, 500, 9, WS, workspace=ws), igd_amd.permute_nearest_host(path, ichr, qs, qe, L, 5, 500, 9, WS, workspace=ws)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    a, b = db.permutation_bp(ichr, qs, qe, L, 5, 9, WS, workspace=ws), igd_amd.permute_bp_host(path, ichr, qs, qe, L, 5, 9, WS, workspace=ws)
    assert all(np.array_equal(x, y) for x, y in zip((a.inter, a.set_bp, a.n_merged, a.file_bp), (b.inter, b.set_bp, b.n_merged, b.file_bp)))


# ---- chunks of permutations -------------------------------------------------------------------------------------------------
CHUNKS = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_workspace as T
from helpers import short_tmpdir
import shutil
d = short_tmpdir("igx")
try:
    fx = T.make_db(d, "c", 40, 1, 47)
    db, (ichr, qs, qe), L, ws = fx["db"], fx["reg"], fx["ctg_len"], fx["ws"]
    assert len(qs) == 100
    sets = T.as_sets(fx, 7, 6)
    h = hashlib.sha256()
    sup, nhit = db.support_sets(*sets)
    rows = np.concatenate([sup, nhit[:, None]], axis=1).astype(np.int64)
    got = db.permutation_support(ichr, qs, qe, L, 7, 6, T.WS, workspace=ws)
    T.check_result(got, rows[0], rows[1:], "support")
    for x in got[:7]: h.update(x.tobytes())
    want = db.nearest_sets(*sets, 500)
    got = db.permutation_nearest(ichr, qs, qe, L, 7, 500, 6, T.WS, workspace=ws)
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])), "nearest"
    for x in got[:3]: h.update(x.tobytes())
    want = db.jaccard_sets(*sets)
    got = db.permutation_bp(ichr, qs, qe, L, 7, 6, T.WS, workspace=ws)
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


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "300"}, {"IGD_HIP_PERM_ROW_BYTES": str(3 * 40 * 8)},
                                 {"IGD_HIP_PERM_ROW_BYTES": str(3 * 3 * 41 * 8 + 8)}])
def test_chunks_of_permutations(env, one_chunk):
    """100 regions, 40 files, 7 permutations.  The batch lowered to 300: 3 + 3 + 1 permutations.  The row budget lowered to 3 rows
    of 40 files: the same cut for the support and the base pairs (one permutation per chunk for the distances, whose chunk
    holds three matrices of 41 columns); to 3 x 3 x 41 x 8 + 8 bytes: 3 + 3 + 1 for the distances.  Equal to the one-chunk
    result (both variables are read once per process)."""
    assert run_chunks(env) == one_chunk


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_callers_arrays_untouched(dbfx):
    from igd_amd import _native as N
    from igd_amd.database import IgdError
    L_ = H()
    db, L, ws, tab = dbfx["db"], dbfx["ctg_len"], dbfx["ws"], dbfx["tab"]
    nC, R = db.nfiles + 1, 3
    longest = int(WR.contig(tab, 0)[1][0])
    ok = (np.zeros(3, np.int32), np.array([0, 5, 9], np.int32), np.array([10, 5 + longest, 9], np.int32))
    bad = (ok[0], ok[1], np.array([10, 5 + longest + 1, 9], np.int32))
    st = [np.full(nC, G64, np.int64) for _ in range(7)]
    mats = [np.full(R * nC, G64, np.int64) for _ in range(3)]
    small = [np.full(R, G64, np.int64), np.full(R, G64, np.int64), np.full(1, G64, np.int64)]
    broken = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tab.items()}
    broken["w_len"][0] += 1                                                       # (the prefix no longer fits the lengths)
    raw = N.HipWorkspace(broken["nctg"], broken["nseg"], broken["w_off"].ctypes.data, broken["w_start"].ctypes.data, broken["w_len"].ctypes.data,
                         broken["w_pre"].ctypes.data)

    def three(reg, mode, w):
        a = (db.dev, ptr(reg[0]), ptr(reg[1]), ptr(reg[2]), 3, ptr(L))
        return (L_.igd_hip_permute_support_ws(*a, mode, 0, 2, NOV, NEST, *[ptr(x) for x in st], None, w),
                L_.igd_hip_permute_nearest_ws(*a, mode, 0, 2, 100, NOV, *[ptr(x) for x in mats], w),
                L_.igd_hip_permute_bp_ws(*a, mode, 0, 2, NOV, NEST, ptr(mats[0]), ptr(small[0]), ptr(small[1]), ptr(small[2]), w))
    for reg, mode, w, text in ((bad, 2, ws.ptr, b"region 1 "), (ok, 1, ws.ptr, None), (ok, 0, ws.ptr, None), (ok, 2, None, None), (ok, 3, ws.ptr, None),
                               (ok, 2, C.cast(C.pointer(raw), C.c_void_p), b"workspace table")):
        assert three(reg, mode, w) == (-2, -2, -2), (mode, text)
        if text:
            assert text in L_.igd_hip_last_error(), L_.igd_hip_last_error()
        for x in st + mats + small:
            assert (x == G64).all()
    # the generic entry: a mismatch and a broken table are refused, a region that fits nowhere passes through
    for mode, w in ((1, ws), (2, None)):
        rc, gs, ge = raw_permute(db, *ok, L, 0, 2, 0, w, mode)
        assert rc == -2 and (gs == G32).all() and (ge == G32).all()
    os_, oe = np.full((2, 3), G32, np.int32), np.full((2, 3), G32, np.int32)
    assert L_.igd_hip_permute_regions_ws(db.dev, ptr(ok[0]), ptr(ok[1]), ptr(ok[2]), 3, ptr(L), len(L), 2, 0, 0, 2, ptr(os_), ptr(oe), C.byref(raw)) == -2
    assert (os_ == G32).all() and (oe == G32).all()
    rc, gs, ge = raw_permute(db, *bad, L, 0, 2, 0, ws)
    assert rc == 0 and (gs[:, 1] == 5).all() and (ge[:, 1] == 5 + longest + 1).all() and not (gs == G32).any()
    # mode 2 without a workspace is still refused by the old entries
    assert L_.igd_hip_permute_regions(db.dev, ptr(ok[0]), ptr(ok[1]), ptr(ok[2]), 3, ptr(L), len(L), 2, 0, 0, 2, ptr(os_), ptr(oe)) == -2
    assert L_.igd_hip_permute_support(db.dev, ptr(ok[0]), ptr(ok[1]), ptr(ok[2]), 3, ptr(L), 2, 0, 2, NOV, NEST, *[ptr(x) for x in st]) == -2
    assert (os_ == G32).all() and all((x == G64).all() for x in st)
    # the calls that are not refused run
    assert three(ok, 2, ws.ptr) == (0, 0, 0) and not any((x == G64).any() for x in st + mats + small)
    # the binding: one without the other is a ValueError before any native call; a region that fits nowhere an IgdError
    for call in (lambda **k: db.permute_regions(*ok, L, 0, 1, **k), lambda **k: db.permutation_support(*ok, L, 2, **k),
                 lambda **k: db.permutation_nearest(*ok, L, 2, 100, **k), lambda **k: db.permutation_bp(*ok, L, 2, **k)):
        with pytest.raises(ValueError):
            call(mode=WS)
        with pytest.raises(ValueError):
            call(mode="shuffle", workspace=ws)
    for f in (lambda: db.permutation_support(*bad, L, 2, 0, WS, workspace=ws), lambda: db.permutation_nearest(*bad, L, 2, 100, 0, WS, workspace=ws),
              lambda: db.permutation_bp(*bad, L, 2, 0, WS, workspace=ws)):
        with pytest.raises(IgdError):
            f()


def test_the_shared_refusals_word_for_word_in_all_three_drivers(dbfx):
    """The faults the three drivers refuse alike, each alone, 3 regions and 2 permutations, with the workspace (mode 2) and without
    (mode 1): every entry answers IGD_HIP_ERR_ARG, its message opens with its own name and carries the same key text, and every
    output array keeps its fill."""
    L_ = H()
    db, L, ws, tab = dbfx["db"], dbfx["ctg_len"], dbfx["ws"], dbfx["tab"]
    nC, R = db.nfiles + 1, 3
    longest = int(WR.contig(tab, 0)[1][0])
    c, s, e = np.zeros(3, np.int32), np.array([0, 5, 9], np.int32), np.array([10, 5 + longest, 9], np.int32)
    assert longest >= 10 and 5 + longest <= L[0]
    zero_len = L.copy()
    zero_len[0] = 0
    perm_max = 1 << 20                                                            # IGD_HIP_PERM_MAX
    put = lambda a, v: np.concatenate([a[:1], np.array([v], np.int32), a[2:]])   # noqa: E731  (region 1 changed)
    faults = [(dict(c=None), b"bad argument"), (dict(L=None), b"bad argument"), (dict(mode=3), b"bad argument"),
              (dict(nperm=0), b"permutations"), (dict(nperm=perm_max + 1), b"permutations"), (dict(e=put(e, 4)), b"region 1 "),
              (dict(s=put(s, -1), e=put(e, 3)), b"region 1 "), (dict(e=put(e, int(L[0]) + 1)), b"region 1 "), (dict(L=zero_len), b"region 0 ")]
    st = [np.full(nC, G64, np.int64) for _ in range(7)]
    mats = [np.full(R * nC, G64, np.int64) for _ in range(3)]
    small = [np.full(R, G64, np.int64), np.full(R, G64, np.int64), np.full(1, G64, np.int64)]
    opt = lambda a: None if a is None else ptr(a)                                 # noqa: E731
    rows = 0
    for fault, key in faults:
        for mode, w in ((2, ws.ptr), (1, None)):
            a = dict(dict(c=c, s=s, e=e, L=L, mode=mode, nperm=2), **fault)
            head = (db.dev, opt(a["c"]), ptr(a["s"]), ptr(a["e"]), 3, opt(a["L"]), a["mode"], 0, a["nperm"])
            calls = (("igd_hip_permute_support", lambda: L_.igd_hip_permute_support_ws(*head, NOV, NEST, *[ptr(x) for x in st], None, w)),
                     ("igd_hip_permute_nearest", lambda: L_.igd_hip_permute_nearest_ws(*head, 100, NOV, *[ptr(x) for x in mats], w)),
                     ("igd_hip_permute_bp", lambda: L_.igd_hip_permute_bp_ws(*head, NOV, NEST, ptr(mats[0]), ptr(small[0]), ptr(small[1]),
                                                                             ptr(small[2]), w)))
            for name, call in calls:
                assert call() == -2, (name, fault, mode)
                msg = L_.igd_hip_last_error()
                assert msg.startswith(name.encode() + b":") and key in msg, (msg, fault, mode)
            assert all((x == G64).all() for x in st + mats + small), (fault, mode)
            rows += 1
    assert rows == 2 * len(faults)


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_cli_W_on_the_engine_route_equals_the_host_route(wfx):  # noqa: F811
    for stat in ([], ["-D", "700"], ["-G"], ["-v", "500"], ["-O", "40"]):
        args = ["search", wfx["db"], "-q", wfx["q"], "-P", "7", "-g", wfx["g"], "-W", wfx["w"], "-S", "5"] + stat
        host, eng = _run(args, HOST), _run(args, ENGINE)
        assert host.returncode == 0 and eng.returncode == 0, eng.stderr
        assert eng.stdout == host.stdout and eng.stdout.count(b"\n") >= 9, stat
        assert eng.stderr.decode().endswith("regions do not lie inside the workspace\n")
    files = igd_amd.Database(wfx["db"])
    try:
        L = files.read_genome(wfx["g"])
        ws = files.read_workspace(wfx["w"], L)
        assert (ws.nseg, ws.w_off.tolist()) == (wfx["tab"]["nseg"], wfx["tab"]["w_off"].tolist()) and np.array_equal(ws.w_pre, wfx["tab"]["w_pre"])
        a = files.permutation_support_files(wfx["q"], wfx["g"], 7, 5, WS, workspace=ws)
        b = files.permutation_support(*wfx["regions"], L, 7, 5, WS, workspace=ws)
        assert all(np.array_equal(x, y) for x, y in zip(a[:7], b[:7]))
        assert files.permutation_nearest_files(wfx["q"], wfx["g"], 3, 700, 5, WS, workspace=ws).n_within.shape == (4, files.nfiles + 1)
        assert files.permutation_bp_files(wfx["q"], wfx["g"], 3, 5, WS, workspace=ws).inter.shape == (4, files.nfiles + 1)
    finally:
        files.close()


from test_permute_host import check_result  # noqa: E402,F401  (the chunk script reaches it as T.check_result)
