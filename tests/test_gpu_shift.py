"""GPU: the support of a region set under rigid shifts (igd_hip_shift_support = igd_shift_regions + igd_sets_support per chunk of
shifts, driven by the chunk driver of the permutation nulls; Database.shift_support / shift_regions / shift_support_files,
`igd search -Z` on the engine route).

The kernel is held against shift_ref (numpy) through its generic entry; the whole call against Database.support_sets over
shift_ref's explicit shifted copies.  Every integer must be EQUAL.  Every output is handed to the engine full of garbage: a call
defines every word of it."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import permute_ref as PR
import sets_fixtures as F
import shift_ref as SR
from helpers import ROOT, short_tmpdir
from test_gpu_sets import DBS, _db
from test_permute_cli import fx  # noqa: F401  (the command line fixture: database, BED file, genome file)
from test_shift_host import CTG_LEN, OFFSETS, SUP_OFFSETS, generator_fixture, support_fixture
from test_support_host import FLAT, HOST, NEST, NOV, _run, clustered_db

pytestmark = pytest.mark.gpu
ENGINE = {"IGD_HOST_MAX_QUERIES": "0"}
G32 = 0x5a5a5a5a
G64 = 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igz")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def anydb(workdir):
    """a small database: the generic entry needs a handle for its device and workspaces, not its records"""
    from igd_amd import Database
    path, _ = clustered_db(random.Random(3), workdir, "any", 1 << 12, 1, 6, 2, 8)
    db = Database(path)
    yield db
    db.close()


def H():
    from igd_amd import _native as N
    return N.hip()


def i32(*arrays):
    return [np.ascontiguousarray(a, np.int32) for a in arrays]


# ---- igd_shift_regions ----------------------------------------------------------------------------------------------------------
def raw_shift(db, ichr, qs, qe, ctg_len, offsets):
    """igd_hip_shift_regions into arrays full of garbage"""
    ichr, qs, qe, ctg_len, offsets = i32(ichr, qs, qe, ctg_len, offsets)
    os_, oe = np.full((len(offsets), len(qs)), G32, np.int32), np.full((len(offsets), len(qs)), G32, np.int32)
    rc = H().igd_hip_shift_regions(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), ctg_len.ctypes.data,
                                   len(ctg_len), offsets.ctypes.data, len(offsets), os_.ctypes.data, oe.ctypes.data)
    assert rc == 0, H().igd_hip_last_error()
    return os_, oe


def test_shift_regions_equals_the_reference_on_the_host_fixture(anydb):
    import igd_amd
    c, s, e = generator_fixture()
    ws, we = SR.shift(c, s, e, CTG_LEN, OFFSETS)
    gs, ge = raw_shift(anydb, c, s, e, CTG_LEN, OFFSETS)
    assert np.array_equal(gs, ws) and np.array_equal(ge, we)
    gs, ge = anydb.shift_regions(c, s, e, CTG_LEN, OFFSETS[::-1])
    assert gs.shape == (len(OFFSETS), len(s)) and np.array_equal(gs, ws[::-1]) and np.array_equal(ge, we[::-1])
    hs, he = igd_amd.shift_regions_host(c, s, e, CTG_LEN, OFFSETS[::-1])
    assert np.array_equal(gs, hs) and np.array_equal(ge, he)
    # one offset; one region; no region
    assert np.array_equal(raw_shift(anydb, c, s, e, CTG_LEN, [6])[0], ws[6:7])
    assert raw_shift(anydb, c[:1], s[:1], e[:1], CTG_LEN, [1, 1])[0].tolist() == [[1], [1]]
    assert anydb.shift_regions(c[:0], s[:0], e[:0], CTG_LEN, [3, 4, 5])[0].shape == (3, 0)


def test_shift_regions_where_a_lane_takes_a_second_output(anydb):
    """8 193 regions x 65 offsets on a single contig = 532 545 outputs, more than 2048 x 256 lanes: some lanes take a second
    output, and the offset index of an output is j0 + t / nq with t well above nq"""
    rng = random.Random(81)
    ctg_len = np.array([3 * 10 ** 8], np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 8193, unknown=())
    offsets = np.array(rng.sample(range(-2 * 10 ** 8, 2 * 10 ** 8), 60) + [1, -1, 2 ** 30, -2 ** 30, 0], np.int32)      # 65 distinct ones
    grid = int(H().igd_hip_permute_grid(1 << 30))
    assert 8193 * 65 == 532545 > 256 * grid
    ws, we = SR.shift(ichr, qs, qe, ctg_len, offsets)
    gs, ge = raw_shift(anydb, ichr, qs, qe, ctg_len, offsets)
    assert np.array_equal(gs, ws) and np.array_equal(ge, we)
    assert np.array_equal(gs[64], qs) and len({tuple(r[:50]) for r in gs.tolist()}) == 65          # every row is its own offset's


# ---- igd_hip_shift_support ------------------------------------------------------------------------------------------------------
def raw_support(db, ichr, qs, qe, ctg_len, offsets, v, rule, mo=None, out=None):
    """igd_hip_shift_support into a matrix full of garbage: (rc, matrix)"""
    import ctypes as C
    ichr, qs, qe, ctg_len, offsets = i32(ichr, qs, qe, ctg_len, offsets)
    out = np.full((len(offsets), db.nfiles + 1), G64, np.int64) if out is None else out
    rc = H().igd_hip_shift_support(db.dev, ichr.ctypes.data if len(qs) else None, qs.ctypes.data if len(qs) else None,
                                   qe.ctypes.data if len(qs) else None, len(qs), ctg_len.ctypes.data, offsets.ctypes.data, len(offsets), v, rule,
                                   out.ctypes.data, None if mo is None else C.byref(mo))
    return rc, out


def reference(db, ichr, qs, qe, ctg_len, offsets, **kw):
    """int64[nshift, nfiles + 1] from Database.support_sets on shift_ref's explicit copies"""
    n, nq = len(offsets), len(qs)
    ws, we = SR.shift(ichr, qs, qe, ctg_len, offsets)
    sup, nhit = db.support_sets(np.tile(ichr, n), ws.ravel(), we.ravel(), np.arange(n + 1, dtype=np.int64) * nq, **kw)
    return np.concatenate([sup, nhit[:, None]], axis=1)


def check(db, ichr, qs, qe, ctg_len, offsets, what, v=0, rule=None, value_filter=None, min_overlap=None):
    from igd_amd.database import _min_overlap
    if rule is None:
        erule, ev = db.cli_dispatch(db.gtype, v)
        kw = dict(v=v)
    else:
        erule, ev = rule, (NOV if value_filter is None else value_filter)
        kw = dict(rule=rule, value_filter=value_filter)
    want = reference(db, ichr, qs, qe, ctg_len, offsets, min_overlap=min_overlap, **kw)
    rc, got = raw_support(db, ichr, qs, qe, ctg_len, offsets, ev, erule, _min_overlap(min_overlap, "t"))
    assert rc == 0, H().igd_hip_last_error()
    assert np.array_equal(got, want), what
    return want


@pytest.mark.parametrize("case", range(len(DBS)))
def test_shift_support_equals_support_sets_over_the_shifted_copies(case, workdir):
    from igd_amd import Database, MinOverlap
    rng = random.Random(900 + case)
    nbp, gtype, nfiles, nctg, span_tiles, dens, hot = DBS[case]
    path, span = _db(rng, workdir, "d%d" % case, nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
    ctg_len = np.array([span // 2 + 17 * c for c in range(nctg)], np.int32)     # inside the records' span: the clamp meets records
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 300)
    step = nbp // 8 + 1
    offsets = np.array([-2 ** 30, -3 * step, -step, 0, step, 3 * step, 2 ** 30, 0, step], np.int32)
    db = Database(path)
    try:
        want = check(db, ichr, qs, qe, ctg_len, offsets, (case, "plain"))
        if dens >= 20:                                            # (the sparse database: 3 records per file)
            assert (want[3] != want[4]).any() and (want[3] != want[2]).any() and want[0, :-1].any() and want[6, :-1].any()
        assert np.array_equal(want[3], want[7]) and (want[:, -1] >= want[:, :-1].max(axis=1)).all()
        check(db, ichr, qs, qe, ctg_len, offsets, (case, "v500"), v=500)
        check(db, ichr, qs, qe, ctg_len, offsets, (case, "bp"), min_overlap=40)
        check(db, ichr, qs, qe, ctg_len, offsets, (case, "fractions"), v=500, min_overlap=MinOverlap.from_fractions(query=0.5, record=0.1))
        for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300)):
            check(db, ichr, qs, qe, ctg_len, offsets, (case, rule, vf), rule=rule, value_filter=vf)
        # the Python face: the same integers, the offset-0 row is support() bit for bit
        ss = db.shift_support(ichr, qs, qe, ctg_len, offsets, v=500)
        assert np.array_equal(ss.shifted, reference(db, ichr, qs, qe, ctg_len, offsets, v=500)) and np.array_equal(ss.offsets, offsets)
        sup, nhit = db.support(ichr, qs, qe, v=500)
        assert np.array_equal(ss.shifted[3, :-1], sup) and ss.shifted[3, -1] == nhit
        # one shift; no region; regions on unknown contigs only
        assert np.array_equal(db.shift_support(ichr, qs, qe, ctg_len, [step]).shifted, want[4:5])
        e = np.zeros(0, np.int32)
        rc, out = raw_support(db, e, e, e, ctg_len, [0, 5, -5], NOV, NEST)
        assert rc == 0 and out.shape == (3, nfiles + 1) and not out.any()
        rc, out = raw_support(db, [-1, nctg, 99], [0, 5, 7], [100, 50, 70000], ctg_len, [0, 5, -5], NOV, NEST)
        assert rc == 0 and not out.any()
    finally:
        db.close()


def test_a_database_wider_than_the_lds_form_of_the_support_kernel(workdir):
    """8 193 files: the rows go through the wide form of igd_sets_support (bitmap stripes in global memory)"""
    from igd_amd import Database
    nfiles = 8193
    path, span, window, edge = F.wide_db(random.Random(8000 + nfiles), workdir, "w%d" % nfiles, nfiles, F.NBP, max(40, nfiles * 3 // 10))
    ctg_len = np.array([span], np.int32)
    rng = random.Random(nfiles)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 150, unknown=(-1,))
    qs[:8], qe[:8], ichr[:8] = window[0] - 300, window[1] + 300, 0
    db = Database(path)
    try:
        assert not F.plan([1], nfiles)["support"]["lds"]
        offsets = np.array([0, 1300, -(window[0] - 200), 2 ** 30, 0], np.int32)
        want = check(db, ichr, qs, qe, ctg_len, offsets, "wide")
        assert (want[0][edge] >= 8).all() and (want[1] != want[0]).any() and want[2:4, :-1].any()
        check(db, ichr, qs, qe, ctg_len, offsets, "wide v", v=500)
    finally:
        db.close()


# ---- chunk seams ----------------------------------------------------------------------------------------------------------------
SEAM = r"""
import hashlib, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_shift as T
import test_shift_host as S
from helpers import short_tmpdir
from igd_amd import Database
d = short_tmpdir("igy")
fx = S.support_fixture(d, nregions=37, seed=77)
ichr, qs, qe = fx["reg"]
offsets = np.array([-2 ** 30, -4000, -37, 0, 37, 4000, 2 ** 30, 11, 37], np.int32)
db = Database(fx["path"])
assert db.nfiles == 40 and len(qs) == 37
h = hashlib.sha256()
for kw in (dict(), dict(v=500), dict(min_overlap=25)):
    want = T.check(db, ichr, qs, qe, fx["ctg_len"], offsets, kw, **kw)
    assert want[:, :-1].any() and (want[3] != want[1]).any() and (want[3] != want[5]).any()
    h.update(want.tobytes())
    h.update(db.shift_support(ichr, qs, qe, fx["ctg_len"], offsets[:5], **kw).shifted.tobytes())
gs, ge = db.shift_regions(ichr, qs, qe, fx["ctg_len"], offsets)
h.update(gs.tobytes()); h.update(ge.tobytes())
print("digest", h.hexdigest())
""" % (os.path.join(ROOT, "tests"), ROOT)


def run_seam(env):
    assert not any(k in os.environ for k in ("IGD_HIP_MAX_BATCH", "IGD_HIP_PERM_ROW_BYTES"))
    p = subprocess.run([sys.executable, "-c", SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env), timeout=600)
    assert p.returncode == 0 and p.stdout.strip().startswith(b"digest "), p.stderr.decode()[-2000:]
    return p.stdout.strip()


@pytest.fixture(scope="module")
def one_chunk():
    return run_seam({})


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "100"}, {"IGD_HIP_MAX_BATCH": "300"}, {"IGD_HIP_PERM_ROW_BYTES": "960"}])
def test_chunks_of_shifts(env, one_chunk):
    """37 regions, 40 files, 9 offsets (and their first 5).  The batch lowered to 100: 2 shifts per chunk, a last chunk of 1; to
    300: 8 per chunk, a ragged last chunk of 1.  The row budget lowered to 960 bytes = 3 rows of 40 files: 3 + 3 + 3 and 3 + 2.
    Each equal to the reference inside the child, and to the unchunked result.  (Both variables are read once per process.)"""
    assert run_seam(env) == one_chunk


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order_write_nothing_and_leave_the_handle_usable(anydb):
    from igd_amd import MinOverlap
    from igd_amd.database import IgdError
    L = H()
    nf = anydb.nfiles
    ctg_len = np.array([5000, 0], np.int32)
    ichr, qs, qe = i32([0, 0, 0], [0, 10, 4999], [5, 10, 5000])
    off = np.array([0, 7], np.int32)
    out = np.full((2, nf + 1), 7, np.int64)
    q = (ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data)
    g, o, sh = ctg_len.ctypes.data, off.ctypes.data, out.ctypes.data
    good = (anydb.dev, *q, 3, g, o, 2, NOV, NEST, sh, None)
    assert L.igd_hip_shift_support(*good) == 0 and (out != 7).any()
    first = out.copy()
    out[:] = 7

    def refused(args, text):
        assert L.igd_hip_shift_support(anydb.dev, *args) == -2, args
        assert (out == 7).all(), args
        err = L.igd_hip_last_error()
        assert err.startswith(b"igd_hip_shift_support: ") and text in err, err
    import ctypes as C
    badmo = MinOverlap()
    badmo.bp = -1
    bad_off = np.array([0, 2 ** 30 + 1], np.int32)
    big = int(L.igd_hip_max_batch()) + 1
    z = np.zeros(big, np.int32)
    zq = (z.ctypes.data, z.ctypes.data, z.ctypes.data)
    bc, bs, be = ichr.copy(), qs.copy(), qe.copy()
    bs[1], be[1] = 4000, 5001
    bq = (bc.ctypes.data, bs.ctypes.data, be.ctypes.data)
    # 1: a missing argument or no such rule
    for args in ((None, q[1], q[2], 3, g, o, 2, NOV, NEST, sh, None), (*q, 3, None, o, 2, NOV, NEST, sh, None),
                 (*q, 3, g, None, 2, NOV, NEST, sh, None), (*q, 3, g, o, 2, NOV, NEST, None, None), (*q, 3, g, o, 2, NOV, 2, sh, None),
                 (*q, -1, g, o, 2, NOV, NEST, sh, None)):
        refused(args, b"bad argument")
    # 2: the number of shifts
    for n in (0, -1, 4097):
        refused((*q, 3, g, o, n, NOV, NEST, sh, None), b"%d shifts, not 1 .. 4096" % n)
    # 3: an offset beyond +-2^30, the first one named
    refused((*q, 3, g, bad_off.ctypes.data, 2, NOV, NEST, sh, None), b"offset 1 = 1073741825 is beyond")
    neg = np.array([-2 ** 30 - 1, 2 ** 30 + 1], np.int32)
    refused((*q, 3, g, neg.ctypes.data, 2, NOV, NEST, sh, None), b"offset 0 = -1073741825 is beyond")
    # 4: more regions than a batch
    refused((*zq, big, g, o, 2, NOV, NEST, sh, None), b"%d regions, more than" % big)
    # 5: the first region off its contig
    refused((*bq, 3, g, o, 2, NOV, NEST, sh, None), b"region 1 = (0, 4000, 5001) does not lie on its contig of length 5000")
    for k, (c, s, e) in enumerate(((0, 10, 9), (0, -1, 5), (1, 0, 0))):
        cc, cs, ce = ichr.copy(), qs.copy(), qe.copy()
        cc[k], cs[k], ce[k] = c, s, e
        refused((cc.ctypes.data, cs.ctypes.data, ce.ctypes.data, 3, g, o, 2, NOV, NEST, sh, None), b"region %d = " % k)
    # the order: each fault wins over the ones behind it
    refused((*bq, 3, g, o, 2, NOV, 2, sh, None), b"bad argument")
    refused((*bq, 3, g, bad_off.ctypes.data, 4097, NOV, NEST, sh, None), b"shifts, not")
    refused((*zq, big, g, bad_off.ctypes.data, 2, NOV, NEST, sh, None), b"is beyond")
    bz = z.copy()
    bz[0] = -1                                                    # (a start of -1 on contig 0)
    refused((z.ctypes.data, bz.ctypes.data, z.ctypes.data, big, g, o, 2, NOV, NEST, sh, None), b"regions, more than")
    # 6: min_overlap out of range first of all
    refused((None, q[1], q[2], 3, g, bad_off.ctypes.data, 0, NOV, 2, sh, C.byref(badmo)), b"min_overlap (-1 bp, 0 ppm, 0 ppm) out of range")
    # the handle serves the next good call
    assert L.igd_hip_shift_support(*good) == 0 and np.array_equal(out, first)

    # the generic entry: the same wording under its own name, regions are not validated, nothing written
    s2 = np.full((2, 3), 7, np.int32)

    def refused_regions(args, text):
        assert L.igd_hip_shift_regions(anydb.dev, *args) == -2, args
        err = L.igd_hip_last_error()
        assert (s2 == 7).all() and err.startswith(b"igd_hip_shift_regions: ") and text in err, err
    p2 = s2.ctypes.data
    refused_regions((*q, 3, g, 2, o, 2, None, p2), b"bad argument")
    refused_regions((*q, 3, g, -1, o, 2, p2, p2), b"bad argument")
    refused_regions((*q, 3, g, 2, o, 0, p2, p2), b"0 shifts, not 1 .. 4096")
    refused_regions((*q, 3, g, 2, bad_off.ctypes.data, 2, p2, p2), b"offset 1 = 1073741825 is beyond")
    refused_regions((*zq, big, g, 2, o, 2, p2, p2), b"regions, more than")
    a, b = np.full((2, 3), 7, np.int32), np.full((2, 3), 7, np.int32)
    assert L.igd_hip_shift_regions(anydb.dev, *bq, 3, g, 2, o, 2, a.ctypes.data, b.ctypes.data) == 0
    assert a.tolist() == [[0, 4000, 4999], [7, 4000, 4999]] and b.tolist() == [[5, 5001, 5000], [12, 5001, 5000]]

    # the Python face: the texts of the argument checker under the entries' own names; no entry takes a caller's array
    full = np.array([5000, 5000], np.int32)
    for call, name in ((lambda *a: anydb.shift_support(*a), "shift_support"), (lambda *a: anydb.shift_regions(*a), "shift_regions")):
        with pytest.raises(IgdError, match="%s: 3 / 3 / 2 regions given" % name):
            call([0, 0, 0], [1, 2, 3], [1, 2], full, [0])
        with pytest.raises(IgdError, match="%s: 2 / 3 / 3 regions given" % name):
            call([0, 0], [1, 2, 3], [1, 2, 3], full, [0])
        with pytest.raises(IgdError, match="%s: 0 shifts, not 1 .. 4096" % name):
            call(ichr, qs, qe, full, [])
        with pytest.raises(IgdError, match="%s: 4097 shifts, not 1 .. 4096" % name):
            call(ichr, qs, qe, full, np.zeros(4097, np.int32))
        with pytest.raises(IgdError, match="%s: offset 2 = 4294967296 is beyond" % name):
            call(ichr, qs, qe, full, [0, 1, 2 ** 32])
    with pytest.raises(IgdError, match="shift_support: ctg_len has 1 entries, the database 2 contigs"):
        anydb.shift_support(ichr, qs, qe, full[:1], [0])
    with pytest.raises(IgdError, match=r"igd_hip_shift_support failed \(code -2\): igd_hip_shift_support: region 1 = \(0, 4000, 5001\)"):
        anydb.shift_support(bc, bs, be, full, [0])
    with pytest.raises(IgdError, match="shift_support: min_overlap must be"):
        anydb.shift_support(ichr, qs, qe, full, [0], min_overlap="half")
    with pytest.raises(TypeError):
        anydb.shift_support(ichr, qs, qe, full, [0], shifted=out)
    assert anydb.shift_support(ichr, qs, qe, ctg_len, off).shifted.tolist() == first.tolist()
    assert type(anydb).shift_support.__name__ == "shift_support" and "igd_hip_shift_support" in type(anydb).shift_support.__doc__


# ---- the three nulls share the driver and its buffers -----------------------------------------------------------------------------
def test_the_three_nulls_are_unchanged_before_and_after_a_shift_call(workdir):
    """permutation_support, _nearest and _bp on one fixture, recorded on a fresh handle, then shift_support on that handle (it
    reuses d_pmReg, d_setRows and the slice table, with other sizes), then the three again: the same integers.  And a shift call
    behind the nulls gives what it gave on a handle that never ran one."""
    from igd_amd import Database
    sf = support_fixture(os.path.join(workdir, ""), nregions=120, seed=31)
    ichr, qs, qe = sf["reg"]
    L = sf["ctg_len"]

    def nulls(db):
        out = []
        for mode in ("circular", "shuffle"):
            out += list(db.permutation_support(ichr, qs, qe, L, 6, seed=4, mode=mode, min_overlap=3)[:7])
            out += list(db.permutation_nearest(ichr, qs, qe, L, 6, 900, seed=4, mode=mode)[:3])
            pb = db.permutation_bp(ichr, qs, qe, L, 6, seed=4, mode=mode)
            out += [pb.inter, pb.set_bp, pb.n_merged, np.array([pb.n_dropped])]
        return [np.array(a).copy() for a in out]
    db = Database(sf["path"])
    try:
        before = nulls(db)
        assert any(a.any() for a in before)
        s1 = db.shift_support(ichr, qs, qe, L, SUP_OFFSETS).shifted
        db.shift_support(ichr[:7], qs[:7], qe[:7], L, [5])
        after = nulls(db)
        assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))
        assert np.array_equal(db.shift_support(ichr, qs, qe, L, SUP_OFFSETS).shifted, s1)
    finally:
        db.close()
    fresh = Database(sf["path"])
    try:
        assert np.array_equal(fresh.shift_support(ichr, qs, qe, L, SUP_OFFSETS).shifted, s1)
        assert np.array_equal(s1, reference(fresh, ichr, qs, qe, L, SUP_OFFSETS))
        import igd_amd
        assert np.array_equal(s1, igd_amd.shift_support_host(sf["path"], ichr, qs, qe, L, SUP_OFFSETS).shifted)
    finally:
        fresh.close()


# ---- command line -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["-v", "500"], ["-O", "40"], ["-P", "20"], ["-P", "20", "-M", "shuffle", "-S", "5", "-v", "500"]])
def test_cli_engine_route_prints_what_the_host_route_prints(fx, extra):  # noqa: F811
    args = ["search", fx["db"], "-q", fx["q"], "-g", fx["g"], "-Z", "8192,4096"] + extra
    got, want = _run(args, ENGINE), _run(args, HOST)
    assert got.returncode == 0 and want.returncode == 0, got.stderr
    assert got.stdout == want.stdout and got.stdout.startswith(b"index\tFile\t") and b"\nany\t-\t" in got.stdout
    assert got.stdout.count(b"\n") == 7 + 2


def test_shift_support_files_is_what_Z_prints(fx):  # noqa: F811
    import igd_amd
    from igd_amd import Database
    db = Database(fx["db"])
    try:
        off = igd_amd.shift_offsets(300, 100)
        ss = db.shift_support_files(fx["q"], fx["g"], off, v=500)
        lines = _run(["search", fx["db"], "-q", fx["q"], "-g", fx["g"], "-Z", "300,100", "-v", "500"], ENGINE).stdout.decode().splitlines()
        assert lines[0] == "index\tFile" + "".join("\tshift_%d" % d for d in off) and len(lines) == db.nfiles + 2
        for f, line in enumerate(lines[1:]):
            c = line.split("\t")
            assert c[0] == (str(f) if f < db.nfiles else "any") and [int(x) for x in c[2:]] == ss.shifted[:, f].tolist()
        assert ss.shifted[:, :-1].any()
        # with -P: the z-scores are local_zscore's
        ps = db.permutation_support_files(fx["q"], fx["g"], 20, seed=5, v=500)
        z = igd_amd.local_zscore(ps, ss)
        lines = _run(["search", fx["db"], "-q", fx["q"], "-g", fx["g"], "-Z", "300,100", "-v", "500", "-P", "20", "-S", "5"],
                     ENGINE).stdout.decode().splitlines()
        for f, line in enumerate(lines[1:]):
            c = line.split("\t")
            assert int(c[2]) == ps.observed[f] and c[5:] == ["NA" if np.isnan(x) else "%.4f" % x for x in z[:, f]]
    finally:
        db.close()
