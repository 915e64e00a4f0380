"""GPU: the permutation null of region-set support (igd_hip_permute_support = igd_permute_regions + igd_sets_support +
igd_perm_stats per chunk of permutations; Database.permutation_support / permute_regions / perm_stats, `igd search -P` on the
engine route).

The two kernels are held against permute_ref (numpy uint64 generator, numpy column statistics) through their generic
entries; the whole test against permute_ref.stats of the rows that Database.support_sets gives for permute_ref's explicit
permuted lists.  Every integer must be EQUAL.  Every output is handed to the engine full of garbage: a call defines every
word of it."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import permute_ref as PR
import sets_fixtures as F
from helpers import ROOT, short_tmpdir
from test_gpu_sets import DBS, _db
from test_permute_cli import fx  # noqa: F401  (the command line fixture: database, BED file, genome file)
from test_permute_host import CTG_LEN, MODES, check_permuted, generator_fixture
from test_support_host import FLAT, HOST, NEST, NOV, _run, clustered_db

pytestmark = pytest.mark.gpu
ENGINE = {"IGD_HOST_MAX_QUERIES": "0"}
GARBAGE = 0x5a5a5a5a5a5a5a5a
MODE_NO = {PR.CIRCULAR: 0, PR.SHUFFLE: 1}


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igp")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def anydb(workdir):
    """a small database: the generic entries need a handle for its device and workspaces, not its records"""
    from igd_amd import Database
    path, _ = clustered_db(random.Random(3), workdir, "any", 1 << 12, 1, 6, 2, 8)
    db = Database(path)
    yield db
    db.close()


def H():
    from igd_amd import _native as N
    return N.hip()


# ---- igd_permute_regions ------------------------------------------------------------------------------------------------------
def raw_permute(db, ichr, qs, qe, ctg_len, p0, n, seed, mode):
    """igd_hip_permute_regions into arrays full of garbage"""
    ichr, qs, qe, ctg_len = (np.ascontiguousarray(a, np.int32) for a in (ichr, qs, qe, ctg_len))
    os_, oe = np.full((n, len(qs)), 0x5a5a5a5a, np.int32), np.full((n, len(qs)), 0x5a5a5a5a, np.int32)
    rc = H().igd_hip_permute_regions(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), ctg_len.ctypes.data, len(ctg_len),
                                     MODE_NO[mode], seed, p0, n, os_.ctypes.data, oe.ctypes.data)
    assert rc == 0, H().igd_hip_last_error()
    return os_, oe


@pytest.mark.parametrize("mode", MODES)
def test_permute_regions_equals_the_reference_on_the_host_fixture(anydb, mode):
    ichr, qs, qe = generator_fixture()
    for seed, p0, n in ((0, 0, 9), (2 ** 64 - 1, 5, 4), (12345678901234567, 2 ** 20 - 2, 2)):
        ws, we = PR.permute(ichr, qs, qe, CTG_LEN, p0, n, seed, mode)
        gs, ge = raw_permute(anydb, ichr, qs, qe, CTG_LEN, p0, n, seed, mode)
        assert np.array_equal(gs, ws) and np.array_equal(ge, we), (seed, p0)
        check_permuted(ichr, qs, qe, CTG_LEN, gs, ge)
    gs, ge = anydb.permute_regions(ichr, qs, qe, CTG_LEN, 5, 4, 2 ** 64 - 1, mode)
    assert np.array_equal(gs, PR.permute(ichr, qs, qe, CTG_LEN, 5, 4, 2 ** 64 - 1, mode)[0]) and gs.shape == (4, len(qs))


@pytest.mark.parametrize("mode", MODES)
def test_permute_regions_sizes_and_many_contigs(anydb, mode):
    """np * nq of 1, 255, 256, 257 -- one lane, a workgroup less one, exactly one, a second one -- and one above
    256 * igd_hip_permute_grid(n): a lane's second output.  150 contigs; p0 > 0."""
    rng = random.Random(77)
    ctg_len = np.array([rng.choice([1, 2, 10, 1000, 5 * 10 ** 6, 2 ** 31 - 1, rng.randint(1, 3 * 10 ** 8)]) for _ in range(150)], np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 1021, unknown=(-1, 150))
    assert len(set(ichr.tolist())) > 100
    grid = int(H().igd_hip_permute_grid(1 << 30))
    big = 256 * grid // 1021 + 1
    assert big * 1021 > 256 * grid and int(H().igd_hip_permute_grid(big * 1021)) == grid and int(H().igd_hip_permute_grid(257)) == 2
    for nq, n, p0 in ((1, 1, 0), (255, 1, 3), (51, 5, 1000), (256, 1, 7), (64, 4, 2), (257, 1, 1), (1021, big, 9)):
        c, s, e = ichr[:nq], qs[:nq], qe[:nq]
        ws, we = PR.permute(c, s, e, ctg_len, p0, n, 42, mode)
        gs, ge = raw_permute(anydb, c, s, e, ctg_len, p0, n, 42, mode)
        assert np.array_equal(gs, ws) and np.array_equal(ge, we), (nq, n, p0)
    check_permuted(ichr, qs, qe, ctg_len, gs, ge)
    assert anydb.permute_regions(ichr[:0], qs[:0], qe[:0], ctg_len, 0, 3)[0].shape == (3, 0)


# ---- igd_perm_stats -----------------------------------------------------------------------------------------------------------
def raw_stats(db, rows, obs):
    out = [np.full(rows.shape[1], GARBAGE, np.int64) for _ in range(6)]
    got = db.perm_stats(rows, obs, out=out)
    assert all(g is o for g, o in zip(got, out))
    return got


def stats_case(rs, nrows, ncols):
    """values up to 2^24 (a column's sum of squares passes 2^32 with the first row); observed: a row's own value in two
    columns of three (n_ge and n_le both count that row), one more or less in the others"""
    rows = rs.integers(0, 2 ** 24 + 1, (nrows, ncols)).astype(np.int64)
    rows[rs.integers(0, nrows), :] = 2 ** 24
    obs = rows[rs.integers(0, nrows, ncols), np.arange(ncols)].copy()
    obs[2::3] += rs.integers(-1, 2, len(obs[2::3]))
    return rows, obs


def test_perm_stats_equals_the_reference(anydb):
    """1, 2, 63, 64, 65, 257 rows (one wave's rows, all four, a second row group) by 1, 63, 64, 65 and 2 082 columns (a ragged
    workgroup, exactly one, a second one, 33 of them)"""
    rs = np.random.default_rng(11)
    both = 0
    for nrows in (1, 2, 63, 64, 65, 257):
        for ncols in (1, 63, 64, 65, 2082):
            rows, obs = stats_case(rs, nrows, ncols)
            want = PR.stats(rows, obs)
            got = raw_stats(anydb, rows, obs)
            for g, w, name in zip(got, want, ("sum", "sumsq", "n_ge", "n_le", "min", "max")):
                assert np.array_equal(g, w), (nrows, ncols, name)
            assert (want[1] > 2 ** 32).all() and (want[5] == 2 ** 24).all()
            both += int((want[2] + want[3] > nrows).sum())
    assert both > 0, "no row equals its observed value: the fixture is vacuous"
    # negative values: the minimum and maximum are signed
    rows = np.array([[-5, 3], [2, -9], [0, 0]], np.int64)
    got = raw_stats(anydb, rows, np.array([0, -9], np.int64))
    assert [g.tolist() for g in got] == [[-3, -6], [29, 90], [2, 3], [2, 1], [-5, -9], [2, 3]]


STATS_SEAM = r"""
import os, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import random
import permute_ref as PR
from helpers import short_tmpdir
import test_support_host as S
from igd_amd import Database
d = short_tmpdir("igq")
path, _ = S.clustered_db(random.Random(3), d, "any", 1 << 12, 1, 6, 2, 8)
db = Database(path)
rs = np.random.default_rng(5)
rows = rs.integers(0, 1000, (7, 5)).astype(np.int64)
rows[6] = [0, 999, 5, 5, 5]                    # the last chunk (one row) holds a column's minimum and another's maximum
rows[0, 2] = 2000                              # the first chunk holds a maximum: it must survive the later launches
obs = rows[3].copy()
got = db.perm_stats(rows, obs, out=[np.full(5, 77, np.int64) for _ in range(6)])
for g, w in zip(got, PR.stats(rows, obs)):
    assert np.array_equal(g, w), (g, w)
assert got[4][0] == 0 and got[5][1] == 999 and got[5][2] == 2000
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


def test_perm_stats_across_launches():
    """the row budget lowered to 120 bytes (read once per process): 7 rows of 5 columns go through as 3, 3 and 1 rows; the
    sums add up and min and max carry over from launch to launch"""
    p = subprocess.run([sys.executable, "-c", STATS_SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, IGD_HIP_PERM_ROW_BYTES="120"), timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


# ---- igd_hip_permute_support --------------------------------------------------------------------------------------------------
def raw_support(db, ichr, qs, qe, ctg_len, nperm, seed, mode, v, rule):
    """igd_hip_permute_support into seven arrays full of garbage: (rc, arrays)"""
    ichr, qs, qe, ctg_len = (np.ascontiguousarray(a, np.int32) for a in (ichr, qs, qe, ctg_len))
    out = [np.full(db.nfiles + 1, GARBAGE, np.int64) for _ in range(7)]
    rc = H().igd_hip_permute_support(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), ctg_len.ctypes.data,
                                     MODE_NO[mode], seed, nperm, v, rule, *[a.ctypes.data for a in out])
    return rc, out


def reference(db, ichr, qs, qe, ctg_len, nperm, seed, mode, **kw):
    """(observed, rows int64[nperm, nfiles + 1]) from Database.support_sets on permute_ref's explicit lists"""
    nq = len(qs)
    ps, pe = PR.permute(ichr, qs, qe, ctg_len, 0, nperm, seed, mode)
    sup, nhit = db.support_sets(np.tile(ichr, nperm), ps.ravel(), pe.ravel(), np.arange(nperm + 1, dtype=np.int64) * nq, **kw)
    osup, onhit = db.support_sets(ichr, qs, qe, np.array([0, nq], np.int64), **kw)
    return np.concatenate([osup[0], onhit]), np.concatenate([sup, nhit[:, None]], axis=1)


def check(db, ichr, qs, qe, ctg_len, nperm, seed, mode, what, v=0, rule=None, value_filter=None):
    if rule is None:
        erule, ev = db.cli_dispatch(db.gtype, v)
        kw = dict(v=v)
    else:
        erule, ev = rule, (NOV if value_filter is None else value_filter)
        kw = dict(rule=rule, value_filter=value_filter)
    obs, rows = reference(db, ichr, qs, qe, ctg_len, nperm, seed, mode, **kw)
    rc, out = raw_support(db, ichr, qs, qe, ctg_len, nperm, seed, mode, ev, erule)
    assert rc == 0, H().igd_hip_last_error()
    assert np.array_equal(out[0], obs), what
    for g, w, name in zip(out[1:], PR.stats(rows, obs), ("sum", "sumsq", "n_ge", "n_le", "min", "max")):
        assert np.array_equal(g, w), (what, name)
    return obs, rows


@pytest.mark.parametrize("case", range(len(DBS)))
def test_permutation_support_equals_the_reference_on_the_small_databases(case, workdir):
    from igd_amd import Database
    rng = random.Random(700 + case)
    nbp, gtype, nfiles, nctg, span_tiles, dens, hot = DBS[case]
    path, span = _db(rng, workdir, "d%d" % case, nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
    ctg_len = np.full(nctg, span + 2 * nbp, np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 333)
    db = Database(path)
    try:
        moved = 0
        for mode in MODES:
            obs, rows = check(db, ichr, qs, qe, ctg_len, 64, 9, mode, (case, mode, 64))
            moved += int((rows != obs[None, :]).sum())
            assert obs[:-1].any() and obs[-1] >= obs[:-1].max()
            check(db, ichr, qs, qe, ctg_len, 5, 1, mode, (case, mode, 5, "v500"), v=500)
            for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300)):
                check(db, ichr, qs, qe, ctg_len, 1 if rule == NEST else 5, 2, mode, (case, mode, rule, vf), rule=rule, value_filter=vf)
        assert moved > 0, "no permuted count differs from the observed one: the fixture is vacuous"
        # the Python face returns the same integers
        ps = db.permutation_support(ichr, qs, qe, ctg_len, 5, seed=1, mode=PR.SHUFFLE, v=500)
        rc, out = raw_support(db, ichr, qs, qe, ctg_len, 5, 1, PR.SHUFFLE, *reversed(db.cli_dispatch(db.gtype, 500)))
        assert rc == 0 and ps.nperm == 5 and all(np.array_equal(a, b) for a, b in zip(ps[:7], out))
        # no region
        e = np.zeros(0, np.int32)
        rc, out = raw_support(db, e, e, e, ctg_len, 4, 0, PR.CIRCULAR, NOV, NEST)
        assert rc == 0 and not any(out[k].any() for k in (0, 1, 2, 5, 6)) and (out[3] == 4).all() and (out[4] == 4).all()
    finally:
        db.close()


@pytest.mark.parametrize("nfiles", [33, 65, 2081, 8193])
def test_wide_databases(nfiles, workdir):
    """33 files: a second bitmap word; 65: a second workgroup of igd_perm_stats with two live columns; 2 081: 66 words;
    8 193: the wide form of igd_sets_support (bitmap stripes in global memory)"""
    from igd_amd import Database
    path, span, window, edge = F.wide_db(random.Random(8000 + nfiles), workdir, "w%d" % nfiles, nfiles, F.NBP, max(40, nfiles * 3 // 10))
    ctg_len = np.array([span], np.int32)
    rng = random.Random(nfiles)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 150, unknown=(-1,))
    # a few regions over the window of the boundary files: they have support in the set as given
    qs[:8], qe[:8], ichr[:8] = window[0] - 300, window[1] + 300, 0
    db = Database(path)
    try:
        assert (nfiles > 8192) == (not F.plan([1], nfiles)["support"]["lds"])
        for mode, v in ((PR.CIRCULAR, 0), (PR.SHUFFLE, 500)):
            obs, rows = check(db, ichr, qs, qe, ctg_len, 5, 4, mode, (nfiles, mode), v=v)
            assert (obs[edge] >= 8).all() and rows[:, :-1].any()
    finally:
        db.close()


BATCH_SEAM = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import permute_ref as PR
import test_gpu_permute as T
import test_support_host as S
from helpers import short_tmpdir
from igd_amd import Database
d = short_tmpdir("igr")
rng = random.Random(12)
path, span = S.clustered_db(rng, d, "b", 1 << 12, 1, 40, 2, 20)
ctg_len = np.full(2, span + 5000, np.int32)
ichr, qs, qe = PR.random_regions(rng, ctg_len, 100)
db = Database(path)
for mode in T.MODES:
    for nperm in (1, 7):
        obs, rows = T.check(db, ichr, qs, qe, ctg_len, nperm, 6, mode, (mode, nperm))
        assert rows.any()
    T.check(db, ichr, qs, qe, ctg_len, 7, 6, mode, (mode, "v"), v=500)
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "100"}, {"IGD_HIP_MAX_BATCH": "300"}, {"IGD_HIP_PERM_ROW_BYTES": "960"}])
def test_chunks_of_permutations(env):
    """100 regions and the batch lowered to 100: one permutation per chunk; to 300: 7 permutations go through as 3, 3 and 1.
    The row budget lowered to 960 bytes = 3 rows of 40 files: the same cut by the other bound.  (Both read once per process.)"""
    p = subprocess.run([sys.executable, "-c", BATCH_SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env),
                       timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def test_refusals_write_nothing(anydb):
    L = H()
    nf = anydb.nfiles
    ctg_len = np.array([5000, 0], np.int32)
    ichr, qs, qe = np.zeros(3, np.int32), np.array([0, 10, 4999], np.int32), np.array([5, 10, 5000], np.int32)
    out = [np.full(nf + 1, 7, np.int64) for _ in range(7)]
    o = [a.ctypes.data for a in out]
    q = (ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data)
    g = ctg_len.ctypes.data
    assert L.igd_hip_permute_support(anydb.dev, *q, 3, g, 0, 0, 2, NOV, NEST, *o) == 0
    assert all((a != 7).any() for a in out)
    for a in out:
        a[:] = 7

    def refused(args, text=None):
        assert L.igd_hip_permute_support(anydb.dev, *args) == -2, args
        assert all((a == 7).all() for a in out), args
        if text:
            assert text in L.igd_hip_last_error(), L.igd_hip_last_error()
    refused((None, q[1], q[2], 3, g, 0, 0, 2, NOV, NEST, *o))                   # a missing array
    refused((*q, 3, None, 0, 0, 2, NOV, NEST, *o))
    refused((*q, 3, g, 0, 0, 2, NOV, NEST, None, *o[1:]))
    refused((*q, 3, g, 0, 0, 2, NOV, 2, *o))                                    # no such rule
    refused((*q, 3, g, 2, 0, 2, NOV, NEST, *o))                                 # no such mode
    for nperm in (0, -1, 2 ** 20 + 1):
        refused((*q, 3, g, 0, 0, nperm, NOV, NEST, *o), b"permutations")
    big = int(L.igd_hip_max_batch()) + 1
    z = np.zeros(big, np.int32)
    refused((z.ctypes.data, z.ctypes.data, z.ctypes.data, big, g, 0, 0, 2, NOV, NEST, *o), b"regions")
    n = 3100000                                                                # 2^20 * n^2 >= 2^63
    assert 2 ** 20 * n * n >= 2 ** 63 and n < big
    refused((z.ctypes.data, z.ctypes.data, z.ctypes.data, n, g, 0, 0, 2 ** 20, NOV, NEST, *o), b"2^63")
    for k, (c, s, e) in enumerate(((0, 10, 9), (0, -1, 5), (0, 4000, 5001), (1, 0, 0))):
        bc, bs, be = ichr.copy(), qs.copy(), qe.copy()
        bc[k % 3], bs[k % 3], be[k % 3] = c, s, e
        refused((bc.ctypes.data, bs.ctypes.data, be.ctypes.data, 3, g, 0, 0, 2, NOV, NEST, *o), b"region %d " % (k % 3))
    # sums, n_ge .. max may be NULL; a region on an unknown contig is not validated
    bc = np.array([-1, 2, -1], np.int32)
    assert L.igd_hip_permute_support(anydb.dev, bc.ctypes.data, be.ctypes.data, bs.ctypes.data, 3, g, 1, 0, 2, NOV, NEST, o[0], *[None] * 6) == 0
    assert (out[0] != 7).any() and all((a == 7).all() for a in out[1:])
    from igd_amd.database import IgdError
    with pytest.raises(IgdError):
        anydb.permutation_support(ichr, qs, qe, ctg_len[:1], 2)
    with pytest.raises(IgdError):
        anydb.permutation_support(ichr, qs, qe, ctg_len, 2, mode="rigid")
    # the generic entries
    s2 = np.full((2, 3), 7, np.int32)
    assert L.igd_hip_permute_regions(anydb.dev, *q, 3, g, 2, 5, 0, 0, 2, s2.ctypes.data, s2.ctypes.data) == -2
    assert L.igd_hip_permute_regions(anydb.dev, *q, 3, g, 2, 0, 0, 0, 2, None, s2.ctypes.data) == -2
    assert L.igd_hip_perm_stats(anydb.dev, None, 1, 1, o[0], *o[1:]) == -2
    assert L.igd_hip_perm_stats(anydb.dev, o[0], 0, 1, o[0], *o[1:]) == -2
    assert (s2 == 7).all() and all((a == 7).all() for a in out[1:])


# ---- command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["-M", "shuffle", "-S", "5"], ["-v", "500"]])
def test_cli_engine_route_prints_what_the_host_route_prints(fx, extra):  # noqa: F811
    args = ["search", fx["db"], "-q", fx["q"], "-P", "20", "-g", fx["g"]] + extra
    got, want = _run(args, ENGINE), _run(args, HOST)
    assert got.returncode == 0 and want.returncode == 0, got.stderr
    assert got.stdout == want.stdout and got.stdout.startswith(b"index\tobserved\tmean\t") and b"Query regions with a hit" in got.stdout


def test_permutation_support_files_is_what_P_prints(fx):  # noqa: F811
    import igd_amd
    from igd_amd import Database
    db = Database(fx["db"])
    try:
        assert np.array_equal(db.read_genome(fx["g"]), fx["ctg_len"])
        ps = db.permutation_support_files(fx["q"], fx["g"], 20, seed=5, mode="shuffle")
        sm = igd_amd.perm_summary(ps)
        lines = _run(["search", fx["db"], "-q", fx["q"], "-P", "20", "-g", fx["g"], "-M", "shuffle", "-S", "5"], ENGINE).stdout.decode().splitlines()
        assert len(lines) == db.nfiles + 2
        for f, line in enumerate(lines[1:-1]):
            c = line.split("\t")
            assert [int(c[0]), int(c[1]), int(c[5]), int(c[6])] == [f, ps.observed[f], ps.n_ge[f], ps.n_le[f]]
            assert c[2:5] == ["%.6f" % sm.mean[f], "%.6f" % sm.sd[f], "%.6f" % sm.z[f]]
        assert lines[-1].startswith("Query regions with a hit: %d of " % ps.observed[-1])
    finally:
        db.close()
