"""GPU: the set statistics of the overlapping records' values through the fused kernel, and their permutation null
(igd_hip_map_sets_fused / igd_hip_permute_map, _ws, _rs; kernel igd_map_slices; Database.map_sets_fused / permutation_map,
`-P -I`).

Expected values never come from the code under test: tests/map_ref.py's definition over the interval lists this test wrote,
tests/permute_map_ref.py's composition of the generators with it, and on the device the composition that existed before --
permute_regions (resample_regions) + map_sets.  Every integer is compared exactly; every output is handed over full of
0x5a5a5a5a5a5a5a5a."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import igd_amd
import permute_map_ref as PM
import permute_ref as PR
import workspace_ref as WR
from helpers import ROOT, short_tmpdir, write_bed
from map_ref import I32_MAX, OPS, ListDb, clustered_lists, crowd_regions, mixed_regions, placed_db, placed_regions, ref_rows, ref_sets, sparse_lists
from test_support_host import HOST, _run

pytestmark = pytest.mark.gpu
GARBAGE = 0x5a5a5a5a5a5a5a5a
SLICE_MIN, SLICES, SLICE_MAX, GRID = 64, 4096, 4096, 2048          # IGD_SETS_SLICE_MIN, IGD_SETS_SLICES, IGD_SETS_SLICE_MAX, IGD_SETS_GRID
OPNUM = {"count": 0, "sum": 1, "min": 2, "max": 3}
# IGD_MAP_FUSED_LDS_BYTES(nF, op) / nF: 20 B of shared accumulators (12 under count) and four tables of 4, 8 or 12 B
FILE_BYTES = {"count": 12 + 4 * 4, "min": 20 + 4 * 8, "max": 20 + 4 * 8, "sum": 20 + 4 * 12}
ERR_ARG = -2


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igm")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def H():
    from igd_amd import _native as N
    return N.hip()


def max_files(op):
    return H().igd_hip_map_fused_max_files(OPNUM[op])


def slice_len(n):
    return max(SLICE_MIN, min(SLICE_MAX, (n + SLICES - 1) // SLICES))


def garbage(shape):
    return [np.full(shape, GARBAGE, np.int64) for _ in range(3)]


def ptr(a):
    return a.ctypes.data if a.size else None


def check_fused(db, ldb, ichr, qs, qe, off, op, v=None):
    """map_sets_fused against the definition and against map_sets"""
    off = np.asarray(off, np.int64)
    want = ref_sets(*ref_rows(ldb, ichr, qs, qe, op, v), off)
    got = db.map_sets_fused(ichr, qs, qe, off, op, value_filter=v, out=garbage((len(off) - 1, db.nfiles)))
    assert got.op == op
    for name, g, w in zip(("n_hit", "pairs", "agg_sum"), got[:3], want):
        bad = np.argwhere(g != w)
        assert g.dtype == np.int64 and len(bad) == 0, (name, op, v, bad[:5].tolist(), [(int(g[tuple(b)]), int(w[tuple(b)])) for b in bad[:5]])
    ms = db.map_sets(ichr, qs, qe, off, op, value_filter=v)
    for g, w in zip(got[:3], ms[:3]):
        assert np.array_equal(g, w), (op, v)
    return want


@pytest.mark.parametrize("op", OPS)
def test_the_limit_is_what_one_workgroup_may_have_and_1900_files_fit(op):
    """the header's bound: IGD_MAP_FUSED_LDS_BYTES(max, op) is within the 160 KiB of a CU, which one workgroup may have, and 64 files
    more are not; the database the project is measured on takes the fused kernel under every op"""
    m = max_files(op)
    assert FILE_BYTES[op] * m <= 160 * 1024 < FILE_BYTES[op] * (m + 64)
    assert 1900 <= m
    assert H().igd_hip_map_fused_max_files(4) == 0 and H().igd_hip_map_fused_max_files(-1) == 0


@pytest.mark.parametrize("which", ["1", "33", "65", "max-1", "max", "max+1"])
@pytest.mark.parametrize("op", OPS)
def test_file_counts_and_set_sizes(op, which, workdir):
    """1, 33, 65 files, both sides of the fused kernel's limit (max + 1 takes igd_map_rows + igd_map_reduce); sets of 0, 1, 4, 5,
    sliceLen, sliceLen + 1 and 4 097 regions -- one wave, one workgroup, a second slice, a slice of one region -- with unknown
    contigs, zero-length and inverted regions among them"""
    from igd_amd import Database
    m = max_files(op)
    nfiles = {"max-1": m - 1, "max": m, "max+1": m + 1}.get(which) or int(which)
    rng = random.Random(9800 + nfiles)
    nbp = 1 << 12
    span = 40 * nbp
    # (sparse_lists' values 0, 400, 1000 moved to -450, -50, 550: signed, one of them above the filter)
    files = [[(c, s, e, val - 450) for c, s, e, val in f] for f in sparse_lists(rng, nbp, nfiles, 2 if nfiles > 100 else 9, span)]
    ldb = ListDb(workdir, "f%d%s" % (nfiles, op), files, nbp, 1)
    sizes = [0, 1, 4, 5, 64, 65, 0, 4097]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert slice_len(int(off[-1])) == 64
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, int(off[-1]))
    db = Database(ldb.path)
    try:
        assert db.nfiles == nfiles
        hit = neg = False
        for v in (None, 500):
            want = check_fused(db, ldb, ichr, qs, qe, off, op, v)
            hit |= bool(want[0].any())
            neg |= bool((want[2] < 0).any())
            assert not any(w[0].any() or w[6].any() for w in want)
        assert hit and (neg or op != "min")
    finally:
        db.close()


@pytest.mark.parametrize("op", OPS)
def test_placed_cases(op, workdir):
    """300 records of one file in one tile (64 lanes into one cell); INT32_MIN and INT32_MAX under one region; three times
    INT32_MAX (the sum needs 64 bits); -v 500 removing the maximum; the record over five tiles, counted once -- as one set and as
    sets of one region"""
    from igd_amd import Database
    nbp = 1 << 14
    ldb = placed_db(workdir, nbp, "fmplaced", crowd=True)
    (pc, ps, pe), _ = placed_regions(nbp)
    (cc, cs, ce), counts = crowd_regions(nbp)
    ichr, qs, qe = np.concatenate([pc, cc]), np.concatenate([ps, cs]), np.concatenate([pe, ce])
    n = len(qs)
    db = Database(ldb.path)
    try:
        for v in (None, 500):
            one = check_fused(db, ldb, ichr, qs, qe, [0, n], op, v)
            each = check_fused(db, ldb, ichr, qs, qe, np.arange(n + 1), op, v)
            assert np.array_equal(one[1][0], each[1].sum(axis=0))
        each = ref_sets(*ref_rows(ldb, ichr, qs, qe, op, None), np.arange(n + 1, dtype=np.int64))
        assert each[1][len(pc):, 6].tolist() == counts                 # the crowd: 300 and 128 records under one region
        assert each[1][0, 0] == 1                                      # the record over five tiles, once
        if op == "sum":
            assert each[2][6, 3] == 3 * I32_MAX
        if op == "max":
            v500 = ref_sets(*ref_rows(ldb, ichr, qs, qe, op, 500), np.arange(n + 1, dtype=np.int64))
            assert each[2][8, 4] == 499 and v500[0][8, 4] == 0         # -v 500 removes the maximum
    finally:
        db.close()


# ---- the permutation null ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nfx(workdir):
    """a clustered database with values, regions on its two contigs (and on unknown ones), a workspace they all fit in, a universe"""
    from igd_amd import Database
    rng = random.Random(9900)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 40, 2, 20, -1000)
    ldb = ListDb(workdir, "null", files, nbp, 1)
    ctg_len = np.array([span + 9 * nbp, span + 5 * nbp + 11], np.int32)
    n = 150
    ichr = np.array([rng.choice([0, 1, 0, 1, -1, 99]) for _ in range(n)], np.int32)
    ln = np.array([rng.choice([0, 1, 50, 300, 700, 1999]) for _ in range(n)], np.int32)
    qs = np.array([rng.randrange(0, span) for _ in range(n)], np.int32)
    seg = WR.random_workspace(rng, ctg_len, 60, 2000)
    tab = WR.table(*seg, ctg_len)
    assert not WR.unplaceable(ichr, qs, qs + ln, ctg_len, tab).any()
    pool = PR.random_regions(rng, ctg_len, 500)
    db = Database(ldb.path)
    yield dict(db=db, ldb=ldb, nbp=nbp, ctg_len=ctg_len, reg=(ichr, qs, qs + ln), tab=tab, ws=igd_amd.build_workspace(*seg, ctg_len), pool=pool)
    db.close()


def placement(fx, mode):
    """(ctg_len, keyword arguments) of a call in this mode"""
    if mode == "workspace":
        return fx["ctg_len"], dict(workspace=fx["ws"])
    if mode == "resample":
        return None, dict(universe=fx["pool"])
    return fx["ctg_len"], {}


def composition(fx, nperm, op, seed, mode, v):
    """what there was before: the generator's sets on the device, then map_sets on the explicit lists"""
    db, (ichr, qs, qe) = fx["db"], fx["reg"]
    nq = len(qs)
    if mode == "resample":
        dc, ds, de = db.resample_regions(*fx["pool"], nq, 0, nperm, seed)
        c = np.concatenate([ichr, dc.reshape(-1)])
    else:
        ctg_len, kw = placement(fx, mode)
        ds, de = db.permute_regions(ichr, qs, qe, ctg_len, 0, nperm, seed=seed, mode=mode, **kw)
        c = np.tile(ichr, nperm + 1)
    s, e = np.concatenate([qs, ds.reshape(-1)]), np.concatenate([qe, de.reshape(-1)])
    return db.map_sets(c, s, e, np.arange(nperm + 2, dtype=np.int64) * nq, PM.run_op(op), value_filter=v)


@pytest.mark.parametrize("mode", ["circular", "shuffle", "workspace", "resample"])
@pytest.mark.parametrize("op", OPS + ("mean",))
def test_null_equals_the_composition_the_definition_and_the_support(op, mode, nfx):
    from igd_amd import _native as N
    db, ldb, reg = nfx["db"], nfx["ldb"], nfx["reg"]
    ctg_len, kw = placement(nfx, mode)
    moved = False
    for nperm, seed, v in ((1, 3, None), (37, 3, None), (37, 8, 500)):
        got = db.permutation_map(*reg, ctg_len, nperm, op, seed=seed, mode=mode, value_filter=v, out=garbage((nperm + 1, db.nfiles)), **kw)
        assert got.op == op and got.nperm == nperm
        comp = composition(nfx, nperm, op, seed, mode, v)
        want = PM.null(ldb, *reg, nfx["ctg_len"], nperm, op, seed, mode, v, tab=nfx["tab"], pool=nfx["pool"])
        row0 = db.map_sets(*reg, [0, len(reg[1])], PM.run_op(op), value_filter=v)
        for i in range(3):
            assert got[i].dtype == np.int64 and np.array_equal(got[i], comp[i]), (i, nperm, seed, v)
            assert np.array_equal(got[i], want[i]) and np.array_equal(got[i][0], row0[i][0]), (i, nperm, seed, v)
        ps = db.permutation_support(*reg, ctg_len, nperm, seed, mode, rule=N.IGD_HIP_RULE_FLAT, value_filter=v, **kw)
        assert np.array_equal(got.n_hit[1:].sum(axis=0), ps.sum[:db.nfiles]) and np.array_equal(got.n_hit[0], ps.observed[:db.nfiles])
        moved |= bool((got.agg_sum[1:] != got.agg_sum[0]).any())
    assert moved


CHUNKS = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import short_tmpdir
import map_ref as R, permute_ref as PR, permute_map_ref as PM
from igd_amd import Database
d = short_tmpdir("imc")
rng = random.Random(15)
nbp = 1 << 12
nfiles = int(os.environ["PM_NFILES"])
if nfiles <= 100:
    files, span = R.clustered_lists(rng, nbp, nfiles, 2, 20, -1000)
    ctg_len = np.array([span + 9 * nbp, span + 5 * nbp + 3], np.int32)
else:
    span = 40 * nbp
    files = [[(c, s, e, val - 450) for c, s, e, val in f] for f in R.sparse_lists(rng, nbp, nfiles, 2, span)]
    ctg_len = np.array([span + 9 * nbp], np.int32)
ldb = R.ListDb(d, "b", files, nbp, 1)
ichr, qs, qe = PR.random_regions(rng, ctg_len, 40)
db = Database(ldb.path)
assert db.nfiles == nfiles
nperm = int(os.environ["PM_NPERM"])
res = []
for op, mode, v in (("sum", PR.CIRCULAR, None), ("min", PR.SHUFFLE, 500), ("count", PR.CIRCULAR, None)):
    want = PM.null(ldb, ichr, qs, qe, ctg_len, nperm, op, 21, mode, v)
    out = [np.full((nperm + 1, nfiles), 0x5a5a5a5a5a5a5a5a, np.int64) for _ in range(3)]
    got = db.permutation_map(ichr, qs, qe, ctg_len, nperm, op, seed=21, mode=mode, value_filter=v, out=out)
    for g, w in zip(got[:3], want):
        assert np.array_equal(g, w), (op, mode, v)
    assert got.n_hit[1:].any()
    res += list(got[:3])
np.save(os.environ["PM_OUT"], np.stack(res))
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


def child(script, env):
    p = subprocess.run([sys.executable, "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env), timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def test_null_in_chunks_is_the_unchunked_null(workdir):
    """37 permutations in chunks of 16 + 16 + 5 by the row budget (sixteen rows of three times 40 words, and a word), against the
    same call in one chunk.  The variable is read once per process: a child process each."""
    a, b = os.path.join(workdir, "whole.npy"), os.path.join(workdir, "chunks.npy")
    child(CHUNKS, {"PM_NFILES": "40", "PM_NPERM": "37", "PM_OUT": a})
    child(CHUNKS, {"PM_NFILES": "40", "PM_NPERM": "37", "PM_OUT": b, "IGD_HIP_PERM_ROW_BYTES": str(16 * 3 * 40 * 8 + 8)})
    assert np.array_equal(np.load(a), np.load(b)) and np.load(a).shape == (9, 38, 40)


def test_null_above_the_fused_limit_takes_the_rows_route(workdir):
    """one file above max_files("sum"): igd_map_rows + igd_map_reduce in pieces of 25 regions (25 rows of 12 bytes per file), which
    cut the permutation rows of 40 regions; "count" and "min" take the fused kernel on the same database"""
    m = max_files("sum")
    assert m + 1 <= max_files("min")
    child(CHUNKS, {"PM_NFILES": str(m + 1), "PM_NPERM": "5", "PM_OUT": os.path.join(workdir, "wide.npy"), "IGD_HIP_MAP_ROW_BYTES": str(25 * 12 * (m + 1))})


def test_bad_arguments_leave_the_callers_arrays_untouched(workdir, nfx):
    from igd_amd import Database
    from igd_amd.database import IgdError
    db, ctg_len, (ichr, qs, qe) = nfx["db"], nfx["ctg_len"], nfx["reg"]
    nf, nq = db.nfiles, len(qs)

    def native(entry, op, mode, nperm, ws=None):
        out = garbage((max(nperm, 0) + 1, nf))
        rc = getattr(H(), entry)(db.dev, ptr(ichr), ptr(qs), ptr(qe), nq, ptr(ctg_len), mode, 0, nperm, op, igd_amd._native.IGD_HIP_NO_VALUE_FILTER,
                                 *[ptr(a) for a in out], *([ws] if entry.endswith("_ws") else []))
        # a refused call leaves every word as it was; an accepted one defines every word
        assert all((x == GARBAGE).all() for x in out) if rc else not any((x == GARBAGE).any() for x in out), (entry, op, mode, nperm, rc)
        return rc
    assert native("igd_hip_permute_map", 0, 0, 2) == 0
    for op in (-1, 4, 7):                                              # an unknown op
        assert native("igd_hip_permute_map", op, 0, 2) == ERR_ARG and b"no such op" in H().igd_hip_last_error()
    for nperm in (0, (1 << 20) + 1):
        assert native("igd_hip_permute_map", 1, 0, nperm) == ERR_ARG
    # a workspace without its mode, and the mode without a workspace
    assert native("igd_hip_permute_map_ws", 1, 0, 2, nfx["ws"].ptr) == ERR_ARG and native("igd_hip_permute_map_ws", 1, 2, 2, None) == ERR_ARG
    assert native("igd_hip_permute_map", 1, 2, 2) == ERR_ARG and native("igd_hip_permute_map", 1, 4, 2) == ERR_ARG
    for kw in (dict(workspace=nfx["ws"]), dict(mode="workspace"), dict(universe=nfx["pool"]), dict(mode="resample", universe=nfx["pool"])):
        out = garbage((3, nf))
        with pytest.raises(ValueError):                               # (the last: a universe beside ctg_len)
            db.permutation_map(ichr, qs, qe, ctg_len, 2, "sum", out=out, **kw)
        assert all((x == GARBAGE).all() for x in out)
    for op in ("median", "mean "):
        with pytest.raises(IgdError):
            db.permutation_map(ichr, qs, qe, ctg_len, 2, op)
    with pytest.raises(IgdError):
        db.map_sets_fused(ichr, qs, qe, [0, nq], "mean")
    # a value op on a database without values; count works there
    files, span = clustered_lists(random.Random(5), 1 << 12, 3, 2, 6)
    blind = ListDb(workdir, "blind", files, 1 << 12, 0)
    with Database(blind.path) as b:
        for op in ("sum", "min", "max", "mean"):
            out = garbage((3, 3))
            with pytest.raises(IgdError):
                b.permutation_map(ichr, qs, qe, ctg_len, 2, op, out=out)
            assert all((x == GARBAGE).all() for x in out)
        out = garbage((1, 3))
        with pytest.raises(IgdError):
            b.map_sets_fused(ichr, qs, qe, [0, nq], "sum", out=out)
        assert all((x == GARBAGE).all() for x in out)
        got = b.permutation_map(ichr, qs, qe, ctg_len, 2, "count", out=garbage((3, 3)))
        want = PM.null(blind, ichr, qs, qe, ctg_len, 2, "count")
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want)) and got.n_hit.any()
    # empty calls: all zeros
    z = np.zeros(0, np.int32)
    got = db.permutation_map(z, z, z, ctg_len, 4, "max", out=garbage((5, nf)))
    assert all(a.shape == (5, nf) and not a.any() for a in got[:3])
    ms = db.map_sets_fused(z, z, z, [0, 0, 0], "min", out=garbage((2, nf)))
    assert all(a.shape == (2, nf) and not a.any() for a in ms[:3])


@pytest.mark.parametrize("extra", [["-I", "mean"], ["-I", "max", "-v", "500", "-M", "shuffle", "-S", "9"]])
def test_cli_engine_route_prints_what_the_host_route_prints(extra, workdir, nfx):
    d = os.path.join(workdir, "cli%d" % len(extra))
    os.makedirs(d)
    ldb, ctg_len, (ichr, qs, qe) = nfx["ldb"], nfx["ctg_len"], nfx["reg"]
    keep = (qe > 0) & (ichr >= 0) & (ichr < 2)
    q = os.path.join(d, "q.bed")
    write_bed(q, [(ldb.ctgs[c], int(s), int(e)) for c, s, e in zip(ichr[keep], qs[keep], qe[keep])] + [("chrNotThere", 5, 50)])
    g = os.path.join(d, "genome.sizes")
    with open(g, "w") as f:
        f.write("".join("%s\t%d\n" % (ldb.ctgs[c], ctg_len[c]) for c in range(2)))
    args = ["search", ldb.path, "-q", q, "-P", "6", "-g", g] + extra
    want = _run(args, HOST)
    got = _run(args)                                                  # (IGD_HOST_MAX_QUERIES = 0: the engine)
    assert want.returncode == 0 and got.returncode == 0, got.stderr
    assert got.stdout == want.stdout and got.stdout.startswith((PM.HEADER % extra[1]).encode()), args
