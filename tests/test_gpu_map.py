"""GPU: the values of the overlapping records per region and dataset (igd_hip_map / igd_hip_map_sets / igd_hip_map_dev, kernels
igd_map_rows, igd_map_rowfix and igd_map_reduce; Database.map_values / map_sets / map_files / map_dev, `-V`).

The device must equal, on every integer, the definition restated in tests/map_ref.py (a numpy broadcast over the interval
lists this test wrote) and the host route (igdc_map_host).  Every output is handed over full of 0x5a: a call defines every
word."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import igd_amd
from helpers import ROOT, short_tmpdir, write_bed
from map_ref import OPS, ListDb, clustered_lists, mixed_regions, placed_db, placed_regions, ref_rows, ref_sets, sparse_lists
from test_sets_cli import _write_list
from test_support_host import FLAT, HOST, NUMPY_DBS, _run

pytestmark = pytest.mark.gpu
GARBAGE32, GARBAGE64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igm")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def lds_files():
    """{op: files the LDS form takes}, read from map_dev.hpp: the wave's bytes divided by the bytes per file"""
    src = open(os.path.join(ROOT, "igd_amd", "csrc", "engine", "map_dev.hpp")).read()
    wave = int(re.search(r"^#define\s+IGD_MAP_LDS_WAVE_BYTES\s+(\d+)", src, re.M).group(1))
    per = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+IGD_MAP_LDS_FILES_(\w+)\s+\(IGD_MAP_LDS_WAVE_BYTES / (\d+)\)", src, re.M)}
    assert per == {"COUNT": 4, "MINMAX": 8, "SUM": 12}
    return {"count": wave // 4, "min": wave // 8, "max": wave // 8, "sum": wave // 12}


def check(db, ldb, ichr, qs, qe, op, v=None, off=None, host=True):
    """rows and the set statistics of one call against the definition (and the host route)"""
    want, wagg = ref_rows(ldb, ichr, qs, qe, op, v)
    shape = (len(qs), db.nfiles)
    count, agg = db.map_values(ichr, qs, qe, op, value_filter=v, count=np.full(shape, GARBAGE32, np.int32), agg=np.full(shape, GARBAGE64, np.int64))
    bad = np.flatnonzero((count != want).any(axis=1) | (agg != wagg).any(axis=1))
    assert count.dtype == np.int32 and agg.dtype == np.int64 and len(bad) == 0, \
        (op, v, bad[:5].tolist(), [(count[i].tolist()[:8], want[i].tolist()[:8], agg[i].tolist()[:8], wagg[i].tolist()[:8]) for i in bad[:3]])
    if host:
        hcount, hagg = igd_amd.map_host(ldb.path, ichr, qs, qe, op, value_filter=v)
        assert np.array_equal(hcount, count) and np.array_equal(hagg, agg), (op, v)
    if off is None:
        off = np.array([0, len(qs)], np.int64)
    ms = db.map_sets(ichr, qs, qe, off, op, value_filter=v, out=[np.full((len(off) - 1, db.nfiles), GARBAGE64, np.int64) for _ in range(3)])
    for got, ref in zip(ms[:3], ref_sets(want, wagg, off)):
        assert got.dtype == np.int64 and np.array_equal(got, ref), (op, v)
    return want, wagg


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_device_equals_the_definition_on_the_four_database_shapes(case, workdir):
    from igd_amd import Database
    from igd_amd.database import IgdError
    rng = random.Random(10100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles, min_value=-300)
    ldb = ListDb(workdir, "c%d" % case, files, nbp, gtype)
    ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 500)
    off = np.array([0, 0, 1, 6, 6, 206, len(qs)], np.int64)
    db = Database(ldb.path)
    try:
        for op in OPS:
            for v in (None, 500):
                if gtype == 0 and op != "count":                          # no values: refused before anything is written
                    count = np.full((len(qs), nfiles), GARBAGE32, np.int32)
                    with pytest.raises(IgdError):
                        db.map_values(ichr, qs, qe, op, value_filter=v, count=count)
                    assert (count == GARBAGE32).all()
                    with pytest.raises(IgdError):
                        db.map_sets(ichr, qs, qe, off, op)
                    continue
                want, _ = check(db, ldb, ichr, qs, qe, op, v, off)
                assert (want > 1).any()
    finally:
        db.close()


def test_placed_cases(workdir):
    from igd_amd import Database
    nbp = 1 << 14
    ldb = placed_db(workdir, nbp, "gmplaced")
    (ichr, qs, qe), _ = placed_regions(nbp)
    db = Database(ldb.path)
    try:
        for op in OPS:
            for v in (None, 500):
                check(db, ldb, ichr, qs, qe, op, v)
    finally:
        db.close()


@pytest.mark.parametrize("nfiles", [1, 31, 32, 33, 65, 1365, 1366, 2048, 2049, 4096, 4097])
def test_file_counts_and_small_calls(nfiles, workdir):
    """1, 31, 32, 33 and 65 files, and the two sides of each op's LDS limit (SUM 1 365, MIN / MAX 2 048, COUNT 4 096); calls of 1, 4,
    5 and 64 regions (one wave, one workgroup, a second workgroup)"""
    from igd_amd import Database
    assert lds_files() == {"count": 4096, "min": 2048, "max": 2048, "sum": 1365}
    rng = random.Random(10200 + nfiles)
    nbp = 1 << 12
    span = 40 * nbp
    ldb = ListDb(workdir, "f%d" % nfiles, sparse_lists(rng, nbp, nfiles, 2 if nfiles > 100 else 9, span), nbp, 1)
    db = Database(ldb.path)
    try:
        assert db.nfiles == nfiles
        ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 64)
        ichr[3], qs[3], qe[3] = 0, 0, span + nbp                                      # one region over every record
        hit = False
        for n in (1, 4, 5, 64):
            for op in OPS:
                for v in (None, 500):
                    want, _ = check(db, ldb, ichr[:n], qs[:n], qe[:n], op, v, host=(n == 64))
                    hit |= bool((want > 0).any())
        assert hit
        # op count without an agg row: agg_sum is the pairs
        ms = db.map_sets(ichr, qs, qe, [0, 64], "count")
        assert np.array_equal(ms.pairs, ms.agg_sum) and ms.pairs.any()
    finally:
        db.close()


def test_a_wave_resets_its_tables_before_its_next_region(workdir):
    """4 x igd_hip_map_grid + 3 regions: the grid is full and its first three waves meet a second region.  Their first regions
    cover the whole contig (every file counted); their second ones are a region on an unknown contig (the rows of zeros that are
    stored without reading the tables), a zero-length region and a short one: tables that were not reset would leak into them."""
    from igd_amd import Database
    from igd_amd import _native as N
    rng = random.Random(10300)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 40, 2, 20, min_value=-300)
    ldb = ListDb(workdir, "w", files, nbp, 1)
    nq = 4 * 2048 + 3
    assert N.hip().igd_hip_map_grid(nq) == 2048 and nq == 4 * N.hip().igd_hip_map_grid(nq) + 3
    assert N.hip().igd_hip_map_grid(5) == 2 and N.hip().igd_hip_map_grid(1) == 1
    ichr, qs, qe = mixed_regions(rng, 2, nbp, span, 2 * 8192 + 3)
    ichr[:3], qs[:3], qe[:3] = 0, 0, span + 6 * nbp
    ichr[8192:8195], qs[8192:8195], qe[8192:8195] = [-1, 0, 1], [5, 3 * nbp, 7 * nbp], [9, 3 * nbp, 7 * nbp + 20]
    ichr[16384:], qs[16384:], qe[16384:] = [1, 1, 0], 0, span + 6 * nbp
    off = np.array([0, 700, 1800, 1800, nq], np.int64)
    db = Database(ldb.path)
    try:
        for op, v in (("sum", None), ("min", 500), ("max", None), ("count", 500)):
            want, _ = check(db, ldb, ichr[:nq], qs[:nq], qe[:nq], op, v, off, host=(op == "sum"))
            assert (want[:3] > 0).all() and not want[8192].any()
        # a third round: wave 0 of the grid meets a full row, an empty one (stored without reading the tables) and a full one
        # again; its neighbour a full row, a zero-length region's and a full one
        for op, v in (("sum", None), ("max", 500)):
            want, _ = check(db, ldb, ichr, qs, qe, op, v, host=False)
            assert (want[0] > 0).all() and not want[8192].any() and (want[16384] > 0).all()
    finally:
        db.close()


def test_identities_with_nearest_and_search(workdir):
    from igd_amd import Database
    rng = random.Random(10400)
    nbp = 1 << 11
    nfiles = 40
    files, span = clustered_lists(rng, nbp, nfiles, 1, 25)
    ldb = ListDb(workdir, "p", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 900)
    off = np.array([0, 5, 5, 400, 900], np.int64)
    ntile = max((e - 1) // nbp + 1 for recs in files for (_, s, e, _) in recs)
    ok = (ichr == 0) & (qs >= 0) & (qs.astype(np.int64) < ntile * nbp)
    db = Database(ldb.path)
    try:
        for v in (None, 500):
            count, _ = db.map_values(ichr, qs, qe, "count", value_filter=v)
            dist, _ = db.nearest(ichr, qs, qe, 0, value_filter=v)
            assert count.any() and np.array_equal(count > 0, dist == 0)
            ms = db.map_sets(ichr, qs, qe, off, "max", value_filter=v)
            ns = db.nearest_sets(ichr, qs, qe, off, 0, value_filter=v)
            assert np.array_equal(ms.n_hit, ns.n_overlap[:, :nfiles])
            vf = igd_amd._native.IGD_HIP_NO_VALUE_FILTER if v is None else v
            hits, total = db.search(ichr[ok], qs[ok], qe[ok], rule=FLAT, value_filter=vf)
            assert np.array_equal(count[ok].sum(axis=0), hits) and total == count[ok].sum()
    finally:
        db.close()


SEAM = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import short_tmpdir
import map_ref as R
from igd_amd import Database
d = short_tmpdir("igk")
rng = random.Random(13)
nbp = 1 << 12
files, span = R.clustered_lists(rng, nbp, 40, 2, 20, min_value=-300)
ldb = R.ListDb(d, "b", files, nbp, 1)
db = Database(ldb.path)
sizes = [0, 1, 5, 700, 0, 1100, 3]
off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
ichr, qs, qe = R.mixed_regions(rng, 2, nbp, span, int(off[-1]))
for op, v in (("sum", None), ("max", 500), ("count", None), ("min", None)):
    want, wagg = R.ref_rows(ldb, ichr, qs, qe, op, v)
    for n in (0, 1, 96, 97, 98, 195, len(qs)):
        count, agg = db.map_values(ichr[:n], qs[:n], qe[:n], op, value_filter=v, count=np.full((n, 40), 0x5a5a5a5a, np.int32),
                                   agg=np.full((n, 40), 0x5a5a5a5a5a5a5a5a, np.int64))
        assert np.array_equal(count, want[:n]) and np.array_equal(agg, wagg[:n]), (op, v, n)
    ms = db.map_sets(ichr, qs, qe, off, op, value_filter=v)
    for got, ref in zip(ms[:3], R.ref_sets(want, wagg, off)):
        assert np.array_equal(got, ref), (op, v)
    assert ms.n_hit[3].any() and ms.n_hit[5].any() and not ms.n_hit[0].any()
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "97"}, {"IGD_HIP_MAP_ROW_BYTES": str(97 * 480 + 5)},
                                 {"IGD_HIP_MAP_ROW_BYTES": str(333 * 480), "IGD_HIP_SETS_ROW_BYTES": "2000"}])
def test_calls_straddle_the_chunk_seams(env):
    """chunks of 97 regions (by the batch limit, and by a row budget of 97 rows of 40 x 12 bytes and a little; op count, with rows
    of 160 bytes, is cut at 291) and of 333: no seam is a multiple of 64, the sets of 700 and 1 100 regions are cut by region
    chunks; groups of two sets (a budget of 2 000 bytes against three rows of 40 x 8).  The variables are read once per process:
    a child process each."""
    p = subprocess.run([sys.executable, "-c", SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env),
                       timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


SHARED = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import short_tmpdir
import map_ref as R
import nearest_ref as NR
import flank_ref as F
from igd_amd import Database
d = short_tmpdir("igk")
rng = random.Random(13)
nbp = 1 << 12
files, span = R.clustered_lists(rng, nbp, 40, 2, 20, min_value=-300)
ldb = R.ListDb(d, "b", files, nbp, 1)
db = Database(ldb.path)
sizes = [0, 1, 5, 700, 0, 1100, 3]
off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
ichr, qs, qe = R.mixed_regions(rng, 2, nbp, span, int(off[-1]))
W, B, G = nbp, 7, 0x5a5a5a5a5a5a5a5a
def garbage(*shape):
    return np.full(shape, G, np.int64)
def map_sets(op):
    ms = db.map_sets(ichr, qs, qe, off, op, out=[garbage(len(sizes), 40) for _ in range(3)])
    for got, ref in zip(ms[:3], R.ref_sets(*R.ref_rows(ldb, ichr, qs, qe, op), off)):
        assert np.array_equal(got, ref), op
    return [a.copy() for a in ms[:3]]
nref = NR.ref_sets(*NR.ref_rows(ldb, ichr, qs, qe, W), off)
first = map_sets("sum")
ns = db.nearest_sets(ichr, qs, qe, off, W, out=[garbage(len(sizes), 41) for _ in range(3)])
assert all(np.array_equal(got, ref) for got, ref in zip(ns[:3], nref)), "nearest_sets"
map_sets("count")
fr = db.flank_reldist(ichr, qs, qe, off, W, B, measure=F.EDGES, hist=garbage(len(sizes), B, 41))
assert np.array_equal(fr.hist, F.ref_hist(*F.ref_flanks(ldb, ichr, qs, qe, W, F.EDGES), off, B)), "flank_reldist"
nf = db.nearest_sets_fused(ichr, qs, qe, off, W, out=[garbage(len(sizes), 41) for _ in range(3)])
assert all(np.array_equal(got, ref) for got, ref in zip(nf[:3], nref)), "nearest_sets_fused"
last = map_sets("sum")
assert all(np.array_equal(a, b) for a, b in zip(first, last))
assert first[0][3].any() and first[0][5].any() and ns.n_within[5].any() and fr.hist[5].any() and not first[0][0].any()
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


def test_set_statistics_share_their_group_workspaces():
    """map_sets and the nearest family keep their group's matrices and their slice table in ONE pair of workspaces of the handle.
    On one Database, in turn: map_sets (sum), nearest_sets, map_sets (count), flank_reldist with 7 bins, nearest_sets_fused,
    map_sets (sum) again -- matrices of 40, 41 and 7 x 41 columns, slices of 256 regions and of sets_slice_len(chunk) -- each
    against its definition, the first and the last result equal: a stale capacity, a matrix that was not zeroed again or a
    table left over from the call before would show.  Chunks of 97 regions, groups of two sets (one for the histogram); the
    variables are read once per process: a child process."""
    env = dict(os.environ, IGD_HIP_MAX_BATCH="97", IGD_HIP_SETS_ROW_BYTES="2000")
    p = subprocess.run([sys.executable, "-c", SHARED], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def test_resident_rows_on_a_torch_stream(workdir):
    import torch
    from igd_amd import Database
    rng = random.Random(10500)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 33, 1, 12, min_value=-300)
    ldb = ListDb(workdir, "t", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 300)
    db = Database(ldb.path)
    try:
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            t = [torch.from_numpy(a).to(dev) for a in (ichr, qs, qe)]
            d_count = torch.full((300, 33), GARBAGE32, dtype=torch.int32, device=dev)
            d_agg = torch.full((300, 33), GARBAGE64, dtype=torch.int64, device=dev)
            stream.synchronize()
            for op, v in (("min", 500), ("sum", None)):
                db.map_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 300, d_count.data_ptr(), d_agg.data_ptr(), op=op,
                           value_filter=v, stream=stream.cuda_stream)
                db.sync(stream.cuda_stream)
                want, wagg = ref_rows(ldb, ichr, qs, qe, op, v)
                assert np.array_equal(d_count.cpu().numpy(), want) and np.array_equal(d_agg.cpu().numpy(), wagg), op
            d_count.fill_(GARBAGE32)
            stream.synchronize()
            db.map_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 300, d_count.data_ptr(), None, op="count", stream=stream.cuda_stream)
            db.sync(stream.cuda_stream)
            assert np.array_equal(d_count.cpu().numpy(), ref_rows(ldb, ichr, qs, qe, "count")[0])
    finally:
        db.close()


def test_bad_arguments_change_nothing_and_empty_calls_are_fine(workdir):
    from igd_amd import Database
    from igd_amd.database import IgdError
    rng = random.Random(10600)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 3, 1, 6)
    ldb = ListDb(workdir, "e", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 20)
    db = Database(ldb.path)
    try:
        count, agg = np.full((20, 3), GARBAGE32, np.int32), np.full((20, 3), GARBAGE64, np.int64)
        for op in (-1, 4):                                                # (past the Python layer's names: the native check)
            assert db._H.igd_hip_map(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, 20, op, 0, count.ctypes.data, agg.ctypes.data) != 0
            assert (count == GARBAGE32).all() and (agg == GARBAGE64).all()
        assert db._H.igd_hip_map(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, 20, 1, 0, count.ctypes.data, None) != 0
        assert (count == GARBAGE32).all()
        with pytest.raises(IgdError):
            db.map_values(ichr, qs, qe, "median")
        for off in ([1, 20], [0, 15, 10, 20]):
            with pytest.raises(IgdError):
                db.map_sets(ichr, qs, qe, off, "sum")
        count, agg = db.map_values(ichr[:0], qs[:0], qe[:0], "sum")
        assert count.shape == (0, 3) and agg.shape == (0, 3)
        ms = db.map_sets(ichr[:0], qs[:0], qe[:0], [0, 0, 0], "max", out=[np.full((2, 3), GARBAGE64, np.int64) for _ in range(3)])
        assert all(a.shape == (2, 3) and not a.any() for a in ms[:3])
        ms = db.map_sets(ichr[:0], qs[:0], qe[:0], [0], "max")
        assert all(a.shape == (0, 3) for a in ms[:3])
        ms = db.map_sets(ichr, qs, qe, [0, 0, 20, 20], "count")
        assert not ms.n_hit[0].any() and not ms.n_hit[2].any() and ms.n_hit[1].any()
    finally:
        db.close()


@pytest.mark.parametrize("extra", [[], ["-v", "500"]])
def test_cli_engine_route_prints_what_the_host_route_prints(extra, workdir):
    rng = random.Random(10700)
    nbp = 1 << 12
    d = os.path.join(workdir, "cli%d" % len(extra))
    os.makedirs(d)
    files, span = clustered_lists(rng, nbp, 9, 2, 15, min_value=-300)
    ldb = ListDb(d, "db", files, nbp, 1)
    beds = []
    for k in range(3):
        ichr, qs, qe = mixed_regions(rng, 2, nbp, span, 300)
        p = os.path.join(d, "q%d.bed" % k)
        write_bed(p, [(ldb.ctgs[c] if 0 <= c < 2 else "chrNotThere", s, e) for c, s, e in zip(ichr.tolist(), qs.tolist(), qe.tolist()) if s >= 0])
        beds.append(p)
    lst = _write_list(d, beds + [os.path.join(d, "missing.bed")])
    db = igd_amd.Database(ldb.path)
    try:
        ms = db.map_files(beds, "sum", value_filter=500 if extra else None)
        assert ms.n_hit.shape == (3, 9) and ms.n_hit.any()
    finally:
        db.close()
    for sel in (["-q", beds[0]], ["-Q", lst]):
        for op in ("count", "sum", "min", "max", "mean"):
            args = ["search", ldb.path] + sel + ["-V", op] + extra
            want = _run(args, HOST)
            got = _run(args)                                      # (IGD_HOST_MAX_QUERIES = 0: the engine)
            assert want.returncode == 0 and got.returncode == 0, got.stderr
            assert got.stdout == want.stdout and b"n_hit" in got.stdout, args
            if sel[0] == "-q" and op == "sum":
                assert ("\n0\t%d\t%d\t" % (ms.n_hit[0, 0], ms.pairs[0, 0])).encode() in got.stdout
