"""GPU: covered base pairs (igd_hip_coverage_sets / igd_sets_coverage, Database.coverage / coverage_sets / coverage_files, `-b`).

    coverage[k, f] = sum over the queries of set k of | [qs, qe) n union of the records of file f that the query counts |
    covered[k]     = the same with the union over the records of all files

Expected values come from tests/test_coverage_host.py's two sources -- the CPU oracle's enumeration united in numpy (v = 0) and
a brute force over the database's rows that must first reproduce the oracle's hits (v > 0, gType 1) -- and, for the explicit
rules, from igdc_coverage_host, which that file holds against the same sources.  The databases and set sizes are those of
tests/test_gpu_sets.py and tests/test_gpu_support.py, plus a hand-written fixture for the order in which the hits of one
file must be applied.  Non-vacuity: coverage below the pair sum somewhere (a kernel that summed pairs fails), covered above the
largest file's coverage somewhere (one that took the longest fails), and the order fixture (out-of-order collisions fail)."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, ROOT, Oracle, short_tmpdir, write_bed, write_igd_numpy
from test_coverage_host import HostCov, coverage_brute, expected_coverage, query_bp
from test_gpu_sets import DBS, SIZES, _db, _sets
from test_sets_cli import _case_files, _many_sets, _write_list
from test_support_host import FLAT, HOST, NEST, NOV, NUMPY_DBS, _run, clustered_db, mixed_queries

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igv")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _check_sets(path, db, orc, ichr, qs, qe, off, v, strict=True):
    """rows and covered[] equal the helper per set; then the cross-checks against support_sets and the pair sums"""
    cov, covered = db.coverage_sets(ichr, qs, qe, off, v)
    nsets = len(off) - 1
    assert cov.shape == (nsets, orc.nfiles) and covered.shape == (nsets,) and cov.dtype == covered.dtype == np.int64
    below = above = False
    for k in range(nsets):
        a, b = off[k], off[k + 1]
        want, wcovered, pairs = expected_coverage(path, orc, ichr[a:b], qs[a:b], qe[a:b], v)
        assert np.array_equal(cov[k], want), (v, k, b - a)
        assert covered[k] == wcovered, (v, k)
        assert (cov[k] <= pairs).all() and (cov[k] <= query_bp(qs[a:b], qe[a:b])).all()
        assert cov[k].max(initial=0) <= covered[k] <= cov[k].sum()
        below |= bool((cov[k] < pairs).any())
        above |= bool(covered[k] > cov[k].max(initial=0))
    if strict:
        assert below, "fixture is vacuous: coverage equals the pair sum in every set"
        assert above, "fixture is vacuous: covered equals the largest file's coverage in every set"
    # coverage > 0 exactly where support > 0: a counted record overlaps its query by at least 1 bp -- of the queries with
    # qe > qs (an inverted or empty query can still count a record that contains both of its ends; it covers nothing)
    keep = qe > qs
    koff = np.concatenate([[0], np.cumsum([int(keep[off[k]:off[k + 1]].sum()) for k in range(nsets)])]).astype(np.int64)
    c2, _ = db.coverage_sets(ichr[keep], qs[keep], qe[keep], koff, v)
    s2, _ = db.support_sets(ichr[keep], qs[keep], qe[keep], koff, v)
    assert np.array_equal(c2, cov), "queries with qe <= qs cover something"
    assert np.array_equal(c2 > 0, s2 > 0)
    return cov, covered


@pytest.mark.parametrize("v", [0, 500])
@pytest.mark.parametrize("case", range(len(DBS)))
def test_rows_equal_the_helper_per_set(case, v, workdir):
    from igd_amd import Database
    rng = random.Random(900 + case)
    nbp, gtype, nfiles, nctg, span_tiles, dens, hot = DBS[case]
    path, span = _db(rng, workdir, "d%d" % case, nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
    (ichr, qs, qe), off = _sets(rng, nctg, nbp, span, SIZES)
    orc, db, H = Oracle(path), Database(path), HostCov(path)
    try:
        _check_sets(path, db, orc, ichr, qs, qe, off, v, strict=dens > 3)    # (the sparse one: no two records of a file overlap)
        if v == 0:
            # the explicit rules, with and without a filter: rows equal igdc_coverage_host with the same rule
            for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300), (NEST, 300)):
                c2, n2 = db.coverage_sets(ichr, qs, qe, off, rule=rule, value_filter=vf)
                for k in range(len(SIZES)):
                    a, b = off[k], off[k + 1]
                    hv = NOV if (vf is None or gtype == 0) else vf
                    c1, n1 = H.coverage(ichr[a:b], qs[a:b], qe[a:b], hv, rule)
                    assert np.array_equal(c2[k], c1) and n2[k] == n1, (rule, vf, k)
    finally:
        H.close()
        db.close()
        orc.close()


@pytest.mark.parametrize("v", [0, 500])
@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_clustered_databases(case, v, workdir):
    """several overlapping records of one file under one query, records over four and six tiles, a set that crosses a slice"""
    from igd_amd import Database
    rng = random.Random(4100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    path, span = clustered_db(rng, workdir, "c%d" % case, nbp, gtype, nfiles, nctg, span_tiles)
    parts = [mixed_queries(rng, nctg, nbp, span, n) for n in (700, 5, 4097, 64)]
    off = np.zeros(5, np.int64)
    off[1:] = np.cumsum([len(p[1]) for p in parts])
    ichr, qs, qe = (np.concatenate([p[i] for p in parts]).astype(np.int32) for i in range(3))
    orc, db = Oracle(path), Database(path)
    try:
        _check_sets(path, db, orc, ichr, qs, qe, off, v)
    finally:
        db.close()
        orc.close()


def order_fixture(d):
    """One contig, nbp = 2^11, three files, everything under the query [0, 6000).  File 0: a container followed by records
    it contains; two abutting records; two identical ones; 150 mutually overlapping records that start 1 bp apart in one
    tile (same-file collisions fill whole steps, cross the 64 / 128 boundary and go on in the next iteration); a record over
    four tiles that starts in the query's second tile.  Files 1 and 2: single records between those of file 0, so that
    lanes alone on their file and lanes with company meet in the same steps."""
    f0 = [(100, 1000), (200, 300), (400, 500), (1100, 1200), (1200, 1300), (1400, 1500), (1400, 1500)]
    f0 += [(2100 + i, 2100 + i + 400) for i in range(150)]
    f0 += [(3000, 9000)]
    f1 = [(150, 250), (1150, 1250), (1420, 1430)] + [(2100 + 7 * i + 3, 2100 + 7 * i + 5) for i in range(20)] + [(2990, 3010)]
    f2 = [(450, 460), (1250, 1260)] + [(2100 + 11 * i + 1, 2100 + 11 * i + 700) for i in range(12)] + [(5000, 5500), (5900, 7000)]
    files = [[("chr1", s, e, 100) for s, e in f] for f in (f0, f1, f2)]
    path = os.path.join(d, "order.igd")
    write_igd_numpy(path, files, nbp=1 << 11, gtype=1)
    # by hand: file 0 covers [100,1000) + [1100,1300) + [1400,1500) + [2100,2649) + [3000,6000)
    return path, 900 + 200 + 100 + 549 + 3000


def test_hits_of_one_file_are_applied_in_start_order(workdir):
    from igd_amd import Database
    path, hand = order_fixture(workdir)
    orc, db = Oracle(path), Database(path)
    try:
        one = (np.zeros(1, np.int32), np.zeros(1, np.int32), np.full(1, 6000, np.int32))
        want, wcovered, pairs = coverage_brute(path, orc, *one, 0)
        assert want[0] == hand and (want[1:] > 0).all() and (want <= pairs).all() and want[0] < pairs[0] and want[2] < pairs[2]
        assert want.max() < wcovered < want.sum()
        sup, _ = db.support(*one)
        assert (sup == 1).all()
        for n in (1, 63, 300, 5000):
            rep = [np.repeat(a, n) for a in one]
            cov, covered = db.coverage(*rep)
            assert np.array_equal(cov, n * want), (n, cov, want)
            assert covered == n * wcovered, n
        # a query that meets nothing between copies of the one that does: n x the single value, or 0
        ichr = np.zeros(600, np.int32)
        qs = np.where(np.arange(600) % 3 == 1, 20000, 0).astype(np.int32)
        qe = (qs + 6000).astype(np.int32)
        cov, covered = db.coverage_sets(ichr, qs, qe, np.array([0, 1, 2, 600], np.int64))
        assert np.array_equal(cov, np.outer([1, 0, 399], want)) and covered.tolist() == [wcovered, 0, 399 * wcovered]
    finally:
        db.close()
        orc.close()


def test_accumulates_and_takes_empty_calls(workdir):
    from igd_amd import Database
    rng = random.Random(5)
    path, span = _db(rng, workdir, "acc", 1 << 14, 1, 6, 2, 8, 50)
    (ichr, qs, qe), off = _sets(rng, 2, 1 << 14, span, [10, 0, 400, 3])
    db = Database(path)
    try:
        base = np.arange(4 * 6, dtype=np.int64).reshape(4, 6) * 1000
        once, n1 = db.coverage_sets(ichr, qs, qe, off)
        assert once.any()
        got, n2 = db.coverage_sets(ichr, qs, qe, off, coverage=base.copy())
        assert np.array_equal(got, base + once) and np.array_equal(n1, n2)
        c, n = db.coverage_sets(ichr[:0], qs[:0], qe[:0], np.zeros(1, np.int64))
        assert c.shape == (0, 6) and n.shape == (0,)
        c, n = db.coverage_sets(ichr[:0], qs[:0], qe[:0], np.zeros(4, np.int64))
        assert c.shape == (3, 6) and not c.any() and not n.any()
        c, n = db.coverage(ichr[:0], qs[:0], qe[:0])
        assert not c.any() and n == 0
        c, n = db.coverage(ichr, qs, qe)
        assert np.array_equal(c, once.sum(axis=0)) and n == n1.sum()
    finally:
        db.close()


def test_bad_set_off_is_refused_before_any_launch(workdir):
    from igd_amd import Database
    from igd_amd import _native as N
    from igd_amd.database import IgdError
    rng = random.Random(6)
    path, span = _db(rng, workdir, "bad", 1 << 14, 1, 4, 1, 8, 30)
    (ichr, qs, qe), off = _sets(rng, 1, 1 << 14, span, [20, 20])
    db = Database(path)
    try:
        keep = np.full((2, 4), 7, np.int64)
        for bad in ([0, 30, 20, 40], [1, 20, 40], [-3, 20, 40]):
            bad = np.array(bad, np.int64)
            n = len(bad) - 1
            h = np.full((n, 4), 7, np.int64)
            nh = np.full(n, 7, np.int64)
            rc = N.hip().igd_hip_coverage_sets(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, bad.ctypes.data, n,
                                               N.IGD_HIP_NO_VALUE_FILTER, N.IGD_HIP_RULE_NEST, h.ctypes.data, nh.ctypes.data)
            assert rc == -2 and (h == 7).all() and (nh == 7).all()           # IGD_HIP_ERR_ARG, nothing added
        with pytest.raises(IgdError):
            db.coverage_sets(ichr, qs, qe, np.array([0, 30, 10, 40], np.int64))
        with pytest.raises(IgdError):
            db.coverage_sets(ichr, qs, qe, np.array([0, 20, 39], np.int64), coverage=keep)
        assert (keep == 7).all()
    finally:
        db.close()


def test_more_files_than_the_lds_form(workdir):
    """20 000 files: the frontiers live in global memory, one stripe per wave (the generator of the support test: a
    neighbour record 50 bp on overlaps its partner).  A second call must give what the first gave."""
    from igd_amd import Database
    rng = random.Random(7)
    nbp = 1 << 14
    files = []
    for f in range(20000):
        rows = []
        s = rng.randrange(0, 20 * nbp)
        rows.append(("chr1", s, s + rng.randint(1, 3 * nbp), rng.randint(0, 1000)))
        rows.append(("chr1", s + 50, s + 50 + rng.randint(1, 3 * nbp), rng.randint(0, 1000)))
        files.append(rows)
    path = os.path.join(workdir, "wide.igd")
    write_igd_numpy(path, files, nbp=nbp, gtype=1)
    (ichr, qs, qe), off = _sets(rng, 1, nbp, 20 * nbp, [0, 1, 64, 65, 300, 33])
    orc, db = Oracle(path), Database(path)
    try:
        for v in (0, 500):
            first, c1 = _check_sets(path, db, orc, ichr, qs, qe, off, v)
            again, c2 = db.coverage_sets(ichr, qs, qe, off, v)
            assert np.array_equal(again, first) and np.array_equal(c1, c2)
    finally:
        db.close()
        orc.close()


def test_coverage_files_equals_coverage_per_file(workdir):
    from igd_amd import Database
    rng = random.Random(8)
    nbp = 1 << 14
    path, span = clustered_db(rng, workdir, "sf", nbp, 1, 8, 2, 8)
    paths = []
    for k, n in enumerate([0, 1, 50, 700, 9]):
        p = os.path.join(workdir, "sf%d.bed" % k)
        rows = []
        for _ in range(n):
            s = rng.randrange(0, span)
            rows.append((rng.choice(["chr1", "chr2", "chrX"]), s, s + rng.randint(1, 2 * nbp)))
        write_bed(p, rows)
        paths.append(p)
    orc, db = Oracle(path), Database(path)
    try:
        for v in (0, 500):
            cov, covered = db.coverage_files(paths, v)
            for k, p in enumerate(paths):
                q = orc.read_queries(p)
                want, wcovered, _ = expected_coverage(path, orc, *q, v)
                one, n1 = db.coverage(*q, v)
                assert np.array_equal(cov[k], want) and covered[k] == wcovered, (v, k)
                assert np.array_equal(one, cov[k]) and n1 == covered[k]
    finally:
        db.close()
        orc.close()


def test_sets_straddle_engine_batches():
    """IGD_HIP_MAX_BATCH (read once per process) lowered to 97 queries: sets cross batch seams"""
    code = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import Oracle, short_tmpdir
import test_gpu_sets as T
import test_coverage_host as S
from igd_amd import Database
d = short_tmpdir("igw")
rng = random.Random(11)
path, span = T._db(rng, d, "b", 1 << 14, 1, 9, 2, 8, 40, 600)
(ichr, qs, qe), off = T._sets(rng, 2, 1 << 14, span, [0, 1, 96, 97, 98, 500, 3, 250])
orc, db = Oracle(path), Database(path)
below = False
for v in (0, 500):
    cov, covered = db.coverage_sets(ichr, qs, qe, off, v)
    for k in range(len(off) - 1):
        a, b = off[k], off[k + 1]
        want, wcovered, pairs = S.expected_coverage(path, orc, ichr[a:b], qs[a:b], qe[a:b], v)
        assert np.array_equal(cov[k], want) and covered[k] == wcovered, (v, k)
        below |= bool((want < pairs).any())
assert below
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)
    env = dict(os.environ, IGD_HIP_MAX_BATCH="97")
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("gtype0", ["-v", "500"]),
                                        ("edge", []), ("edge", ["-v", "500"])])
def test_cli_engine_route_prints_what_the_host_route_prints(case, extra, workdir):
    """IGD_HOST_MAX_QUERIES=0 (this marker's default): everything through igd_hip_coverage_sets"""
    db = os.path.join(GOLDEN, case, "db.igd")
    d = short_tmpdir("igq")
    try:
        files = _case_files(case) + _many_sets(d)
        for q in files[:2]:
            got = _run(["search", db, "-q", q, "-b"] + extra)
            want = _run(["search", db, "-q", q, "-b"] + extra, HOST)
            assert got.returncode == 0 and want.returncode == 0, got.stderr
            assert got.stdout == want.stdout and b"Query bp with a hit" in got.stdout
        lst = _write_list(d, files)
        got = _run(["search", db, "-Q", lst, "-b"] + extra)
        want = _run(["search", db, "-Q", lst, "-b"] + extra, HOST)
        assert got.returncode == 0 and want.returncode == 0, got.stderr
        assert got.stdout == want.stdout and got.stdout.count(b"Query set ") == len(files)
    finally:
        shutil.rmtree(d, ignore_errors=True)
