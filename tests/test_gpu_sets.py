"""GPU: many query sets in one call (igd_hip_search_sets, Database.search_sets / search_files).  Row k of the result must be
what the CPU oracle counts for set k alone -- and what Database.search returns for it -- bit for bit; totals[k] is the row's
sum.  Both routes are covered: the slice kernel for small sets (igd_sets_count) and the batch pipeline for sets of at least
IGD_SETS_BIG_MIN queries (a test-only variable, read per call), alone and mixed in one call.  Databases come from the
independent numpy writer of tests/helpers.py."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT, Oracle, short_tmpdir, write_bed, write_igd_numpy

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 5000, 17, 0, 300]


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igs")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _db(rng, d, name, nbp, gtype, nfiles, nctg, span_tiles, dens, hot=0):
    ctgs = ["chr%d" % (i + 1) for i in range(nctg)]
    span = nbp * span_tiles
    files = []
    for f in range(nfiles):
        rows = []
        for _ in range(dens):
            c = rng.choice(ctgs)
            L = rng.choice([1, 5, nbp // 3, nbp, 3 * nbp + 7, rng.randint(1, 2 * nbp)])
            s = rng.randrange(0, span)
            if rng.random() < 0.2:
                s = (s // nbp) * nbp
            rows.append((c, s, s + L, rng.randint(0, 1000)))
        for _ in range(hot):                              # one tile with more than 512 records
            s = 5 * nbp + rng.randrange(0, nbp)
            rows.append((ctgs[0], s, s + rng.randint(1, nbp // 2), rng.randint(0, 1000)))
        files.append(rows)
    path = os.path.join(d, name + ".igd")
    write_igd_numpy(path, files, nbp=nbp, gtype=gtype)
    return path, span


def _queries(rng, nctg, nbp, span, n):
    """random order; unknown contigs (-1, 99), inverted, zero-length and multi-tile queries"""
    ichr = np.array([rng.choice(list(range(nctg)) + [-1, 99]) for _ in range(n)], np.int32)
    qs = np.array([rng.randrange(0, span + 3 * nbp) for _ in range(n)], np.int32)
    ln = np.array([rng.choice([0, 1, 200, nbp, 5 * nbp, 9 * nbp + 3, rng.randint(1, 3 * nbp), -rng.randint(1, 50)])
                   for _ in range(n)], np.int32)
    return ichr, qs, qs + ln


def _sets(rng, nctg, nbp, span, sizes):
    parts = [_queries(rng, nctg, nbp, span, n) for n in sizes]
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    cat = [np.concatenate([p[i] for p in parts]).astype(np.int32) for i in range(3)]
    return cat, off


DBS = [
    # nbp, gtype, nfiles, nctg, span_tiles, dens, hot
    (1 << 14, 1, 9, 2, 8, 40, 600),      # hot tile of > 512 records
    (1 << 11, 1, 5, 2, 8, 3, 0),         # sparse: empty tiles, rule NEST and FLAT differ
    (1 << 12, 0, 7, 3, 40, 20, 0),       # gType 0
    (1 << 16, 1, 12, 2, 6, 60, 0),       # -b 16: searched over the re-tiled copy
    (1 << 12, 1, 12, 2, 30, 60, 0),      # -b 12: re-tiled copy
]


@pytest.mark.parametrize("big", ["1000000000", "64", "1"])
@pytest.mark.parametrize("v", [0, 500])
@pytest.mark.parametrize("case", range(len(DBS)))
def test_rows_equal_the_oracle_per_set(case, v, big, workdir, monkeypatch):
    from igd_amd import Database
    monkeypatch.setenv("IGD_SETS_BIG_MIN", big)
    rng = random.Random(900 + case)
    nbp, gtype, nfiles, nctg, span_tiles, dens, hot = DBS[case]
    path, span = _db(rng, workdir, "d%d" % case, nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
    (ichr, qs, qe), off = _sets(rng, nctg, nbp, span, SIZES)
    orc = Oracle(path)
    db = Database(path)
    try:
        hits, totals = db.search_sets(ichr, qs, qe, off, v)
        assert hits.shape == (len(SIZES), nfiles) and totals.shape == (len(SIZES),)
        for k in range(len(SIZES)):
            a, b = off[k], off[k + 1]
            want, wtot = orc.search(ichr[a:b], qs[a:b], qe[a:b], v)
            assert np.array_equal(hits[k], want), (k, SIZES[k])
            assert totals[k] == hits[k].sum() == wtot
        assert hits.sum() > 0
        # the explicit rules, filter off: rows equal Database.search with the same rule
        from igd_amd import _native as N
        for rule in (N.IGD_HIP_RULE_NEST, N.IGD_HIP_RULE_FLAT):
            h2, t2 = db.search_sets(ichr, qs, qe, off, rule=rule)
            for k in range(len(SIZES)):
                a, b = off[k], off[k + 1]
                h1, t1 = db.search(ichr[a:b], qs[a:b], qe[a:b], rule=rule)
                assert np.array_equal(h2[k], h1) and t2[k] == t1, (rule, k)
    finally:
        db.close()
        orc.close()


def test_accumulates_into_hits_and_takes_empty_calls(workdir):
    from igd_amd import Database
    rng = random.Random(5)
    path, span = _db(rng, workdir, "acc", 1 << 14, 1, 6, 2, 8, 50)
    (ichr, qs, qe), off = _sets(rng, 2, 1 << 14, span, [10, 0, 400, 3])
    db = Database(path)
    try:
        base = np.arange(4 * 6, dtype=np.int64).reshape(4, 6) * 1000
        once, _ = db.search_sets(ichr, qs, qe, off)
        got, tot = db.search_sets(ichr, qs, qe, off, hits=base.copy())
        assert np.array_equal(got, base + once) and np.array_equal(tot, once.sum(axis=1))
        h, t = db.search_sets(ichr[:0], qs[:0], qe[:0], np.zeros(1, np.int64))
        assert h.shape == (0, 6) and t.shape == (0,)
        h, t = db.search_sets(ichr[:0], qs[:0], qe[:0], np.zeros(4, np.int64))
        assert not h.any() and not t.any()
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
        hits = np.full((2, 4), 7, np.int64)
        for bad in ([0, 30, 20, 40], [1, 20, 40], [-3, 20, 40]):
            bad = np.array(bad, np.int64)
            n = len(bad) - 1
            h = np.full((n, 4), 7, np.int64)
            rc = N.hip().igd_hip_search_sets(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, bad.ctypes.data, n,
                                             N.IGD_HIP_NO_VALUE_FILTER, N.IGD_HIP_RULE_NEST, 0, h.ctypes.data, None)
            assert rc == -2 and (h == 7).all()           # IGD_HIP_ERR_ARG, nothing added
        with pytest.raises(IgdError):
            db.search_sets(ichr, qs, qe, np.array([0, 30, 10, 40], np.int64))   # decreasing: refused by the engine
        with pytest.raises(IgdError):
            db.search_sets(ichr, qs, qe, np.array([0, 20, 39], np.int64), hits=hits)   # set_off[-1] != number of queries
        assert (hits == 7).all()
    finally:
        db.close()


def test_more_files_than_the_lds_row(workdir):
    from igd_amd import Database
    rng = random.Random(7)
    nbp = 1 << 14
    files = []
    for f in range(20000):
        rows = []
        for _ in range(2):
            s = rng.randrange(0, 20 * nbp)
            rows.append(("chr1", s, s + rng.randint(1, 3 * nbp), rng.randint(0, 1000)))
        files.append(rows)
    path = os.path.join(workdir, "wide.igd")
    write_igd_numpy(path, files, nbp=nbp, gtype=1)
    (ichr, qs, qe), off = _sets(rng, 1, nbp, 20 * nbp, [0, 1, 64, 65, 900, 33])
    orc = Oracle(path)
    db = Database(path)
    try:
        for v in (0, 500):
            hits, totals = db.search_sets(ichr, qs, qe, off, v)
            for k in range(len(off) - 1):
                a, b = off[k], off[k + 1]
                want, wtot = orc.search(ichr[a:b], qs[a:b], qe[a:b], v)
                assert np.array_equal(hits[k], want) and totals[k] == wtot, (v, k)
    finally:
        db.close()
        orc.close()


def test_search_files_equals_search_per_file(workdir):
    from igd_amd import Database
    rng = random.Random(8)
    nbp = 1 << 14
    path, span = _db(rng, workdir, "sf", nbp, 1, 8, 2, 8, 60)
    paths = []
    for k, n in enumerate([0, 1, 50, 700, 9]):
        p = os.path.join(workdir, "sf%d.bed" % k)
        rows = []
        for _ in range(n):
            s = rng.randrange(0, span)
            rows.append((rng.choice(["chr1", "chr2", "chrX"]), s, s + rng.randint(1, 2 * nbp)))
        write_bed(p, rows)
        paths.append(p)
    db = Database(path)
    try:
        for v in (0, 500):
            hits, totals = db.search_files(paths, v)
            for k, p in enumerate(paths):
                h1, t1 = db.search(*db.read_queries(p), v=v)
                assert np.array_equal(hits[k], h1) and totals[k] == t1, (v, k)
    finally:
        db.close()


def test_sets_straddle_engine_batches():
    """IGD_HIP_MAX_BATCH (read once per process) lowered to 97 queries: sets cross batch seams, on both routes."""
    code = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import Oracle, short_tmpdir
import test_gpu_sets as T
from igd_amd import Database
d = short_tmpdir("igb")
rng = random.Random(11)
path, span = T._db(rng, d, "b", 1 << 14, 1, 9, 2, 8, 40, 600)
(ichr, qs, qe), off = T._sets(rng, 2, 1 << 14, span, [0, 1, 96, 97, 98, 500, 3, 250])
orc, db = Oracle(path), Database(path)
for big in ("1000000000", "97", "1"):
    os.environ["IGD_SETS_BIG_MIN"] = big
    for v in (0, 500):
        hits, tot = db.search_sets(ichr, qs, qe, off, v)
        for k in range(len(off) - 1):
            a, b = off[k], off[k + 1]
            want, wtot = orc.search(ichr[a:b], qs[a:b], qe[a:b], v)
            assert np.array_equal(hits[k], want) and tot[k] == wtot, (big, v, k)
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)
    env = dict(os.environ, IGD_HIP_MAX_BATCH="97")
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]
