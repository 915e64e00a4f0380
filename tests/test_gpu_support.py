"""GPU: support counts (igd_hip_support_sets / igd_sets_support, Database.support / support_sets / support_files, `-u`).

    support[k, f] = the queries of set k that overlap AT LEAST ONE record of file f;  nhit[k] = those that overlap any record

Expected values come from the CPU oracle one query at a time (test_support_host.oracle_support) and, for v = 0, from its
enumeration; for the explicit rules from igdc_support_host, which tests/test_support_host.py holds against the oracle.
The databases and set sizes are those of tests/test_gpu_sets.py, plus the clustered ones of tests/test_support_host.py.
Non-vacuity: support <= hits everywhere and support < hits somewhere, so a kernel that counted pairs would fail."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, ROOT, Oracle, short_tmpdir, write_bed, write_igd_numpy
from test_gpu_sets import DBS, SIZES, _db, _sets
from test_sets_cli import _case_files, _many_sets, _write_list
from test_support_host import (FLAT, HOST, NEST, NOV, NUMPY_DBS, HostDb, _run, clustered_db, mixed_queries, oracle_support,
                               oracle_support_enum, sparse_db)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igu")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _check_sets(db, orc, ichr, qs, qe, off, v, strict=True):
    sup, nhit = db.support_sets(ichr, qs, qe, off, v)
    nsets = len(off) - 1
    assert sup.shape == (nsets, orc.nfiles) and nhit.shape == (nsets,)
    hits, _ = db.search_sets(ichr, qs, qe, off, v)
    below = False
    for k in range(nsets):
        a, b = off[k], off[k + 1]
        want, wnhit, whits = oracle_support(orc, ichr[a:b], qs[a:b], qe[a:b], v)
        assert np.array_equal(sup[k], want), (v, k, b - a)
        assert nhit[k] == wnhit, (v, k)
        assert (want <= whits).all() and (sup[k] <= b - a).all() and np.array_equal(hits[k], whits)
        below |= bool((want < whits).any())
        if v == 0:
            e_sup, e_nhit = oracle_support_enum(orc, ichr[a:b], qs[a:b], qe[a:b])
            assert np.array_equal(e_sup, want) and e_nhit == wnhit
    if strict:
        assert below, "fixture is vacuous: support equals the pair counts in every set"
    return sup, nhit


@pytest.mark.parametrize("v", [0, 500])
@pytest.mark.parametrize("case", range(len(DBS)))
def test_rows_equal_the_oracle_per_set(case, v, workdir):
    from igd_amd import Database
    rng = random.Random(900 + case)
    nbp, gtype, nfiles, nctg, span_tiles, dens, hot = DBS[case]
    path, span = _db(rng, workdir, "d%d" % case, nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
    (ichr, qs, qe), off = _sets(rng, nctg, nbp, span, SIZES)
    orc, db, H = Oracle(path), Database(path), HostDb(path)
    try:
        _check_sets(db, orc, ichr, qs, qe, off, v)
        if v == 0:
            # the explicit rules, with and without a filter: rows equal igdc_support_host with the same rule
            for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300), (NEST, 300)):
                s2, n2 = db.support_sets(ichr, qs, qe, off, rule=rule, value_filter=vf)
                for k in range(len(SIZES)):
                    a, b = off[k], off[k + 1]
                    hv = NOV if (vf is None or gtype == 0) else vf
                    s1, n1 = H.support(ichr[a:b], qs[a:b], qe[a:b], hv, rule)
                    assert np.array_equal(s2[k], s1) and n2[k] == n1, (rule, vf, k)
    finally:
        H.close()
        db.close()
        orc.close()


@pytest.mark.parametrize("v", [0, 500])
@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_clustered_databases(case, v, workdir):
    """several records of one file under one query, records over four and six tiles, more than 32 files, repeated queries"""
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
        _check_sets(db, orc, ichr, qs, qe, off, v)
    finally:
        db.close()
        orc.close()


def test_explicit_rules_differ_on_a_sparse_database(workdir):
    from igd_amd import Database
    rng = random.Random(4200)
    path, span, nbp = sparse_db(rng, workdir, "spg")
    ichr, qs, qe = mixed_queries(rng, 2, nbp, span, 2000)
    orc, db = Oracle(path), Database(path)
    try:
        nest, nest_nhit, _ = oracle_support(orc, ichr, qs, qe, 0)
        flat, flat_nhit, _ = oracle_support(orc, ichr, qs, qe, 1)       # values >= 1: rule FLAT, every record passes
        assert not np.array_equal(nest, flat)
        got, nhit = db.support(ichr, qs, qe, rule=NEST)
        assert np.array_equal(got, nest) and nhit == nest_nhit
        got, nhit = db.support(ichr, qs, qe, rule=FLAT)
        assert np.array_equal(got, flat) and nhit == flat_nhit
    finally:
        db.close()
        orc.close()


def test_support_is_row_0_and_copies_of_one_query_count_n_or_0(workdir):
    from igd_amd import Database
    rng = random.Random(31)
    nbp = 1 << 14
    path, span = clustered_db(rng, workdir, "one", nbp, 1, 9, 2, 10)
    ichr, qs, qe = mixed_queries(rng, 2, nbp, span, 900)
    orc, db = Oracle(path), Database(path)
    try:
        for v in (0, 500):
            s1, n1 = db.support(ichr, qs, qe, v)
            s2, n2 = db.support_sets(ichr, qs, qe, np.array([0, len(qs)], np.int64), v)
            assert s1.shape == (9,) and np.array_equal(s1, s2[0]) and n1 == n2[0]
            want, wnhit, _ = oracle_support(orc, ichr, qs, qe, v)
            assert np.array_equal(s1, want) and n1 == wnhit
        seen = 0
        for n in (1, 63, 300, 5000):
            for i in (3, 10, 17, 40):
                one, _ = orc.search(ichr[i:i + 1], qs[i:i + 1], qe[i:i + 1], 0)
                s, nh = db.support(np.repeat(ichr[i], n), np.repeat(qs[i], n), np.repeat(qe[i], n))
                assert np.array_equal(s, n * (one > 0)) and nh == (n if one.any() else 0), (n, i)
                seen += int(one.max() > 1)
        assert seen, "no repeated query meets a file more than once"
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
        once, n1 = db.support_sets(ichr, qs, qe, off)
        assert once.any()
        got, n2 = db.support_sets(ichr, qs, qe, off, support=base.copy())
        assert np.array_equal(got, base + once) and np.array_equal(n1, n2)
        s, n = db.support_sets(ichr[:0], qs[:0], qe[:0], np.zeros(1, np.int64))
        assert s.shape == (0, 6) and n.shape == (0,)
        s, n = db.support_sets(ichr[:0], qs[:0], qe[:0], np.zeros(4, np.int64))
        assert s.shape == (3, 6) and not s.any() and not n.any()
        s, n = db.support(ichr[:0], qs[:0], qe[:0])
        assert not s.any() and n == 0
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
            rc = N.hip().igd_hip_support_sets(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, bad.ctypes.data, n,
                                              N.IGD_HIP_NO_VALUE_FILTER, N.IGD_HIP_RULE_NEST, h.ctypes.data, nh.ctypes.data)
            assert rc == -2 and (h == 7).all() and (nh == 7).all()           # IGD_HIP_ERR_ARG, nothing added
        with pytest.raises(IgdError):
            db.support_sets(ichr, qs, qe, np.array([0, 30, 10, 40], np.int64))
        with pytest.raises(IgdError):
            db.support_sets(ichr, qs, qe, np.array([0, 20, 39], np.int64), support=keep)
        assert (keep == 7).all()
    finally:
        db.close()


def test_more_files_than_the_lds_form(workdir):
    """20 000 files: the bitmaps live in global memory, one stripe per wave"""
    from igd_amd import Database
    rng = random.Random(7)
    nbp = 1 << 14
    files = []
    for f in range(20000):
        rows = []
        s = rng.randrange(0, 20 * nbp)
        rows.append(("chr1", s, s + rng.randint(1, 3 * nbp), rng.randint(0, 1000)))
        rows.append(("chr1", s + 50, s + 50 + rng.randint(1, 3 * nbp), rng.randint(0, 1000)))   # a neighbour: one query, two records
        files.append(rows)
    path = os.path.join(workdir, "wide.igd")
    write_igd_numpy(path, files, nbp=nbp, gtype=1)
    (ichr, qs, qe), off = _sets(rng, 1, nbp, 20 * nbp, [0, 1, 64, 65, 300, 33])
    orc, db = Oracle(path), Database(path)
    try:
        for v in (0, 500):
            first, _ = _check_sets(db, orc, ichr, qs, qe, off, v)
            again, _ = db.support_sets(ichr, qs, qe, off, v)         # the stripes were left all clear
            assert np.array_equal(again, first)
    finally:
        db.close()
        orc.close()


def test_support_files_equals_support_per_file(workdir):
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
            sup, nhit = db.support_files(paths, v)
            for k, p in enumerate(paths):
                want, wnhit, _ = oracle_support(orc, *orc.read_queries(p), v)
                assert np.array_equal(sup[k], want) and nhit[k] == wnhit, (v, k)
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
import test_support_host as S
from igd_amd import Database
d = short_tmpdir("igb")
rng = random.Random(11)
path, span = T._db(rng, d, "b", 1 << 14, 1, 9, 2, 8, 40, 600)
(ichr, qs, qe), off = T._sets(rng, 2, 1 << 14, span, [0, 1, 96, 97, 98, 500, 3, 250])
orc, db = Oracle(path), Database(path)
below = False
for v in (0, 500):
    sup, nhit = db.support_sets(ichr, qs, qe, off, v)
    for k in range(len(off) - 1):
        a, b = off[k], off[k + 1]
        want, wnhit, whits = S.oracle_support(orc, ichr[a:b], qs[a:b], qe[a:b], v)
        assert np.array_equal(sup[k], want) and nhit[k] == wnhit, (v, k)
        below |= bool((want < whits).any())
assert below
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)
    env = dict(os.environ, IGD_HIP_MAX_BATCH="97")
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("gtype0", ["-v", "500"]),
                                        ("edge", [])])
def test_cli_engine_route_prints_what_the_host_route_prints(case, extra, workdir):
    """IGD_HOST_MAX_QUERIES=0 (this marker's default): everything through igd_hip_support_sets"""
    db = os.path.join(GOLDEN, case, "db.igd")
    d = short_tmpdir("igq")
    try:
        files = _case_files(case) + _many_sets(d)
        for q in files[:2]:
            got = _run(["search", db, "-q", q, "-u"] + extra)
            want = _run(["search", db, "-q", q, "-u"] + extra, HOST)
            assert got.returncode == 0 and want.returncode == 0, got.stderr
            assert got.stdout == want.stdout and b"Query regions with a hit" in got.stdout
        lst = _write_list(d, files)
        got = _run(["search", db, "-Q", lst, "-u"] + extra)
        want = _run(["search", db, "-Q", lst, "-u"] + extra, HOST)
        assert got.returncode == 0 and want.returncode == 0, got.stderr
        assert got.stdout == want.stdout and got.stdout.count(b"Query set ") == len(files)
    finally:
        shutil.rmtree(d, ignore_errors=True)
