"""GPU: dataset co-occurrence (igd_hip_cooccur = igd_hip_membership_dev + igd_bits_transpose + igd_bitrows_gram per chunk;
Database.cooccurrence / cooccurrence_files / transpose_bits / bitrows_gram, `igd search -q F -C` on the engine route).

The two kernels are held against cooccur_ref (np.unpackbits and an integer matrix product) through their generic entries;
the co-occurrence against member.T @ member on the CPU oracle's membership, one region at a time
(test_membership_host.oracle_member).  Every integer must be EQUAL.  Every output is handed to the engine full of ones or
of garbage: a call defines every word of it.  The decomposition of the Gram kernel (tile edge, K-step, slices) is read
from the engine's accessors."""
import ctypes as C
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cooccur_ref as CR
import sets_fixtures as F
from helpers import GOLDEN, ROOT, Oracle, short_tmpdir
from test_enrich_host import enrich_fixture
from test_gpu_sets import DBS, _db, _sets
from test_membership_host import oracle_member
from test_sets_cli import _case_files
from test_support_host import FLAT, HOST, NEST, NOV, _run, clustered_db, mixed_queries

pytestmark = pytest.mark.gpu
ENGINE = {"IGD_HOST_MAX_QUERIES": "0"}
SIZES = [300, 0, 65, 700]
GARBAGE = 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igc")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def anydb(workdir):
    """a small database: the generic entries need a handle for its device and workspaces, not its records"""
    from igd_amd import Database
    path, _ = clustered_db(random.Random(3), workdir, "any", 1 << 12, 1, 6, 1, 8)
    db = Database(path)
    yield db
    db.close()


def H():
    from igd_amd import _native as N
    return N.hip()


# ---- igd_bits_transpose -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["half", "ones"])
def test_transpose_equals_unpackbits(anydb, kind):
    """1 .. 257 rows: one ragged block, exactly one, one and a bit, five; 513 and 1 100 rows: a second and a third workgroup
    of a word column (eight 64-row blocks each).  1, 2 and 17 words per row."""
    rs = np.random.default_rng(21)
    for nrows in (1, 63, 64, 65, 257, 513, 1100):
        for nW in (1, 2, 17):
            bits = CR.random_rows(rs, nrows, nW, kind)
            cols = np.full((32 * nW, (nrows + 63) // 64), 0xffffffffffffffff, np.uint64)
            got = anydb.transpose_bits(bits, cols=cols)
            assert got is cols and np.array_equal(got, CR.transpose(bits)), (nrows, nW)
            if nrows % 64:                                       # bits at positions >= nrows are 0 in every column
                assert not (got[:, -1] >> np.uint64(nrows % 64)).any(), (nrows, nW)
            if kind == "ones":
                assert int(sum(bin(int(x)).count("1") for x in got.ravel())) == nrows * 32 * nW
    assert anydb.transpose_bits(np.zeros((0, 3), np.uint32)).shape == (96, 0)
    assert anydb.transpose_bits(np.zeros((5, 0), np.uint32)).shape == (0, 1)


# ---- igd_bitrows_gram ---------------------------------------------------------------------------------------------------------
def widths():
    """1, 2, 3 uint32 words; one K-step of 64-bit words less a half, exactly, plus a half; two steps and a half; and the
    narrowest power of two at which a 129 x 129 product is cut into at least two slices"""
    k = int(H().igd_hip_gram_kstep())
    assert k >= 2 and int(H().igd_hip_gram_tile()) == 64
    w = 64
    while H().igd_hip_gram_slices(129, 129, w) < 2:
        w *= 2
        assert w <= 1 << 16, "no width up to 2^16 words is sliced"
    assert H().igd_hip_gram_slices(129, 129, 1) == 1
    return [1, 2, 3, 2 * k - 1, 2 * k, 2 * k + 1, 4 * k + 1], w


@pytest.mark.parametrize("kind", ["half", "sparse", "ones"])
def test_gram_rectangular_equals_the_reference(anydb, kind):
    """m, n in 1, 63, 64, 65, 129: at 129 a second tile with a ragged edge"""
    rs = np.random.default_rng(31)
    ws, wide = widths()
    for nw in ws + [wide]:
        sizes = (1, 63, 64, 65, 129) if nw != wide else (65, 129)
        rows = {n: CR.random_rows(rs, n, nw, kind) for n in sizes}
        other = {n: CR.random_rows(rs, n, nw, kind) for n in sizes}
        for m in sizes:
            for n in sizes:
                out = np.full((m, n), GARBAGE, np.int64)
                got = anydb.bitrows_gram(rows[m], other[n], out=out)
                assert got is out and np.array_equal(got, CR.gram(rows[m], other[n])), (m, n, nw)
                if kind == "ones":
                    assert (got == 32 * nw).all(), (m, n, nw)     # (a wrong tail pad would add or lose bits)
    assert H().igd_hip_gram_slices(129, 129, wide) >= 2


@pytest.mark.parametrize("kind", ["half", "sparse", "ones"])
def test_gram_symmetric_equals_the_rectangular_form(anydb, kind):
    """129 rows: tiles (0,0), (0,1), (1,1) -- a mirrored off-diagonal tile with a ragged edge; 200 rows: four tiles a side"""
    rs = np.random.default_rng(41)
    ws, wide = widths()
    for nw in ws + [wide]:
        for m in (1, 63, 64, 65, 129) if nw != wide else (129, 200):
            a = CR.random_rows(rs, m, nw, kind)
            want = CR.gram(a)
            sym = anydb.bitrows_gram(a, out=np.full((m, m), GARBAGE, np.int64))
            rect = anydb.bitrows_gram(a, a, out=np.full((m, m), GARBAGE, np.int64))
            assert np.array_equal(sym, want) and np.array_equal(rect, want), (m, nw)
            assert np.array_equal(sym, sym.T)
            assert H().igd_hip_gram_slices(m, 0, nw) >= 1
    assert H().igd_hip_gram_slices(129, 0, wide) >= 2
    assert anydb.bitrows_gram(np.zeros((0, 4), np.uint32)).shape == (0, 0)
    z = anydb.bitrows_gram(np.zeros((3, 0), np.uint32), out=np.full((3, 3), GARBAGE, np.int64))
    assert z.shape == (3, 3) and not z.any()


def test_gram_bad_arguments_write_nothing(anydb):
    a = np.ones((4, 2), np.uint32)
    out = np.full((4, 4), 7, np.int64)
    L = H()
    for args in ((None, 4, None, 0, 2, out.ctypes.data), (a.ctypes.data, -1, None, 0, 2, out.ctypes.data),
                 (a.ctypes.data, 4, None, 0, -2, out.ctypes.data), (a.ctypes.data, 4, None, 0, 2, None),
                 (a.ctypes.data, 1 << 15, a.ctypes.data, 1 << 15, 2, out.ctypes.data)):
        assert L.igd_hip_bitrows_gram(anydb.dev, *args) == -2
        assert (out == 7).all()
    cols = np.full((64, 1), 7, np.uint64)
    assert L.igd_hip_bits_transpose(anydb.dev, None, 4, 2, cols.ctypes.data) == -2
    assert L.igd_hip_bits_transpose(anydb.dev, a.ctypes.data, -4, 2, cols.ctypes.data) == -2
    assert (cols == 7).all()


# ---- igd_hip_cooccur ----------------------------------------------------------------------------------------------------------
def check_cooc(db, cooc, nhit, member, ichr, qs, qe, what, **kw):
    want = CR.cooc(member)
    assert cooc.dtype == np.int64 and cooc.shape == want.shape, what
    assert np.array_equal(cooc, want), what
    assert np.array_equal(cooc, cooc.T), what
    assert nhit == int(member.any(axis=1).sum()), what
    sup, snhit = db.support_sets(ichr, qs, qe, np.array([0, len(qs)], np.int64), **kw)
    assert np.array_equal(np.diagonal(cooc), sup[0]) and nhit == snhit[0], what


def ones_matrix(db):
    return np.ones((db.nfiles, db.nfiles), np.int64)


@pytest.mark.parametrize("v", [0, 500])
@pytest.mark.parametrize("case", range(len(DBS)))
def test_cooccurrence_equals_the_oracle(case, v, workdir):
    from igd_amd import Database
    rng = random.Random(900 + case)
    nbp, gtype, nfiles, nctg, span_tiles, dens, hot = DBS[case]
    path, span = _db(rng, workdir, "d%d" % case, nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
    (ichr, qs, qe), _ = _sets(rng, nctg, nbp, span, SIZES)
    orc, db = Oracle(path), Database(path)
    try:
        member, _ = oracle_member(orc, ichr, qs, qe, v)
        if v == 0:
            assert (CR.cooc(member) - np.diag(member.sum(axis=0))).any(), "no two files share a region"
        m = ones_matrix(db)
        cooc, nhit = db.cooccurrence(ichr, qs, qe, v, cooc=m)
        assert cooc is m
        check_cooc(db, cooc, nhit, member, ichr, qs, qe, (case, v), v=v)
        if v == 0:
            # the explicit rules, with and without a filter: member from membership() with the same rule
            for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300), (NEST, 300)):
                bits, _, _ = db.membership(ichr, qs, qe, rule=rule, value_filter=vf)
                mem = db.unpack_membership(bits, nfiles)
                cooc, nhit = db.cooccurrence(ichr, qs, qe, rule=rule, value_filter=vf, cooc=ones_matrix(db))
                check_cooc(db, cooc, nhit, mem, ichr, qs, qe, (case, rule, vf), rule=rule, value_filter=vf)
            # two identical region lists count twice; no region gives a zero matrix
            twice, nh2 = db.cooccurrence(np.tile(ichr, 2), np.tile(qs, 2), np.tile(qe, 2), cooc=ones_matrix(db))
            once, nh1 = db.cooccurrence(ichr, qs, qe)
            assert np.array_equal(twice, 2 * once) and nh2 == 2 * nh1
            zero, nh0 = db.cooccurrence(ichr[:0], qs[:0], qe[:0], cooc=ones_matrix(db))
            assert not zero.any() and nh0 == 0
    finally:
        db.close()
        orc.close()


@pytest.mark.parametrize("nfiles", [33, 65, 2081])
def test_wide_databases(nfiles, workdir):
    """33 files: a second row word; 65 files: a second tile with one row in it, a third word; 2 081 files: 33 tiles a side,
    66 words -- a lane's second word in igd_member_rows -- and nfiles % 32 = 1.  The boundary files of
    sets_fixtures.wide_db lie under a window that an eighth of the regions covers."""
    from igd_amd import Database
    path, span, window, edge = F.wide_db(random.Random(8000 + nfiles), workdir, "w%d" % nfiles, nfiles, F.NBP, max(40, nfiles * 3 // 10))
    (ichr, qs, qe), _ = F.make_sets(np.random.default_rng(nfiles), 1, F.NBP, span, [0, 1, 65, 234], window)
    orc, db = Oracle(path), Database(path)
    try:
        for v in (0, 500):
            member, _ = oracle_member(orc, ichr, qs, qe, v)
            want = CR.cooc(member)
            assert (want[np.ix_(edge, edge)] > 0).all(), "two boundary files share no region"
            cooc, nhit = db.cooccurrence(ichr, qs, qe, v, cooc=ones_matrix(db))
            check_cooc(db, cooc, nhit, member, ichr, qs, qe, (nfiles, v), v=v)
    finally:
        db.close()
        orc.close()


SEAM = r"""
import ctypes as C, os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import Oracle, short_tmpdir
import test_support_host as S
import test_membership_host as M
import cooccur_ref as CR
from igd_amd import Database
from igd_amd import _native as N
d = short_tmpdir("igk")
rng = random.Random(12)
path, span = S.clustered_db(rng, d, "b", 1 << 12, 1, 40, 2, 20)
orc, db = Oracle(path), Database(path)
assert 4 * db.member_words == 8
if os.environ.get("IGD_HIP_COOCCUR_MAX_FILES"):
    ichr, qs, qe = S.mixed_queries(rng, 2, 1 << 12, span, 50)
    cooc = np.full((40, 40), 7, np.int64)
    nhit = C.c_int64(7)
    rc = N.hip().igd_hip_cooccur(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, 50, S.NOV, S.NEST, cooc.ctypes.data, C.byref(nhit))
    assert rc == -2 and (cooc == 7).all() and nhit.value == 7, rc
    assert b"more than 39" in N.hip().igd_hip_last_error()
else:
    for n in (0, 1, 99, 100, 101, 333):
        ichr, qs, qe = S.mixed_queries(rng, 2, 1 << 12, span, n)
        for v in (0, 500):
            member, _ = M.oracle_member(orc, ichr, qs, qe, v)
            cooc, nhit = db.cooccurrence(ichr, qs, qe, v, cooc=np.ones((40, 40), np.int64))
            assert np.array_equal(cooc, CR.cooc(member)), (n, v)
            assert nhit == int(member.any(axis=1).sum()), (n, v)
            assert n < 99 or cooc.any()
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


@pytest.mark.parametrize("env", [{"IGD_HIP_MEMBER_ROW_BYTES": "800"}, {"IGD_HIP_MAX_BATCH": "97"}, {"IGD_HIP_COOCCUR_MAX_FILES": "39"}])
def test_chunk_seams_and_the_file_limit(env):
    """The row budget lowered to 100 rows of 8 bytes, the batch to 97 regions (both read once per process): 333 regions run
    in four chunks whose ends (100, 200, 300 / 97, 194, 291) are no multiples of 64 -- the tail bits of a chunk's last
    column word must be zero.  The file limit lowered to 39 on a database of 40 files: refused, nothing written."""
    p = subprocess.run([sys.executable, "-c", SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env),
                       timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def test_bad_arguments_write_nothing(anydb):
    L = H()
    n = anydb.nfiles
    ichr, qs, qe = np.zeros(4, np.int32), np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32) + 500
    cooc = np.full((n, n), 7, np.int64)
    nhit = C.c_int64(7)
    q = (ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data)
    for args in ((None, q[1], q[2], 4, NOV, NEST, cooc.ctypes.data), (q[0], q[1], q[2], -1, NOV, NEST, cooc.ctypes.data),
                 (q[0], q[1], q[2], 4, NOV, 2, cooc.ctypes.data), (q[0], q[1], q[2], 4, NOV, FLAT, None)):
        assert L.igd_hip_cooccur(anydb.dev, *args, C.byref(nhit)) == -2
        assert (cooc == 7).all() and nhit.value == 7
    from igd_amd.database import IgdError
    with pytest.raises(IgdError):
        anydb.cooccurrence(ichr, qs, qe, cooc=np.zeros((n, n + 1), np.int64))


# ---- cross-check with the restricted sets ---------------------------------------------------------------------------------------
def test_gram_reproduces_the_restricted_supports(workdir):
    """bitrows_gram(R.bits, transpose of the universe's membership) is enrichment_restricted's support; the diagonal of
    bitrows_gram(R.bits) is its size"""
    from igd_amd import Database
    path, upath, sets, _ = enrich_fixture(workdir, nfiles=40, name="gc")
    db = Database(path)
    try:
        q = [db.read_queries(p) for p in sets]
        off = np.zeros(len(q) + 1, np.int64)
        off[1:] = np.cumsum([len(s[1]) for s in q])
        cat = tuple(np.concatenate([s[i] for s in q]).astype(np.int32) for i in range(3))
        uni = db.read_queries(upath)
        nu = len(uni[1])
        for kw in (dict(), dict(v=400)):
            r = db.enrichment_restricted(*cat, off, *uni, **kw)
            assert r.support.any() and (r.size > 0).all()
            bits, _, _ = db.membership(*uni, **kw)
            cols = db.transpose_bits(bits)                            # uint64[32 * nW, ceil(nu / 64)]
            assert np.array_equal(cols, CR.transpose(bits))
            colw = np.ascontiguousarray(cols[:db.nfiles]).view(np.uint32)
            rb = np.zeros((len(sets), colw.shape[1]), np.uint32)
            rb[:, :r.bits.shape[1]] = r.bits
            assert np.array_equal(db.bitrows_gram(rb, colw), r.support), kw
            overlap = db.bitrows_gram(r.bits)
            assert np.array_equal(np.diagonal(overlap), r.size) and np.array_equal(overlap, CR.gram(r.bits))
            # and the co-occurrence over the universe is the symmetric product of the columns
            cooc, nhit = db.cooccurrence(*uni, **kw)
            assert np.array_equal(cooc, db.bitrows_gram(colw)) and np.array_equal(np.diagonal(cooc), r.usupport)
        assert nu > 2000
    finally:
        db.close()


# ---- command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("edge", [])])
def test_cli_engine_route_prints_what_the_host_route_prints(case, extra):
    db = os.path.join(GOLDEN, case, "db.igd")
    for q in _case_files(case)[:2]:
        got = _run(["search", db, "-q", q, "-C"] + extra, ENGINE)
        want = _run(["search", db, "-q", q, "-C"] + extra, HOST)
        assert got.returncode == 0 and want.returncode == 0, got.stderr
        assert got.stdout == want.stdout and got.stdout.startswith(b"index_a\tindex_b\t") and b"Query regions with a hit" in got.stdout


def test_cooccurrence_files_is_what_C_prints(workdir):
    from igd_amd import Database, jaccard
    dbp, q = os.path.join(GOLDEN, "branch", "db.igd"), os.path.join(GOLDEN, "branch", "q.bed")
    db = Database(dbp)
    try:
        cooc, nhit = db.cooccurrence_files(q)
        j = jaccard(cooc)
        lines = _run(["search", dbp, "-q", q, "-C"], ENGINE).stdout.decode().splitlines()
        pairs = [(a, b) for a in range(db.nfiles) for b in range(a + 1, db.nfiles) if cooc[a, b] > 0]
        assert pairs and len(lines) == len(pairs) + 2
        for line, (a, b) in zip(lines[1:], pairs):
            f = line.split("\t")
            assert [int(x) for x in f[:5]] == [a, b, cooc[a, a], cooc[b, b], cooc[a, b]] and f[5] == "%.6f" % j[a, b]
        assert lines[-1] == "Query regions with a hit: %d of %d" % (nhit, len(db.read_queries(q)[1]))
    finally:
        db.close()
