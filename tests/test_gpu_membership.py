"""GPU: per-query dataset membership (igd_hip_membership / igd_member_rows, Database.membership / membership_files /
membership_dev, `-w`).

    bit f & 31 of bits[q, f >> 5] = query q overlaps AT LEAST ONE record of file f;  nfiles_hit[q] = popcount of row q;
    nhit = the rows with any bit set (what support() returns)

Expected values come from the CPU oracle one query at a time (test_membership_host.oracle_member: each distinct query
once) and, for v = 0, from its enumeration; for the explicit rules from igdc_membership_host, which
tests/test_membership_host.py holds against the oracle.  Every row is handed to the engine full of ones: a call defines
every word, the bits above nfiles included."""
import ctypes as C
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sets_fixtures as F
from helpers import GOLDEN, ROOT, Oracle, short_tmpdir, write_bed, write_igd_numpy
from test_gpu_sets import DBS, SIZES, _db, _sets
from test_membership_host import MemberHost, assert_not_vacuous, check_rows, oracle_member, oracle_member_enum, pack_rows
from test_sets_cli import _case_files, _many_sets, _write_list
from test_support_host import FLAT, HOST, NEST, NOV, NUMPY_DBS, _run, clustered_db, mixed_queries, sparse_db

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igw")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def ones(db, nq):
    return np.full((nq, db.member_words), 0xffffffff, np.uint32)


def _check(db, orc, ichr, qs, qe, v, off=None, strict=False):
    """rows, nfiles_hit and nhit against the oracle; column sums per set against support_sets"""
    member, pairs = oracle_member(orc, ichr, qs, qe, v)
    if v == 0:
        assert np.array_equal(oracle_member_enum(orc, ichr, qs, qe), member)
        if strict:
            assert_not_vacuous(member, pairs)
    bits, nfh, nhit = db.membership(ichr, qs, qe, v, bits=ones(db, len(qs)))
    check_rows(bits, nfh, nhit, member, v)
    got = db.unpack_membership(bits, db.nfiles)
    assert got.shape == member.shape and np.array_equal(got, member)
    assert np.array_equal(got.sum(axis=1), nfh)                                  # popcount == nfiles_hit
    if off is not None:
        sup, snhit = db.support_sets(ichr, qs, qe, off, v)
        for k in range(len(off) - 1):
            a, b = off[k], off[k + 1]
            assert np.array_equal(got[a:b].sum(axis=0), sup[k]), (v, k)
            assert int((nfh[a:b] > 0).sum()) == snhit[k], (v, k)
    return bits, nfh, nhit


@pytest.mark.parametrize("v", [0, 500])
@pytest.mark.parametrize("case", range(len(DBS)))
def test_rows_equal_the_oracle(case, v, workdir):
    from igd_amd import Database
    rng = random.Random(900 + case)
    nbp, gtype, nfiles, nctg, span_tiles, dens, hot = DBS[case]
    path, span = _db(rng, workdir, "d%d" % case, nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
    (ichr, qs, qe), off = _sets(rng, nctg, nbp, span, SIZES)
    orc, db = Oracle(path), Database(path)
    try:
        _check(db, orc, ichr, qs, qe, v, off)
        if v == 0:
            # the explicit rules, with and without a filter: rows equal igdc_membership_host with the same rule
            H = MemberHost(path)
            try:
                for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300), (NEST, 300)):
                    got = db.membership(ichr, qs, qe, rule=rule, value_filter=vf, bits=ones(db, len(qs)))
                    want = H.membership(ichr, qs, qe, NOV if (vf is None or gtype == 0) else vf, rule)
                    for g, w in zip(got, want):
                        assert np.array_equal(g, w), (rule, vf)
            finally:
                H.close()
    finally:
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
    parts = [mixed_queries(rng, nctg, nbp, span, n) for n in (700, 5, 1100, 64)]
    off = np.zeros(5, np.int64)
    off[1:] = np.cumsum([len(p[1]) for p in parts])
    ichr, qs, qe = (np.concatenate([p[i] for p in parts]).astype(np.int32) for i in range(3))
    orc, db = Oracle(path), Database(path)
    try:
        bits, _, _ = _check(db, orc, ichr, qs, qe, v, off, strict=True)
        for i in range(5, 700, 5):                               # two identical query lines: two identical rows
            assert np.array_equal(bits[i], bits[i - 1])
    finally:
        db.close()
        orc.close()


def test_explicit_rules_differ_on_a_sparse_database(workdir):
    from igd_amd import Database
    rng = random.Random(4200)
    path, span, nbp = sparse_db(rng, workdir, "spw")
    ichr, qs, qe = mixed_queries(rng, 2, nbp, span, 2000)
    orc, db = Oracle(path), Database(path)
    try:
        nest, _ = oracle_member(orc, ichr, qs, qe, 0)
        flat, _ = oracle_member(orc, ichr, qs, qe, 1)           # values >= 1: rule FLAT, every record passes
        assert not np.array_equal(nest, flat)
        check_rows(*db.membership(ichr, qs, qe, rule=NEST, bits=ones(db, len(qs))), nest)
        check_rows(*db.membership(ichr, qs, qe, rule=FLAT, bits=ones(db, len(qs))), flat)
    finally:
        db.close()
        orc.close()


@pytest.mark.parametrize("nfiles", [1, 31, 32, 33, 64, 65])
def test_word_boundaries(nfiles, workdir):
    """file nfiles - 1 is the highest valid bit; the bits above it stay 0 in rows handed over full of ones"""
    from igd_amd import Database
    rng = random.Random(50 + nfiles)
    nbp = 1 << 14
    files = [[("chr1", 1000 * f + 10, 1000 * f + 400, rng.randint(0, 1000)), ("chr1", 1000 * f + 300, 1000 * f + 900, rng.randint(0, 1000)),
              ("chr1", 30 * nbp + 7 * f, 32 * nbp, 700)] for f in range(nfiles)]
    path = os.path.join(workdir, "wb%d.igd" % nfiles)
    write_igd_numpy(path, files, nbp=nbp, gtype=1)
    last = nfiles - 1
    ichr = np.zeros(6, np.int32)
    qs = np.array([1000 * last + 350, 0, 31 * nbp, 1000 * last + 950, 40 * nbp, 5], np.int32)
    qe = np.array([1000 * last + 360, 1000 * nfiles, 31 * nbp + 1, 1000 * last + 999, 41 * nbp, 6], np.int32)
    orc, db = Oracle(path), Database(path)
    try:
        assert db.member_words == (nfiles + 31) // 32
        for v in (0, 500):
            member, _ = oracle_member(orc, ichr, qs, qe, v)
            bits, nfh, nhit = db.membership(ichr, qs, qe, v, bits=ones(db, 6))
            check_rows(bits, nfh, nhit, member, v)
            if nfiles % 32:
                assert not (bits[:, -1] >> np.uint32(nfiles % 32)).any()
        member, _ = oracle_member(orc, ichr, qs, qe, 0)
        assert member[0, last] and member[0].sum() == 1 and member[1].all() and member[2].all() and not member[3].any()
    finally:
        db.close()
        orc.close()


@pytest.mark.parametrize("nfiles", [2081, 16383, 16384, 16385])
def test_file_count_edges(nfiles, workdir):
    """igd_member_rows at the edges of its LDS form: IGD_MEMBER_LDS_FILES = 16 384 files are 512 words, eight full steps of
    the stream-and-clear loop, with 16 383 below it and 16 385, the first wide form, above; 2 081 files are 66 words, no
    multiple of 64, with nfiles % 32 = 1.  The boundary files of sets_fixtures.wide_db (bit 0 and bit 31 of the first, 64th,
    65th and last word) lie under the window that an eighth of the queries covers."""
    from igd_amd import Database
    c = F.consts()
    assert c["IGD_MEMBER_LDS_FILES"] == 16384 and c["IGD_WAVE"] == 64
    nW = (nfiles + 31) // 32
    assert {2081: (66, 1), 16383: (512, 31), 16384: (512, 0), 16385: (513, 1)}[nfiles] == (nW, nfiles % 32)
    path, span, window, edge = F.wide_db(random.Random(8000 + nfiles), workdir, "e%d" % nfiles, nfiles, F.NBP,
                                         max(40, nfiles * 3 // 10))
    (ichr, qs, qe), off = F.make_sets(np.random.default_rng(nfiles), 1, F.NBP, span, [0, 1, 65, 234], window)
    assert len(qs) == 300 and edge == F.boundary_files(nfiles) and edge[-1] == nfiles - 1
    orc, db = Oracle(path), Database(path)
    try:
        assert db.member_words == nW
        for v in (0, 500):
            member, pairs = oracle_member(orc, ichr, qs, qe, v)
            if v == 0:
                assert_not_vacuous(member, pairs)
            assert member[:, edge].any(axis=0).all(), "a boundary file is in no row of the expectation"
            bits, nfh, nhit = db.membership(ichr, qs, qe, v, bits=ones(db, len(qs)))
            check_rows(bits, nfh, nhit, member, (nfiles, v))
            if nfiles % 32:
                assert not (bits[:, -1] >> np.uint32(nfiles % 32)).any()         # nfiles - 1 is the highest valid bit
            got = db.unpack_membership(bits, nfiles)
            assert got[:, edge].any(axis=0).all()
            sup, snhit = db.support_sets(ichr, qs, qe, off, v)
            for k in range(len(off) - 1):
                a, b = off[k], off[k + 1]
                assert np.array_equal(got[a:b].sum(axis=0), sup[k]) and int((nfh[a:b] > 0).sum()) == snhit[k], (nfiles, v, k)
            again, nfh2, nhit2 = db.membership(ichr, qs, qe, v, bits=ones(db, len(qs)))
            assert np.array_equal(again, bits) and np.array_equal(nfh2, nfh) and nhit2 == nhit
    finally:
        db.close()
        orc.close()


def test_a_wave_leaves_its_bitmap_clear_for_its_next_query(workdir):
    """More queries than two and a half times the waves of the kernel's largest grid: every wave meets a second and a third
    query.  A few hundred distinct queries are tiled in a fixed pattern -- one with hits in several words, one without a hit,
    one that hits other files -- in both orders of the last two, so that every kind follows every other kind in some wave.
    Every row equals the row of its distinct query: a bitmap that was not cleared, or cleared too early, shows."""
    from igd_amd import Database
    from igd_amd import _native as N
    rng = random.Random(61)
    nbp = 1 << 12
    path, span = clustered_db(rng, workdir, "reuse", nbp, 1, 100, 2, 30)
    waves = 4 * N.hip().igd_hip_member_grid(1 << 40)
    nq = (5 * waves) // 2 + 7
    assert nq < N.hip().igd_hip_max_batch()
    trip = []
    for _ in range(100):
        c = rng.randrange(2)
        s = rng.randrange(0, span - 8 * nbp)
        many = (c, s, s + 7 * nbp + 3)                              # long: files of several words
        none = rng.choice([(99, s, s + 50), (c, span + 9 * nbp + s, span + 9 * nbp + s + 700), (-1, s, s + 3 * nbp)])
        s = rng.randrange(0, span)
        few = (c, s, s + rng.choice([1, 200, 700]))
        trip.append((many, none, few))
    orc, db = Oracle(path), Database(path)
    try:
        for order in ((0, 1, 2), (0, 2, 1)):
            d = np.array([t[k] for t in trip for k in order], np.int32)
            member, _ = oracle_member(orc, d[:, 0], d[:, 1], d[:, 2], 0)
            words = (pack_rows(member) != 0).sum(axis=1).reshape(-1, 3)
            kinds = member.reshape(100, 3, -1)
            a, b, c = order.index(0), order.index(1), order.index(2)
            assert (words[:, a] >= 2).all() and (words[:, b] == 0).all()
            assert (kinds[:, c] & ~kinds[:, a]).any(), "no short query hits a file that its long neighbour does not"
            reps = -(-nq // len(d))
            ichr, qs, qe = (np.ascontiguousarray(np.tile(d[:, k], reps)[:nq]) for k in range(3))
            want = np.tile(member, (reps, 1))[:nq]
            check_rows(*db.membership(ichr, qs, qe, bits=ones(db, nq)), want, order)
    finally:
        db.close()
        orc.close()


def test_more_files_than_the_lds_form(workdir):
    """20 000 files: no bitmap in LDS, the lanes OR into rows that the call zeroes on the stream"""
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
        assert db.member_words == 625
        for v in (0, 500):
            first, nfh, nhit = _check(db, orc, ichr, qs, qe, v, off, strict=(v == 0))
            again, nfh2, nhit2 = db.membership(ichr, qs, qe, v, bits=ones(db, len(qs)))
            assert np.array_equal(again, first) and np.array_equal(nfh2, nfh) and nhit2 == nhit
    finally:
        db.close()
        orc.close()


SEAM = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import Oracle, short_tmpdir
import test_support_host as S
import test_membership_host as M
from igd_amd import Database
d = short_tmpdir("igb")
rng = random.Random(11)
path, span = S.clustered_db(rng, d, "b", 1 << 12, 1, 40, 2, 20)
orc, db = Oracle(path), Database(path)
row = 4 * db.member_words
assert row == 8
for n in (0, 1, 96, 97, 98, 500):
    ichr, qs, qe = S.mixed_queries(rng, 2, 1 << 12, span, n)
    for v in (0, 500):
        member, _ = M.oracle_member(orc, ichr, qs, qe, v)
        bits = np.full((n, db.member_words), 0xffffffff, np.uint32)
        M.check_rows(*db.membership(ichr, qs, qe, v, bits=bits), member, (n, v))
        assert n < 96 or member.any()
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "97"}, {"IGD_HIP_MEMBER_ROW_BYTES": "25"}])
def test_calls_straddle_the_chunk_seams(env):
    """IGD_HIP_MAX_BATCH lowered to 97 queries; the row budget lowered to a little over three rows of 8 bytes (both read
    once per process): calls of 0, 1, 96, 97, 98 and 500 queries"""
    p = subprocess.run([sys.executable, "-c", SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env),
                       timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def test_resident_rows_on_a_torch_stream(workdir):
    import torch
    from igd_amd import Database
    from igd_amd import _native as N
    rng = random.Random(71)
    nbp = 1 << 12
    path, span = clustered_db(rng, workdir, "dev", nbp, 1, 40, 2, 20)
    ichr, qs, qe = mixed_queries(rng, 2, nbp, span, 3000)
    db = Database(path)
    try:
        want_bits, want_nfh, want_nhit = db.membership(ichr, qs, qe, 500)
        assert want_nhit > 0
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            t = [torch.from_numpy(a).to(dev) for a in (ichr, qs, qe)]
            bits = torch.full((len(qs), db.member_words), -1, dtype=torch.int32, device=dev)
            nfh = torch.full((len(qs),), -1, dtype=torch.int32, device=dev)
            nhit = torch.full((1,), 5, dtype=torch.int64, device=dev)
            stream.synchronize()
            db.membership_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(qs), bits.data_ptr(), nfh.data_ptr(),
                              nhit.data_ptr(), v=500, stream=stream.cuda_stream)
            db.sync(stream.cuda_stream)
            assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_bits)
            assert np.array_equal(nfh.cpu().numpy(), want_nfh) and int(nhit.item()) == 5 + want_nhit     # d_nhit is added to
            # without d_nfiles_hit and d_nhit the rows are still filled
            bits.fill_(-1)
            stream.synchronize()
            db.membership_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(qs), bits.data_ptr(), v=500,
                              stream=stream.cuda_stream)
            db.sync(stream.cuda_stream)
            assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_bits)
            # more queries than one engine batch: refused, not chunked silently
            rc = N.hip().igd_hip_membership_dev(db.dev, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                                N.hip().igd_hip_max_batch() + 1, N.IGD_HIP_NO_VALUE_FILTER, NEST,
                                                bits.data_ptr(), None, None, stream.cuda_stream)
            assert rc == -2
            db.sync(stream.cuda_stream)
            assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_bits)
    finally:
        db.close()


def test_bad_arguments_change_nothing_and_empty_calls_are_fine(workdir):
    from igd_amd import Database
    from igd_amd import _native as N
    from igd_amd.database import IgdError
    rng = random.Random(6)
    path, span = _db(rng, workdir, "bad", 1 << 14, 1, 4, 1, 8, 30)
    (ichr, qs, qe), _ = _sets(rng, 1, 1 << 14, span, [20])
    db = Database(path)
    H = N.hip()
    try:
        bits = np.full((20, 1), 7, np.uint32)
        nfh = np.full(20, 7, np.int32)
        nhit = C.c_int64(7)
        q = (ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data)
        for args in ((q[0], q[1], q[2], 20, NOV, NEST, None, nfh.ctypes.data),            # no rows with nq > 0
                     (q[0], q[1], q[2], -1, NOV, NEST, bits.ctypes.data, nfh.ctypes.data),  # negative nq
                     (q[0], q[1], q[2], 20, NOV, 2, bits.ctypes.data, nfh.ctypes.data),     # no such rule
                     (None, q[1], q[2], 20, NOV, FLAT, bits.ctypes.data, nfh.ctypes.data)):
            assert H.igd_hip_membership(db.dev, *args, C.byref(nhit)) == -2             # IGD_HIP_ERR_ARG
            assert (bits == 7).all() and (nfh == 7).all() and nhit.value == 7
        assert H.igd_hip_membership(db.dev, None, None, None, 0, NOV, NEST, None, None, None) == 0
        b, n, h = db.membership(ichr[:0], qs[:0], qe[:0])
        assert b.shape == (0, 1) and n.shape == (0,) and h == 0
        with pytest.raises(IgdError):
            db.membership(ichr, qs, qe, bits=np.zeros((20, 2), np.uint32))
        with pytest.raises(IgdError):
            db.membership(ichr, qs, qe, bits=np.zeros((20, 1), np.int64))
    finally:
        db.close()


def test_membership_files_equals_membership_per_file(workdir):
    from igd_amd import Database
    rng = random.Random(8)
    nbp = 1 << 14
    path, span = clustered_db(rng, workdir, "sf", nbp, 1, 8, 2, 8)
    paths = []
    for k, n in enumerate([0, 1, 50, 700, 9]):
        p = os.path.join(workdir, "mf%d.bed" % k)
        rows = []
        for _ in range(n):
            s = rng.randrange(0, span)
            rows.append((rng.choice(["chr1", "chr2", "chrX"]), s, s + rng.randint(1, 2 * nbp)))
        write_bed(p, rows)
        paths.append(p)
    orc, db = Oracle(path), Database(path)
    try:
        for v in (0, 500):
            bits, nfh, nhit, off = db.membership_files(paths, v)
            assert nhit.shape == (len(paths),) and off.shape == (len(paths) + 1,) and off[-1] == len(nfh) == len(bits)
            for k, p in enumerate(paths):
                q = db.read_queries(p)
                assert off[k + 1] - off[k] == len(q[1])
                b1, n1, h1 = db.membership(*q, v)
                assert np.array_equal(bits[off[k]:off[k + 1]], b1) and np.array_equal(nfh[off[k]:off[k + 1]], n1) and nhit[k] == h1
                member, _ = oracle_member(orc, *orc.read_queries(p), v)
                check_rows(b1, n1, h1, member, (v, k))
    finally:
        db.close()
        orc.close()


@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("gtype0", ["-v", "500"]),
                                        ("edge", [])])
def test_cli_engine_route_prints_what_the_host_route_prints(case, extra, workdir):
    """IGD_HOST_MAX_QUERIES=0 (this marker's default): everything through igd_hip_membership"""
    db = os.path.join(GOLDEN, case, "db.igd")
    d = short_tmpdir("igq")
    try:
        files = _case_files(case) + _many_sets(d)
        for q in files[:2]:
            got = _run(["search", db, "-q", q, "-w"] + extra)
            want = _run(["search", db, "-q", q, "-w"] + extra, HOST)
            assert got.returncode == 0 and want.returncode == 0, got.stderr
            assert got.stdout == want.stdout and b"Query regions with a hit" in got.stdout
        lst = _write_list(d, files)
        got = _run(["search", db, "-Q", lst, "-w"] + extra)
        want = _run(["search", db, "-Q", lst, "-w"] + extra, HOST)
        assert got.returncode == 0 and want.returncode == 0, got.stderr
        assert got.stdout == want.stdout and got.stdout.count(b"Query set ") == len(files)
    finally:
        shutil.rmtree(d, ignore_errors=True)
