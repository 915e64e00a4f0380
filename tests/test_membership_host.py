"""Per-query dataset membership without a GPU: igdc_membership_host (igd_hostpath.c) and `igd search -q F -w` / `-Q list -w`
on the host route.

    member[q][f] = 1 iff query q overlaps at least one record of file f      row q: ceil(nfiles / 32) uint32 words,
    nfiles_hit[q] = popcount of row q;  nhit = the rows with any bit set      file f = bit f & 31 of word f >> 5

The expected values never come from the code under test.  They come from the CPU oracle, one query at a time
(helpers.Oracle.search on a batch of one, then `> 0`; a batch of repeated queries asks it once per distinct query), for
v = 0 a second time from the oracle's enumeration (distinct (query, idx) pairs), and from the reference binary's `-f`
listing (marker `ref`).

Non-vacuity, from the oracle: some query meets two files or more, some query meets one file through several records (so
n < pairs: a build that counted pairs would print another n), some row is all zero."""
import ctypes as C
import os
import random
import shutil

import numpy as np
import pytest

from helpers import GOLDEN, Oracle, have_ref, run_ref, short_tmpdir, write_bed
from test_golden_oracle import CASES, materialize
from test_sets_cli import _case_files, _write_list
from test_support_host import (FLAT, HOST, NEST, NOV, NUMPY_DBS, HostDb, _index, _run, cli_rule, clustered_db, mixed_queries,
                               sparse_db)


# ---- expected values from the oracle -------------------------------------------------------------------------------------
def oracle_member(orc, ichr, qs, qe, v=0):
    """(member bool[nq, nfiles], pairs int64[nq]): Oracle.search on one query at a time, each distinct query once"""
    seen = {}
    member = np.zeros((len(qs), orc.nfiles), bool)
    pairs = np.zeros(len(qs), np.int64)
    for i in range(len(qs)):
        key = (int(ichr[i]), int(qs[i]), int(qe[i]))
        if key not in seen:
            h, _ = orc.search(ichr[i:i + 1], qs[i:i + 1], qe[i:i + 1], v)
            seen[key] = (h > 0, int(h.sum()))
        member[i], pairs[i] = seen[key]
    return member, pairs


def oracle_member_enum(orc, ichr, qs, qe):
    """the same matrix for v = 0 from the oracle's enumeration: distinct (query, idx) pairs"""
    qoff, rec = orc.enumerate(ichr, qs, qe)
    qno = np.repeat(np.arange(len(qs), dtype=np.int64), np.diff(qoff))
    idx = rec[:, 0].astype(np.int64)
    ok = (idx >= 0) & (idx < orc.nfiles)
    member = np.zeros((len(qs), orc.nfiles), bool)
    member[qno[ok], idx[ok]] = True
    return member


def pack_rows(member):
    """bool[nq, nfiles] -> uint32[nq, ceil(nfiles / 32)], file f = bit f & 31 of word f >> 5"""
    nq, nf = member.shape
    nW = (nf + 31) // 32
    wide = np.zeros((nq, nW * 32), np.uint8)
    wide[:, :nf] = member
    return np.packbits(wide, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(nq, nW)


def assert_not_vacuous(member, pairs):
    n = member.sum(axis=1)
    assert (n <= pairs).all()
    assert (n >= 2).any(), "no query meets two files"
    assert (n < pairs).any(), "no query meets one file through several records"
    assert (n == 0).any(), "no all-zero row"


# ---- igdc_membership_host through ctypes ---------------------------------------------------------------------------------
class MemberHost(HostDb):
    def membership(self, ichr, qs, qe, v, rule, nhit0=0, want_nf=True):
        """rows and nfiles_hit are handed over full of ones: the call must define every word of them"""
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        nW = (self.nfiles + 31) // 32
        bits = np.full((len(qs), nW), 0xffffffff, np.uint32)
        nfh = np.full(len(qs), -1, np.int32)
        nhit = C.c_int64(nhit0)
        rc = self.L.igdc_membership_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), v, rule,
                                         bits.ctypes.data if bits.size else None, nfh.ctypes.data if want_nf else None,
                                         C.byref(nhit))
        assert rc == 0
        return bits, nfh, nhit.value


def check_rows(bits, nfh, nhit, member, what=None):
    """the three results against the oracle's matrix, exactly; the padding bits of the last word included"""
    assert bits.dtype == np.uint32 and bits.shape == (member.shape[0], (member.shape[1] + 31) // 32), what
    assert np.array_equal(bits, pack_rows(member)), what
    assert np.array_equal(nfh, member.sum(axis=1)), what
    assert nhit == int(member.any(axis=1).sum()), what


@pytest.fixture
def tmp():
    d = short_tmpdir("imb")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", t)
    os.environ.pop("IGD_HOST_THREADS", None)


def _tiled(ichr, qs, qe, member, n=7 * 2048 + 5):
    """the queries repeated until seven host threads are worth starting (one per 2048 queries), and their rows"""
    reps = -(-n // len(qs))
    return np.tile(ichr, reps), np.tile(qs, reps), np.tile(qe, reps), np.tile(member, (reps, 1))


def _host_equals_oracle(path, ichr, qs, qe, host_threads, strict):
    orc, H = Oracle(path), MemberHost(path)
    try:
        assert H.nfiles == orc.nfiles
        for v in (0, 500):
            member, pairs = oracle_member(orc, ichr, qs, qe, v)
            if v == 0:
                assert np.array_equal(oracle_member_enum(orc, ichr, qs, qe), member)
                if strict:
                    assert_not_vacuous(member, pairs)
            rule, ev = cli_rule(orc.gtype, v)
            tc, ts, te, tm = _tiled(ichr, qs, qe, member)
            for threads in ("1", "3", "7"):
                host_threads(threads)
                check_rows(*H.membership(ichr, qs, qe, ev, rule), member, (v, threads))
                check_rows(*H.membership(tc, ts, te, ev, rule), tm, (v, threads, "tiled"))
        # nhit is ADDED to, nfiles_hit may be NULL, an empty call is fine
        rule, ev = cli_rule(orc.gtype, 0)
        member, _ = oracle_member(orc, ichr, qs, qe, 0)
        bits, _, nhit = H.membership(ichr, qs, qe, ev, rule, nhit0=11, want_nf=False)
        assert np.array_equal(bits, pack_rows(member)) and nhit == 11 + int(member.any(axis=1).sum())
        bits, _, nhit = H.membership(ichr[:0], qs[:0], qe[:0], ev, rule)
        assert bits.shape[0] == 0 and nhit == 0
    finally:
        H.close()
        orc.close()


@pytest.mark.parametrize("case", CASES)
def test_host_membership_equals_the_oracle_on_the_golden_families(case, host_threads):
    d, dst, man = materialize(case)
    try:
        path = os.path.join(dst, "db.igd")
        orc = Oracle(path)
        ichr, qs, qe = orc.read_queries(os.path.join(dst, "q.bed"))
        orc.close()
        if len(qs) > 1500:                                   # (config1: 10 000 queries; one oracle call per query)
            ichr, qs, qe = ichr[:1500], qs[:1500], qe[:1500]
        _host_equals_oracle(path, ichr, qs, qe, host_threads, strict=False)
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_membership_equals_the_oracle_on_clustered_databases(case, tmp, host_threads):
    rng = random.Random(4100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    path, span = clustered_db(rng, tmp, "c%d" % case, nbp, gtype, nfiles, nctg, span_tiles)
    ichr, qs, qe = mixed_queries(rng, nctg, nbp, span, 1500)
    _host_equals_oracle(path, ichr, qs, qe, host_threads, strict=True)


def test_explicit_rules_differ_on_a_sparse_database(tmp, host_threads):
    rng = random.Random(4200)
    path, span, nbp = sparse_db(rng, tmp)
    ichr, qs, qe = mixed_queries(rng, 2, nbp, span, 2000)
    orc, H = Oracle(path), MemberHost(path)
    try:
        nest, _ = oracle_member(orc, ichr, qs, qe, 0)
        flat, _ = oracle_member(orc, ichr, qs, qe, 1)          # values >= 1: rule FLAT, every record passes
        flat5, _ = oracle_member(orc, ichr, qs, qe, 500)
        assert not np.array_equal(nest, flat), "the two rules do not differ on this fixture"
        for threads in ("1", "4"):
            host_threads(threads)
            check_rows(*H.membership(ichr, qs, qe, NOV, NEST), nest)
            check_rows(*H.membership(ichr, qs, qe, NOV, FLAT), flat)
            check_rows(*H.membership(ichr, qs, qe, 1, FLAT), flat)
            check_rows(*H.membership(ichr, qs, qe, 500, FLAT), flat5)
    finally:
        H.close()
        orc.close()


def test_identical_query_lines_have_identical_rows(tmp):
    rng = random.Random(31)
    nbp = 1 << 14
    path, span = clustered_db(rng, tmp, "one", nbp, 1, 40, 2, 10)
    ichr, qs, qe = mixed_queries(rng, 2, nbp, span, 300)
    H = MemberHost(path)
    try:
        bits, nfh, _ = H.membership(ichr, qs, qe, NOV, NEST)
        for i in range(5, 300, 5):                               # mixed_queries repeats every fifth query
            assert np.array_equal(bits[i], bits[i - 1]) and nfh[i] == nfh[i - 1]
        assert bits.any()
    finally:
        H.close()


# ---- command line ---------------------------------------------------------------------------------------------------------
def expected_text(db, orc, qfile, v):
    """the text of `igd search db -q qfile -w [-v v]`, from the oracle; also (member, pairs)"""
    try:
        ichr, qs, qe = orc.read_queries(qfile)
    except IOError:
        ichr = qs = qe = np.zeros(0, np.int32)
    member, pairs = oracle_member(orc, ichr, qs, qe, v)
    names = orc.ctg_names()
    out = []
    for i in range(len(qs)):
        files = np.flatnonzero(member[i])
        out.append("%s\t%d\t%d\t%d\t%s\n" % (names[ichr[i]], qs[i], qe[i], len(files), ",".join(map(str, files)) if len(files) else "."))
    out.append("Query regions with a hit: %d of %d\n" % (member.any(axis=1).sum(), len(qs)))
    return "".join(out), member, pairs


CLI_CASES = [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("gtype0", ["-v", "500"]), ("edge", []), ("edge", ["-v", "500"])]


@pytest.mark.parametrize("case,extra", CLI_CASES)
def test_cli_w_prints_the_oracles_rows_on_the_host_route(case, extra, tmp):
    db = os.path.join(GOLDEN, case, "db.igd")
    v = int(extra[1]) if extra else 0
    orc = Oracle(db)
    try:
        files = _case_files(case)
        q = files[0]
        want, member, pairs = expected_text(db, orc, q, v)
        if v == 0:
            assert_not_vacuous(member, pairs)
        for args in (["-q", q, "-w"] + extra, ["-w"] + extra + ["-q", q]):
            got = _run(["search", db] + args, HOST)
            assert got.returncode == 0, got.stderr
            assert got.stdout.decode() == want, args
        # a file with a query on a contig the database does not have, lines that are not accepted, and a missing file
        names = orc.ctg_names()
        odd = os.path.join(tmp, "odd.bed")
        write_bed(odd, [(names[0], 100, 90000), ("chrNotThere", 5, 500), (names[-1], 0, 1), ("x", 1, 2), (names[0], 100, 90000)])
        files = files + [odd, os.path.join(tmp, "missing.bed")]
        lst = _write_list(tmp, files, crlf=True)
        got = _run(["search", db, "-Q", lst, "-w"] + extra, HOST)
        assert got.returncode == 0, got.stderr
        want = "".join("Query set %d: %s\n" % (k, p) + expected_text(db, orc, p, v)[0] for k, p in enumerate(files))
        assert got.stdout.decode() == want
        assert "chrNotThere" not in want and want.count("Query regions with a hit:") == len(files)
        assert want.endswith("Query set %d: %s\nQuery regions with a hit: 0 of 0\n" % (len(files) - 1, files[-1]))
    finally:
        orc.close()


@pytest.mark.parametrize("other", [["-q", "Q", "-f"], ["-r", "chr1", "1000", "90000"], ["-r", "chr1", "1000", "90000", "-f"],
                                   ["-r", "chr1", "1000", "90000", "-v", "300"], ["-f"], ["-c"]])
def test_w_has_no_effect_on_the_other_command_lines(other, tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    other = [q if a == "Q" else a for a in other]
    want = _run(["search", db] + other, HOST)
    for args in (["-w"] + other, other + ["-w"]):
        got = _run(["search", db] + args, HOST)
        assert (got.returncode, got.stdout) == (want.returncode, want.stdout), args


def test_command_lines_without_w_keep_their_output(tmp):
    """-q, -q -u, -q -b and -Q -u print what they printed before -w existed: -w is what selects the rows"""
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    lst = _write_list(tmp, _case_files("branch"))
    for args in (["-q", q], ["-q", q, "-u"], ["-q", q, "-b"], ["-Q", lst, "-u"]):
        got = _run(["search", db] + args, HOST)
        assert got.returncode == 0 and b"\t.\n" not in got.stdout and got.stdout.startswith((b"index\t", b"Query set 0"))


@pytest.mark.parametrize("other", [["-u"], ["-b"], ["-u", "-b"]])
def test_w_together_with_u_or_b_is_not_supported(other, tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    lst = _write_list(tmp, _case_files("branch"))
    for sel in (["-q", q], ["-Q", lst]):
        for args in (sel + ["-w"] + other, other + ["-w"] + sel):
            got = _run(["search", db] + args, HOST)
            assert got.returncode == 0 and got.stdout.startswith(b"Not supported") and got.stdout.count(b"\n") == 1, args


def test_engine_route_without_a_device_fails_loudly(tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    nodev = {"IGD_HOST_MAX_QUERIES": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
    lst = _write_list(tmp, _case_files("branch"))
    for args in (["-q", q, "-w"], ["-q", q, "-w", "-v", "500"], ["-Q", lst, "-w"]):
        got = _run(["search", db] + args, nodev)
        assert got.returncode == 69 and b"no CPU search path" in got.stderr, args
        assert got.stdout == b"", args


@pytest.mark.ref
@pytest.mark.parametrize("case", ["branch", "gtype0", "edge"])
def test_w_lists_equal_the_distinct_files_of_the_references_f_listing(case, tmp):
    """v = 0: the distinct file names inside each `Query ...:` block of the reference's `-q F -f` output are the list of
    that query's -w line; blocks and lines are matched in order by contig, start and end"""
    if not have_ref():
        pytest.skip("no reference binary")
    db = os.path.join(tmp, "db.igd")
    shutil.copy(os.path.join(GOLDEN, case, "db.igd"), db)
    shutil.copy(os.path.join(GOLDEN, case, "db_index.tsv"), os.path.join(tmp, "db_index.tsv"))
    names = [name for _, name in _index(db)]
    for k, p in enumerate(_case_files(case)):
        q = os.path.join(tmp, "q%d.bed" % k)
        shutil.copy(p, q)
        blocks = []                                              # [(contig, start, end), {file names}]
        for line in run_ref(["search", db, "-q", q, "-f"]).splitlines():
            if line.startswith("Query "):
                c, a, b = line[len("Query "):].rstrip().rstrip(":").split(", ")
                blocks.append(((c, int(a), int(b)), set()))
            elif line.startswith("Total overlaps"):
                break
            elif blocks and line.count("\t") == 3:
                blocks[-1][1].add(line.split("\t")[3].strip())
        got = _run(["search", db, "-q", q, "-w"], HOST)
        assert got.returncode == 0, got.stderr
        lines = got.stdout.decode().splitlines()
        at = nhit = 0
        for line in lines[:-1]:
            f = line.split("\t")
            mine = set() if f[4] == "." else {names[int(x)] for x in f[4].split(",")}
            assert int(f[3]) == len(mine), line
            nhit += bool(mine)
            # (the reference prints no block for a query that starts beyond the contig's tiles: such a line lists nothing)
            if at < len(blocks) and blocks[at][0] == (f[0], int(f[1]), int(f[2])):
                assert mine == blocks[at][1], (case, k, line)
                at += 1
            else:
                assert not mine, (case, k, line)
        assert at == len(blocks) and at > 0, (case, k)
        assert lines[-1] == "Query regions with a hit: %d of %d" % (nhit, len(lines) - 1)
        assert nhit == sum(1 for b in blocks if b[1])
