"""Support counts without a GPU: igdc_support_host (igd_hostpath.c) and `igd search -q F -u` / `-Q list -u` on the host route.

    support[f] = the query regions that overlap AT LEAST ONE record of file f        (hits[f] counts every overlapping record)
    nhit       = the query regions that overlap any record

The expected values never come from the code under test.  They come from the CPU oracle, one query at a time
(helpers.Oracle.search on a batch of one, then `> 0`, summed over the set), for v = 0 a second time from the oracle's
enumeration (distinct (query, idx) pairs), and from the reference binary's `-f` listing (marker `ref`).

The fixtures are checked not to be vacuous: support <= hits everywhere, and support < hits for at least one file in every
numpy-written database and in the golden families named in STRICT -- a build that returned pair counts would fail."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, ROOT, Oracle, have_ref, run_ref, short_tmpdir, write_igd_numpy
from test_golden_oracle import CASES, materialize
from test_sets_cli import _case_files, _write_list

EXE = os.path.join(ROOT, "bin", "igd")
HOST = {"IGD_HOST_MAX_QUERIES": "100000000"}
NOV = -2 ** 31                      # IGD_HIP_NO_VALUE_FILTER
NEST, FLAT = 0, 1
# golden families in which some query meets several records of one file (support < hits for at least one file) at v = 0
STRICT = {"edge", "quirk", "branch", "gtype0", "smallrand", "config1"}          # ("parse" has no such query)


# ---- expected values from the oracle -------------------------------------------------------------------------------------
def oracle_support(orc, ichr, qs, qe, v=0):
    """(support int64[nfiles], nhit, hits int64[nfiles]) of one set: Oracle.search on one query at a time."""
    sup = np.zeros(orc.nfiles, np.int64)
    hits = np.zeros(orc.nfiles, np.int64)
    nhit = 0
    for i in range(len(qs)):
        h, _ = orc.search(ichr[i:i + 1], qs[i:i + 1], qe[i:i + 1], v)
        sup += h > 0
        hits += h
        nhit += int((h > 0).any())
    return sup, nhit, hits


def oracle_support_enum(orc, ichr, qs, qe):
    """the same for v = 0 from the oracle's enumeration: distinct (query, idx) pairs"""
    qoff, rec = orc.enumerate(ichr, qs, qe)
    qno = np.repeat(np.arange(len(qs), dtype=np.int64), np.diff(qoff))
    idx = rec[:, 0].astype(np.int64)
    ok = (idx >= 0) & (idx < orc.nfiles)
    pairs = np.unique(qno[ok] * orc.nfiles + idx[ok])
    sup = np.bincount(pairs % orc.nfiles, minlength=orc.nfiles).astype(np.int64)
    return sup, len(np.unique(pairs // orc.nfiles))


# ---- igdc_support_host through ctypes ------------------------------------------------------------------------------------
class HostDb:
    def __init__(self, path):
        from igd_amd import _native as N
        self.N, self.L = N, N.cli()
        self.core = self.L.igdc_open(path.encode())
        assert self.core
        tsv = self.L.igdc_index_path(path.encode())
        assert self.L.igdc_load_index(self.core, C.cast(tsv, C.c_char_p)) == 0
        N.free(tsv)
        fd = os.open(path, os.O_RDONLY)
        self.m = self.L.igdc_map_open(self.core, fd)
        os.close(fd)
        assert self.m
        self.nfiles = self.core.contents.nFiles

    def support(self, ichr, qs, qe, v, rule, support=None, nhit0=0):
        ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
        sup = np.zeros(self.nfiles, np.int64) if support is None else support
        nhit = C.c_int64(nhit0)
        rc = self.L.igdc_support_host(self.core, self.m, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, len(qs), v, rule,
                                      sup.ctypes.data, C.byref(nhit))
        assert rc == 0
        return sup, nhit.value

    def close(self):
        self.L.igdc_map_close(self.m)
        self.L.igdc_close(self.core)


def cli_rule(gtype, v):
    """the dispatch of `igd search -q ... -v V`"""
    return (FLAT, v) if (gtype != 0 and v > 0) else (NEST, NOV)


@pytest.fixture
def tmp():
    d = short_tmpdir("isu")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", t)
    os.environ.pop("IGD_HOST_THREADS", None)


@pytest.mark.parametrize("case", CASES)
def test_host_support_equals_the_oracle_on_the_golden_families(case, host_threads):
    d, dst, man = materialize(case)
    try:
        path = os.path.join(dst, "db.igd")
        orc = Oracle(path)
        ichr, qs, qe = orc.read_queries(os.path.join(dst, "q.bed"))
        if len(qs) > 3000:                                   # (config1: 10 000 queries; one oracle call per query)
            ichr, qs, qe = ichr[:3000], qs[:3000], qe[:3000]
        H = HostDb(path)
        assert H.nfiles == orc.nfiles
        for v in (0, 500):
            want, wnhit, hits = oracle_support(orc, ichr, qs, qe, v)
            print(case, "v", v, "support", int(want.sum()), "hits", int(hits.sum()), "nhit", wnhit, "of", len(qs))
            assert (want <= hits).all() and (want <= len(qs)).all()
            if v == 0:
                e_sup, e_nhit = oracle_support_enum(orc, ichr, qs, qe)
                assert np.array_equal(e_sup, want) and e_nhit == wnhit
                if case in STRICT:
                    assert (want < hits).any(), "fixture is vacuous: support equals the pair counts"
            rule, ev = cli_rule(orc.gtype, v)
            for threads in ("1", "3"):
                host_threads(threads)
                got, nhit = H.support(ichr, qs, qe, ev, rule)
                assert np.array_equal(got, want), (case, v, threads)
                assert nhit == wnhit
        H.close()
        orc.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def clustered_db(rng, d, name, nbp, gtype, nfiles, nctg, span_tiles, min_value=0):
    """Per file and contig: clusters of neighbouring records (several records of ONE file under one query), long records
    that span four and six tiles, two long ones that overlap each other, plus scattered short ones."""
    ctgs = ["chr%d" % (i + 1) for i in range(nctg)]
    span = nbp * span_tiles
    files = []
    for f in range(nfiles):
        rows = []
        for c in ctgs:
            for _ in range(3):
                s = rng.randrange(0, span - 2000)
                for k in range(rng.randint(2, 5)):               # a cluster: 2-5 records within a few hundred bp
                    rows.append((c, s + 90 * k, s + 90 * k + rng.randint(20, 400), rng.randint(min_value, 1000)))
            for L in (3 * nbp + 7, 5 * nbp + 1):                  # long: 4 and 6 tiles
                s = rng.randrange(0, span)
                rows.append((c, s, s + L, rng.randint(min_value, 1000)))
            s = rng.randrange(nbp, span)                          # two long ones that overlap each other
            rows.append((c, s, s + 3 * nbp, rng.randint(min_value, 1000)))
            rows.append((c, s + nbp // 2, s + 4 * nbp, rng.randint(min_value, 1000)))
            for _ in range(6):
                s = rng.randrange(0, span)
                rows.append((c, s, s + rng.choice([1, 5, nbp // 3]), rng.randint(min_value, 1000)))
        files.append(rows)
    path = os.path.join(d, name + ".igd")
    write_igd_numpy(path, files, nbp=nbp, gtype=gtype)
    return path, span


def mixed_queries(rng, nctg, nbp, span, n):
    """unknown contigs, inverted, zero-length, short and many-tile queries, every fifth one repeated"""
    ichr = np.array([rng.choice(list(range(nctg)) + [-1, 99]) for _ in range(n)], np.int32)
    qs = np.array([rng.randrange(0, span + 3 * nbp) for _ in range(n)], np.int32)
    ln = np.array([rng.choice([0, 1, 200, 700, nbp, 2 * nbp + 5, 7 * nbp + 3, rng.randint(1, 3 * nbp), -rng.randint(1, 50)])
                   for _ in range(n)], np.int32)
    qe = qs + ln
    for i in range(5, n, 5):                                     # two identical query lines are two regions
        ichr[i], qs[i], qe[i] = ichr[i - 1], qs[i - 1], qe[i - 1]
    return ichr, qs, qe


NUMPY_DBS = [
    # nbp, gtype, nfiles, nctg, span_tiles
    (1 << 14, 1, 7, 2, 10),
    (1 << 12, 0, 5, 3, 30),          # gType 0
    (1 << 11, 1, 40, 1, 25),         # more than 32 files: several bitmap words
    (1000, 1, 6, 2, 40),             # tile width that is no power of two
]


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_host_support_equals_the_oracle_on_clustered_databases(case, tmp, host_threads):
    rng = random.Random(4100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    path, span = clustered_db(rng, tmp, "c%d" % case, nbp, gtype, nfiles, nctg, span_tiles)
    ichr, qs, qe = mixed_queries(rng, nctg, nbp, span, 1500)
    orc = Oracle(path)
    H = HostDb(path)
    try:
        for v in (0, 500):
            want, wnhit, hits = oracle_support(orc, ichr, qs, qe, v)
            assert (want <= hits).all() and (want < hits).any() and 0 < wnhit < len(qs)
            if v == 0:
                e_sup, e_nhit = oracle_support_enum(orc, ichr, qs, qe)
                assert np.array_equal(e_sup, want) and e_nhit == wnhit
            rule, ev = cli_rule(gtype, v)
            for threads in ("1", "2", "7"):
                host_threads(threads)
                got, nhit = H.support(ichr, qs, qe, ev, rule)
                assert np.array_equal(got, want) and nhit == wnhit, (case, v, threads)
        # ADDED to the caller's vector and counter
        base = np.arange(nfiles, dtype=np.int64) * 100
        rule, ev = cli_rule(gtype, 0)
        want, wnhit, _ = oracle_support(orc, ichr, qs, qe, 0)
        got, nhit = H.support(ichr, qs, qe, ev, rule, support=base.copy(), nhit0=11)
        assert np.array_equal(got, base + want) and nhit == 11 + wnhit
        got, nhit = H.support(ichr[:0], qs[:0], qe[:0], ev, rule)
        assert not got.any() and nhit == 0
    finally:
        H.close()
        orc.close()


def sparse_db(rng, d, name="sp"):
    """few records, many empty tiles, values >= 1: rule NEST ends a query at an empty first tile, rule FLAT visits every
    tile -- so the oracle's v = 1 (rule FLAT, a filter that every record passes) is rule FLAT without a filter"""
    nbp = 1 << 11
    return clustered_db(rng, d, name, nbp, 1, 4, 2, 120, min_value=1) + (nbp,)


def test_explicit_rules_on_a_sparse_database(tmp, host_threads):
    rng = random.Random(4200)
    path, span, nbp = sparse_db(rng, tmp)
    ichr, qs, qe = mixed_queries(rng, 2, nbp, span, 2000)
    orc = Oracle(path)
    H = HostDb(path)
    try:
        nest, nest_nhit, nest_hits = oracle_support(orc, ichr, qs, qe, 0)
        flat, flat_nhit, flat_hits = oracle_support(orc, ichr, qs, qe, 1)
        flat5, flat5_nhit, _ = oracle_support(orc, ichr, qs, qe, 500)
        assert not np.array_equal(nest, flat) and nest_nhit < flat_nhit, "the two rules do not differ on this fixture"
        assert (nest < nest_hits).any() and (flat < flat_hits).any()
        for threads in ("1", "4"):
            host_threads(threads)
            got, nhit = H.support(ichr, qs, qe, NOV, NEST)
            assert np.array_equal(got, nest) and nhit == nest_nhit
            got, nhit = H.support(ichr, qs, qe, NOV, FLAT)
            assert np.array_equal(got, flat) and nhit == flat_nhit
            got, nhit = H.support(ichr, qs, qe, 1, FLAT)
            assert np.array_equal(got, flat) and nhit == flat_nhit
            got, nhit = H.support(ichr, qs, qe, 500, FLAT)
            assert np.array_equal(got, flat5) and nhit == flat5_nhit
    finally:
        H.close()
        orc.close()


# ---- command line ---------------------------------------------------------------------------------------------------------
def _run(args, env=None, cwd=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, cwd=cwd, timeout=600)


def _index(db):
    """(number of regions, name) per file, from the database's index file"""
    rows = open(os.path.splitext(db)[0] + "_index.tsv").read().splitlines()[1:]
    return [(int(r.split("\t")[2]), r.split("\t")[1]) for r in rows if r.strip()]


def expected_table(db, orc, qfile, v):
    """the text of `igd search db -q qfile -u [-v v]`, from the oracle"""
    try:
        ichr, qs, qe = orc.read_queries(qfile)
    except IOError:
        ichr = qs = qe = np.zeros(0, np.int32)
    sup, nhit, _ = oracle_support(orc, ichr, qs, qe, v)
    out = "index\t number of regions\t number of query regions\t File_name\n"
    for i, (nr, name) in enumerate(_index(db)):
        if sup[i] > 0:
            out += "%d\t%d\t%d\t%s\n" % (i, nr, sup[i], name)
    return out + "Query regions with a hit: %d of %d\n" % (nhit, len(qs))


CLI_CASES = [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("gtype0", ["-v", "500"]), ("edge", []), ("edge", ["-v", "500"])]


@pytest.mark.parametrize("case,extra", CLI_CASES)
def test_cli_u_prints_the_oracles_support_on_the_host_route(case, extra, tmp):
    db = os.path.join(GOLDEN, case, "db.igd")
    v = int(extra[1]) if extra else 0
    orc = Oracle(db)
    try:
        files = _case_files(case)
        q = files[0]
        for args in (["-q", q, "-u"] + extra, ["-u"] + extra + ["-q", q]):
            got = _run(["search", db] + args, HOST)
            assert got.returncode == 0, got.stderr
            assert got.stdout.decode() == expected_table(db, orc, q, v), args
        files = files + [os.path.join(tmp, "missing.bed")]
        lst = _write_list(tmp, files, crlf=True)
        got = _run(["search", db, "-Q", lst, "-u"] + extra, HOST)
        assert got.returncode == 0, got.stderr
        want = "".join("Query set %d: %s\n" % (k, p) + expected_table(db, orc, p, v) for k, p in enumerate(files))
        assert got.stdout.decode() == want
        assert "Total:" not in want and want.count("Query regions with a hit:") == len(files)
    finally:
        orc.close()


@pytest.mark.parametrize("other", [["-q", "Q", "-f"], ["-r", "chr1", "1000", "90000"], ["-r", "chr1", "1000", "90000", "-f"],
                                   ["-r", "chr1", "1000", "90000", "-v", "300"], ["-f"], ["-c"]])
def test_u_has_no_effect_on_the_other_command_lines(other, tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    other = [q if a == "Q" else a for a in other]
    want = _run(["search", db] + other, HOST)
    for args in (["-u"] + other, other + ["-u"]):
        got = _run(["search", db] + args, HOST)
        assert (got.returncode, got.stdout) == (want.returncode, want.stdout), args


@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("edge", [])])
def test_command_lines_without_u_still_print_the_pair_counts(case, extra, tmp):
    """`-q F` and `-Q list` without -u: the table of hits, from the oracle's batch counts (what they printed before -u)"""
    db = os.path.join(GOLDEN, case, "db.igd")
    v = int(extra[1]) if extra else 0
    orc = Oracle(db)
    try:
        files = _case_files(case)

        def table(p):
            hits, _ = orc.search(*orc.read_queries(p), v)
            out = "index\t number of regions\t number of hits\t File_name\n"
            for i, (nr, name) in enumerate(_index(db)):
                if hits[i] > 0:
                    out += "%d\t%d\t%d\t%s\n" % (i, nr, hits[i], name)
            return out + "Total: %d\n" % hits.sum()
        got = _run(["search", db, "-q", files[0]] + extra, HOST)
        assert got.returncode == 0 and got.stdout.decode() == table(files[0])
        lst = _write_list(tmp, files)
        got = _run(["search", db, "-Q", lst] + extra, HOST)
        assert got.returncode == 0
        assert got.stdout.decode() == "".join("Query set %d: %s\n" % (k, p) + table(p) for k, p in enumerate(files))
    finally:
        orc.close()


def test_engine_route_without_a_device_fails_loudly(tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    nodev = {"IGD_HOST_MAX_QUERIES": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
    lst = _write_list(tmp, _case_files("branch"))
    for args in (["-q", q, "-u"], ["-q", q, "-u", "-v", "500"], ["-Q", lst, "-u"]):
        got = _run(["search", db] + args, nodev)
        assert got.returncode == 69 and b"no CPU search path" in got.stderr, args
        assert b"index\t" not in got.stdout and b"Query regions" not in got.stdout and b"Query set" not in got.stdout


@pytest.mark.ref
@pytest.mark.parametrize("case", ["branch", "gtype0", "edge"])
def test_u_column_equals_the_distinct_files_of_the_references_f_listing(case, tmp):
    """v = 0: inside each `Query ...:` block of the reference's `-q F -f` output a file counts once; summed per file over
    the blocks that is the -u column."""
    if not have_ref():
        pytest.skip("no reference binary")
    db = os.path.join(tmp, "db.igd")
    shutil.copy(os.path.join(GOLDEN, case, "db.igd"), db)
    shutil.copy(os.path.join(GOLDEN, case, "db_index.tsv"), os.path.join(tmp, "db_index.tsv"))
    for k, p in enumerate(_case_files(case)):
        q = os.path.join(tmp, "q%d.bed" % k)
        shutil.copy(p, q)
        want, blocks_with_hit, seen = {}, 0, None
        for line in run_ref(["search", db, "-q", q, "-f"]).splitlines():
            if line.startswith("Query "):
                seen = set()
            elif line.startswith("Total overlaps"):
                break
            elif seen is not None and line.count("\t") == 3:
                name = line.split("\t")[3].strip()
                if not seen:
                    blocks_with_hit += 1
                if name not in seen:
                    seen.add(name)
                    want[name] = want.get(name, 0) + 1
        got = _run(["search", db, "-q", q, "-u"], HOST)
        assert got.returncode == 0, got.stderr
        lines = got.stdout.decode().splitlines()
        col = {l.split("\t")[3]: int(l.split("\t")[2]) for l in lines[1:-1]}
        assert col == want, (case, k)
        assert lines[-1].startswith("Query regions with a hit: %d of " % blocks_with_hit)
