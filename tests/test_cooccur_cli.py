"""`igd search db.igd -q regions.bed -C [-v N]` on the host route: the header, one line per pair of datasets a < b that some
region overlaps both of, in ascending (a, b), the Jaccard index as %.6f, then `-u`'s last line.

Expected values never come from the code under test: the membership from the CPU oracle one region at a time
(test_membership_host.oracle_member), the matrix and the Jaccard index from cooccur_ref.  -C together with any other
selector is refused; without -C every command line prints what it printed (tests/golden)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import cooccur_ref as CR
from helpers import GOLDEN, Oracle, short_tmpdir, write_bed
from test_membership_host import oracle_member
from test_sets_cli import EXE, _case_files, _write_list
from test_support_host import HOST, _index, _run

HEADER = "index_a\tindex_b\tsupport_a\tsupport_b\tboth\tjaccard\tFile_a\tFile_b\n"
REFUSED = "Not supported: -C together with -Q, -u, -b, -w, -U, -R, -X, -f, -m, -s or -r\n"


@pytest.fixture
def tmp():
    d = short_tmpdir("icc")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def expected_text(db, orc, qfile, v):
    """(the text of `igd search db -q qfile -C [-v v]`, the matrix) from the oracle"""
    try:
        ichr, qs, qe = orc.read_queries(qfile)
    except IOError:
        ichr = qs = qe = np.zeros(0, np.int32)
    member, _ = oracle_member(orc, ichr, qs, qe, v)
    c = CR.cooc(member)
    j = CR.jaccard(c)
    names = [name for _, name in _index(db)]
    out = [HEADER]
    for a in range(orc.nfiles):
        for b in range(a + 1, orc.nfiles):
            if c[a, b] > 0:
                out.append("%d\t%d\t%d\t%d\t%d\t%.6f\t%s\t%s\n" % (a, b, c[a, a], c[b, b], c[a, b], j[a, b], names[a], names[b]))
    out.append("Query regions with a hit: %d of %d\n" % (member.any(axis=1).sum(), len(qs)))
    return "".join(out), c


@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("gtype0", []), ("gtype0", ["-v", "500"]),
                                        ("edge", []), ("edge", ["-v", "500"])])
def test_cli_C_prints_the_oracles_pairs_on_the_host_route(case, extra, tmp):
    db = os.path.join(GOLDEN, case, "db.igd")
    v = int(extra[1]) if extra else 0
    orc = Oracle(db)
    try:
        pairs = 0
        for q in _case_files(case)[:3]:
            want, c = expected_text(db, orc, q, v)
            pairs += int(np.triu(c, 1).astype(bool).sum())
            for args in (["-q", q, "-C"] + extra, ["-C"] + extra + ["-q", q]):
                got = _run(["search", db] + args, HOST)
                assert got.returncode == 0, got.stderr
                assert got.stdout.decode() == want, args
        assert pairs > 0 or v > 0, "no pair at all: the fixture is vacuous"
        # lines on a contig the database does not have and lines that are not accepted; an empty and a missing file
        names = orc.ctg_names()
        odd = os.path.join(tmp, "odd.bed")
        write_bed(odd, [(names[0], 100, 90000), ("chrNotThere", 5, 500), (names[-1], 0, 1), ("x", 1, 2), (names[0], 100, 90000)])
        empty = os.path.join(tmp, "empty.bed")
        open(empty, "w").close()
        for q in (odd, empty, os.path.join(tmp, "missing.bed")):
            want, _ = expected_text(db, orc, q, v)
            got = _run(["search", db, "-q", q, "-C"] + extra, HOST)
            assert got.returncode == 0 and got.stdout.decode() == want, q
        assert want == HEADER + "Query regions with a hit: 0 of 0\n"
    finally:
        orc.close()


def test_pairs_are_in_ascending_order_and_jaccard_has_six_decimals():
    db, q = os.path.join(GOLDEN, "branch", "db.igd"), os.path.join(GOLDEN, "branch", "q.bed")
    lines = _run(["search", db, "-q", q, "-C"], HOST).stdout.decode().splitlines()
    assert lines[0] + "\n" == HEADER and lines[-1].startswith("Query regions with a hit: ") and len(lines) > 3
    keys = []
    for line in lines[1:-1]:
        f = line.split("\t")
        assert len(f) == 8 and int(f[0]) < int(f[1]) and int(f[4]) > 0
        assert len(f[5].split(".")[1]) == 6 and f[5] == "%.6f" % (int(f[4]) / (int(f[2]) + int(f[3]) - int(f[4])))
        assert int(f[4]) <= min(int(f[2]), int(f[3]))
        keys.append((int(f[0]), int(f[1])))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    # the last line is -u's
    assert lines[-1] == _run(["search", db, "-q", q, "-u"], HOST).stdout.decode().splitlines()[-1]


@pytest.mark.parametrize("other", [["-u"], ["-b"], ["-w"], ["-U", "Q"], ["-U", "Q", "-R"], ["-U", "Q", "-X"], ["-R"], ["-X"], ["-f"],
                                   ["-m"], ["-s"], ["-r", "chr1", "1000", "90000"]])
def test_C_together_with_another_selector_is_refused(other, tmp):
    db, q = os.path.join(GOLDEN, "branch", "db.igd"), os.path.join(GOLDEN, "branch", "q.bed")
    other = [q if a == "Q" else a for a in other]
    for args in (["-q", q, "-C"] + other, other + ["-C", "-q", q]):
        got = _run(["search", db] + args, HOST)
        assert got.returncode == 0 and got.stdout.decode() == REFUSED, args


def test_C_with_a_list_or_without_a_query_file_is_refused(tmp):
    db, q = os.path.join(GOLDEN, "branch", "db.igd"), os.path.join(GOLDEN, "branch", "q.bed")
    lst = _write_list(tmp, _case_files("branch"))
    for args in (["-Q", lst, "-C"], ["-C", "-Q", lst, "-q", q], ["-Q", lst, "-C", "-u"]):
        assert _run(["search", db] + args, HOST).stdout.decode() == REFUSED, args
    got = _run(["search", db, "-C"], HOST)
    assert got.returncode == 0 and got.stdout.decode() == "Not supported: -C without -q\n"
    usage = subprocess.run([EXE, "search"], stderr=subprocess.PIPE, stdout=subprocess.PIPE).stderr.decode()
    assert "    -C   " in usage and "    -w   " in usage


def _golden_runs():
    out = []
    for fam in ("branch", "edge", "gtype0"):
        man = json.load(open(os.path.join(GOLDEN, fam, "manifest.json")))
        for k, run in enumerate(man["runs"]):
            if "-q" in run["args"] and "-m" not in run["args"] and "-s" not in run["args"]:
                out.append((fam, k))
    return out


@pytest.mark.parametrize("fam,k", _golden_runs())
def test_command_lines_without_C_keep_their_output(fam, k):
    """the golden `-q` runs (with -v, with -f) are byte-identical to the recorded reference output"""
    man = json.load(open(os.path.join(GOLDEN, fam, "manifest.json")))
    run = man["runs"][k]
    args = [os.path.join(GOLDEN, fam, a) if a in ("db.igd", "q.bed") else a for a in run["args"]]
    got = _run(args, HOST)
    assert got.returncode == 0, got.stderr.decode()[-300:]
    assert got.stdout.decode() == open(os.path.join(GOLDEN, fam, run["stdout"])).read(), run["args"]


def test_engine_route_without_a_device_fails_loudly():
    db, q = os.path.join(GOLDEN, "branch", "db.igd"), os.path.join(GOLDEN, "branch", "q.bed")
    nodev = {"IGD_HOST_MAX_QUERIES": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
    got = _run(["search", db, "-q", q, "-C"], nodev)
    assert got.returncode == 69 and b"no CPU search path" in got.stderr and got.stdout == b""
