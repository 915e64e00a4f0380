"""`igd search db.igd -q regions.bed -J [-v V]` and `-Q list.txt -J` on the host route, byte for byte against a table formatted
from tests/jaccard_ref.py (the definitions over the interval lists this test wrote; the BED files are read by the oracle's reader,
as the other command-line tests read them); every refusal and its exit code; a command line without -J unchanged."""
import os
import random
import shutil

import numpy as np
import pytest

from helpers import Oracle, short_tmpdir, write_bed
from jaccard_ref import jaccard_regions, ref_jaccard, table_text
from nearest_ref import ListDb, clustered_lists
from test_jaccard_host import cli_rule
from test_sets_cli import _write_list
from test_support_host import HOST, _run


@pytest.fixture
def tmp():
    d = short_tmpdir("ijq")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def db_and_beds(tmp, nbp, gtype, nfiles, nctg, span_tiles, seed, nbeds=3):
    rng = random.Random(seed)
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    db = ListDb(tmp, "db", files, nbp, gtype)
    beds = []
    for k in range(nbeds):
        ichr, qs, qe = jaccard_regions(rng, nctg, nbp, span, 150 + 40 * k)
        p = os.path.join(tmp, "q%d.bed" % k)
        write_bed(p, [(db.ctgs[c] if 0 <= c < nctg else "chrNotThere", s, e) for c, s, e in zip(ichr.tolist(), qs.tolist(), qe.tolist())])
        beds.append(p)
    return db, beds


def expected_block(db, orc, qfile, v):
    try:
        ichr, qs, qe = orc.read_queries(qfile)
    except IOError:
        ichr = qs = qe = np.zeros(0, np.int32)
    rule, ev = cli_rule(db.gtype, v)
    inter, set_bp, file_bp, nm, nd = ref_jaccard(db, ichr, qs, qe, np.array([0, len(qs)], np.int64), ev, rule)
    return table_text(db.names, inter[0], set_bp[0], file_bp, nm[0], nd[0]), inter[0]


@pytest.mark.parametrize("nbp,gtype,nfiles,nctg,span_tiles", [(1 << 14, 1, 7, 2, 10), (1 << 12, 0, 5, 3, 30), (1000, 1, 6, 2, 40)])
def test_cli_j_prints_the_definitions_table_on_the_host_route(nbp, gtype, nfiles, nctg, span_tiles, tmp):
    db, beds = db_and_beds(tmp, nbp, gtype, nfiles, nctg, span_tiles, 15100 + nfiles)
    orc = Oracle(db.path)
    try:
        assert orc.ctg_names() == db.ctgs
        for v in (0, 500):
            extra = ["-v", str(v)] if v else []
            want, inter = expected_block(db, orc, beds[0], v)
            assert inter.sum() > 0, "fixture is vacuous"
            for args in (["-q", beds[0], "-J"] + extra, ["-J"] + extra + ["-q", beds[0]]):
                got = _run(["search", db.path] + args, HOST)
                assert got.returncode == 0, got.stderr
                assert got.stdout.decode() == want, args
            # -Q: one block per file; an unreadable file is an empty set
            files = beds + [os.path.join(tmp, "missing.bed")]
            got = _run(["search", db.path, "-Q", _write_list(tmp, files, crlf=True), "-J"] + extra, HOST)
            assert got.returncode == 0, got.stderr
            want = "".join("Query set %d: %s\n" % (k, p) + expected_block(db, orc, p, v)[0] for k, p in enumerate(files))
            assert got.stdout.decode() == want, v
            assert "Any dataset: 0 of 0 bp in 0 merged regions (0 dropped); jaccard 0.000000\n" in want
    finally:
        orc.close()


def test_the_table_by_hand(tmp):
    db = ListDb(tmp, "hand", [[("chrA", 100, 200, 900)], [("chrA", 150, 300, 900)], [("chrB", 5, 6, 900)]], 1 << 12, 1)
    bed = os.path.join(tmp, "q.bed")
    write_bed(bed, [("chrA", 120, 160), ("chrA", 160, 180), ("chrA", 170, 175), ("chrA", 7, 7), ("chrZ", 1, 2), ("chrA", 9, 7)])   # (the reader skips chrZ)
    got = _run(["search", db.path, "-q", bed, "-J"], HOST)
    assert got.returncode == 0, got.stderr
    assert got.stdout.decode() == ("index\tintersection\tunion\tjaccard\tset_fraction\tfile_bp\tFile\n"
                                   "0\t60\t100\t0.600000\t1.000000\t100\tf0000.bed\n"
                                   "1\t30\t180\t0.166667\t0.500000\t150\tf0001.bed\n"
                                   "2\t0\t61\t0.000000\t0.000000\t1\tf0002.bed\n"
                                   "Any dataset: 60 of 60 bp in 1 merged regions (2 dropped); jaccard 0.298507\n")
    empty = os.path.join(tmp, "e.bed")
    write_bed(empty, [("chrZ", 1, 2)])
    lines = _run(["search", db.path, "-q", empty, "-J"], HOST).stdout.decode().splitlines()
    assert lines[1] == "0\t0\t100\t0.000000\tNA\t100\tf0000.bed" and lines[-1] == "Any dataset: 0 of 0 bp in 0 merged regions (0 dropped); jaccard 0.000000"


WITH = ["-u", "-b", "-w", "-U", "-R", "-X", "-C", "-P", "-D", "-N", "-H", "-L", "-E", "-V", "-f", "-m", "-s", "-r", "-O", "-A", "-B"]
VALUE = {"-U": ["q.bed"], "-P": ["10"], "-D": ["100"], "-N": ["100"], "-H": ["0"], "-L": ["10"], "-V": ["count"], "-r": ["chrA", "1", "2"],
         "-O": ["5"], "-A": ["0.5"], "-B": ["0.5"]}


@pytest.mark.parametrize("flag", WITH)
def test_j_with_another_table_is_a_usage_error(flag, tmp):
    db = ListDb(tmp, "ref", [[("chrA", 100, 200, 900)]], 1 << 12, 1)
    bed = os.path.join(tmp, "q.bed")
    write_bed(bed, [("chrA", 120, 160)])
    other = [flag] + [os.path.join(tmp, a) if a == "q.bed" else a for a in VALUE.get(flag, [])]
    msg = b"Not supported: -J together with -u, -b, -w, -U, -R, -X, -C, -P, -D, -N, -H, -L, -E, -V, -f, -m, -s, -r, -O, -A or -B\n"
    for args in (["-q", bed, "-J"] + other, other + ["-J", "-q", bed], ["-Q", _write_list(tmp, [bed]), "-J"] + other):
        got = _run(["search", db.path] + args, HOST)
        assert got.returncode == 64 and got.stdout == msg, args


def test_j_without_a_query_file_is_a_usage_error_and_other_lines_are_unchanged(tmp):
    db = ListDb(tmp, "ref", [[("chrA", 100, 200, 900)], [("chrA", 150, 300, 900)]], 1 << 12, 1)
    bed = os.path.join(tmp, "q.bed")
    write_bed(bed, [("chrA", 120, 160), ("chrA", 10, 20)])
    got = _run(["search", db.path, "-J"], HOST)
    assert got.returncode == 64 and got.stdout == b"Not supported: -J without -q or -Q\n"
    for args in (["-q", bed], ["-q", bed, "-b"], ["-q", bed, "-u", "-v", "500"], ["-Q", _write_list(tmp, [bed]), "-b"]):
        a = _run(["search", db.path] + args, HOST)
        assert a.returncode == 0 and b"jaccard" not in a.stdout and b"intersection" not in a.stdout
