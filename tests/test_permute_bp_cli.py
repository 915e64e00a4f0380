"""`igd search db.igd -q regions.bed -P N -g genome.sizes -G [-S seed] [-M circular|shuffle] [-v V]` on the host route, byte for
byte against a table this test formats from the reference matrices (tests/permute_bp_ref.py: permute_ref's generator,
jaccard_ref's sort, sweep and boolean arrays over the interval lists written here, the summary in Python integers, Fractions
and floats); every refusal is exit code 64 with -G's own message; plain -J and plain -P command lines print what they
printed."""
import os
import random
import shutil

import numpy as np
import pytest

import permute_bp_ref as PB
import permute_ref as PR
from helpers import short_tmpdir, write_bed
from jaccard_ref import ref_jaccard
from jaccard_ref import table_text as jaccard_table
from nearest_ref import ListDb, clustered_lists
from test_jaccard_host import cli_rule
from test_support_host import HOST, _run

NBP, NCTG, NFILES = 1 << 12, 2, 7
HEADER = "index\tobserved_bp\tmean\tsd\tz\tfold\tn_ge\tn_le\tnlog10_p_upper\tnlog10_p_lower\tjaccard\tjaccard_mean\tFile"
TOGETHER = ("Not supported: -G together with -D, -J, -O, -A, -B, -N, -H, -L, -E, -V, -Q, -u, -b, -w, -U, -R, -X, -C, -f, -m, -s or -r\n")


@pytest.fixture(scope="module")
def fx():
    d = short_tmpdir("ipg")
    rng = random.Random(73)
    files, span = clustered_lists(rng, NBP, NFILES, NCTG, 12)
    ldb = ListDb(d, "db", files, NBP, 1)
    assert ldb.ctgs == ["chr1", "chr2"]
    ctg_len = np.array([span + 9 * NBP, span + 7 * NBP + 777], np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 300, unknown=())
    keep = qe > 0                                             # (the command line accepts lines with end > 0)
    ichr, qs, qe = ichr[keep], qs[keep], qe[keep]
    rows = [(ldb.ctgs[c], int(s), int(e)) for c, s, e in zip(ichr, qs, qe)]
    rows[3:3] = [("chrNotThere", 5, 500), ("x", 1, 2)]
    q = os.path.join(d, "q.bed")
    write_bed(q, rows)
    g = os.path.join(d, "genome.sizes")
    with open(g, "w") as f:
        f.write("chr2\t%d\nchrOther\t5000000000\nchr1\t%d\r\n\n" % (ctg_len[1], ctg_len[0]))
    yield dict(d=d, ldb=ldb, db=ldb.path, q=q, g=g, ctg_len=ctg_len, regions=(ichr, qs, qe))
    shutil.rmtree(d, ignore_errors=True)


def expected_text(fx, nperm, seed, mode, v, regions=None):
    ichr, qs, qe = fx["regions"] if regions is None else regions
    rule, ev = cli_rule(fx["ldb"].gtype, v)
    return PB.table_text(fx["ldb"].names, *PB.null(fx["ldb"], ichr, qs, qe, fx["ctg_len"], nperm, seed, mode, ev, rule))


@pytest.mark.parametrize("extra,nperm,seed,mode,v", [([], 7, 0, PR.CIRCULAR, 0), (["-S", "5", "-M", "shuffle"], 20, 5, PR.SHUFFLE, 0),
                                                    (["-M", "circular", "-v", "500"], 3, 0, PR.CIRCULAR, 500),
                                                    (["-S", "18446744073709551615"], 1, 2 ** 64 - 1, PR.CIRCULAR, 0),
                                                    (["-v", "999"], 2, 0, PR.CIRCULAR, 999)])
def test_cli_G_prints_the_reference_table_on_the_host_route(fx, extra, nperm, seed, mode, v):
    want = expected_text(fx, nperm, seed, mode, v)
    for args in (["-q", fx["q"], "-P", str(nperm), "-g", fx["g"], "-G"] + extra, extra + ["-G", "-g", fx["g"], "-P", str(nperm), "-q", fx["q"]]):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 0, got.stderr
        assert got.stdout.decode() == want, args
    lines = want.splitlines()
    assert lines[0] == HEADER and len(lines) == NFILES + 2 and len(lines[1].split("\t")) == 13
    assert lines[-1].startswith("Any dataset: ") and len(lines[-1].split("\t")) == 11
    if nperm == 1:
        assert "\tNA\t" in lines[1]
    # the head of the last line, the observed column and the Jaccards are -J's
    j = _run(["search", fx["db"], "-q", fx["q"], "-J"] + (["-v", str(v)] if v else []), HOST).stdout.decode().splitlines()
    assert j[-1].startswith(lines[-1].split("\t")[0] + "; jaccard ")
    assert [(l.split("\t")[0], l.split("\t")[1], l.split("\t")[10]) for l in lines[1:-1]] == \
           [(l.split("\t")[0], l.split("\t")[1], l.split("\t")[3]) for l in j[1:-1]]


def test_an_empty_or_missing_query_file_gives_zeros_and_NA(fx):
    e = np.zeros(0, np.int32)
    want = expected_text(fx, 3, 0, PR.CIRCULAR, 0, regions=(e, e, e))
    empty = os.path.join(fx["d"], "empty.bed")
    open(empty, "w").close()
    for q in (empty, os.path.join(fx["d"], "missing.bed")):
        got = _run(["search", fx["db"], "-q", q, "-P", "3", "-g", fx["g"], "-G"], HOST)
        assert got.returncode == 0 and got.stdout.decode() == want, q
    assert want.endswith("Any dataset: 0 of 0 bp in 0 merged regions (0 dropped)\t0.000000\t0.000000\tNA\tNA\t3\t3\t0.000000\t0.000000\t0.000000\t0.000000\n")


@pytest.mark.parametrize("other", [["-D", "100"], ["-J"], ["-N", "5"], ["-N", "5", "-H", "0"], ["-N", "5", "-L", "10"], ["-N", "5", "-L", "10", "-E"],
                                   ["-V", "count"], ["-O", "5"], ["-A", "0.5"], ["-B", "0.5"], ["-Q", "Q"], ["-u"], ["-b"], ["-w"], ["-U", "Q"],
                                   ["-U", "Q", "-R"], ["-U", "Q", "-X"], ["-R"], ["-X"], ["-C"], ["-f"], ["-m"], ["-s"],
                                   ["-r", "chr1", "1000", "90000"]])
def test_G_together_with_another_selector_is_refused(fx, other):
    other = [fx["q"] if a == "Q" else a for a in other]
    for args in (["-q", fx["q"], "-P", "5", "-g", fx["g"], "-G"] + other, other + ["-G", "-P", "5", "-g", fx["g"], "-q", fx["q"]]):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 64 and got.stdout.decode() == TOGETHER, (args, got.stdout)


def test_G_without_P_g_or_q_and_bad_numbers_are_refused(fx):
    def run(args):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 64 and b"index" not in got.stdout, (args, got.stdout)
        return got.stdout.decode()
    assert run(["-q", fx["q"], "-G"]) == "Not supported: -G without -P\n"
    assert run(["-q", fx["q"], "-g", fx["g"], "-G"]) == "Not supported: -G without -P\n"
    assert run(["-q", fx["q"], "-J", "-G"]) == "Not supported: -G without -P\n"
    assert run(["-q", fx["q"], "-P", "5", "-G"]) == "Not supported: -G -P without -g\n"
    assert run(["-P", "5", "-g", fx["g"], "-G"]) == "Not supported: -G -P without -q\n"
    for n in ("0", "-4", "1048577", "ten", "5x"):
        assert run(["-q", fx["q"], "-g", fx["g"], "-P", n, "-G"]) == "Not supported: -G with a number of permutations outside 1 to 1048576\n"
    assert run(["-q", fx["q"], "-g", fx["g"], "-P", "5", "-M", "rotate", "-G"]) == "Not supported: -G with a -M that is neither circular nor shuffle\n"


def test_a_region_outside_its_contig_ends_the_run_as_under_P(fx):
    bad = os.path.join(fx["d"], "bad.bed")
    write_bed(bad, [("chr1", 5, 50), ("chr1", 10, int(fx["ctg_len"][0]) + 1)])
    a = _run(["search", fx["db"], "-q", bad, "-P", "3", "-g", fx["g"], "-G"], HOST)
    b = _run(["search", fx["db"], "-q", bad, "-P", "3", "-g", fx["g"]], HOST)
    assert a.returncode == b.returncode == 0 and a.stdout == b.stdout and b"line 2: region chr1:10-" in a.stdout


def test_plain_J_and_plain_P_print_what_they_printed(fx):
    """without -G the -J table is jaccard_ref's and the -P table is the support table, on the same inputs"""
    ichr, qs, qe = fx["regions"]
    for v in (0, 500):
        rule, ev = cli_rule(fx["ldb"].gtype, v)
        inter, set_bp, file_bp, nm, nd = ref_jaccard(fx["ldb"], ichr, qs, qe, np.array([0, len(qs)], np.int64), ev, rule)
        j = _run(["search", fx["db"], "-q", fx["q"], "-J"] + (["-v", str(v)] if v else []), HOST)
        assert j.returncode == 0 and j.stdout.decode() == jaccard_table(fx["ldb"].names, inter[0], set_bp[0], file_bp, nm[0], nd[0])
    p = _run(["search", fx["db"], "-q", fx["q"], "-P", "4", "-g", fx["g"]], HOST)
    assert p.returncode == 0
    lines = p.stdout.decode().splitlines()
    assert lines[0] == "index\tobserved\tmean\tsd\tz\tn_ge\tn_le\tnlog10_p_upper\tnlog10_p_lower\tFile" and len(lines) == NFILES + 2
    assert lines[-1].startswith("Query regions with a hit: ")
    d = _run(["search", fx["db"], "-q", fx["q"], "-P", "4", "-g", fx["g"], "-D", "100"], HOST)
    assert d.returncode == 0 and d.stdout.decode().startswith("index\tn_within\tmean_dist\t")
    # the refusals of -J and of -P keep their text and their exit codes
    r = _run(["search", fx["db"], "-q", fx["q"], "-J", "-P", "4", "-g", fx["g"]], HOST)
    assert r.returncode == 64 and r.stdout.decode().startswith("Not supported: -J together with -u, -b, -w, -U, -R, -X, -C, -P, -D,")
    r = _run(["search", fx["db"], "-q", fx["q"], "-P", "4"], HOST)
    assert r.returncode == 0 and r.stdout == b"Not supported: -P without -g\n"
    r = _run(["search", fx["db"], "-q", fx["q"], "-g", fx["g"]], HOST)
    assert r.returncode == 0 and r.stdout == b"Not supported: -g, -S or -M without -P\n"
