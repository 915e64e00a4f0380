"""`igd search db.igd -q regions.bed -P N -g genome.sizes -D W [-S seed] [-M circular|shuffle] [-v V]` on the host route, byte
for byte against a table this test formats from the reference matrices (tests/permute_nearest_ref.py: permute_ref's generator,
nearest_ref's definition over the interval lists written here, numpy's summary); every refusal is exit code 64; plain -P and
plain -N command lines print what they printed."""
import os
import random
import shutil

import numpy as np
import pytest

import permute_nearest_ref as PN
import permute_ref as PR
from helpers import short_tmpdir, write_bed
from nearest_ref import MAX_WINDOW, ListDb, clustered_lists, ref_rows, ref_sets
from nearest_ref import table_text as nearest_table
from test_support_host import HOST, _run

NBP, NCTG, NFILES = 1 << 12, 2, 7


@pytest.fixture(scope="module")
def fx():
    d = short_tmpdir("ipd")
    rng = random.Random(71)
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


def expected_text(fx, nperm, W, seed, mode, v, regions=None):
    ichr, qs, qe = fx["regions"] if regions is None else regions
    nw, no, sd = PN.null(fx["ldb"], ichr, qs, qe, fx["ctg_len"], nperm, W, seed, mode, v if v > 0 else None)
    return PN.table_text(fx["ldb"].names, nw, no, sd, W, len(qs))


@pytest.mark.parametrize("extra,nperm,W,seed,mode,v", [([], 7, NBP, 0, PR.CIRCULAR, 0), (["-S", "5", "-M", "shuffle"], 20, 700, 5, PR.SHUFFLE, 0),
                                                      (["-M", "circular", "-v", "500"], 3, 0, 0, PR.CIRCULAR, 500),
                                                      (["-S", "18446744073709551615"], 1, MAX_WINDOW, 2 ** 64 - 1, PR.CIRCULAR, 0),
                                                      (["-v", "999"], 2, 3, 0, PR.CIRCULAR, 999)])
def test_cli_D_prints_the_reference_table_on_the_host_route(fx, extra, nperm, W, seed, mode, v):
    want = expected_text(fx, nperm, W, seed, mode, v)
    for args in (["-q", fx["q"], "-P", str(nperm), "-g", fx["g"], "-D", str(W)] + extra,
                 extra + ["-D", str(W), "-g", fx["g"], "-P", str(nperm), "-q", fx["q"]]):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 0, got.stderr
        assert got.stdout.decode() == want, args
    lines = want.splitlines()
    assert lines[0] == PN.HEADER.rstrip("\n") and len(lines) == NFILES + 2 and len(lines[1].split("\t")) == 14
    assert lines[-1].startswith("Regions with a dataset within %d bp: " % W) and len(lines[-1].split("\t")) == 11
    if nperm == 1:
        assert "\tNA\t" in lines[1]
    # the head of the last line and the first columns are -N's
    n = _run(["search", fx["db"], "-q", fx["q"], "-N", str(W)] + (["-v", str(v)] if v else []), HOST).stdout.decode().splitlines()
    assert lines[-1].split("\t")[0] == n[-1]
    assert [(l.split("\t")[0], l.split("\t")[1], l.split("\t")[2]) for l in lines[1:-1]] == \
           [(l.split("\t")[0], l.split("\t")[1], l.split("\t")[3]) for l in n[1:-1]]


def test_an_empty_or_missing_query_file_gives_zeros_and_NA(fx):
    e = np.zeros(0, np.int32)
    want = expected_text(fx, 3, 100, 0, PR.CIRCULAR, 0, regions=(e, e, e))
    empty = os.path.join(fx["d"], "empty.bed")
    open(empty, "w").close()
    for q in (empty, os.path.join(fx["d"], "missing.bed")):
        got = _run(["search", fx["db"], "-q", q, "-P", "3", "-g", fx["g"], "-D", "100"], HOST)
        assert got.returncode == 0 and got.stdout.decode() == want, q
    assert want.endswith("Regions with a dataset within 100 bp: 0 of 0; overlapping: 0; mean distance NA\t0.000000\t0.000000\tNA\t0.000000\t"
                         "NA\tNA\tNA\t0\t0\t0.602060\n")


@pytest.mark.parametrize("other", [["-N", "5"], ["-O", "5"], ["-A", "0.5"], ["-B", "0.5"], ["-Q", "Q"], ["-u"], ["-b"], ["-w"], ["-U", "Q"],
                                   ["-U", "Q", "-R"], ["-U", "Q", "-X"], ["-R"], ["-X"], ["-C"], ["-f"], ["-m"], ["-s"],
                                   ["-r", "chr1", "1000", "90000"]])
def test_D_together_with_another_selector_is_refused(fx, other):
    other = [fx["q"] if a == "Q" else a for a in other]
    for args in (["-q", fx["q"], "-P", "5", "-g", fx["g"], "-D", "100"] + other, other + ["-D", "100", "-P", "5", "-g", fx["g"], "-q", fx["q"]]):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 64 and got.stdout.decode().startswith("Not supported: -D together with "), (args, got.stdout)
        assert b"n_within" not in got.stdout


def test_D_without_P_g_or_q_and_bad_numbers_are_refused(fx):
    def run(args):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 64 and b"index" not in got.stdout, (args, got.stdout)
        return got.stdout.decode()
    assert run(["-q", fx["q"], "-D", "100"]) == "Not supported: -D without -P\n"
    assert run(["-q", fx["q"], "-g", fx["g"], "-D", "100"]) == "Not supported: -D without -P\n"
    assert run(["-q", fx["q"], "-P", "5", "-D", "100"]) == "Not supported: -D -P without -g\n"
    assert run(["-P", "5", "-g", fx["g"], "-D", "100"]) == "Not supported: -D -P without -q\n"
    assert run(["-q", fx["q"], "-P", "5", "-g", fx["g"], "-D"]) == "Not supported: -D without a window\n"
    for n in ("0", "-4", "1048577", "ten", "5x"):
        assert run(["-q", fx["q"], "-g", fx["g"], "-P", n, "-D", "100"]).startswith("Not supported: -D with a number of permutations")
    assert run(["-q", fx["q"], "-g", fx["g"], "-P", "5", "-M", "rotate", "-D", "100"]).startswith("Not supported: -D with a -M")
    for w in ("-1", "-5", "1073741825", "99999999999999999999", "ten", "5x", ""):
        assert run(["-q", fx["q"], "-g", fx["g"], "-P", "5", "-D", w]) == \
               "Not supported: -D %s (a window of 0 to 1073741824 base pairs)\n" % w


def test_plain_P_and_plain_N_print_what_they_printed(fx):
    """without -D the -P table is the support table and the -N table is nearest_ref's"""
    p = _run(["search", fx["db"], "-q", fx["q"], "-P", "4", "-g", fx["g"]], HOST)
    assert p.returncode == 0
    lines = p.stdout.decode().splitlines()
    assert lines[0] == "index\tobserved\tmean\tsd\tz\tn_ge\tn_le\tnlog10_p_upper\tnlog10_p_lower\tFile" and len(lines) == NFILES + 2
    assert lines[-1].startswith("Query regions with a hit: ")
    ichr, qs, qe = fx["regions"]
    dist, dmin = ref_rows(fx["ldb"], ichr, qs, qe, 900, None)
    nw, no, sd = ref_sets(dist, dmin, np.array([0, len(qs)], np.int64))
    n = _run(["search", fx["db"], "-q", fx["q"], "-N", "900"], HOST)
    assert n.returncode == 0 and n.stdout.decode() == nearest_table(fx["ldb"].names, nw[0], no[0], sd[0], 900, len(qs))
    # -N -P stays refused as it was
    r = _run(["search", fx["db"], "-q", fx["q"], "-N", "900", "-P", "4", "-g", fx["g"]], HOST)
    assert r.returncode == 0 and r.stdout.decode().startswith("Not supported: -N together with")
