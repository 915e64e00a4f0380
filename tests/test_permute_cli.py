"""`igd search db.igd -q regions.bed -P N -g genome.sizes [-S seed] [-M circular|shuffle] [-v N]` on the host route: the
header, one line per dataset (floats as %.6f), then `-u`'s last line carrying the statistics of the any-dataset column.

Expected text never comes from the code under test: permute_ref's explicit lists through igdc_support_host (held against the
oracle in tests/test_support_host.py), the statistics and the summary from permute_ref in numpy.  Every refusal, and the
genome file's errors."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import permute_ref as PR
from helpers import GOLDEN, short_tmpdir, write_bed
from test_permute_host import reference_rows
from test_sets_cli import EXE
from test_support_host import HOST, HostDb, _index, _run, cli_rule, clustered_db

HEADER = "index\tobserved\tmean\tsd\tz\tn_ge\tn_le\tnlog10_p_upper\tnlog10_p_lower\tFile\n"
REFUSED = "Not supported: -P together with -Q, -u, -b, -w, -U, -R, -X, -C, -f, -m, -s or -r\n"
NBP, NCTG = 1 << 12, 2


@pytest.fixture(scope="module")
def fx():
    """a clustered database of 7 files on two contigs, a BED file of valid regions (with lines that are not accepted and a
    contig the database lacks) and a genome file that names one contig more"""
    d = short_tmpdir("ipc")
    rng = random.Random(61)
    db, span = clustered_db(rng, d, "db", NBP, 1, 7, NCTG, 12)
    ctg_len = np.array([span + 2 * NBP, span + 777], np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 400, unknown=())
    keep = qe > 0                                             # (the command line accepts lines with end > 0)
    ichr, qs, qe = ichr[keep], qs[keep], qe[keep]
    rows = [("chr%d" % (c + 1), int(s), int(e)) for c, s, e in zip(ichr, qs, qe)]
    rows[3:3] = [("chrNotThere", 5, 500), ("x", 1, 2)]
    q = os.path.join(d, "q.bed")
    write_bed(q, rows)
    g = os.path.join(d, "genome.sizes")
    with open(g, "w") as f:
        f.write("chr2\t%d\nchrOther\t5000000000\nchr1\t%d\r\n\n" % (ctg_len[1], ctg_len[0]))
    yield dict(d=d, db=db, q=q, g=g, ctg_len=ctg_len, regions=(ichr, qs, qe))
    shutil.rmtree(d, ignore_errors=True)


def fmt(x):
    return "%.6f" % x


def expected_text(fx, nperm, seed, mode, v, regions=None):
    ichr, qs, qe = fx["regions"] if regions is None else regions
    H = HostDb(fx["db"])
    try:
        rule, ev = cli_rule(1, v)
        obs, rows = reference_rows(H, ichr, qs, qe, fx["ctg_len"], nperm, seed, mode, ev, rule)
    finally:
        H.close()
    st = PR.stats(rows, obs)
    mean, sd, z, pu, pl = PR.summary(rows, obs)
    out = [HEADER]
    names = [name for _, name in _index(fx["db"])]
    for f in range(len(names)):
        out.append("%d\t%d\t%s\t%s\t%s\t%d\t%d\t%s\t%s\t%s\n" % (f, obs[f], fmt(mean[f]), fmt(sd[f]), fmt(z[f]), st[2][f], st[3][f],
                                                                fmt(pu[f]), fmt(pl[f]), names[f]))
    a = len(names)
    out.append("Query regions with a hit: %d of %d\t%s\t%s\t%s\t%d\t%d\t%s\t%s\n" % (obs[a], len(qs), fmt(mean[a]), fmt(sd[a]), fmt(z[a]),
                                                                                   st[2][a], st[3][a], fmt(pu[a]), fmt(pl[a])))
    return "".join(out)


@pytest.mark.parametrize("extra,nperm,seed,mode,v", [([], 7, 0, PR.CIRCULAR, 0), (["-S", "5", "-M", "shuffle"], 20, 5, PR.SHUFFLE, 0),
                                                    (["-M", "circular", "-v", "500"], 3, 0, PR.CIRCULAR, 500),
                                                    (["-S", "18446744073709551615"], 1, 2 ** 64 - 1, PR.CIRCULAR, 0)])
def test_cli_P_prints_the_reference_table_on_the_host_route(fx, extra, nperm, seed, mode, v):
    want = expected_text(fx, nperm, seed, mode, v)
    for args in (["-q", fx["q"], "-P", str(nperm), "-g", fx["g"]] + extra, extra + ["-g", fx["g"], "-P", str(nperm), "-q", fx["q"]]):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 0, got.stderr
        assert got.stdout.decode() == want, args
    lines = want.splitlines()
    assert len(lines) == 7 + 2 and lines[-1].startswith("Query regions with a hit: ")
    if nperm == 1:
        assert "\tnan\tnan\t" in lines[1]
    # the observed column and the last line's head are -u's
    u = _run(["search", fx["db"], "-q", fx["q"], "-u"] + (["-v", str(v)] if v else []), HOST).stdout.decode().splitlines()
    assert lines[-1].split("\t")[0] == u[-1]
    sup = {int(l.split("\t")[0]): int(l.split("\t")[2]) for l in u[1:-1]}
    assert {int(l.split("\t")[0]): int(l.split("\t")[1]) for l in lines[1:-1] if int(l.split("\t")[1])} == sup


def test_an_empty_or_missing_query_file_gives_zeros(fx):
    e = np.zeros(0, np.int32)
    want = expected_text(fx, 3, 0, PR.CIRCULAR, 0, regions=(e, e, e))
    empty = os.path.join(fx["d"], "empty.bed")
    open(empty, "w").close()
    for q in (empty, os.path.join(fx["d"], "missing.bed")):
        got = _run(["search", fx["db"], "-q", q, "-P", "3", "-g", fx["g"]], HOST)
        assert got.returncode == 0 and got.stdout.decode() == want, q
    assert want.endswith("Query regions with a hit: 0 of 0\t0.000000\t0.000000\tnan\t3\t3\t0.000000\t0.000000\n")


@pytest.mark.parametrize("other", [["-u"], ["-b"], ["-w"], ["-U", "Q"], ["-U", "Q", "-R"], ["-U", "Q", "-X"], ["-R"], ["-X"], ["-C"], ["-f"],
                                   ["-m"], ["-s"], ["-r", "chr1", "1000", "90000"], ["-Q", "Q"]])
def test_P_together_with_another_selector_is_refused(fx, other):
    other = [fx["q"] if a == "Q" else a for a in other]
    for args in (["-q", fx["q"], "-P", "5", "-g", fx["g"]] + other, other + ["-P", "5", "-g", fx["g"], "-q", fx["q"]]):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 0 and got.stdout.decode() == REFUSED, args


def test_P_without_g_and_g_S_M_without_P_are_refused(fx):
    run = lambda args: _run(["search", fx["db"]] + args, HOST).stdout.decode()
    assert run(["-q", fx["q"], "-P", "5"]) == "Not supported: -P without -g\n"
    assert run(["-P", "5", "-g", fx["g"]]) == "Not supported: -P without -q\n"
    for args in (["-g", fx["g"]], ["-S", "4"], ["-M", "shuffle"], ["-u", "-g", fx["g"]], ["-S", "1", "-M", "circular", "-g", fx["g"]]):
        assert run(["-q", fx["q"]] + args) == "Not supported: -g, -S or -M without -P\n", args
    for n in ("0", "-4", "1048577", "ten", "5x"):
        assert run(["-q", fx["q"], "-g", fx["g"], "-P", n]) == "Not supported: -P %s (1 to 1048576 permutations)\n" % n
    assert run(["-q", fx["q"], "-g", fx["g"], "-P", "5", "-M", "rigid"]) == "Not supported: -M rigid (circular or shuffle)\n"
    assert run(["-q", fx["q"], "-g", fx["g"], "-P"]) == "No number of permutations.\n"
    usage = subprocess.run([EXE, "search"], stderr=subprocess.PIPE, stdout=subprocess.PIPE).stderr.decode()
    assert "    -P <" in usage and "    -g <" in usage and "-S <seed>" in usage and "    -C   " in usage


def test_regions_outside_their_contig_and_genome_file_errors_name_the_line(fx):
    d = fx["d"]
    run = lambda q, g: _run(["search", fx["db"], "-q", q, "-P", "2", "-g", g], HOST)
    L0 = int(fx["ctg_len"][0])
    q = os.path.join(d, "out.bed")
    write_bed(q, [("chr1", 5, 50), ("chrNotThere", 1, 2), ("chr1", 100, L0 + 1), ("chr1", 7, 3)])
    got = run(q, fx["g"])
    assert got.returncode == 0
    assert got.stdout.decode() == "%s, line 3: region chr1:100-%d does not lie on its contig of length %d\n" % (q, L0 + 1, L0)
    write_bed(q, [("chr1", 5, 50), ("chr1", L0 - 1, L0), ("chr1", 70, 30)])
    assert run(q, fx["g"]).stdout.decode() == "%s, line 3: region chr1:70-30 does not lie on its contig of length %d\n" % (q, L0)
    # a contig the genome file lacks
    g1 = os.path.join(d, "one.sizes")
    open(g1, "w").write("chr1\t%d\n" % L0)
    write_bed(q, [("chr1", 5, 50), ("chr2", 5, 50)])
    assert run(q, g1).stdout.decode() == "%s, line 2: contig chr2 is not in the genome file %s\n" % (q, g1)
    write_bed(q, [("chr1", 5, 50)])
    assert run(q, g1).stdout.decode().startswith(HEADER)
    # the genome file itself
    missing = os.path.join(d, "nowhere.sizes")
    assert run(q, missing).stdout.decode() == "Cannot open genome file %s\n" % missing
    for k, text in enumerate(("chr1\t%d\nchr2\t2147483648\n" % L0, "chr1\t%d\nchr2\n" % L0, "chr1\t%d\nchr2\t-5\n" % L0, "chr1\t%d\nchr2\tlong\n" % L0)):
        gb = os.path.join(d, "bad%d.sizes" % k)
        open(gb, "w").write(text)
        assert run(q, gb).stdout.decode() == "Genome file %s, line 2: not a name, a tab and a length of at most 2147483647\n" % gb, text
    gm = os.path.join(d, "max.sizes")
    open(gm, "w").write("chr1\t2147483647\n")
    assert run(q, gm).stdout.decode().startswith(HEADER)


@pytest.mark.parametrize("args", [["-u"], ["-C"], [], ["-v", "500"]])
def test_command_lines_without_P_keep_their_output(args):
    """the new flags' parsing leaves the other selectors alone: the golden branch family prints what the oracle-held tests of
    those selectors expect (they run unchanged); here only that nothing of -P's leaks into them"""
    db, q = os.path.join(GOLDEN, "branch", "db.igd"), os.path.join(GOLDEN, "branch", "q.bed")
    got = _run(["search", db, "-q", q] + args, HOST)
    assert got.returncode == 0 and b"observed" not in got.stdout and b"Not supported" not in got.stdout


def test_engine_route_without_a_device_fails_loudly(fx):
    nodev = {"IGD_HOST_MAX_QUERIES": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
    got = _run(["search", fx["db"], "-q", fx["q"], "-P", "3", "-g", fx["g"]], nodev)
    assert got.returncode == 69 and b"no CPU search path" in got.stderr and got.stdout == b""
