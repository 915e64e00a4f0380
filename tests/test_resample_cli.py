"""`igd search db.igd -q set.bed -P N -M resample -U universe.bed [-S seed] [-D W | -G] [-v V] [-O bp]` on the host route: the three
tables keep the layout of -P, -P -D and -P -G and are, byte for byte, those tables computed from resample_ref's explicit lists
through igd_amd.support_host / nearest_sets_host / jaccard_host.  Every refusal with its exit code, and the two answers that must
stay what they were: -P with -U but without -M resample, and -M with any other word."""
import os
import random
import shutil

import numpy as np
import pytest

import permute_bp_ref as PB
import permute_nearest_ref as PN
import permute_ref as PR
import resample_ref as RR
import test_permute_cli as SP
from helpers import short_tmpdir, write_bed
from nearest_ref import ListDb, clustered_lists
from test_resample_host import support_rows
from test_support_host import HOST, _run

NBP = 1 << 12


@pytest.fixture(scope="module")
def rfx():
    d = short_tmpdir("irc")
    rng = random.Random(87)
    files, span = clustered_lists(rng, NBP, 7, 2, 12)
    ldb = ListDb(d, "db", files, NBP, 1)
    assert ldb.ctgs == ["chr1", "chr2"]

    def regions(n):
        c = np.array([rng.choice([0, 1]) for _ in range(n)], np.int32)
        s = np.array([rng.randrange(0, span + 5 * NBP) for _ in range(n)], np.int32)
        return c, s, s + np.array([rng.choice([1, 50, 300, 700, 4000]) for _ in range(n)], np.int32)

    def bed(name, reg, junk):
        rows = [(ldb.ctgs[c], int(s), int(e)) for c, s, e in zip(*reg)]
        rows[3:3] = junk                                        # (lines the reader drops: contigs the database lacks)
        path = os.path.join(d, name)
        write_bed(path, rows)
        return path
    pool, reg = regions(400), regions(60)
    yield dict(d=d, ldb=ldb, db=ldb.path, pool=pool, regions=reg, q=bed("q.bed", reg, [("chrNotThere", 5, 500), ("x", 1, 2)]),
               u=bed("u.bed", pool, [("chrNotThere", 7, 70)]))
    shutil.rmtree(d, ignore_errors=True)


def support_text(fx, nperm, seed, **kw):
    rows = support_rows(fx["db"], RR.resample_sets(fx["regions"], fx["pool"], nperm, seed), **kw)
    obs, rows = rows[0], rows[1:]
    st = PR.stats(rows, obs)
    mean, sd, z, pu, pl = PR.summary(rows, obs)
    f = SP.fmt
    out = [SP.HEADER]
    for i, name in enumerate(fx["ldb"].names):
        out.append("%d\t%d\t%s\t%s\t%s\t%d\t%d\t%s\t%s\t%s\n" % (i, obs[i], f(mean[i]), f(sd[i]), f(z[i]), st[2][i], st[3][i], f(pu[i]), f(pl[i]), name))
    a = len(fx["ldb"].names)
    out.append("Query regions with a hit: %d of %d\t%s\t%s\t%s\t%d\t%d\t%s\t%s\n" % (obs[a], len(fx["regions"][1]), f(mean[a]), f(sd[a]), f(z[a]),
                                                                                   st[2][a], st[3][a], f(pu[a]), f(pl[a])))
    return "".join(out)


def nearest_text(fx, nperm, W, seed):
    import igd_amd
    ns = igd_amd.nearest_sets_host(fx["db"], *RR.resample_sets(fx["regions"], fx["pool"], nperm, seed), W)
    return PN.table_text(fx["ldb"].names, ns.n_within, ns.n_overlap, ns.sum_dist, W, len(fx["regions"][1]))


def bp_text(fx, nperm, seed):
    import igd_amd
    js = igd_amd.jaccard_host(fx["db"], *RR.resample_sets(fx["regions"], fx["pool"], nperm, seed))
    return PB.table_text(fx["ldb"].names, js.inter, js.set_bp, js.n_merged.astype(np.int64), int(js.n_dropped[0]), js.file_bp)


@pytest.mark.parametrize("extra,nperm,seed", [([], 7, 0), (["-S", "5"], 20, 5), (["-S", "18446744073709551615"], 2, 2 ** 64 - 1)])
def test_cli_M_resample_prints_the_three_reference_tables_on_the_host_route(rfx, extra, nperm, seed):
    want = {(): support_text(rfx, nperm, seed), ("-D", "700"): nearest_text(rfx, nperm, 700, seed), ("-G",): bp_text(rfx, nperm, seed)}
    base = ["search", rfx["db"], "-q", rfx["q"], "-P", str(nperm), "-M", "resample", "-U", rfx["u"]] + extra
    for stat, text in want.items():
        for args in (base + list(stat), ["search", rfx["db"]] + list(stat) + extra + ["-U", rfx["u"], "-M", "resample", "-P", str(nperm), "-q", rfx["q"]]):
            got = _run(args, HOST)
            assert got.returncode == 0 and got.stderr == b"", (args, got.stderr)
            assert got.stdout.decode() == text, args
    assert len({*want.values()}) == 3
    assert want[()].splitlines()[0] + "\n" == SP.HEADER and want[("-D", "700")].startswith(PN.HEADER)


def test_the_support_table_under_a_filter_and_a_minimum_overlap(rfx):
    base = ["search", rfx["db"], "-q", rfx["q"], "-P", "5", "-M", "resample", "-U", rfx["u"]]
    got = _run(base + ["-v", "500"], HOST)
    assert got.returncode == 0 and got.stdout.decode() == support_text(rfx, 5, 0, v=500)
    got = _run(base + ["-O", "40"], HOST)
    assert got.returncode == 0 and got.stdout.decode() == support_text(rfx, 5, 0, min_overlap=40)
    assert support_text(rfx, 5, 0, min_overlap=40) != support_text(rfx, 5, 0)


def test_a_set_that_is_the_universe(rfx):
    """every draw is the universe in another order: mean = observed, sd 0, every permutation both >= and <= the observed count"""
    got = _run(["search", rfx["db"], "-q", rfx["u"], "-P", "4", "-M", "resample", "-U", rfx["u"]], HOST)
    assert got.returncode == 0 and got.stderr == b""
    lines = got.stdout.decode().splitlines()
    names = rfx["ldb"].names
    assert lines[0] + "\n" == SP.HEADER and len(lines) == len(names) + 2
    for i, line in enumerate(lines[1:-1]):
        f = line.split("\t")
        assert len(f) == 10 and int(f[0]) == i and f[9] == names[i], line
        assert float(f[2]) == int(f[1]) and f[3] == "0.000000" and f[5] == "4" and f[6] == "4", line
    assert any(int(line.split("\t")[1]) > 0 for line in lines[1:-1])
    f = lines[-1].split("\t")
    nhit = int(f[0].split(": ")[1].split(" of ")[0])
    assert f[0] == "Query regions with a hit: %d of 400" % nhit and nhit > 0 and len(f) == 8
    assert float(f[1]) == nhit and f[2] == "0.000000" and f[4] == "4" and f[5] == "4"


def test_refusals_and_exit_codes(rfx):
    run = lambda args: _run(["search", rfx["db"]] + args, HOST)
    g = os.path.join(rfx["d"], "genome.sizes")
    with open(g, "w") as f:
        f.write("chr1\t100000000\nchr2\t100000000\n")
    ok = ["-q", rfx["q"], "-P", "5", "-M", "resample"]

    def refused(args, text):
        got = run(args)
        assert got.returncode == 64 and got.stdout == b"" and got.stderr.decode() == "Not supported: " + text + "\n", (args, got.stdout, got.stderr)
    for stat in ([], ["-D", "100"], ["-G"]):
        refused(ok + stat, "-M resample without -U")
        refused(ok + stat + ["-U", rfx["u"], "-g", g], "-M resample together with -g or -W (the universe is the placement)")
        refused(ok + stat + ["-U", rfx["u"], "-W", rfx["u"]], "-M resample together with -g or -W (the universe is the placement)")
    for other in (["-Q", rfx["q"]], ["-R"], ["-X"], ["-K", rfx["q"]]):
        refused(ok + ["-U", rfx["u"]] + other, "-M resample together with -Q, -R, -X, -K or -Z")
    # -Z refuses it itself, in its own words: its -M knows circular and shuffle only
    got = run(ok + ["-U", rfx["u"], "-Z", "100,10"])
    assert got.returncode == 64 and got.stdout == b"" and got.stderr.decode().startswith("Not supported: -Z together with")
    got = run(["-q", rfx["q"], "-g", g, "-P", "5", "-M", "resample", "-Z", "100,10"])
    assert got.returncode == 64 and got.stderr.decode() == "Not supported: -Z with a -M that is neither circular nor shuffle\n"
    refused(ok + ["-U", rfx["u"], "-u"], "-M resample together with -u, -b, -w, -C, -f, -m, -s, -r, -J, -V, -N, -H, -L or -E")
    refused(["-q", rfx["q"], "-P", "0", "-M", "resample", "-U", rfx["u"]], "-M resample with a number of permutations outside 1 to 1048576")
    for w in ("-1", "1073741825", "7x"):
        refused(ok + ["-U", rfx["u"], "-D", w], "-D %s (a window of 0 to 1073741824 base pairs)" % w)
    refused(ok + ["-U", rfx["u"], "-D", "5", "-G"], "-M resample together with both -D and -G")
    refused(ok + ["-U", rfx["u"], "-G", "-O", "5"], "-M resample -D or -G together with -O, -A or -B")
    # a set larger than the universe: 400 accepted lines against 60
    for stat in ([], ["-D", "100"], ["-G"]):
        refused(["-q", rfx["u"], "-P", "5", "-M", "resample", "-U", rfx["q"]] + stat,
                "-M resample with a set of 400 regions, more than the 60 of the universe %s" % rfx["q"])
    # a universe above the batch (lowered to 100 regions for the child; the set of 60 still fits)
    for stat in ([], ["-D", "100"], ["-G"]):
        got = _run(["search", rfx["db"]] + ok + ["-U", rfx["u"]] + stat, dict(HOST, IGD_HIP_MAX_BATCH="100"))
        assert got.returncode == 64 and got.stdout == b"" and got.stderr.decode() == "Not supported: -M resample with a universe of 400 regions, more than 100\n"
    # a universe that cannot be read, or holds nothing: -U's own words and code
    missing = os.path.join(rfx["d"], "missing.bed")
    got = run(ok + ["-U", missing])
    assert got.returncode == 0 and got.stdout.decode() == "Cannot read universe file %s, or it holds no region\n" % missing
    assert "    -M resample -U <universe>" in _run(["search"]).stderr.decode()


def test_the_two_answers_that_stay_what_they_were(rfx):
    run = lambda args: _run(["search", rfx["db"]] + args, HOST)
    g = os.path.join(rfx["d"], "genome2.sizes")
    with open(g, "w") as f:
        f.write("chr1\t100000000\nchr2\t100000000\n")
    text = "Not supported: -P together with -Q, -u, -b, -w, -U, -R, -X, -C, -f, -m, -s or -r\n"
    for extra in ([], ["-g", g], ["-g", g, "-M", "shuffle"], ["-M", "circular"]):
        got = run(["-q", rfx["q"], "-P", "5", "-U", rfx["u"]] + extra)
        assert got.returncode == 0 and got.stderr == b"" and got.stdout.decode() == text, extra
    for word in ("rigid", "Resample", "resampled", "resample "):
        got = run(["-q", rfx["q"], "-g", g, "-P", "5", "-M", word])
        assert got.returncode == 0 and got.stderr == b"" and got.stdout.decode() == "Not supported: -M %s (circular or shuffle)\n" % word
    # (what did change: the word `resample` is now a mode of its own, refused for what it lacks and not as an unknown word)
    got = run(["-q", rfx["q"], "-g", g, "-P", "5", "-M", "resample"])
    assert got.returncode == 64 and got.stdout == b"" and got.stderr.decode() == "Not supported: -M resample without -U\n"
    # and the word itself without -U's companion -P is what any -M without -P is
    assert run(["-q", rfx["q"], "-M", "resample"]).stdout.decode() == "Not supported: -g, -S or -M without -P\n"
