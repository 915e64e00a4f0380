"""`igd search db.igd -q regions.bed -P N -g genome.sizes -I <op> [-S seed] [-M circular|shuffle | -W workspace.bed] [-v V]` and
`-P N -M resample -U universe.bed -I <op>` on the host route, byte for byte against a table this test formats from the reference
matrices (tests/permute_map_ref.py); every refusal of -I is one line and exit code 64; command lines without -I print what the
parent commit printed (tests/golden/permute_map_cli_parent.json, recorded from a build of it on this module's fixture)."""
import json
import os
import random
import shutil

import numpy as np
import pytest

import permute_map_ref as PM
import permute_ref as PR
import workspace_ref as WR
from helpers import ROOT, short_tmpdir, write_bed
from nearest_ref import ListDb, clustered_lists
from test_support_host import HOST, _run

NBP = 1 << 12
OPS = ("count", "sum", "min", "max", "mean")
PARENT = os.path.join(ROOT, "tests", "golden", "permute_map_cli_parent.json")
# the command lines whose answers the parent commit gave, run in the fixture's directory
UNCHANGED = {"P": ["-q", "q.bed", "-P", "5", "-g", "genome.sizes"], "PD": ["-q", "q.bed", "-P", "5", "-g", "genome.sizes", "-D", "100"],
             "V": ["-q", "q.bed", "-V", "sum"], "VP": ["-q", "q.bed", "-V", "sum", "-P", "5", "-g", "genome.sizes"]}


def make_fixture(d):
    """a database with signed values on two contigs, a query file, a genome file, a workspace file every region fits in, a universe
    file; everything from one seed, so that the recorded answers of the parent commit stay the answers"""
    rng = random.Random(91)
    files, span = clustered_lists(rng, NBP, 7, 2, 12, -1000)
    ldb = ListDb(d, "db", files, NBP, 1)
    assert ldb.ctgs == ["chr1", "chr2"]
    ctg_len = np.array([span + 9 * NBP, span + 7 * NBP + 777], np.int32)
    seg = WR.random_workspace(rng, ctg_len, 40, 2500)
    tab = WR.table(*seg, ctg_len)

    def regions(n):
        c = np.array([rng.choice([0, 1]) for _ in range(n)], np.int32)
        s = np.array([rng.randrange(0, int(ctg_len[k]) - 2500) for k in c], np.int32)
        return c, s, s + np.array([rng.choice([1, 50, 300, 700, 2499]) for _ in range(n)], np.int32)

    def bed(name, reg, junk):
        rows = [(ldb.ctgs[c], int(s), int(e)) for c, s, e in zip(*reg)]
        rows[3:3] = junk                                        # (lines the reader drops: contigs the database lacks)
        write_bed(os.path.join(d, name), rows)
        return os.path.join(d, name)
    reg, pool = regions(200), regions(400)
    assert not WR.unplaceable(*reg, ctg_len, tab).any()
    names = {0: "chr1", 1: "chr2", 2: "chrNotThere", -1: "chrNotThere"}
    w = os.path.join(d, "w.bed")
    write_bed(w, [(names[int(c)], int(a), int(b)) for c, a, b in zip(*seg) if int(b) > 0])
    g = os.path.join(d, "genome.sizes")
    with open(g, "w") as f:
        f.write("chr2\t%d\nchrOther\t5000000000\nchr1\t%d\n" % (ctg_len[1], ctg_len[0]))
    return dict(d=d, ldb=ldb, db=ldb.path, ctg_len=ctg_len, tab=tab, regions=reg, pool=pool, w=w, g=g,
                q=bed("q.bed", reg, [("chrNotThere", 5, 500), ("x", 1, 2)]), u=bed("u.bed", pool, [("chrNotThere", 7, 70)]))


@pytest.fixture(scope="module")
def fx():
    d = short_tmpdir("imq")
    yield make_fixture(d)
    shutil.rmtree(d, ignore_errors=True)


def expected_text(fx, nperm, op, seed, mode, v):
    rows = PM.null(fx["ldb"], *fx["regions"], fx["ctg_len"], nperm, op, seed, mode, v if v > 0 else None, tab=fx["tab"], pool=fx["pool"])
    return PM.table_text(fx["ldb"].names, *rows, op)


def placement_args(fx, mode):
    return {"circular": ["-g", fx["g"]], "shuffle": ["-g", fx["g"], "-M", "shuffle"], "workspace": ["-g", fx["g"], "-W", fx["w"]],
            "resample": ["-M", "resample", "-U", fx["u"]]}[mode]


@pytest.mark.parametrize("mode", ["circular", "workspace", "resample"])
@pytest.mark.parametrize("op", OPS)
def test_cli_I_prints_the_reference_table_on_the_host_route(fx, op, mode):
    for extra, nperm, seed, v in (([], 7, 0, 0), (["-S", "5", "-v", "500"], 20, 5, 500)):
        want = expected_text(fx, nperm, op, seed, mode, v)
        place = placement_args(fx, mode)
        for args in (["-q", fx["q"], "-P", str(nperm)] + place + ["-I", op] + extra, ["-I", op] + extra + place + ["-P", str(nperm), "-q", fx["q"]]):
            got = _run(["search", fx["db"]] + args, HOST)
            assert got.returncode == 0, got.stderr
            assert got.stdout.decode() == want, args
        lines = want.splitlines()
        assert lines[0] == (PM.HEADER % op).rstrip("\n") and len(lines) == len(fx["ldb"].names) + 1 and len(lines[1].split("\t")) == 15


def test_the_seed_changes_the_table_and_repeats_it(fx):
    def run(seed):
        got = _run(["search", fx["db"], "-q", fx["q"], "-P", "9", "-g", fx["g"], "-I", "mean", "-M", "shuffle", "-S", seed], HOST)
        assert got.returncode == 0
        return got.stdout
    assert run("7") == run("7") != run("8")
    assert run("7").decode() == expected_text(fx, 9, "mean", 7, PR.SHUFFLE, 0)
    # the observed columns are -V's
    v = _run(["search", fx["db"], "-q", fx["q"], "-V", "mean"], HOST).stdout.decode().splitlines()[1:-1]
    assert [l.split("\t")[1] for l in run("7").decode().splitlines()[1:]] == [l.split("\t")[1] for l in v]


def test_one_permutation_and_an_empty_query_file_print_NA(fx):
    one = _run(["search", fx["db"], "-q", fx["q"], "-P", "1", "-g", fx["g"], "-I", "sum"], HOST).stdout.decode()
    assert one == expected_text(fx, 1, "sum", 0, PR.CIRCULAR, 0) and "\tNA\t" in one
    empty = os.path.join(fx["d"], "empty.bed")
    open(empty, "w").close()
    e = np.zeros(0, np.int32)
    want = PM.table_text(fx["ldb"].names, *PM.null(fx["ldb"], e, e, e, fx["ctg_len"], 3, "max"), "max")
    got = _run(["search", fx["db"], "-q", empty, "-P", "3", "-g", fx["g"], "-I", "max"], HOST)
    assert got.returncode == 0 and got.stdout.decode() == want
    assert want.splitlines()[1].startswith("0\t0\tNA\t0\tNA\tNA\tNA\t0\t0\tNA\tNA\t0.000000\t0.000000\tNA\t")


TOGETHER = "Not supported: -I together with -D, -G, -V, -N, -H, -L, -E, -J, -Z, -K, -Q, -u, -b, -w, -R, -X, -C, -f, -m, -s, -r, -O, -A or -B\n"


@pytest.mark.parametrize("other", [["-D", "100"], ["-G"], ["-V", "sum"], ["-N", "5"], ["-N", "5", "-H", "0"], ["-N", "5", "-L", "4"], ["-N", "5", "-L", "4", "-E"],
                                   ["-J"], ["-Z", "100,50"], ["-K", "Q"], ["-Q", "Q"], ["-u"], ["-b"], ["-w"], ["-U", "Q", "-R"], ["-U", "Q", "-X"],
                                   ["-C"], ["-f"], ["-m"], ["-s"], ["-r", "chr1", "1000", "90000"], ["-O", "5"], ["-A", "0.5"], ["-B", "0.5"]])
def test_I_together_with_another_selector_is_refused(fx, other):
    other = [fx["q"] if a == "Q" else a for a in other]
    for args in (["-q", fx["q"], "-P", "5", "-g", fx["g"], "-I", "sum"] + other, other + ["-I", "sum", "-P", "5", "-g", fx["g"], "-q", fx["q"]]):
        got = _run(["search", fx["db"]] + args, HOST)
        assert got.returncode == 64 and got.stdout.decode() == TOGETHER and got.stderr == b"", (args, got.stdout)


def test_the_other_refusals_of_I(fx, tmp_path):
    def run(args, db=fx["db"]):
        got = _run(["search", db] + args, HOST)
        assert got.returncode == 64 and b"index" not in got.stdout and got.stdout.count(b"\n") == 1, (args, got.stdout, got.stderr)
        return got.stdout.decode()
    # -I sum before and after -q
    assert run(["-q", fx["q"], "-I", "sum"]) == run(["-I", "sum", "-q", fx["q"]]) == "Not supported: -I without -P\n"
    assert run(["-q", fx["q"], "-g", fx["g"], "-I", "sum"]) == "Not supported: -I without -P\n"
    assert run(["-q", fx["q"], "-P", "5", "-U", fx["u"], "-I", "sum"]) == "Not supported: -I with -U but without -M resample\n"
    assert run(["-q", fx["q"], "-P", "5", "-g", fx["g"], "-M", "shuffle", "-U", fx["u"], "-I", "sum"]) == \
        "Not supported: -I with -U but without -M resample\n"
    for op in ("median", "SUM", "5", ""):
        assert run(["-q", fx["q"], "-P", "5", "-g", fx["g"], "-I", op]) == "Not supported: -I %s (count, sum, min, max or mean)\n" % op
    assert run(["-q", fx["q"], "-P", "5", "-g", fx["g"], "-I"]) == "Not supported: -I without an op (count, sum, min, max or mean)\n"
    # a value op on a database without values; count works there
    files, _ = clustered_lists(random.Random(3), NBP, 3, 2, 12)
    blind = ListDb(str(tmp_path), "blind", files, NBP, 0)
    for op in ("sum", "min", "max", "mean"):
        assert run(["-q", fx["q"], "-P", "5", "-g", fx["g"], "-I", op], blind.path) == \
            "Not supported: -I %s on a database without values (gType 0); -I count works there\n" % op
    got = _run(["search", blind.path, "-q", fx["q"], "-P", "5", "-g", fx["g"], "-I", "count"], HOST)
    assert got.returncode == 0 and got.stdout.decode() == PM.table_text(
        blind.names, *PM.null(blind, *fx["regions"], fx["ctg_len"], 5, "count"), "count")


def test_behind_its_block_I_falls_through_to_the_rows_that_stand(fx):
    """the refusals of -M resample, -W and -P answer a command line with -I as they answer one without"""
    def run(args):
        got = _run(["search", fx["db"]] + args, HOST)
        return got.returncode, got.stdout.decode(), got.stderr.decode()
    base = ["-q", fx["q"], "-P", "5"]
    for tail in (["-g", fx["g"], "-M", "rotate"], [], ["-M", "resample"], ["-M", "resample", "-U", fx["u"], "-g", fx["g"]],
                 ["-g", fx["g"], "-W", fx["w"], "-M", "shuffle"]):
        assert run(base + tail + ["-I", "sum"]) == run(base + tail), tail
    assert run(["-P", "5", "-g", fx["g"], "-I", "sum"]) == run(["-P", "5", "-g", fx["g"]])
    assert run(["-q", fx["q"], "-P", "0", "-g", fx["g"], "-I", "sum"]) == run(["-q", fx["q"], "-P", "0", "-g", fx["g"]])


def test_command_lines_without_I_print_what_the_parent_commit_printed(fx):
    with open(PARENT) as f:
        parent = json.load(f)
    assert sorted(parent) == sorted(UNCHANGED)
    for name, args in UNCHANGED.items():
        got = _run(["search", "db.igd"] + args, HOST, cwd=fx["d"])
        assert [got.returncode, got.stdout.decode(), got.stderr.decode()] == parent[name], name
    assert parent["VP"][1].startswith("Not supported: -V together with ") and parent["P"][1].startswith("index\tobserved\t")
