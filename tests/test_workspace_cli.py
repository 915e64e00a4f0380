"""`igd search db.igd -q regions.bed -P N -g genome.sizes -W workspace.bed [-S seed] [-D W | -G] [-v N]` on the host route: the
three tables keep their layout and are, byte for byte, the reference tables of -P, -P -D and -P -G computed from workspace_ref's
explicit lists (the references of those tables take their permuted lists from permute_ref.permute; here that one function is
replaced by workspace_ref.place).  The stderr line, every refusal with its exit code, and -P without -W unchanged."""
import os
import random
import shutil
from unittest import mock

import numpy as np
import pytest

import permute_ref as PR
import test_permute_bp_cli as BP
import test_permute_cli as SP
import test_permute_nearest_cli as NR
import workspace_ref as WR
from helpers import short_tmpdir, write_bed
from nearest_ref import ListDb, clustered_lists
from test_support_host import HOST, _run

NBP = 1 << 12


@pytest.fixture(scope="module")
def wfx():
    d = short_tmpdir("iwc")
    rng = random.Random(83)
    files, span = clustered_lists(rng, NBP, 7, 2, 12)
    ldb = ListDb(d, "db", files, NBP, 1)
    assert ldb.ctgs == ["chr1", "chr2"]
    ctg_len = np.array([span + 9 * NBP, span + 7 * NBP + 777], np.int32)
    seg = WR.random_workspace(rng, ctg_len, 40, 2500)
    tab = WR.table(*seg, ctg_len)
    n = 250
    ichr = np.array([rng.choice([0, 1]) for _ in range(n)], np.int32)
    ln = np.array([rng.choice([0, 1, 50, 300, 700, 2499, 4000]) for _ in range(n)], np.int32)
    qs = np.array([rng.randrange(0, int(ctg_len[c]) - 4000) for c in ichr], np.int32)
    qe = qs + ln
    keep = qe > 0                                             # (the command line accepts lines with end > 0)
    ichr, qs, qe = ichr[keep], qs[keep], qe[keep]
    assert not WR.unplaceable(ichr, qs, qe, ctg_len, tab).any()
    rows = [(ldb.ctgs[c], int(s), int(e)) for c, s, e in zip(ichr, qs, qe)]
    rows[3:3] = [("chrNotThere", 5, 500), ("x", 1, 2)]
    q = os.path.join(d, "q.bed")
    write_bed(q, rows)
    w = os.path.join(d, "w.bed")
    names = {0: "chr1", 1: "chr2", 2: "chrNotThere", -1: "chrNotThere"}
    write_bed(w, [(names[int(c)], int(a), int(b)) for c, a, b in zip(*seg) if int(b) > 0])
    g = os.path.join(d, "genome.sizes")
    with open(g, "w") as f:
        f.write("chr2\t%d\nchrOther\t5000000000\nchr1\t%d\r\n\n" % (ctg_len[1], ctg_len[0]))
    yield dict(d=d, ldb=ldb, db=ldb.path, q=q, g=g, w=w, ctg_len=ctg_len, regions=(ichr, qs, qe), tab=tab, seg=seg)
    shutil.rmtree(d, ignore_errors=True)


def placed_by(tab):
    """permute_ref.permute replaced by the workspace placement (the mode argument is not looked at)"""
    return mock.patch.object(PR, "permute", lambda ichr, qs, qe, ctg_len, p0, np_, seed=0, mode=None: WR.place(ichr, qs, qe, ctg_len, tab, p0, np_, seed))


def outside_line(fx):
    ichr, qs, qe = fx["regions"]
    n = int((~WR.inside(ichr, qs, qe, fx["tab"])).sum())
    assert 0 < n < len(qs)
    return "%d of %d regions do not lie inside the workspace\n" % (n, len(qs))


@pytest.mark.parametrize("extra,nperm,seed,v", [([], 7, 0, 0), (["-S", "5"], 20, 5, 0), (["-v", "500"], 3, 0, 500)])
def test_cli_W_prints_the_three_reference_tables_on_the_host_route(wfx, extra, nperm, seed, v):
    with placed_by(wfx["tab"]):
        want = {(): SP.expected_text(wfx, nperm, seed, None, v), ("-D", "700"): NR.expected_text(wfx, nperm, 700, seed, None, v),
                ("-G",): BP.expected_text(wfx, nperm, seed, None, v)}
        shuffled = SP.expected_text(wfx, nperm, seed, PR.SHUFFLE, v)
    assert PR.permute.__module__ == "permute_ref"               # (the patch is gone)
    base = ["search", wfx["db"], "-q", wfx["q"], "-P", str(nperm), "-g", wfx["g"], "-W", wfx["w"]] + extra
    for stat, text in want.items():
        for args in (base + list(stat), ["search", wfx["db"]] + list(stat) + extra + ["-W", wfx["w"], "-g", wfx["g"], "-P", str(nperm), "-q", wfx["q"]]):
            got = _run(args, HOST)
            assert got.returncode == 0, got.stderr
            assert got.stdout.decode() == text, args
            assert got.stderr.decode() == outside_line(wfx)
    assert want[()] == shuffled and len({*want.values()}) == 3          # (the patch was in force for all four)
    # the placement is not the free shuffle's
    free = _run(["search", wfx["db"], "-q", wfx["q"], "-P", str(nperm), "-g", wfx["g"], "-M", "shuffle"] + extra, HOST)
    assert free.returncode == 0 and free.stderr == b"" and (nperm < 7 or free.stdout.decode() != want[()])


def test_P_without_W_prints_what_it_printed(wfx):
    for extra, mode, seed in (([], PR.CIRCULAR, 0), (["-M", "shuffle", "-S", "5"], PR.SHUFFLE, 5)):
        got = _run(["search", wfx["db"], "-q", wfx["q"], "-P", "7", "-g", wfx["g"]] + extra, HOST)
        assert got.returncode == 0 and got.stderr == b"" and got.stdout.decode() == SP.expected_text(wfx, 7, seed, mode, 0)
    got = _run(["search", wfx["db"], "-q", wfx["q"], "-P", "3", "-g", wfx["g"], "-D", "700", "-M", "shuffle"], HOST)
    assert got.returncode == 0 and got.stdout.decode() == NR.expected_text(wfx, 3, 700, 0, PR.SHUFFLE, 0)
    got = _run(["search", wfx["db"], "-q", wfx["q"], "-P", "3", "-g", wfx["g"], "-G", "-M", "shuffle"], HOST)
    assert got.returncode == 0 and got.stdout.decode() == BP.expected_text(wfx, 3, 0, PR.SHUFFLE, 0)
    # the pinned -M messages
    run = lambda args: _run(["search", wfx["db"]] + args, HOST)
    assert run(["-q", wfx["q"], "-M", "shuffle"]).stdout.decode() == "Not supported: -g, -S or -M without -P\n"
    assert run(["-q", wfx["q"], "-g", wfx["g"], "-P", "5", "-M", "rigid"]).stdout.decode() == "Not supported: -M rigid (circular or shuffle)\n"


def test_a_workspace_that_holds_every_region_is_silent(wfx):
    w = os.path.join(wfx["d"], "whole.bed")
    write_bed(w, [("chr1", 0, int(wfx["ctg_len"][0])), ("chr2", 0, int(wfx["ctg_len"][1]))])
    got = _run(["search", wfx["db"], "-q", wfx["q"], "-P", "7", "-g", wfx["g"], "-W", w, "-S", "5"], HOST)
    # one segment [0, L) per contig: the free shuffle's table, bit for bit
    assert got.returncode == 0 and got.stderr == b"" and got.stdout.decode() == SP.expected_text(wfx, 7, 5, PR.SHUFFLE, 0)


def test_refusals_and_exit_codes(wfx):
    run = lambda args: _run(["search", wfx["db"]] + args, HOST)
    ok = ["-q", wfx["q"], "-P", "5", "-g", wfx["g"]]

    def refused(args, text, code=64):
        got = run(args)
        assert got.returncode == code and got.stdout.decode() == text, (args, got.stdout, got.stderr)
    refused(["-q", wfx["q"], "-W", wfx["w"]], "Not supported: -W without -P\n")
    refused(["-q", wfx["q"], "-W", wfx["w"], "-g", wfx["g"]], "Not supported: -W without -P\n")
    for m in ("circular", "shuffle", "rigid"):
        for stat in ([], ["-D", "100"], ["-G"]):
            refused(ok + stat + ["-W", wfx["w"], "-M", m], "Not supported: -W together with -M (the workspace is the placement)\n")
    refused(ok + ["-W"], "Not supported: -W without a workspace file\n")
    # a workspace file with no usable segment: empty, contigs the database lacks, nothing left on the contigs
    for name, rows in (("e.bed", []), ("o.bed", [("chrNotThere", 5, 500)]), ("z.bed", [("chr1", 2000000000, 2000000100), ("chr2", 7, 7)])):
        w = os.path.join(wfx["d"], name)
        write_bed(w, rows)
        for stat in ([], ["-D", "100"], ["-G"]):
            refused(ok + stat + ["-W", w], "Workspace file %s: no usable segment on a contig of the database\n" % w)
    refused(ok + ["-W", os.path.join(wfx["d"], "missing.bed")], "Cannot open workspace file %s\n" % os.path.join(wfx["d"], "missing.bed"), 0)
    # a region that fits in no segment of its contig: the message names its line
    longest = int(WR.contig(wfx["tab"], 1)[1][0])
    q = os.path.join(wfx["d"], "long.bed")
    write_bed(q, [("chr1", 10, 20), ("x", 1, 2), ("chrNotThere", 5, 500), ("chr2", 100, 100 + longest), ("chr2", 100, 101 + longest), ("chr1", 5, 6)])
    for stat in ([], ["-D", "100"], ["-G"]):
        refused(["-q", q, "-P", "5", "-g", wfx["g"], "-W", wfx["w"]] + stat,
                "%s, line 5: region chr2:100-%d fits in no segment of the workspace %s on its contig\n" % (q, 101 + longest, wfx["w"]))
    # the contig-length refusal comes first and keeps its code
    write_bed(q, [("chr1", 10, 20), ("chr2", 100, 2000000000)])
    got = run(["-q", q, "-P", "5", "-g", wfx["g"], "-W", wfx["w"]])
    assert got.returncode == 0 and got.stdout.decode().startswith("%s, line 2: region chr2:100-2000000000 does not lie on its contig" % q)
    usage = _run(["search"]).stderr.decode()
    assert "    -W <workspace file>" in usage
