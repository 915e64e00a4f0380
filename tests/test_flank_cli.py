"""`igd search db.igd -q regions.bed -N <bp> -L <bins> [-E] [-v V]` and `-Q list.txt -N <bp> -L ...` on the host route, byte for
byte against a table formatted from tests/flank_ref.py (the definition over the interval lists this test wrote; the BED files are
read by the oracle's reader, as the other command-line tests read them); every refusal and its exit code; a command line
without -L unchanged."""
import os
import shutil

import numpy as np
import pytest

from flank_ref import EDGES, MIDPOINTS, ref_flanks, ref_hist, table_text
from helpers import Oracle, short_tmpdir
from nearest_ref import MAX_WINDOW
from test_nearest_cli import _db_and_beds
from test_nearest_cli import expected_block as n_block
from test_sets_cli import _write_list
from test_support_host import HOST, _run


@pytest.fixture
def tmp():
    d = short_tmpdir("ifc")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def expected_block(db, orc, qfile, window, v, nbins, measure):
    try:
        ichr, qs, qe = orc.read_queries(qfile)
    except IOError:
        ichr = qs = qe = np.zeros(0, np.int32)
    rows = ref_flanks(db, ichr, qs, qe, window, measure, v if v > 0 else None)
    h = ref_hist(*rows, np.array([0, len(qs)], np.int64), nbins)
    return table_text(db.names, h[0], window, len(qs)), h[0]


@pytest.mark.parametrize("nbp,gtype,nfiles,nctg,span_tiles", [(1 << 14, 1, 7, 2, 10), (1 << 12, 0, 5, 3, 30), (1000, 1, 6, 2, 40)])
def test_cli_l_prints_the_definitions_table_on_the_host_route(nbp, gtype, nfiles, nctg, span_tiles, tmp):
    db, beds = _db_and_beds(tmp, nbp, gtype, nfiles, nctg, span_tiles, 14100 + nfiles)
    orc = Oracle(db.path)
    try:
        assert orc.ctg_names() == db.ctgs
        flanked = 0
        for W in (0, 1, nbp, 3 * nbp + 5, MAX_WINDOW):
            for v in (0, 500):
                extra = ["-v", str(v)] if v else []
                for B in (1, 2, 50, 64):
                    for ms, flag in ((MIDPOINTS, []), (EDGES, ["-E"])):
                        want, h = expected_block(db, orc, beds[0], W, v, B, ms)
                        flanked += int(h.sum())
                        for args in (["-q", beds[0], "-N", str(W), "-L", str(B)] + flag + extra, flag + ["-L", str(B), "-N", str(W)] + extra + ["-q", beds[0]]):
                            got = _run(["search", db.path] + args, HOST)
                            assert got.returncode == 0, got.stderr
                            assert got.stdout.decode() == want, args
        assert flanked > 100, "fixture is vacuous: hardly a flanked region"
        # -Q: one block per file, laid out as -N's; an unreadable file is an empty set
        files = beds + [os.path.join(tmp, "missing.bed")]
        lst = _write_list(tmp, files, crlf=True)
        for W, v, B, ms in ((nbp, 0, 50, MIDPOINTS), (700, 500, 10, EDGES), (0, 0, 1, MIDPOINTS)):
            got = _run(["search", db.path, "-Q", lst, "-N", str(W), "-L", str(B)] + (["-E"] if ms == EDGES else []) + (["-v", str(v)] if v else []), HOST)
            assert got.returncode == 0, got.stderr
            want = "".join("Query set %d: %s\n" % (k, p) + expected_block(db, orc, p, W, v, B, ms)[0] for k, p in enumerate(files))
            assert got.stdout.decode() == want, (W, v)
            assert want.endswith("Any dataset within %d bp: 0 of 0%s\n" % (W, "\t0" * B))
    finally:
        orc.close()


def test_the_header_by_hand(tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 14200, nbeds=1)
    got = _run(["search", db.path, "-q", beds[0], "-N", "5000", "-L", "4"], HOST)
    assert got.returncode == 0
    lines = got.stdout.decode().splitlines()
    assert lines[0] == "index\tn_flanked\t0.0000\t0.1250\t0.2500\t0.3750\tFile"
    assert len(lines) == 5 and lines[1].startswith("0\t") and lines[1].endswith("\tf0000.bed")
    assert lines[4].startswith("Any dataset within 5000 bp: ") and lines[4].count("\t") == 4
    got = _run(["search", db.path, "-q", beds[0], "-N", "5000", "-L", "50", "-E"], HOST)
    head = got.stdout.decode().splitlines()[0].split("\t")
    assert head[:4] == ["index", "n_flanked", "0.0000", "0.0100"] and head[-2:] == ["0.4900", "File"] and len(head) == 53


BAD_BINS = ["", "0", "65", "-1", "abc", "5x", "0.5", "1e1", " 5", "+5", "5,6", "99999999999999999999"]


@pytest.mark.parametrize("bad", BAD_BINS, ids=lambda b: "bins:" + b[:24])
def test_a_bad_number_of_bins_is_a_usage_error(bad, tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 14300, nbeds=1)
    lst = _write_list(tmp, beds)
    for sel in (["-q", beds[0]], ["-Q", lst]):
        for args in (sel + ["-N", "100", "-L", bad], ["-L", bad, "-N", "100", "-E"] + sel):
            got = _run(["search", db.path] + args, HOST)
            assert got.returncode == 64 and got.stdout == b"Not supported: -L " + bad.encode() + b" (1 to 64 bins)\n", args


def test_the_other_refusals_and_the_limits(tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 14400, nbeds=1)
    gen = os.path.join(tmp, "genome.txt")
    open(gen, "w").write("chr1\t1000000\n")
    q = ["-q", beds[0]]
    together = b"Not supported: -L together with -H, -P, -D, -O, -A or -B\n"
    for args, msg in ((q + ["-L", "50"], b"Not supported: -L without -N\n"),
                      (["-L", "50"], b"Not supported: -L without -N\n"),
                      (q + ["-N", "100", "-E"], b"Not supported: -E without -L\n"),
                      (q + ["-E"], b"Not supported: -E without -L\n"),
                      (q + ["-N", "100", "-H", "0,1", "-E"], b"Not supported: -E without -L\n"),
                      (q + ["-N", "100", "-L"], b"Not supported: -L without a number of bins\n"),
                      (q + ["-N", "100", "-L", "50", "-H", "0,1"], together),
                      (q + ["-N", "100", "-L", "50", "-P", "5", "-g", gen], together),
                      (q + ["-N", "100", "-L", "50", "-D", "100"], together),
                      (q + ["-N", "100", "-L", "50", "-P", "5", "-g", gen, "-D", "100"], together),
                      (q + ["-N", "100", "-L", "50", "-O", "10"], together),
                      (q + ["-N", "100", "-L", "50", "-E", "-A", "0.5"], together),
                      (q + ["-N", "100", "-L", "50", "-B", "0.5"], together),
                      (q + ["-L", "50", "-P", "5", "-g", gen, "-D", "100"], b"Not supported: -L without -N\n")):
        got = _run(["search", db.path] + args, HOST)
        assert got.returncode == 64 and got.stdout == msg, args
    # what -N refuses, it refuses with -L too (its own message and exit code)
    got = _run(["search", db.path] + q + ["-N", "100", "-L", "50", "-u"], HOST)
    assert got.returncode == 0 and got.stdout.startswith(b"Not supported: -N together with")
    got = _run(["search", db.path] + q + ["-N", "-5", "-L", "50"], HOST)
    assert got.returncode == 0 and got.stdout.startswith(b"Not supported: -N -5 (")
    for ok in ("1", "64", "050"):
        got = _run(["search", db.path] + q + ["-N", "100", "-L", ok], HOST)
        assert got.returncode == 0 and got.stdout.startswith(b"index\tn_flanked\t0.0000"), ok


def test_engine_route_without_a_device_fails_loudly(tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 14500, nbeds=1)
    nodev = {"IGD_HOST_MAX_QUERIES": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
    got = _run(["search", db.path, "-q", beds[0], "-N", "100", "-L", "50"], nodev)
    assert got.returncode == 69 and b"no CPU search path" in got.stderr and got.stdout == b""


def test_command_lines_without_l_print_what_they_printed(tmp):
    """-N alone still prints -N's table (tests/test_nearest_cli.py holds it byte for byte; here: the same bytes beside a -L run)"""
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 4, 2, 8, 14600, nbeds=2)
    orc = Oracle(db.path)
    try:
        lst = _write_list(tmp, beds)
        for W, v in ((0, 0), (700, 500)):
            extra = ["-v", str(v)] if v else []
            got = _run(["search", db.path, "-q", beds[0], "-N", str(W)] + extra, HOST)
            assert got.returncode == 0 and got.stdout.decode() == n_block(db, orc, beds[0], W, v)[0]
            got = _run(["search", db.path, "-Q", lst, "-N", str(W)] + extra, HOST)
            assert got.stdout.decode() == "".join("Query set %d: %s\n" % (k, p) + n_block(db, orc, p, W, v)[0] for k, p in enumerate(beds))
    finally:
        orc.close()
