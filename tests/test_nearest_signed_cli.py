"""`igd search db.igd -q regions.bed -N <bp> -H e1,e2,... [-v V]` and `-Q list.txt -N <bp> -H ...` on the host route, byte for
byte against a table formatted from tests/nearest_signed_ref.py (the definition over the interval lists this test wrote; the BED
files are read by the oracle's reader, as the other command-line tests read them); every refusal and its exit code; a command
line without -H unchanged."""
import os
import shutil

import numpy as np
import pytest

from helpers import Oracle, short_tmpdir
from nearest_ref import MAX_WINDOW
from nearest_signed_ref import edge_lists, ref_hist, ref_signed_rows, table_text
from test_nearest_cli import _db_and_beds
from test_nearest_cli import expected_block as n_block
from test_sets_cli import _write_list
from test_support_host import HOST, _run


@pytest.fixture
def tmp():
    d = short_tmpdir("ihc")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def expected_block(db, orc, qfile, window, v, edges):
    try:
        ichr, qs, qe = orc.read_queries(qfile)
    except IOError:
        ichr = qs = qe = np.zeros(0, np.int32)
    sdist, sdmin = ref_signed_rows(db, ichr, qs, qe, window, v if v > 0 else None)
    h = ref_hist(sdist, sdmin, np.array([0, len(qs)], np.int64), edges)
    return table_text(db.names, h[0], edges, window, len(qs)), h[0]


def arg(edges):
    return ",".join(str(e) for e in edges)


@pytest.mark.parametrize("nbp,gtype,nfiles,nctg,span_tiles", [(1 << 14, 1, 7, 2, 10), (1 << 12, 0, 5, 3, 30), (1000, 1, 6, 2, 40)])
def test_cli_h_prints_the_definitions_table_on_the_host_route(nbp, gtype, nfiles, nctg, span_tiles, tmp):
    db, beds = _db_and_beds(tmp, nbp, gtype, nfiles, nctg, span_tiles, 9100 + nfiles)
    orc = Oracle(db.path)
    try:
        assert orc.ctg_names() == db.ctgs
        up = down = False
        for W in (0, 1, nbp, 3 * nbp + 5, MAX_WINDOW):
            for v in (0, 500):
                extra = ["-v", str(v)] if v else []
                for edges in edge_lists(W):
                    want, h = expected_block(db, orc, beds[0], W, v, edges)
                    if edges == (0, 1):
                        up |= bool(h[0].any())
                        down |= bool(h[2].any())
                        # the n_within column is -N's
                        nw = n_block(db, orc, beds[0], W, v)[1]
                        assert np.array_equal(h.sum(axis=0), nw)
                    for args in (["-q", beds[0], "-N", str(W), "-H", arg(edges)] + extra, ["-H", arg(edges), "-N", str(W)] + extra + ["-q", beds[0]]):
                        got = _run(["search", db.path] + args, HOST)
                        assert got.returncode == 0, got.stderr
                        assert got.stdout.decode() == want, args
        assert up and down, "fixture is vacuous: no region with its nearest record upstream, or none downstream"
        # -Q: one block per file, laid out as -N's; an unreadable file is an empty set
        files = beds + [os.path.join(tmp, "missing.bed")]
        lst = _write_list(tmp, files, crlf=True)
        for W, v, edges in ((nbp, 0, (-nbp, 0, 1, nbp + 1)), (700, 500, (-100, -10, 0, 1, 11, 101)), (0, 0, (0,))):
            got = _run(["search", db.path, "-Q", lst, "-N", str(W), "-H", arg(edges)] + (["-v", str(v)] if v else []), HOST)
            assert got.returncode == 0, got.stderr
            want = "".join("Query set %d: %s\n" % (k, p) + expected_block(db, orc, p, W, v, edges)[0] for k, p in enumerate(files))
            assert got.stdout.decode() == want, (W, v)
            assert want.endswith("Any dataset within %d bp: 0 of 0%s\n" % (W, "\t0" * (len(edges) + 1)))
    finally:
        orc.close()


def test_the_header_by_hand(tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 9200, nbeds=1)
    got = _run(["search", db.path, "-q", beds[0], "-N", "500", "-H", "-500,0,1,501"], HOST)
    assert got.returncode == 0
    lines = got.stdout.decode().splitlines()
    assert lines[0] == "index\tn_within\t<-500\t[-500,0)\t[0,1)\t[1,501)\t>=501\tFile"
    assert len(lines) == 5 and lines[1].startswith("0\t") and lines[1].endswith("\tf0000.bed")
    assert lines[4].startswith("Any dataset within 500 bp: ") and lines[4].count("\t") == 5
    got = _run(["search", db.path, "-q", beds[0], "-N", "500", "-H", "7"], HOST)
    assert got.stdout.decode().splitlines()[0] == "index\tn_within\t<7\t>=7\tFile"


BAD_LISTS = ["", ",", "0,", ",0", "abc", "1x", "1,2,x", "0.5", "1e3", " 1", "+1", "1, 2", "1,1", "2,1", "0,5,5", "2147483648", "-2147483649",
             "99999999999999999999", ",".join(str(i) for i in range(64))]


@pytest.mark.parametrize("bad", BAD_LISTS, ids=lambda b: "list:" + b[:24])
def test_a_bad_edge_list_is_a_usage_error(bad, tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 9300, nbeds=1)
    lst = _write_list(tmp, beds)
    for sel in (["-q", beds[0]], ["-Q", lst]):
        for args in (sel + ["-N", "100", "-H", bad], ["-H", bad, "-N", "100"] + sel):
            got = _run(["search", db.path] + args, HOST)
            assert got.returncode == 64 and got.stdout.startswith(b"Not supported: -H " + bad.encode() + b" (") and got.stdout.count(b"\n") == 1, args


def test_the_other_refusals_and_the_limits(tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 9400, nbeds=1)
    gen = os.path.join(tmp, "genome.txt")
    open(gen, "w").write("chr1\t1000000\n")
    q = ["-q", beds[0]]
    for args, msg in ((q + ["-H", "0,1"], b"Not supported: -H without -N\n"),
                      (["-H", "0,1"], b"Not supported: -H without -N\n"),
                      (q + ["-N", "100", "-H"], b"Not supported: -H without a list of edges\n"),
                      (q + ["-N", "100", "-H", "0,1", "-P", "5", "-g", gen], b"Not supported: -H together with -P or -D\n"),
                      (q + ["-H", "0,1", "-P", "5", "-g", gen, "-D", "100"], b"Not supported: -H without -N\n"),
                      (q + ["-N", "100", "-H", "0,1", "-P", "5", "-g", gen, "-D", "100"], b"Not supported: -H together with -P or -D\n"),
                      (q + ["-N", "100", "-H", "0,1", "-D", "100"], b"Not supported: -H together with -P or -D\n")):
        got = _run(["search", db.path] + args, HOST)
        assert got.returncode == 64 and got.stdout == msg, args
    # what -N refuses, it refuses with -H too (its own message and exit code)
    got = _run(["search", db.path] + q + ["-N", "100", "-H", "0,1", "-u"], HOST)
    assert got.returncode == 0 and got.stdout.startswith(b"Not supported: -N together with")
    got = _run(["search", db.path] + q + ["-N", "-5", "-H", "0,1"], HOST)
    assert got.returncode == 0 and got.stdout.startswith(b"Not supported: -N -5 (")
    # the list is taken as the next argument even when it begins with '-'; 63 edges and the ends of int32 are accepted
    for ok in ("-5", "-2147483648", "2147483647", "-2147483648,2147483647", ",".join(str(i) for i in range(-31, 32))):
        got = _run(["search", db.path] + q + ["-N", "100", "-H", ok], HOST)
        assert got.returncode == 0 and got.stdout.startswith(b"index\tn_within\t<" + ok.split(",")[0].encode()), ok


def test_engine_route_without_a_device_fails_loudly(tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 9500, nbeds=1)
    nodev = {"IGD_HOST_MAX_QUERIES": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
    got = _run(["search", db.path, "-q", beds[0], "-N", "100", "-H", "0,1"], nodev)
    assert got.returncode == 69 and b"no CPU search path" in got.stderr and got.stdout == b""


def test_command_lines_without_h_print_what_they_printed(tmp):
    """-N alone still prints -N's table (tests/test_nearest_cli.py holds it byte for byte; here: the same bytes beside a -H run)"""
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 4, 2, 8, 9600, nbeds=2)
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
