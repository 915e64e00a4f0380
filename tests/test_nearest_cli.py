"""`igd search db.igd -q regions.bed -N <bp> [-v V]` and `-Q list.txt -N <bp>` on the host route, byte for byte against a table
formatted from tests/nearest_ref.py (the definition over the interval lists this test wrote; the BED files are read by the
oracle's reader, as the other command-line tests read them); every refusal; a command line without -N unchanged."""
import os
import random
import shutil

import numpy as np
import pytest

from helpers import Oracle, short_tmpdir, write_bed
from nearest_ref import MAX_WINDOW, ListDb, clustered_lists, mixed_regions, ref_rows, ref_sets, table_text
from test_golden_oracle import materialize
from test_sets_cli import _write_list
from test_support_host import HOST, _run


@pytest.fixture
def tmp():
    d = short_tmpdir("inc")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _db_and_beds(tmp, nbp, gtype, nfiles, nctg, span_tiles, seed, nbeds=3):
    rng = random.Random(seed)
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    db = ListDb(tmp, "db", files, nbp, gtype)
    beds = []
    for k in range(nbeds):
        ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 150 + 40 * k)
        rows = [(db.ctgs[c] if 0 <= c < nctg else "chrNotThere", s, e) for c, s, e in zip(ichr.tolist(), qs.tolist(), qe.tolist()) if s >= 0]
        p = os.path.join(tmp, "q%d.bed" % k)
        write_bed(p, rows)
        beds.append(p)
    return db, beds


def expected_block(db, orc, qfile, window, v):
    try:
        ichr, qs, qe = orc.read_queries(qfile)
    except IOError:
        ichr = qs = qe = np.zeros(0, np.int32)
    dist, dmin = ref_rows(db, ichr, qs, qe, window, v if v > 0 else None)
    nw, no, sd = ref_sets(dist, dmin, np.array([0, len(qs)], np.int64))
    return table_text(db.names, nw[0], no[0], sd[0], window, len(qs)), nw[0]


@pytest.mark.parametrize("nbp,gtype,nfiles,nctg,span_tiles", [(1 << 14, 1, 7, 2, 10), (1 << 12, 0, 5, 3, 30), (1000, 1, 6, 2, 40)])
def test_cli_n_prints_the_definitions_table_on_the_host_route(nbp, gtype, nfiles, nctg, span_tiles, tmp):
    db, beds = _db_and_beds(tmp, nbp, gtype, nfiles, nctg, span_tiles, 6100 + nfiles)
    orc = Oracle(db.path)
    try:
        assert orc.ctg_names() == db.ctgs
        some_na = some_far = False
        for W in (0, 1, nbp, 3 * nbp + 5, MAX_WINDOW):
            for v in (0, 500):
                extra = ["-v", str(v)] if v else []
                want, nw = expected_block(db, orc, beds[0], W, v)
                some_na |= "\tNA\t" in want
                some_far |= W > 0 and any(float(l.split("\t")[3]) > 0 for l in want.splitlines()[1:-1] if l.split("\t")[3] != "NA")
                for args in (["-q", beds[0], "-N", str(W)] + extra, ["-N", str(W)] + extra + ["-q", beds[0]]):
                    got = _run(["search", db.path] + args, HOST)
                    assert got.returncode == 0, got.stderr
                    assert got.stdout.decode() == want, args
        assert some_far, "fixture is vacuous: every mean distance is 0"
        # -Q: one block per file, laid out as -u's; an unreadable file is an empty set
        files = beds + [os.path.join(tmp, "missing.bed")]
        lst = _write_list(tmp, files, crlf=True)
        for W, v in ((nbp, 0), (700, 500), (0, 0)):
            got = _run(["search", db.path, "-Q", lst, "-N", str(W)] + (["-v", str(v)] if v else []), HOST)
            assert got.returncode == 0, got.stderr
            want = "".join("Query set %d: %s\n" % (k, p) + expected_block(db, orc, p, W, v)[0] for k, p in enumerate(files))
            assert got.stdout.decode() == want, (W, v)
            assert want.endswith("Regions with a dataset within %d bp: 0 of 0; overlapping: 0; mean distance NA\n" % W)
            assert "\tNA\t" in want
    finally:
        orc.close()


REFUSED = [["-u"], ["-b"], ["-w"], ["-U", "UNI"], ["-U", "UNI", "-R"], ["-U", "UNI", "-X"], ["-R"], ["-X"], ["-C"], ["-P", "5", "-g", "GEN"],
           ["-P", "5"], ["-f"], ["-m"], ["-s"], ["-r", "chr1", "1000", "90000"], ["-O", "5"], ["-A", "0.5"], ["-B", "0.25"]]


@pytest.mark.parametrize("other", REFUSED, ids=lambda o: "".join(o))
def test_n_together_with_another_selector_is_not_supported(other, tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 6200, nbeds=1)
    gen = os.path.join(tmp, "genome.txt")
    open(gen, "w").write("chr1\t1000000\n")
    other = [beds[0] if a == "UNI" else gen if a == "GEN" else a for a in other]
    lst = _write_list(tmp, beds)
    for sel in (["-q", beds[0]], ["-Q", lst]):
        for args in (sel + ["-N", "100"] + other, other + ["-N", "100"] + sel):
            got = _run(["search", db.path] + args, HOST)
            assert got.returncode == 0 and got.stdout.startswith(b"Not supported: -N together with") and got.stdout.count(b"\n") == 1, args


@pytest.mark.parametrize("bad", ["-1", "-5000", "abc", "12x", "", "1073741825", "99999999999999999999", "1e3", "0.5"])
def test_a_bad_window_is_not_supported(bad, tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 6300, nbeds=1)
    lst = _write_list(tmp, beds)
    for sel in (["-q", beds[0]], ["-Q", lst]):
        for args in (sel + ["-N", bad], ["-N", bad] + sel):
            got = _run(["search", db.path] + args, HOST)
            assert got.returncode == 0 and got.stdout.startswith(b"Not supported: -N " + bad.encode() + b" (") and got.stdout.count(b"\n") == 1, args
    got = _run(["search", db.path, "-q", beds[0], "-N"], HOST)
    assert got.returncode == 0 and got.stdout == b"No window.\n"
    got = _run(["search", db.path, "-N", "100"], HOST)
    assert got.returncode == 0 and got.stdout == b"Not supported: -N without -q or -Q\n"
    # the largest window is accepted
    got = _run(["search", db.path, "-q", beds[0], "-N", str(MAX_WINDOW)], HOST)
    assert got.returncode == 0 and got.stdout.startswith(b"index\tn_within\t")


def test_engine_route_without_a_device_fails_loudly(tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 6400, nbeds=1)
    nodev = {"IGD_HOST_MAX_QUERIES": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
    lst = _write_list(tmp, beds)
    for args in (["-q", beds[0], "-N", "100"], ["-Q", lst, "-N", "100", "-v", "500"]):
        got = _run(["search", db.path] + args, nodev)
        assert got.returncode == 69 and b"no CPU search path" in got.stderr, args
        assert got.stdout == b"", args


@pytest.mark.parametrize("case", ["branch", "gtype0", "edge"])
def test_command_lines_without_n_print_what_they_printed(case):
    """the golden families' stdout files were written by the reference binary: -q, -q -v, -r and -f print them still"""
    d, dst, man = materialize(case)
    try:
        ran = 0
        for run in man["runs"]:
            if "-m" in run["args"] or "-N" in run["args"]:
                continue
            args = [os.path.join(dst, a) if a in ("db.igd", "q.bed", "q.bed.gz", "q100.bed") else a for a in run["args"]]
            got = _run(args, HOST)
            assert got.returncode == 0 and got.stdout.decode() == open(os.path.join(dst, run["stdout"])).read(), run["args"]
            ran += 1
        assert ran >= 3
    finally:
        shutil.rmtree(d, ignore_errors=True)
