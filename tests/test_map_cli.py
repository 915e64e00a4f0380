"""`igd search db.igd -q regions.bed -V count|sum|min|max|mean [-v V]` and `-Q list.txt -V <op>` on the host route, byte for byte
against a table formatted from tests/map_ref.py (the definition over the interval lists this test wrote; the BED files are read
by the oracle's reader, as the other command-line tests read them); every refusal and its exit code; a command line without -V
unchanged."""
import os
import random
import shutil

import numpy as np
import pytest

from helpers import Oracle, short_tmpdir, write_bed
from map_ref import ListDb, clustered_lists, mixed_regions, ref_rows, ref_sets, table_text
from test_golden_oracle import materialize
from test_sets_cli import _write_list
from test_support_host import HOST, _run

EX_USAGE = 64
CLI_OPS = ("count", "sum", "min", "max", "mean")


@pytest.fixture
def tmp():
    d = short_tmpdir("imc")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _db_and_beds(tmp, nbp, gtype, nfiles, nctg, span_tiles, seed, nbeds=3):
    rng = random.Random(seed)
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles, min_value=-300)
    files.append([])                                                      # a dataset nobody overlaps: NA, and "n of nFiles"
    db = ListDb(tmp, "db", files, nbp, gtype)
    beds = []
    for k in range(nbeds):
        ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 150 + 40 * k)
        rows = [(db.ctgs[c] if 0 <= c < nctg else "chrNotThere", s, e) for c, s, e in zip(ichr.tolist(), qs.tolist(), qe.tolist()) if s >= 0]
        p = os.path.join(tmp, "q%d.bed" % k)
        write_bed(p, rows)
        beds.append(p)
    return db, beds


def expected_block(db, orc, qfile, op, v):
    try:
        ichr, qs, qe = orc.read_queries(qfile)
    except IOError:
        ichr = qs = qe = np.zeros(0, np.int32)
    count, agg = ref_rows(db, ichr, qs, qe, "sum" if op == "mean" else op, v if v > 0 else None)
    nh, npairs, sa = ref_sets(count, agg, np.array([0, len(qs)], np.int64))
    return table_text(db.names, nh[0], npairs[0], sa[0], op)


@pytest.mark.parametrize("nbp,gtype,nfiles,nctg,span_tiles", [(1 << 14, 1, 7, 2, 10), (1 << 12, 0, 5, 3, 30), (1000, 1, 6, 2, 40)])
def test_cli_v_prints_the_definitions_table_on_the_host_route(nbp, gtype, nfiles, nctg, span_tiles, tmp):
    db, beds = _db_and_beds(tmp, nbp, gtype, nfiles, nctg, span_tiles, 9100 + nfiles)
    orc = Oracle(db.path)
    try:
        assert orc.ctg_names() == db.ctgs
        ops = CLI_OPS if gtype == 1 else ("count",)
        negative = False
        for op in ops:
            for v in (0, 500):
                extra = ["-v", str(v)] if v else []
                want = expected_block(db, orc, beds[0], op, v)
                assert "\tNA\t" in want and want.startswith("index\tn_hit\tpairs\tmean_%s\tFile\n" % op)
                negative |= "\t-" in want
                for args in (["-q", beds[0], "-V", op] + extra, ["-V", op] + extra + ["-q", beds[0]]):
                    got = _run(["search", db.path] + args, HOST)
                    assert got.returncode == 0, got.stderr
                    assert got.stdout.decode() == want, args
        assert negative == (gtype == 1), "fixture is vacuous: no negative mean"
        # -Q: one block per file, laid out as -u's; an unreadable file is an empty set
        files = beds + [os.path.join(tmp, "missing.bed")]
        lst = _write_list(tmp, files, crlf=True)
        for op, v in ((ops[-1], 0), (ops[0], 500), (ops[len(ops) // 2], 0)):
            got = _run(["search", db.path, "-Q", lst, "-V", op] + (["-v", str(v)] if v else []), HOST)
            assert got.returncode == 0, got.stderr
            want = "".join("Query set %d: %s\n" % (k, p) + expected_block(db, orc, p, op, v) for k, p in enumerate(files))
            assert got.stdout.decode() == want, (op, v)
            assert want.endswith("Pairs: 0; datasets with a hit: 0 of %d\n" % (nfiles + 1))
    finally:
        orc.close()


REFUSED = [["-u"], ["-b"], ["-w"], ["-U", "UNI"], ["-U", "UNI", "-R"], ["-U", "UNI", "-X"], ["-R"], ["-X"], ["-C"], ["-P", "5", "-g", "GEN"],
           ["-P", "5"], ["-P", "5", "-g", "GEN", "-D", "100"], ["-D", "100"], ["-N", "100"], ["-f"], ["-m"], ["-s"],
           ["-r", "chr1", "1000", "90000"], ["-O", "5"], ["-A", "0.5"], ["-B", "0.25"]]


@pytest.mark.parametrize("other", REFUSED, ids=lambda o: "".join(o))
def test_v_together_with_another_selector_is_a_usage_error(other, tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 9200, nbeds=1)
    gen = os.path.join(tmp, "genome.txt")
    open(gen, "w").write("chr1\t1000000\n")
    other = [beds[0] if a == "UNI" else gen if a == "GEN" else a for a in other]
    lst = _write_list(tmp, beds)
    for sel in (["-q", beds[0]], ["-Q", lst]):
        for args in (sel + ["-V", "sum"] + other, other + ["-V", "sum"] + sel):
            got = _run(["search", db.path] + args, HOST)
            assert got.returncode == EX_USAGE, (args, got.stdout)
            assert got.stdout.startswith(b"Not supported: -V together with") and got.stdout.count(b"\n") == 1, args


def test_the_other_refusals_and_their_exit_code(tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 9300, nbeds=1)
    lst = _write_list(tmp, beds)
    for bad in ("median", "SUM", "", "5", "count,sum"):
        for sel in (["-q", beds[0]], ["-Q", lst]):
            for args in (sel + ["-V", bad], ["-V", bad] + sel):
                got = _run(["search", db.path] + args, HOST)
                assert got.returncode == EX_USAGE and got.stdout.startswith(b"Not supported: -V " + bad.encode() + b" (") and \
                    got.stdout.count(b"\n") == 1, args
    got = _run(["search", db.path, "-q", beds[0], "-V"], HOST)
    assert got.returncode == EX_USAGE and got.stdout.startswith(b"Not supported: -V without an op")
    got = _run(["search", db.path, "-V", "sum"], HOST)
    assert got.returncode == EX_USAGE and got.stdout == b"Not supported: -V without -q or -Q\n"
    # a database without values: count is answered, the value ops are usage errors
    d0 = os.path.join(tmp, "g0")
    os.makedirs(d0)
    db0, beds0 = _db_and_beds(d0, 1 << 12, 0, 3, 1, 6, 9301, nbeds=1)
    for op in ("sum", "min", "max", "mean"):
        got = _run(["search", db0.path, "-q", beds0[0], "-V", op], HOST)
        assert got.returncode == EX_USAGE and got.stdout.startswith(b"Not supported: -V " + op.encode() + b" on a database without values"), op
    got = _run(["search", db0.path, "-q", beds0[0], "-V", "count", "-v", "500"], HOST)
    assert got.returncode == 0 and got.stdout.startswith(b"index\tn_hit\tpairs\tmean_count\tFile\n")


def test_engine_route_without_a_device_fails_loudly(tmp):
    db, beds = _db_and_beds(tmp, 1 << 12, 1, 3, 1, 6, 9400, nbeds=1)
    nodev = {"IGD_HOST_MAX_QUERIES": "0", "HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}
    lst = _write_list(tmp, beds)
    for args in (["-q", beds[0], "-V", "sum"], ["-Q", lst, "-V", "count", "-v", "500"]):
        got = _run(["search", db.path] + args, nodev)
        assert got.returncode == 69 and b"no CPU search path" in got.stderr, args
        assert got.stdout == b"", args


@pytest.mark.parametrize("case", ["branch"])
def test_command_lines_without_v_print_what_they_printed(case):
    """the golden family's stdout files were written by the reference binary: -q, -q -v, -r and -f print them still"""
    d, dst, man = materialize(case)
    try:
        ran = 0
        for run in man["runs"]:
            if "-m" in run["args"] or "-V" in run["args"]:
                continue
            args = [os.path.join(dst, a) if a in ("db.igd", "q.bed", "q.bed.gz", "q100.bed") else a for a in run["args"]]
            got = _run(args, HOST)
            assert got.returncode == 0 and got.stdout.decode() == open(os.path.join(dst, run["stdout"])).read(), run["args"]
            ran += 1
        assert ran >= 3
    finally:
        shutil.rmtree(d, ignore_errors=True)
