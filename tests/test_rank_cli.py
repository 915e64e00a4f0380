"""`igd search ... -U universe -R`: the six rank and q-value columns behind the enrichment table, on the host route.
The expected columns come from rank_ref.py over ALL files of the set: the printed files' tables (a, b, c, d are printed
exactly) and, for the files left out because a = 0, the table that follows from the universe's support; pValueLog and
oddsRatio of the tables in full precision from fisher_host (the printed %.4f would tie values that differ).  Without -R the
output is what it was; -R without -U is refused."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rank_ref as R
from helpers import GOLDEN, Oracle, short_tmpdir
from test_enrich_host import HEADER, _universe_for_case, enrich_fixture, universe_of
from test_sets_cli import EXE, _case_files, _write_list
from test_support_host import HOST, _run

EXTRA = "\t rnkSup\t rnkPV\t rnkOR\t maxRnk\t meanRnk\t qValueLog"
REFUSED = "Not supported: -R without -U\n"


@pytest.fixture
def tmp():
    d = short_tmpdir("irk")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def blocks(text):
    """[(header, [table lines], last line)] of a -U output, with or without 'Query set' lines"""
    out, lines = [], [l for l in text.splitlines() if not l.startswith("Query set ")]
    i = 0
    while i < len(lines):
        j = i + 1
        while not lines[j].startswith("Query regions with a hit:"):
            j += 1
        out.append((lines[i], lines[i + 1:j], lines[j]))
        i = j + 1
    return out


def check_block(plain, ranked, usup, what):
    import igd_amd
    assert plain[0] == HEADER and ranked[0] == HEADER + EXTRA, what
    assert ranked[2] == plain[2] and len(ranked[1]) == len(plain[1]), what
    nk, nu = int(plain[2].split(" of ")[1].split(";")[0]), int(plain[2].split("universe regions: ")[1].split(";")[0])
    nf = len(usup)
    a = np.zeros(nf, np.int64)
    b, c = usup.astype(np.int64).copy(), np.full(nf, nk, np.int64)
    d = np.maximum(nu - b - c, 0)
    for l in plain[1]:
        f = l.split("\t")
        a[int(f[0])], b[int(f[0])], c[int(f[0])], d[int(f[0])] = (int(x) for x in f[2:6])
    plog, odds = igd_amd.fisher_host(a, b, c, d)
    want = R.reference(a[None, :], plog[None, :], odds[None, :])
    for lp, lr in zip(plain[1], ranked[1]):
        f = lr.split("\t")
        assert len(f) == 15 and "\t".join(f[:9]) == lp, (what, lr)                   # the line of -U, six fields more
        i = int(f[0])
        assert [int(x) for x in f[9:13]] == [int(w[0, i]) for w in (want.rnk_sup, want.rnk_pv, want.rnk_or, want.max_rnk)], (what, lr)
        assert f[13] == "%.2f" % want.mean_rnk[0, i], (what, lr)
        assert len(f[14].split(".")[-1]) == 4 and abs(float(f[14]) - want.qvalue_log[0, i]) <= 5e-5 + R.tol(want.qvalue_log[0, i]), (what, lr)
    return len(plain[1]), nf


def check_cli(db, files, ufile, extra, tmp):
    orc = Oracle(db)
    try:
        usup, _ = universe_of(orc, ufile, int(extra[1]) if extra else 0)
    finally:
        orc.close()
    lst = _write_list(tmp, files)
    seen = []
    for args in (["-q", files[0], "-U", ufile], ["-Q", lst, "-U", ufile]):
        plain = _run(["search", db] + args + extra, HOST)
        assert plain.returncode == 0, plain.stderr
        for rargs in (args + ["-R"] + extra, ["-R"] + extra + args):
            ranked = _run(["search", db] + rargs, HOST)
            assert ranked.returncode == 0, ranked.stderr
            bp, br = blocks(plain.stdout.decode()), blocks(ranked.stdout.decode())
            assert len(bp) == len(br) == (1 if "-q" in args else len(files))
            assert [l for l in ranked.stdout.decode().splitlines() if l.startswith("Query set ")] == \
                   [l for l in plain.stdout.decode().splitlines() if l.startswith("Query set ")]
            seen += [check_block(p, r, usup, rargs) for p, r in zip(bp, br)]
    return seen


@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("edge", [])])
def test_R_on_the_golden_families(case, extra, tmp):
    db = os.path.join(GOLDEN, case, "db.igd")
    seen = check_cli(db, _case_files(case), _universe_for_case(case, tmp), extra, tmp)
    assert any(n > 1 for n, _ in seen), "no block with two printed files: the fixture is vacuous"


def test_R_on_an_engineered_database_with_files_left_out(tmp):
    db, upath, sets, _ = enrich_fixture(tmp)
    seen = check_cli(db, sets, upath, [], tmp)
    assert any(0 < n < nf for n, nf in seen), "no block with a file left out for a = 0"


def test_R_without_U_is_refused_and_U_alone_is_unchanged(tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    lst = _write_list(tmp, _case_files("branch"))
    for args in (["-q", q, "-R"], ["-R", "-q", q], ["-Q", lst, "-R"], ["-q", q, "-u", "-R"], ["-q", q, "-f", "-R"], ["-R", "-m"]):
        got = _run(["search", db] + args, HOST)
        assert got.returncode == 0 and got.stdout.decode() == REFUSED, args
    # -U alone: the header and every line of nine fields, nothing of -R's
    got = _run(["search", db, "-q", q, "-U", q], HOST).stdout.decode()
    assert got.startswith(HEADER + "\n") and "rnk" not in got
    assert all(len(l.split("\t")) == 9 for l in got.splitlines()[1:-1])
    # -U's own refusals come first, as before
    got = _run(["search", db, "-q", q, "-U", q, "-b", "-R"], HOST)
    assert got.stdout.decode() == "Not supported: -U together with -b, -w, -f, -m, -s or -r\n"
    usage = subprocess.run([EXE, "search"], stderr=subprocess.PIPE, stdout=subprocess.PIPE).stderr.decode()
    assert "    -R   " in usage and "-U <universe file>" in usage
