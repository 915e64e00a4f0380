"""`igd search ... -U universe -X`: the enrichment table of the sets restricted to the universe, on the host route.

Expected values never come from the code under test: R_k from restrict_ref.join over the lines as the oracle reads them,
the membership of the universe from the oracle one region at a time, supports, sizes and tables from the definitions, the
statistics from exact arithmetic (fisher_ref.py); with -R the six columns from rank_ref.py over the full-precision
statistics of fisher_host.  Without -X every command line prints what it printed; -X without -U is refused."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import fisher_ref as FR
import rank_ref as KR
import restrict_ref as RR
from helpers import GOLDEN, Oracle, short_tmpdir
from test_enrich_host import HEADER, _universe_for_case, enrich_fixture
from test_membership_host import oracle_member
from test_rank_cli import EXTRA
from test_sets_cli import EXE, _case_files, _write_list
from test_support_host import HOST, _index, _run

REFUSED = "Not supported: -X without -U\n"


@pytest.fixture
def tmp():
    d = short_tmpdir("irc")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def expected(db, orc, files, ufile, v):
    """per file of the list: (rows [(index, nr, a, b, c, d, odds, plog, name)], last line, full tables of the set)"""
    import igd_amd
    q = []
    for p in files:
        try:
            q.append(orc.read_queries(p))
        except IOError:
            q.append(tuple(np.zeros(0, np.int32) for _ in range(3)))
    off = np.zeros(len(q) + 1, np.int64)
    off[1:] = np.cumsum([len(s[1]) for s in q])
    cat = tuple(np.concatenate([s[i] for s in q]).astype(np.int32) for i in range(3))
    u = orc.read_queries(ufile)
    nu = len(u[1])
    R = RR.join(*cat, off, *u)
    member, _ = oracle_member(orc, *u, v)
    sup, usup, nhit, _ = RR.gather(R, member)
    size = R.sum(axis=1)
    b, c, d = RR.tables(sup, usup, size, nu)
    assert (b >= 0).all() and (c >= 0).all() and (d >= 0).all()
    out = []
    for k in range(len(q)):
        rows = []
        for i, (nr, name) in enumerate(_index(db)):
            if sup[k, i] > 0:
                t = (int(sup[k, i]), int(b[k, i]), int(c[k, i]), int(d[k, i]))
                rows.append((i, nr) + t + (FR.odds(*t), FR.exact_plog(*t), name))
        last = "Restricted regions with a hit: %d of %d (from %d query regions); universe regions: %d" % (nhit[k], size[k], len(q[k][1]), nu)
        plog, odds = igd_amd.fisher_host(sup[k], b[k], c[k], d[k])
        out.append((rows, last, KR.reference(sup[k][None, :], plog[None, :], odds[None, :]), int(size[k]), len(q[k][1])))
    return out


def compare_block(lines, want, ranked, what):
    """one printed block (header .. last line) against the expectation; returns the lines that follow it"""
    rows, last, ranks, _, _ = want
    assert lines[0] == HEADER + (EXTRA if ranked else ""), (what, lines[0])
    for k, w in enumerate(rows):
        f = lines[1 + k].split("\t")
        assert len(f) == (15 if ranked else 9), (what, lines[1 + k])
        assert [int(x) for x in f[:6]] == list(w[:6]) and f[8] == w[8], (what, f, w)
        if math.isinf(w[6]) or math.isnan(w[6]):
            assert f[6] == ("inf" if math.isinf(w[6]) else "nan"), (what, f, w)
        else:
            assert len(f[6].split(".")[-1]) == 4 and abs(float(f[6]) - w[6]) <= 5e-5 + 1e-15 * abs(w[6]), (what, f, w)
        assert abs(float(f[7]) - w[7]) <= 5e-5 + FR.tol(*w[2:6], w[7]), (what, f, w)
        if ranked:
            i = w[0]
            assert [int(x) for x in f[9:13]] == [int(r[0, i]) for r in (ranks.rnk_sup, ranks.rnk_pv, ranks.rnk_or, ranks.max_rnk)], (what, f)
            assert f[13] == "%.2f" % ranks.mean_rnk[0, i], (what, f)
            assert abs(float(f[14]) - ranks.qvalue_log[0, i]) <= 5e-5 + KR.tol(ranks.qvalue_log[0, i]), (what, f)
    assert lines[1 + len(rows)] == last, (what, lines[1 + len(rows)], last)
    return lines[2 + len(rows):]


def check_cli(db, files, ufile, extra, tmp):
    v = int(extra[1]) if extra else 0
    orc = Oracle(db)
    try:
        files = files + [os.path.join(tmp, "missing.bed")]
        want = expected(db, orc, files, ufile, v)
    finally:
        orc.close()
    lst = _write_list(tmp, files)
    for ranks in ([], ["-R"]):
        for args in (["-q", files[0], "-U", ufile, "-X"], ["-X", "-U", ufile, "-q", files[0]]):
            got = _run(["search", db] + args + ranks + extra, HOST)
            assert got.returncode == 0, got.stderr
            assert compare_block(got.stdout.decode().splitlines(), want[0], bool(ranks), args) == []
        got = _run(["search", db, "-Q", lst, "-X", "-U", ufile] + ranks + extra, HOST)
        assert got.returncode == 0, got.stderr
        lines = got.stdout.decode().splitlines()
        for k, p in enumerate(files):
            assert lines[0] == "Query set %d: %s" % (k, p)
            lines = compare_block(lines[1:], want[k], bool(ranks), (k, p))
        assert lines == []
    return want


@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("edge", [])])
def test_X_on_the_golden_families(case, extra, tmp):
    db = os.path.join(GOLDEN, case, "db.igd")
    want = check_cli(db, _case_files(case), _universe_for_case(case, tmp), extra, tmp)
    assert any(rows for rows, _, _, _, _ in want), "no row at all: the fixture is vacuous"
    assert any(size != n for _, _, _, size, n in want), "the restriction changes no set: the fixture is vacuous"


@pytest.mark.parametrize("extra", [[], ["-v", "400"]])
def test_X_on_an_engineered_database(extra, tmp):
    db, upath, sets, _ = enrich_fixture(tmp)
    want = check_cli(db, sets, upath, extra, tmp)
    rows = [r for block, _, _, _, _ in want for r in block]
    assert any(r[7] > 2 for r in rows), "no row with pValueLog > 2"
    assert want[1][3] < want[1][4], "set 1 has no region outside the universe"
    assert any(0 < len(block) < 6 for block, _, _, _, _ in want), "no file left out for a = 0"
    # the unrestricted table of the same sets clamps cells; the restricted one has none to clamp
    plain = _run(["search", db, "-q", sets[1], "-U", upath] + extra, HOST).stdout.decode()
    assert "clamped cells: 0" not in plain.splitlines()[-1] and plain.splitlines()[-1].startswith("Query regions with a hit:")


def test_X_without_U_is_refused_and_U_alone_is_unchanged(tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    lst = _write_list(tmp, _case_files("branch"))
    for args in (["-q", q, "-X"], ["-X", "-q", q], ["-Q", lst, "-X"], ["-q", q, "-u", "-X"], ["-X", "-m"]):
        got = _run(["search", db] + args, HOST)
        assert got.returncode == 0 and got.stdout.decode() == REFUSED, args
    # -R's refusal comes first, -U's own conflicts hold with -X too
    assert _run(["search", db, "-q", q, "-X", "-R"], HOST).stdout.decode() == "Not supported: -R without -U\n"
    got = _run(["search", db, "-q", q, "-U", q, "-b", "-X"], HOST)
    assert got.stdout.decode() == "Not supported: -U together with -b, -w, -f, -m, -s or -r\n"
    # -U alone: the unrestricted table and its last line
    got = _run(["search", db, "-q", q, "-U", q], HOST).stdout.decode()
    assert got.startswith(HEADER + "\n") and "Restricted" not in got and "clamped cells: " in got.splitlines()[-1]
    usage = subprocess.run([EXE, "search"], stderr=subprocess.PIPE, stdout=subprocess.PIPE).stderr.decode()
    assert "    -X   " in usage and "-U <universe file>" in usage and "    -R   " in usage
