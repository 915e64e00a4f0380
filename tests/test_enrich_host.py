"""Region-set enrichment without a GPU: `igd search db -q F -U universe` / `-Q list -U universe` on the host route
(igdc_support_host for the sets and the universe, igdc_fisher_host for the statistics).

Per set k (n_k accepted lines), universe (n_U accepted lines) and file f, with the supports of `-u`:
    a = support[k][f]   b = u[f] - a   c = n_k - a   d = n_U - a - b - c;   a negative b or d is 0 and counts as clamped
    pValueLog = -log10 P(X >= a), X ~ Hypergeometric(a+b+c+d, a+b, a+c);   oddsRatio = (a d) / (b c)

Expected a and u come from the CPU oracle one query at a time (test_support_host.oracle_support), b, c, d and the clamp
count from the definitions, the statistics from exact arithmetic (fisher_ref.py).  The printed %.4f fields are compared as
numbers, to 5e-5 + the Fisher bound."""
import math
import os
import random
import shutil

import numpy as np
import pytest

import fisher_ref as R
from helpers import GOLDEN, Oracle, short_tmpdir, write_bed, write_igd_numpy
from test_golden_oracle import CASES
from test_sets_cli import _case_files, _write_list
from test_support_host import HOST, _index, _run, oracle_support

HEADER = "index\t number of regions\t support\t b\t c\t d\t oddsRatio\t pValueLog\t File_name"
CONFLICT = "Not supported: -U together with -b, -w, -f, -m, -s or -r\n"
_memo = {}


@pytest.fixture
def tmp():
    d = short_tmpdir("ien")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def tables_from_supports(sup, usup, nk, nu):
    """(b, c, d, clamped) of one set from the definitions"""
    b = usup - sup
    c = nk - sup
    d = nu - sup - b - c
    return np.maximum(b, 0), c, np.maximum(d, 0), int(((b < 0) | (d < 0)).sum())


def expected_block(db, orc, qfile, uni, v):
    """what `-q qfile -U universe` prints: (rows [(index, nr, a, b, c, d, odds, plog, name)], last line)"""
    try:
        ichr, qs, qe = orc.read_queries(qfile)
    except IOError:
        ichr = qs = qe = np.zeros(0, np.int32)
    sup, nhit, _ = oracle_support(orc, ichr, qs, qe, v)
    usup, nu = uni
    b, c, d, clamped = tables_from_supports(sup, usup, len(qs), nu)
    rows = []
    for i, (nr, name) in enumerate(_index(db)):
        if sup[i] > 0:
            t = (int(sup[i]), int(b[i]), int(c[i]), int(d[i]))
            if t not in _memo:
                _memo[t] = R.exact_plog(*t)
            rows.append((i, nr) + t + (R.odds(*t), _memo[t], name))
    return rows, "Query regions with a hit: %d of %d; universe regions: %d; clamped cells: %d" % (nhit, len(qs), nu, clamped)


def compare_block(lines, rows, last, what):
    """one printed block (header .. last line) against the expected rows; returns the lines that follow it"""
    assert lines[0] == HEADER, (what, lines[0])
    for k, w in enumerate(rows):
        f = lines[1 + k].split("\t")
        assert len(f) == 9, (what, lines[1 + k])
        assert [int(x) for x in f[:6]] == list(w[:6]) and f[8] == w[8], (what, f, w)
        assert len(f[6].split(".")[-1]) == 4 or f[6] in ("inf", "nan"), f[6]           # %.4f
        o, p = float(f[6]), float(f[7])
        if math.isinf(w[6]) or math.isnan(w[6]):
            assert f[6] == ("inf" if math.isinf(w[6]) else "nan"), (what, f, w)
        else:
            assert abs(o - w[6]) <= 5e-5 + 1e-15 * abs(w[6]), (what, f, w)
        assert abs(p - w[7]) <= 5e-5 + R.tol(*w[2:6], w[7]), (what, f, w)
    assert lines[1 + len(rows)] == last, (what, lines[1 + len(rows)], last)
    return lines[2 + len(rows):]


def universe_of(orc, ufile, v):
    ichr, qs, qe = orc.read_queries(ufile)
    usup, _, _ = oracle_support(orc, ichr, qs, qe, v)
    return usup, len(qs)


def check_cli(db, orc, files, ufile, extra, tmp, env=HOST):
    """-q on the first file, -Q on all of them and a missing one; returns every expected row"""
    v = int(extra[1]) if extra else 0
    uni = universe_of(orc, ufile, v)
    seen = []
    q = files[0]
    for args in (["-q", q, "-U", ufile] + extra, ["-U", ufile] + extra + ["-q", q], ["-u", "-q", q, "-U", ufile] + extra):
        got = _run(["search", db] + args, env)
        assert got.returncode == 0, got.stderr
        rows, last = expected_block(db, orc, q, uni, v)
        assert compare_block(got.stdout.decode().splitlines(), rows, last, args) == []
    files = files + [os.path.join(tmp, "missing.bed")]
    lst = _write_list(tmp, files, crlf=True)
    got = _run(["search", db, "-Q", lst, "-U", ufile] + extra, env)
    assert got.returncode == 0, got.stderr
    lines = got.stdout.decode().splitlines()
    for k, p in enumerate(files):
        assert lines[0] == "Query set %d: %s" % (k, p)
        rows, last = expected_block(db, orc, p, uni, v)
        lines = compare_block(lines[1:], rows, last, (k, p))
        seen.append((rows, last, uni))
    assert lines == []
    return seen


def _universe_for_case(case, tmp):
    """the case's query file and its database files' lines, every other one: most set regions are in it, some are not"""
    files = _case_files(case)
    lines = []
    for p in files:
        lines += [l for l in open(p).read().splitlines() if l.strip()]
    path = os.path.join(tmp, "universe.bed")
    with open(path, "w") as f:
        f.write("\n".join(lines[::2]) + "\n")
    return path


@pytest.mark.parametrize("case,extra", [("branch", []), ("branch", ["-v", "500"]), ("edge", [])])
def test_cli_U_on_the_golden_families(case, extra, tmp):
    assert case in CASES
    db = os.path.join(GOLDEN, case, "db.igd")
    orc = Oracle(db)
    try:
        seen = check_cli(db, orc, _case_files(case), _universe_for_case(case, tmp), extra, tmp)
        assert any(rows for rows, _, _ in seen), "no row at all: the fixture is vacuous"
    finally:
        orc.close()


def enrich_fixture(d, nfiles=6, name="en", nbp=1 << 11):
    """A database, a universe and three set files built so that the table is not vacuous:
       file 0 lies in the first twentieth of chr1 and set 0 is drawn from the universe's regions there (strong enrichment);
       file 1 lies in a stretch of chr1 the universe leaves out and set 1 has regions there (a > u: b is clamped);
       the last file lies on chr2, where the universe has regions and no set has any (a = 0: its row is left out);
       the files between are scattered.  Returns (db path, universe path, set paths, universe regions)."""
    rng = random.Random(5150 + nfiles)
    span = nbp * 200
    hole = (span // 2, span // 2 + span // 10)
    files = []
    for f in range(nfiles):
        rows = []
        if f == 0:
            for _ in range(120):
                s = rng.randrange(0, span // 20)
                rows.append(("chr1", s, s + rng.randint(50, 400), rng.randint(0, 1000)))
        elif f == 1:
            for _ in range(150):
                s = rng.randrange(hole[0], hole[1] - 500)
                rows.append(("chr1", s, s + rng.randint(50, 400), rng.randint(0, 1000)))
            for _ in range(10):
                s = rng.randrange(0, span)
                rows.append(("chr1", s, s + 300, rng.randint(0, 1000)))
        elif f == nfiles - 1:
            for _ in range(100):
                s = rng.randrange(0, span)
                rows.append(("chr2", s, s + rng.randint(50, 900), rng.randint(0, 1000)))
        else:
            for _ in range(rng.randint(150, 400)):
                s = rng.randrange(0, span)
                rows.append(("chr1", s, s + rng.choice([30, 200, 3 * nbp]), rng.randint(0, 1000)))
            rows.append(("chr2", 5, 50, 700))
        files.append(rows)
    db = os.path.join(d, name + ".igd")
    write_igd_numpy(db, files, nbp=nbp)
    uni = []
    for s in range(0, span, 160):
        if not (hole[0] - 200 <= s < hole[1]):
            uni.append(("chr1", s, s + 100))
    uni += [("chr2", s, s + 100) for s in range(0, span, 4000)]
    head = [r for r in uni if r[0] == "chr1" and r[1] < span // 20]
    rest = [r for r in uni if r[0] == "chr1" and r[1] >= span // 20]
    set0 = rng.sample(head, 60) + rng.sample(rest, 15)
    set1 = [("chr1", s, s + 150) for s in rng.sample(range(hole[0], hole[1] - 200), 40)] + rng.sample(rest, 50)
    set2 = rng.sample(rest, 300)
    upath = os.path.join(d, name + "_universe.bed")
    write_bed(upath, uni)
    sets = []
    for k, rows in enumerate((set0, set1, set2)):
        p = os.path.join(d, "%s_set%d.bed" % (name, k))
        write_bed(p, rows)
        sets.append(p)
    return db, upath, sets, uni


def assert_not_vacuous(seen, nfiles):
    rows = [r for block, _, _ in seen for r in block]
    assert any(r[7] > 2 for r in rows), "no row with pValueLog > 2"
    assert any("clamped cells: 0" not in last for _, last, _ in seen), "no clamped cell"
    assert any(r[3] == 0 and uni[0][r[0]] < r[2] for block, _, uni in seen for r in block), "no row whose b was clamped"
    assert any(len(block) < nfiles for block, _, _ in seen if block), "no file left out for a = 0"


@pytest.mark.parametrize("extra", [[], ["-v", "400"]])
def test_cli_U_on_an_engineered_database(extra, tmp):
    db, upath, sets, _ = enrich_fixture(tmp)
    orc = Oracle(db)
    try:
        seen = check_cli(db, orc, sets, upath, extra, tmp)
        assert_not_vacuous(seen, orc.nfiles)
    finally:
        orc.close()


def test_conflicts_and_bad_universes(tmp):
    db = os.path.join(GOLDEN, "branch", "db.igd")
    q = os.path.join(GOLDEN, "branch", "q.bed")
    lst = _write_list(tmp, _case_files("branch"))
    for other in (["-b"], ["-w"], ["-f"], ["-m"], ["-s"], ["-r", "chr1", "1000", "90000"]):
        for args in (["-q", q, "-U", q] + other, other + ["-U", q, "-q", q], ["-Q", lst, "-U", q] + other):
            got = _run(["search", db] + args, HOST)
            assert got.returncode == 0 and got.stdout.decode() == CONFLICT, args
    missing = os.path.join(tmp, "nothing.bed")
    empty = os.path.join(tmp, "empty.bed")
    open(empty, "w").write("\n# no region\n")
    for u in (missing, empty):
        for args in (["-q", q, "-U", u], ["-Q", lst, "-U", u]):
            got = _run(["search", db] + args, HOST)
            out = got.stdout.decode()
            assert got.returncode == 0 and out == "Cannot read universe file %s, or it holds no region\n" % u, (args, out)
    got = _run(["search", db, "-q", q, "-U"], HOST)
    assert got.returncode == 0 and got.stdout.decode() == "No universe file.\n"
    # the other command lines are as they were: -u alone still prints its own table
    got = _run(["search", db, "-q", q, "-u"], HOST)
    assert got.stdout.decode().startswith("index\t number of regions\t number of query regions\t File_name\n")
    import subprocess
    usage = subprocess.run([os.path.join(os.path.dirname(os.path.dirname(db)), "..", "..", "bin", "igd"), "search"],
                           stderr=subprocess.PIPE, stdout=subprocess.PIPE).stderr.decode()
    assert "-U <universe file>" in usage
