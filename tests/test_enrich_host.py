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


# ---- the cell kernel's regimes beyond one cell per wave and one launch: fixtures, checked here on the host route ------------
# (tests/test_gpu_enrich.py runs the same fixtures through igd_hip_enrich_sets)
RECUT_FILES = 40
SEAM_FILES, SEAM_SETS = 2081, 505          # 1 050 905 cells; 2^20 = 503 * 2081 + 1833: the seam lies inside set 503
SEAM_U = 300


def recut_sets(q, hole, seed=206):
    """The regions of enrich_fixture's three sets re-cut into a few hundred small ones: the 40 regions inside `hole`
    (where the universe has nothing and file 1 is dense) stay together as the LAST set -- a > u, a clamped b, needs more of
    them than the 23 universe regions that file 1 meets -- and all others, shuffled, go into sets of 1, 2, 3, 0, 2, ..
    regions.
    Returns ((ichr, qs, qe), off)."""
    cat = [np.concatenate([s[i] for s in q]).astype(np.int32) for i in range(3)]
    inside = (cat[1] >= hole[0]) & (cat[1] < hole[1])
    h, rest = np.flatnonzero(inside), np.flatnonzero(~inside)
    assert len(h) >= 40
    rng = random.Random(seed)
    rest = list(rest)
    rng.shuffle(rest)
    parts, at, k = [], 0, 0
    while at < len(rest):
        m = (1, 2, 3, 0, 2)[k % 5]
        parts.append(rest[at:at + m])
        at += m
        k += 1
    parts.append(list(h))
    order = np.array([i for p in parts for i in p], np.int64)
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return tuple(a[order] for a in cat), off


def recut_fixture(d, name="rc"):
    """enrich_fixture's 40-file database and universe with its set regions re-cut: (db path, (ichr, qs, qe), off, universe
    (ichr, qs, qe)); more than 206 sets, so nsets * 40 exceeds the 8 192 waves of the cell kernel's full grid"""
    path, upath, sets, _ = enrich_fixture(d, nfiles=RECUT_FILES, name=name)
    span = (1 << 11) * 200
    orc = Oracle(path)
    try:
        cat, off = recut_sets([orc.read_queries(p) for p in sets], (span // 2, span // 2 + span // 10))
        uni = orc.read_queries(upath)
    finally:
        orc.close()
    return path, cat, off, uni


def seam_fixture(d, name="seam", nfiles=SEAM_FILES, nsets=SEAM_SETS):
    """2 081 files x 505 sets (the smaller of the two shapes that put the 2^20 seam inside a row: its database is an eighth
    of the 16 385-file one).  One contig, nbp = 2^12.
       universe  300 regions of 100 bp, 400 bp apart, over [0, 120 000)
       files     f % 50 == 27: one record over the whole universe (u = n_U: any set region that misses it makes d < 0);
                 f % 50 == 33: one record over the "hole" [130 000, 150 000) behind the universe and a short one inside it
                 (u is 1 or 2: a set with hole regions has a > u, b < 0);  all others: three records of 50 .. 12 000 bp
       sets      3 .. 12 universe regions; every fourth (k % 4 == 3, set 503 among them) and the last one 3 .. 10 universe regions and
                 5 .. 10 regions in the hole; set 100 is empty
    Files 1833, 1877, 1883, .. lie behind the seam, 27, 33, .. before it: the straddling set is clamped on both sides.
    Returns (db path, (ichr, qs, qe), off, universe (ichr, qs, qe))."""
    rng = random.Random(2081)
    nbp, end, hole = 1 << 12, 400 * SEAM_U, (130000, 150000)
    files = []
    for f in range(nfiles):
        if f % 50 == 27:
            rows = [("chr1", 0, end, 900)]
        elif f % 50 == 33:
            s = rng.randrange(0, end - 600)
            rows = [("chr1", hole[0], hole[1], 800), ("chr1", s, s + 500, rng.randint(0, 1000))]
        else:
            rows = []
            for _ in range(3):
                s = rng.randrange(0, end)
                rows.append(("chr1", s, s + rng.choice([50, 500, 3000, 12000]), rng.randint(0, 1000)))
        files.append(rows)
    path = os.path.join(d, name + ".igd")
    write_igd_numpy(path, files, nbp=nbp)
    uni = [(400 * i, 400 * i + 100) for i in range(SEAM_U)]
    regs, off = [], [0]
    for k in range(nsets):
        if k == 100:
            rows = []
        elif k % 4 == 3 or k == nsets - 1:
            rows = rng.sample(uni, rng.randint(3, 10))
            for _ in range(rng.randint(5, 10)):
                s = rng.randrange(hole[0], hole[1] - 200)
                rows.append((s, s + 150))
        else:
            rows = rng.sample(uni, rng.randint(3, 12))
        rng.shuffle(rows)
        regs += rows
        off.append(len(regs))
    r = np.array(regs, np.int32)
    u = np.array(uni, np.int32)
    return (path, (np.zeros(len(r), np.int32), r[:, 0].copy(), r[:, 1].copy()), np.array(off, np.int64),
            (np.zeros(len(u), np.int32), u[:, 0].copy(), u[:, 1].copy()))


def one_file_fixture(d):
    """nF = 1: one file, 30 universe regions of which 15 meet it, six sets -- enriched, without a hit, empty, outside the
    universe (b < 0), mostly beside everything (d < 0), ordinary.  Returns (db path, (ichr, qs, qe), off, universe)."""
    path = os.path.join(d, "one.igd")
    write_igd_numpy(path, [[("chr1", 100 * i, 100 * i + 60, 500) for i in range(0, 40, 2)] + [("chr1", 9000, 9900, 700)]], nbp=1 << 12)
    u = np.array([(100 * i, 100 * i + 50) for i in range(30)], np.int32)                 # 15 of 30 meet the file
    sets = [[(100 * i + 10, 100 * i + 20) for i in range(0, 12, 2)],                     # all six meet it: enriched
            [(100 * i + 10, 100 * i + 20) for i in range(1, 12, 2)],                     # none does
            [],
            [(9000 + 40 * i, 9000 + 40 * i + 30) for i in range(18)],                    # outside the universe: a = 18 > u, b < 0
            [(100 * i + 10, 100 * i + 20) for i in range(12)] + [(20000, 20100)] * 19,   # c = 25 > n_U - u = 15: d < 0
            [(100 * i + 10, 100 * i + 20) for i in range(4, 11)]]
    off = np.zeros(len(sets) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    r = np.array([x for s in sets for x in s], np.int32)
    return (path, (np.zeros(len(r), np.int32), r[:, 0].copy(), r[:, 1].copy()), off,
            (np.zeros(len(u), np.int32), u[:, 0].copy(), u[:, 1].copy()))


def one_file_conditions(W):
    assert W["support"].shape == (6, 1)
    assert W["usupport"][0] == 15 and list(W["support"][:, 0]) == [6, 0, 0, 18, 6, 4] and list(W["clamped"]) == [0, 0, 0, 1, 1, 0]
    assert W["raw_b"][3, 0] < 0 and W["raw_d"][4, 0] < 0 and W["d"][4, 0] == 0
    plog = [W["plog"][i] for i in W["idx"]]
    assert plog[0] > 2 and plog[3] > 9 and 0.3 < plog[5] < 0.31 and plog[1] == plog[2] == plog[4] == 0.0


def expected_matrix(orc, cat, off, uni, v=0):
    """dict of the whole matrix from the oracle one query at a time, the definitions and exact arithmetic memoised on the
    distinct tables: usupport, support, b, c, d [nsets, nfiles], clamped [nsets], the distinct tables, their exact values
    and idx [nsets * nfiles] into them"""
    usup, _, _ = oracle_support(orc, *uni, v)
    nu, nsets = len(uni[1]), len(off) - 1
    sup = np.zeros((nsets, orc.nfiles), np.int64)
    for k in range(nsets):
        a, b = int(off[k]), int(off[k + 1])
        sup[k], _, _ = oracle_support(orc, cat[0][a:b], cat[1][a:b], cat[2][a:b], v)
    B, Cc, D, clamped = (np.zeros_like(sup), np.zeros_like(sup), np.zeros_like(sup), np.zeros(nsets, np.int64))
    for k in range(nsets):
        B[k], Cc[k], D[k], clamped[k] = tables_from_supports(sup[k], usup, int(off[k + 1] - off[k]), nu)
    cells = np.stack([sup.ravel(), B.ravel(), Cc.ravel(), D.ravel()], axis=1)
    distinct, idx = np.unique(cells, axis=0, return_inverse=True)
    tables = [tuple(int(x) for x in t) for t in distinct]
    for t in tables:
        if t not in _memo:
            _memo[t] = R.exact_plog(*t)
    return dict(usupport=usup, support=sup, b=B, c=Cc, d=D, clamped=clamped, raw_b=usup[None, :] - sup,
                raw_d=nu - usup[None, :] - Cc, tables=tables, plog=[_memo[t] for t in tables], idx=idx.ravel())


def second_cell_conditions(W, grid):
    """the re-cut fixture: more cells than the waves of the full grid, and the cells a wave takes second are not idle"""
    nsets, nf = W["support"].shape
    waves = 4 * grid
    assert nsets >= 206 and nf == RECUT_FILES and nsets * nf > waves >= 8192
    late = np.arange(nsets * nf) >= waves
    plog = np.array(W["plog"])[W["idx"]]
    assert (W["support"].ravel()[late] > 0).any() and (plog[late] > 0).any()
    assert ((W["raw_b"].ravel() < 0) & late).any(), "no clamped cell among those a wave takes second"
    assert W["clamped"][-1] > 0 and not W["clamped"][:-1].any()
    assert (np.diff(np.flatnonzero(np.diff(W["idx"]) != 0)) < 64).any() and len(W["tables"]) > 100


def seam_conditions(W, chunk):
    """the seam fixture: the 2^20-th cell lies inside a row whose set has support and clamped cells on both sides of it"""
    nsets, nf = W["support"].shape
    assert nsets * nf > chunk and chunk % nf != 0 and nsets * nf - chunk < chunk
    k, f = divmod(chunk, nf)
    assert (k, f) == (503, 1833) and k < nsets - 1
    cl = (W["raw_b"][k] < 0) | (W["raw_d"][k] < 0)
    assert (W["support"][k, :f] > 0).any() and (W["support"][k, f:] > 0).any()
    assert cl[:f].any() and cl[f:].any() and W["clamped"][k] == cl.sum() > cl[:f].sum() > 0
    assert not np.array_equal(W["support"][0], W["support"][-1]) and W["support"][-1].any() and W["clamped"][-1] != W["clamped"][0]
    assert (W["raw_b"] < 0).any() and (W["raw_d"] < 0).any(), "both kinds of clamp"
    assert (W["raw_d"][k] < 0).any() and (W["raw_b"][k] < 0).any()
    assert max(sum(t) for t in W["tables"]) <= 400 and 1000 < len(W["tables"]) < 20000
    plog = np.array(W["plog"])
    assert (plog > 2).any() and (plog[W["idx"][chunk:]] > 0).any() and plog[W["idx"][chunk - 1]] != plog[W["idx"][chunk]]
    assert not W["support"][100].any()                          # the empty set


def check_matrix(W, usup, sup, clamped, plog, odds, what, b=None, c=None, d=None):
    """a whole answer against expected_matrix(): integers equal, statistics within the bound; returns the worst ratio"""
    assert np.array_equal(usup, W["usupport"]) and np.array_equal(sup, W["support"]), what
    for got, key in ((b, "b"), (c, "c"), (d, "d")):
        assert got is None or np.array_equal(got, W[key]), (what, key)
    assert np.array_equal(clamped, W["clamped"]), (what, "clamped")
    return R.check_many(W["tables"], W["plog"], W["idx"], np.asarray(plog).ravel(), np.asarray(odds).ravel(), what)


def host_answer(path, cat, off, uni, v=0):
    """the host route's pieces on the same sets: igdc_support_host per set and for the universe, the tables by the
    definitions (as enrich_tables of igd_cli_abi.c forms them), igdc_fisher_host for the statistics"""
    import igd_amd
    from test_support_host import HostDb, cli_rule
    h = HostDb(path)
    try:
        rule, ev = cli_rule(1, v)
        usup, _ = h.support(*uni, ev, rule)
        nsets = len(off) - 1
        sup = np.zeros((nsets, h.nfiles), np.int64)
        for k in range(nsets):
            a, b = int(off[k]), int(off[k + 1])
            sup[k], _ = h.support(cat[0][a:b], cat[1][a:b], cat[2][a:b], ev, rule)
    finally:
        h.close()
    nk = np.diff(off)[:, None]
    b = usup[None, :] - sup
    c = nk - sup
    d = len(uni[1]) - sup - b - c
    clamped = ((b < 0) | (d < 0)).sum(axis=1)
    b, d = np.maximum(b, 0), np.maximum(d, 0)
    p, o = igd_amd.fisher_host(sup.ravel(), b.ravel(), c.ravel(), d.ravel())
    return usup, sup, clamped, p, o


def test_recut_fixture_meets_its_conditions_and_the_host_answers_it(tmp):
    import time
    path, cat, off, uni = recut_fixture(tmp)
    orc = Oracle(path)
    try:
        W = expected_matrix(orc, cat, off, uni)
    finally:
        orc.close()
    second_cell_conditions(W, 2048)                             # (the GPU test reads the grid from igd_hip_fisher_grid)
    assert np.diff(off)[:-1].max() <= 3 and (np.diff(off) == 0).any() and off[-1] - off[-2] == 40
    t0 = time.perf_counter()
    worst = check_matrix(W, *host_answer(path, cat, off, uni), "recut, host")
    print("recut: %d sets x %d files, %d distinct tables, host worst |x - y| / bound = %.3g (%.2f s)"
          % (len(off) - 1, RECUT_FILES, len(W["tables"]), worst, time.perf_counter() - t0))


def test_seam_fixture_meets_its_conditions_and_the_host_answers_it(tmp):
    import time
    t0 = time.perf_counter()
    path, cat, off, uni = seam_fixture(tmp)
    t1 = time.perf_counter()
    orc = Oracle(path)
    try:
        W = expected_matrix(orc, cat, off, uni)
    finally:
        orc.close()
    t2 = time.perf_counter()
    assert np.diff(off).max() <= 20 and len(uni[1]) == SEAM_U
    seam_conditions(W, R.chunk_cells())
    worst = check_matrix(W, *host_answer(path, cat, off, uni), "seam, host")
    print("seam: %d x %d cells, %d distinct tables, host worst |x - y| / bound = %.3g; database %.2f s, oracle and exact "
          "values %.2f s, host route and check %.2f s" % (SEAM_SETS, SEAM_FILES, len(W["tables"]), worst, t1 - t0, t2 - t1,
                                                         time.perf_counter() - t2))


def test_one_file_fixture_meets_its_conditions_and_the_host_answers_it(tmp):
    path, cat, off, uni = one_file_fixture(tmp)
    orc = Oracle(path)
    try:
        assert orc.nfiles == 1
        W = expected_matrix(orc, cat, off, uni)
    finally:
        orc.close()
    one_file_conditions(W)
    check_matrix(W, *host_answer(path, cat, off, uni), "one file, host")
