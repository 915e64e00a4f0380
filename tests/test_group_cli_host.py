"""`igd search -K groups.tsv` with `-u` and with `-U [-R]` on the host route, the refusals, and the command lines without -K.

The goldens under tests/golden/groups/ (groups.tsv and universe.bed for the database of tests/golden/branch; K_u.txt, K_u_v500.txt,
K_U_R.txt) are the texts golden_u() / golden_UR() below produce from the CPU oracle one region at a time (group_support_ref), exact
hypergeometric tails (fisher_ref) and the rank definitions (rank_ref): the first test regenerates them and compares the bytes,
so they cannot drift from their source.  `-K -u` is held to them byte for byte.  The `-K -U -R` table's integers, names and ranks
are held to the golden exactly; its %.4f fields within the bound tests/test_enrich_host.py holds the dataset table to (the host's
lgamma sum and the exact tail may round a printed tie differently)."""
import json
import math
import os
import shutil

import numpy as np
import pytest

import fisher_ref as R
import group_support_ref as G
import rank_ref as RK
from helpers import GOLDEN, Oracle, short_tmpdir
from test_enrich_host import tables_from_supports
from test_sets_cli import _write_list
from test_support_host import HOST, _index, _run

DB = os.path.join(GOLDEN, "branch", "db.igd")
Q = os.path.join(GOLDEN, "branch", "q.bed")
DIR = os.path.join(GOLDEN, "groups")
GROUPS, UNIVERSE = os.path.join(DIR, "groups.tsv"), os.path.join(DIR, "universe.bed")
U_HEAD = "index\t number of datasets\t number of query regions\t Group_name\n"
UR_HEAD = ("index\t number of datasets\t support\t b\t c\t d\t oddsRatio\t pValueLog\t Group_name"
           "\t rnkSup\t rnkPV\t rnkOR\t maxRnk\t meanRnk\t qValueLog\n")


@pytest.fixture
def tmp():
    d = short_tmpdir("igc")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def groups_of(db=DB, path=GROUPS):
    from igd_amd.database import read_groups_file
    return read_groups_file(path, [name for _, name in _index(db)])


def group_counts(orc, g, qfile, v):
    ichr, qs, qe = orc.read_queries(qfile)
    off = np.array([0, len(qs)], np.int64)
    sup, nhit = G.expected(G.oracle_member(orc, ichr, qs, qe, v), g, off)
    return sup[0], int(nhit[0]), len(qs)


def golden_u(orc, g, qfile, v=0):
    sup, nhit, nq = group_counts(orc, g, qfile, v)
    nds = g.n_datasets
    out = U_HEAD
    for i in range(g.ngroups):
        if sup[i] > 0:
            out += "%d\t%d\t%d\t%s\n" % (i, nds[i], sup[i], g.names[i])
    return out + "Query regions with a hit: %d of %d\n" % (nhit, nq)


def golden_UR(orc, g, qfile, ufile, v=0):
    sup, nhit, nq = group_counts(orc, g, qfile, v)
    usup, _, nu = group_counts(orc, g, ufile, v)
    b, c, d, clamped = tables_from_supports(sup, usup, nq, nu)
    tabs = [(int(sup[i]), int(b[i]), int(c[i]), int(d[i])) for i in range(g.ngroups)]
    plog = np.array([R.exact_plog(*t) for t in tabs])
    odds = np.array([R.odds(*t) for t in tabs])
    rk = RK.reference(sup[None, :], plog[None, :], odds[None, :])
    nds = g.n_datasets
    out = UR_HEAD
    for i in range(g.ngroups):
        if sup[i] > 0:
            out += "%d\t%d\t%d\t%d\t%d\t%d\t%.4f\t%.4f\t%s" % ((i, nds[i]) + tabs[i] + (odds[i], plog[i], g.names[i]))
            out += "\t%d\t%d\t%d\t%d\t%.2f\t%.4f\n" % (rk.rnk_sup[0, i], rk.rnk_pv[0, i], rk.rnk_or[0, i], rk.max_rnk[0, i], rk.mean_rnk[0, i],
                                                    rk.qvalue_log[0, i])
    return out + "Query regions with a hit: %d of %d; universe regions: %d; clamped cells: %d\n" % (nhit, nq, nu, clamped)


def same_table(got, want, what):
    """a -U [-R] text against its golden: lines, integers, names and ranks exactly, the printed decimals within the bound"""
    gl, wl = got.splitlines(), want.splitlines()
    assert len(gl) == len(wl), (what, got, want)
    for a, b in zip(gl, wl):
        fa, fb = a.split("\t"), b.split("\t")
        if len(fb) < 9 or not fb[0].isdigit():
            assert a == b, what
            continue
        assert len(fa) == len(fb) and fa[:6] == fb[:6] and fa[8:14] == fb[8:14], (what, a, b)
        for j in [6, 7] + ([14] if len(fb) > 14 else []):
            x, y = float(fa[j]), float(fb[j])
            assert fa[j] == fb[j] or (math.isfinite(x) and abs(x - y) <= 1.01e-4), (what, j, a, b)


def test_the_goldens_are_what_the_oracle_and_the_exact_statistics_give():
    g = groups_of()
    assert g.ngroups == 6 and g.names[-1] == "late  name with blanks" and g.n_datasets.tolist() == [4, 3, 3, 9, 2, 1]
    orc = Oracle(DB)
    try:
        member = G.oracle_member(orc, *orc.read_queries(Q), 0)
        off = np.array([0, len(member)], np.int64)
        G.nonvacuous(member, g, off, G.expected(member, g, off)[0])
        for name, text in (("K_u.txt", golden_u(orc, g, Q)), ("K_u_v500.txt", golden_u(orc, g, Q, 500)),
                           ("K_U_R.txt", golden_UR(orc, g, Q, UNIVERSE))):
            assert open(os.path.join(DIR, name), newline="").read() == text, name
    finally:
        orc.close()


def test_K_u_prints_the_golden_on_the_host_route(tmp):
    for args, name in ((["-q", Q, "-u", "-K", GROUPS], "K_u.txt"), (["-K", GROUPS, "-u", "-q", Q], "K_u.txt"),
                       (["-q", Q, "-u", "-K", GROUPS, "-v", "500"], "K_u_v500.txt")):
        got = _run(["search", DB] + args, HOST)
        assert got.returncode == 0, got.stderr
        assert got.stdout.decode() == open(os.path.join(DIR, name), newline="").read(), args
    # -Q: a block per file, a missing file an empty set; and a minimum overlap reaches the group counts
    files = [Q, os.path.join(tmp, "missing.bed"), os.path.join(GOLDEN, "branch", "beds", "f00.bed")]
    got = _run(["search", DB, "-Q", _write_list(tmp, files), "-u", "-K", GROUPS], HOST)
    assert got.returncode == 0, got.stderr
    orc, g = Oracle(DB), groups_of()
    try:
        want = "Query set 0: %s\n" % files[0] + golden_u(orc, g, Q)
        want += "Query set 1: %s\n" % files[1] + U_HEAD + "Query regions with a hit: 0 of 0\n"
        want += "Query set 2: %s\n" % files[2] + golden_u(orc, g, files[2])
        assert got.stdout.decode() == want
        ichr, qs, qe = orc.read_queries(Q)
        m = G.oracle_member_ov(orc, ichr, qs, qe, 40, 0, 0)
        sup, nhit = G.expected(m, g, np.array([0, len(qs)], np.int64))
        assert 0 < sup.sum() < G.expected(G.oracle_member(orc, ichr, qs, qe, 0), g, np.array([0, len(qs)], np.int64))[0].sum()
        got = _run(["search", DB, "-q", Q, "-u", "-K", GROUPS, "-O", "40"], HOST).stdout.decode().splitlines()
        assert [int(l.split("\t")[2]) for l in got[1:-1]] == [int(x) for x in sup[0] if x > 0]
        assert got[-1] == "Query regions with a hit: %d of %d" % (nhit[0], len(qs))
    finally:
        orc.close()


def test_K_U_R_prints_the_golden_on_the_host_route(tmp):
    want = open(os.path.join(DIR, "K_U_R.txt"), newline="").read()
    got = _run(["search", DB, "-q", Q, "-U", UNIVERSE, "-R", "-K", GROUPS], HOST)
    assert got.returncode == 0, got.stderr
    same_table(got.stdout.decode(), want, "-U -R -K")
    assert len(want.splitlines()) > 4
    # without -R: the same lines without the six rank columns
    plain = _run(["search", DB, "-q", Q, "-U", UNIVERSE, "-K", GROUPS], HOST)
    assert plain.returncode == 0
    cut = "\n".join("\t".join(l.split("\t")[:9]) for l in want.splitlines()) + "\n"
    same_table(plain.stdout.decode(), cut, "-U -K")
    lst = _write_list(tmp, [Q, Q])
    both = _run(["search", DB, "-Q", lst, "-U", UNIVERSE, "-R", "-K", GROUPS], HOST)
    assert both.returncode == 0
    same_table(both.stdout.decode(), "Query set 0: %s\n" % Q + want + "Query set 1: %s\n" % Q + want, "-Q -U -R -K")


@pytest.mark.parametrize("other", [["-b"], ["-w"], ["-U", "U", "-X"], ["-C"], ["-P", "10", "-g", "G"], ["-J"], ["-V", "count"], ["-N", "100"],
                                   ["-f"], ["-m"], ["-s"], ["-r", "chr1", "1000", "90000"]])
def test_K_with_another_selector_is_refused(other, tmp):
    other = [UNIVERSE if a == "U" else os.path.join(tmp, "genome") if a == "G" else a for a in other]
    for args in (["-q", Q, "-u", "-K", GROUPS] + other, other + ["-K", GROUPS, "-u", "-q", Q]):
        got = _run(["search", DB] + args, HOST)
        assert got.returncode == 64 and got.stdout.decode().startswith("Not supported: -K together with"), (args, got.stdout)
        assert b"index\t" not in got.stdout


def test_K_alone_and_bad_group_files_are_refused(tmp):
    for args, text in ((["-q", Q, "-K", GROUPS], "Not supported: -K without -u or -U\n"), (["-u", "-K", GROUPS], "Not supported: -K without -q or -Q\n"),
                       (["-q", Q, "-u", "-K"], "Not supported: -K without a groups file\n")):
        got = _run(["search", DB] + args, HOST)
        assert got.returncode == 64 and got.stdout.decode() == text, (args, got.stdout)
    p = os.path.join(tmp, "bad.tsv")
    for body, text in (("f00.bed\tx\n\n# c\nnope.bed\ty\n", "line 4: the database has no such dataset"), ("f00.bed\tx\n10\ty\n", "line 2: the database has no such dataset"),
                       ("f00.bed\tx\nf01.bed\n", "line 2: not a dataset, a tab and a group"), ("# nothing\n", "(the file names no group)"),
                       ("".join("f00.bed\tg%d\n" % i for i in range(8193)), "line 8193: more than 8192 groups")):
        with open(p, "w") as fh:
            fh.write(body)
        for sel in (["-u"], ["-U", UNIVERSE, "-R"]):
            got = _run(["search", DB, "-q", Q, "-K", p] + sel, HOST)
            assert got.returncode == 64, (body[:30], got.stdout)
            assert got.stdout.decode() == "Not supported: -K %s%s%s\n" % (p, " " if text.startswith("(") else ", ", text)
    got = _run(["search", DB, "-q", Q, "-u", "-K", os.path.join(tmp, "none.tsv")], HOST)
    assert got.returncode == 64 and b"cannot open the groups file" in got.stdout
    # 8 192 groups are served
    with open(p, "w") as fh:
        fh.write("".join("%d\tg%d\n" % (i % 10, i) for i in range(8192)))
    got = _run(["search", DB, "-q", Q, "-u", "-K", p], HOST)
    assert got.returncode == 0 and got.stdout.decode().startswith(U_HEAD)


def test_command_lines_without_K_keep_their_bytes():
    """the reference's own goldens, and the -u / -U tables of the datasets: what they were before -K existed"""
    d = os.path.join(GOLDEN, "branch")
    man = json.load(open(os.path.join(d, "manifest.json")))
    for run in man["runs"]:
        got = _run(run["args"], HOST, cwd=d)
        assert got.stdout == open(os.path.join(d, run["stdout"]), "rb").read(), run["args"]
    from test_support_host import expected_table
    orc = Oracle(DB)
    try:
        assert _run(["search", DB, "-q", Q, "-u"], HOST).stdout.decode() == expected_table(DB, orc, Q, 0)
    finally:
        orc.close()
    got = _run(["search", DB, "-q", Q, "-U", UNIVERSE, "-R"], HOST).stdout.decode()
    assert got.startswith("index\t number of regions\t support\t b\t c\t d\t oddsRatio\t pValueLog\t File_name\t rnkSup") and "f00.bed" in got


def test_the_probe_finds_the_two_routes_equal_on_the_host():
    """tools/group_support_probe.py --host: group_support_host against igdc_membership_host folded in numpy, equal integers"""
    import subprocess
    import sys
    from helpers import ROOT
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "group_support_probe.py"), "--host", "--sets", "3", "--regions", "1500"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    out = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert out["equal"] is True and out["route"] == "host" and out["group_regions"] > 0 and out["ngroups"] > 100
