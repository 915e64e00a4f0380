"""`igd search ... -O N -A F -B F` without a GPU: parsing, refusals, and the tables of plain `-q` / `-Q`, `-u`, `-U` and `-P` on
the host route (small files) against tables made from tests/minoverlap_ref.py -- the oracle's enumeration, the predicate in
integers.  The layouts are those of the commands without the options; only the numbers differ."""
import os
import random
import shutil

import numpy as np
import pytest

import fisher_ref as FR
import minoverlap_ref as R
import permute_ref as PR
from helpers import Oracle, short_tmpdir, write_bed
from test_enrich_host import compare_block, tables_from_supports
from test_permute_cli import HEADER as P_HEADER
from test_permute_cli import fmt
from test_sets_cli import _write_list
from test_support_host import HOST, _index, _run


@pytest.fixture(scope="module")
def fx():
    d = short_tmpdir("imc")
    f = R.tiles_fixture(random.Random(31), d, set_sizes=(300, 200, 250))
    f.d, f.orc = d, Oracle(f.path)
    f.beds = []
    for k in range(len(f.off) - 1):
        a, b = f.off[k], f.off[k + 1]
        p = os.path.join(d, "s%d.bed" % k)
        write_bed(p, [(f.ctgs[c], int(s), int(e)) for c, s, e in zip(f.ichr[a:b], f.qs[a:b], f.qe[a:b])])
        f.beds.append(p)
    f.p = R.pairs(f.orc, f.ichr, f.qs, f.qe)
    f.bd = R.boundary_fixture(d)
    yield f
    f.orc.close()
    shutil.rmtree(d, ignore_errors=True)


def ref(f, t):
    """(hits, totals, support, nhit) per set under threshold t; the threshold must cut"""
    k = R.keep(t, f.p, f.qs, f.qe)
    if any(t):
        R.assert_cuts(f.nfiles, f.p, k)
    return R.counts(f.nfiles, f.p, k, f.off)


def hits_table(f, row):
    out = "index\t number of regions\t number of hits\t File_name\n"
    for i, (nr, name) in enumerate(_index(f.path)):
        if row[i] > 0:
            out += "%d\t%d\t%d\t%s\n" % (i, nr, row[i], name)
    return out + "Total: %d\n" % row.sum()


def support_table(f, row, nhit, n):
    out = "index\t number of regions\t number of query regions\t File_name\n"
    for i, (nr, name) in enumerate(_index(f.path)):
        if row[i] > 0:
            out += "%d\t%d\t%d\t%s\n" % (i, nr, row[i], name)
    return out + "Query regions with a hit: %d of %d\n" % (nhit, n)


def run(f, args, env=HOST):
    return _run(["search", f.path] + args, env)


OPTS = [(["-O", "120"], (120, 0, 0)), (["-A", "0.5", "-B", "0.5"], (0, 500000, 500000)), (["-B", "0.4", "-O", "30", "-A", "0.25"], (30, 250000, 400000))]


@pytest.mark.parametrize("opts,t", OPTS)
def test_plain_counts_and_u_tables_equal_the_reference(fx, opts, t):
    hits, tot, sup, nhit = ref(fx, t)
    plain = ref(fx, (0, 0, 0))
    assert (hits.sum(axis=1) < plain[0].sum(axis=1)).all() and (sup.sum(axis=1) < plain[2].sum(axis=1)).all()
    for k, bed in enumerate(fx.beds):
        n = int(fx.off[k + 1] - fx.off[k])
        for args in (["-q", bed] + opts, opts + ["-q", bed]):
            got = run(fx, args)
            assert got.returncode == 0 and got.stdout.decode() == hits_table(fx, hits[k]), args
            got = run(fx, args + ["-u"])
            assert got.returncode == 0 and got.stdout.decode() == support_table(fx, sup[k], nhit[k], n), args
    lst = _write_list(fx.d, fx.beds)
    got = run(fx, ["-Q", lst] + opts)
    assert got.stdout.decode() == "".join("Query set %d: %s\n" % (k, p) + hits_table(fx, hits[k]) for k, p in enumerate(fx.beds))
    got = run(fx, ["-Q", lst, "-u"] + opts)
    want = "".join("Query set %d: %s\n" % (k, p) + support_table(fx, sup[k], nhit[k], int(fx.off[k + 1] - fx.off[k])) for k, p in enumerate(fx.beds))
    assert got.stdout.decode() == want
    # without the options, and with all of them zero, the tables are the plain ones
    for extra in ([], ["-O", "0"], ["-A", "0", "-B", "0.000000"]):
        assert run(fx, ["-q", fx.beds[0], "-u"] + extra).stdout.decode() == support_table(fx, plain[2][0], plain[3][0], int(fx.off[1]))
        assert run(fx, ["-q", fx.beds[0]] + extra).stdout.decode() == hits_table(fx, plain[0][0])


@pytest.mark.parametrize("opts,t", OPTS[1:])
def test_U_tables_take_sets_and_universe_under_the_threshold(fx, opts, t):
    """`-U -A`: the universe is the third set's file; a, b, c, d from the reference's supports of sets and universe"""
    _, _, sup, nhit = ref(fx, t)
    _, _, psup, _ = ref(fx, (0, 0, 0))
    uni, nu = fx.beds[2], int(fx.off[3] - fx.off[2])
    assert (sup[2] < psup[2]).any()
    for ranks in ([], ["-R"]):
        got = run(fx, ["-Q", _write_list(fx.d, fx.beds[:2]), "-U", uni] + opts + ranks)
        assert got.returncode == 0, got.stderr
        lines = got.stdout.decode().splitlines()
        for k in range(2):
            n = int(fx.off[k + 1] - fx.off[k])
            b, c, d, clamped = tables_from_supports(sup[k], sup[2], n, nu)
            rows = []
            for i, (nr, name) in enumerate(_index(fx.path)):
                if sup[k][i] > 0:
                    tb = (int(sup[k][i]), int(b[i]), int(c[i]), int(d[i]))
                    rows.append((i, nr) + tb + (FR.odds(*tb), FR.exact_plog(*tb), name))
            last = "Query regions with a hit: %d of %d; universe regions: %d; clamped cells: %d" % (nhit[k], n, nu, clamped)
            assert lines[0] == "Query set %d: %s" % (k, fx.beds[k])
            if ranks:                                             # six more columns: the first nine are the table's
                assert all(len(l.split("\t")) == 15 for l in lines[2:2 + len(rows)])
                lines = [lines[0], lines[1].split("\t rnkSup")[0]] + ["\t".join(l.split("\t")[:9]) for l in lines[2:2 + len(rows)]] + lines[2 + len(rows):]
            lines = compare_block(lines[1:], rows, last, (k, opts))
        assert lines == []


@pytest.mark.parametrize("opts,t,mode", [(["-B", "0.5"], (0, 0, 500000), "circular"), (["-O", "120", "-M", "shuffle"], (120, 0, 0), "shuffle")])
def test_P_table_counts_observed_and_permuted_rows_under_the_threshold(fx, opts, t, mode):
    ctg_len = np.array([6 * fx.nbp, 8 * fx.nbp], np.int32)
    ok = fx.qe <= ctg_len[fx.ichr]
    ichr, qs, qe = fx.ichr[ok][:250], fx.qs[ok][:250], fx.qe[ok][:250]
    bed, g = os.path.join(fx.d, "p.bed"), os.path.join(fx.d, "g.sizes")
    write_bed(bed, [(fx.ctgs[c], int(s), int(e)) for c, s, e in zip(ichr, qs, qe)])
    open(g, "w").write("chr1\t%d\nchr2\t%d\n" % tuple(ctg_len))
    nperm, seed, nq = 6, 3, len(qs)
    ps, pe = PR.permute(ichr, qs, qe, ctg_len, 0, nperm, seed, PR.SHUFFLE if mode == "shuffle" else PR.CIRCULAR)
    ci, cs, ce = np.tile(ichr, nperm + 1), np.concatenate([qs, ps.ravel()]), np.concatenate([qe, pe.ravel()])
    p = R.pairs(fx.orc, ci, cs, ce)
    k = R.keep(t, p, cs, ce)
    R.assert_cuts(fx.nfiles, p, k)
    _, _, sup, nhit = R.counts(fx.nfiles, p, k, np.arange(nperm + 2) * nq)
    rows = np.concatenate([sup, nhit[:, None]], axis=1)
    obs, rows = rows[0], rows[1:]
    st = PR.stats(rows, obs)
    mean, sd, z, pu, pl = PR.summary(rows, obs)
    names = [name for _, name in _index(fx.path)]
    want = P_HEADER
    for f in range(fx.nfiles):
        want += "%d\t%d\t%s\t%s\t%s\t%d\t%d\t%s\t%s\t%s\n" % (f, obs[f], fmt(mean[f]), fmt(sd[f]), fmt(z[f]), st[2][f], st[3][f], fmt(pu[f]),
                                                               fmt(pl[f]), names[f])
    a = fx.nfiles
    want += "Query regions with a hit: %d of %d\t%s\t%s\t%s\t%d\t%d\t%s\t%s\n" % (obs[a], nq, fmt(mean[a]), fmt(sd[a]), fmt(z[a]), st[2][a], st[3][a],
                                                                               fmt(pu[a]), fmt(pl[a]))
    got = run(fx, ["-q", bed, "-P", str(nperm), "-g", g, "-S", str(seed)] + opts)
    assert got.returncode == 0, got.stderr
    assert got.stdout.decode() == want


def one(bd, q):
    p = os.path.join(os.path.dirname(bd.path), "one%d.bed" % q)
    write_bed(p, [("chr1", int(bd.qs[q]), int(bd.qe[q]))])
    return p


def counted(fx, q, opts):
    got = _run(["search", fx.bd.path, "-q", one(fx.bd, q)] + opts, HOST)
    assert got.returncode == 0, (opts, got.stdout, got.stderr)
    return int(got.stdout.decode().splitlines()[-1].split(":")[1])


def test_fractions_are_parsed_to_ppm_exactly(fx):
    """the boundary fixture: query 0 has ov = 100 of 200 bp on a record of 1 000 bp; query 2 has ov = 2 of 3 bp; query 4 lies
    inside its record, 5 equals it, 6 contains it"""
    assert counted(fx, 0, ["-A", "0.5"]) == 1 and counted(fx, 0, ["-A", "0.500001"]) == 0 and counted(fx, 0, ["-A", ".5"]) == 1
    assert counted(fx, 0, ["-B", "0.1"]) == 1 and counted(fx, 0, ["-B", "0.100001"]) == 0 and counted(fx, 0, ["-B", "0.100000"]) == 1
    assert counted(fx, 0, ["-O", "100"]) == 1 and counted(fx, 0, ["-O", "101"]) == 0
    assert counted(fx, 2, ["-A", "0.666666"]) == 1 and counted(fx, 2, ["-A", "0.666667"]) == 0
    assert counted(fx, 3, ["-A", "0.333333"]) == 1 and counted(fx, 3, ["-A", "0.333334"]) == 0
    assert [counted(fx, q, ["-A", "1"]) for q in (4, 5, 6)] == [1, 1, 0] and [counted(fx, q, ["-B", "1.0"]) for q in (4, 5, 6)] == [0, 1, 1]
    assert [counted(fx, q, ["-A", "1", "-B", "1.000000"]) for q in (4, 5, 6)] == [0, 1, 0]
    # one part per million: every well-formed pair counts, as with no option
    assert [counted(fx, q, ["-A", "0.000001"]) for q in (0, 1, 2, 3, 4, 5, 6, 7)] == [counted(fx, q, []) for q in (0, 1, 2, 3, 4, 5, 6, 7)]
    for bad in (["-A", "0.5000001"], ["-A", "1.5"], ["-B", "1.000001"], ["-A", "-0.5"], ["-A", "0,5"], ["-B", "5e-1"], ["-A", "2"],
                ["-A", "."], ["-A", ""], ["-O", "-1"], ["-O", "1.5"], ["-O", "2147483648"], ["-O", "x"], ["-A"]):
        got = _run(["search", fx.bd.path, "-q", one(fx.bd, 0)] + bad, HOST)
        assert got.returncode != 0 and got.stdout.decode().startswith("Not supported: " + bad[0]), (bad, got.stdout)
        assert b"index\t" not in got.stdout


def test_zero_length_and_inverted_lines_count_only_without_a_threshold(fx):
    """the reader keeps a line with start >= end when its end is positive; the plain search counts it under a record that spans
    it, a threshold never does"""
    bd = fx.bd
    z = [q for q in range(len(bd.qs)) if bd.qe[q] <= bd.qs[q]]
    assert len(z) == 2
    for q in z:
        assert counted(fx, q, []) == 1
        assert counted(fx, q, ["-O", "1"]) == counted(fx, q, ["-A", "0.000001"]) == counted(fx, q, ["-B", "0.000001"]) == 0


@pytest.mark.parametrize("other", [["-b"], ["-w"], ["-C"], ["-U", "UNI", "-X"], ["-f"], ["-m"], ["-s"]])
def test_other_selectors_are_refused_with_a_threshold(fx, other):
    other = [fx.beds[2] if a == "UNI" else a for a in other]
    for opts in (["-O", "5"], ["-A", "0.5"], ["-B", "0.25"], ["-O", "0"]):
        for args in (["-q", fx.beds[0]] + other + opts, opts + other + ["-q", fx.beds[0]]):
            got = run(fx, args)
            assert got.returncode != 0, args
            assert got.stdout.decode() == "Not supported: -O, -A or -B together with -b, -w, -X, -C, -f, -m, -s or -r, or without -q or -Q\n"
    for args in (["-r", "chr1", "100", "9000", "-O", "5"], ["-O", "5"]):
        got = run(fx, args)
        assert got.returncode != 0 and got.stdout.decode().startswith("Not supported: -O, -A or -B"), args
