"""GPU: region-set enrichment (igd_hip_enrich_sets = igd_hip_support_sets over the sets and the universe + igd_fisher_cells;
Database.enrichment_sets / enrichment_files, `igd search -U` on the engine route).

Expected supports come from the CPU oracle one query at a time, b, c, d and the clamp counts from the definitions, the
statistics from exact arithmetic (fisher_ref.py) within the issue's bound; the engine's two forms of the cell kernel must
agree bit for bit, and the engine route of the command line must print the host route's table."""
import os
import shutil

import numpy as np
import pytest

import fisher_ref as R
from helpers import Oracle, short_tmpdir
import test_enrich_host as EH
from test_enrich_host import HEADER, enrich_fixture, tables_from_supports
from test_sets_cli import _write_list
from test_support_host import FLAT, HOST, NEST, NOV, _run, oracle_support

pytestmark = pytest.mark.gpu
ENGINE = {"IGD_HOST_MAX_QUERIES": "0"}
NFILES = 40


@pytest.fixture(scope="module")
def fx():
    """about 40 files, a universe of a few thousand regions, three user sets of which the second is empty"""
    from igd_amd import Database
    d = short_tmpdir("ige")
    path, upath, sets, uni = enrich_fixture(d, nfiles=NFILES, name="ge")
    empty = os.path.join(d, "ge_empty.bed")
    open(empty, "w").close()
    files = [sets[0], empty, sets[1]]
    orc, db = Oracle(path), Database(path)
    assert 2000 < len(uni) < 10000 and orc.nfiles == NFILES
    q = [orc.read_queries(p) for p in files]
    off = np.zeros(len(q) + 1, np.int64)
    off[1:] = np.cumsum([len(s[1]) for s in q])
    cat = [np.concatenate([s[i] for s in q]).astype(np.int32) for i in range(3)]
    other = orc.read_queries(sets[2])
    yield dict(d=d, path=path, upath=upath, files=files, sets=sets, orc=orc, db=db, q=q, off=off, cat=cat, other=other,
               uni=orc.read_queries(upath), want={})
    db.close()
    orc.close()
    shutil.rmtree(d, ignore_errors=True)


def expected(fx, key, sets, v):
    """oracle supports, defined tables and exact statistics of `sets` against the universe (computed once per key)"""
    if key not in fx["want"]:
        orc = fx["orc"]
        usup, _, _ = oracle_support(orc, *fx["uni"], v)
        nu = len(fx["uni"][1])
        out = []
        for ichr, qs, qe in sets:
            sup, _, _ = oracle_support(orc, ichr, qs, qe, v)
            b, c, d, clamped = tables_from_supports(sup, usup, len(qs), nu)
            tabs = [(int(sup[f]), int(b[f]), int(c[f]), int(d[f])) for f in range(orc.nfiles)]
            out.append((sup, b, c, d, clamped, tabs, [R.exact_plog(*t) for t in tabs]))
        fx["want"][key] = (usup, out)
    return fx["want"][key]


def check_result(fx, res, want, what):
    usup, sets = want
    db = fx["db"]
    assert np.array_equal(res.usupport, usup), what
    for k, (sup, b, c, d, clamped, tabs, plog) in enumerate(sets):
        assert np.array_equal(res.support[k], sup), (what, k)
        assert np.array_equal(res.b[k], b) and np.array_equal(res.c[k], c) and np.array_equal(res.d[k], d), (what, k)
        assert res.clamped[k] == clamped, (what, k)
        R.check(tabs, plog, res.pvalue_log[k], res.odds_ratio[k], (what, k))
    # the enrichment form and the generic form of the cell kernel: the same bits
    p, o = db.fisher(res.support.ravel(), res.b.ravel(), res.c.ravel(), res.d.ravel())
    assert np.array_equal(p.view(np.int64), res.pvalue_log.ravel().view(np.int64)), what
    assert np.array_equal(o.view(np.int64), res.odds_ratio.ravel().view(np.int64)), what


@pytest.mark.parametrize("mode", ["nest", "v400"])
def test_enrichment_sets_equals_oracle_definitions_and_exact_statistics(fx, mode):
    db = fx["db"]
    v = 0 if mode == "nest" else 400
    want = expected(fx, mode, fx["q"], v)
    if mode == "nest":
        res = db.enrichment_sets(*fx["cat"], fx["off"], *fx["uni"], rule=NEST)
    else:
        res = db.enrichment_sets(*fx["cat"], fx["off"], *fx["uni"], v=400)
        res2 = db.enrichment_sets(*fx["cat"], fx["off"], *fx["uni"], rule=FLAT, value_filter=400)
        for x, y in zip(res, res2):
            assert np.array_equal(x, y, equal_nan=True)
    assert res.support.shape == (3, NFILES) and res.pvalue_log.shape == (3, NFILES) and res.clamped.shape == (3,)
    check_result(fx, res, want, mode)
    # the empty set: a = 0 everywhere, p = 1, nothing clamped unless the universe itself is
    assert not res.support[1].any() and not res.pvalue_log[1].any() and (res.c[1] == 0).all()
    if mode == "nest":                                         # not vacuous: enrichment, a clamped b, a file without support
        assert res.pvalue_log.max() > 2 and res.clamped.sum() > 0 and (res.usupport[None, :] < res.support).any()
        assert (res.support[0] == 0).any() and (res.support[0] > 0).any()


def test_second_call_on_the_same_handle_is_untouched_by_the_first(fx):
    """outputs are DEFINED, not accumulated: other sets, then the first ones again"""
    db = fx["db"]
    first = db.enrichment_sets(*fx["cat"], fx["off"], *fx["uni"])
    o = fx["other"]
    res = db.enrichment_sets(o[0], o[1], o[2], np.array([0, len(o[1])], np.int64), *fx["uni"])
    check_result(fx, res, expected(fx, "other", [o], 0), "other")
    again = db.enrichment_sets(*fx["cat"], fx["off"], *fx["uni"])
    for x, y in zip(first, again):
        assert np.array_equal(x, y, equal_nan=True)
    check_result(fx, again, expected(fx, "nest", fx["q"], 0), "again")
    # no set at all: the universe's supports are still defined
    none = db.enrichment_sets(o[0][:0], o[1][:0], o[2][:0], np.zeros(1, np.int64), *fx["uni"])
    assert none.support.shape == (0, NFILES) and np.array_equal(none.usupport, first.usupport)


def _parse(text):
    """[(set line or None, rows [[fields]], last line)] of a -U output"""
    blocks, cur = [], None
    title = None
    for line in text.splitlines():
        if line.startswith("Query set "):
            title = line
        elif line == HEADER:
            cur = []
        elif line.startswith("Query regions with a hit:"):
            blocks.append((title, cur, line))
            cur, title = None, None
        else:
            assert cur is not None, line
            cur.append(line.split("\t"))
    return blocks


@pytest.mark.parametrize("extra", [[], ["-v", "400"]])
def test_files_and_the_engine_route_of_the_command_line_equal_the_host_route(fx, extra):
    db, path, upath, files = fx["db"], fx["path"], fx["upath"], fx["files"]
    v = int(extra[1]) if extra else 0
    res = db.enrichment_files(files, upath, v)
    direct = db.enrichment_sets(*fx["cat"], fx["off"], *fx["uni"], v=v)
    for x, y in zip(res, direct):
        assert np.array_equal(x, y, equal_nan=True)
    lst = _write_list(fx["d"], files)
    for args in (["-Q", lst, "-U", upath] + extra, ["-q", files[2], "-U", upath] + extra):
        host = _run(["search", path] + args, HOST)
        eng = _run(["search", path] + args, ENGINE)
        assert host.returncode == 0 and eng.returncode == 0, (host.stderr, eng.stderr)
        H, E = _parse(host.stdout.decode()), _parse(eng.stdout.decode())
        assert len(H) == len(E) == (3 if args[0] == "-Q" else 1)
        for (ht, hrows, hlast), (et, erows, elast) in zip(H, E):
            assert ht == et and hlast == elast and len(hrows) == len(erows)
            for h, e in zip(hrows, erows):
                assert h[:6] == e[:6] and h[8] == e[8]
                for j in (6, 7):                               # %.4f fields as numbers: the routes may round a tie differently
                    assert h[j] == e[j] or abs(float(h[j]) - float(e[j])) <= 1.01e-4, (h, e)
    # the -Q table is enrichment_files' matrix
    for k, (_, rows, last) in enumerate(_parse(_run(["search", path, "-Q", lst, "-U", upath] + extra, ENGINE).stdout.decode())):
        shown = [int(r[0]) for r in rows]
        assert shown == [f for f in range(NFILES) if res.support[k, f] > 0]
        for r in rows:
            f = int(r[0])
            assert [int(x) for x in r[2:6]] == [res.support[k, f], res.b[k, f], res.c[k, f], res.d[k, f]]
            assert abs(float(r[7]) - res.pvalue_log[k, f]) <= 5.01e-5
        assert last.endswith("clamped cells: %d" % res.clamped[k])


def test_bad_arguments_leave_nothing_written(fx):
    from igd_amd import _native as N
    db = fx["db"]
    H = N.hip()
    ichr, qs, qe = fx["cat"]
    u = fx["uni"]
    sup, usup = np.full((3, NFILES), -5, np.int64), np.full(NFILES, -5, np.int64)
    p, o, cl = np.full((3, NFILES), -5.0), np.full((3, NFILES), -5.0), np.full(3, -5, np.int64)
    for bad in (np.array([1, 2, 3, len(qs)], np.int64), np.array([0, 50, 20, len(qs)], np.int64)):
        rc = H.igd_hip_enrich_sets(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, bad.ctypes.data, 3, u[0].ctypes.data,
                                   u[1].ctypes.data, u[2].ctypes.data, len(u[1]), NOV, NEST, sup.ctypes.data, usup.ctypes.data,
                                   p.ctypes.data, o.ctypes.data, cl.ctypes.data)
        assert rc != 0
        assert (sup == -5).all() and (usup == -5).all() and (p == -5.0).all() and (o == -5.0).all() and (cl == -5).all()


# ---- the cell kernel beyond one cell per wave and beyond one launch (fixtures and their conditions: test_enrich_host.py) ----
def _open(path):
    from igd_amd import Database
    return Oracle(path), Database(path)


def test_waves_take_a_second_cell_in_the_enrichment_form():
    """267 sets x 40 files = 10 680 cells, more than the waves of the full grid: a wave's second cell g = cell0 + i has its
    own k = g / nF and f = g - k nF, so B[f] and C[k] follow the cell.  The last set, reached only as a second cell, is
    the one with clamped cells."""
    from igd_amd import _native as N
    d = short_tmpdir("igr")
    try:
        path, cat, off, uni = EH.recut_fixture(d)
        orc, db = _open(path)
        try:
            W = EH.expected_matrix(orc, cat, off, uni)
            nsets = len(off) - 1
            grid = int(N.hip().igd_hip_fisher_grid(nsets * NFILES))
            assert grid == int(N.hip().igd_hip_fisher_grid(1 << 40)) and nsets * NFILES > 4 * grid
            EH.second_cell_conditions(W, grid)
            res = db.enrichment_sets(*cat, off, *uni)
            want = (W["usupport"], [(W["support"][k], W["b"][k], W["c"][k], W["d"][k], int(W["clamped"][k]),
                                     [W["tables"][i] for i in W["idx"][k * NFILES:(k + 1) * NFILES]],
                                     [W["plog"][i] for i in W["idx"][k * NFILES:(k + 1) * NFILES]]) for k in range(nsets)])
            check_result(dict(db=db), res, want, "recut")
            late = np.arange(nsets * NFILES) >= 4 * grid
            assert (res.support.ravel()[late] > 0).any() and (res.pvalue_log.ravel()[late] > 0).any() and res.clamped[-1] > 0
        finally:
            db.close()
            orc.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_enrichment_form_across_the_chunk_seam():
    """2 081 files x 505 sets = 2^20 + 2 329 cells: the second launch has cell0 = 2^20 = 503 * 2081 + 1833, so its first cell
    is file 1833 of set 503; it reads rows + 2^20, writes pvalue_log + 2^20 / odds_ratio + 2^20 from a workspace laid out
    for 2^20 cells, and adds to clamped[503], which the first launch has already counted into.  Then the same tables go
    through the generic form, which crosses its own seam, and must give the same bits."""
    import time
    d = short_tmpdir("igm")
    try:
        t0 = time.perf_counter()
        path, cat, off, uni = EH.seam_fixture(d)
        orc, db = _open(path)
        try:
            W = EH.expected_matrix(orc, cat, off, uni)
            EH.seam_conditions(W, R.chunk_cells())
            t1 = time.perf_counter()
            res = db.enrichment_sets(*cat, off, *uni)
            t2 = time.perf_counter()
            worst = EH.check_matrix(W, res.usupport, res.support, res.clamped, res.pvalue_log, res.odds_ratio, "seam", res.b, res.c, res.d)
            k, f = divmod(R.chunk_cells(), EH.SEAM_FILES)
            for kk, ff in ((k, f - 1), (k, f), (EH.SEAM_SETS - 1, EH.SEAM_FILES - 1)):          # by name: the seam and the last cell
                i = kk * EH.SEAM_FILES + ff
                t, y = W["tables"][W["idx"][i]], W["plog"][W["idx"][i]]
                assert abs(res.pvalue_log[kk, ff] - y) <= R.tol(*t, y), (kk, ff, t)
            n = res.support.size
            p, o = db.fisher(res.support.ravel(), res.b.ravel(), res.c.ravel(), res.d.ravel(), pvalue_log=np.full(n, -7.0),
                             odds_ratio=np.full(n, -7.0))
            t3 = time.perf_counter()
            assert np.array_equal(p.view(np.int64), res.pvalue_log.ravel().view(np.int64))
            assert np.array_equal(o.view(np.int64), res.odds_ratio.ravel().view(np.int64))
            print("seam: worst |x - y| / bound = %.3g; preparation (database, oracle, exact values) %.2f s, enrichment_sets %.3f s, "
                  "generic form of the same tables %.3f s" % (worst, t1 - t0, t2 - t1, t3 - t2))
        finally:
            db.close()
            orc.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_without_odds_ratios_the_rest_is_unchanged(fx):
    """odds_ratio = NULL in the enrichment form: the same p-values, supports and clamp counts, nothing written around them"""
    from igd_amd import _native as N
    db = fx["db"]
    ichr, qs, qe = fx["cat"]
    off, u = fx["off"], fx["uni"]
    res = db.enrichment_sets(ichr, qs, qe, off, *u)
    assert res.clamped.sum() > 0
    n = 3 * NFILES
    sup, usup, cl = np.full(n + 8, -5, np.int64), np.full(NFILES + 8, -5, np.int64), np.full(3 + 8, -5, np.int64)
    p = np.full(n + 16, -5.0)
    rc = N.hip().igd_hip_enrich_sets(db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, off.ctypes.data, 3, u[0].ctypes.data,
                                     u[1].ctypes.data, u[2].ctypes.data, len(u[1]), NOV, NEST, sup[4:].ctypes.data, usup[4:].ctypes.data,
                                     p[8:].ctypes.data, None, cl[4:].ctypes.data)
    assert rc == 0
    assert np.array_equal(p[8:8 + n].view(np.int64), res.pvalue_log.ravel().view(np.int64))
    assert np.array_equal(sup[4:4 + n], res.support.ravel()) and np.array_equal(usup[4:4 + NFILES], res.usupport)
    assert np.array_equal(cl[4:7], res.clamped)
    for a, lo, hi in ((p, 8, 8 + n), (sup, 4, 4 + n), (usup, 4, 4 + NFILES), (cl, 4, 7)):
        assert (a[:lo] == -5).all() and (a[hi:] == -5).all()


def test_one_file_database():
    """nF = 1: the matrix is one column, k = g / 1 = g and f = 0 for every cell"""
    d = short_tmpdir("ig1")
    try:
        path, cat, off, uni = EH.one_file_fixture(d)
        orc, db = _open(path)
        try:
            assert orc.nfiles == 1
            W = EH.expected_matrix(orc, cat, off, uni)
            EH.one_file_conditions(W)
            res = db.enrichment_sets(*cat, off, *uni)
            assert res.support.shape == (6, 1)
            EH.check_matrix(W, res.usupport, res.support, res.clamped, res.pvalue_log, res.odds_ratio, "one file", res.b, res.c, res.d)
            p, o = db.fisher(res.support.ravel(), res.b.ravel(), res.c.ravel(), res.d.ravel())
            assert np.array_equal(p.view(np.int64), res.pvalue_log.ravel().view(np.int64))
            assert np.array_equal(o.view(np.int64), res.odds_ratio.ravel().view(np.int64))
        finally:
            db.close()
            orc.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
