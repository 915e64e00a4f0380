"""Dataset co-occurrence without a GPU: igdc_cooccur_host and igdc_bitrows_gram_host (igd_hostpath.c) through
igd_amd.cooccur_host / bitrows_gram_host, and igd_amd.jaccard.

    cooc[f, g] = #{ q : member[q, f] and member[q, g] }      nhit = the regions with any file

The expected matrix is member.T @ member (cooccur_ref.cooc) on the CPU oracle's membership, one region at a time
(test_membership_host.oracle_member); for the explicit rules on the rows of igdc_membership_host, which
tests/test_membership_host.py holds against the oracle.  All integers must be EQUAL; igd_amd.jaccard must be bit-equal to
the formula evaluated in numpy."""
import ctypes as C
import os
import random
import shutil

import numpy as np
import pytest

import cooccur_ref as CR
from helpers import Oracle, short_tmpdir, write_igd_numpy
from test_gpu_sets import DBS, _db, _sets
from test_membership_host import MemberHost, oracle_member
from test_support_host import FLAT, NEST, NOV, NUMPY_DBS, cli_rule, clustered_db, mixed_queries

SIZES = [300, 0, 65, 700]


@pytest.fixture
def tmp():
    d = short_tmpdir("ich")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def host_threads():
    yield lambda t: os.environ.__setitem__("IGD_HOST_THREADS", t)
    os.environ.pop("IGD_HOST_THREADS", None)


def check_matrix(cooc, nhit, member, what=None):
    want = CR.cooc(member)
    assert cooc.dtype == np.int64 and cooc.shape == want.shape, what
    assert np.array_equal(cooc, want), what
    assert np.array_equal(cooc, cooc.T), what
    assert np.array_equal(np.diagonal(cooc), member.sum(axis=0)), what
    assert nhit == int(member.any(axis=1).sum()), what


def _check_db(path, ichr, qs, qe, host_threads):
    import igd_amd
    orc, H = Oracle(path), MemberHost(path)
    try:
        for v in (0, 500):
            member, _ = oracle_member(orc, ichr, qs, qe, v)
            if v == 0:
                off = CR.cooc(member) - np.diag(member.sum(axis=0))
                assert off.any(), "no two files share a region: the fixture is vacuous"
                assert (member.sum(axis=1) == 0).any()
            for threads in ("1", "3"):
                host_threads(threads)
                cooc, nhit = igd_amd.cooccur_host(path, ichr, qs, qe, v)
                check_matrix(cooc, nhit, member, (v, threads))
            # the diagonal is the support of the region list: igdc_support_host
            rule, ev = cli_rule(orc.gtype, v)
            sup, snhit = H.support(ichr, qs, qe, ev, rule)
            assert np.array_equal(np.diagonal(cooc), sup) and nhit == snhit
        # both explicit rules, with and without a filter: member from igdc_membership_host with the same rule
        for rule, vf in ((NEST, None), (FLAT, None), (FLAT, 300), (NEST, 300)):
            bits, _, _ = H.membership(ichr, qs, qe, NOV if (vf is None or orc.gtype == 0) else vf, rule)
            member = CR.unpack(bits, orc.nfiles)
            cooc, nhit = igd_amd.cooccur_host(path, ichr, qs, qe, rule=rule, value_filter=vf)
            check_matrix(cooc, nhit, member, (rule, vf))
        # no region: a zero matrix
        cooc, nhit = igd_amd.cooccur_host(path, ichr[:0], qs[:0], qe[:0])
        assert cooc.shape == (orc.nfiles, orc.nfiles) and not cooc.any() and nhit == 0
    finally:
        H.close()
        orc.close()


@pytest.mark.parametrize("case", range(len(DBS)))
def test_cooccur_host_equals_the_oracle_on_the_small_databases(case, tmp, host_threads):
    rng = random.Random(900 + case)
    nbp, gtype, nfiles, nctg, span_tiles, dens, hot = DBS[case]
    path, span = _db(rng, tmp, "d%d" % case, nbp, gtype, nfiles, nctg, span_tiles, dens, hot)
    (ichr, qs, qe), _ = _sets(rng, nctg, nbp, span, SIZES)
    _check_db(path, ichr, qs, qe, host_threads)


def test_cooccur_host_on_a_clustered_database_with_more_than_32_files(tmp, host_threads):
    rng = random.Random(4102)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[2]
    assert nfiles > 32
    path, span = clustered_db(rng, tmp, "c2", nbp, gtype, nfiles, nctg, span_tiles)
    ichr, qs, qe = mixed_queries(rng, nctg, nbp, span, 1500)
    _check_db(path, ichr, qs, qe, host_threads)


def test_identical_regions_count_twice_and_chunks_add_up(tmp, host_threads):
    """70 000 regions: more than one chunk of 2^16 of the host route, the chunk end no multiple of the tiled pattern"""
    import igd_amd
    rng = random.Random(77)
    nbp = 1 << 12
    path, span = clustered_db(rng, tmp, "rep", nbp, 1, 40, 2, 20)
    ichr, qs, qe = mixed_queries(rng, 2, nbp, span, 333)
    orc = Oracle(path)
    try:
        member, _ = oracle_member(orc, ichr, qs, qe, 0)
    finally:
        orc.close()
    n = 70000
    reps = -(-n // 333)
    tc, ts, te = (np.ascontiguousarray(np.tile(a, reps)[:n]) for a in (ichr, qs, qe))
    tm = np.tile(member, (reps, 1))[:n]
    for threads in ("1", "5"):
        host_threads(threads)
        cooc, nhit = igd_amd.cooccur_host(path, tc, ts, te)
        check_matrix(cooc, nhit, tm, threads)
    assert cooc.max() > 2 * CR.cooc(member).max()


def test_one_file_database(tmp):
    import igd_amd
    path = os.path.join(tmp, "one.igd")
    write_igd_numpy(path, [[("chr1", 100, 200, 5), ("chr1", 150, 400, 900), ("chr1", 9000, 9100, 700)]], nbp=1 << 12, gtype=1)
    ichr = np.zeros(5, np.int32)
    qs = np.array([0, 120, 120, 500, 9050], np.int32)
    qe = np.array([50, 160, 160, 600, 9051], np.int32)
    cooc, nhit = igd_amd.cooccur_host(path, ichr, qs, qe)
    assert cooc.tolist() == [[3]] and nhit == 3
    cooc, nhit = igd_amd.cooccur_host(path, ichr, qs, qe, 800)
    assert cooc.tolist() == [[2]] and nhit == 2
    cooc, nhit = igd_amd.cooccur_host(path, ichr[:0], qs[:0], qe[:0])
    assert cooc.tolist() == [[0]] and nhit == 0
    j = igd_amd.jaccard(cooc)
    assert j.shape == (1, 1) and np.isnan(j[0, 0])


@pytest.mark.parametrize("kind", ["half", "sparse", "ones"])
def test_bitrows_gram_host_equals_the_reference(kind, host_threads):
    import igd_amd
    rs = np.random.default_rng(5)
    for m, n, nw in ((1, 1, 1), (7, 5, 3), (65, 33, 2), (40, 129, 17), (3, 4, 0), (0, 4, 2)):
        a, b = CR.random_rows(rs, m, nw, kind), CR.random_rows(rs, n, nw, kind)
        for threads in ("1", "4"):
            host_threads(threads)
            got = igd_amd.bitrows_gram_host(a, b)
            assert got.dtype == np.int64 and got.shape == (m, n) and np.array_equal(got, CR.gram(a, b)), (m, n, nw, threads)
            sym = igd_amd.bitrows_gram_host(a)
            assert sym.shape == (m, m) and np.array_equal(sym, CR.gram(a)) and np.array_equal(sym, igd_amd.bitrows_gram_host(a, a))
        if kind == "ones" and m and n:
            assert (got == 32 * nw).all()
    # many rows: several threads share the triangle
    a = CR.random_rows(rs, 300, 40, kind)
    host_threads("6")
    assert np.array_equal(igd_amd.bitrows_gram_host(a), CR.gram(a))


def test_jaccard_is_the_formula_bit_for_bit():
    import igd_amd
    rs = np.random.default_rng(9)
    member = rs.random((500, 23)) < 0.2
    member[:, 4] = False                                      # a file without a region: NaN against itself, 0 against the others
    member[:, 9] = member[:, 8]                               # two identical files: exactly 1.0
    c = CR.cooc(member)
    got = igd_amd.jaccard(c)
    d = np.diagonal(c).astype(np.int64)
    den = d[:, None] + d[None, :] - c
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(den == 0, np.nan, c.astype(np.float64) / den.astype(np.float64))
    assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))
    assert np.array_equal(np.isnan(got), den == 0) and np.isnan(got[4, 4]) and int(np.isnan(got).sum()) == 1
    assert not np.delete(got[4], 4).any() and not np.delete(got[:, 4], 4).any()
    assert got[8, 9] == 1.0 and (np.diagonal(got)[d > 0] == 1.0).all()
    ref = CR.jaccard(c)
    assert np.array_equal(np.isnan(ref), np.isnan(got)) and np.array_equal(ref[~np.isnan(ref)], got[~np.isnan(got)])
    assert "jaccard" in igd_amd.__all__ and "cooccur_host" in igd_amd.__all__ and "bitrows_gram_host" in igd_amd.__all__
