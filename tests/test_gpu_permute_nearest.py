"""GPU: the set statistics of the nearest record per dataset through the fused kernel, and their permutation null
(igd_hip_nearest_sets_fused / igd_hip_permute_nearest, kernel igd_nearest_slices; Database.nearest_sets_fused /
permutation_nearest, `-P -D`).

Expected values never come from the code under test: tests/nearest_ref.py's definition over the interval lists this test wrote,
tests/permute_ref.py's generator, and on the device the composition that existed before -- permute_regions + nearest_sets.
Every integer is compared exactly; every output is handed over full of garbage."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import igd_amd
import permute_nearest_ref as PN
import permute_ref as PR
from helpers import ROOT, short_tmpdir, write_bed
from nearest_ref import MAX_WINDOW, ListDb, clustered_lists, mixed_regions, placed_db, placed_regions, ref_rows, ref_sets, sparse_lists
from test_support_host import HOST, _run

pytestmark = pytest.mark.gpu
GARBAGE = 0x5a5a5a5a5a5a5a5a
SLICE_MIN, SLICES, SLICE_MAX, GRID = 64, 4096, 4096, 2048          # IGD_SETS_SLICE_MIN, IGD_SETS_SLICES, IGD_SETS_SLICE_MAX, IGD_SETS_GRID


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igf")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def max_files():
    from igd_amd import _native as N
    return N.hip().igd_hip_nearest_fused_max_files()


def slice_len(n):
    return max(SLICE_MIN, min(SLICE_MAX, (n + SLICES - 1) // SLICES))


def garbage(shape):
    return [np.full(shape, GARBAGE, np.int64) for _ in range(3)]


def check_fused(db, ldb, ichr, qs, qe, off, W, v=None, rows_route=True):
    """nearest_sets_fused against the definition and against nearest_sets"""
    off = np.asarray(off, np.int64)
    want = ref_sets(*ref_rows(ldb, ichr, qs, qe, W, v), off)
    got = db.nearest_sets_fused(ichr, qs, qe, off, W, value_filter=v, out=garbage((len(off) - 1, db.nfiles + 1)))
    for name, g, w in zip(("n_within", "n_overlap", "sum_dist"), got[:3], want):
        bad = np.argwhere(g != w)
        assert g.dtype == np.int64 and len(bad) == 0, (name, W, v, bad[:5].tolist(), [(int(g[tuple(b)]), int(w[tuple(b)])) for b in bad[:5]])
    if rows_route:
        ns = db.nearest_sets(ichr, qs, qe, off, W, value_filter=v)
        for g, w in zip(got[:3], ns[:3]):
            assert np.array_equal(g, w), (W, v)
    return want


def test_the_limit_is_where_two_workgroups_fit_a_cu():
    m = max_files()
    assert 28 * m + 12 <= 160 * 1024 // 2 < 28 * (m + 64) + 12


@pytest.mark.parametrize("which", ["1", "33", "65", "max-1", "max", "max+1"])
def test_file_counts_and_set_sizes(which, workdir):
    """1, 33, 65 files, both sides of the fused kernel's limit (max + 1 takes igd_nearest_rows + igd_nearest_reduce); sets of 0, 1,
    4, 5, sliceLen, sliceLen + 1 and 4 097 regions -- one wave, one workgroup, a second slice, a slice of one region -- with
    unknown contigs, zero-length and inverted regions among them"""
    from igd_amd import Database
    m = max_files()
    nfiles = {"max-1": m - 1, "max": m, "max+1": m + 1}.get(which) or int(which)
    rng = random.Random(9200 + nfiles)
    nbp = 1 << 12
    span = 40 * nbp
    ldb = ListDb(workdir, "f%d" % nfiles, sparse_lists(rng, nbp, nfiles, 2 if nfiles > 100 else 9, span), nbp, 1)
    sizes = [0, 1, 4, 5, 64, 65, 0, 4097]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert slice_len(int(off[-1])) == 64
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, int(off[-1]))
    db = Database(ldb.path)
    try:
        assert db.nfiles == nfiles
        hit = far = False
        for W, v in ((0, None), (700, 500), (3 * nbp + 5, None), (MAX_WINDOW, None), (MAX_WINDOW, 500)) if nfiles < 100 else \
                ((700, None), (MAX_WINDOW, 500)):
            want = check_fused(db, ldb, ichr, qs, qe, off, W, v)
            hit |= bool(want[0].any())
            far |= bool(want[2].any())
            assert not want[0][0].any() and not want[0][6].any()
        assert hit and far
    finally:
        db.close()


def test_placed_cases_and_the_filter_picks_the_farther_record(workdir):
    from igd_amd import Database
    nbp = 1 << 14
    ldb = placed_db(workdir, nbp, "fplaced")
    (ichr, qs, qe), _ = placed_regions(nbp)
    n = len(qs)
    db = Database(ldb.path)
    try:
        for W in (0, 1, nbp, 2 * nbp, 500, MAX_WINDOW):
            for v in (None, 500):
                check_fused(db, ldb, ichr, qs, qe, [0, n], W, v)
                check_fused(db, ldb, ichr, qs, qe, np.arange(n + 1), W, v)
        # f1, region [50000, 50100): the nearer record (d = 11) fails -v 500, the farther one (d = 301) passes
        a = db.nearest_sets_fused(ichr[3:4], qs[3:4], qe[3:4], [0, 1], 500).sum_dist[0, 1]
        b = db.nearest_sets_fused(ichr[3:4], qs[3:4], qe[3:4], [0, 1], 500, value_filter=500).sum_dist[0, 1]
        assert (a, b) == (11, 301)
    finally:
        db.close()


def test_workgroups_take_further_slices_with_cleared_accumulators(workdir):
    """4 x grid + 3 slices (sets of one to three regions: a slice each): every workgroup takes a second, third and fourth slice and
    three take a fifth.  The first round's regions cover whole contigs (every file within reach, distance 0); an accumulator or a
    table that was not cleared would leak them into the later slices' rows."""
    from igd_amd import Database
    from igd_amd import _native as N
    rng = random.Random(9300)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 40, 2, 20)
    ldb = ListDb(workdir, "w", files, nbp, 1)
    ns = 4 * GRID + 3
    assert N.hip().igd_hip_nearest_fused_grid(ns) == GRID and N.hip().igd_hip_nearest_fused_grid(5) == 5 and N.hip().igd_hip_nearest_fused_grid(0) == 1
    sizes = [rng.choice([1, 2, 3]) for _ in range(ns)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ichr, qs, qe = mixed_regions(rng, 2, nbp, span, int(off[-1]))
    first = int(off[GRID])
    ichr[:first], qs[:first], qe[:first] = rng.choice([0, 1]), 0, span + 6 * nbp
    db = Database(ldb.path)
    try:
        for W, v in ((nbp, None), (300, 500)):
            want = check_fused(db, ldb, ichr, qs, qe, off, W, v)
            assert (want[1][:GRID, :-1].sum(axis=0) > 0).all() and (want[0][GRID:] == 0).any() and (want[2][GRID:] > 0).any()
    finally:
        db.close()


def test_the_sum_of_distances_needs_64_bits_in_lds(workdir):
    """one file with one record [0, 1) and 8 identical regions [2^30, 2^30 + 1) in one slice, W = 2^30: each lies 2^30 away and
    sum_dist = 2^33, which a 32-bit LDS sum gets wrong"""
    from igd_amd import Database
    ldb = ListDb(workdir, "s64", [[("chr1", 0, 1, 700)]], 1 << 14, 1)
    ichr = np.zeros(8, np.int32)
    qs = np.full(8, 1 << 30, np.int32)
    qe = qs + 1
    db = Database(ldb.path)
    try:
        want = check_fused(db, ldb, ichr, qs, qe, [0, 8], MAX_WINDOW)
        assert want[2].tolist() == [[1 << 33, 1 << 33]] and want[0].tolist() == [[8, 8]] and want[1].tolist() == [[0, 0]]
        want = check_fused(db, ldb, ichr, qs, qe, [0, 8], MAX_WINDOW - 1)
        assert not want[0].any()
    finally:
        db.close()


def test_the_packed_counts_hold_a_full_slice(workdir):
    """2^24 regions in one set are one chunk cut into slices of IGD_SETS_SLICE_MAX = 4 096; the first slice's regions all overlap the
    one file's record: n_within = n_overlap = 4 096 in one flush of one packed word.  The others lie on an unknown contig."""
    from igd_amd import Database
    from igd_amd import _native as N
    ldb = ListDb(workdir, "pk", [[("chr1", 100, 200, 700)]], 1 << 14, 1)
    n = 1 << 24
    assert N.hip().igd_hip_max_batch() == n and slice_len(n) == 4096
    ichr = np.full(n, -1, np.int32)
    qs = np.full(n, 150, np.int32)
    qe = np.full(n, 160, np.int32)
    ichr[:4096] = 0
    ichr[3 * 4096:3 * 4096 + 100] = 0                                      # a further slice: 100 regions, 50 bp away
    qs[3 * 4096:3 * 4096 + 100], qe[3 * 4096:3 * 4096 + 100] = 249, 260
    db = Database(ldb.path)
    try:
        got = db.nearest_sets_fused(ichr, qs, qe, [0, n], 1000, out=garbage((1, 2)))
        assert got.n_within.tolist() == [[4196, 4196]] and got.n_overlap.tolist() == [[4096, 4096]] and got.sum_dist.tolist() == [[5000, 5000]]
    finally:
        db.close()


SEAM = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import short_tmpdir
import nearest_ref as R
from igd_amd import Database
d = short_tmpdir("igs")
rng = random.Random(13)
nbp = 1 << 12
files, span = R.clustered_lists(rng, nbp, 40, 2, 20)
ldb = R.ListDb(d, "b", files, nbp, 1)
db = Database(ldb.path)
sizes = [0, 1, 5, 700, 0, 1100, 3]
off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
ichr, qs, qe = R.mixed_regions(rng, 2, nbp, span, int(off[-1]))
for W, v in ((nbp, None), (3 * nbp + 5, 500), (0, None)):
    want = R.ref_sets(*R.ref_rows(ldb, ichr, qs, qe, W, v), off)
    out = [np.full((len(sizes), 41), 0x5a5a5a5a, np.int64) for _ in range(3)]
    ns = db.nearest_sets_fused(ichr, qs, qe, off, W, value_filter=v, out=out)
    for got, ref in zip(ns[:3], want):
        assert np.array_equal(got, ref), (W, v)
    assert ns.n_within[3].any() and ns.n_within[5].any() and not ns.n_within[0].any()
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


def child(script, env):
    p = subprocess.run([sys.executable, "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env), timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "97"}, {"IGD_HIP_SETS_ROW_BYTES": "2000"},
                                 {"IGD_HIP_MAX_BATCH": "333", "IGD_HIP_SETS_ROW_BYTES": "2000"}])
def test_sets_cut_by_a_chunk_seam_and_groups_of_two_sets(env):
    """chunks of 97 and of 333 regions: the sets of 700 and 1 100 regions are cut by chunk seams that are no multiple of 64; groups
    of two sets (a budget of 2 000 bytes against three rows of 41 x 8).  The variables are read once per process: a child each."""
    child(SEAM, env)


# ---- the permutation null ---------------------------------------------------------------------------------------------------
def composition(db, ichr, qs, qe, ctg_len, nperm, W, seed, mode, v):
    """what there was before: permute_regions, then nearest_sets on the explicit lists"""
    nq = len(qs)
    ps, pe = db.permute_regions(ichr, qs, qe, ctg_len, 0, nperm, seed=seed, mode=mode)
    c = np.tile(ichr, nperm + 1)
    s = np.concatenate([qs, ps.reshape(-1)])
    e = np.concatenate([qe, pe.reshape(-1)])
    return db.nearest_sets(c, s, e, np.arange(nperm + 2, dtype=np.int64) * nq, W, value_filter=v)


def null_fixture(workdir, name, nfiles, nq, seed):
    rng = random.Random(seed)
    nbp = 1 << 12
    if nfiles <= 100:
        files, span = clustered_lists(rng, nbp, nfiles, 2, 20)
        nctg = 2
    else:
        span, nctg = 40 * nbp, 1
        files = sparse_lists(rng, nbp, nfiles, 2, span)
    ldb = ListDb(workdir, name, files, nbp, 1)
    ctg_len = np.array([span + 9 * nbp + 11 * c for c in range(nctg)], np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, nq)
    return ldb, nbp, ctg_len, ichr, qs, qe


def check_null(db, ldb, ichr, qs, qe, ctg_len, nperm, W, seed, mode, v, ref=True):
    got = db.permutation_nearest(ichr, qs, qe, ctg_len, nperm, W, seed=seed, mode=mode, value_filter=v,
                                 out=garbage((nperm + 1, db.nfiles + 1)))
    assert got.nperm == nperm and got.window == W
    comp = composition(db, ichr, qs, qe, ctg_len, nperm, W, seed, mode, v)
    host = igd_amd.permute_nearest_host(ldb.path, ichr, qs, qe, ctg_len, nperm, W, seed=seed, mode=mode, value_filter=v)
    for i in range(3):
        assert got[i].dtype == np.int64 and np.array_equal(got[i], comp[i]), (i, nperm, W, mode, v)
        assert np.array_equal(got[i], host[i]), (i, nperm, W, mode, v)
    if ref:
        for g, w in zip(got[:3], PN.null(ldb, ichr, qs, qe, ctg_len, nperm, W, seed, mode, v)):
            assert np.array_equal(g, w), (nperm, W, mode, v)
    return got


@pytest.mark.parametrize("mode", [PR.CIRCULAR, PR.SHUFFLE])
def test_null_equals_the_composition_the_host_route_and_the_definition(mode, workdir):
    from igd_amd import Database
    ldb, nbp, ctg_len, ichr, qs, qe = null_fixture(workdir, "n" + mode, 40, 150, 9400)
    db = Database(ldb.path)
    try:
        moved = False
        for nperm in (1, 5, 64):
            for W, v in ((nbp, None), (0, 500), (MAX_WINDOW, None), (700, 500)):
                got = check_null(db, ldb, ichr, qs, qe, ctg_len, nperm, W, 3 + nperm, mode, v)
                moved |= bool((got.sum_dist[1:] != got.sum_dist[0]).any())
        assert moved
        # one region, and a set of regions on unknown contigs only
        check_null(db, ldb, ichr[:1], qs[:1], qe[:1], ctg_len, 5, nbp, 1, mode, None)
        unk = np.flatnonzero((ichr < 0) | (ichr >= len(ctg_len)))
        got = check_null(db, ldb, ichr[unk], qs[unk], qe[unk], ctg_len, 3, nbp, 1, mode, None)
        assert len(unk) and not got.n_within.any()
    finally:
        db.close()


def test_null_above_the_fused_limit_takes_the_rows_route(workdir):
    from igd_amd import Database
    m = max_files()
    ldb, nbp, ctg_len, ichr, qs, qe = null_fixture(workdir, "nbig", m + 1, 40, 9500)
    db = Database(ldb.path)
    try:
        assert db.nfiles == m + 1
        for mode, W, v in ((PR.CIRCULAR, 3 * nbp, None), (PR.SHUFFLE, MAX_WINDOW, 500)):
            got = check_null(db, ldb, ichr, qs, qe, ctg_len, 5, W, 7, mode, v)
            assert got.n_within.any()
    finally:
        db.close()


CHUNKS = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import short_tmpdir
import nearest_ref as R, permute_ref as PR, permute_nearest_ref as PN
from igd_amd import Database
from igd_amd.database import IgdError
d = short_tmpdir("igc")
rng = random.Random(14)
nbp = 1 << 12
files, span = R.clustered_lists(rng, nbp, 40, 2, 20)
ldb = R.ListDb(d, "b", files, nbp, 1)
ctg_len = np.array([span + 9 * nbp, span + 5 * nbp + 3], np.int32)
ichr, qs, qe = PR.random_regions(rng, ctg_len, 100)
db = Database(ldb.path)
for mode, W, v in ((PR.CIRCULAR, nbp, None), (PR.SHUFFLE, 3 * nbp + 5, 500)):
    want = PN.null(ldb, ichr, qs, qe, ctg_len, 7, W, 21, mode, v)
    out = [np.full((8, 41), 0x5a5a5a5a, np.int64) for _ in range(3)]
    got = db.permutation_nearest(ichr, qs, qe, ctg_len, 7, W, seed=21, mode=mode, value_filter=v, out=out)
    for g, w in zip(got[:3], want):
        assert np.array_equal(g, w), (mode, W, v)
    assert got.n_within[1:].any()
if os.environ.get("IGD_HIP_MAX_BATCH") == "100":
    # more regions than a batch: refused, nothing written
    c2, s2, e2 = np.append(ichr, ichr[:1]), np.append(qs, qs[:1]), np.append(qe, qe[:1])
    out = [np.full((3, 41), 0x5a5a5a5a, np.int64) for _ in range(3)]
    try:
        db.permutation_nearest(c2, s2, e2, ctg_len, 2, nbp, out=out)
        raise SystemExit("101 regions were accepted")
    except IgdError:
        pass
    assert all((a == 0x5a5a5a5a).all() for a in out)
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "100"}, {"IGD_HIP_PERM_ROW_BYTES": str(3 * 41 * 8)},
                                 {"IGD_HIP_MAX_BATCH": "305"}, {"IGD_HIP_PERM_ROW_BYTES": str(3 * 3 * 41 * 8 + 8)}])
def test_null_in_chunks_of_one_and_of_three_permutations(env):
    """7 permutations of 100 regions in chunks of 1 and of 3 + 3 + 1, by the batch limit (100 and 305 regions) and by the row budget
    (three rows of 41 words, and nine and a word).  The variables are read once per process: a child process each."""
    child(CHUNKS, env)


def test_bad_arguments_leave_the_callers_arrays_untouched(workdir):
    from igd_amd import Database
    from igd_amd.database import IgdError
    ldb, nbp, ctg_len, ichr, qs, qe = null_fixture(workdir, "bad", 3, 20, 9600)
    db = Database(ldb.path)
    try:
        known = np.flatnonzero((ichr >= 0) & (ichr < len(ctg_len)))
        e_out, s_neg, inv = qe.copy(), qs.copy(), qe.copy()
        e_out[known[0]] = ctg_len[ichr[known[0]]] + 1
        s_neg[known[1]] = -1
        inv[known[2]] = qs[known[2]] - 1
        zero_len = ctg_len.copy()
        zero_len[ichr[known[0]]] = 0
        cases = [dict(nperm=0), dict(nperm=(1 << 20) + 1), dict(window=-1), dict(window=MAX_WINDOW + 1), dict(qe=e_out), dict(qs=s_neg),
                 dict(qe=inv), dict(ctg_len=zero_len)]
        for case in cases:
            a = dict(dict(qs=qs, qe=qe, ctg_len=ctg_len, nperm=3, window=100), **case)
            out = garbage((max(a["nperm"], 0) + 1, 4))
            with pytest.raises(IgdError):
                db.permutation_nearest(ichr, a["qs"], a["qe"], a["ctg_len"], a["nperm"], a["window"], out=out)
            assert all((x == GARBAGE).all() for x in out), case
            assert igd_amd._native.hip().igd_hip_last_error(), case
        for W in (-1, MAX_WINDOW + 1):
            out = garbage((1, 4))
            with pytest.raises(IgdError):
                db.nearest_sets_fused(ichr, qs, qe, [0, 20], W, out=out)
            assert all((x == GARBAGE).all() for x in out)
        for off in ([1, 20], [0, 15, 10, 20]):
            with pytest.raises(IgdError):
                db.nearest_sets_fused(ichr, qs, qe, off, 100)
        # empty calls: all zeros
        z = np.zeros(0, np.int32)
        got = db.permutation_nearest(z, z, z, ctg_len, 4, 100, out=garbage((5, 4)))
        assert all(a.shape == (5, 4) and not a.any() for a in got[:3])
        ns = db.nearest_sets_fused(z, z, z, [0, 0, 0], 100, out=garbage((2, 4)))
        assert all(a.shape == (2, 4) and not a.any() for a in ns[:3])
        ns = db.nearest_sets_fused(ichr, qs, qe, [0, 0, 20, 20], MAX_WINDOW, out=garbage((3, 4)))
        assert not ns.n_within[0].any() and not ns.n_within[2].any() and ns.n_within[1].any()
    finally:
        db.close()


@pytest.mark.parametrize("extra", [[], ["-v", "500", "-M", "shuffle", "-S", "9"]])
def test_cli_engine_route_prints_what_the_host_route_prints(extra, workdir):
    d = os.path.join(workdir, "cli%d" % len(extra))
    os.makedirs(d)
    ldb, nbp, ctg_len, ichr, qs, qe = null_fixture(d, "db", 9, 300, 9700)
    keep = (qe > 0) & (ichr >= 0) & (ichr < 2)
    q = os.path.join(d, "q.bed")
    write_bed(q, [(ldb.ctgs[c], int(s), int(e)) for c, s, e in zip(ichr[keep], qs[keep], qe[keep])] + [("chrNotThere", 5, 50)])
    g = os.path.join(d, "genome.sizes")
    with open(g, "w") as f:
        f.write("".join("%s\t%d\n" % (ldb.ctgs[c], ctg_len[c]) for c in range(2)))
    for W in ("0", str(nbp), str(MAX_WINDOW)):
        args = ["search", ldb.path, "-q", q, "-P", "6", "-g", g, "-D", W] + extra
        want = _run(args, HOST)
        got = _run(args)                                              # (IGD_HOST_MAX_QUERIES = 0: the engine)
        assert want.returncode == 0 and got.returncode == 0, got.stderr
        assert got.stdout == want.stdout and got.stdout.startswith(PN.HEADER.encode()), args
