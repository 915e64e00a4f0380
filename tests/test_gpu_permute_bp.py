"""The permutation null of the base-pair overlap on the device: igd_hip_permute_bp (kernels igd_merge_slices and
igd_merge_row_bp between the merge launches and igd_sets_coverage) against tests/permute_bp_ref.py (permute_ref's generator,
jaccard_ref's sort, sweep and boolean arrays over the interval lists this test wrote) AND against the host route
(igdc_permute_bp_host).  Every integer must be equal; outputs are handed over full of 0x5a.

The shapes are the smallest at which the hand-over can go wrong.  A row of nq regions gets ceil(nq / sliceLen) slice slots,
sliceLen at its floor of 64 here, whatever the merge makes of it: rows of 1, 63, 64, 65, 128 and 129 regions; a set whose every
region is dropped (every slot empty); a set that merges into one run (one slot filled, the others empty); rows of exactly 64 and
65 runs beside rows of the other number (no slot may reach into the next row's runs).  Chunk seams and a one-workgroup grid
run in child processes, because their variables are read once per process."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import igd_amd
import igd_amd.database
import permute_bp_ref as PB
import permute_ref as PR
import sets_fixtures as F
from helpers import ROOT, short_tmpdir, write_bed
from jaccard_ref import FLAT, NEST
from nearest_ref import NOV, ListDb, sparse_lists
from test_jaccard_host import cli_rule
from test_permute_bp_host import NUMPY_DBS, equal_null, fixture_db
from test_support_host import HOST, _run

pytestmark = pytest.mark.gpu

G64 = 0x5a5a5a5a5a5a5a5a
SLICE_MIN = 64


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igb")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _p(a):
    return a.ctypes.data if a.size else None


def dev_null(db, ichr, qs, qe, ctg_len, nperm, seed, mode, ev, rule, rows=None):
    """igd_hip_permute_bp through ctypes, the outputs full of 0x5a: (rc, inter, set_bp, n_merged, n_dropped array of one)"""
    ichr, qs, qe, ctg_len = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe, ctg_len))
    rows = nperm + 1 if rows is None else rows
    inter, sbp, nm, nd = np.full((rows, db.nfiles + 1), G64, np.int64), np.full(rows, G64, np.int64), np.full(rows, G64, np.int64), np.full(1, G64, np.int64)
    rc = db._H.igd_hip_permute_bp(db.dev, _p(ichr), _p(qs), _p(qe), len(qs), _p(ctg_len), {"circular": 0, "shuffle": 1}.get(mode, mode),
                                  seed & (2 ** 64 - 1), nperm, ev, rule, inter.ctypes.data, sbp.ctypes.data, nm.ctypes.data, nd.ctypes.data)
    return rc, inter, sbp, nm, nd


def check(D, ldb, ichr, qs, qe, ctg_len, nperm, seed=0, mode=PR.CIRCULAR, ev=NOV, rule=FLAT):
    """the device against the reference and against the host route; returns the PermutationBp"""
    want = PB.null(ldb, ichr, qs, qe, ctg_len, nperm, seed, mode, ev, rule)
    rc, inter, sbp, nm, nd = dev_null(D, ichr, qs, qe, ctg_len, nperm, seed, mode, ev, rule)
    assert rc == 0
    assert np.array_equal(inter, want[0]) and np.array_equal(sbp, want[1]) and np.array_equal(nm, want[2]) and nd[0] == want[3]
    got = D.permutation_bp(ichr, qs, qe, ctg_len, nperm, seed=seed, mode=mode, rule=rule, value_filter=ev)
    assert equal_null(got, want)
    host = igd_amd.permute_bp_host(ldb.path, ichr, qs, qe, ctg_len, nperm, seed=seed, mode=mode, rule=rule, value_filter=ev)
    assert all(np.array_equal(g, h) for g, h in zip(got[:3], host[:3])) and got.n_dropped == host.n_dropped and np.array_equal(got.file_bp, host.file_bp)
    # the identities
    nf = ldb.nfiles
    assert (got.inter <= np.minimum(got.set_bp[:, None], got.file_bp[None, :])).all()
    assert (got.inter[:, :nf].max(axis=1) <= got.inter[:, nf]).all() and (got.inter[:, nf] <= got.set_bp).all()
    return got


# ---- the hand-over ----------------------------------------------------------------------------------------------------------
def handover_db(d):
    """chrA with records all along it in five files; chrB, 25 bp for the generator, with two short records"""
    rng = random.Random(5)
    files = [[("chrA", s, s + rng.randint(50, 3000), rng.choice([100, 900])) for s in (rng.randrange(0, 900000) for _ in range(60))] for _ in range(5)]
    files[1] += [("chrB", 3, 9, 900), ("chrB", 12, 20, 900)]
    ldb = ListDb(d, "hand", files, 1 << 12, 1)
    assert ldb.ctgs == ["chrA", "chrB"]
    return ldb


@pytest.fixture(scope="module")
def hand(workdir):
    ldb = handover_db(workdir)
    D = igd_amd.Database(ldb.path, device=0)
    yield ldb, D, np.array([1000000, 25], np.int32)
    D.close()


def test_slots_per_row_follow_the_formula(hand):
    H = hand[1]._H
    c = F.consts()
    assert c["IGD_SETS_SLICE_MIN"] == SLICE_MIN
    for pc, nq in ((1, 1), (6, 63), (6, 64), (6, 65), (6, 128), (6, 129), (1000, 10000), (40, 100000), (3, 4000000), (1, 1 << 24), (7, 1 << 22)):
        sl = min(max(-(-pc * nq // c["IGD_SETS_SLICES"]), c["IGD_SETS_SLICE_MIN"]), c["IGD_SETS_SLICE_MAX"])
        assert H.igd_hip_merge_slices_per_row(pc, nq) == -(-nq // sl), (pc, nq)
    assert H.igd_hip_merge_slices_per_row(0, 5) == 0 and H.igd_hip_merge_slices_per_row(5, 0) == 0


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 128, 129])
def test_rows_around_the_slice_length(nq, hand):
    """nq one-bp regions far apart on chrA: a circular shift keeps them apart (a region of one bp is never pushed back), so every
    row has nq runs and fills its slots to the last: 1, 63, 64, 65, 128, 129 runs in 1, 1, 1, 2, 2, 3 slots"""
    ldb, D, ctg_len = hand
    qs = (np.arange(nq, dtype=np.int32) * 7001 + 13)
    got = check(D, ldb, np.zeros(nq, np.int32), qs, qs + 1, ctg_len, 5, seed=nq)
    assert (got.n_merged == nq).all() and (got.set_bp == nq).all()
    assert D._H.igd_hip_merge_slices_per_row(5, nq) == -(-nq // SLICE_MIN)
    # longer regions, placed anew: rows of different numbers of runs below nq
    rng = random.Random(nq)
    qe = qs + np.array([rng.choice([1, 300, 9000, 40000]) for _ in range(nq)], np.int32)
    got = check(D, ldb, np.zeros(nq, np.int32), qs, qe, ctg_len, 5, seed=nq, mode=PR.SHUFFLE, ev=500)
    assert got.inter.sum() > 0 and (nq < 63 or len(set(got.n_merged.tolist())) > 1)


def test_every_region_dropped_and_no_region(hand):
    ldb, D, ctg_len = hand
    n = 129
    ichr = np.array([-1, 2, 0] * (n // 3), np.int32)                 # unknown contigs and zero-length regions: every slot of every row is empty
    qs = np.arange(n, dtype=np.int32) * 100
    qe = np.where(ichr == 0, qs, qs + 50).astype(np.int32)
    for mode in (PR.CIRCULAR, PR.SHUFFLE):
        got = check(D, ldb, ichr, qs, qe, ctg_len, 4, seed=2, mode=mode)
        assert not got.inter.any() and not got.set_bp.any() and not got.n_merged.any() and got.n_dropped == n
    z = np.zeros(0, np.int32)
    rc, inter, sbp, nm, nd = dev_null(D, z, z, z, ctg_len, 4, 0, PR.CIRCULAR, NOV, FLAT)
    assert rc == 0 and not inter.any() and not sbp.any() and not nm.any() and nd[0] == 0


def test_a_row_that_merges_into_one_run(hand):
    """129 regions nested in the first: three slots per row, row 0 fills one run into the first and leaves two empty"""
    ldb, D, ctg_len = hand
    rng = random.Random(3)
    qs = np.array([100000] + [rng.randrange(100000, 590000) for _ in range(128)], np.int32)
    qe = np.array([600000] + [s + rng.randint(1, 9000) for s in qs[1:]], np.int32)
    got = check(D, ldb, np.zeros(129, np.int32), qs, qe, ctg_len, 5, seed=9)
    assert got.n_merged[0] == 1 and got.set_bp[0] == 500000 and got.inter[0, ldb.nfiles] > 0
    got = check(D, ldb, np.zeros(129, np.int32), qs, qe, ctg_len, 5, seed=9, mode=PR.SHUFFLE)
    assert got.n_merged[0] == 1 and (got.n_merged[1:] > 1).any()


@pytest.mark.parametrize("sparse", [62, 63])
def test_rows_of_exactly_one_slice_and_one_more_beside_shorter_ones(sparse, hand):
    """`sparse` one-bp regions on chrA stay `sparse` runs in every row; [5, 15) and [15, 25) on the 25 bp of chrB are one run as
    given and one or two under a shift: rows of sparse + 1 and sparse + 2 runs -- 63 / 64, then 64 / 65 -- side by side, in two
    slots each."""
    ldb, D, ctg_len = hand
    qs = np.concatenate([np.arange(sparse, dtype=np.int32) * 9001 + 77, [5, 15]]).astype(np.int32)
    qe = np.concatenate([qs[:sparse] + 1, [15, 25]]).astype(np.int32)
    ichr = np.concatenate([np.zeros(sparse, np.int32), [1, 1]]).astype(np.int32)
    got = check(D, ldb, ichr, qs, qe, ctg_len, 24, seed=4)
    assert got.n_merged[0] == sparse + 1 and set(got.n_merged.tolist()) == {sparse + 1, sparse + 2}
    change = np.flatnonzero(np.diff(got.n_merged))
    assert len(change) >= 2, "fixture is vacuous: no row beside one of another length"
    assert (got.set_bp[got.n_merged == sparse + 2] == sparse + 20).all() and (got.set_bp < sparse + 20).any()


# ---- the four database shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_device_equals_the_reference_and_the_host_route_on_the_four_database_shapes(case, workdir):
    ldb, ctg_len, ichr, qs, qe = fixture_db(workdir, case, 200)
    D = igd_amd.Database(ldb.path, device=0)
    try:
        for nperm, seed in ((1, 0), (6, 17), (6, 2 ** 64 - 1)):
            for mode in (PR.CIRCULAR, PR.SHUFFLE):
                for v in (0, 500):
                    rule, ev = cli_rule(ldb.gtype, v)
                    got = check(D, ldb, ichr, qs, qe, ctg_len, nperm, seed, mode, ev, rule)
                    if seed != 17:
                        continue
                    check(D, ldb, ichr, qs, qe, ctg_len, nperm, seed, mode, NOV, FLAT if rule == NEST else NEST)
                    # the composition through the calls that were there before: row 0 and the permuted rows as jaccard_sets' sets
                    js = D.jaccard_sets(ichr, qs, qe, [0, len(qs)], rule=rule, value_filter=ev)
                    assert np.array_equal(js.inter[0], got.inter[0]) and js.set_bp[0] == got.set_bp[0] and js.n_merged[0] == got.n_merged[0]
                    assert js.n_dropped[0] == got.n_dropped and np.array_equal(js.file_bp, got.file_bp)
                    ps, pe = D.permute_regions(ichr, qs, qe, ctg_len, 0, nperm, seed=seed, mode=mode)
                    jp = D.jaccard_sets(np.tile(ichr, nperm), ps.reshape(-1), pe.reshape(-1), np.arange(nperm + 1) * len(qs), rule=rule, value_filter=ev)
                    assert np.array_equal(jp.inter, got.inter[1:]) and np.array_equal(jp.set_bp, got.set_bp[1:])
                    assert np.array_equal(jp.n_merged, got.n_merged[1:]) and (jp.n_dropped == got.n_dropped).all()
        assert got.inter.sum() > 0 and got.n_dropped > 0 and len(set(got.set_bp.tolist())) > 1, "fixture is vacuous"
        # the same seed gives the same bytes
        a = dev_null(D, ichr, qs, qe, ctg_len, 6, 17, PR.SHUFFLE, NOV, FLAT)
        b = dev_null(D, ichr, qs, qe, ctg_len, 6, 17, PR.SHUFFLE, NOV, FLAT)
        assert a[0] == b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
        c = dev_null(D, ichr, qs, qe, ctg_len, 6, 18, PR.SHUFFLE, NOV, FLAT)
        assert c[1].tobytes() != a[1].tobytes()
        # the CLI's dispatch through v alone
        rule, ev = cli_rule(ldb.gtype, 500)
        assert equal_null(D.permutation_bp(ichr, qs, qe, ctg_len, 3, seed=5, v=500), PB.null(ldb, ichr, qs, qe, ctg_len, 3, 5, PR.CIRCULAR, ev, rule))
    finally:
        D.close()


# ---- the first wide form ----------------------------------------------------------------------------------------------------
def test_2041_files_take_the_wide_form_of_the_coverage_kernel(workdir):
    """2 041 files are the first database whose frontier words lie in global stripes under rising tags; the tags of a chunk are
    budgeted by rows x nq, the most runs it can hold.  Two calls on one handle: the second starts from the tags the first left."""
    nfiles = F.consts()["IGD_COVERAGE_LDS_FILES"] + 1
    assert nfiles == 2041
    rng = random.Random(2041)
    span = 24000
    ldb = ListDb(workdir, "wide", sparse_lists(rng, 1 << 10, nfiles, 3, span), 1 << 10, 1)
    ctg_len = np.array([span + 5000], np.int32)
    ichr, qs, qe = PR.random_regions(rng, ctg_len, 130)
    D = igd_amd.Database(ldb.path, device=0)
    try:
        got = check(D, ldb, ichr, qs, qe, ctg_len, 4, seed=1)
        assert (got.inter[:, :nfiles] > 0).any(axis=1).all() and got.inter.shape == (5, nfiles + 1)
        check(D, ldb, ichr, qs, qe, ctg_len, 3, seed=2, mode=PR.SHUFFLE, ev=500)
    finally:
        D.close()


# ---- chunk seams and a grid of one workgroup, in child processes ---------------------------------------------------------------
CHILD = r"""
import os, shutil, sys
import numpy as np
sys.path.insert(0, os.path.join(%r, "tests"))
from helpers import short_tmpdir
import igd_amd
import permute_bp_ref as PB
from test_permute_bp_host import fixture_db, equal_null
nq, nperm, one_chunk = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
d = short_tmpdir("igc")
try:
    ldb, ctg_len, ichr, qs, qe = fixture_db(d, 0, nq)
    D = igd_amd.Database(ldb.path, device=0)
    for k, mode in enumerate(("circular", "shuffle")):
        got = D.permutation_bp(ichr, qs, qe, ctg_len, nperm, seed=11, mode=mode, v=500 * k)
        with np.load(one_chunk) as z:
            assert all(np.array_equal(got[i], z["m%%d_%%d" %% (k, i)]) for i in (0, 1, 2, 4)) and got.n_dropped == int(z["m%%d_3" %% k]), mode
        assert equal_null(got, PB.null(ldb, ichr, qs, qe, ctg_len, nperm, 11, mode, 500 if k else -2 ** 31, k))
        host = igd_amd.permute_bp_host(ldb.path, ichr, qs, qe, ctg_len, nperm, seed=11, mode=mode, v=500 * k)
        assert all(np.array_equal(got[i], host[i]) for i in (0, 1, 2, 4)) and got.n_dropped == host.n_dropped
    D.close()
    print("ok")
finally:
    shutil.rmtree(d, ignore_errors=True)
""" % ROOT


@pytest.mark.parametrize("env,nq,nperm", [({"IGD_HIP_MAX_BATCH": "350"}, 100, 7), ({"IGD_HIP_PERM_ROW_BYTES": str(3 * 7 * 8)}, 100, 7),
                                          ({"IGD_HIP_MAX_BATCH": "250", "IGD_HIP_PERM_ROW_BYTES": str(3 * 7 * 8)}, 100, 7),
                                          ({"IGD_HIP_MERGE_GRID": "1"}, 70, 300)])
def test_chunk_seams_and_a_grid_of_one_workgroup(env, nq, nperm, workdir):
    """7 permutations of 100 regions in chunks of three (350 regions of staging, or rows of three times 7 files), of two (250
    regions), the last chunk shorter; the table must be the one-chunk table of this process.  A grid of one workgroup of 256
    threads: 300 rows of two slots are three rounds of igd_merge_slices and 75 of igd_merge_row_bp's four waves."""
    assert not any(k in os.environ for k in ("IGD_HIP_MAX_BATCH", "IGD_HIP_PERM_ROW_BYTES", "IGD_HIP_MERGE_GRID"))
    ldb, ctg_len, ichr, qs, qe = fixture_db(workdir, 0, nq)
    assert ldb.nfiles == 7
    D = igd_amd.Database(ldb.path, device=0)
    try:
        save = {}
        for k, mode in enumerate(("circular", "shuffle")):
            got = D.permutation_bp(ichr, qs, qe, ctg_len, nperm, seed=11, mode=mode, v=500 * k)
            save.update({"m%d_%d" % (k, i): np.asarray(got[i]) for i in range(5)})
    finally:
        D.close()
    one_chunk = os.path.join(workdir, "one_%d_%d.npz" % (nq, nperm))
    np.savez(one_chunk, **save)
    p = subprocess.run([sys.executable, "-c", CHILD, str(nq), str(nperm), one_chunk], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **env), timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


# ---- the command line and the refusals --------------------------------------------------------------------------------------
def test_cli_G_on_both_routes_byte_for_byte(workdir):
    d = os.path.join(workdir, "cli")
    os.makedirs(d)
    ldb, ctg_len, ichr, qs, qe = fixture_db(d, 0, 150)
    keep = (ichr >= 0) & (ichr < len(ctg_len)) & (qe > 0)
    bed, g = os.path.join(d, "q.bed"), os.path.join(d, "genome.sizes")
    write_bed(bed, [(ldb.ctgs[c], int(s), int(e)) for c, s, e in zip(ichr[keep], qs[keep], qe[keep])])
    with open(g, "w") as f:
        f.write("".join("%s\t%d\n" % (n, L) for n, L in zip(ldb.ctgs, ctg_len)))
    for extra in ([], ["-v", "500", "-M", "shuffle", "-S", "9"]):
        args = ["search", ldb.path, "-q", bed, "-P", "12", "-g", g, "-G"] + extra
        want = _run(args, HOST)
        got = _run(args)                                      # (IGD_HOST_MAX_QUERIES = 0: the engine)
        assert want.returncode == 0 and got.returncode == 0, got.stderr
        assert got.stdout == want.stdout and got.stdout.startswith(b"index\tobserved_bp\tmean\t") and b"Any dataset: " in got.stdout, args
        rule, ev = cli_rule(ldb.gtype, 500 if extra else 0)
        null = PB.null(ldb, ichr[keep], qs[keep], qe[keep], ctg_len, 12, 9 if extra else 0, PR.SHUFFLE if extra else PR.CIRCULAR, ev, rule)
        assert got.stdout.decode() == PB.table_text(ldb.names, *null)


def test_refused_arguments_write_nothing(hand):
    ldb, D, ctg_len = hand
    ichr, qs, qe = np.array([0, 1], np.int32), np.array([10, 5], np.int32), np.array([500, 15], np.int32)
    ok = dict(qe=qe, mode=0, nperm=3, rule=FLAT)
    e2 = np.array([500, 26], np.int32)
    for bad in (dict(nperm=0), dict(nperm=(1 << 20) + 1), dict(mode=2), dict(rule=7), dict(qe=e2), dict(qe=np.array([5, 15], np.int32))):
        a = dict(ok, **bad)
        rc, inter, sbp, nm, nd = dev_null(D, ichr, qs, a["qe"], ctg_len, a["nperm"], 0, a["mode"], NOV, a["rule"], rows=4)
        assert rc == -2 and all((x == G64).all() for x in (inter, sbp, nm, nd)), bad
    from igd_amd.database import IgdError
    with pytest.raises(IgdError):
        D.permutation_bp(ichr, qs, qe, ctg_len[:1], 3)
    with pytest.raises(IgdError):
        D.permutation_bp(ichr, qs, qe, ctg_len, 3, mode="rotate")
    # NULL outputs are allowed, one at a time
    H = D._H
    sbp = np.full(4, G64, np.int64)
    assert H.igd_hip_permute_bp(D.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, 2, ctg_len.ctypes.data, 0, 0, 3, NOV, FLAT, None,
                                sbp.ctypes.data, None, None) == 0
    assert sbp[0] == 500 and (sbp <= 500).all() and (sbp >= 490).all()
