"""Merged region sets and the base-pair Jaccard on the device: igd_hip_merge_sets / _dev, igd_hip_dataset_bp and
igd_hip_jaccard_sets against tests/jaccard_ref.py (the definitions over the interval lists this test wrote) and against the host
route.  Every integer must be equal; outputs are handed over full of 0x5a.  The merge sizes sit around the constants of the
scan and the sort (read from the source), the carry cases aim at the segmented scan's hand-over between waves and tiles."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import igd_amd
import igd_amd.database
from helpers import ROOT, short_tmpdir
from jaccard_ref import MAX_GAP, ref_dataset_bp, ref_jaccard, ref_merge, ref_merge_np
from nearest_ref import TOP, ListDb, sparse_lists
from test_jaccard_cli import db_and_beds
from test_jaccard_host import G32, G64, NUMPY_DBS, PLACED, JaccardHost, _p, cli_rule, cut_merge, merge_equal, placed_arrays, shape_case, two_contig_db
from test_sets_cli import _write_list
from test_support_host import HOST, _run

pytestmark = pytest.mark.gpu


def constants():
    src = open(os.path.join(ROOT, "igd_amd", "csrc", "igd_sortscan.hpp")).read()
    g = lambda name: int(re.search(r"^#define\s+%s\s+(\d+)" % name, src, re.M).group(1))       # noqa: E731
    return g("SCAN_WG") * g("SCAN_PER"), g("RS_WG") * g("RS_STRIPS")


SCAN_TILE, RS_BLOCK = constants()


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igj")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def placed(workdir):
    db = igd_amd.Database(two_contig_db(workdir).path, device=0)
    yield db
    db.close()


def dev_merge(db, ichr, qs, qe, off, gap=0, want_count=True):
    """igd_hip_merge_sets through ctypes, the outputs full of 0x5a: what JaccardHost.merge returns"""
    ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
    off = np.ascontiguousarray(off, dtype=np.int64)
    n, nsets = len(qs), len(off) - 1
    mc, ms, me, cnt = (np.full(n, G32, np.int32) for _ in range(4))
    moff, dropped = np.full(nsets + 1, G64, np.int64), np.full(nsets, G64, np.int64)
    rc = db._H.igd_hip_merge_sets(db.dev, _p(ichr), _p(qs), _p(qe), off.ctypes.data, nsets, gap, _p(mc), _p(ms), _p(me), moff.ctypes.data,
                                  _p(cnt) if want_count else None, _p(dropped))
    return rc, mc, ms, me, moff, cnt, dropped


def dev_jaccard(db, ichr, qs, qe, off, v, rule):
    ichr, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (ichr, qs, qe))
    off = np.ascontiguousarray(off, dtype=np.int64)
    nsets = len(off) - 1
    inter, fbp = np.full((nsets, db.nfiles + 1), G64, np.int64), np.full(db.nfiles + 1, G64, np.int64)
    sbp, nm, nd = (np.full(nsets, G64, np.int64) for _ in range(3))
    rc = db._H.igd_hip_jaccard_sets(db.dev, _p(ichr), _p(qs), _p(qe), off.ctypes.data, nsets, v, rule, _p(inter), _p(sbp), fbp.ctypes.data, _p(nm), _p(nd))
    return rc, (inter, sbp, fbp, nm, nd)


def check_merge(db, nctg, ichr, qs, qe, off, gap=0, what=None):
    rc, got, rest = cut_merge(dev_merge(db, ichr, qs, qe, off, gap))
    want = ref_merge(nctg, ichr, qs, qe, off, gap)
    assert rc == 0 and merge_equal(got, want) and (rest == 0).all(), what
    return want


def test_placed_cases_and_refusals(placed):
    for case in PLACED:
        (ichr, qs, qe, off, gap), want = placed_arrays(case)
        rc, got, rest = cut_merge(dev_merge(placed, ichr, qs, qe, off, gap))
        assert rc == 0 and merge_equal(got, want) and (rest == 0).all(), case[0]
    rc, got, _ = cut_merge(dev_merge(placed, *placed_arrays(PLACED[0])[0], want_count=False))
    assert rc == 0 and (got[4] == G32).all() and got[3].tolist() == [0, 1]
    c, s, e = [0, 0], [0, 5], [10, 20]
    for off, gap in (([0, 2], -1), ([0, 2], MAX_GAP + 1), ([1, 2], 0), ([0, 2, 1], 0)):
        out = dev_merge(placed, c, s, e, off, gap)
        assert out[0] == -2 and all((a == G32).all() for a in (out[1], out[2], out[3], out[5])) and (out[4] == G64).all() and (out[6] == G64).all()
    rc, js = dev_jaccard(placed, c, s, e, [1, 2], -2 ** 31, 0)
    assert rc == -2 and all((a == G64).all() for a in js)
    # no sets, empty sets
    rc, js = dev_jaccard(placed, [], [], [], [0], -2 ** 31, 0)
    assert rc == 0 and js[2].tolist() == [200, 160, 310]
    rc, js = dev_jaccard(placed, [], [], [], [0, 0, 0], -2 ** 31, 0)
    assert rc == 0 and not js[0].any() and not js[1].any() and not js[3].any() and not js[4].any() and js[2].tolist() == [200, 160, 310]
    rc, got, _ = cut_merge(dev_merge(placed, [], [], [], [0, 0]))
    assert rc == 0 and got[3].tolist() == [0, 0] and got[5].tolist() == [0]


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_device_equals_the_reference_and_the_host_route_on_the_four_database_shapes(case, workdir):
    db, ichr, qs, qe, off = shape_case(case, workdir)
    H, D = JaccardHost(db.path), igd_amd.Database(db.path, device=0)
    try:
        for gap in (0, 1, 300, MAX_GAP):
            want = check_merge(D, len(db.ctgs), ichr, qs, qe, off, gap, gap)
            assert merge_equal(cut_merge(H.merge(ichr, qs, qe, off, gap))[1], want)
        for v in (0, 500):
            rule, ev = cli_rule(db.gtype, v)
            want = ref_jaccard(db, ichr, qs, qe, off, ev, rule)
            rc, got = dev_jaccard(D, ichr, qs, qe, off, ev, rule)
            assert rc == 0 and all(np.array_equal(g, w) for g, w in zip(got, want)), v
            assert all(np.array_equal(g, w) for g, w in zip(got, H.jaccard(ichr, qs, qe, off, ev, rule)[1])), v
            js = D.jaccard_sets(ichr, qs, qe, off, v=v)
            assert all(np.array_equal(g, w) for g, w in zip(js, want))
        m = D.merge_sets(ichr, qs, qe, off)
        cov, covered = D.coverage_sets(m[0], m[1], m[2], m[3], v=500)
        assert np.array_equal(cov, got[0][:, :db.nfiles]) and np.array_equal(covered, got[0][:, db.nfiles])
        assert (got[0] <= np.minimum(got[1][:, None], got[2][None, :])).all()
    finally:
        H.close()
        D.close()


def sized_sets(rng, sizes, span=2_000_000):
    """sets of the given sizes on two contigs: short regions, some nested, some book-ended, some far apart"""
    n = sum(sizes)
    ichr = np.array([rng.choice([0, 0, 1]) for _ in range(n)], np.int32)
    qs = np.array([rng.randrange(0, span) for _ in range(n)], np.int64)
    qe = qs + np.array([rng.choice([1, 30, 400, 5000]) for _ in range(n)], np.int64)
    return ichr, qs.astype(np.int32), qe.astype(np.int32), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_merge_sizes_around_the_scan_and_sort_constants(placed):
    rng = random.Random(9100)
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 0, RS_BLOCK - 1, RS_BLOCK, RS_BLOCK + 1]
    ichr, qs, qe, off = sized_sets(rng, sizes)
    assert len(qs) > 3 * max(SCAN_TILE, RS_BLOCK)          # (several tiles of the scan and blocks of the sort)
    for gap in (0, 1, MAX_GAP):
        check_merge(placed, 2, ichr, qs, qe, off, gap, gap)
    for size in sizes:                                     # each size alone: the last tile is ragged at that size
        a = sized_sets(rng, [size])
        check_merge(placed, 2, *a, 0, size)
    a = sized_sets(rng, [3 * SCAN_TILE + 5], span=40_000)  # dense: long runs across tile boundaries
    want = check_merge(placed, 2, *a, 0, "dense")
    assert int(want[4].max()) > 8


def test_carry_cases_of_the_segmented_scan(placed):
    rng = random.Random(9200)
    n = 3 * SCAN_TILE + 17
    inner = np.array(sorted(rng.randrange(10, 10 ** 6 - 10) for _ in range(n)), np.int32)
    # one region [0, 10^6) and small ones inside it over three scan tiles and more: one run
    qs, qe = np.concatenate([[0], inner]).astype(np.int32), np.concatenate([[10 ** 6], inner + 3]).astype(np.int32)
    want = check_merge(placed, 2, np.zeros(n + 1, np.int32), qs, qe, [0, n + 1], 0, "one run")
    assert want[3].tolist() == [0, 1] and want[4].tolist() == [n + 1] and (want[1][0], want[2][0]) == (0, 10 ** 6)
    # a segment boundary exactly on a tile boundary, and one element either side of it; the second set's first region lies inside
    # the first set's long run (and the same with a contig boundary)
    for first in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE):
        a_qs = np.concatenate([[0], inner[:first - 1]]).astype(np.int32)
        a_qe = np.concatenate([[10 ** 6], inner[:first - 1] + 3]).astype(np.int32)
        b_qs, b_qe = np.array([500, 700, 2 * 10 ** 6], np.int32), np.array([600, 800, 2 * 10 ** 6 + 5], np.int32)
        qs, qe = np.concatenate([a_qs, b_qs]), np.concatenate([a_qe, b_qe])
        want = check_merge(placed, 2, np.zeros(first + 3, np.int32), qs, qe, [0, first, first + 3], 0, ("sets", first))
        assert want[3].tolist() == [0, 1, 4] and want[2][:2].tolist() == [10 ** 6, 600]
        ichr = np.concatenate([np.zeros(first, np.int32), np.ones(3, np.int32)])
        want = check_merge(placed, 2, ichr, qs, qe, [0, first + 3], 0, ("contigs", first))
        assert want[3].tolist() == [0, 4] and want[2][:2].tolist() == [10 ** 6, 600]
    # all regions identical; strictly disjoint regions
    m = 2 * SCAN_TILE + 3
    want = check_merge(placed, 2, np.ones(m, np.int32), np.full(m, 77, np.int32), np.full(m, 99, np.int32), [0, m], 0, "identical")
    assert want[4].tolist() == [m]
    qs = (np.arange(m, dtype=np.int64) * 10)[rng.sample(range(m), m)].astype(np.int32)
    want = check_merge(placed, 2, np.zeros(m, np.int32), qs, qs + 9, [0, m], 0, "disjoint")
    assert len(want[0]) == m and (want[4] == 1).all()
    want = check_merge(placed, 2, np.zeros(m, np.int32), qs, qs + 9, [0, m], 1, "disjoint, gap 1")
    assert want[4].tolist() == [m]
    # ends at INT32_MAX under the largest gap
    qs = np.array([TOP - 1, 5, TOP - MAX_GAP - 2, 0], np.int32)
    qe = np.array([TOP, TOP - MAX_GAP - 3, TOP - MAX_GAP - 1, 1], np.int32)
    for gap in (0, 1, MAX_GAP):
        check_merge(placed, 2, np.ones(4, np.int32), qs, qe, [0, 4], gap, ("top", gap))


def test_shuffled_sets_give_the_sorted_sets_output(placed):
    rng = random.Random(9300)
    ichr, qs, qe, off = sized_sets(rng, [rng.randrange(200, 900) for _ in range(10)], span=300_000)
    order = np.concatenate([int(off[k]) + np.lexsort((qe[off[k]:off[k + 1]], qs[off[k]:off[k + 1]], ichr[off[k]:off[k + 1]])) for k in range(10)])
    want = check_merge(placed, 2, ichr[order], qs[order], qe[order], off, 0, "sorted")
    for seed in range(10):
        perm = np.concatenate([int(off[k]) + np.random.RandomState(seed * 10 + k).permutation(int(off[k + 1] - off[k])) for k in range(10)])
        assert merge_equal(cut_merge(dev_merge(placed, ichr[perm], qs[perm], qe[perm], off, 0))[1], want), seed


def test_resident_sets_on_a_torch_stream(placed):
    import torch
    rng = random.Random(9400)
    ichr, qs, qe, off = sized_sets(rng, [0, 700, 3, SCAN_TILE + 9], span=200_000)
    ichr[5], qe[9] = -1, qs[9]
    n, nsets = len(qs), len(off) - 1
    want = ref_merge(2, ichr, qs, qe, off, 5)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        t = [torch.from_numpy(a).to(dev) for a in (ichr, qs, qe, off)]
        o32 = [torch.full((n,), G32, dtype=torch.int32, device=dev) for _ in range(4)]
        o64 = [torch.full((k,), G64, dtype=torch.int64, device=dev) for k in (nsets + 1, nsets)]
        placed.merge_sets_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), nsets, n, o32[0].data_ptr(), o32[1].data_ptr(),
                              o32[2].data_ptr(), o64[0].data_ptr(), o64[1].data_ptr(), d_m_count=o32[3].data_ptr(), gap=5, stream=stream.cuda_stream)
        got = [x.cpu().numpy() for x in o32[:3] + [o64[0], o32[3], o64[1]]]
    stream.synchronize()
    rc, cut, rest = cut_merge([0] + got)
    assert merge_equal(cut, want) and (rest == 0).all()


@pytest.mark.parametrize("nfiles", [1, 63, 64, 65, 2041])
def test_dataset_bp_is_the_reference_and_is_computed_once(nfiles, workdir):
    rng = random.Random(9500 + nfiles)
    nbp, span = 4096, 20_000
    db = ListDb(workdir, "bp%d" % nfiles, sparse_lists(rng, nbp, nfiles, 6, span), nbp, 1)
    D = igd_amd.Database(db.path, device=0)
    try:
        assert D.dataset_bp_computed() == 0
        for k, v in enumerate((0, 500)):
            want = ref_dataset_bp(db, v if v else None)
            got = D.dataset_bp(v=v)
            assert np.array_equal(got, want) and D.dataset_bp_computed() == k + 1
            assert np.array_equal(D.dataset_bp(v=v), want) and D.dataset_bp_computed() == k + 1, "the second call computed it again"
            assert np.array_equal(igd_amd.dataset_bp_host(db.path, v=v), want)
        all_bp = D.dataset_bp(v=0)                          # (-v 500 may leave a database of one file nothing)
        assert all_bp[:nfiles].max() <= all_bp[nfiles] <= all_bp[:nfiles].sum() and all_bp[nfiles] > 0
        assert nfiles == 1 or not np.array_equal(all_bp, D.dataset_bp(v=500))
        D.jaccard_sets([0], [5], [900], [0, 1], v=500)
        assert D.dataset_bp_computed() == 2
    finally:
        D.close()


SEAM = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, os.path.join(%r, "tests"))
from helpers import short_tmpdir
import shutil
import igd_amd
from test_jaccard_host import shape_case
from jaccard_ref import ref_jaccard, ref_merge
d = short_tmpdir("igs")
try:
    db, ichr, qs, qe, off = shape_case(0, d, nreg=900)
    off = np.concatenate([[0, 0], off[1:], [off[-1]]]).astype(np.int64)          # empty sets at both ends
    D = igd_amd.Database(db.path, device=0)
    for v in (0, 500):
        want = ref_jaccard(db, ichr, qs, qe, off, v if v else -2 ** 31, 1 if v else 0)
        got = D.jaccard_sets(ichr, qs, qe, off, v=v)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), v
    assert len(D.jaccard_sets([], [], [], [0]).inter) == 0
    for gap in (0, 300):
        got, want = D.merge_sets(ichr, qs, qe, off, gap=gap), ref_merge(len(db.ctgs), ichr, qs, qe, off, gap)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), gap
    D.close()
    print("ok")
finally:
    shutil.rmtree(d, ignore_errors=True)
""" % ROOT


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "97"}, {"IGD_HIP_SETS_ROW_BYTES": "200"}, {"IGD_HIP_MERGE_GRID": "1"}])
def test_jaccard_sets_across_the_chunk_seams(env):
    """engine batches of 97 runs, and groups of three sets (a row budget of 200 bytes against 7 files x 8 bytes): merged sets are
    cut by batches and the sets come in several chunks; empty sets at both ends.  A merge grid of one workgroup: 900 regions are
    its first, second, third and fourth round of 256"""
    p = subprocess.run([sys.executable, "-c", SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env), timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


CARRY_WG = 128
CARRY = r"""
import os, random, shutil, sys
import numpy as np
sys.path.insert(0, os.path.join(%r, "tests"))
from helpers import short_tmpdir
import igd_amd
from jaccard_ref import ref_merge
from test_jaccard_host import two_contig_db
R, rng = %d, random.Random(9600)                  # R: the regions of one round of the carry workgroup
d = short_tmpdir("igc")
try:
    path = two_contig_db(d).path
    D = igd_amd.Database(path, device=0)
    # sorted positions [0, R): ONE run, [0, 10^8) and R - 1 small regions inside it -- it ends on the first round seam.
    # [R, 2R + 53): the next segment; its first region [500, 600) lies inside that run's span and must open a run; then
    # [1000, 10^8) with R + 50 small regions inside it: one run ACROSS the second seam; then a region behind it.
    # the rest: disjoint regions, into the third round.
    a_s = np.concatenate([[0], np.sort(rng.sample(range(10, 10 ** 8 - 10), R - 1))])
    a_e = np.concatenate([[10 ** 8], a_s[1:] + 3])
    b_in = np.sort(rng.sample(range(1001, 10 ** 8 - 10), R + 50))
    b_s = np.concatenate([[500, 1000], b_in, [10 ** 8 + 7]])
    b_e = np.concatenate([[600, 10 ** 8], b_in + 3, [10 ** 8 + 9]])
    c_s = 2 * 10 ** 8 + 10 * np.arange(1500)
    c_e = c_s + 9
    qs, qe = (np.concatenate(x).astype(np.int32) for x in ((a_s, b_s, c_s), (a_e, b_e, c_e)))
    n, nb = len(qs), -(-len(qs) // %d)
    assert 2 * %d < nb, "the carry workgroup does not reach a third round"
    sets = (np.zeros(n, np.int32), [0, R, R + len(b_s), n])
    contigs = (np.concatenate([np.zeros(R, np.int32), np.ones(n - R, np.int32)]), [0, n])
    for what, (ichr, off) in (("sets", sets), ("contigs", contigs)):
        off = np.array(off, np.int64)
        perm = np.concatenate([int(off[k]) + np.random.RandomState(k).permutation(int(off[k + 1] - off[k])) for k in range(len(off) - 1)])
        got = D.merge_sets(ichr[perm], qs[perm], qe[perm], off)
        want = ref_merge(2, ichr, qs, qe, off)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), what
        assert all(np.array_equal(g, w) for g, w in zip(got, igd_amd.merge_host(path, ichr, qs, qe, off))), what
        assert got[2][:4].tolist() == [10 ** 8, 600, 10 ** 8, 10 ** 8 + 9] and got[4][:4].tolist() == [R, 1, R + 51, 1], what
    D.close()
    print("ok")
finally:
    shutil.rmtree(d, ignore_errors=True)
""" % (ROOT, CARRY_WG * SCAN_TILE, SCAN_TILE, CARRY_WG)


def test_the_carry_workgroup_hands_the_pair_from_round_to_round():
    """igd_merge_scan_carry takes the tile aggregates in rounds of its workgroup size and keeps the (head, max) pair between
    rounds; in production a second round begins past 1 024 tiles = 2 097 152 regions.  A workgroup of 128 threads (two waves, so
    the waves' partials are met in every round) takes 128 tiles = 262 144 regions per round: about 526 000 regions are three
    rounds, with a run that ends on the first seam, a set (and a contig) boundary on it whose first region lies inside that
    run, and a run across the second seam.  Against the Python sweep and the host route."""
    p = subprocess.run([sys.executable, "-c", CARRY], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, IGD_HIP_MERGE_CARRY_WG=str(CARRY_WG)), timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def shipped_round():
    """regions of one round of igd_merge_scan_carry and of ss_scan_of_sums as shipped (both 1 024 tiles of SCAN_TILE)"""
    src = open(os.path.join(ROOT, "igd_amd", "csrc", "engine", "merge_dev.hpp")).read()
    wg = int(re.search(r"^#define\s+IGD_MERGE_CARRY_WG\s+(\d+)", src, re.M).group(1))
    from test_gpu_sortscan import SUMS_WG
    assert wg == SUMS_WG and wg // 64 == 16, (wg, SUMS_WG)      # (16 waves' partials in wagg[])
    return wg * SCAN_TILE


def seam_case(R, what):
    """the construction of CARRY above with R regions per round: sorted positions [0, R) ONE run that ends on the first seam;
    the next segment (a set or a contig) begins there with [500, 600) inside that run's span, then [1000, 10^8) with R + 50
    small regions inside it, one run ACROSS the second seam, a region behind it, and disjoint regions into the third round"""
    rng = np.random.default_rng(9800)
    a_in = 10 + np.cumsum(rng.integers(1, 40, R - 1))
    b_in = 1001 + np.cumsum(rng.integers(1, 40, R + 50))
    assert a_in[-1] < 10 ** 8 - 10 and b_in[-1] < 10 ** 8 - 10
    a_s, a_e = np.concatenate([[0], a_in]), np.concatenate([[10 ** 8], a_in + 3])
    b_s, b_e = np.concatenate([[500, 1000], b_in, [10 ** 8 + 7]]), np.concatenate([[600, 10 ** 8], b_in + 3, [10 ** 8 + 9]])
    c_s = 2 * 10 ** 8 + 10 * np.arange(1500)
    qs, qe = (np.concatenate(x).astype(np.int32) for x in ((a_s, b_s, c_s), (a_e, b_e, c_s + 9)))
    n = len(qs)
    if what == "sets":
        ichr, off = np.zeros(n, np.int32), np.array([0, R, R + len(b_s), n], np.int64)
    else:
        ichr, off = np.concatenate([np.zeros(R, np.int32), np.ones(n - R, np.int32)]), np.array([0, n], np.int64)
    perm = np.concatenate([int(off[k]) + np.random.RandomState(k).permutation(int(off[k + 1] - off[k])) for k in range(len(off) - 1)])
    return ichr[perm], qs[perm], qe[perm], off


def random_case(n):
    """three sets on two contigs, a few regions that do not take part; about every second region joins its neighbour"""
    rng = np.random.default_rng(9900)
    ichr = rng.integers(0, 2, n).astype(np.int32)
    qs = rng.integers(0, 2 * 10 ** 9, n)
    qe = qs + rng.choice([1, 30, 400, 5000], n)
    for k, i in enumerate(rng.integers(0, n, 40)):
        if k % 2:
            ichr[i] = (-1, 2)[k % 4 == 1]
        else:
            qe[i] = qs[i] - (k % 4)
    return ichr, qs.astype(np.int32), qe.astype(np.int32), np.array([0, n // 5, n // 5 + n // 2, n], np.int64)


@pytest.mark.parametrize("what", ["sets", "contigs", "random"])
def test_the_merge_past_a_round_under_the_shipped_constants(what, placed):
    """No test variable is set: igd_merge_scan_carry runs with its 1 024 threads and 16 waves' partials, and the run-flag scan
    inside the merge (exclusive_scan) with ss_scan_of_sums, both into a third round of 1 024 tiles.  Every integer against
    ref_merge_np (tests/test_jaccard_host.py pins it to the Python sweep)."""
    assert not any(v in os.environ for v in ("IGD_HIP_MERGE_CARRY_WG", "IGD_HIP_MERGE_GRID"))
    R = shipped_round()
    ichr, qs, qe, off = random_case(2 * R + SCAN_TILE + 5) if what == "random" else seam_case(R, what)
    n = len(qs)
    assert -(-n // SCAN_TILE) > 2 * (R // SCAN_TILE), "%d regions do not reach a third round of %d tiles" % (n, R // SCAN_TILE)
    want = ref_merge_np(2, ichr, qs, qe, off)
    rc, got, rest = cut_merge(dev_merge(placed, ichr, qs, qe, off))
    assert rc == 0 and merge_equal(got, want) and (rest == 0).all(), [np.flatnonzero(g != w)[:3] if g.shape == w.shape else (g.shape, w.shape)
                                                                       for g, w in zip(got, want)]
    if what == "random":
        assert want[5].sum() >= 20 and (want[5] > 0).all() and 0.2 * n < len(want[0]) < 0.8 * n and want[4].max() > 3
    else:
        assert got[2][:4].tolist() == [10 ** 8, 600, 10 ** 8, 10 ** 8 + 9] and got[4][:4].tolist() == [R, 1, R + 51, 1]


def test_cli_j_on_both_routes_byte_for_byte(workdir):
    d = os.path.join(workdir, "cli")
    os.makedirs(d)
    db, beds = db_and_beds(d, 1 << 12, 1, 9, 2, 12, 9700)
    lst = _write_list(d, beds + [os.path.join(d, "missing.bed")])
    for sel in (["-q", beds[0]], ["-Q", lst]):
        for extra in ([], ["-v", "500"]):
            args = ["search", db.path] + sel + ["-J"] + extra
            want = _run(args, HOST)
            got = _run(args)                                      # (IGD_HOST_MAX_QUERIES = 0: the engine)
            assert want.returncode == 0 and got.returncode == 0, got.stderr
            assert got.stdout == want.stdout and b"intersection" in got.stdout and b"Any dataset: " in got.stdout, args
