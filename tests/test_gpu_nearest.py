"""GPU: the nearest record per dataset within a window (igd_hip_nearest / igd_hip_nearest_sets / igd_hip_nearest_dev, kernels
igd_nearest_rows, igd_nearest_rowmin and igd_nearest_reduce; Database.nearest / nearest_sets / nearest_files, `-N`).

The device must equal, on every integer, the definition restated in tests/nearest_ref.py (a numpy broadcast over the interval
lists this test wrote) and the host route (igdc_nearest_host).  Every output is handed over full of garbage: a call defines
every word."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import igd_amd
from helpers import ROOT, short_tmpdir, write_bed
from nearest_ref import (MAX_WINDOW, ListDb, clustered_lists, mixed_regions, placed_db, placed_regions, ref_rows, ref_sets, sparse_lists,
                         windows)
from test_sets_cli import _write_list
from test_support_host import FLAT, HOST, NUMPY_DBS, _run

pytestmark = pytest.mark.gpu
GARBAGE = 0x5a5a5a5a


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("ign")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def lds_files():
    src = open(os.path.join(ROOT, "igd_amd", "csrc", "engine", "nearest_dev.hpp")).read()
    return int(re.search(r"^#define\s+IGD_NEAREST_LDS_FILES\s+(\d+)", src, re.M).group(1))


def check(db, ldb, ichr, qs, qe, W, v=None, off=None, host=True):
    """rows, dmin and the set statistics of one call against the definition (and the host route)"""
    want, wmin = ref_rows(ldb, ichr, qs, qe, W, v)
    dist, dmin = db.nearest(ichr, qs, qe, W, value_filter=v, dist=np.full((len(qs), db.nfiles), GARBAGE, np.int32))
    bad = np.flatnonzero((dist != want).any(axis=1) | (dmin != wmin))
    assert dist.dtype == np.int32 and len(bad) == 0, (W, v, bad[:5].tolist(), [(dist[i].tolist()[:8], want[i].tolist()[:8]) for i in bad[:3]])
    if host:
        hdist, hmin = igd_amd.nearest_host(ldb.path, ichr, qs, qe, W, value_filter=v)
        assert np.array_equal(hdist, dist) and np.array_equal(hmin, dmin), (W, v)
    if off is None:
        off = np.array([0, len(qs)], np.int64)
    ns = db.nearest_sets(ichr, qs, qe, off, W, value_filter=v)
    for got, ref in zip(ns[:3], ref_sets(want, wmin, off)):
        assert got.dtype == np.int64 and np.array_equal(got, ref), (W, v)
    return want, wmin


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_device_equals_the_definition_on_the_four_database_shapes(case, workdir):
    from igd_amd import Database
    rng = random.Random(7100 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    ldb = ListDb(workdir, "c%d" % case, files, nbp, gtype)
    ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 500)
    off = np.array([0, 0, 1, 6, 6, 206, len(qs)], np.int64)
    db = Database(ldb.path)
    try:
        far = False
        for W in windows(nbp):
            for v in (None, 500):
                want, _ = check(db, ldb, ichr, qs, qe, W, v, off)
                far |= bool((want > 0).any())
        assert far
    finally:
        db.close()


def test_placed_cases(workdir):
    from igd_amd import Database
    nbp = 1 << 14
    ldb = placed_db(workdir, nbp, "gplaced")
    (ichr, qs, qe), _ = placed_regions(nbp)
    db = Database(ldb.path)
    try:
        for W in windows(nbp) + [2 * nbp, 500]:
            for v in (None, 500):
                check(db, ldb, ichr, qs, qe, W, v)
    finally:
        db.close()


@pytest.mark.parametrize("nfiles", [1, 31, 32, 33, 65, 2081, 4096, 4097])
def test_file_counts_and_small_calls(nfiles, workdir):
    """1, 31, 32, 33, 65 and 2 081 files, and the two sides of the LDS form's limit; calls of 1, 4 and 5 regions (one wave, one
    workgroup, a second workgroup)"""
    from igd_amd import Database
    assert lds_files() == 4096
    rng = random.Random(7200 + nfiles)
    nbp = 1 << 12
    span = 40 * nbp
    ldb = ListDb(workdir, "f%d" % nfiles, sparse_lists(rng, nbp, nfiles, 2 if nfiles > 100 else 9, span), nbp, 1)
    db = Database(ldb.path)
    try:
        assert db.nfiles == nfiles
        ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 64)
        hit = False
        for n in (1, 4, 5, 64):
            for W in (0, 700, 3 * nbp + 5, MAX_WINDOW):
                for v in (None, 500):
                    want, _ = check(db, ldb, ichr[:n], qs[:n], qe[:n], W, v, host=(n == 64))
                    hit |= bool((want >= 0).any())
        assert hit
    finally:
        db.close()


def test_a_wave_resets_its_table_before_its_next_region(workdir):
    """4 x igd_hip_nearest_grid + 3 regions: the grid is full and its first three waves meet a second region.  Their first
    regions cover the whole contig (every file at distance 0); their second ones are a region on an unknown contig (the row
    of -1 that is stored without reading the table), a zero-length region and a short one: a table that was not reset would
    leak zeros into them."""
    from igd_amd import Database
    from igd_amd import _native as N
    rng = random.Random(7300)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 40, 2, 20)
    ldb = ListDb(workdir, "w", files, nbp, 1)
    nq = 4 * 2048 + 3
    assert N.hip().igd_hip_nearest_grid(nq) == 2048 and nq == 4 * N.hip().igd_hip_nearest_grid(nq) + 3
    assert N.hip().igd_hip_nearest_grid(5) == 2 and N.hip().igd_hip_nearest_grid(1) == 1
    ichr, qs, qe = mixed_regions(rng, 2, nbp, span, nq)
    ichr[:3], qs[:3], qe[:3] = 0, 0, span + 6 * nbp
    ichr[8192:], qs[8192:], qe[8192:] = [-1, 0, 1], [5, 3 * nbp, 7 * nbp], [9, 3 * nbp, 7 * nbp + 20]
    off = np.array([0, 700, 1800, 1800, nq], np.int64)
    db = Database(ldb.path)
    try:
        for W, v in ((nbp, None), (300, 500)):
            want, _ = check(db, ldb, ichr, qs, qe, W, v, off)
            assert (want[:3] == 0).all() and (want[8192] == -1).all() and (want[8193:] != 0).any()
    finally:
        db.close()


def test_n_within_is_the_support_of_the_padded_regions(workdir):
    """the only device route there was: support_sets over the regions padded by W (where padding does not clamp at 0), rule
    FLAT -- it yields n_within; and n_overlap is the support of the regions as given"""
    from igd_amd import Database
    rng = random.Random(7400)
    nbp = 1 << 11
    files, span = clustered_lists(rng, nbp, 40, 1, 25)
    ldb = ListDb(workdir, "p", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 900)
    off = np.array([0, 5, 5, 400, 900], np.int64)
    db = Database(ldb.path)
    try:
        for W in (0, 1, nbp - 1, 3 * nbp + 5):
            keep = qs.astype(np.int64) - W >= 0
            c, s, e = ichr[keep], qs[keep], qe[keep]
            o = np.concatenate([[0], np.cumsum(keep)])[off].astype(np.int64)
            for v in (None, 500):
                ns = db.nearest_sets(c, s, e, o, W, value_filter=v)
                vf = igd_amd._native.IGD_HIP_NO_VALUE_FILTER if v is None else v
                sup, nhit = db.support_sets(c, s - W, e + W, o, rule=FLAT, value_filter=vf)
                assert sup.any() and np.array_equal(ns.n_within[:, :-1], sup) and np.array_equal(ns.n_within[:, -1], nhit), (W, v)
                sup0, nhit0 = db.support_sets(c, s, e, o, rule=FLAT, value_filter=vf)
                assert np.array_equal(ns.n_overlap[:, :-1], sup0) and np.array_equal(ns.n_overlap[:, -1], nhit0), (W, v)
                if W == 0:
                    assert np.array_equal(ns.n_within, ns.n_overlap) and not ns.sum_dist.any()
    finally:
        db.close()


SEAM = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import short_tmpdir
import nearest_ref as R
from igd_amd import Database
d = short_tmpdir("igb")
rng = random.Random(12)
nbp = 1 << 12
files, span = R.clustered_lists(rng, nbp, 40, 2, 20)
ldb = R.ListDb(d, "b", files, nbp, 1)
db = Database(ldb.path)
sizes = [0, 1, 5, 700, 0, 1100, 3]
off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
ichr, qs, qe = R.mixed_regions(rng, 2, nbp, span, int(off[-1]))
for W, v in ((nbp, None), (3 * nbp + 5, 500), (0, None)):
    want, wmin = R.ref_rows(ldb, ichr, qs, qe, W, v)
    for n in (0, 1, 96, 97, 98, 195, len(qs)):
        dist, dmin = db.nearest(ichr[:n], qs[:n], qe[:n], W, value_filter=v, dist=np.full((n, 40), 0x5a5a5a5a, np.int32))
        assert np.array_equal(dist, want[:n]) and np.array_equal(dmin, wmin[:n]), (W, v, n)
    ns = db.nearest_sets(ichr, qs, qe, off, W, value_filter=v)
    for got, ref in zip(ns[:3], R.ref_sets(want, wmin, off)):
        assert np.array_equal(got, ref), (W, v)
    assert ns.n_within[3].any() and ns.n_within[5].any() and not ns.n_within[0].any()
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


@pytest.mark.parametrize("env", [{"IGD_HIP_MAX_BATCH": "97"}, {"IGD_HIP_NEAREST_ROW_BYTES": str(97 * 160 + 5)},
                                 {"IGD_HIP_NEAREST_ROW_BYTES": str(333 * 160), "IGD_HIP_SETS_ROW_BYTES": "2000"}])
def test_calls_straddle_the_chunk_seams(env):
    """chunks of 97 regions (by the batch limit, and by a row budget of 97 rows of 160 bytes and a little) and of 333: no seam
    is a multiple of 64, the sets of 700 and 1 100 regions are cut by region chunks; groups of two sets (a budget of 2 000
    bytes against three rows of 41 x 8).  The variables are read once per process: a child process each."""
    p = subprocess.run([sys.executable, "-c", SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env),
                       timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def test_resident_rows_on_a_torch_stream(workdir):
    import torch
    from igd_amd import Database
    rng = random.Random(7500)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 33, 1, 12)
    ldb = ListDb(workdir, "t", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 300)
    db = Database(ldb.path)
    try:
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            t = [torch.from_numpy(a).to(dev) for a in (ichr, qs, qe)]
            d_dist = torch.full((300, 33), GARBAGE, dtype=torch.int32, device=dev)
            d_min = torch.full((300,), GARBAGE, dtype=torch.int32, device=dev)
            stream.synchronize()
            db.nearest_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 300, 2 * nbp, d_dist.data_ptr(), d_min.data_ptr(),
                           value_filter=500, stream=stream.cuda_stream)
            db.sync(stream.cuda_stream)
            want, wmin = ref_rows(ldb, ichr, qs, qe, 2 * nbp, 500)
            assert np.array_equal(d_dist.cpu().numpy(), want) and np.array_equal(d_min.cpu().numpy(), wmin)
    finally:
        db.close()


def test_bad_arguments_change_nothing_and_empty_calls_are_fine(workdir):
    from igd_amd import Database
    from igd_amd.database import IgdError
    rng = random.Random(7600)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 3, 1, 6)
    ldb = ListDb(workdir, "e", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 20)
    db = Database(ldb.path)
    try:
        for W in (-1, MAX_WINDOW + 1):
            dist = np.full((20, 3), GARBAGE, np.int32)
            with pytest.raises(IgdError):
                db.nearest(ichr, qs, qe, W, dist=dist)
            assert (dist == GARBAGE).all()
            with pytest.raises(IgdError):
                db.nearest_sets(ichr, qs, qe, [0, 20], W)
        for off in ([1, 20], [0, 15, 10, 20]):
            with pytest.raises(IgdError):
                db.nearest_sets(ichr, qs, qe, off, 100)
        dist, dmin = db.nearest(ichr[:0], qs[:0], qe[:0], 100)
        assert dist.shape == (0, 3) and dmin.shape == (0,)
        ns = db.nearest_sets(ichr[:0], qs[:0], qe[:0], [0, 0, 0], 100)
        assert all(a.shape == (2, 4) and not a.any() for a in ns[:3])
        ns = db.nearest_sets(ichr, qs, qe, [0, 0, 20, 20], MAX_WINDOW)
        assert not ns.n_within[0].any() and not ns.n_within[2].any() and ns.n_within[1].any()
    finally:
        db.close()


@pytest.mark.parametrize("extra", [[], ["-v", "500"]])
def test_cli_engine_route_prints_what_the_host_route_prints(extra, workdir):
    rng = random.Random(7700)
    nbp = 1 << 12
    d = os.path.join(workdir, "cli%d" % len(extra))
    os.makedirs(d)
    files, span = clustered_lists(rng, nbp, 9, 2, 15)
    ldb = ListDb(d, "db", files, nbp, 1)
    beds = []
    for k in range(3):
        ichr, qs, qe = mixed_regions(rng, 2, nbp, span, 300)
        p = os.path.join(d, "q%d.bed" % k)
        write_bed(p, [(ldb.ctgs[c] if 0 <= c < 2 else "chrNotThere", s, e) for c, s, e in zip(ichr.tolist(), qs.tolist(), qe.tolist()) if s >= 0])
        beds.append(p)
    lst = _write_list(d, beds + [os.path.join(d, "missing.bed")])
    for sel in (["-q", beds[0]], ["-Q", lst]):
        for W in ("0", str(nbp), str(MAX_WINDOW)):
            args = ["search", ldb.path] + sel + ["-N", W] + extra
            want = _run(args, HOST)
            got = _run(args)                                      # (IGD_HOST_MAX_QUERIES = 0: the engine)
            assert want.returncode == 0 and got.returncode == 0, got.stderr
            assert got.stdout == want.stdout and b"n_within" in got.stdout, args
