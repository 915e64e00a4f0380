"""GPU: flanking records per dataset and the relative-distance histogram (igd_hip_flank / igd_hip_flank_dev /
igd_hip_flank_reldist, kernels igd_flank_rows and igd_flank_reldist; Database.flanks / flanks_dev / flank_reldist /
flank_reldist_files, `-N W -L B [-E]`).

The device must equal, on every integer, the definition restated in tests/flank_ref.py (a numpy broadcast over the interval lists
this test wrote) and the host route (igdc_flank_host / igdc_flank_reldist_host).  Every output is handed over full of 0x5a: a
call defines every word."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import igd_amd
from flank_ref import EDGES, MIDPOINTS, flanked, ref_flanks, ref_hist
from helpers import ROOT, short_tmpdir, write_bed
from nearest_ref import MAX_WINDOW, ListDb, clustered_lists, mixed_regions, sparse_lists, windows
from test_flank_host import flank_identities, placed_flank_db, placed_flank_regions, wide_db
from test_nearest_signed_host import top_db, top_regions
from test_sets_cli import _write_list
from test_support_host import HOST, NUMPY_DBS, _run

pytestmark = pytest.mark.gpu
GARBAGE = 0x5a5a5a5a
GARBAGE64 = 0x5a5a5a5a5a5a5a5a
MEASURES = (EDGES, MIDPOINTS)


def lds_files():
    src = open(os.path.join(ROOT, "igd_amd", "csrc", "engine", "flank_dev.hpp")).read()
    return int(re.search(r"^#define\s+IGD_FLANK_LDS_FILES\s+(\d+)", src, re.M).group(1))


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igf")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def check(db, ldb, ichr, qs, qe, W, ms, v=None, off=None, nbins=(50,), host=True):
    """the rows, the minima and the histograms of one call against the definition and the host route"""
    want = ref_flanks(ldb, ichr, qs, qe, W, ms, v)
    got = db.flanks(ichr, qs, qe, W, measure=ms, value_filter=v, up=np.full((len(qs), db.nfiles), GARBAGE, np.int32),
                    down=np.full((len(qs), db.nfiles), GARBAGE, np.int32))
    for name, g, w in zip(("up", "down", "upmin", "downmin"), got, want):
        bad = np.flatnonzero((g != w).reshape(len(qs), -1).any(axis=1))
        assert g.dtype == np.int32 and len(bad) == 0, (name, W, ms, v, bad[:5].tolist(), g[bad[:2]].tolist(), w[bad[:2]].tolist())
    if host:
        hg = igd_amd.flanks_host(ldb.path, ichr, qs, qe, W, measure=ms, value_filter=v)
        assert all(np.array_equal(a, b) for a, b in zip(hg, got)), (W, ms, v)
    if off is None:
        off = np.array([0, len(qs)], np.int64)
    for B in nbins:
        fr = db.flank_reldist(ichr, qs, qe, off, W, B, measure=ms, value_filter=v, hist=np.full((len(off) - 1, B, db.nfiles + 1), GARBAGE64, np.int64))
        assert fr.hist.dtype == np.int64 and np.array_equal(fr.hist, ref_hist(*want, off, B)), (W, ms, v, B)
        if host:
            assert np.array_equal(igd_amd.flank_reldist_host(ldb.path, ichr, qs, qe, off, W, B, measure=ms, value_filter=v).hist, fr.hist), (W, ms, v, B)
    return want


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_device_equals_the_definition_on_the_four_database_shapes(case, workdir):
    from igd_amd import Database
    rng = random.Random(12700 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    ldb = ListDb(workdir, "c%d" % case, files, nbp, gtype)
    ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 500)
    off = np.array([0, 0, 1, 6, 6, 206, len(qs)], np.int64)
    db = Database(ldb.path)
    try:
        seen = 0
        for W in windows(nbp):
            for v in (None, 500):
                for ms in MEASURES:
                    want = check(db, ldb, ichr, qs, qe, W, ms, v, off, (1, 2, 50, 64))
                    seen += int(flanked(want[0], want[1]).sum())
                    if ms == EDGES:
                        flank_identities(want[0], want[1], db.nearest_signed(ichr, qs, qe, W, value_filter=v)[0])
        assert seen > 1000
    finally:
        db.close()


def test_placed_cases(workdir):
    from igd_amd import Database
    nbp = 1 << 14
    ldb = placed_flank_db(workdir, nbp, "gplaced")
    ichr, qs, qe = placed_flank_regions()
    db = Database(ldb.path)
    try:
        for W in windows(nbp) + [500, 1000]:
            for v in (None, 500):
                for ms in MEASURES:
                    check(db, ldb, ichr, qs, qe, W, ms, v, np.array([0, 5, 5, len(qs)], np.int64), (1, 2, 50, 64))
        eu, ed, eum, edm = db.flanks(ichr, qs, qe, 1000, measure="edges")
        mu, md, _, mdm = db.flanks(ichr, qs, qe, 1000, measure="midpoints")
        assert eu[0, 0] == 1 and ed[0, 0] == 1 and mu[0, 0] == 550 and md[0, 0] == 750
        assert eu[1, 1] == -1 and ed[1, 1] == -1 and mu[1, 1] == -1 and md[1, 1] == 125 and md[2, 2] == 0 and mdm[2] == 0
        assert ed[3, 3] == 91 and db.flanks(ichr, qs, qe, 500)[1][3, 3] == -1
        assert eu[4, 4] == 11 and db.flanks(ichr, qs, qe, 1000, measure="edges", value_filter=500)[0][4, 4] == 901
        assert eu[5, 5] == 1 and ed[5, 5] == 3 and (eu[8:] == -1).all() and (edm[8:] == -1).all() and eum[0] == 1
        h = db.flank_reldist(ichr, qs, qe, [0, len(qs)], 1000, 50, measure="edges").hist
        assert h[0, 49, 0] == 1 and h[0, 25, 5] == 1
    finally:
        db.close()
    # a distance of 2^30 at W = 2^30 and nothing at 2^30 - 1; up + down = 2^31 in the last bin
    tdb = top_db(workdir, nbp, "gtop")
    db = Database(tdb.path)
    try:
        want = check(db, tdb, *top_regions(), MAX_WINDOW, EDGES)
        assert want[1][0, 0] == 2 ** 30 and want[0][1, 1] == 2 ** 30
        want = check(db, tdb, *top_regions(), MAX_WINDOW - 1, EDGES)
        assert want[1][0, 0] == -1 and want[0][1, 1] == -1
    finally:
        db.close()
    wdb = wide_db(workdir, nbp, "gwide")
    db = Database(wdb.path)
    try:
        r = (np.array([0], np.int32), np.array([2 ** 30], np.int32), np.array([2 ** 30 - 1], np.int32))
        want = check(db, wdb, *r, MAX_WINDOW, EDGES, nbins=(1, 2, 63, 64))
        assert want[0][0, 0] == 2 ** 30 and want[1][0, 0] == 2 ** 30
        assert db.flank_reldist(*r, [0, 1], MAX_WINDOW, 64, measure="edges").hist[0, 63].tolist() == [1, 1]
        check(db, wdb, *r, MAX_WINDOW, MIDPOINTS, nbins=(64,))
    finally:
        db.close()


@pytest.mark.parametrize("nfiles", [1, 63, 64, 65, 2048, 2049, 4097])
def test_file_counts_small_calls_and_bin_counts(nfiles, workdir):
    """1, 63, 64 and 65 files (the any-dataset column moves into a second column block at 64), the two sides of the LDS form's
    limit and 4 097 files; calls of 1, 4, 5 and 64 regions (one wave, one workgroup, a second workgroup); 1, 2, 63 and 64 bins;
    the wide form with and without the minima"""
    from igd_amd import Database
    assert lds_files() == 2048
    rng = random.Random(12800 + nfiles)
    nbp = 1 << 12
    span = 40 * nbp
    ldb = ListDb(workdir, "f%d" % nfiles, sparse_lists(rng, nbp, nfiles, 3 if nfiles > 100 else 9, span), nbp, 1)
    db = Database(ldb.path)
    try:
        assert db.nfiles == nfiles
        ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 64)
        seen = 0
        # (thousands of files: the reference's broadcast is what takes time, so fewer combinations)
        for n in (1, 4, 5, 64) if nfiles < 100 else (5, 64):
            off = np.array([0, n // 2, n], np.int64)
            for W in (0, 700, 3 * nbp + 5, MAX_WINDOW) if nfiles < 100 else (3 * nbp + 5, MAX_WINDOW):
                for ms, v in ((EDGES, None), (MIDPOINTS, 500)) if nfiles > 100 else ((EDGES, None), (EDGES, 500), (MIDPOINTS, None), (MIDPOINTS, 500)):
                    want = check(db, ldb, ichr[:n], qs[:n], qe[:n], W, ms, v, off, (1, 2, 63, 64), host=(n == 64))
                    seen += int(flanked(want[0], want[1]).sum())
        assert seen > 0
        # resident rows with no minimum, with one and with both (the wide form launches igd_nearest_rowmin per wanted minimum)
        import torch
        dev = torch.device("cuda", 0)
        t = [torch.from_numpy(a).to(dev) for a in (ichr, qs, qe)]
        want = ref_flanks(ldb, ichr, qs, qe, 3 * nbp + 5, MIDPOINTS)
        for k in range(3):
            d_u, d_d = (torch.full((64, nfiles), GARBAGE, dtype=torch.int32, device=dev) for _ in range(2))
            d_um, d_dm = (torch.full((64,), GARBAGE, dtype=torch.int32, device=dev) for _ in range(2))
            torch.cuda.synchronize()
            db.flanks_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 64, 3 * nbp + 5, d_u.data_ptr(), d_d.data_ptr(),
                          d_um.data_ptr() if k == 2 else None, d_dm.data_ptr() if k >= 1 else None)
            db.sync()
            assert np.array_equal(d_u.cpu().numpy(), want[0]) and np.array_equal(d_d.cpu().numpy(), want[1]), k
            assert np.array_equal(d_um.cpu().numpy(), want[2] if k == 2 else np.full(64, GARBAGE, np.int32)), k
            assert np.array_equal(d_dm.cpu().numpy(), want[3] if k >= 1 else np.full(64, GARBAGE, np.int32)), k
    finally:
        db.close()


def test_a_wave_resets_both_tables(workdir):
    """4 x igd_hip_nearest_grid + 3 regions: the grid is full and its first three waves meet a second region, and 2 x 8 192 + 3:
    they meet a third one.  Wave 0: a region with records of every file on both sides (two full tables), an unknown contig (rows
    of -1 stored without reading the tables), the first region again.  Wave 1: a region at the contig's start, whose records are
    all downstream, then one past its end, whose records are all upstream, then the first again: an up table that was not reset
    would leak into the second, a down table into the third.  Wave 2: full, zero-length, full."""
    from igd_amd import Database
    from igd_amd import _native as N
    rng = random.Random(12900)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 12, 1, 20)
    ldb = ListDb(workdir, "w", files, nbp, 1)
    nq = 2 * 8192 + 3
    assert N.hip().igd_hip_nearest_grid(8195) == 2048 and N.hip().igd_hip_nearest_grid(nq) == 2048
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, nq)
    end = span + 6 * nbp
    mid = (span // 2, span // 2 + 1)
    for base, regs in ((0, [mid, (5, 9), mid]), (8192, [(0, 0), (end, end + 5), (3 * nbp, 3 * nbp)]), (16384, [mid, mid, mid])):
        for i, (a, b) in enumerate(regs):
            ichr[base + i], qs[base + i], qe[base + i] = 0, a, b
    ichr[8192] = -1
    db = Database(ldb.path)
    try:
        for n, off in ((8195, [0, 700, 1800, 1800, 8195]), (nq, [0, 0, 1, 256, 512, 769, 1869, nq])):
            for ms in MEASURES:
                up, down, _, _ = check(db, ldb, ichr[:n], qs[:n], qe[:n], MAX_WINDOW, ms, None, np.array(off, np.int64), (50,), host=(ms == EDGES))
                assert (up[0] >= 0).all() and (down[0] >= 0).all() and (up[8192] == -1).all() and (down[8192] == -1).all()
                assert (up[1] == -1).all() and (down[1] >= 0).all() and (up[8193] >= 0).all() and (down[8193] == -1).all()
                assert n < nq or ((up[16384:] >= 0).all() and (down[16384:] >= 0).all())
    finally:
        db.close()


def test_sets_around_the_slice_length(workdir):
    """sets of 0, 1, 255, 256, 257 and 1 100 regions: slices that end inside, at and past a slice of 256"""
    from igd_amd import Database
    rng = random.Random(13000)
    nbp = 1 << 11
    files, span = clustered_lists(rng, nbp, 40, 1, 25)
    ldb = ListDb(workdir, "s", files, nbp, 1)
    sizes = [0, 1, 255, 256, 257, 0, 1100]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, int(off[-1]))
    db = Database(ldb.path)
    try:
        for W, ms, v in ((0, MIDPOINTS, None), (nbp, EDGES, None), (3 * nbp + 5, MIDPOINTS, 500)):
            check(db, ldb, ichr, qs, qe, W, ms, v, off, (1, 2, 63, 64))
        h = db.flank_reldist(ichr, qs, qe, off, 3 * nbp + 5, 50).hist
        assert h[6].any() and h[4].any() and not h[0].any() and not h[5].any()
    finally:
        db.close()


SEAM = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import short_tmpdir
import nearest_ref as R
import flank_ref as F
from igd_amd import Database
d = short_tmpdir("igt")
rng = random.Random(17)
nbp = 1 << 12
files, span = R.clustered_lists(rng, nbp, 40, 2, 20)
ldb = R.ListDb(d, "b", files, nbp, 1)
db = Database(ldb.path)
sizes = [0, 1, 255, 256, 257, 0, 1100, 3]
off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
ichr, qs, qe = R.mixed_regions(rng, 2, nbp, span, int(off[-1]))
for W, ms, v in ((nbp, F.EDGES, None), (3 * nbp + 5, F.MIDPOINTS, 500), (0, F.MIDPOINTS, None)):
    want = F.ref_flanks(ldb, ichr, qs, qe, W, ms, v)
    for n in (0, 1, 96, 97, 98, 195, len(qs)):
        got = db.flanks(ichr[:n], qs[:n], qe[:n], W, measure=ms, value_filter=v, up=np.full((n, 40), 0x5a5a5a5a, np.int32),
                        down=np.full((n, 40), 0x5a5a5a5a, np.int32))
        assert all(np.array_equal(g, w[:n]) for g, w in zip(got, want)), (W, ms, v, n)
    for B in (2, 50, 64):
        fr = db.flank_reldist(ichr, qs, qe, off, W, B, measure=ms, value_filter=v, hist=np.full((len(sizes), B, 41), 0x5a5a5a5a5a5a5a5a, np.int64))
        assert np.array_equal(fr.hist, F.ref_hist(*want, off, B)), (W, ms, v, B)
    assert W == 0 or (fr.hist[4].any() and fr.hist[6].any() and not fr.hist[0].any())
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


@pytest.mark.parametrize("env", [{"IGD_HIP_NEAREST_ROW_BYTES": str(97 * 8 * 40 + 5)},
                                 {"IGD_HIP_NEAREST_ROW_BYTES": str(333 * 8 * 40), "IGD_HIP_SETS_ROW_BYTES": "2000"}])
def test_calls_straddle_the_chunk_seams(env):
    """chunks of 97 regions (a row budget of 97 x 2 rows of 160 bytes and a little) and of 333: no seam is a multiple of 64, the
    sets of 255 to 1 100 regions are cut by region chunks and start mid-chunk; groups of two sets (a budget of 2 000 bytes against
    the 2 x 41 x 8 = 656 of a set's two-bin histogram) and of one set (50 and 64 bins).  The variables are read once per
    process: a child process each."""
    p = subprocess.run([sys.executable, "-c", SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env),
                       timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def test_resident_rows_on_a_torch_stream(workdir):
    import torch
    from igd_amd import Database
    rng = random.Random(13100)
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
            d_u, d_d = (torch.full((300, 33), GARBAGE, dtype=torch.int32, device=dev) for _ in range(2))
            d_um, d_dm = (torch.full((300,), GARBAGE, dtype=torch.int32, device=dev) for _ in range(2))
            stream.synchronize()
            db.flanks_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 300, 2 * nbp, d_u.data_ptr(), d_d.data_ptr(), d_um.data_ptr(),
                          d_dm.data_ptr(), measure="edges", value_filter=500, stream=stream.cuda_stream)
            db.sync(stream.cuda_stream)
            want = ref_flanks(ldb, ichr, qs, qe, 2 * nbp, EDGES, 500)
            assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((d_u, d_d, d_um, d_dm), want))
    finally:
        db.close()


def test_bad_arguments_change_nothing_and_empty_calls_are_fine(workdir):
    from igd_amd import Database
    from igd_amd import _native as N
    from igd_amd.database import IgdError
    rng = random.Random(13200)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 3, 1, 6)
    ldb = ListDb(workdir, "e", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 20)
    db = Database(ldb.path)
    try:
        for W in (-1, MAX_WINDOW + 1):
            u, d = np.full((20, 3), GARBAGE, np.int32), np.full((20, 3), GARBAGE, np.int32)
            h = np.full((1, 50, 4), GARBAGE64, np.int64)
            with pytest.raises(IgdError):
                db.flanks(ichr, qs, qe, W, up=u, down=d)
            with pytest.raises(IgdError):
                db.flank_reldist(ichr, qs, qe, [0, 20], W, hist=h)
            assert (u == GARBAGE).all() and (d == GARBAGE).all() and (h == GARBAGE64).all()
        for off in ([1, 20], [0, 15, 10, 20]):
            with pytest.raises(IgdError):
                db.flank_reldist(ichr, qs, qe, off, 100)
        # the native calls refuse a bad measure, bad bins and a missing array before they write anything
        c, s_, e_ = (np.ascontiguousarray(a, np.int32) for a in (ichr, qs, qe))
        off = np.array([0, 20], np.int64)
        NOV = N.IGD_HIP_NO_VALUE_FILTER
        for ms, B in ((2, 50), (-1, 50), (EDGES, 0), (EDGES, 65), (MIDPOINTS, -1)):
            h = np.full((1, 65, 4), GARBAGE64, np.int64)
            rc = N.hip().igd_hip_flank_reldist(db.dev, c.ctypes.data, s_.ctypes.data, e_.ctypes.data, off.ctypes.data, 1, 100, ms, NOV, B, h.ctypes.data)
            assert rc != 0 and (h == GARBAGE64).all(), (ms, B)
        for ms, has_up in ((2, True), (EDGES, False)):
            u, d, m = np.full((20, 3), GARBAGE, np.int32), np.full((20, 3), GARBAGE, np.int32), np.full(20, GARBAGE, np.int32)
            rc = N.hip().igd_hip_flank(db.dev, c.ctypes.data, s_.ctypes.data, e_.ctypes.data, 20, 100, ms, NOV, u.ctypes.data if has_up else None,
                                       d.ctypes.data, m.ctypes.data, None)
            assert rc != 0 and (u == GARBAGE).all() and (d == GARBAGE).all() and (m == GARBAGE).all(), ms
        got = db.flanks(ichr[:0], qs[:0], qe[:0], 100)
        assert got[0].shape == (0, 3) and got[3].shape == (0,)
        fr = db.flank_reldist(ichr[:0], qs[:0], qe[:0], [0, 0, 0], 100, 5, hist=np.full((2, 5, 4), GARBAGE64, np.int64))
        assert fr.hist.shape == (2, 5, 4) and not fr.hist.any()
        assert db.flank_reldist(ichr[:0], qs[:0], qe[:0], [0], 100, 5).hist.shape == (0, 5, 4)
        fr = db.flank_reldist(ichr, qs, qe, [0, 0, 20, 20], MAX_WINDOW, 3)
        assert not fr.hist[0].any() and not fr.hist[2].any() and fr.hist[1].any()
    finally:
        db.close()


@pytest.mark.parametrize("extra", [[], ["-v", "500", "-E"]])
def test_cli_engine_route_prints_what_the_host_route_prints(extra, workdir):
    rng = random.Random(13300)
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
        for W, B in (("0", "1"), (str(nbp), "50"), (str(MAX_WINDOW), "64")):
            args = ["search", ldb.path] + sel + ["-N", W, "-L", B] + extra
            want = _run(args, HOST)
            got = _run(args)                                      # (IGD_HOST_MAX_QUERIES = 0: the engine)
            assert want.returncode == 0 and got.returncode == 0, got.stderr
            assert got.stdout == want.stdout and b"n_flanked" in got.stdout and b"Any dataset within" in got.stdout, args
