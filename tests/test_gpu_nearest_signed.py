"""GPU: signed nearest distances and their histogram per set and dataset (igd_hip_nearest_signed / igd_hip_nearest_signed_dev /
igd_hip_nearest_hist, kernels igd_nearest_rows<., ., true>, igd_nearest_rowdecode and igd_nearest_hist; Database.nearest_signed /
nearest_hist / nearest_hist_files / nearest_signed_dev, `-N W -H e1,e2,...`).

The device must equal, on every integer, the definition restated in tests/nearest_signed_ref.py (a numpy broadcast over the
interval lists this test wrote) and the host route (igdc_nearest_signed_host / igdc_nearest_hist_host).  Every output is handed
over full of 0x5a: a call defines every word."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import igd_amd
from helpers import ROOT, short_tmpdir, write_bed
from nearest_ref import MAX_WINDOW, ListDb, clustered_lists, mixed_regions, placed_db, placed_regions, sparse_lists, windows
from nearest_signed_ref import NO_RECORD, edge_lists, ref_hist, ref_signed_rows
from test_gpu_nearest import lds_files
from test_nearest_signed_host import identities, top_db, top_regions
from test_sets_cli import _write_list
from test_support_host import HOST, NUMPY_DBS, _run

pytestmark = pytest.mark.gpu
GARBAGE = 0x5a5a5a5a
GARBAGE64 = 0x5a5a5a5a5a5a5a5a


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igh")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def check(db, ldb, ichr, qs, qe, W, v=None, off=None, edges=((0, 1),), host=True):
    """the signed rows, sdmin and the histograms of one call against the definition, the host route and the unsigned calls"""
    want, wmin = ref_signed_rows(ldb, ichr, qs, qe, W, v)
    sdist, sdmin = db.nearest_signed(ichr, qs, qe, W, value_filter=v, sdist=np.full((len(qs), db.nfiles), GARBAGE, np.int32))
    bad = np.flatnonzero((sdist != want).any(axis=1) | (sdmin != wmin))
    assert sdist.dtype == np.int32 and len(bad) == 0, (W, v, bad[:5].tolist(), [(sdist[i].tolist()[:8], want[i].tolist()[:8]) for i in bad[:3]])
    identities(sdist, sdmin, *db.nearest(ichr, qs, qe, W, value_filter=v))
    if host:
        hs, hmin = igd_amd.nearest_signed_host(ldb.path, ichr, qs, qe, W, value_filter=v)
        assert np.array_equal(hs, sdist) and np.array_equal(hmin, sdmin), (W, v)
    if off is None:
        off = np.array([0, len(qs)], np.int64)
    nw = db.nearest_sets(ichr, qs, qe, off, W, value_filter=v).n_within
    for e in edges:
        nh = db.nearest_hist(ichr, qs, qe, off, W, e, value_filter=v, hist=np.full((len(off) - 1, len(e) + 1, db.nfiles + 1), GARBAGE64, np.int64))
        assert nh.hist.dtype == np.int64 and np.array_equal(nh.hist, ref_hist(want, wmin, off, e)), (W, v, e)
        assert np.array_equal(nh.hist.sum(axis=1), nw), (W, v, e)
        if host:
            assert np.array_equal(igd_amd.nearest_hist_host(ldb.path, ichr, qs, qe, off, W, e, value_filter=v).hist, nh.hist), (W, v, e)
    return want, wmin


@pytest.mark.parametrize("case", range(len(NUMPY_DBS)))
def test_device_equals_the_definition_on_the_four_database_shapes(case, workdir):
    from igd_amd import Database
    rng = random.Random(9700 + case)
    nbp, gtype, nfiles, nctg, span_tiles = NUMPY_DBS[case]
    files, span = clustered_lists(rng, nbp, nfiles, nctg, span_tiles)
    ldb = ListDb(workdir, "c%d" % case, files, nbp, gtype)
    ichr, qs, qe = mixed_regions(rng, nctg, nbp, span, 500)
    off = np.array([0, 0, 1, 6, 6, 206, len(qs)], np.int64)
    db = Database(ldb.path)
    try:
        up = down = False
        for W in windows(nbp):
            for v in (None, 500):
                want, _ = check(db, ldb, ichr, qs, qe, W, v, off, edge_lists(W))
                up |= bool(((want < 0) & (want != NO_RECORD)).any())
                down |= bool((want > 0).any())
        assert up and down
    finally:
        db.close()


def test_placed_cases(workdir):
    from igd_amd import Database
    nbp = 1 << 14
    ldb = placed_db(workdir, nbp, "hplaced")
    (ichr, qs, qe), _ = placed_regions(nbp)
    db = Database(ldb.path)
    try:
        for W in windows(nbp) + [2 * nbp, 500]:
            for v in (None, 500):
                check(db, ldb, ichr, qs, qe, W, v, np.array([0, 5, 5, len(qs)], np.int64), edge_lists(W))
        # the expected values by hand
        a, amin = db.nearest_signed(ichr, qs, qe, 500)
        b, _ = db.nearest_signed(ichr, qs, qe, 500, value_filter=500)
        assert a[0, 0] == 1 and a[1, 0] == -1                             # book-ended downstream, upstream
        assert a[4, 2] == -51 and amin[4] == -51                          # the tie: upstream wins
        assert a[3, 1] == -11 and b[3, 1] == 301                          # the filter flips the side
        for W in (1, 51, 301):
            s, _ = db.nearest_signed(ichr, qs, qe, W)
            assert s[0, 0] == 1 and s[1, 0] == -1 and s[4, 2] == (-51 if W >= 51 else NO_RECORD)
            assert db.nearest_signed(ichr, qs, qe, W, value_filter=500)[0][3, 1] == (301 if W >= 301 else NO_RECORD)
        big, bmin = db.nearest_signed(ichr, qs, qe, MAX_WINDOW)
        assert big[11, 4] == 0 and big[12, 4] == -1 and (big[18:] == NO_RECORD).all() and (bmin[18:] == NO_RECORD).all()
    finally:
        db.close()
    # the largest key, 2^31 + 1, survives the table, the decoding and the histogram
    tdb = top_db(workdir, nbp, "htop")
    ichr, qs, qe = top_regions()
    db = Database(tdb.path)
    try:
        want, _ = check(db, tdb, ichr, qs, qe, MAX_WINDOW, edges=[(-2 ** 30, 0, 2 ** 30), (-2 ** 31 + 1, 2 ** 31 - 1)])
        assert want[0, 0] == 2 ** 30 and want[1, 1] == -2 ** 30
        want, _ = check(db, tdb, ichr, qs, qe, MAX_WINDOW - 1)
        assert want[0, 0] == NO_RECORD and want[1, 1] == NO_RECORD
    finally:
        db.close()


@pytest.mark.parametrize("nfiles", [1, 63, 64, 65, 4096, 4097])
def test_file_counts_small_calls_and_edge_counts(nfiles, workdir):
    """1, 63, 64 and 65 files (the any-dataset column moves into a second column block at 64) and the two sides of the LDS form's
    limit; calls of 1, 4, 5 and 64 regions (one wave, one workgroup, a second workgroup); 1, 2 and 63 edges"""
    from igd_amd import Database
    assert lds_files() == 4096
    rng = random.Random(9800 + nfiles)
    nbp = 1 << 12
    span = 40 * nbp
    ldb = ListDb(workdir, "f%d" % nfiles, sparse_lists(rng, nbp, nfiles, 2 if nfiles > 100 else 9, span), nbp, 1)
    db = Database(ldb.path)
    try:
        assert db.nfiles == nfiles
        ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 64)
        seen = set()
        # (thousands of files: the reference's 63-edge broadcast is what takes time, so fewer combinations)
        for n in (1, 4, 5, 64) if nfiles < 100 else (5, 64):
            off = np.array([0, n // 2, n], np.int64)
            for W in (0, 700, 3 * nbp + 5, MAX_WINDOW) if nfiles < 100 else (700, MAX_WINDOW):
                e63 = tuple(int(x) for x in np.linspace(-W - 1, W + 1, 63).astype(np.int64)) if W >= 31 else tuple(range(-31, 32))
                for v in (None, 500):
                    want, _ = check(db, ldb, ichr[:n], qs[:n], qe[:n], W, v, off, [(0,), (0, 1), e63], host=(n == 64))
                    seen |= set(np.sign(want[want != NO_RECORD]).tolist())
        assert seen == {-1, 0, 1}
        # the wide form decodes its rows whether sdmin is wanted or not (and the LDS form has nothing to decode)
        import torch
        dev = torch.device("cuda", 0)
        t = [torch.from_numpy(a).to(dev) for a in (ichr, qs, qe)]
        d_s = torch.full((64, nfiles), GARBAGE, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        db.nearest_signed_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 64, 700, d_s.data_ptr(), None)
        db.sync()
        assert np.array_equal(d_s.cpu().numpy(), ref_signed_rows(ldb, ichr, qs, qe, 700)[0])
    finally:
        db.close()


def test_a_wave_resets_its_table_and_an_empty_row_lies_between_two_full_ones(workdir):
    """4 x igd_hip_nearest_grid + 3 regions: the grid is full and its first three waves meet a second region; and 2 x 8 192 + 3
    regions: they meet a third one.  Their first and third regions cover the whole contig (every file at distance 0), their
    second ones are a region on an unknown contig (the row of INT32_MIN that is stored without reading the table), a
    zero-length region and a short one: a table that was not reset would leak zeros into them."""
    from igd_amd import Database
    from igd_amd import _native as N
    rng = random.Random(9900)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 12, 2, 20)
    ldb = ListDb(workdir, "w", files, nbp, 1)
    nq = 2 * 8192 + 3
    assert N.hip().igd_hip_nearest_grid(8195) == 2048 and 8195 == 4 * N.hip().igd_hip_nearest_grid(8195) + 3
    assert N.hip().igd_hip_nearest_grid(nq) == 2048
    ichr, qs, qe = mixed_regions(rng, 2, nbp, span, nq)
    ichr[:3], qs[:3], qe[:3] = 0, 0, span + 6 * nbp
    ichr[8192:8195], qs[8192:8195], qe[8192:8195] = [-1, 0, 1], [5, 3 * nbp, 7 * nbp], [9, 3 * nbp, 7 * nbp + 20]
    ichr[16384:], qs[16384:], qe[16384:] = 0, 0, span + 6 * nbp
    db = Database(ldb.path)
    try:
        for n, off in ((8195, [0, 700, 1800, 1800, 8195]), (nq, [0, 0, 1, 256, 512, 769, 1869, nq])):
            for W, v in ((nbp, None), (300, 500)):
                want, _ = check(db, ldb, ichr[:n], qs[:n], qe[:n], W, v, np.array(off, np.int64), [(-300, 0, 1, 301)], host=(v is None))
                assert (want[:3] == 0).all() and (want[8192] == NO_RECORD).all() and (want[8193:8195] != 0).any()
                assert n < nq or (want[16384:] == 0).all()
    finally:
        db.close()


def test_sets_around_the_slice_length(workdir):
    """sets of 0, 1, 255, 256, 257 and 1 100 regions: slices that end inside, at and past a slice of 256"""
    from igd_amd import Database
    rng = random.Random(10000)
    nbp = 1 << 11
    files, span = clustered_lists(rng, nbp, 40, 1, 25)
    ldb = ListDb(workdir, "s", files, nbp, 1)
    sizes = [0, 1, 255, 256, 257, 0, 1100]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, int(off[-1]))
    db = Database(ldb.path)
    try:
        for W, v in ((0, None), (nbp, None), (3 * nbp + 5, 500)):
            check(db, ldb, ichr, qs, qe, W, v, off, [(0,), (0, 1), tuple(range(-31, 32)), (-nbp, -100, 0, 1, 101, nbp + 1)])
        ns = db.nearest_sets(ichr, qs, qe, off, nbp)
        nh = db.nearest_hist(ichr, qs, qe, off, nbp, (0, 1))
        assert np.array_equal(nh.hist[:, 1], ns.n_overlap) and nh.hist[6].any() and not nh.hist[0].any() and not nh.hist[5].any()
    finally:
        db.close()


SEAM = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import short_tmpdir
import nearest_ref as R
import nearest_signed_ref as S
from igd_amd import Database
d = short_tmpdir("igs")
rng = random.Random(13)
nbp = 1 << 12
files, span = R.clustered_lists(rng, nbp, 40, 2, 20)
ldb = R.ListDb(d, "b", files, nbp, 1)
db = Database(ldb.path)
sizes = [0, 1, 255, 256, 257, 0, 1100, 3]
off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
ichr, qs, qe = R.mixed_regions(rng, 2, nbp, span, int(off[-1]))
for W, v in ((nbp, None), (3 * nbp + 5, 500), (0, None)):
    want, wmin = S.ref_signed_rows(ldb, ichr, qs, qe, W, v)
    for n in (0, 1, 96, 97, 98, 195, len(qs)):
        s, smin = db.nearest_signed(ichr[:n], qs[:n], qe[:n], W, value_filter=v, sdist=np.full((n, 40), 0x5a5a5a5a, np.int32))
        assert np.array_equal(s, want[:n]) and np.array_equal(smin, wmin[:n]), (W, v, n)
    nw = db.nearest_sets(ichr, qs, qe, off, W, value_filter=v).n_within
    for e in ((0, 1), (-nbp, -100, 0, 1, 101, nbp + 1), tuple(range(-31, 32))):
        nh = db.nearest_hist(ichr, qs, qe, off, W, e, value_filter=v, hist=np.full((len(sizes), len(e) + 1, 41), 0x5a5a5a5a5a5a5a5a, np.int64))
        assert np.array_equal(nh.hist, S.ref_hist(want, wmin, off, e)), (W, v, e)
        assert np.array_equal(nh.hist.sum(axis=1), nw), (W, v, e)
    assert nh.hist[4].any() and nh.hist[6].any() and not nh.hist[0].any()
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)


@pytest.mark.parametrize("env", [{"IGD_HIP_NEAREST_ROW_BYTES": str(97 * 160 + 5)},
                                 {"IGD_HIP_NEAREST_ROW_BYTES": str(333 * 160), "IGD_HIP_SETS_ROW_BYTES": "2000"}])
def test_calls_straddle_the_chunk_seams(env):
    """chunks of 97 regions (a row budget of 97 rows of 160 bytes and a little) and of 333: no seam is a multiple of 64, the sets
    of 255 to 1 100 regions are cut by region chunks and start mid-chunk; groups of two sets (a budget of 2 000 bytes against
    the 3 x 41 x 8 = 984 of a set's (0, 1) histogram) and of one set (the longer edge lists: 2 296 and 20 992 bytes per set).
    The variables are read once per process: a child process each."""
    p = subprocess.run([sys.executable, "-c", SEAM], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env),
                       timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def test_resident_rows_on_a_torch_stream(workdir):
    import torch
    from igd_amd import Database
    rng = random.Random(10100)
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
            d_s = torch.full((300, 33), GARBAGE, dtype=torch.int32, device=dev)
            d_min = torch.full((300,), GARBAGE, dtype=torch.int32, device=dev)
            stream.synchronize()
            db.nearest_signed_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 300, 2 * nbp, d_s.data_ptr(), d_min.data_ptr(),
                                  value_filter=500, stream=stream.cuda_stream)
            db.sync(stream.cuda_stream)
            want, wmin = ref_signed_rows(ldb, ichr, qs, qe, 2 * nbp, 500)
            assert np.array_equal(d_s.cpu().numpy(), want) and np.array_equal(d_min.cpu().numpy(), wmin)
    finally:
        db.close()


def test_bad_arguments_change_nothing_and_empty_calls_are_fine(workdir):
    from igd_amd import Database
    from igd_amd import _native as N
    from igd_amd.database import IgdError
    rng = random.Random(10200)
    nbp = 1 << 12
    files, span = clustered_lists(rng, nbp, 3, 1, 6)
    ldb = ListDb(workdir, "e", files, nbp, 1)
    ichr, qs, qe = mixed_regions(rng, 1, nbp, span, 20)
    db = Database(ldb.path)
    try:
        for W in (-1, MAX_WINDOW + 1):
            s = np.full((20, 3), GARBAGE, np.int32)
            h = np.full((1, 3, 4), GARBAGE64, np.int64)
            with pytest.raises(IgdError):
                db.nearest_signed(ichr, qs, qe, W, sdist=s)
            with pytest.raises(IgdError):
                db.nearest_hist(ichr, qs, qe, [0, 20], W, (0, 1), hist=h)
            assert (s == GARBAGE).all() and (h == GARBAGE64).all()
        for off in ([1, 20], [0, 15, 10, 20]):
            with pytest.raises(IgdError):
                db.nearest_hist(ichr, qs, qe, off, 100, (0, 1))
        for bad in ([], [1, 0], [0, 0], list(range(64))):
            with pytest.raises(IgdError):
                db.nearest_hist(ichr, qs, qe, [0, 20], 100, bad)
        # the native call refuses the same lists before it writes anything
        c, s_, e_ = (np.ascontiguousarray(a, np.int32) for a in (ichr, qs, qe))
        off = np.array([0, 20], np.int64)
        for edges, ne in (((1, 0), 2), ((0, 0), 2), (tuple(range(64)), 64), ((0,), 0)):
            ed = np.array(edges, np.int32)
            h = np.full((1, 65, 4), GARBAGE64, np.int64)
            rc = N.hip().igd_hip_nearest_hist(db.dev, c.ctypes.data, s_.ctypes.data, e_.ctypes.data, off.ctypes.data, 1, 100,
                                              N.IGD_HIP_NO_VALUE_FILTER, ed.ctypes.data, ne, h.ctypes.data)
            assert rc != 0 and (h == GARBAGE64).all(), edges
        s, smin = db.nearest_signed(ichr[:0], qs[:0], qe[:0], 100)
        assert s.shape == (0, 3) and smin.shape == (0,)
        nh = db.nearest_hist(ichr[:0], qs[:0], qe[:0], [0, 0, 0], 100, (0, 1), hist=np.full((2, 3, 4), GARBAGE64, np.int64))
        assert nh.hist.shape == (2, 3, 4) and not nh.hist.any()
        assert db.nearest_hist(ichr[:0], qs[:0], qe[:0], [0], 100, (0, 1)).hist.shape == (0, 3, 4)
        nh = db.nearest_hist(ichr, qs, qe, [0, 0, 20, 20], MAX_WINDOW, (0,))
        assert not nh.hist[0].any() and not nh.hist[2].any() and nh.hist[1].any()
    finally:
        db.close()


@pytest.mark.parametrize("extra", [[], ["-v", "500"]])
def test_cli_engine_route_prints_what_the_host_route_prints(extra, workdir):
    rng = random.Random(10300)
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
        for W, H in (("0", "0,1"), (str(nbp), "-%d,-100,0,1,101,%d" % (nbp, nbp + 1)), (str(MAX_WINDOW), ",".join(str(i) for i in range(-31, 32)))):
            args = ["search", ldb.path] + sel + ["-N", W, "-H", H] + extra
            want = _run(args, HOST)
            got = _run(args)                                      # (IGD_HOST_MAX_QUERIES = 0: the engine)
            assert want.returncode == 0 and got.returncode == 0, got.stderr
            assert got.stdout == want.stdout and b"n_within" in got.stdout and b"Any dataset within" in got.stdout, args
