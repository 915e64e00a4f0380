"""The batch's last launch (k_reduce_slabs) sums the slab by column blocks of 64 files: a lane is a file, 16 waves share a
block's rows, their partial sums meet in LDS and one wave adds them to hits[].  What that can get wrong, against the oracle:
  * file counts around the block width (1, 63, 64, 65, 127, 128, 129), on both sides of 1024 and the headline's 1900
    (29 blocks + 44 lanes);
  * a windowed batch (more files than LDS counters: windows and offsets that are no multiples of 64);
  * the four kinds of rows: 32-bit (merge join), 64-bit (bucket path), 64-bit where 32-bit were expected (the device found
    the batch unordered) and the DIRECT step's;
  * a broken order promise (nothing added), the batch total given or not, accumulation and IGD_HIP_FLAG_ZERO_FIRST;
  * the exact walks and the coverage sums riding in the same launch."""
import os
import shutil

import numpy as np
import pytest

from helpers import Oracle, short_tmpdir

pytestmark = pytest.mark.gpu

FLAG_SORTED, FLAG_BUCKET, FLAG_ZERO_FIRST, FLAG_SHORT = 1, 2, 8, 16
FILE_COUNTS = (1, 63, 64, 65, 127, 128, 129, 1024, 1025, 1900)
PER_FILE = 300
NBP_LOG = 14
NQ = 3000
# the smallest database that needs two windows: one file more than the 15 360 LDS counters of 64 bits -- two windows of
# 7712 and 7649 files, the second at file 7712 (120.5 column blocks in)
WINDOW_FILES = 15361


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("igc")
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def world(workdir):
    """files -> (path, position-sorted queries, the same queries in generation order, the oracle's counts and total): built
    once per file count and left unchanged"""
    from igd_amd import synth
    cache = {}

    def get(files, per_file=PER_FILE):
        if files not in cache:
            path = os.path.join(workdir, "c%d.igd" % files)
            synth.make_db(path, files=files, per_file=per_file, seed=40 + files, nbp_log=NBP_LOG, genome=synth.SMALL)
            # (100 .. 1999 bp: shorter than a tile, so the same batch also goes in under IGD_HIP_FLAG_SHORT)
            srt = synth.make_queries(NQ, seed=9, genome=synth.SMALL, min_len=100, max_len=1999, sorted_=True)
            shuf = synth.make_queries(NQ, seed=9, genome=synth.SMALL, min_len=100, max_len=1999, sorted_=False)
            orc = Oracle(path)
            try:
                want, wtot = orc.search(*srt, 0)
                w2, t2 = orc.search(*shuf, 0)
            finally:
                orc.close()
            assert wtot == t2 and np.array_equal(want, w2) and wtot == int(want.sum()) and wtot > 0
            want.setflags(write=False)
            cache[files] = (path, srt, shuf, want, wtot)
        return cache[files]
    return get


def _batch(db, torch, q, flags, hits=None, total=True):
    """one resident batch into `hits` (zeros when not given); returns (hits tensor, total tensor or None)"""
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev) for x in q]
    if hits is None:
        hits = torch.zeros(db.nfiles, dtype=torch.int64, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev) if total is True else total if total is not None else None
    torch.cuda.synchronize()
    db.search_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(q[1]), hits.data_ptr(),
                  tot.data_ptr() if tot is not None else None, v=0, flags=flags)
    return hits, tot


@pytest.mark.parametrize("files", FILE_COUNTS)
def test_file_counts_around_the_block_width(files, world):
    import torch
    from igd_amd import Database
    path, srt, _, want, wtot = world(files)
    db = Database(path)
    try:
        assert db.nfiles == files
        hits, tot = _batch(db, torch, srt, FLAG_SORTED)
        db.sync()
        np.testing.assert_array_equal(hits.cpu().numpy(), want)
        assert int(tot.item()) == wtot
    finally:
        db.close()


@pytest.mark.parametrize("kind", ["sorted", "bucket", "unordered", "direct"])
@pytest.mark.parametrize("files", [65, 1900])
def test_every_kind_of_rows(files, kind, world, monkeypatch):
    import torch
    from igd_amd import Database
    path, srt, shuf, want, wtot = world(files)
    if kind == "direct":
        monkeypatch.setenv("IGD_HIP_DIRECT", "1")
    db = Database(path)
    try:
        q, flags = {"sorted": (srt, FLAG_SORTED), "bucket": (shuf, FLAG_BUCKET), "unordered": (shuf, 0),
                    "direct": (srt, FLAG_SORTED | FLAG_SHORT)}[kind]
        hits, tot = _batch(db, torch, q, flags)
        db.sync()
        # the kernel that left the rows: the merge join (32-bit rows), the bucket path (64-bit rows; for "unordered" that is
        # the device's own switch, found in the control words where 32-bit rows were expected) or the DIRECT step
        assert db.last_scan_kernel() == {"sorted": "igd_scan_sorted", "bucket": "igd_scan_tiles", "unordered": "igd_scan_tiles",
                                         "direct": "igd_scan_direct"}[kind], db.last_scan_kernel()
        np.testing.assert_array_equal(hits.cpu().numpy(), want, err_msg="%d files, %s" % (files, kind))
        assert int(tot.item()) == wtot
    finally:
        db.close()


def test_windowed_pass(world):
    """Two windows of 7712 and 7649 files: neither the widths nor the second window's first file is a multiple of 64."""
    import torch
    from igd_amd import Database
    path, srt, shuf, want, wtot = world(WINDOW_FILES, per_file=200)
    db = Database(path)
    try:
        assert db.nfiles == WINDOW_FILES
        for q, flags in ((srt, FLAG_SORTED), (shuf, 0), (shuf, FLAG_BUCKET)):
            hits, tot = _batch(db, torch, q, flags)
            db.sync()
            np.testing.assert_array_equal(hits.cpu().numpy(), want, err_msg="flags %d" % flags)
            assert int(tot.item()) == wtot
    finally:
        db.close()


@pytest.mark.parametrize("files", [65, 1900])
def test_a_broken_promise_leaves_hits_and_total_as_they_were(files, world):
    import torch
    from igd_amd import Database
    from igd_amd.database import IgdError
    path, srt, shuf, want, wtot = world(files)
    db = Database(path)
    try:
        dev = torch.device("cuda", 0)
        before = (torch.arange(files, dtype=torch.int64, device=dev) * 7 + 3)
        hits, tot = _batch(db, torch, shuf, FLAG_SORTED, hits=before.clone(), total=torch.full((1,), 12345, dtype=torch.int64, device=dev))
        with pytest.raises(IgdError):
            db.sync()
        np.testing.assert_array_equal(hits.cpu().numpy(), before.cpu().numpy())
        assert int(tot.item()) == 12345
        # ... and the handle goes on counting
        hits, tot = _batch(db, torch, srt, FLAG_SORTED)
        db.sync()
        np.testing.assert_array_equal(hits.cpu().numpy(), want)
        assert int(tot.item()) == wtot
    finally:
        db.close()


@pytest.mark.parametrize("flags", [FLAG_SORTED, FLAG_BUCKET])
def test_batch_total_given_and_not_given(flags, world):
    import torch
    from igd_amd import Database
    path, srt, shuf, want, wtot = world(1900)
    db = Database(path)
    try:
        q = srt if flags == FLAG_SORTED else shuf
        hits, tot = _batch(db, torch, q, flags, total=None)
        db.sync()
        assert tot is None
        np.testing.assert_array_equal(hits.cpu().numpy(), want)
        hits, tot = _batch(db, torch, q, flags)
        db.sync()
        np.testing.assert_array_equal(hits.cpu().numpy(), want)
        assert int(tot.item()) == int(hits.sum().item()) == wtot
    finally:
        db.close()


@pytest.mark.parametrize("files", [129, 1900])
def test_batches_accumulate_until_zero_first(files, world):
    import torch
    from igd_amd import Database
    path, srt, shuf, want, wtot = world(files)
    db = Database(path)
    try:
        hits, tot = _batch(db, torch, srt, FLAG_SORTED)
        _batch(db, torch, shuf, FLAG_BUCKET, hits=hits, total=tot)       # (no ZERO_FIRST: the second batch adds)
        db.sync()
        np.testing.assert_array_equal(hits.cpu().numpy(), 2 * want)
        assert int(tot.item()) == 2 * wtot
        _batch(db, torch, srt, FLAG_SORTED | FLAG_ZERO_FIRST, hits=hits, total=tot)
        db.sync()
        np.testing.assert_array_equal(hits.cpu().numpy(), want)
        assert int(tot.item()) == wtot
    finally:
        db.close()


@pytest.mark.parametrize("files", [65, 1900])
def test_the_tail_rides_in_the_same_launch(files, world):
    """A few queries longer than four tiles (coverage sums + an exact walk of the last tile) and one first-tile query that
    ends before its tile starts (an exact walk): what the tail counts arrives in hits[] and the total next to the column sums."""
    import torch
    from igd_amd import Database
    path, srt, _, _, _ = world(files)
    nbp = 1 << NBP_LOG
    ichr, qs, qe = (a.copy() for a in srt)
    qe[100:2900:400] = qs[100:2900:400] + np.arange(5, 12) * nbp + 77            # seven long queries
    k = 1500
    qs[k] = (qs[k] // nbp) * nbp + 5
    qe[k] = qs[k] - 12                                                           # inverted across the tile's start
    o = np.lexsort((qs, ichr))
    q = (ichr[o], qs[o], qe[o])
    # what puts a query on the tail's lists (the engine does not tell their lengths): more than IGD_SHORT_TILES = 4 tiles,
    # or a first tile whose start the query's end does not reach
    assert int(((((q[2] - 1) >> NBP_LOG) - (q[1] >> NBP_LOG)) > 4).sum()) == 7
    assert int((q[2] <= (q[1] >> NBP_LOG << NBP_LOG)).sum()) == 1
    orc = Oracle(path)
    try:
        want, wtot = orc.search(*q, 0)
    finally:
        orc.close()
    db = Database(path)
    try:
        for flags in (FLAG_SORTED, 0, FLAG_BUCKET):
            hits, tot = _batch(db, torch, q, flags)
            db.sync()
            np.testing.assert_array_equal(hits.cpu().numpy(), want, err_msg="%d files, flags %d" % (files, flags))
            assert int(tot.item()) == wtot
    finally:
        db.close()
