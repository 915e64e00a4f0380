"""GPU: the four reductions over a slice table -- igd_nearest_reduce, igd_map_reduce, igd_nearest_hist, igd_flank_reldist -- past
one slice per workgroup.

All four loop `for (s = blockIdx.y; s < nSlices; s += gridDim.y)` and are launched with igd_hip_reduce_grid_y() rows of
workgroups.  A workgroup's SECOND slice is where these can go wrong: the per-slice accumulators must start from zero again, h[]
must be zeroed again behind the trailing barrier, the edges loaded before the loop must survive, part[] must not be overwritten
while wave 0 still reads it, and consecutive slices of one workgroup belong to different result rows.  Every test here asserts
from igd_hip_reduce_grid_y that there are more slices than the grid has rows.

Everything goes through Database.nearest_sets / map_sets / nearest_hist / flank_reldist and is compared integer for integer with
the numpy references (nearest_ref, map_ref, nearest_signed_ref, flank_ref); outputs are handed over full of 0x5a."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

from flank_ref import MIDPOINTS, ref_flanks
from flank_ref import ref_hist as ref_reldist
from helpers import ROOT, short_tmpdir
from map_ref import ref_rows as ref_map_rows
from map_ref import ref_sets as ref_map_sets
from nearest_ref import MAX_WINDOW, ListDb, mixed_regions, ref_rows, ref_sets, sparse_lists
from nearest_signed_ref import ref_hist, ref_signed_rows

pytestmark = pytest.mark.gpu
GARBAGE64 = 0x5a5a5a5a5a5a5a5a
NFILES = 4097
W = 700


def garbage(*shape):
    return np.full(shape, GARBAGE64, np.int64)


class Big:
    """4 097 files under the shipped constants: 65 column blocks, 16 384 / 65 = 252 rows of workgroups.  2 x 252 + 3 sets of one to
    three regions, a slice each: every workgroup takes a second slice and three take a third.  The regions of the first 252 sets
    -- the first round -- cover the whole contig, so every file column of their rows is non-zero: an accumulator or a counter
    that is not cleared leaks them into the second round's rows, two thirds of whose regions lie on unknown contigs."""

    def __init__(self):
        from igd_amd import Database
        from igd_amd import _native as N
        self.dir = short_tmpdir("igr")
        rng = random.Random(14100)
        nbp = 1 << 12
        span = 40 << 12
        self.ldb = ListDb(self.dir, "big", sparse_lists(rng, nbp, NFILES, 2, span), nbp, 1)
        self.grid_y = N.hip().igd_hip_reduce_grid_y
        self.gy = gy = self.grid_y(NFILES + 1, 1 << 30)
        assert gy == 252 and self.grid_y(NFILES, 1 << 30) == 252          # (the nearest family's columns, and map's)
        self.ns = ns = 2 * gy + 3
        sizes = [rng.choice([1, 2, 3]) for _ in range(ns)]
        self.off = off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.ichr, self.qs, self.qe = mixed_regions(rng, 1, nbp, span, int(off[-1]))
        first = int(off[gy])
        self.ichr[:first], self.qs[:first], self.qe[:first] = 0, 0, span + 6 * nbp
        # one slice per set (no set is longer than a slice), more slices than twice the grid's rows, whatever the launch is asked
        assert max(sizes) <= 256 and ns > 2 * gy and self.grid_y(NFILES + 1, ns) == gy and self.grid_y(NFILES, ns) == gy
        self.db = Database(self.ldb.path)
        assert self.db.nfiles == NFILES
        self.regions = (self.ichr, self.qs, self.qe)
        self._refs = {}

    def ref(self, key, make):
        """a reference computed once and shared (nobody writes to it)"""
        if key not in self._refs:
            self._refs[key] = make()
            for a in self._refs[key]:
                a.setflags(write=False)
        return self._refs[key]

    def later_rows_are_mixed(self, stat):
        """among the sets of the second and third round some rows are all zero and some are not"""
        later = stat[self.gy:].reshape(self.ns - self.gy, -1)
        assert (later == 0).all(axis=1).any() and (later != 0).any(axis=1).any()

    def close(self):
        self.db.close()
        shutil.rmtree(self.dir, ignore_errors=True)


@pytest.fixture(scope="module")
def big():
    b = Big()
    yield b
    b.close()


def test_nearest_reduce_second_and_third_round(big):
    dist, dmin = big.ref("nearest", lambda: ref_rows(big.ldb, *big.regions, W))
    want = ref_sets(dist, dmin, big.off)
    got = big.db.nearest_sets(*big.regions, big.off, W, out=[garbage(big.ns, NFILES + 1) for _ in range(3)])
    for name, g, w in zip(("n_within", "n_overlap", "sum_dist"), got[:3], want):
        assert g.dtype == np.int64 and np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist())
    assert big.ns > 2 * big.gy and (want[1][:big.gy] > 0).all()
    big.later_rows_are_mixed(want[0])
    big.later_rows_are_mixed(want[2])


@pytest.mark.parametrize("op", ["sum", "count"])
def test_map_reduce_second_and_third_round(op, big):
    """op count is the route without agg rows: agg_sum is summed from the counts"""
    count, agg = big.ref("map " + op, lambda: ref_map_rows(big.ldb, *big.regions, op))
    want = ref_map_sets(count, agg, big.off)
    got = big.db.map_sets(*big.regions, big.off, op, out=[garbage(big.ns, NFILES) for _ in range(3)])
    for name, g, w in zip(("n_hit", "pairs", "agg_sum"), got[:3], want):
        assert g.dtype == np.int64 and np.array_equal(g, w), (op, name, np.argwhere(g != w)[:5].tolist())
    assert big.ns > 2 * big.gy and (want[0][:big.gy] > 0).all() and (want[1][:big.gy] >= 2).all()
    big.later_rows_are_mixed(want[0])
    big.later_rows_are_mixed(want[2])


@pytest.mark.parametrize("edges", [(0, 1), (-300, 0, 1, 301)])
def test_nearest_hist_second_and_third_round(edges, big):
    sdist, sdmin = big.ref("signed", lambda: ref_signed_rows(big.ldb, *big.regions, W))
    want = ref_hist(sdist, sdmin, big.off, edges)
    got = big.db.nearest_hist(*big.regions, big.off, W, edges, hist=garbage(big.ns, len(edges) + 1, NFILES + 1)).hist
    assert got.dtype == np.int64 and np.array_equal(got, want), (edges, np.argwhere(got != want)[:5].tolist())
    # the first round: every region overlaps every file, distance 0, the bin with one edge (two edges) at or below 0
    assert big.ns > 2 * big.gy and (want[:big.gy, edges.index(0) + 1] > 0).all()
    big.later_rows_are_mixed(want)


@pytest.mark.parametrize("nbins", [2, 5])
def test_flank_reldist_second_and_third_round(nbins, big):
    """measure midpoints at the largest window: a region over the whole contig has the two records of a file on either side of its
    midpoint for about half of the files, and a record of SOME file on either side, so the first round's rows are non-zero in
    those columns and in the any-dataset column (no region is flanked by a file whose records lie on one side of it: `every
    file column` cannot hold for this statistic)"""
    want4 = big.ref("flank", lambda: ref_flanks(big.ldb, *big.regions, MAX_WINDOW, MIDPOINTS))
    want = ref_reldist(*want4, big.off, nbins)
    got = big.db.flank_reldist(*big.regions, big.off, MAX_WINDOW, nbins, measure=MIDPOINTS, hist=garbage(big.ns, nbins, NFILES + 1)).hist
    assert got.dtype == np.int64 and np.array_equal(got, want), (nbins, np.argwhere(got != want)[:5].tolist())
    first = want[:big.gy].sum(axis=1)
    assert big.ns > 2 * big.gy and (first[:, -1] > 0).all() and ((first > 0).sum(axis=1) > NFILES // 3).all()
    big.later_rows_are_mixed(want)


# ---- a lowered grid: IGD_HIP_REDUCE_WGS is read once per process, a child process each ---------------------------------------
ROUNDS = r"""
import os, random, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from helpers import short_tmpdir
import nearest_ref as R
import nearest_signed_ref as S
import flank_ref as F
import map_ref as M
from igd_amd import Database
from igd_amd import _native as N
nfiles, want_gy = int(sys.argv[1]), int(sys.argv[2])
SLICE = 256
G64 = 0x5a5a5a5a5a5a5a5a
d = short_tmpdir("igo")
rng = random.Random(23)
nbp = 1 << 12
files, span = R.clustered_lists(rng, nbp, nfiles, 2, 20, min_value=-300)
ldb = R.ListDb(d, "b", files, nbp, 1)
db = Database(ldb.path)
sizes = [300, 0, 1, 255, 256, 257, 0, 1100, 3, 40]
off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
nq = int(off[-1])
ichr, qs, qe = R.mixed_regions(rng, 2, nbp, span, nq)
ichr[:300], qs[:300], qe[:300] = 0, 0, span + 6 * nbp        # set 0: the whole contig, every file, a slice of 256 and one of 44
ichr[off[9]:] = -1                                            # the last set: an unknown contig, its slice must add nothing
a7 = int(off[7]) + 768                                        # set 7's fourth slice: the whole of the other contig
ichr[a7:a7 + 256], qs[a7:a7 + 256], qe[a7:a7 + 256] = 1, 0, span + 6 * nbp
ichr[off[2]], qs[off[2]], qe[off[2]] = 0, files[0][0][1], files[0][0][2]      # set 2: one region, on file 0's first record
assert files[0][0][0] == "chr1" and ldb.ctgs[0] == "chr1"


def slice_counts(step):
    # slices per chunk of `step` regions: a slice is at most 256 regions of one set within one chunk
    out = []
    for c0 in range(0, nq, step):
        c1 = min(c0 + step, nq)
        out.append(sum(-(-(min(int(off[k + 1]), c1) - max(int(off[k]), c0)) // SLICE) for k in range(len(sizes))
                       if min(int(off[k + 1]), c1) > max(int(off[k]), c0)))
    return out


def rounds(ncols, row_bytes, bytes_per_region):
    # the launch's rows of workgroups are what the table of the test says, and FEWER than the slices: second rounds happen
    # (without IGD_HIP_REDUCE_WGS this fails: the grid then has a row per slice)
    step = nq if row_bytes is None else int(row_bytes) // bytes_per_region
    per_chunk = slice_counts(step)
    assert row_bytes is not None or per_chunk == [14], per_chunk
    assert row_bytes is None or sum(1 for n in per_chunk if n > want_gy) >= 2, per_chunk
    for n in per_chunk:
        gy = N.hip().igd_hip_reduce_grid_y(ncols, n)
        assert gy == min(want_gy, n), "igd_hip_reduce_grid_y(%%d, %%d) is %%d, not %%d" %% (ncols, n, gy, min(want_gy, n))
    assert N.hip().igd_hip_reduce_grid_y(ncols, max(per_chunk)) == want_gy < max(per_chunk), (ncols, per_chunk, want_gy)


nrb, mrb = os.environ.get("IGD_HIP_NEAREST_ROW_BYTES"), os.environ.get("IGD_HIP_MAP_ROW_BYTES")
W = 3 * nbp + 5
# igd_nearest_reduce
rounds(nfiles + 1, nrb, 4 * nfiles)
dist, dmin = R.ref_rows(ldb, ichr, qs, qe, W)
want = R.ref_sets(dist, dmin, off)
got = db.nearest_sets(ichr, qs, qe, off, W, out=[np.full((len(sizes), nfiles + 1), G64, np.int64) for _ in range(3)])
for g, w in zip(got[:3], want):
    assert np.array_equal(g, w), ("nearest_sets", np.argwhere(g != w)[:5].tolist())
assert (want[1][0, :nfiles] == 300).all() and not want[0][9].any() and not want[0][1].any() and want[1][2, 0] == 1 and want[0][7].all()
# igd_map_reduce
for op in M.OPS:
    rounds(nfiles, mrb, (4 if op == "count" else 12) * nfiles)
    count, agg = M.ref_rows(ldb, ichr, qs, qe, op)
    want = M.ref_sets(count, agg, off)
    got = db.map_sets(ichr, qs, qe, off, op, out=[np.full((len(sizes), nfiles), G64, np.int64) for _ in range(3)])
    for g, w in zip(got[:3], want):
        assert np.array_equal(g, w), ("map_sets", op, np.argwhere(g != w)[:5].tolist())
    assert (want[0][0] == 300).all() and not want[0][9].any() and not want[1][6].any() and want[1][7].any()
# igd_nearest_hist: 1, 2 and 63 edges (63: every wave's flush loop runs 16 times per slice)
rounds(nfiles + 1, nrb, 4 * nfiles)
sdist, sdmin = S.ref_signed_rows(ldb, ichr, qs, qe, W)
spread = tuple(int(x) for x in np.linspace(-W - 1, W + 1, 63).astype(np.int64))
assert len(set(spread)) == 63 and spread[0] == -W - 1 and spread[-1] == W + 1
for edges in ((0,), (0, 1), tuple(range(-31, 32)), spread):
    want = S.ref_hist(sdist, sdmin, off, edges)
    got = db.nearest_hist(ichr, qs, qe, off, W, edges, hist=np.full((len(sizes), len(edges) + 1, nfiles + 1), G64, np.int64)).hist
    assert np.array_equal(got, want), ("nearest_hist", len(edges), np.argwhere(got != want)[:5].tolist())
    assert want[0].sum() == 300 * (nfiles + 1) and not want[9].any() and not want[1].any() and want[7].any() and want[2].any()
    assert edges is not spread or (want.sum(axis=(0, 2)) > 0).sum() > 32      # (many bins are in use)
# igd_flank_reldist: 1, 2, 50 and 64 bins under both measures (64: every wave's flush loop runs 16 times per slice)
rounds(nfiles + 1, nrb, 8 * nfiles)
for ms in (F.EDGES, F.MIDPOINTS):
    want4 = F.ref_flanks(ldb, ichr, qs, qe, W, ms)
    for B in (1, 2, 50, 64):
        want = F.ref_hist(*want4, off, B)
        got = db.flank_reldist(ichr, qs, qe, off, W, B, measure=ms, hist=np.full((len(sizes), B, nfiles + 1), G64, np.int64)).hist
        assert np.array_equal(got, want), ("flank_reldist", ms, B, np.argwhere(got != want)[:5].tolist())
        assert not want[9].any() and not want[1].any() and want[7].any() and want[5].any()
        assert B < 50 or (want.sum(axis=(0, 2)) > 0).sum() > B // 2
db.close()
print("ok")
""" % (os.path.join(ROOT, "tests"), ROOT)

ENVS = [
    # IGD_HIP_REDUCE_WGS, files, rows of workgroups, further variables
    (3, 40, 3, {}),                                   # one column block; the slices strided by three
    (1, 63, 1, {}),                                   # the any-dataset column is lane 63 of block 0
    (1, 64, 1, {}),                                   # ... lane 0 of block 1, alone in its workgroup (map: 64 files are one full block)
    (2, 100, 1, {}),                                  # two column blocks, one workgroup each, which walks every slice of every row in order
    (2, 100, 1, {"IGD_HIP_NEAREST_ROW_BYTES": str(333 * 4 * 100), "IGD_HIP_MAP_ROW_BYTES": str(333 * 12 * 100)}),
]


@pytest.mark.parametrize("wgs,nfiles,gy,more", ENVS, ids=["wgs%d-%dfiles%s" % (e[0], e[1], "-chunks" if e[3] else "") for e in ENVS])
def test_lowered_grid_walks_many_slices_per_workgroup(wgs, nfiles, gy, more):
    """Sets of [300, 0, 1, 255, 256, 257, 0, 1100, 3, 40] regions are 14 slices in one chunk: 256 + 44 of set 0 (the whole contig:
    every file in every region), 1, 255, 256, 256 + 1, 4 x 256 + 76, 3, and 40 regions of an unknown contig that must add nothing.
    With three rows of workgroups, row 1 takes the slices 1, 4, 7, 10, 13: from a full slice of set 7 (whole-contig regions again)
    to the one that adds nothing; row 0 goes from the full first slice of set 0 to set 3, to the one-region slice of set 5.  With
    one row a workgroup walks all 14 in order: from the 44 whole-contig regions of set 0 to the one region of set 2, another row
    of the result; from a full slice of set 5 to its one-region slice.  The last case cuts the regions into chunks of 333 (map with
    agg rows, nearest), 166 (flank: two rows per region) and 999 (map count), so rounds happen in several launches.  The script
    asserts from igd_hip_reduce_grid_y that every launch has the rows of workgroups of this table and fewer than it has slices;
    without IGD_HIP_REDUCE_WGS it fails there."""
    env = dict(os.environ, IGD_HIP_REDUCE_WGS=str(wgs), **more)
    p = subprocess.run([sys.executable, "-c", ROUNDS, str(nfiles), str(gy)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-2000:]


def test_the_script_needs_the_lowered_grid():
    """the same script under the shipped constant: a row of workgroups per slice, no second round -- its grid assertion fails"""
    env = {k: v for k, v in os.environ.items() if k != "IGD_HIP_REDUCE_WGS"}
    p = subprocess.run([sys.executable, "-c", ROUNDS, "40", "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert p.returncode != 0 and b"AssertionError" in p.stderr and b"igd_hip_reduce_grid_y" in p.stderr, p.stderr.decode()[-2000:]
