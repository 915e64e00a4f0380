"""The row seam of the chunk driver (run_set_chunks, engine/host_common.hpp): IGD_HIP_SETS_ROW_BYTES (read once per process)
lowered so that a chunk holds two sets, alone and together with a batch seam (IGD_HIP_MAX_BATCH) and the large-set route
(IGD_SETS_BIG_MIN).  Each case runs in a child process with the variables set.

40 files (two bitmap words); seven sets of 0, 1, 70, 0, 130, 5 and 64 regions: empty sets at a chunk's start and end, sets of
more than one slice at IGD_SETS_SLICE_MIN = 64.  Everything is held against the host twins (search_host, support_host,
igdc_coverage_host), exactly: matrix and totals."""
import os
import subprocess
import sys

import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu

CHILD = r"""
import ctypes as C, os, random, sys
import numpy as np
sys.path.insert(0, %(tests)r); sys.path.insert(0, %(root)r)
from helpers import short_tmpdir
import sets_fixtures as F
from test_coverage_host import HostCov
from test_support_host import cli_rule
from igd_amd import Database, search_host, support_host
from igd_amd import _native as N

NFILES, SIZES = 40, [0, 1, 70, 0, 130, 5, 64]
kinds = %(kinds)r
env = lambda n: int(os.environ[n]) if n in os.environ else None
assert env("IGD_HIP_SETS_ROW_BYTES") == 2 * NFILES * 8
p = F.plan(SIZES, NFILES, big_min=env("IGD_SETS_BIG_MIN"), max_batch=env("IGD_HIP_MAX_BATCH"), row_bytes=env("IGD_HIP_SETS_ROW_BYTES"))
assert p["rowCap"] == 2
for kind in kinds:
    ch = p[kind]["chunks"]
    assert len(ch) >= 3 and max(c["rows"] for c in ch) == 2, (kind, ch)       # the seam is crossed, more than once
    assert p[kind]["sliceLen"] == 64 < max(SIZES)                               # sets of more than one slice
    if env("IGD_HIP_MAX_BATCH"):                                                # set 4 is cut: it opens a second chunk
        assert sum(c["first"] == 4 for c in ch) == 2, (kind, ch)
if env("IGD_SETS_BIG_MIN"):
    assert sum(c["bigs"] for c in p["search"]["chunks"]) == 2                   # both parts of set 4 take the batch pipeline

d = short_tmpdir("igr")
path, span, window, _ = F.wide_db(random.Random(41), d, "r", NFILES, F.NBP, 8)
(ichr, qs, qe), off = F.make_sets(np.random.default_rng(42), 1, F.NBP, span, SIZES, window)
nsets = len(SIZES)
db, hc = Database(path), HostCov(path)
assert db.nfiles == NFILES and N.hip().igd_hip_member_words(db.dev) == 2
part = lambda k: (ichr[off[k]:off[k + 1]], qs[off[k]:off[k + 1]], qe[off[k]:off[k + 1]])


def want(kind, v, mo=None):
    rows, tot = np.zeros((nsets, NFILES), np.int64), np.zeros(nsets, np.int64)
    for k in range(nsets):
        if kind == "search":
            rows[k], tot[k] = search_host(path, *part(k), v, min_overlap=mo)
        elif kind == "support":
            rows[k], tot[k] = support_host(path, *part(k), v, min_overlap=mo)
        else:
            rule, ev = cli_rule(db.gtype, v)
            rows[k], tot[k] = hc.coverage(*part(k), ev, rule)
    return rows, tot


call = dict(search=db.search_sets, support=db.support_sets, coverage=db.coverage_sets)
for kind in kinds:
    for v in (0, 500):
        rows, tot = call[kind](ichr, qs, qe, off, v)
        wrows, wtot = want(kind, v)
        assert np.array_equal(rows, wrows) and np.array_equal(tot, wtot), (kind, v)
        assert wtot[0] == 0 and wtot[3] == 0 and (wtot[[2, 4, 6]] > 0).all(), (kind, v, wtot)
    if kind != "coverage":
        rows, tot = call[kind](ichr, qs, qe, off, 0, min_overlap=50)
        wrows, wtot = want(kind, 0, 50)
        assert np.array_equal(rows, wrows) and np.array_equal(tot, wtot), (kind, "min_overlap")
        assert wrows.sum() < want(kind, 0)[0].sum()                             # the threshold drops something

# the three entry points ADD: non-zero output arrays through the raw entry points
H = N.hip()
rule, vf = Database.cli_dispatch(db.gtype, 500)
for kind in kinds:
    rows = (np.arange(nsets * NFILES, dtype=np.int64).reshape(nsets, NFILES) %% 97) + 3
    tot = np.arange(nsets, dtype=np.int64) * 1000 + 7
    pat_rows, pat_tot = rows.copy(), tot.copy()
    a = [db.dev, ichr.ctypes.data, qs.ctypes.data, qe.ctypes.data, off.ctypes.data, nsets, vf, rule]
    if kind == "search":
        rc = H.igd_hip_search_sets(*a, 0, rows.ctypes.data, tot.ctypes.data)
    elif kind == "support":
        rc = H.igd_hip_support_sets(*a, rows.ctypes.data, tot.ctypes.data)
    else:
        rc = H.igd_hip_coverage_sets(*a, rows.ctypes.data, tot.ctypes.data)
    assert rc == 0, H.igd_hip_last_error()
    wrows, wtot = want(kind, 500)
    assert wrows.any() and np.array_equal(rows, pat_rows + wrows) and np.array_equal(tot, pat_tot + wtot), kind
db.close(); hc.close()
print("ok")
"""

ROW = {"IGD_HIP_SETS_ROW_BYTES": str(2 * 40 * 8)}
ALL = ("search", "support", "coverage")


@pytest.mark.parametrize("extra,kinds", [
    ({}, ALL),                                                          # chunks of two sets
    ({"IGD_HIP_MAX_BATCH": "97"}, ALL),                                 # ... and set 4 cut inside a chunk: row and batch seam in one call
    ({"IGD_HIP_MAX_BATCH": "97", "IGD_SETS_BIG_MIN": "100"}, ("search",)),   # ... and the cut set down the batch pipeline
], ids=["rows", "rows-batch", "rows-batch-big"])
def test_sets_cross_the_row_seam(extra, kinds):
    code = CHILD % dict(tests=os.path.join(ROOT, "tests"), root=ROOT, kinds=tuple(kinds))
    env = {k: v for k, v in os.environ.items() if k not in ("IGD_HIP_MAX_BATCH", "IGD_SETS_BIG_MIN")}
    env.update(ROW, **extra)
    p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith(b"ok"), p.stderr.decode()[-3000:]
