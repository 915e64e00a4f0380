"""GPU: the Seqpare path (igd_amd/csrc/engine/seqpare.hpp: k_seq_key1, k_seq_key2, k_seq_greedy, k_seq_accumulate, seqpare_core)
past its first decomposition edges, bit for bit.

Every comparison is of doubles as words: Database.seqpare's raw sums against tests/seqpare_ref.py (the matching restated
literally over the CPU oracle's per-query overlaps), and sums / (Nq + nr - sums) against the oracle's orc_seqOverlaps.  No
tolerance: every value is a float32 quotient formed in a fixed order and added in double in a fixed order.  tests/
test_seqpare_ref.py holds the literal reference to the oracle on the same fixtures without a GPU; the conditions that keep a
fixture from going vacuous (group sizes, chain counters, classes of the groups) are asserted on the reference's diagnostics
there and again here.

  edges      (contig, dataset) groups of 1, 63, 64, 65, 128, 129 (the batch of 64), 1023, 1024, 1025 (SQ_CAP: LDS -> HBM hash sets),
             2048, 2049 (the HBM table's power of two steps from 4096 to 8192 slots); mixed lengths, then identical intervals
  chains     144 candidates per group with many equal scores: candidates knocked out inside a run of 64, candidates accepted
             although a rejected candidate of their run shares their row or column, candidates rejected by an earlier run
  near ties  float32 similarities one or two steps apart, and equal in float32 where the exact quotients differ
  waves      IGD_HIP_WG_PER_CU=1 in a child: 1 120 groups > 3 x compute units, so waves take a second and a third group: an LDS
             group behind an HBM group, a full group behind an empty one
  few        1, 2 and 257 groups: the second radix sort makes no pass, one pass, two passes
  carry      igd_hip_seqpare into garbage, igd_hip_seqpare_add over contig ranges with an empty range and a range without
             overlaps in the middle
  awkward    zero-length queries, 1-bp records, queries over several tiles, unknown contigs, duplicates"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import seqpare_fixtures as F
import seqpare_ref as SR
from helpers import ROOT, Oracle, short_tmpdir
from test_seqpare_ref import check_conditions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def made():
    """name -> fixture with its literal reference, the oracle's doubles and an open Database; each built once"""
    from igd_amd import Database
    d = short_tmpdir("sqg")
    cache = {}

    def get(name):
        if name not in cache:
            fx = F.BUILDERS[name](d)
            orc = Oracle(fx["igd"])
            fx.update(ref=SR.seqpare(orc, fx["q"]), want=orc.seqpare_file(fx["q"]), nr=orc.file_nr(), db=Database(fx["igd"]))
            orc.close()
            for a in (fx["ref"].sums, fx["ref"].sm, fx["want"]):
                a.setflags(write=False)
            assert np.array_equal(SR.bits(fx["ref"].sm), SR.bits(fx["want"])), name
            check_conditions(name, fx, fx["ref"])
            cache[name] = fx
        return cache[name]

    yield get
    for fx in cache.values():
        fx["db"].close()
    shutil.rmtree(d, ignore_errors=True)


def check(fx):
    """the engine's sums are the literal reference's, and its similarities the oracle's, word for word"""
    db, ref = fx["db"], fx["ref"]
    assert db.gtype == 1 and db.nfiles == len(ref.sums)
    got = db.seqpare(*ref.args)
    assert np.array_equal(SR.bits(got), SR.bits(ref.sums)), (got, ref.sums)
    sm = db.seqpare(*ref.args, n_queries_total=ref.nq, nr=fx["nr"])
    assert np.array_equal(SR.bits(sm), SR.bits(fx["want"])), (sm, fx["want"])


@pytest.mark.parametrize("name", ["edges_mixed", "edges_identical"])
def test_group_sizes_at_the_batch_the_lds_capacity_and_the_table_size(made, name):
    fx = made(name)
    assert {d.size for d in fx["ref"].diag.values()} == {1, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2048, 2049}
    check(fx)


def test_chains_inside_a_batch(made):
    fx = made("chains")
    assert any(d.knocked_in_batch > 0 and d.survived_chain > 0 and d.rejected_by_earlier_batch > 0 for d in fx["ref"].diag.values())
    check(fx)


def test_near_ties_in_float32(made):
    """tests/test_seqpare_ref.py asserts on this fixture that similarities lie one or two float32 steps apart and that pairs tie
    in float32 whose exact quotients differ."""
    check(made("near_ties"))


@pytest.mark.parametrize("name", ["few_1x1", "few_2x1", "few_257x1", "few_1x257"])
def test_few_groups(made, name):
    fx = made(name)
    assert fx["ref"].args[4] * fx["db"].nfiles == {"few_1x1": 1, "few_2x1": 2}.get(name, 257)
    check(fx)


def test_awkward_queries(made):
    fx = made("awkward")
    ichr, qs, qe, grp, ng = fx["ref"].args
    nbp = 4096
    assert ng == 3 and (qs == qe).any() and ((qe - 1) // nbp - qs // nbp >= 3).any() and fx["ref"].nq > len(qs)
    assert len(set(zip(ichr.tolist(), qs.tolist(), qe.tolist()))) < len(qs)
    check(fx)


# ---- a wave's second and third group ------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
from igd_amd import Database
a = np.load(sys.argv[3])
db = Database(sys.argv[2])
np.save(sys.argv[4], db.seqpare(a["ichr"], a["qs"], a["qe"], a["grp"], int(a["ng"])))
db.close()
print("compute units", torch.cuda.get_device_properties(0).multi_processor_count)
"""


def test_waves_take_a_second_and_a_third_group(made):
    """One workgroup per compute unit (IGD_HIP_WG_PER_CU=1, read at open): k_seq_greedy runs min(nG, 3 x compute units) waves
    over 1 120 groups.  The first 800 groups, one per wave and then some, all keep their hash sets in HBM; the 320 behind them
    cycle through empty, below 64, 65 .. 1 024 and above 1 024, so what a wave takes after its first group is an LDS group behind
    an HBM group, and a wave that takes an empty group goes on to a full one."""
    fx = made("waves")
    ref = fx["ref"]
    assert 'getenv("IGD_HIP_WG_PER_CU")' in open(os.path.join(ROOT, "igd_amd", "csrc", "engine", "host_open.hpp")).read()
    d = os.path.dirname(fx["igd"])
    inp, out = os.path.join(d, "wv_in.npz"), os.path.join(d, "wv_out.npy")
    ichr, qs, qe, grp, ng = ref.args
    np.savez(inp, ichr=ichr, qs=qs, qe=qe, grp=grp, ng=ng)
    env = dict(os.environ, IGD_HIP_WG_PER_CU="1")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, fx["igd"], inp, out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    cus = int(p.stdout.decode().split("compute units")[1])
    n_groups = ng * fx["db"].nfiles
    seq = F.waves_classes(ref)
    print("compute units", cus, "groups", n_groups)
    assert n_groups == len(seq) > 3 * cus
    assert set(seq[:3 * cus]) == {3} and all(seq[3 * cus:].count(k) >= 40 for k in range(4))
    got = np.load(out)
    assert np.array_equal(SR.bits(got), SR.bits(ref.sums)), (got, ref.sums)
    check(fx)                                            # and with the default grid


# ---- definedness and carry ----------------------------------------------------------------------------------------------------
def garbage(n):
    g = np.empty(max(n, 1), np.float64)
    g[0::2] = np.nan
    g[1::2] = -1.2345e300
    return g


def call(db, entry, args, sums):
    ichr, qs, qe, grp, ng = args
    a = [np.ascontiguousarray(x, dtype=np.int32) for x in (ichr, qs, qe, grp)]
    rc = getattr(db._H, entry)(db.dev, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, len(a[0]), a[3].ctypes.data, int(ng),
                               sums.ctypes.data)
    assert rc == 0, (entry, rc)


def cut(args, g0, g1):
    """the queries of contig groups g0 .. g1 - 1 as a call of their own: group numbers start at 0"""
    ichr, qs, qe, grp, _ = args
    k = (grp >= g0) & (grp < g1)
    return ichr[k], qs[k], qe[k], grp[k] - g0, g1 - g0


@pytest.mark.parametrize("name", ["edges_mixed", "awkward", "few_1x257"])
def test_every_word_is_defined_and_ranges_carry(made, name):
    fx = made(name)
    db, ref = fx["db"], fx["ref"]
    nf, ng = db.nfiles, ref.args[4]
    want = SR.bits(ref.sums)
    sums = garbage(nf)
    call(db, "igd_hip_seqpare", ref.args, sums)
    assert np.array_equal(SR.bits(sums[:nf]), want)
    # no query at all; queries that overlap nothing (E == 0): zeros, whatever was there
    none = (np.zeros(0, np.int32),) * 4
    far = (ref.args[0][:3], np.full(3, 2 ** 30, np.int32), np.full(3, 2 ** 30 + 50, np.int32), np.zeros(3, np.int32), 1)
    for args in (none + (0,), none + (ng,), far):
        sums = garbage(nf)
        call(db, "igd_hip_seqpare", args, sums)
        assert not SR.bits(sums[:nf]).any(), args
    # contig ranges through igd_hip_seqpare_add, as the command line passes a file beyond one batch
    if name == "edges_mixed":
        e = fx["empty_group"]
        ranges = [(0, 3), (3, e), None, (e, e + 1), "far", (e + 1, ng)]       # None: nq = 0; (e, e + 1) and "far": no overlap
    elif name == "awkward":
        ranges = [(0, 1), None, (1, 2), "far", (2, 3)]
    else:
        ranges, g = [], 0
        while g < ng:
            step = min(1 + len(ranges) % 7 * 4, ng - g)
            ranges += [(g, g + step), None if len(ranges) % 4 == 0 else "far"]
            g += step
        assert len(ranges) > 16
    sums = np.zeros(nf, np.float64)
    for r in ranges:
        before = SR.bits(sums).copy()
        call(db, "igd_hip_seqpare_add", none + (0,) if r is None else far if r == "far" else cut(ref.args, *r), sums)
        if r is None or r == "far" or (name == "edges_mixed" and r == (fx["empty_group"], fx["empty_group"] + 1)):
            assert np.array_equal(SR.bits(sums), before), r
    assert np.array_equal(SR.bits(sums), want)
