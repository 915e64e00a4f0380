"""GPU: igd_bits_support (Database.enrichment_restricted) past one item per workgroup, one block per row and two busy waves;
igd_restrict_bits and igd_member_popc over more than 2 000 rows.

tests/test_gpu_restrict.py holds every output against the brute force, but its universes have at most 75 words per bit row
and its calls at most 5 rows: every launch of the gather has one block per row (nblk == 1), fewer items than workgroups, and
nothing in waves 2 and 3.  A work item is (row k, block of IGD_RESTRICT_BLOCK_WORDS words); IGD_SETS_GRID persistent
workgroups stride over the items, row-major, and flush and clear their LDS counters and lhit[0] after each.  The cases:

    a  IGD_SETS_GRID + 300 sets over a universe of one block: workgroups 0 .. 300 take a second item, the last of them the
       ones row (usupport, unhit) behind set 300.  The join bisects more than 2 000 rows
    b  a universe of three blocks (20 011 regions, the last word inside wave 1 of block 2) and 900 sets: 2 703 items, 655
       second items, each in another row and another block than the workgroup's first; every wave of every block is reached
       by a second item; full words
    c  child processes.  Membership chunks of 9 001 universe regions: u0 = 9 001 and 18 002 lie inside a word, a chunk has
       282 words = 2 blocks counted from w0, the low and the high mask fall in different blocks.  IGD_HIP_MAX_BATCH = 4 096
       with the sets of case a: batches cut sets, hoff[] is clamped over more than 2 000 rows
    d  the wide form (IGD_RESTRICT_LDS_FILES + 1 files) with two blocks

Every expectation is restrict_ref.join and restrict_ref.gather_rows over the CPU oracle's membership of the universe
(test_membership_host); tests/test_restrict_host.py holds the fixtures of a and b, their conditions and the agreement of
gather_rows with gather on a machine without a GPU.  The conditions that keep a case from being vacuous are asserted on that
expectation before the device is asked (restrict_ref.second_item_conditions, block_conditions, seam_conditions).

Not reachable: a workgroup whose two items lie in the same row.  Its items are gridDim = min(items, IGD_SETS_GRID) apart and
a row has nblk <= items of them, so they share a row only if the launch has a single row, and then every workgroup has one
item.  Case b asserts what does hold: all 655 second items lie in another row and in another block."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import restrict_ref as RR
import sets_fixtures as F
from helpers import ROOT, Oracle, short_tmpdir
from test_enrich_host import enrich_fixture
from test_gpu_restrict import CHILD, MODES, NFILES, check_equivalence, check_restricted
from test_membership_host import oracle_member, oracle_member_enum
from test_restrict_host import SEAM_SETS, SPAN, scale_consts, scale_fixture_a

pytestmark = pytest.mark.gpu
K = scale_consts()
V = {"nest": 0, "v400": 400}


@pytest.fixture(scope="module")
def fx():
    """the 40-file database of tests/test_gpu_restrict.py; the fixtures of cases a and b with their joins, built once"""
    from igd_amd import Database
    d = short_tmpdir("igz")
    path, upath, _, _ = enrich_fixture(d, nfiles=NFILES, name="gz")
    orc, db = Oracle(path), Database(path)
    assert db.gtype == 1 and db.nfiles == NFILES
    yield dict(d=d, path=path, db=db, orc=orc, uni=orc.read_queries(upath), made={})
    db.close()
    orc.close()
    shutil.rmtree(d, ignore_errors=True)


def case_a(fx):
    if "a" not in fx["made"]:
        a = scale_fixture_a(fx["orc"], fx["uni"])
        a["R"] = RR.join(*a["cat"], a["off"], *a["uni"])
        fx["made"]["a"] = a
    return fx["made"]["a"]


def case_b(fx):
    """(fixture with its join R, the oracle's membership of its universe)"""
    if "b" not in fx["made"]:
        b = RR.scale_b(SPAN, K["block_words"])
        b["R"] = RR.join(*b["cat"], b["off"], *b["uni"])
        b["member"] = oracle_member_enum(fx["orc"], *b["uni"])
        fx["made"]["b"] = b
    return fx["made"]["b"]


def rows_of(res, idx):
    """the RestrictedEnrichment of the sets `idx` alone"""
    return type(res)(**{n: (getattr(res, n) if n == "usupport" else getattr(res, n)[idx]) for n in res._fields})


# ---- a ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["nest", "v400"])
def test_a_second_items_one_block(fx, mode):
    """2 348 sets and the ones row are 2 349 items of one block against 2 048 workgroups: workgroup w <= 300 computes set
    2 048 + w (the ones row for w = 300) with the counters and lhit[0] that set w left.  Every set from 2 048 on with
    support has a zero in a file where its workgroup's first set has none, 88 of them are empty behind a set with support
    or behind an empty one, and set bits fall on universe regions without a hit."""
    db, a = fx["db"], case_a(fx)
    cat, off, uni, R = a["cat"], a["off"], a["uni"], a["R"]
    nu = len(uni[1])
    assert len(off) - 1 == K["grid"] + 300 and (nu + 31) // 32 <= K["block_words"]
    member, _ = oracle_member(fx["orc"], *uni, V[mode])
    sup, usup, _, _ = RR.gather_rows(R, member)
    print(mode, RR.second_item_conditions(R, member, sup, usup, K["grid"], mode))
    res, nhit, unhit = db.enrichment_restricted(*cat, off, *uni, with_nhit=True, **MODES[mode])
    check_restricted(db, res, nhit, unhit, R, member, nu, mode, gather=RR.gather_rows)
    bits, size = db.restrict_sets(*cat, off, *uni)
    assert np.array_equal(bits, RR.pack(R)) and np.array_equal(size, R.sum(axis=1)), mode


# ---- b ----------------------------------------------------------------------------------------------------------------------
def test_b_three_blocks_four_waves(fx):
    """901 rows of 3 blocks: 2 703 items, 655 of them second items.  check_equivalence on the first 20 sets, the last 20 and
    20 around set IGD_SETS_GRID / 3, where the second items begin."""
    db, b = fx["db"], case_b(fx)
    cat, off, uni, R, member = b["cat"], b["off"], b["uni"], b["R"], b["member"]
    nu = len(uni[1])
    print(RR.block_conditions(R, member, K["grid"], K["block_words"], K["wg"] // K["wave"], "b"))
    res, nhit, unhit = db.enrichment_restricted(*cat, off, *uni, with_nhit=True, **MODES["nest"])
    check_restricted(db, res, nhit, unhit, R, member, nu, "b", gather=RR.gather_rows)
    nsets, mid = len(off) - 1, K["grid"] // 3
    idx = np.r_[0:20, mid - 10:mid + 10, nsets - 20:nsets]
    assert len(set(idx.tolist())) == 60 and res.support[idx].any(axis=1).sum() > 40
    check_equivalence(db, rows_of(res, idx), R[idx], uni, "b", **MODES["nest"])


# ---- c ----------------------------------------------------------------------------------------------------------------------
def run_child(script, args, env):
    e = dict(os.environ)
    e.update(env)
    got = subprocess.run([sys.executable, "-c", script, ROOT] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert got.returncode == 0, got.stderr.decode()


def test_c_membership_chunks_cut_inside_a_word(fx):
    """IGD_HIP_MEMBER_ROW_BYTES = 8 x 9 001 with rows of 2 words: chunks [0, 9 001), [9 001, 18 002), [18 002, 20 011).  The
    middle one begins at bit 9 of word 281 and ends at bit 18 of word 562: 282 words, two blocks counted from word 281, the
    low mask in the first and the high mask in the second.  Five sets and the ones row: 6 rows x 2 blocks in the child's
    middle chunk and 6 x 3 in the parent's call.  That 6 has a common factor with both block counts is what lets this test
    see an item map of the kind (it % rows, it % nblk): with coprime counts (case b: 901 x 3, case d: 5 x 2) such a map only
    permutes the items and every sum stays what it was."""
    db, b = fx["db"], case_b(fx)
    uni, member = b["uni"], b["member"]
    nu, step = len(uni[1]), 9001
    assert (NFILES + 31) // 32 == 2
    cat, off = RR.sets_of([b["lists"][k] for k in SEAM_SETS])
    R = b["R"][list(SEAM_SETS)]
    print(RR.seam_conditions(R, member, step, K["block_words"], "c"))
    want, wnhit, wunhit = db.enrichment_restricted(*cat, off, *uni, with_nhit=True)
    check_restricted(db, want, wnhit, wunhit, R, member, nu, "parent", gather=RR.gather_rows)
    inp, out = os.path.join(fx["d"], "c_in.npz"), os.path.join(fx["d"], "c_out.npz")
    np.savez(inp, ichr=cat[0], qs=cat[1], qe=cat[2], off=off, uc=uni[0], us=uni[1], ue=uni[2])
    run_child(CHILD, [fx["path"], inp, out], dict(IGD_HIP_MEMBER_ROW_BYTES=str(8 * step)))
    z = np.load(out)
    got = type(want)(**{n: z[n] for n in want._fields})
    check_restricted(db, got, z["nhit"], int(z["unhit"]), R, member, nu, "child", gather=RR.gather_rows)
    for name in want._fields:
        assert np.array_equal(z[name], getattr(want, name), equal_nan=True), name
    assert np.array_equal(z["bits2"], want.bits) and np.array_equal(z["size2"], want.size)


CHILD_JOIN = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from igd_amd import Database
z = np.load(sys.argv[3])
db = Database(sys.argv[2])
bits, size = db.restrict_sets(z["ichr"], z["qs"], z["qe"], z["off"], z["uc"], z["us"], z["ue"])
np.savez(sys.argv[4], bits=bits, size=size)
db.close()
"""


def test_c_batches_cut_sets_over_many_rows(fx):
    """IGD_HIP_MAX_BATCH = 4 096 and the sets of case a: 33 000 regions reach the join in 9 batches whose ends fall inside
    sets, each with hoff[] clamped to the batch over 2 349 entries; rows before and behind the batch are empty ranges."""
    db, a = fx["db"], case_a(fx)
    cat, off, uni, R = a["cat"], a["off"], a["uni"], a["R"]
    step = 4096
    cuts = np.arange(step, int(off[-1]), step)
    inside = [int(c) for c in cuts if not (off == c).any()]
    print("regions", int(off[-1]), "batch ends", len(cuts), "inside a set", len(inside))
    assert len(off) - 1 > 2000 and len(cuts) >= 7 and len(inside) >= 5
    both = 0                                             # cut sets whose bits come from either side of the cut
    for c in inside:
        k = int(np.searchsorted(off, c, "right")) - 1
        a, e = int(off[k]), int(off[k + 1])
        part = RR.join(cat[0][a:e], cat[1][a:e], cat[2][a:e], np.array([0, c - a, e - a], np.int64), *uni)
        both += bool(part[0].any() and part[1].any() and (part[0] != part[1]).any())
    assert both >= 4, "only %d batch ends cut a set with universe regions on either side" % both
    bits, size = db.restrict_sets(*cat, off, *uni)
    assert np.array_equal(bits, RR.pack(R)) and np.array_equal(size, R.sum(axis=1))
    inp, out = os.path.join(fx["d"], "j_in.npz"), os.path.join(fx["d"], "j_out.npz")
    np.savez(inp, ichr=cat[0], qs=cat[1], qe=cat[2], off=off, uc=uni[0], us=uni[1], ue=uni[2])
    run_child(CHILD_JOIN, [fx["path"], inp, out], dict(IGD_HIP_MAX_BATCH=str(step)))
    z = np.load(out)
    assert np.array_equal(z["bits"], bits) and np.array_equal(z["size"], size)


# ---- d ----------------------------------------------------------------------------------------------------------------------
def test_d_wide_form_with_two_blocks():
    """IGD_RESTRICT_LDS_FILES + 1 files and a universe of one block + 70 regions: 5 rows of 2 blocks, every set bit adds
    straight into support[k][f].  Set 0 holds 130 universe regions, the last ten among them; set 1 the window of the boundary
    files; set 2 a third of the contig; set 3 is empty."""
    from igd_amd import Database
    nfiles = K["lds_files"] + 1
    assert nfiles == 8193
    d = short_tmpdir("igw")
    try:
        path, span, window, edge = F.wide_db(random.Random(8100 + nfiles), d, "s%d" % nfiles, nfiles, F.NBP, max(40, nfiles * 3 // 10))
        nu = K["block_words"] * 32 + 70
        uni, _ = F.make_sets(np.random.default_rng(nfiles), 1, F.NBP, span, [nu], window)
        rs = np.random.default_rng(nfiles + 1)
        pick = np.concatenate([rs.permutation(nu - 10)[:120], np.arange(nu - 10, nu)])
        lists = [[(int(uni[0][i]), int(uni[1][i]), int(uni[2][i])) for i in pick],
                 [(0, window[0], window[1])], [(0, 0, span // 3), (0, span // 2, span // 2 + 5 * F.NBP)], []]
        cat, off = RR.sets_of(lists)
        R = RR.join(*cat, off, *uni)
        orc = Oracle(path)
        try:
            member = oracle_member_enum(orc, *uni)
        finally:
            orc.close()
        live = R & member.any(axis=1)[None, :]
        per = K["block_words"] // 4 * 32
        reach = [int(live[:, w * per:(w + 1) * per].sum()) for w in range(4)] + [int(live[:, 4 * per:].sum())]
        print("set bits with a hit in waves 0-3 of block 0 and in block 1:", reach, "sizes", R.sum(axis=1).tolist())
        assert min(reach) > 0 and live[0, 4 * per:].any() and live[2, 4 * per:].any()
        assert member[:, edge].any(axis=0).all() and R[:3].any(axis=1).all() and not R[3].any() and (uni[0] < 0).any()
        db = Database(path)
        try:
            res, nhit, unhit = db.enrichment_restricted(*cat, off, *uni, with_nhit=True)
            check_restricted(db, res, nhit, unhit, R, member, nu, nfiles, gather=RR.gather_rows)
            assert res.support[:, edge].any(axis=0).all(), "a boundary file has no support in any set"
        finally:
            db.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
