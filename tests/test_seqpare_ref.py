"""The literal Seqpare reference of the tests (tests/seqpare_ref.py) against the CPU oracle's orc_seqOverlaps (pinned to the real
reference by tests/test_oracle_seqpare.py): the doubles are equal bit for bit on every fixture of
tests/test_gpu_seqpare_scale.py and on tests/golden/create, and the fixtures' conditions -- group sizes at the kernel's edges,
the three chain counters, near-ties in float32 -- hold on the reference's own diagnostics.  No GPU."""
import os
import shutil

import numpy as np
import pytest

import seqpare_fixtures as F
import seqpare_ref as SR
from helpers import GOLDEN, Oracle, short_tmpdir


@pytest.fixture(scope="module")
def tmp():
    d = short_tmpdir("sqr")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def solve(igd, q):
    orc = Oracle(igd)
    try:
        return SR.seqpare(orc, q), orc.seqpare_file(q)
    finally:
        orc.close()


@pytest.mark.parametrize("name", sorted(F.BUILDERS))
def test_literal_reference_equals_the_oracle_bit_for_bit(tmp, name):
    fx = F.BUILDERS[name](tmp)
    ref, want = solve(fx["igd"], fx["q"])
    assert np.array_equal(SR.bits(ref.sm), SR.bits(want)), name
    assert (ref.sums > 0).any() and np.isfinite(want).all()
    check_conditions(name, fx, ref)


def test_literal_reference_equals_the_oracle_on_the_golden_database():
    g = os.path.join(GOLDEN, "create")
    ref, want = solve(g + "/ref.igd", g + "/q.bed")
    assert np.array_equal(SR.bits(ref.sm), SR.bits(want))
    text = open(g + "/search_s.txt").read().splitlines()[1:]
    assert ["%10.6f" % x for x in ref.sm] == [l.split("\t")[2] for l in text]


def check_conditions(name, fx, ref):
    """What keeps a fixture from going vacuous, asserted on the reference's diagnostics (shared with the GPU tests)."""
    sizes = sorted(d.size for d in ref.diag.values())
    if name.startswith("edges"):
        assert sizes == sorted(F.EDGE_SIZES), sizes
        assert {1, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2048, 2049} == set(sizes)
        assert all(g != fx["empty_group"] for g, _ in ref.diag) and ref.args[4] == 12
        for (g, m), d in ref.diag.items():
            j, k = F.EDGE_SHAPES[m]
            assert d.accepted == min(j, k), (g, m, d)            # every pair overlaps: a full matching of the smaller side
    elif name == "chains":
        assert len(ref.diag) == 4 and all(d.size == 144 for d in ref.diag.values())
        assert any(d.knocked_in_batch > 0 and d.survived_chain > 0 and d.rejected_by_earlier_batch > 0
                   for d in ref.diag.values()), ref.diag
    elif name == "waves":
        assert ref.args[4] == F.WAVES_CONTIGS
        seq = F.waves_classes(ref)
        lead = F.WAVES_LEAD * F.WAVES_FILES
        assert None not in seq and set(seq[:lead]) == {3} and lead >= 3 * 256      # 256 compute units: every wave's first group
        tail = seq[lead:]
        assert all(tail.count(k) == len(tail) // 4 for k in range(4)) and all(a != b for a, b in zip(tail, tail[1:]))
        assert tail[-1] != 0                                                        # whoever takes an empty group finds another
    elif name.startswith("few"):
        nfiles, nctg = (int(x) for x in name[4:].split("x"))
        assert ref.args[4] == nctg and len(ref.sums) == nfiles
        ng = nfiles * nctg
        assert len(ref.diag) == ng if ng <= 2 else ng // 2 < len(ref.diag) < ng       # 257 groups: some of them empty


def test_near_ties_differ_in_the_last_bits_or_only_in_double(tmp):
    """Per dataset of the near-tie fixture: similarities one or two float32 steps apart, and fewer distinct float32 values
    than distinct exact quotients -- pairs that tie in float32 and would not in double."""
    fx = F.near_ties(tmp)
    orc = Oracle(fx["igd"])
    contigs, _ = SR.read_query_file(orc, fx["q"])
    close = 0
    for m, (name, ivs) in enumerate(contigs):
        rows, cols, vals = SR.contig_groups(orc, name, ivs)[m]
        assert len(vals) == 120 and (vals > 0).all()
        b = np.unique(vals.view(np.int32))
        assert len(b) < len(fx["exact"][m]), (m, len(b), len(fx["exact"][m]))
        close += int((np.diff(b) <= 2).sum())
    orc.close()
    assert close >= 10, close


def test_walk_counts_a_hand_made_chain():
    """Three candidates in one run: A (row 0, column 0), B (row 0, column 1) knocked out by A, C (row 1, column 1) accepted
    although it shares its column with B.  With runs of one candidate, B is rejected by an EARLIER run instead."""
    rows, cols = np.array([0, 0, 1]), np.array([0, 1, 1])
    vals = np.array([0.9, 0.8, 0.7], np.float32)
    acc, d = SR.walk(rows, cols, vals)
    assert acc == [0, 2] == SR.greedy(rows, cols, vals)
    assert d == SR.Diag(3, 2, 1, 1, 0)
    acc, d = SR.walk(rows, cols, vals, run=1)
    assert acc == [0, 2] and d == SR.Diag(3, 2, 0, 0, 1)
    # equal scores: scan order decides; a zero is never taken
    vals = np.array([0.5, 0.5, 0.0], np.float32)
    assert SR.greedy(rows, cols, vals) == [0] == SR.walk(rows, cols, vals)[0]
