"""The constructed merge-join cases (tests/mergejoin_cases.py) are what they claim to be -- checked on the CPU, before any
device run: every claimed property (records and first-tile queries per tile, later candidates per tile, later-block boundaries
crossed at blocks of 2^8 and 2^10 queries, tiles per query) is recomputed from the arrays, and every batch is run through the
CPU oracle: it finds something, and where every query is ordinary and starts in a tile with records (no rule-NEST quirk) the
oracle's counts are those of a literal count over all (query, record) pairs, with and without the value filter."""
import shutil

import numpy as np
import pytest

import mergejoin_cases as mj
from helpers import Oracle, short_tmpdir

CASES = {c.name: c for c in mj.host_cases()}


@pytest.fixture(scope="module")
def workdir():
    d = short_tmpdir("imj")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def test_every_route_of_the_issue_has_its_cases():
    K = mj.DEFAULTS
    want = {"unit_edges", "second_round", "spans+0", "spans+1", "spans+2", "later%d" % K["later_max"], "later%d" % (K["later_max"] + 1),
            "seam_inside_8", "seam_ends_on_8", "seam_one_8", "seam_two_8", "seam_one_10", "seam_two_10",
            "far_wide%d" % (K["far_wide"] - 1), "far_wide%d" % K["far_wide"], "far_wide%d" % (K["heavy_first"] // 256 + 1), "rank_exceptions", "coords16_512", "coords16_32768",
            "dense%d_swapped" % (K["lean_first"] + 1)}
    want |= {"dense%d" % n for n in (31, 32, 33, 512, 513, K["sbcap"] - 1, K["sbcap"], K["sbcap"] + 1, 8192, 8193, 8192 + 511, 8192 + 513)}
    assert set(CASES) == want


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_case_is_what_it_claims(name):
    case, K = CASES[name], mj.DEFAULTS
    p = mj.properties(case, K)
    assert p["sorted"] or name.endswith("_swapped")
    if not name.endswith("_swapped"):                         # ordered by (contig, start) inside every key as well
        same = np.diff(p["key"]) == 0
        assert np.all(np.diff(case.qs.astype(np.int64))[same] >= 0)
    for prop, claim in case.claims.items():
        if prop == "n_units_over":
            assert int(np.maximum(p["units"], 1).sum()) > claim              # (an empty tile has a unit of its own)
        elif prop == "max_tiles":
            assert int(p["tiles"].max()) == claim
        elif prop == "n_long":
            assert int(p["long"].sum()) == claim
        elif prop == "n_covered":
            assert int(p["covered"].sum()) == claim
        elif prop == "n_walk_first":
            assert int(p["walk_first"].sum()) == claim
        elif prop == "n_invalid":
            assert int((~p["valid"]).sum()) == claim
        elif prop == "min_queries":
            assert len(case.qs) >= claim and len(case.qs) <= claim + 70000
        else:
            for tile, value in claim.items():
                assert p[prop][tile] == value, (prop, tile, int(p[prop][tile]), value)
    assert len(case.qs) <= 20000 or case.claims.get("min_queries", 0) >= 65536, "only the 2^10-query later blocks need more"


def test_the_thresholds_sit_between_neighbouring_cases():
    """what flips between a case and its neighbour, as predict() reads it off the properties"""
    K = mj.DEFAULTS
    P = lambda name, full, sh=8: mj.predict(CASES[name], K, full, sh)
    assert P("later64", False)["nfar"] == 0 and P("later65", False)["nfar"] == 1 and P("later65", True)["nfar"] == 0
    assert P("spans+0", True)["nfix"] == 0 and P("spans+1", True)["nfix"] == 5 and P("spans+2", True)["nfix"] == 5
    assert [P("spans+%d" % k, True)["cov_sorted"] for k in (0, 1, 2)] == [0, 0, 1]
    assert [P("seam_%s_8" % k, False)["nfar"] for k in ("inside", "ends_on", "one", "two")] == [0, 0, 0, 1]
    assert P("seam_one_10", False, 10)["nfar"] == 0 and P("seam_two_10", False, 10)["nfar"] == 1
    assert P("dense512", False)["nheavys"] == 0 and P("dense513", False)["nheavys"] == 1 and P("dense513", True)["nheavys"] == 0
    assert P("dense8192", True)["nheavys"] == 0 and P("dense8193", True)["nheavys"] == 1
    assert P("far_wide7", True)["nfar"] == 0 and P("far_wide8", True)["nfar"] == 1 and P("far_wide7", False)["nfar"] == 1
    assert [(P("far_wide33", f)["nfar"], P("far_wide33", f)["nheavys"]) for f in (False, True)] == [(1, 1), (1, 1)]
    assert P("rank_exceptions", True)["nfix"] == 4 and P("unit_edges", False)["nfix"] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_oracle_finds_something_and_agrees_with_all_pairs(name, workdir):
    case = CASES[name]
    p = mj.properties(case)
    ordinary = bool(np.all(p["valid"] & (case.qs >= 0) & (case.qs < case.qe) & (p["rec"][np.clip(p["n1"], 0, case.ntile - 1)] > 0)))
    assert ordinary == case.literal
    orc = Oracle(case.write("%s/%s.igd" % (workdir, name.replace("+", "p"))))
    try:
        assert orc.nfiles == mj.NF and orc.nctg == 1 and orc.nbp == case.nbp
        for v in (0, mj.VCUT):
            hits, total = orc.search(case.ichr, case.qs, case.qe, v)
            assert total > 0 and total == hits.sum()
            if v:
                assert total < orc.search(case.ichr, case.qs, case.qe, 0)[1]       # the filter removes some records, not all
            if case.literal:
                np.testing.assert_array_equal(hits, mj.literal_hits(case, v))
    finally:
        orc.close()
