"""The merge join's rare routes, each reached on purpose and PROVED taken: the constructed cases of tests/mergejoin_cases.py
(checked on the CPU by tests/test_mergejoin_cases_host.py) run on the lean and on the full build of igd_scan_sorted
(IGD_HIP_RANK), with the order promised (flags = 1) and left to the device (flags = 0), without and with a value threshold that
removes every second record.  Every batch must equal the CPU oracle integer for integer, and the route words of the batch
(Database.last_batch_routes: the control words the kernels count their lists in) must be what the construction predicts --
positive for the case on the route, zero for its neighbour just below the threshold.

The shapes follow the engine's own constants (Database.route_constants), so a constant that moves takes its cases along.

Later blocks: a batch below 2^16 queries always takes one query per thread and blocks of 2^8 queries, aligned or not; from
2^16 queries on, 16-byte aligned arrays give blocks of 2^10 and arrays that are not give 2^8 (host_search.hpp).  Blocks of 2^12
need 2^22 queries and stay with tests/test_gpu_stress.py."""
import os
import shutil

import numpy as np
import pytest

import mergejoin_cases as mj
from helpers import Oracle, short_tmpdir

pytestmark = pytest.mark.gpu
FLAG_SORTED = 1
BUILDS = ("lean", "full")


class Ctx:
    """what the module's tests share: the directory of the databases, the engine's constants, the cases built from them, the
    oracle's counts and the engine's results per (case, build) -- each computed once, on first use, and not written to again"""

    def __init__(self, workdir):
        self.dir, self._ref, self._run = workdir, {}, {}
        first = mj.unit_edges()
        first.name = "constants"                          # (a file of its own: the cases proper are built from what it reports)
        db = self.open_db(first, "full")
        try:
            self.K = db.route_constants()
        finally:
            db.close()
        self.cases = {c.name: c for c in mj.host_cases(self.K)}

    def path_of(self, case):
        path = "%s/%s.igd" % (self.dir, case.name.replace("+", "p"))
        return path if os.path.exists(path) else case.write(path)

    def open_db(self, case, build):
        from igd_amd import Database
        with pytest.MonkeyPatch.context() as mp:          # the engine reads these when a database is opened
            mp.setenv("IGD_HIP_RANK", "0" if build == "lean" else "1")
            if case.nbp not in (1 << 14, 1 << 15):
                mp.setenv("IGD_HIP_NO_RETILE", "1")       # tiles of another width are searched as they are, not on a 2^14 bp copy
            return Database(self.path_of(case))

    def dense_sizes(self):
        K = self.K
        return K["dense_min"], K["lean_first"], K["heavy_first"], K["heavy_slice"], K["sbcap"]

    def reference(self, name):
        """the oracle's (hits, total) without and with the value threshold"""
        if name not in self._ref:
            case = self.cases[name]
            orc = Oracle(self.path_of(case))
            try:
                out = {v: orc.search(case.ichr, case.qs, case.qe, v) for v in (0, mj.VCUT)}
            finally:
                orc.close()
            for h, _ in out.values():
                h.setflags(write=False)
            self._ref[name] = out
        return self._ref[name]

    def run(self, name, build):
        """the case on one build: {(flags, v): (hits, total, route words)}"""
        if (name, build) not in self._run:
            case = self.cases[name]
            db = self.open_db(case, build)
            try:
                assert db.last_batch_routes() == {}      # no batch yet
                out = {}
                for flags in (FLAG_SORTED, 0):
                    for v in (0, mj.VCUT):
                        hits, total = db.search(case.ichr, case.qs, case.qe, v, flags=flags)
                        out[(flags, v)] = (hits, total, db.last_batch_routes())
            finally:
                db.close()
            self._run[(name, build)] = out
        return self._run[(name, build)]

    def check(self, name, build, sh=None):
        """every batch of the case equals the oracle and has the predicted route words; returns the prediction"""
        case = self.cases[name]
        sh = (10 if len(case.qs) >= 65536 else 8) if sh is None else sh
        want = mj.predict(case, self.K, build == "full", sh)
        for (flags, v), (hits, total, routes) in self.run(name, build).items():
            print(name, build, "flags", flags, "v", v, routes)
            ref_hits, ref_total = self.reference(name)[v]
            assert total == ref_total, (name, build, flags, v)
            np.testing.assert_array_equal(hits, ref_hits, err_msg="%s %s flags %d v %d" % (name, build, flags, v))
            assert {w: routes[w] for w in want} == want, (name, build, flags, v)
            assert routes["nlong"] == 0 and routes["nheavy"] == 0 and routes["cov_bucket"] == 0      # nothing of the bucket path
        return want


@pytest.fixture(scope="module")
def ctx():
    d = short_tmpdir("imr")
    yield Ctx(d)
    shutil.rmtree(d, ignore_errors=True)


def test_the_host_defaults_are_the_engines_constants(ctx):
    """tests/test_mergejoin_cases_host.py validated the cases at these values (sbcap and lean_waves belong to the handle)"""
    K = ctx.K
    assert {k: K[k] for k in mj.DEFAULTS if k not in ("sbcap", "lean_waves")} == {k: v for k, v in mj.DEFAULTS.items() if k not in ("sbcap", "lean_waves")}
    assert K["sbcap"] >= 64 and K["sbcap"] & (K["sbcap"] - 1) == 0 and K["lean_waves"] > 0


@pytest.mark.parametrize("build", BUILDS)
def test_unit_edges(build, ctx):
    """tiles of 1 .. 2U + 1 records, queries on the first and last record of every slot and unit; nothing is listed"""
    want = ctx.check("unit_edges", build)
    assert (want["nfix"], want["nheavys"], want["nfar"], want["cov_sorted"]) == (0, 0, 0, 0)


@pytest.mark.parametrize("build", BUILDS)
def test_a_wave_with_more_units_than_one_round(build, ctx):
    """more units than ROUND x the lean build's waves.  No route word tells that a wave took a second round: the shape is
    asserted from the constants, and exactness (records and queries in the last tiles, which only a second round reads on
    the lean build) is the only check on the device"""
    case, K = ctx.cases["second_round"], ctx.K
    assert case.ntile > K["round"] * K["lean_waves"]     # one unit per tile at least
    ctx.check("second_round", build)


@pytest.mark.parametrize("build", BUILDS)
def test_later_tiles_and_long_queries(build, ctx):
    """2, 3, 4 tiles (k = 1 .. 3) and exactly short_tiles: nothing walked, nothing covered; one tile more: WALK_LAST alone
    (no tile lies between); two more: WALK_LAST and coverage"""
    w0, w1, w2 = (ctx.check("spans+%d" % k, build) for k in (0, 1, 2))
    assert (w0["nfix"], w0["cov_sorted"]) == (0, 0)
    assert (w1["nfix"], w1["cov_sorted"]) == (5, 0)
    assert (w2["nfix"], w2["cov_sorted"]) == (5, 1)


@pytest.mark.parametrize("build", BUILDS)
def test_later_candidates_at_the_limit(build, ctx):
    """later_max candidates come with the unit's records; one more makes the unit far: listed by the lean build, walked in
    place by the full build"""
    K = ctx.K
    below, above = ctx.check("later%d" % K["later_max"], build), ctx.check("later%d" % (K["later_max"] + 1), build)
    assert below["nfar"] == 0 and above["nfar"] == (1 if build == "lean" else 0)


@pytest.mark.parametrize("build", BUILDS)
def test_later_block_seams_at_256_queries(build, ctx):
    got = {kind: ctx.check("seam_%s_8" % kind, build, 8) for kind in ("inside", "ends_on", "one", "two")}
    assert [got[k]["nfar"] for k in ("inside", "ends_on", "one")] == [0, 0, 0]
    assert got["two"]["nfar"] == (1 if build == "lean" else 0)          # far by boundary, with ten candidates


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("kind", ["one", "two"])
def test_later_block_seams_at_1024_queries_and_unaligned_arrays(kind, build, ctx):
    """2^16 queries and more from aligned arrays: four queries per thread, blocks of 2^10 (the host entry's staging arrays);
    the same batch from device arrays 4 bytes off a 16-byte boundary: one query per thread, blocks of 2^8"""
    import torch
    name = "seam_%s_10" % kind
    want = ctx.check(name, build, 10)
    assert want["lb_shift"] == 10 and want["nfar"] == (1 if (kind, build) == ("two", "lean") else 0)
    case, K = ctx.cases[name], ctx.K
    want8 = mj.predict(case, K, build == "full", 8)
    db = ctx.open_db(case, build)
    try:
        dev, n = torch.device("cuda:0"), len(case.qs)
        buf = [torch.empty(n + 1, dtype=torch.int32, device=dev) for _ in range(3)]
        for b, a in zip(buf, (case.ichr, case.qs, case.qe)):
            b[1:].copy_(torch.from_numpy(a))
        assert all(b[1:].data_ptr() % 16 == 4 for b in buf)
        for flags in (FLAG_SORTED, 0):
            d_hits = torch.zeros(db.nfiles, dtype=torch.int64, device=dev)
            d_tot = torch.zeros(1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            db.search_dev(buf[0][1:].data_ptr(), buf[1][1:].data_ptr(), buf[2][1:].data_ptr(), n, d_hits.data_ptr(), d_tot.data_ptr(), flags=flags)
            db.sync()
            routes = db.last_batch_routes()
            print(name, build, "unaligned flags", flags, routes)
            np.testing.assert_array_equal(d_hits.cpu().numpy(), ctx.reference(name)[0][0])
            assert int(d_tot.item()) == ctx.reference(name)[0][1]
            assert {w: routes[w] for w in want8} == want8
        assert want8["lb_shift"] == 8
    finally:
        db.close()


@pytest.mark.parametrize("build", BUILDS)
def test_dense_tiles_around_the_rank_methods_start_and_its_lds_array(build, ctx):
    """dense_min - 1, dense_min, dense_min + 1 first-tile queries (the full build counts by rank from dense_min on), and sbcap - 1,
    sbcap, sbcap + 1 (the tile's query starts fit the wave's LDS array below sbcap); the lean build lists the tile from
    lean_first + 1 queries on"""
    D, L, H, S, C = ctx.dense_sizes()
    for n in (D - 1, D, D + 1, C - 1, C, C + 1):
        want = ctx.check("dense%d" % n, build)
        assert want["nheavys"] == (1 if build == "lean" and n > L else 0) and want["nfar"] == 0


@pytest.mark.parametrize("build", BUILDS)
def test_dense_tiles_at_the_skew_valves_thresholds(build, ctx):
    """lean_first / + 1: the lean build lists the tile for heavy_sorted_body (0 -> 1); heavy_first / + 1: the full build does;
    one query short of a full last slice and a full slice plus one"""
    D, L, H, S, C = ctx.dense_sizes()
    assert ctx.check("dense%d" % L, build)["nheavys"] == 0
    assert ctx.check("dense%d" % (L + 1), build)["nheavys"] == (1 if build == "lean" else 0)
    assert ctx.check("dense%d" % H, build)["nheavys"] == (1 if build == "lean" else 0)
    for n in (H + 1, H + S - 1, H + S + 1):
        assert ctx.check("dense%d" % n, build)["nheavys"] == 1


@pytest.mark.parametrize("build", BUILDS)
def test_far_units_over_many_later_blocks(build, ctx):
    """a far unit whose candidates span far_wide - 1 blocks is walked in place by the full build and listed from far_wide on;
    the lean build lists both (and the dense tile in front of them); with more than heavy_first queries in that tile both
    builds list the tile AND the unit behind it"""
    K = ctx.K
    both = ctx.check("far_wide%d" % (K["heavy_first"] // 256 + 1), build)
    assert (both["nfar"], both["nheavys"]) == (1, 1)
    below, at = ctx.check("far_wide%d" % (K["far_wide"] - 1), build), ctx.check("far_wide%d" % K["far_wide"], build)
    assert below["nfar"] == (1 if build == "lean" else 0) and at["nfar"] == 1
    assert below["nheavys"] == at["nheavys"] == (1 if build == "lean" else 0)


@pytest.mark.parametrize("build", BUILDS)
def test_rank_exceptions_inside_dense_tiles(build, ctx):
    want = ctx.check("rank_exceptions", build)
    assert want["nfix"] == 4 and want["notstart"] == 0   # the four WALK_FIRST queries; the rank method stays on


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("width", [512, 32768])
def test_sixteen_bit_coordinates(width, build, ctx):
    want = ctx.check("coords16_%d" % width, build)
    assert want["packed"] == 1 and want["nfix"] == 0


def dev_batch(db, torch, case, hits, total, flags=FLAG_SORTED):
    dev = torch.device("cuda:0")
    arrs = [torch.from_numpy(a).to(dev) for a in (case.ichr, case.qs, case.qe)]
    torch.cuda.synchronize()
    db.search_dev(arrs[0].data_ptr(), arrs[1].data_ptr(), arrs[2].data_ptr(), len(case.qs), hits.data_ptr(), total.data_ptr(), flags=flags)
    db.sync()
    return db.last_batch_routes()


@pytest.mark.parametrize("build", BUILDS)
def test_the_lists_of_a_batch_are_its_own(build, ctx):
    """one handle: a batch that lists a far unit AND a heavy tile on either build (more than heavy_first first-tile queries in
    the tile in front of the far unit), one that lists nothing, the first again -- each exact, each with its own route words;
    then the same three accumulating into one hits[]"""
    import torch
    K = ctx.K
    busy, quiet = ctx.cases["far_wide%d" % (K["heavy_first"] // 256 + 1)], ctx.cases["later%d" % K["later_max"]]
    assert busy.recs == quiet.recs and busy.ntile == quiet.ntile            # one database serves both batches
    db = ctx.open_db(busy, build)
    orc = Oracle(ctx.path_of(busy))
    try:
        ref = {id(c): orc.search(c.ichr, c.qs, c.qe, 0) for c in (busy, quiet)}
        dev = torch.device("cuda:0")
        acc, acct = torch.zeros(db.nfiles, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        sum_h, sum_t = np.zeros(db.nfiles, np.int64), 0
        for accumulate in (False, True):
            for c in (busy, quiet, busy):
                hits = acc if accumulate else torch.zeros(db.nfiles, dtype=torch.int64, device=dev)
                tot = acct if accumulate else torch.zeros(1, dtype=torch.int64, device=dev)
                routes = dev_batch(db, torch, c, hits, tot)
                want = mj.predict(c, K, build == "full", 8)
                assert {w: routes[w] for w in want} == want
                if c is quiet:
                    assert routes["nfar"] == 0 and routes["nheavys"] == 0
                else:
                    assert routes["nfar"] == 1 and routes["nheavys"] == 1     # both lists, on either build
                if accumulate:
                    sum_h, sum_t = sum_h + ref[id(c)][0], sum_t + ref[id(c)][1]
                np.testing.assert_array_equal(hits.cpu().numpy(), sum_h if accumulate else ref[id(c)][0])
                assert int(tot.item()) == (sum_t if accumulate else ref[id(c)][1])
    finally:
        db.close(); orc.close()


@pytest.mark.parametrize("build", BUILDS)
def test_a_broken_promise_inside_a_dense_tile(build, ctx):
    """two starts swapped inside the dense tile under flags = 1: the batch adds nothing and is reported; unpromised the same
    batch is a legal merge-join batch (ordered by tile, not by start); the handle serves the next batch exactly"""
    import torch
    from igd_amd.database import IgdError
    K = ctx.K
    good, bad = ctx.cases["dense%d" % (K["lean_first"] + 1)], ctx.cases["dense%d_swapped" % (K["lean_first"] + 1)]
    db = ctx.open_db(good, build)
    try:
        dev = torch.device("cuda:0")
        hits, tot = torch.zeros(db.nfiles, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        with pytest.raises(IgdError):
            dev_batch(db, torch, bad, hits, tot)
        assert int(hits.sum().item()) == 0 and int(tot.item()) == 0
        assert db.last_batch_routes()["unsorted"] == 1
        ref_hits, ref_total = ctx.reference(good.name)[0]                       # (the same queries, so the same counts)
        routes = dev_batch(db, torch, bad, hits, tot, flags=0)
        assert routes["unsorted"] == 0 and routes["notstart"] == 1 and routes["kernel"] == "igd_scan_sorted"
        np.testing.assert_array_equal(hits.cpu().numpy(), ref_hits)
        assert int(tot.item()) == ref_total
        hits.zero_(); tot.zero_()
        routes = dev_batch(db, torch, good, hits, tot)
        want = mj.predict(good, K, build == "full", 8)
        assert {w: routes[w] for w in want} == want
        np.testing.assert_array_equal(hits.cpu().numpy(), ref_hits)
        assert int(tot.item()) == ref_total
    finally:
        db.close()
