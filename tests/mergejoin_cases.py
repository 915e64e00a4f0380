"""Constructed databases and position-sorted batches that put the merge join (k_query_bounds + igd_scan_sorted and the
batch's last launch) on each of its rare routes, with the property that puts a case there stated as plain numbers.

Pure numpy; nothing here touches a device.  tests/test_mergejoin_cases_host.py recomputes every claimed property from the
arrays and checks the batches against the CPU oracle; tests/test_gpu_mergejoin_routes.py runs them on the engine and reads
the route words back (Database.last_batch_routes).

One contig ("chr1") of `ntile` tiles of `nbp` base pairs, NF files.  Definitions (engine/query_bounds.hpp, scan_sorted.hpp):
  n1, n2      first / last tile of a query: qs / nbp and (qe - 1) / nbp as C divides (towards zero), n2 clamped to the last tile
  valid       the contig is known and 0 <= n1 <= last tile: the query has a first-tile word
  key         n1 clamped into the contig (an unknown contig: tile 0 for c < 0, the last tile for c >= nctg); firstQ[t] = first
              query with key >= t, and a tile's FIRST-TILE QUERIES are the c0 = firstQ[t + 1] - firstQ[t] queries with key t
  entry       a valid query with n2 > n1 leaves one word in later[]
  candidates  of tile t: the entries of the queries [firstQ[t - lb], firstQ[t]), lb = min(t, 3); looked at only when some
              query REACHES t (k = 1 .. min(n2 - n1, 3))
  crossings   (firstQ[t] >> sh) - (firstQ[t - lb] >> sh): later-block boundaries of that range at blocks of 2^sh queries
  far         reached, and more than `later_max` candidates or more than one crossing
  long        n2 - n1 >= short_tiles: tile n2 is walked exactly (WALK_LAST); n2 - n1 > short_tiles: the tiles between are COVERED
  walk_first  valid and qe <= start of tile n1: the compact image cannot express it (WALK_FIRST)
"""
import numpy as np

NF = 9                     # more than eight files: the general build of igd_scan_sorted, not one of the few-files builds
VLOW, VHIGH, VCUT = 100, 500, 300          # record values alternate; `-v VCUT` keeps every second record
# what the engine reports through Database.route_constants() on the device; the host test runs on these
DEFAULTS = dict(unit=320, round=62, short_tiles=4, dense_min=32, lean_first=512, heavy_first=8192, heavy_slice=512,
                far_wide=8, later_max=64, sbcap=2048, lean_waves=4096)


def cdiv(x, w):
    """x / w as C divides"""
    x = np.asarray(x, np.int64)
    return np.where(x >= 0, x // w, -((-x) // w))


class Case:
    def __init__(self, name, nbp, ntile, recs, queries, claims, literal=True, note=""):
        self.name, self.nbp, self.ntile, self.note = name, int(nbp), int(ntile), note
        self.recs = [(int(s), int(e), int(v), int(f)) for s, e, v, f in recs]
        q = np.array(queries, np.int64).reshape(-1, 3)
        self.ichr, self.qs, self.qe = (np.ascontiguousarray(q[:, k], np.int32) for k in range(3))
        self.claims = claims                    # property -> value, asserted by the host test against properties()
        self.literal = literal                  # every query ordinary (known contig, 0 <= qs < qe, first tile in range and not empty)

    def files(self):
        """the argument of helpers.write_igd_numpy; a record in the last tile pins ntile"""
        out = [[] for _ in range(NF)]
        for s, e, v, f in self.recs:
            out[f].append(("chr1", s, e, v))
        return out

    def write(self, path):
        from helpers import write_igd_numpy
        write_igd_numpy(path, self.files(), nbp=self.nbp, gtype=1)
        return path


def tile_recs(j, n, W, first=0, length=10, reach=None):
    """n records spread over tile j, the first on the tile's first base and the last on its last base (n >= 2), none leaving
    the tile (the last one ends exactly at the tile's end) unless reach[i] gives record i its end"""
    out = []
    for i in range(n):
        s = j * W + (i * (W - 1)) // max(n - 1, 1) if n > 1 else j * W + W // 2
        e = min(s + length, (j + 1) * W)
        if reach and i in reach:
            e = reach[i]
        k = first + i
        out.append((s, e, VHIGH if k % 2 else VLOW, k % NF))
    return out


def fill_db(counts, W, ntile=None):
    recs = []
    for j, n in sorted(counts.items()):
        recs += tile_recs(j, n, W, first=len(recs))
    nt = (max(counts) + 1) if ntile is None else ntile
    assert max(counts) == nt - 1, "the last tile must hold a record: it pins the contig's tile count"
    return recs, nt


def inside(j, W, n, lo=3, hi=None, length=700):
    """n ordinary queries with first tile j and ascending starts, none leaving the tile"""
    hi = W - 2 if hi is None else hi
    out = []
    for i in range(n):
        s = j * W + lo + (i * (hi - lo)) // max(n - 1, 1) if n > 1 else j * W + lo
        out.append((0, s, min(s + length, (j + 1) * W)))
    return out


def spanning(j, W, n, tiles, lo=100):
    """n queries that start in tile j and cover `tiles` tiles"""
    return [(0, j * W + lo + 7 * i, (j + tiles - 1) * W + 50 + i) for i in range(n)]


def ordered(qs):
    return sorted(qs, key=lambda q: (q[0] if q[0] >= 0 else -1, q[1]))          # stable: equal starts keep their order


# ------------------------------------------------------------------------------------------------------------------------
def properties(case, K=DEFAULTS, nctg=1):
    """every figure a claim or a prediction is made of, from the arrays alone"""
    W, nT = case.nbp, case.ntile
    c, qs, qe = case.ichr.astype(np.int64), case.qs.astype(np.int64), case.qe.astype(np.int64)
    rec = np.zeros(nT, np.int64)                                      # records per tile: one copy in every tile a record reaches
    for s, e, _, _ in case.recs:
        rec[s // W:(e - 1) // W + 1] += 1
    known = (c >= 0) & (c < nctg)
    n1 = cdiv(qs, W)
    n2 = np.minimum(cdiv(qe - 1, W), nT - 1)
    valid = known & (n1 >= 0) & (n1 <= nT - 1)
    key = np.where(c < 0, 0, np.where(c >= nctg, nT - 1, np.clip(n1, 0, nT - 1)))
    firstQ = np.searchsorted(key, np.arange(nT + 1), side="left")    # (a sorted batch: keys do not decrease)
    span = np.where(valid, np.maximum(n2 - n1, 0), 0)                 # tiles behind the first one
    entry = valid & (span > 0)
    cum = np.concatenate(([0], np.cumsum(entry)))
    reached = np.zeros(nT + 4, bool)
    for i in np.nonzero(entry)[0]:
        reached[n1[i] + 1:n1[i] + min(span[i], K["short_tiles"] - 1) + 1] = True
    lb = np.minimum(np.arange(nT), K["short_tiles"] - 1)
    fl, f0 = firstQ[np.arange(nT) - lb], firstQ[:nT]
    cand = cum[f0] - cum[fl]
    out = dict(rec=rec, units=-(-rec // K["unit"]), first=np.diff(firstQ), firstQ=firstQ, key=key, valid=valid, n1=n1, n2=n2,
               tiles=np.where(valid, span + 1, 0), entry=entry, cand=cand, reached=reached[:nT],
               long=valid & (span >= K["short_tiles"]), covered=valid & (span > K["short_tiles"]) & (rec[np.clip(n1, 0, nT - 1)] > 0),
               walk_first=valid & (qe <= n1 * W), sorted=bool(np.all(np.diff(key) >= 0)))
    for sh in (8, 10, 12):
        out["cross%d" % sh] = (f0 >> sh) - (fl >> sh)
    return out


def predict(case, K, full, sh):
    """the route words the construction determines (Database.last_batch_routes), for the lean or the full build of
    igd_scan_sorted at later blocks of 2^sh queries"""
    p = properties(case, K)
    cross = p["cross%d" % sh]
    far = p["reached"] & ((cross > 1) | (p["cand"] > K["later_max"]))
    listed = far if not full else far & (cross >= K["far_wide"])
    heavy = (p["rec"] > 0) & (p["first"] > (K["heavy_first"] if full else K["lean_first"]))
    return dict(kernel="igd_scan_sorted", full=1 if full else 0, packed=1, lb_shift=sh, nfix=int((p["long"] | p["walk_first"]).sum()),
                nheavys=int(heavy.sum()), nfar=int(p["units"][listed].sum()), cov_sorted=1 if p["covered"].any() else 0,
                unsorted=0, notstart=0)


def literal_hits(case, v=0):
    """all pairs: a record counts for a query when they share a base pair (and its value reaches v).  Equal to the
    reference's count for ordinary queries whose first tile is not empty."""
    hits = np.zeros(NF, np.int64)
    rs = np.array([r[0] for r in case.recs], np.int64)
    re_ = np.array([r[1] for r in case.recs], np.int64)
    rv = np.array([r[2] for r in case.recs], np.int64)
    rf = np.array([r[3] for r in case.recs], np.int64)
    keep = rv >= v if v > 0 else np.ones(len(rs), bool)
    for s, e in zip(case.qs.astype(np.int64), case.qe.astype(np.int64)):
        m = keep & (rs < e) & (re_ > s)
        hits += np.bincount(rf[m], minlength=NF)
    return hits


# ------------------------------------------------------------------------------------------------------------------------
# the cases.  W: 2^14 unless the case is about the tile width.
W14 = 1 << 14


def unit_edges(K=DEFAULTS):
    """tiles of 1, 63, 64, 65, U, U + 1, 2U and 2U + 1 records (U = records per unit): queries on the first and the last
    record of every slot of 64 records and of every unit, and one over each whole tile"""
    U = K["unit"]
    sizes = [1, 63, 64, 65, U, U + 1, 2 * U, 2 * U + 1]
    recs, nt = fill_db({j + 1: n for j, n in enumerate(sizes)}, W14)          # (tile 0 stays empty: units of empty tiles)
    qs = []
    for j, n in enumerate(sizes):
        mine = [r for r in recs if r[0] // W14 == j + 1]
        edge = sorted(set([0, n - 1] + [k for k in range(n) if k % 64 in (0, 63) or k % U in (0, U - 1)]))
        qs += [(0, mine[k][0], mine[k][0] + 1) for k in edge]
        qs.append((0, (j + 1) * W14, (j + 2) * W14))
    return Case("unit_edges", W14, nt, recs, ordered(qs),
                dict(rec={j + 1: n for j, n in enumerate(sizes)}, units={1: 1, 5: 1, 6: 2, 7: 2, 8: 3}))


def second_round(K=DEFAULTS):
    """more units than ROUND x the waves of one launch of the lean build (one unit per tile, most of them empty): the waves
    with the lowest numbers take a second round of descriptors.  Records and queries sit in the first and the last tiles.
    Tiles of 2^11 bp (searched as they are: IGD_HIP_NO_RETILE), so that half a million of them stay below 2^31 bp."""
    W = 1 << 11
    nt = K["round"] * K["lean_waves"] + 40
    assert nt * W < 2 ** 31
    tiles = list(range(1, 6)) + list(range(nt - 30, nt))
    recs, nt = fill_db({j: 7 for j in tiles}, W, nt)
    qs = []
    for j in tiles:
        qs += inside(j, W, 3) + (spanning(j, W, 1, 2) if j < nt - 1 else [])
    return Case("second_round", W, nt, recs, ordered(qs), dict(n_units_over=K["round"] * K["lean_waves"]))


def spans(extra, K=DEFAULTS):
    """queries over 2, 3 and 4 tiles (k = 1 .. 3) and exactly short_tiles tiles; `extra` > 0: five more over short_tiles + extra
    tiles (1: WALK_LAST, the tiles between are none; 2: WALK_LAST and one covered tile)"""
    S = K["short_tiles"]
    recs, nt = fill_db({j: 6 for j in range(S + 6)}, W14)
    qs = []
    for j in (0, 1, 2):
        qs += inside(j, W14, 4)
        for t in range(2, S + 1):
            qs += spanning(j, W14, 3, t, lo=200 * t)
    nlong = 0
    if extra:
        qs += spanning(1, W14, 5, S + extra, lo=5000)
        nlong = 5
    return Case("spans+%d" % extra, W14, nt, recs, ordered(qs),
                dict(max_tiles=S + extra, n_long=nlong, n_covered=nlong if extra > 1 else 0))


def later_candidates(n, K=DEFAULTS):
    """tile 5 gets n later candidates (n - 1 entries from tile 2, over tiles 2 .. 4, and one from tile 4 into tile 5); tile 4 has
    n - 1.  n = later_max + 1: tile 5's unit is far."""
    recs, nt = fill_db({j: 5 for j in range(9)}, W14)                           # (the database of far_wide(): one handle serves both)
    qs = inside(0, W14, 5) + spanning(2, W14, n - 1, 3) + inside(3, W14, 4) + spanning(4, W14, 1, 2) + inside(5, W14, 6) + inside(6, W14, 2)
    return Case("later%d" % n, W14, nt, recs, ordered(qs), dict(cand={3: n - 1, 4: n - 1, 5: n, 6: 1}, reached={3: True, 4: True, 5: True, 6: False}))


def seam(kind, sh, K=DEFAULTS):
    """the candidate range of tile 7 -- the queries of tiles 4 .. 6 -- against the boundaries of later blocks of 2^sh queries:
    kind "inside" (no boundary), "ends_on" (ends exactly on one: nothing taken from the next block), "one" (crosses one: nB > 0),
    "two" (crosses two: far by boundary, with ten candidates).  sh = 10 needs 2^16 queries: tiles 12 .. fill the batch up."""
    B = 1 << sh
    recs, nt = fill_db({j: 5 for j in range(12 + (170 if sh == 10 else 0))}, W14)
    head = {"inside": B - 16, "ends_on": B - 10, "one": B - 6, "two": B - 6}[kind]
    qs = inside(0, W14, head, length=40)
    if kind == "two":
        qs += inside(5, W14, B + 40, length=40)
    qs += spanning(6, W14, 10, 2) + inside(7, W14, 5) + inside(8, W14, 3)
    if sh == 10:
        per = -(-(65536 + 64 - len(qs)) // 170)
        for j in range(12, 182):
            qs += inside(j, W14, per, length=40)
    f0 = head + (B + 40 if kind == "two" else 0) + 10
    return Case("seam_%s_%d" % (kind, sh), W14, nt, recs, ordered(qs),
                {"cand": {7: 10}, "cross%d" % sh: {7: {"inside": 0, "ends_on": 1, "one": 1, "two": 2}[kind]},
                 "firstQ": {4: head, 7: f0}, "min_queries": 65536 if sh == 10 else 0})


def dense(n, K=DEFAULTS, swap=False):
    """n first-tile queries in tile 1, which holds two units of records (the valve deals (unit, slice) items); a few around it.
    swap: two neighbours with different starts exchanged inside the tile -- a broken order promise"""
    recs, nt = fill_db({0: 5, 1: K["unit"] + 11, 2: 5}, W14)
    mid = inside(1, W14, n, length=300)
    if swap:
        k = next(i for i in range(n // 2, n - 1) if mid[i][1] != mid[i + 1][1])
        mid[k], mid[k + 1] = mid[k + 1], mid[k]
    qs = inside(0, W14, 3) + mid + inside(2, W14, 2)
    return Case("dense%d%s" % (n, "_swapped" if swap else ""), W14, nt, recs, qs if swap else ordered(qs), dict(first={0: 3, 1: n, 2: 2}, rec={1: K["unit"] + 11}))


def far_wide(blocks, K=DEFAULTS):
    """tile 6 holds blocks x 256 first-tile queries, later_max + 6 of them reaching tile 7: tile 7's unit is far, and its
    candidates span `blocks` later blocks of 256 queries (the full build lists the unit from far_wide blocks on)"""
    recs, nt = fill_db({j: 5 for j in range(9)}, W14)
    n, m = blocks * 256, K["later_max"] + 6
    body = inside(6, W14, n - m, length=40) + spanning(6, W14, m, 2, lo=37)
    qs = body + inside(7, W14, 4)
    return Case("far_wide%d" % blocks, W14, nt, recs, ordered(qs), dict(cand={7: m}, cross8={7: blocks}, first={6: n}))


def rank_exceptions(K=DEFAULTS):
    """two dense tiles (the contig's first and last) whose ordinary queries are interleaved with every kind the rank method
    takes out of its terms: qe < qs, qe == qs, a query ending at or before its tile's start (WALK_FIRST), contig numbers the
    database does not have (keys of tile 0 and of the last tile), starts below -nbp, just below 0 and past the last tile"""
    recs, nt = fill_db({0: 90, 1: 20, 2: 20, 3: 90}, W14)
    T3 = 3 * W14
    qs = [(-1, 5, 900), (-2, 40, 90)] + [(0, -3 * W14, 50), (0, -W14, 40), (0, -W14 + 1, 300), (0, -5, 200)]
    qs += inside(0, W14, 70, lo=0, length=500)
    qs += [(0, 100, 0), (0, 2500, -3), (0, 700, 700), (0, 5000, 4000), (0, 9000, 8999), (0, 12000, 12000)]
    qs += inside(1, W14, 3) + inside(2, W14, 3)
    qs += inside(3, W14, 70, lo=0, length=500)
    qs += [(0, T3 + 50, T3), (0, T3 + 6000, 2 * W14), (0, T3 + 300, T3 + 300), (0, T3 + 7000, T3 + 6000), (0, T3 + 9000, T3 + 1)]
    qs += [(1, T3 + 20, T3 + 900), (3, T3 + 8000, T3 + 9000)]
    qs += [(0, 4 * W14 + 5, 4 * W14 + 900), (0, 9 * W14, 9 * W14 + 10)]
    # by (key, start): a contig number the database does not have shares the key of tile 0 / the last tile and stands in the
    # MIDDLE of that tile's queries, in start order (starts that decrease inside a key would switch the rank method off)
    tkey = lambda q: 0 if q[0] < 0 else nt - 1 if q[0] >= 1 else min(max(int(cdiv(q[1], W14)), 0), nt - 1)
    qs = sorted(qs, key=lambda q: (tkey(q), q[1]))
    return Case("rank_exceptions", W14, nt, recs, qs,
                dict(n_walk_first=4, first={0: 70 + 6 + 2 + 4, 3: 70 + 5 + 2 + 2}, n_invalid=2 + 2 + 2 + 2), literal=False)


def coords16(W):
    """the compact image's 16-bit coordinates at tile width W: records starting on a tile's last base that end exactly at the
    tile's end, one base past it and far past it; queries ending one base into a tile and with qe - T at W - 1, W and W + 1"""
    recs, nt = fill_db({j: 12 for j in range(7)}, W)
    last = lambda j: j * W + W - 1
    recs += [(last(1), 2 * W, VLOW, 1), (last(1), 2 * W + 1, VHIGH, 2), (last(2), 5 * W + 7, VHIGH, 3), (last(3), 4 * W + 1, VLOW, 4),
             (2 * W, 2 * W + 1, VHIGH, 5), (3 * W + 1, 4 * W, VLOW, 6)]
    qs = []
    for j in range(1, 5):
        T = j * W
        qs += [(0, T + 5, T + W - 1), (0, T + 5, T + W), (0, T + 5, T + W + 1), (0, T + W - 1, T + W), (0, T + W - 1, T + W + 1),
               (0, T + W - 2, T + W + 1), (0, T, T + 1), (0, T + W // 2, T + 2 * W + 1)]
    return Case("coords16_%d" % W, W, nt, recs, ordered(qs), dict(rec={1: 14, 2: 12 + 1 + 1 + 1, 3: 12 + 1 + 1 + 1, 4: 12 + 1 + 1, 5: 12 + 1}))


def host_cases(K=DEFAULTS):
    """every case, at the constants given"""
    L, H, S, C = K["lean_first"], K["heavy_first"], K["heavy_slice"], K["sbcap"]
    out = [unit_edges(K), second_round(K), spans(0, K), spans(1, K), spans(2, K), later_candidates(K["later_max"], K),
           later_candidates(K["later_max"] + 1, K)]
    out += [seam(kind, 8, K) for kind in ("inside", "ends_on", "one", "two")] + [seam("one", 10, K), seam("two", 10, K)]
    out += [dense(n, K) for n in (K["dense_min"] - 1, K["dense_min"], K["dense_min"] + 1, L, L + 1, C - 1, C, C + 1, H, H + 1,
                                  H + S - 1, H + S + 1)]
    out += [dense(L + 1, K, swap=True), far_wide(K["far_wide"] - 1, K), far_wide(K["far_wide"], K), far_wide(H // 256 + 1, K), rank_exceptions(K),
            coords16(512), coords16(32768)]
    return out
