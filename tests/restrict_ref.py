"""Brute-force reference and fixtures for query sets restricted to a universe (igdc_restrict_host / igd_hip_restrict_sets,
igdc_enrich_restricted_host / igd_hip_enrich_restricted, `-U -X`).  A plain module: no pytest hooks.

    R_k = { u : some region q of set k has ichr_q == u_ichr_u >= 0, u_qs_u < qe_q and u_qe_u > qs_q }

    join()            bool[nsets, nu]: an O(regions x nu) numpy broadcast of that predicate (each distinct region of a set once:
                      duplicate set regions add nothing)
    pack()            the rows as uint32 words, region u = bit u & 31 of word u >> 5, bits >= nu zero
    gather()          support, usupport, nhit, unhit from R and the universe's membership matrix (bool[nu, nfiles])
    tables()          b, c, d of every cell from the definitions
    explicit_lists()  R_k as explicit regions, the universe's own triples in universe order: the input of the equivalence
    join_cases()      the join's edge fixtures, each with the conditions that keep it from being vacuous
    many_regions()    600 000 set regions drawn from a small pool, more than the lanes of the join kernel's largest grid"""
import numpy as np


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def sets_of(lists):
    """[[(ichr, qs, qe), ..], ..] -> ((ichr, qs, qe), off)"""
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in lists])
    flat = [r for s in lists for r in s]
    cat = tuple(_i32([r[i] for r in flat]) for i in range(3))
    return cat, off


def universe_of(regions):
    return tuple(_i32([r[i] for r in regions]) for i in range(3))


def join(ichr, qs, qe, off, u_ichr, u_qs, u_qe, block=4096):
    ichr, qs, qe = _i32(ichr), _i32(qs), _i32(qe)
    uc, us, ue = _i32(u_ichr)[None, :], _i32(u_qs)[None, :], _i32(u_qe)[None, :]
    R = np.zeros((len(off) - 1, uc.shape[1]), bool)
    for k in range(len(off) - 1):
        a, b = int(off[k]), int(off[k + 1])
        if b == a:
            continue
        q = np.unique(np.stack([ichr[a:b], qs[a:b], qe[a:b]], axis=1), axis=0)
        for i in range(0, len(q), block):
            c, s, e = (q[i:i + block, j][:, None] for j in range(3))
            R[k] |= ((c == uc) & (uc >= 0) & (us < e) & (ue > s)).any(axis=0)
    return R


def pack(R):
    n, nu = R.shape
    nW = (nu + 31) // 32
    wide = np.zeros((n, nW * 32), np.uint8)
    wide[:, :nu] = R
    if nW == 0:
        return np.zeros((n, 0), np.uint32)
    return np.packbits(wide, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(n, nW)


def gather(R, member):
    """(support int64[nsets, nfiles], usupport int64[nfiles], nhit int64[nsets], unhit)"""
    m = member.astype(np.int64)
    anyf = member.any(axis=1)
    return R.astype(np.int64) @ m, m.sum(axis=0), (R & anyf[None, :]).sum(axis=1).astype(np.int64), int(anyf.sum())


def tables(support, usupport, size, nu):
    b = usupport[None, :] - support
    c = np.asarray(size, np.int64)[:, None] - support
    d = nu - usupport[None, :] - c
    return b, c, d


def explicit_lists(R, u_ichr, u_qs, u_qe):
    """((ichr, qs, qe), off): set k = the universe regions of R_k, in universe order"""
    idx = [np.flatnonzero(r) for r in R]
    off = np.zeros(len(idx) + 1, np.int64)
    off[1:] = np.cumsum([len(i) for i in idx])
    cat = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    return (_i32(u_ichr)[cat], _i32(u_qs)[cat], _i32(u_qe)[cat]), off


# ---- fixtures of the join ------------------------------------------------------------------------------------------------------
BIT_EDGES = (1, 31, 32, 33, 64, 65, 2049)


def bit_edges(nu):
    """universe: nu disjoint regions on contig 0.  Set 0 = {0, nu - 1}, set 1 empty, set 2 the whole universe (the last word
    of its row is followed by the first word of set 3's), set 3 = {0, 1}: its hits fall into set 0's first word."""
    uni = [(0, 100 * u, 100 * u + 50) for u in range(nu)]
    last = nu - 1
    lists = [[(0, 10, 20), (0, 100 * last + 49, 100 * last + 60)], [], [(0, 0, 100 * nu)], [(0, 40, 100 * min(1, last) + 1)]]

    def check(R):
        assert R[0].sum() == min(2, nu) and R[0, 0] and R[0, last] and not R[1].any() and R[2].all()
        assert R[3].sum() == min(2, nu) and R[3, 0] and R[3, min(1, last)]
    return sets_of(lists), universe_of(uni), check


def order_and_contigs(seed=7):
    """A shuffled universe on contigs 0, 2 and 5 and ichr = -1; contig 3 has set regions and no universe region, contig 5
    universe regions and no set region; a set region and a universe region on -1 share their coordinates."""
    rng = np.random.default_rng(seed)
    uni = [(0, 50 * u, 50 * u + 70) for u in range(60)] + [(2, 1000 + 30 * u, 1000 + 30 * u + 10) for u in range(45)]
    uni += [(5, 10 * u, 10 * u + 100) for u in range(20)] + [(-1, 100, 200), (-1, 0, 10 ** 6)]
    uni = [uni[i] for i in rng.permutation(len(uni))]
    lists = [[(0, 120, 180), (3, 0, 10 ** 6), (2, 1000, 1015)], [(-1, 100, 200), (3, 5, 6)], [(2, 0, 5000), (0, 2990, 3100), (-1, 0, 10 ** 6)]]

    def check(R):
        c = np.array([r[0] for r in uni])
        assert R[0].any() and not R[1].any() and R[2][c == 2].all() and not R[:, c == 5].any() and not R[:, c < 0].any()
        assert not all(uni[i] <= uni[i + 1] for i in range(len(uni) - 1))
    return sets_of(lists), universe_of(uni), check


def pmax_cases():
    """[(name, sets, universe, check)]: the prefix maximum of the ends makes the walk exact and finite"""
    out = []
    short = [(0, 1000 + 100 * i, 1000 + 100 * i + 10) for i in range(300)]
    q = (0, 1000 + 100 * 299 + 2, 1000 + 100 * 299 + 7)
    uni = [(0, 0, 10 ** 6)] + short

    def far(R):
        assert R.sum() == 2 and R[0, 0] and R[0, 300]
    out.append(("long region far to the left", sets_of([[q]]), universe_of(uni), far))
    uni = [(0, 0, 500)] + short

    def stop(R):
        assert R.sum() == 1 and R[0, 300]
    out.append(("long region that ends before the query", sets_of([[q]]), universe_of(uni), stop))
    uni = [(0, 100, 900), (0, 200, 300), (0, 200, 300), (0, 250, 260), (0, 100, 900), (0, 850, 2000), (0, 300, 400)]
    lists = [[(0, 255, 256)], [(0, 299, 301)], [(0, 899, 900), (0, 899, 900)], [(0, 400, 850)]]

    def nested(R):
        assert R[0].tolist() == [True, True, True, True, True, False, False] and R[1, 1] and R[1, 2] and R[1, 6] and not R[1, 3]
        assert R[2].tolist() == [True, False, False, False, True, True, False] and R[3].tolist() == [True, False, False, False, True, False, False]
    out.append(("nested and duplicate universe regions", sets_of(lists), universe_of(uni), nested))
    uni = [(0, 100, 200), (0, 200, 300), (0, 300, 400)]
    lists = [[(0, 200, 300)], [(0, 0, 100), (0, 400, 500)], [(0, 199, 201)]]

    def touch(R):
        assert R[0].tolist() == [False, True, False] and not R[1].any() and R[2].tolist() == [True, True, False]
    out.append(("touching ends", sets_of(lists), universe_of(uni), touch))
    # empty and inverted regions, against the predicate as written: u_qs < qe and u_qe > qs
    uni = [(0, 5, 5), (0, 0, 10), (0, 8, 3), (0, 20, 20), (0, 30, 25), (0, 0, 50)]
    lists = [[(0, 0, 10)], [(0, 5, 5)], [(0, 7, 4)], [(0, 20, 20)], [(0, 26, 29)], [(0, 40, 1)]]
    F, T = False, True

    def empty(R):
        assert R[0].tolist() == [T, T, T, F, F, T]          # [5,5) and [8,3) lie "in" [0,10)
        assert R[1].tolist() == [F, T, F, F, F, T]          # [5,5) does not meet itself: 5 < 5 fails
        assert R[2].tolist() == [F, T, F, F, F, T]          # the inverted [7,4): u_qs < 4 and u_qe > 7
        assert R[3].tolist() == [F, F, F, F, F, T] and R[4].tolist() == [F, F, F, F, F, T]
        assert R[5].tolist() == [F, F, F, F, F, T]          # the inverted [40,1) lies "in" [0,50): 0 < 1 and 50 > 40
    out.append(("empty and inverted regions", sets_of(lists), universe_of(uni), empty))
    return out


def many_regions(n=600000, nu=5000, pool=1500, seed=11):
    """3 sets of n / 3 regions drawn from a pool of distinct triples over a universe of nu regions on two contigs, one of them
    long: ((ichr, qs, qe), off), universe.  Set 2's pool misses the right half of the universe."""
    rng = np.random.default_rng(seed)
    us = np.sort(rng.integers(0, 10 ** 6, nu)).astype(np.int32)
    uc = (np.arange(nu) % 2).astype(np.int32)
    ue = (us + rng.integers(1, 300, nu)).astype(np.int32)
    ue[3] = 10 ** 6 + 500
    order = rng.permutation(nu)
    uni = (uc[order], us[order], ue[order])
    pc = rng.integers(0, 2, pool).astype(np.int32)
    ps = rng.integers(0, 10 ** 6, pool).astype(np.int32)
    pe = (ps + rng.integers(-5, 120, pool)).astype(np.int32)
    per = n // 3
    pick = [rng.integers(0, pool, per), rng.integers(0, pool // 3, per), rng.integers(0, pool, per)]
    ichr, qs, qe = (np.concatenate([a[p] for p in pick]) for a in (pc, ps, pe))
    keep = qs[2 * per:] < 500000
    qs[2 * per:][~keep] = 10
    qe[2 * per:][~keep] = 5
    return (ichr.astype(np.int32), qs.astype(np.int32), qe.astype(np.int32)), np.array([0, per, 2 * per, 3 * per], np.int64), uni


def join_cases():
    """[(name, ((ichr, qs, qe), off), (u_ichr, u_qs, u_qe), check or None)]"""
    out = [("bit edges nu=%d" % nu,) + bit_edges(nu) for nu in BIT_EDGES]
    out.append(("order and contigs",) + order_and_contigs())
    out += pmax_cases()
    z = np.zeros(0, np.int32)
    out.append(("no set", ((z, z, z), np.zeros(1, np.int64)), universe_of([(0, 1, 2), (0, 5, 9)]), None))
    out.append(("no universe", sets_of([[(0, 1, 2)], [], [(0, 5, 9)]]), (z, z, z), None))
    return out
