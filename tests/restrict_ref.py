"""Brute-force reference and fixtures for query sets restricted to a universe (igdc_restrict_host / igd_hip_restrict_sets,
igdc_enrich_restricted_host / igd_hip_enrich_restricted, `-U -X`).  A plain module: no pytest hooks.

    R_k = { u : some region q of set k has ichr_q == u_ichr_u >= 0, u_qs_u < qe_q and u_qe_u > qs_q }

    join()            bool[nsets, nu]: an O(regions x nu) numpy broadcast of that predicate (each distinct region of a set once:
                      duplicate set regions add nothing)
    pack()            the rows as uint32 words, region u = bit u & 31 of word u >> 5, bits >= nu zero
    gather()          support, usupport, nhit, unhit from R and the universe's membership matrix (bool[nu, nfiles])
    tables()          b, c, d of every cell from the definitions
    explicit_lists()  R_k as explicit regions, the universe's own triples in universe order: the input of the equivalence
    gather_rows()     the same four results row by row (member[R[k]].sum(axis=0)): exact, and cheap where the rows are sparse
    join_cases()      the join's edge fixtures, each with the conditions that keep it from being vacuous
    many_regions()    600 000 set regions drawn from a small pool, more than the lanes of the join kernel's largest grid
    scale_a(), scale_b(), scale_d_sets()   the fixtures that take igd_bits_support past one item per workgroup, one block per
                      row and two busy waves, with their conditions (second_item_conditions, block_conditions, seam_conditions)"""
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


def gather_rows(R, member):
    """gather() without the nsets x nu x nfiles product: per row the sum over the member rows of its set bits.  Exact (int64
    sums of booleans); the form for many sparse rows or a wide membership matrix."""
    anyf = member.any(axis=1)
    sup = np.zeros((R.shape[0], member.shape[1]), np.int64)
    nhit = np.zeros(R.shape[0], np.int64)
    for k in range(R.shape[0]):
        idx = np.flatnonzero(R[k])
        if len(idx):
            sup[k] = member[idx].sum(axis=0, dtype=np.int64)
            nhit[k] = anyf[idx].sum()
    return sup, member.sum(axis=0, dtype=np.int64), nhit, int(anyf.sum())


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


def many_contigs(seed=13, ncontig=150):
    """Universe regions on 150 contig numbers -- odd numbers with gaps, given in shuffled order -- so that cval[] has 150
    entries.  Set 0 has one region on every contig present, set 1 regions on even numbers between them, set 2 on numbers
    below the lowest contig, set 3 on numbers above the highest, set 4 present and absent numbers mixed."""
    rng = np.random.default_rng(seed)
    odd = np.arange(11, 1400, 2)
    ctg = np.sort(rng.choice(odd, ncontig, replace=False))
    assert (np.diff(ctg) > 2).any() and (np.diff(ctg) == 2).any() and ctg[0] > 2
    uni = [(int(c), 1000 * j + int(c), 1000 * j + int(c) + 300) for c in ctg for j in range(3)]
    uni = [uni[i] for i in rng.permutation(len(uni))]
    gaps = [int(c) + 1 for c in ctg[:-1]]
    lists = [[(int(c), 1100 + int(c), 1200 + int(c)) for c in ctg[rng.permutation(ncontig)]],
             [(c, 0, 10 ** 6) for c in gaps],
             [(0, 0, 10 ** 6), (2, 0, 10 ** 6), (int(ctg[0]) - 1, 0, 10 ** 6)],
             [(int(ctg[-1]) + 1, 0, 10 ** 6), (int(ctg[-1]) + 2, 0, 10 ** 6), (2 ** 31 - 1, 0, 10 ** 6)],
             [(gaps[0], 0, 10 ** 6), (int(ctg[0]), 0, 10 ** 6), (gaps[70], 0, 10 ** 6), (int(ctg[-1]), 2000 + int(ctg[-1]), 2001 + int(ctg[-1])), (5000, 0, 9)]]

    def check(R):
        c = np.array([r[0] for r in uni])
        s = np.array([r[1] for r in uni])
        assert len(np.unique(c)) == ncontig and not all(uni[i] <= uni[i + 1] for i in range(len(uni) - 1))
        assert R[0].sum() == ncontig and all(R[0][(c == x) & (s == 1000 + x)].all() for x in ctg)     # the middle region of each
        assert not R[1].any() and not R[2].any() and not R[3].any()
        assert R[4][c == ctg[0]].all() and R[4].sum() == 4 and R[4][(c == ctg[-1]) & (s == 2000 + ctg[-1])].all()
    return sets_of(lists), universe_of(uni), check


I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def coordinate_extremes():
    """INT32_MIN, INT32_MAX, 0 and negative starts as starts and as ends, on both sides; one set per region, so every pair is
    a cell of R.  The expectation is the predicate in Python integers: u_qs < qe and u_qe > qs, nothing special-cased."""
    lo, hi = I32_MIN, I32_MAX
    uni = [(0, lo, lo + 10), (0, lo, hi), (0, lo, lo), (0, -100, -50), (0, -5, 5), (0, 0, 0), (0, 0, 1), (0, 0, hi), (0, hi - 1, hi),
           (0, hi, hi), (0, hi, lo), (0, 100, lo), (0, -70, hi), (0, lo + 1, 0), (0, lo, 0), (0, 7, hi)]
    regs = [(0, lo, lo + 1), (0, lo, 0), (0, lo, hi), (0, lo, lo), (0, -60, -55), (0, -1, 0), (0, 0, 1), (0, 0, hi), (0, hi - 1, hi),
            (0, hi, hi), (0, hi, lo), (0, 0, lo), (0, -2 ** 30, 2 ** 30), (0, lo + 9, lo + 10), (0, lo + 10, lo + 11), (0, 3, -2)]
    want = np.array([[u[1] < q[2] and u[2] > q[1] for u in uni] for q in regs])

    def check(R):
        assert np.array_equal(R, want)
        assert R[0].tolist()[:3] == [True, True, False] and R[2].sum() == sum(1 for u in uni if u[1] < hi and u[2] > lo)
        assert R[9].sum() == 0 and not R[3].any()                    # [hi, hi) and [lo, lo) meet nothing: nothing starts below lo
        assert R[8].tolist()[7:10] == [True, True, False]            # [hi - 1, hi) meets [0, hi) and itself, not [hi, hi)
        assert R[13, 0] and not R[14, 0]                             # the last base of [lo, lo + 10), and the one behind it
        assert R[10].sum() == 0 and R[15].any()                      # inverted: [hi, lo) meets nothing, [3, -2) what starts below -2 and ends behind 3
        assert want.any(axis=0).sum() >= 12 and want.any(axis=1).sum() >= 12
    return sets_of([[r] for r in regs]), universe_of(uni), check


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
    out.append(("many contigs",) + many_contigs())
    out.append(("coordinate extremes",) + coordinate_extremes())
    z = np.zeros(0, np.int32)
    out.append(("no set", ((z, z, z), np.zeros(1, np.int64)), universe_of([(0, 1, 2), (0, 5, 9)]), None))
    out.append(("no universe", sets_of([[(0, 1, 2)], [], [(0, 5, 9)]]), (z, z, z), None))
    return out


# ---- igd_bits_support past one item per workgroup, one block per row and two busy waves ----------------------------------------
# A work item is (row k, block of `block_words` words of the row); gridDim = min(items, grid) persistent workgroups stride over
# the items, row-major: item it = k * nblk + block.  The first launch carries one row more than there are sets: the ones row.
def _regions_of(uni, idx):
    return [(int(uni[0][i]), int(uni[1][i]), int(uni[2][i])) for i in idx]


def scale_a(uni, anchors, grid, span, extra_sets=300, dead=24, seed=31):
    """Case A: second items with one block per row.  `uni` is the universe of test_enrich_host.enrich_fixture (contig 0 =
    chr1 over [0, span) without a hole of span / 10 in the middle, contig 1 = chr2; file 0 lies in the first twentieth of
    chr1, the last file on chr2); `dead` regions are appended on chr1 behind every record.  grid + extra_sets sets of 3 to
    30 regions; sets 0, 1, the last one and every 7th are empty.
      sets below grid        begin with two of `anchors` -- universe regions of the first twentieth that the caller knows
                             file 0 to meet under every filter it uses -- and may hold chr2 regions
      sets from grid on      hold neither, so their support in file 0 and in the last file is 0 while that of the set `grid`
                             below them -- the first item of the workgroup that takes them as its second -- is not;
                             those whose partner below is empty lie where the universe has nothing: R_k is empty
    Regions are copies of universe regions, intervals of 1 to 400 bp that meet 0 to 3 of them, regions in the hole, on
    contigs 99 and -1, inverted ones; every 9th set from grid on also takes a dead region.
    Returns dict(uni, cat, off, lists, ndead)."""
    rng = np.random.default_rng(seed)
    uc, us, ue = (np.asarray(a, np.int64) for a in uni)
    far = span + 16 * 2048
    uc = np.concatenate([uc, np.zeros(dead, np.int64)])
    us = np.concatenate([us, far + 160 * np.arange(dead)])
    ue = np.concatenate([ue, far + 160 * np.arange(dead) + 100])
    uni = (_i32(uc), _i32(us), _i32(ue))
    nu = len(us)
    hole = (span // 2, span // 2 + span // 10)
    head = np.asarray(anchors, np.int64)
    assert ((uc[head] == 0) & (us[head] < span // 20)).all()
    rest = np.flatnonzero((uc == 0) & (us >= span // 20 + 1000) & (us < span))
    chr2 = np.flatnonzero(uc == 1)
    deadi = np.arange(nu - dead, nu)
    assert len(head) >= 20 and len(rest) > 1000 and len(chr2) > 20
    nsets = grid + extra_sets

    def empty(k):
        return k in (0, 1, nsets - 1) or k % 7 == 0

    def off_universe():
        kind = rng.integers(0, 4)
        s = int(rng.integers(hole[0], hole[1] - 500))
        if kind == 0:
            return (0, s, s + int(rng.integers(1, 300)))
        if kind == 1:
            return (int(rng.choice([99, -1])), int(rng.integers(0, span)), int(rng.integers(0, span)) + span)
        if kind == 2:
            i = int(rng.choice(rest))
            return (0, int(ue[i]) + 5, int(us[i]) - 5)                     # an inverted region around a universe region
        return (0, span + 1000 + s, span + 1400 + s)                       # behind the universe, before the dead regions

    lists = []
    for k in range(nsets):
        if empty(k):
            lists.append([])
            continue
        n = int(rng.integers(3, 31))
        late = k >= grid
        if late and empty(k - grid):
            lists.append([off_universe() for _ in range(n)])
            continue
        regs = []
        if not late:
            regs += _regions_of(uni, rng.choice(head, 2, replace=False))
        if late and k % 9 == 0:
            regs += _regions_of(uni, rng.choice(deadi, 1))
        while len(regs) < n:
            kind = rng.integers(0, 10)
            if kind < 6:
                regs += _regions_of(uni, rng.choice(rest, 1))
            elif kind < 8:
                s = int(rng.integers(span // 20 + 1200, span - 500))
                regs.append((0, s, s + int(rng.integers(1, 401))))
            elif kind == 8 and not late:
                regs += _regions_of(uni, rng.choice(chr2, 1))
            else:
                regs.append(off_universe())
        lists.append([regs[i] for i in rng.permutation(len(regs))])
    cat, off = sets_of(lists)
    return dict(uni=uni, cat=cat, off=off, lists=lists, ndead=dead)


def second_item_conditions(R, member, sup, usup, grid, what=""):
    """Case A, on the reference alone.  Returns the figures it asserts on."""
    nsets = R.shape[0]
    assert nsets + 1 > grid and R.shape[1] <= 8192
    late = [k for k in range(grid, nsets) if sup[k].any()]
    assert len(late) >= 200, "%s: only %d sets from %d on have support" % (what, len(late), grid)
    for k in late:
        first = sup[k - grid]
        assert first.any() and ((sup[k] == 0) & (first != 0)).any(), "%s: set %d and its workgroup's first set %d" % (what, k, k - grid)
    quiet = [k for k in range(grid, nsets) if not R[k].any()]
    assert len(quiet) >= 30 and any(not R[k - grid].any() for k in quiet) and any(sup[k - grid].any() for k in quiet)
    nohit = ~member.any(axis=1)
    dead_bits = int(R[:, nohit].sum())
    dead_late = int(R[grid:, nohit].sum())
    assert dead_bits > 0 and dead_late > 0, "%s: no set bit on a universe region without a hit" % what
    assert usup.any() and sup[nsets - grid].any(), "%s: the ones row's workgroup holds nothing from its first item" % what
    assert not R[0].any() and not R[1].any() and not R[nsets - 1].any() and not R[::7].any()
    return dict(sets=nsets, late_with_support=len(late), late_empty=len(quiet), dead_bits=dead_bits, dead_bits_late=dead_late,
                universe_without_hit=int(nohit.sum()), ones_row_workgroup=nsets - grid)


def scale_b(span, block_words, nsets=900, seed=41):
    """Case B: a universe of 2 blocks + 114 words - 21 regions (20 011 for blocks of 256 words: nu % 32 = 11, the last word
    is word 113 of block 2, inside wave 1) over the database of enrich_fixture.  Regions overlap: 90 % of 10 to 90 bp, 8 %
    of 100 to 2 000, 2 % of 3 to 9 tiles of 2 048 bp; 1 500 lie behind everything the database reaches, 40 on chr2, 12 have
    ichr = -1; the order is shuffled.  nsets sets of 0 to 40 regions (every 11th empty): copies of universe regions and
    intervals of 1 to 300 bp, which meet some twenty regions each; sets 5 and 700 are the whole of chr1.
    Returns dict(uni, cat, off, lists)."""
    rng = np.random.default_rng(seed)
    nu = (2 * block_words + block_words // 4 + 50) * 32 - 21
    nfar, nchr2, nneg = 1500, 40, 12
    n0 = nu - nfar - nchr2 - nneg
    kind = rng.random(n0)
    ln = np.where(kind < 0.9, rng.integers(10, 91, n0), np.where(kind < 0.98, rng.integers(100, 2001, n0), rng.integers(3 * 2048, 9 * 2048, n0)))
    us = rng.integers(0, span, n0)
    uc = np.zeros(n0, np.int64)
    fs = rng.integers(span + 20000, span + 60000, nfar)
    cs = rng.integers(0, span, nchr2)
    ns = rng.integers(0, span, nneg)
    uc = np.concatenate([uc, np.zeros(nfar, np.int64), np.ones(nchr2, np.int64), -np.ones(nneg, np.int64)])
    ue = np.concatenate([us + ln, fs + rng.integers(10, 91, nfar), cs + rng.integers(50, 2000, nchr2), ns + 100])
    us = np.concatenate([us, fs, cs, ns])
    order = rng.permutation(nu)
    uni = (_i32(uc[order]), _i32(us[order]), _i32(ue[order]))
    lists = []
    for k in range(nsets):
        if k % 11 == 0:
            lists.append([])
            continue
        if k in (5, 700):
            lists.append([(0, 0, span + 10 ** 5)])
            continue
        regs = []
        for _ in range(int(rng.integers(1, 41))):
            if rng.random() < 0.6:
                regs += _regions_of(uni, rng.integers(0, nu, 1))
            else:
                s = int(rng.integers(-100, span + 70000))
                regs.append((int(rng.choice([0, 0, 0, 0, 0, 0, 1, 7])), s, s + int(rng.integers(1, 301))))
        lists.append(regs)
    cat, off = sets_of(lists)
    return dict(uni=uni, cat=cat, off=off, lists=lists)


def block_conditions(R, member, grid, block_words, waves=4, what=""):
    """Case B, on the reference alone: rows + 1 rows of nblk blocks are more items than `grid`; every (block, wave) that
    holds words of the universe has, in some item >= grid of a set other than the whole-chr1 ones, a set bit with a hit;
    waves 2 and 3 of block 0 have one in an item < grid too.  Returns the figures."""
    nsets, nu = R.shape
    nUW = (nu + 31) // 32
    nblk = -(-nUW // block_words)
    per = block_words // waves
    items = (nsets + 1) * nblk
    assert nblk == 3 and nu % 32 != 0 and items > grid
    last = (nUW - 1) % block_words
    assert per <= last < 2 * per, "%s: the last word is word %d of its block, not inside wave 1" % (what, last)
    live = R & member.any(axis=1)[None, :]
    small = R.sum(axis=1) < 2000
    reach = {}
    for it in range(nsets * nblk):                                          # (the ones row reaches every wave by itself)
        k, blk = divmod(it, nblk)
        if not small[k]:
            continue
        for w in range(waves):
            a = (blk * block_words + w * per) * 32
            if a < nu and live[k, a:a + per * 32].any():
                key = (blk, w, it >= grid)
                reach[key] = reach.get(key, 0) + 1
    want = [(b, w) for b in range(nblk) for w in range(waves) if (b * block_words + w * per) * 32 < nu]
    assert len(want) == 2 * waves + 2
    for b, w in want:
        assert reach.get((b, w, True), 0) > 0, "%s: no second item reaches block %d, wave %d" % (what, b, w)
    assert reach.get((0, 2, False), 0) > 0 and reach.get((0, 3, False), 0) > 0
    # a workgroup's two items are `grid` items apart: another row always (grid > nblk), another block unless nblk divides grid
    second = [(w // nblk, (w + grid) // nblk, w % nblk, (w + grid) % nblk) for w in range(items - grid)]
    other_row = sum(1 for a, b, _, _ in second if a != b)
    other_blk = sum(1 for _, _, a, b in second if a != b)
    assert other_row == len(second) > 600 and other_blk == len(second)
    full = int((pack(R) == 0xffffffff).sum())
    assert full > 1000 and R[5].sum() == R[700].sum() > nu - 2000
    return dict(nu=nu, nUW=nUW, nblk=nblk, items=items, second_items=len(second), other_row=other_row, other_block=other_blk,
                full_words=full, late_items_per_block_wave={"%d/%d" % (b, w): reach[(b, w, True)] for b, w in want},
                universe_without_hit=int((~member.any(axis=1)).sum()))


def seam_conditions(R, member, step, block_words, what=""):
    """Case C, on the reference alone: membership chunks of `step` universe regions begin inside a word, hold more than one
    block of words, and some set has bits with a hit on either side of each cut and in each block of the middle chunk."""
    nu = R.shape[1]
    live = R & member.any(axis=1)[None, :]
    cuts = list(range(step, nu, step))
    assert len(cuts) >= 2 and all(c % 32 for c in cuts)
    w0, w1 = cuts[0] >> 5, (cuts[1] + 31) >> 5
    assert block_words < w1 - w0 <= 2 * block_words
    for c in cuts:
        lo = (c >> 5) << 5
        assert live[:, lo:c].any() and live[:, c:lo + 32].any(), "%s: no bit with a hit on both sides of the cut at %d" % (what, c)
    mid = (w0 + block_words) << 5
    assert live[:, cuts[0]:mid].any() and live[:, mid:cuts[1]].any()
    return dict(cuts=cuts, words_of_middle_chunk=w1 - w0)
