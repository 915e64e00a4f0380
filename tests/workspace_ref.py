"""Reference for the permutation nulls inside a workspace, in plain Python and numpy uint64.  A plain module: no pytest hooks.

Written from the definition (include/igd_hip.h, THE WORKSPACE), not from the C code.

    table(...)    the workspace table of a segment list: per contig the segments merged at gap 0 (touching ones join, empty
                  and inverted ones and those on unknown contigs are dropped), clipped to [0, L], ordered by length
                  descending then start ascending; w_off int64[nctg + 1], w_start / w_len int32[nseg] and w_pre
                  int32[nseg + nctg] with n + 1 prefix sums per contig (contig c's begin at w_off[c] + c)
    place(...)    the explicit permuted lists int32[np, nq]: region i = (c, s, e), len = e - s, r = r(p, i) of permute_ref;
                  kk = #{segments of c with w_len >= len}; F(j) = prefix(j) - j (len - 1); T = F(kk); T == 0: unchanged;
                  u = r mod T; j with F(j) <= u < F(j + 1); s' = w_start[j] + u - F(j)
    inside(...)   which regions lie inside one segment of the table"""
import numpy as np

import permute_ref as PR


def table(ichr, a, b, ctg_len):
    ctg_len = [int(x) for x in ctg_len]
    nctg = len(ctg_len)
    per = [[] for _ in range(nctg)]
    for c, x, y in zip(ichr, a, b):
        if 0 <= int(c) < nctg and int(y) > int(x):
            per[int(c)].append((int(x), int(y)))
    w_off, w_start, w_len, w_pre = [0], [], [], []
    for c in range(nctg):
        runs = []
        for x, y in sorted(per[c]):
            if runs and x <= runs[-1][1]:
                runs[-1][1] = max(runs[-1][1], y)
            else:
                runs.append([x, y])
        segs = []
        for x, y in runs:
            x, y = max(x, 0), min(y, ctg_len[c])
            if y - x >= 1:
                segs.append((x, y - x))
        segs.sort(key=lambda t: (-t[1], t[0]))
        w_pre.append(0)
        for x, ln in segs:
            w_start.append(x)
            w_len.append(ln)
            w_pre.append(w_pre[-1] + ln)
        w_off.append(len(w_start))
    return dict(nctg=nctg, nseg=len(w_start), w_off=np.array(w_off, np.int64), w_start=np.array(w_start, np.int32).reshape(-1),
                w_len=np.array(w_len, np.int32).reshape(-1), w_pre=np.array(w_pre, np.int32).reshape(-1))


def contig(tab, c):
    """(starts, lengths, prefix[n + 1]) of contig c as Python-int arrays"""
    o, e = int(tab["w_off"][c]), int(tab["w_off"][c + 1])
    return (tab["w_start"][o:e].astype(np.int64), tab["w_len"][o:e].astype(np.int64), tab["w_pre"][o + c:e + c + 1].astype(np.int64))


def weights(tab, c, ln):
    """(kk, F int64[kk + 1]) of a region of length ln on contig c"""
    st, wl, pre = contig(tab, c)
    kk = int((wl >= ln).sum())
    assert (wl[:kk] >= ln).all() and (wl[kk:] < ln).all()
    return kk, pre[:kk + 1] - np.arange(kk + 1, dtype=np.int64) * (ln - 1)


def place(ichr, qs, qe, ctg_len, tab, p0, np_, seed=0):
    """(qs', qe') int32[np_, nq]; regions on unknown contigs, invalid regions and regions that fit nowhere pass through"""
    ichr, qs, qe = np.asarray(ichr, np.int64), np.asarray(qs, np.int64), np.asarray(qe, np.int64)
    nq, nctg = len(qs), len(ctg_len)
    out_s, out_e = np.tile(qs, (np_, 1)), np.tile(qe, (np_, 1))
    p = np.arange(np_, dtype=np.uint64) + np.uint64(p0)
    for i in range(nq):
        c, s, e = int(ichr[i]), int(qs[i]), int(qe[i])
        if not 0 <= c < nctg:
            continue
        L, ln = int(ctg_len[c]), e - s
        if L < 1 or s < 0 or ln < 0 or e > L:
            continue
        kk, F = weights(tab, c, ln)
        T = int(F[kk])
        if T == 0:
            continue
        assert (np.diff(F) >= 1).all() and T <= 2 ** 32
        u = (PR.r(seed, p, np.full(np_, i, np.uint64)) % np.uint64(T)).astype(np.int64)
        j = np.searchsorted(F, u, side="right") - 1
        assert (j >= 0).all() and (j < kk).all()
        st = contig(tab, c)[0]
        out_s[:, i] = st[j] + (u - F[j])
        out_e[:, i] = out_s[:, i] + ln
    return out_s.astype(np.int32), out_e.astype(np.int32)


def unplaceable(ichr, qs, qe, ctg_len, tab):
    """bool[nq]: valid regions on known contigs with T == 0"""
    out = np.zeros(len(qs), bool)
    for i, (c, s, e) in enumerate(zip(ichr, qs, qe)):
        c, s, e = int(c), int(s), int(e)
        if 0 <= c < len(ctg_len) and int(ctg_len[c]) >= 1 and 0 <= s <= e <= int(ctg_len[c]):
            kk, F = weights(tab, c, e - s)
            out[i] = F[kk] == 0
    return out


def inside(ichr, s, e, tab):
    """bool[...]: (c, s, e) lies inside one segment of its contig; ichr is per column, s and e may be [np, nq]"""
    s, e = np.asarray(s, np.int64), np.asarray(e, np.int64)
    out = np.zeros(s.shape, bool)
    for i, c in enumerate(ichr):
        if not 0 <= int(c) < tab["nctg"]:
            continue
        st, wl, _ = contig(tab, int(c))
        si, ei = s[..., i], e[..., i]
        out[..., i] = ((st[:, None] <= si.reshape(1, -1)) & (ei.reshape(1, -1) <= (st + wl)[:, None]) & (ei >= si).reshape(1, -1)).any(axis=0).reshape(si.shape)
    return out


def random_workspace(rng, ctg_len, nseg_per_ctg, max_len):
    """segment lists (ichr, a, b): per contig about nseg_per_ctg segments, some overlapping, touching, nested, empty, inverted
    or past the contig's end, one contig number the call does not know"""
    rows = []
    for c, L in enumerate(int(x) for x in ctg_len):
        for _ in range(nseg_per_ctg):
            x = rng.randrange(-50, L + 50)
            rows.append((c, x, x + rng.choice([0, -3, 1, 2, rng.randint(1, max_len), max_len])))
        rows.append((c, L // 2, L // 2 + max_len))
        rows.append((c, L // 2 + max_len, L // 2 + 2 * max_len))          # touching
        rows.append((c, L // 2 + 5, L // 2 + 6))                          # nested
    rows.append((len(ctg_len), 5, 500))
    rows.append((-1, 5, 500))
    rng.shuffle(rows)
    a = np.array(rows, np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32)


SEG_COUNTS = (0, 1, 2, 3, 63, 64, 65, 1000)


def segment_cases():
    """(ctg_len, segments (ichr, a, b), regions (ichr, qs, qe)): one contig per segment count of SEG_COUNTS and kind -- all
    lengths equal (7), all distinct (1 .. n, shuffled along the contig) -- and on each regions of length 0, 1, the k-th length
    for several k, one above and one below it, the longest (one start per longest segment) and one above the longest (it fits
    nowhere and stays), at several starts"""
    import random
    rng = random.Random(77)
    ctg_len, seg, reg = [], [], []
    for kind in ("equal", "distinct"):
        for n in SEG_COUNTS:
            c = len(ctg_len)
            lens = [7] * n if kind == "equal" else list(range(1, n + 1))
            rng.shuffle(lens)
            at = 3
            for ln in lens:
                seg.append((c, at, at + ln))
                at += ln + rng.randint(1, 4)
            L = at + 11
            ctg_len.append(L)
            srt = sorted(lens, reverse=True)
            want = {0, 1, 2}
            for k in (0, 1, n // 2, n - 2, n - 1):
                if 0 <= k < n:
                    want |= {srt[k], srt[k] + 1, max(srt[k] - 1, 0)}
            want |= {(srt[0] if n else 0) + 1, (srt[0] if n else 0) + 5}
            for ln in sorted(x for x in want if x <= L):
                for s in (0, L - ln, (L - ln) // 2):
                    reg.append((c, s, s + ln))
    reg += [(-1, 5, 9), (len(ctg_len), 0, 3)]
    s3 = lambda rows: tuple(np.array(rows, np.int64).reshape(-1, 3)[:, k].astype(np.int32) for k in range(3))
    return np.array(ctg_len, np.int32), s3(seg), s3(reg)
