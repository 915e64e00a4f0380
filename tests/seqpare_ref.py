"""Seqpare (`igd search db.igd -q f.bed -s`) restated literally, for the tests: no pytest hooks, never the engine.

The definition (head of igd_amd/csrc/engine/seqpare.hpp, Database.seqpare's docstring): the query file's contigs in
first-seen order, each contig's queries ordered by start with ties in file order.  One query's overlaps come from the CPU
oracle's orc_seq_overlaps as (idx_t = first tile of the QUERY, idx_g = index inside the record's tile, idx_f = dataset, bits
of the float32 similarity) in discovery order.  Per (query contig, dataset) group the best remaining pair is accepted again
and again: float32 similarity descending, only values > 0, ties in scan order (queries in order, a query's pairs in discovery
order); the accepted pair's query ("row") and its column (idx_t, idx_g) leave the group.  The accepted similarities are added
in float64, contigs in the query file's order and acceptance order inside a contig, one Python float at a time.

`greedy` is that loop as written (an arg-max over what remains, first maximum in scan order).  `walk` resolves the same group
in ONE pass over the candidates in greedy order (similarity descending, position ascending) -- the decomposition the kernel
uses -- cut into runs of RUN candidates, and classifies every decision; `seqpare` asserts that both accept the same pairs in
the same order, so the diagnostics describe the matching whose sums are returned."""
import collections
import ctypes as C

import numpy as np

RUN = 64            # candidates the kernel settles together

Diag = collections.namedtuple("Diag", "size accepted knocked_in_batch survived_chain rejected_by_earlier_batch")
Result = collections.namedtuple("Result", "sums sm nq args diag")
# sums: float64[nfiles], the added similarities; sm = sums / (nq + nr - sums), what the command prints
# nq: accepted query lines, known contig or not; args: (ichr, qs, qe, qgroup, ngroups) as igd_hip_seqpare takes them
# diag: {(group number of the contig, dataset): Diag} of the groups with candidates


def read_query_file(orc, qfile):
    """[(contig name, [(start, end), ..] by start, ties in file order)] in first-seen order, and the number of accepted
    lines.  A line counts when the oracle's orc_parse_bed takes it and uint32(start) <= uint32(end)."""
    lib = orc.lib
    st, en = C.c_int32(0), C.c_int32(0)
    order, ivs = [], {}
    nq = 0
    with open(qfile, "rb") as f:
        lines = f.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for line in lines:
        if len(line) > 1 and line.endswith(b"\r"):
            line = line[:-1]
        buf = C.create_string_buffer(line)
        if not lib.orc_parse_bed(buf, C.byref(st), C.byref(en)):
            continue
        if (st.value & 0xffffffff) > (en.value & 0xffffffff):
            continue
        name = buf.value.decode()
        if name not in ivs:
            ivs[name] = []
            order.append(name)
        ivs[name].append((st.value, en.value))
        nq += 1
    return [(name, sorted(ivs[name], key=lambda iv: iv[0])) for name in order], nq     # sorted() is stable


def engine_args(orc, contigs):
    """The arrays igd_hip_seqpare takes: queries of the contigs the database knows, group numbers 0, 1, .. in file order."""
    ichr, qs, qe, grp = [], [], [], []
    ng = 0
    for name, ivs in contigs:
        cid = orc.get_id(name)
        if cid < 0:
            continue
        for s, e in ivs:
            ichr.append(cid); qs.append(s); qe.append(e); grp.append(ng)
        ng += 1
    return tuple(np.array(a, np.int32) for a in (ichr, qs, qe, grp)) + (ng,)


def contig_groups(orc, name, ivs):
    """{dataset: (rows, cols, vals)} of one contig's queries, candidates in scan order: row = number of the query inside the
    contig, col = (idx_t << 32) | idx_g, val = the float32 similarity."""
    per = {}
    for j, (s, e) in enumerate(ivs):
        ov = orc.seq_overlaps(name, s, e)
        for it, ig, m, bits in ov.tolist():
            per.setdefault(m, ([], [], []))
            r, c, v = per[m]
            r.append(j); c.append((it << 32) | (ig & 0xffffffff)); v.append(bits)
    return {m: (np.array(r, np.int64), np.array(c, np.int64), np.array(v, np.int32).view(np.float32))
            for m, (r, c, v) in per.items()}


def greedy(rows, cols, vals):
    """The definition: indices (scan positions) of the accepted pairs, in acceptance order."""
    left = np.where(vals > 0, vals, np.float32(0))
    acc = []
    while len(left):
        i = int(np.argmax(left))                 # the FIRST maximum: strict '>' while scanning in order
        if not left[i] > 0:
            break
        acc.append(i)
        left[(rows == rows[i]) | (cols == cols[i])] = 0
    return acc


def walk(rows, cols, vals, run=RUN):
    """One pass in greedy order.  Returns (accepted scan positions in order, Diag)."""
    order = np.argsort(-vals, kind="stable")     # similarity descending, ties in scan order; what is not > 0 comes last
    row_by, col_by = {}, {}                      # row / column -> number (in greedy order) of the candidate that took it
    acc = []
    knocked = chain = earlier = 0
    rej_rows, rej_cols, cur = set(), set(), -1
    for i, p in enumerate(order.tolist()):
        if not vals[p] > 0:
            break
        if i // run != cur:
            cur, rej_rows, rej_cols = i // run, set(), set()
        r, c = int(rows[p]), int(cols[p])
        by = [b for b in (row_by.get(r), col_by.get(c)) if b is not None]
        if by:
            if min(by) // run < cur:
                earlier += 1
            else:
                knocked += 1
            rej_rows.add(r); rej_cols.add(c)
            continue
        if r in rej_rows or c in rej_cols:
            chain += 1
        row_by[r] = col_by[c] = i
        acc.append(p)
    return acc, Diag(len(vals), len(acc), knocked, chain, earlier)


def seqpare(orc, qfile):
    contigs, nq = read_query_file(orc, qfile)
    sums = [0.0] * orc.nfiles
    diag = {}
    g = 0
    for name, ivs in contigs:
        if orc.get_id(name) < 0:
            continue
        for m, (rows, cols, vals) in sorted(contig_groups(orc, name, ivs).items()):
            acc = greedy(rows, cols, vals)
            acc2, d = walk(rows, cols, vals)
            assert acc == acc2, "the one-pass walk is not the arg-max loop (contig %s, dataset %d)" % (name, m)
            for p in acc:
                sums[m] += float(vals[p])        # float32 -> float64 exactly, one addition at a time
            diag[(g, m)] = d
        g += 1
    sums = np.array(sums, np.float64)
    sm = sums / (float(nq) + orc.file_nr().astype(np.float64) - sums)
    return Result(sums, sm, nq, engine_args(orc, contigs), diag)


def bits(a):
    """float64 array -> its words, for bit-for-bit comparisons"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
