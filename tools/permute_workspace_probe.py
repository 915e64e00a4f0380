#!/usr/bin/env python3
"""tools/permute_workspace_probe.py -- GPU box: what the placement inside a workspace costs (kernel igd_permute_workspace: two
dependent binary searches per output in a resident table) beside the free shuffle OF THE SAME BUILD, on the inputs of
tools/permute_probe.py.

Database: config 2's (synth.make_db defaults: 1 900 files, bench.py's file under --dir).  Regions = synth.make_queries(
--regions, seed=999); contig lengths as permute_probe.py.  Workspace = the genome minus --gaps synthetic gaps of 1 000 bp,
spread over the contigs in proportion to their lengths at even distances with a jitter (seed 4242); regions that fit in no
segment of their contig are left out of BOTH modes (regions_dropped).  One JSON line:
  workspace_ms, shuffle_ms      Database.permutation_support under mode "workspace" / "shuffle", median of --reps after a warm-up
  ratio                         workspace_ms / shuffle_ms
  regions_ws_ms, regions_sh_ms  the generic entry (permute_regions) on --list-perms permutations: kernel + the lists to the host
  nseg, build_ms                segments of the table, and build_workspace on the host
  equal                         on the first 10 000 regions: the lists of --list-perms permutations and the statistics of
                                --host-perms permutations agree with the host route (permute_regions_host, permute_host)
  parent_P_ms                   the parent's recorded -P figure (circular, 10^4 regions, 1 000 permutations), for the eye
No threshold: nobody has measured two dependent binary searches per output against the walk they precede.
Usage: tools/permute_workspace_probe.py [--regions 10000] [--perms 1000] [--gaps 1000] [--out profiles/enrich/permute_workspace_probe.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import igd_amd  # noqa: E402
from igd_amd import Database, synth  # noqa: E402


def med(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def gapped_genome(ctg_len, gaps, rng, width=1000):
    """segments (ichr, a, b): every contig minus its share of `gaps` gaps of `width` bp"""
    total = float(ctg_len.astype(np.int64).sum())
    c_, a_, b_ = [], [], []
    for c, L in enumerate(int(x) for x in ctg_len):
        if L < 1:
            continue
        k = min(int(round(gaps * L / total)), max(L // (4 * width), 0))
        step = L / (k + 1)
        cuts = [int((i + 1) * step + rng.integers(-width, width + 1)) for i in range(k)]
        at = 0
        for g in cuts:
            g = min(max(g, at), L)
            c_.append(c); a_.append(at); b_.append(g)
            at = min(g + width, L)
        c_.append(c); a_.append(at); b_.append(L)
    return np.array(c_, np.int32), np.array(a_, np.int32), np.array(b_, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/igdb")
    ap.add_argument("--regions", type=int, default=10000)
    ap.add_argument("--perms", type=int, default=1000)
    ap.add_argument("--gaps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--list-perms", type=int, default=16)
    ap.add_argument("--host-perms", type=int, default=4)
    ap.add_argument("--out", default=None, help="also append the line to this file")
    a = ap.parse_args()
    path = os.path.join(a.dir, "rm1900x26316.igd")
    if not (os.path.exists(path) and os.path.exists(path + ".done")):
        os.makedirs(a.dir, exist_ok=True)
        synth.make_db(path, files=1900, per_file=26316, seed=1000, nbp_log=14, genome=synth.HG38)
        open(path + ".done", "w").write("ok")
    db = Database(path)
    ichr, qs, qe = (np.ascontiguousarray(x, np.int32) for x in synth.make_queries(a.regions, seed=999))
    ctg_len = np.array(db.ntile, np.int64) * db.nbp
    np.maximum.at(ctg_len, ichr, qe.astype(np.int64))
    ctg_len = ctg_len.astype(np.int32)
    seg = gapped_genome(ctg_len, a.gaps, np.random.default_rng(4242))
    t = time.perf_counter()
    ws = igd_amd.build_workspace(*seg, ctg_len)
    build_ms = 1e3 * (time.perf_counter() - t)
    # regions that fit nowhere leave both modes
    keep = np.ones(len(qs), bool)
    while True:
        i = ws.first_unplaceable(ichr[keep], qs[keep], qe[keep])
        if i < 0:
            break
        keep[np.flatnonzero(keep)[i]] = False
    dropped = int((~keep).sum())
    ichr, qs, qe = (np.ascontiguousarray(x[keep]) for x in (ichr, qs, qe))
    nq, P = len(qs), a.perms

    run = {"workspace": lambda: db.permutation_support(ichr, qs, qe, ctg_len, P, mode="workspace", workspace=ws),
           "shuffle": lambda: db.permutation_support(ichr, qs, qe, ctg_len, P, mode="shuffle")}
    res, ms = {}, {}
    for k, f in run.items():
        res[k] = f()                                                          # warm-up (workspaces)
        ms[k] = med(f, a.reps)
    lp = a.list_perms
    lists_ws = db.permute_regions(ichr, qs, qe, ctg_len, 0, lp, 0, "workspace", workspace=ws)
    reg_ws = med(lambda: db.permute_regions(ichr, qs, qe, ctg_len, 0, lp, 0, "workspace", workspace=ws), a.reps)
    reg_sh = med(lambda: db.permute_regions(ichr, qs, qe, ctg_len, 0, lp, 0, "shuffle"), a.reps)

    n = min(nq, 10000)
    h = igd_amd.permute_regions_host(ichr[:n], qs[:n], qe[:n], ctg_len, 0, lp, 0, "workspace", workspace=ws)
    g = lists_ws if n == nq else db.permute_regions(ichr[:n], qs[:n], qe[:n], ctg_len, 0, lp, 0, "workspace", workspace=ws)
    equal = bool(np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1]))
    hp = igd_amd.permute_host(path, ichr[:n], qs[:n], qe[:n], ctg_len, a.host_perms, 0, "workspace", workspace=ws)
    dp = db.permutation_support(ichr[:n], qs[:n], qe[:n], ctg_len, a.host_perms, 0, "workspace", workspace=ws)
    equal = equal and all(bool(np.array_equal(x, y)) for x, y in zip(hp[:7], dp[:7]))

    line = dict(regions=int(nq), regions_dropped=dropped, perms=int(P), gaps=int(a.gaps), nseg=int(ws.nseg), nfiles=int(db.nfiles),
                workspace_ms=round(ms["workspace"], 3), shuffle_ms=round(ms["shuffle"], 3), ratio=round(ms["workspace"] / ms["shuffle"], 3),
                regions_ws_ms=round(reg_ws, 3), regions_sh_ms=round(reg_sh, 3), list_perms=lp, build_ms=round(build_ms, 3), equal=equal,
                host_perms=a.host_perms, outside=ws.outside(ichr, qs, qe), parent_P_ms=11.424,
                mean_any_workspace=round(float(res["workspace"].sum[-1]) / P, 3), mean_any_shuffle=round(float(res["shuffle"].sum[-1]) / P, 3))
    s = json.dumps(line)
    print(s, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    db.close()


if __name__ == "__main__":
    main()
