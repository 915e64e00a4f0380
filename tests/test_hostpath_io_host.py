"""The host route on a database whose tiles cannot be read (igd_amd/csrc/igd_hostpath.c: tile_records fails, the walk stops,
the worker reports it, the entry answers -1).  igdc_map_open checks the file's size once, at open; the file is cut to nothing
while the map holds its descriptor, so every pread of a tile comes back short.  Every entry that reads tiles is called once
with 1 and with 3 threads: each answers -1, and the entries that promise it leave the caller's outputs as they were -- the
pair, support and coverage counts (added to the caller's only if every tile could be read), the enumeration (*out stays NULL,
*total untouched) and the three permutation drivers (computed into a buffer, copied out at the end).  The rows and per-set
entries write or zero their outputs as they go: after -1 those are undefined, and nothing is asserted about them.

The same program, and the same case at its end, run under AddressSanitizer and UBSan stand-alone (tests/c/hostpath_san_main.c).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import GOLDEN, ROOT, short_tmpdir

NOV = -2 ** 31
i32, i64, u64 = C.c_int32, C.c_int64, C.c_uint64
PAT = 0x5A


def ptr(a):
    return C.c_void_p(None if a is None else a.ctypes.data)


def pat(dtype, n):
    return np.frombuffer(bytes([PAT]) * (np.dtype(dtype).itemsize * int(n)), dtype).copy()


def untouched(*arrays):
    return all(a.tobytes() == bytes([PAT]) * a.nbytes for a in arrays)


@pytest.fixture(scope="module")
def cut():
    """(library, database handle, map of a file that has been cut to nothing, number of files)"""
    L = C.CDLL(os.path.join(ROOT, "igd_amd", "lib", "libigd.so"))
    for f in ("igdc_open", "igdc_map_open", "igdc_index_path"):
        getattr(L, f).restype = C.c_void_p
    d = short_tmpdir("igio")
    path = os.path.join(d, "db.igd")
    shutil.copy(os.path.join(GOLDEN, "smallrand", "db.igd"), path)
    shutil.copy(os.path.join(GOLDEN, "smallrand", "db_index.tsv"), os.path.join(d, "db_index.tsv"))
    db = L.igdc_open(path.encode())
    assert db
    tsv = L.igdc_index_path(path.encode())
    assert L.igdc_load_index(C.c_void_p(db), C.c_void_p(tsv)) == 0
    fd = os.open(path, os.O_RDONLY)
    m = L.igdc_map_open(C.c_void_p(db), fd)
    os.close(fd)
    assert m
    nf = sum(1 for _ in open(os.path.join(d, "db_index.tsv"))) - 1
    # while the file is whole the same call answers: the -1 below is the cut's doing, not an argument's
    ichr, qs, qe = regions()
    hits = np.zeros(nf, np.int64)
    tot = i64(0)
    assert L.igdc_search_host(C.c_void_p(db), C.c_void_p(m), ptr(ichr), ptr(qs), ptr(qe), i64(len(qs)), i32(NOV), i32(0), ptr(hits), C.byref(tot)) == 0
    assert tot.value > 0 and hits.sum() == tot.value
    os.truncate(path, 0)
    yield L, C.c_void_p(db), C.c_void_p(m), nf
    L.igdc_map_close(C.c_void_p(m))
    L.igdc_close(C.c_void_p(db))
    shutil.rmtree(d, ignore_errors=True)


LEN = 1 << 30


def regions(n=6000):
    """whole contigs, again and again: every thread's share meets a tile with records (6000 regions: three threads' worth)"""
    ichr = (np.arange(n) % 8).astype(np.int32)
    return ichr, np.zeros(n, np.int32), np.full(n, LEN, np.int32)


@pytest.mark.parametrize("threads", ["1", "3"])
def test_every_entry_answers_minus_one_when_tiles_cannot_be_read(cut, threads, monkeypatch):
    L, db, m, nf = cut
    monkeypatch.setenv("IGD_HOST_THREADS", threads)
    ichr, qs, qe = regions()
    nq, nC, nW = len(qs), nf + 1, (nf + 31) // 32
    q = (db, m, ptr(ichr), ptr(qs), ptr(qe))
    set_off = np.array([0, 0, 2500, 2500, nq, nq], np.int64)
    nsets = len(set_off) - 1
    s = q + (ptr(set_off), i32(nsets))
    mo = np.array([1, 0, 0], np.int32)
    ctg_len = np.full(64, LEN, np.int32)
    edges = np.array([-10, 0, 10], np.int32)

    # the counts: -1 and nothing added
    for name, extra in (("igdc_search_host", ()), ("igdc_search_host_ov", (ptr(mo),)), ("igdc_support_host", ()), ("igdc_support_host_ov", (ptr(mo),)),
                        ("igdc_coverage_host", ())):
        for rule in (0, 1):
            vec, tot = pat(np.int64, nf), pat(np.int64, 1)
            assert getattr(L, name)(*q, i64(nq), i32(NOV), i32(rule), ptr(vec), ptr(tot), *extra) == -1, name
            assert untouched(vec, tot), name

    # the enumeration: -1, no list, *total as it was
    qoff, tot, out = pat(np.int64, nq + 1), pat(np.int64, 1), C.c_void_p(12345)
    assert L.igdc_enumerate_host(*q, i64(nq), ptr(qoff), C.byref(out), ptr(tot)) == -1
    assert out.value is None and untouched(tot)

    # the permutation drivers: -1 and nothing written (2 permutations of 2100 regions: two threads' worth where there are threads)
    n, nperm = 2100, 2
    g = q + (i64(n), ptr(ctg_len), i32(1), u64(7), i64(nperm))
    seven = [pat(np.int64, nC) for _ in range(7)]
    assert L.igdc_permute_host(*g, i32(NOV), i32(0), *[ptr(a) for a in seven]) == -1
    assert L.igdc_permute_host_ov(*g, i32(NOV), i32(1), *[ptr(a) for a in seven], ptr(mo)) == -1
    assert L.igdc_permute_host_ws(*g, i32(NOV), i32(0), *[ptr(a) for a in seven], None, None) == -1
    assert untouched(*seven)
    three = [pat(np.int64, (nperm + 1) * nC) for _ in range(3)]
    assert L.igdc_permute_nearest_host(*g, i32(0), i32(NOV), *[ptr(a) for a in three]) == -1
    assert L.igdc_permute_nearest_host_ws(*g, i32(100), i32(NOV), *[ptr(a) for a in three], None) == -1
    assert untouched(*three)
    four = [pat(np.int64, (nperm + 1) * nC), pat(np.int64, nperm + 1), pat(np.int64, nperm + 1), pat(np.int64, 1)]
    assert L.igdc_permute_bp_host(*g, i32(NOV), i32(0), *[ptr(a) for a in four]) == -1
    assert L.igdc_permute_bp_host_ws(*g, i32(NOV), i32(1), *[ptr(a) for a in four], None) == -1
    assert untouched(*four)

    # rows and per-set statistics: -1 (their outputs are undefined after it)
    r32 = [pat(np.int32, nq * max(nf, nW)) for _ in range(2)]
    m32 = [pat(np.int32, nq) for _ in range(2)]
    r64 = [pat(np.int64, nq * nf)]
    st = [pat(np.int64, nsets * 16 * nC) for _ in range(3)]
    one = pat(np.int64, 1)
    assert L.igdc_membership_host(*q, i64(nq), i32(NOV), i32(0), ptr(r32[0]), ptr(m32[0]), ptr(one)) == -1
    assert L.igdc_cooccur_host(*q, i64(nq), i32(NOV), i32(0), ptr(pat(np.int64, nf * nf)), ptr(one)) == -1
    assert L.igdc_nearest_host(*q, i64(nq), i32(0), i32(NOV), ptr(r32[0]), ptr(m32[0])) == -1
    assert L.igdc_nearest_signed_host(*q, i64(nq), i32(50), i32(NOV), ptr(r32[0]), ptr(m32[0])) == -1
    assert L.igdc_flank_host(*q, i64(nq), i32(50), i32(0), i32(NOV), ptr(r32[0]), ptr(r32[1]), ptr(m32[0]), ptr(m32[1])) == -1
    assert L.igdc_map_host(*q, i64(nq), i32(1), i32(NOV), ptr(r32[0]), ptr(r64[0])) == -1
    assert L.igdc_nearest_sets_host(*s, i32(0), i32(NOV), ptr(st[0]), ptr(st[1]), ptr(st[2])) == -1
    assert L.igdc_nearest_hist_host(*s, i32(0), i32(NOV), ptr(edges), i32(len(edges)), ptr(st[0])) == -1
    assert L.igdc_flank_reldist_host(*s, i32(50), i32(1), i32(NOV), i32(10), ptr(st[0])) == -1
    assert L.igdc_map_sets_host(*s, i32(0), i32(NOV), ptr(st[0]), ptr(st[1]), ptr(st[2])) == -1
    assert L.igdc_dataset_bp_host(db, m, i32(NOV), i32(0), ptr(pat(np.int64, nC))) == -1
    assert L.igdc_jaccard_host(*s, i32(NOV), i32(0), ptr(st[0]), ptr(pat(np.int64, nsets)), ptr(pat(np.int64, nC)), ptr(pat(np.int64, nsets)),
                               ptr(pat(np.int64, nsets))) == -1
    u = nq
    assert L.igdc_enrich_restricted_host(*s, ptr(ichr), ptr(qs), ptr(qe), i64(u), i32(NOV), i32(0), ptr(st[0]), ptr(pat(np.int64, nf)),
                                         ptr(pat(np.int64, nsets)), ptr(pat(np.float64, nsets * nf)), None, None, None, None) == -1


SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


def test_host_entries_clean_under_sanitizers_one_and_five_threads():
    """tests/c/hostpath_san_main.c -- every host entry once on a golden database, a short run of each permutation driver, and at
    the end the cut file of the test above -- compiled stand-alone with the host route under ASan + UBSan (leaks included: the
    workers' tile buffers and private vectors are freed on the failure path too); no engine library, nothing loaded into Python.
    Both thread counts print the same digest."""
    d = short_tmpdir("igsh")
    try:
        exe = os.path.join(d, "hostpath_san")
        subprocess.check_call(["gcc", "-std=gnu99", *SAN, "-Iinclude", "-Iigd_amd/csrc", "-o", exe, "tests/c/hostpath_san_main.c",
                               "igd_amd/csrc/igd_core.c", "igd_amd/csrc/igd_hostpath.c", "igd_amd/csrc/igd_hip_lazy.c", "-lz", "-lm", "-lpthread", "-ldl"],
                              cwd=ROOT)
        db = os.path.join(d, "db.igd")
        outs = []
        for threads in ("1", "5"):
            shutil.copy(os.path.join(GOLDEN, "smallrand", "db.igd"), db)
            shutil.copy(os.path.join(GOLDEN, "smallrand", "db_index.tsv"), os.path.join(d, "db_index.tsv"))
            p = subprocess.run([exe, db], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(SAN_ENV, IGD_HOST_THREADS=threads), timeout=600)
            err = p.stderr.decode(errors="replace")
            assert "Sanitizer" not in err and "runtime error" not in err and p.returncode == 0, (p.returncode, err[-3000:])
            outs.append(p.stdout)
        assert outs[0] == outs[1] and outs[0].startswith(b"hostpath_san ok")
    finally:
        shutil.rmtree(d, ignore_errors=True)
