"""ctypes bindings of the native libraries (built in-tree under igd_amd/lib by `make`).

Nothing here computes overlaps: every search entry point ends in libigd_hip.so (hand-written
HIP for gfx950).  If a library is missing this module raises -- there is no Python or CPU
fallback."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# IGD_AMD_LIBDIR: kernel-variant experiments (tools/ab.sh, tools/valu_ab.sh) load another build of the libraries.  Which
# build is mapped is never a guess: igd_hip_build_flags() names it, and Database() refuses one that gives wrong counts.
LIBDIR = os.environ.get("IGD_AMD_LIBDIR") or os.path.join(HERE, "lib")

i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)


class NativeMissing(RuntimeError):
    pass


def build(verbose=False):
    """Compile every native target for gfx950 (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", ROOT, "all"], stdout=out)


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP
    runtimes in one process cannot both own the GPU, so when torch is installed but not imported
    yet, map ITS runtime first; libigd_hip.so's NEEDED libamdhip64.so.7 then binds to it by
    SONAME and a later `import torch` finds its own file already mapped."""
    import sys
    if "torch" in sys.modules or os.environ.get("IGD_AMD_SYSTEM_HIP"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def _load(name):
    path = os.path.join(LIBDIR, name)
    if not os.path.exists(path):
        raise NativeMissing(
            "%s not built: run `make` (or `python -c 'import __graft_entry__ as g; g.build()'`) "
            "in %s -- igd_amd has no fallback path" % (path, ROOT))
    return C.CDLL(path)


class HipDesc(C.Structure):
    _fields_ = [("nbp", C.c_int32), ("gType", C.c_int32), ("nCtg", C.c_int32), ("nFiles", C.c_int32),
                ("nTile", i32p), ("nCnt", i32p), ("records", C.c_void_p), ("nRecords", C.c_int64),
                ("fd", C.c_int), ("fd_offset", C.c_int64)]


class HipCreateDesc(C.Structure):
    _fields_ = [("nbp", C.c_int32), ("gType", C.c_int32), ("nCtg", C.c_int32), ("n", C.c_int64),
                ("ctg", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p), ("value", C.c_void_p),
                ("file", C.c_void_p), ("ctgName", C.c_void_p), ("out_fd", C.c_int)]


class HipCreated(C.Structure):
    _fields_ = [("nTile", C.c_void_p), ("nCnt", C.c_void_p), ("nTiles", C.c_int64), ("nRecords", C.c_int64),
                ("records", C.c_void_p)]


class HipHit(C.Structure):
    _fields_ = [("q", C.c_int32), ("idx", C.c_int32), ("start", C.c_int32), ("end", C.c_int32)]


class HipStats(C.Structure):
    _fields_ = [("queries", C.c_int64), ("pairs", C.c_int64), ("S", C.c_int64), ("B", C.c_int64),
                ("H", C.c_int64)]


class CoreDb(C.Structure):
    """struct igdc_db of igd_amd/csrc/igd_core.h"""
    _fields_ = [("nbp", C.c_int32), ("gType", C.c_int32), ("nCtg", C.c_int32), ("nFiles", C.c_int32),
                ("nTile", i32p), ("nCntFlat", i32p), ("nCnt", C.POINTER(i32p)),
                ("tBase", i64p), ("reserved_", C.c_void_p),
                ("cName", C.POINTER(C.c_char_p)), ("fileName", C.POINTER(C.c_char_p)),
                ("fileNr", i32p), ("fileMd", C.POINTER(C.c_double)),
                ("nTileTotal", C.c_int64), ("nRecords", C.c_int64), ("dataOff", C.c_int64),
                ("dict", i32p), ("dictCap", C.c_int32), ("dev", C.c_void_p),
                ("ndev", C.c_int32), ("devs", C.c_void_p * 16), ("grp", C.c_void_p)]


class CoreQueries(C.Structure):
    _fields_ = [("n", C.c_int64), ("cap", C.c_int64), ("ichr", i32p), ("qs", i32p), ("qe", i32p),
                ("unsorted", C.c_int32), ("max_len", C.c_int32)]


class HipWorkspace(C.Structure):
    """struct igd_hip_workspace of include/igd_hip.h: the table of a workspace (w_off int64[nctg + 1], w_start and w_len
    int32[nseg], w_pre int32[nseg + nctg])"""
    _fields_ = [("nctg", C.c_int32), ("nseg", C.c_int64), ("w_off", C.c_void_p), ("w_start", C.c_void_p), ("w_len", C.c_void_p),
                ("w_pre", C.c_void_p)]


IGD_HIP_RULE_NEST = 0
IGD_HIP_RULE_FLAT = 1
class HipTraffic(C.Structure):
    _fields_ = [("units", C.c_int64), ("records", C.c_int64), ("record_bytes", C.c_int64), ("unit_bytes", C.c_int64),
                ("query_bytes", C.c_int64), ("slab_bytes", C.c_int64), ("total", C.c_int64)]


ENUM_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_void_p)
ENUM_SINK8 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int)

IGD_HIP_NO_VALUE_FILTER = -(2 ** 31)
IGD_HIP_FLAG_SORTED = 1
IGD_HIP_FLAG_BUCKET = 2
IGD_HIP_FLAG_EXACT = 4
IGD_HIP_FLAG_ZERO_FIRST = 8
IGD_HIP_FLAG_SHORT = 16        # with SORTED: no query is as long as a tile (verified on the device; dense batches take the DIRECT step)
IGD_HIP_ERR_UNSORTED = -4

_hip = None
_cli = None
_py = None
_synth = None
_r = None


def hip():
    """libigd_hip.so -- include/igd_hip.h"""
    global _hip
    if _hip is None:
        _share_hip_runtime_with_torch()
        L = _load("libigd_hip.so")
        L.igd_hip_device_count.restype = C.c_int
        L.igd_hip_last_error.restype = C.c_char_p
        L.igd_hip_open.argtypes = [C.POINTER(HipDesc), C.c_int, C.POINTER(C.c_void_p)]
        L.igd_hip_close.argtypes = [C.c_void_p]
        L.igd_hip_nfiles.argtypes = [C.c_void_p]
        L.igd_hip_nfiles.restype = C.c_int32
        L.igd_hip_resident_bytes.argtypes = [C.c_void_p]
        L.igd_hip_resident_bytes.restype = C.c_int64
        L.igd_hip_search.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_int32, C.c_int, C.c_void_p, i64p]
        L.igd_hip_search_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_int32, C.c_int, C.c_int, C.c_void_p, i64p]
        L.igd_hip_search_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.igd_hip_support_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_int32, C.c_int, C.c_void_p, C.c_void_p]
        # the `_ov` forms: the same arguments, then a pointer to an igd_hip_min_overlap (three int32; NULL: no threshold)
        L.igd_hip_search_sets_ov.argtypes = L.igd_hip_search_sets.argtypes + [C.c_void_p]
        L.igd_hip_support_sets_ov.argtypes = L.igd_hip_support_sets.argtypes + [C.c_void_p]
        # per group of datasets: db, ichr, qs, qe, set_off, nsets, grp_off, grp_idx, ngroups, v, rule, gsupport, gnhit, min_overlap /
        # ..., nsets, u_ichr, u_qs, u_qe, nu, grp_off, grp_idx, ngroups, v, rule, gsupport, gusupport, pvalue_log, odds_ratio,
        # clamped, gnhit, gunhit, min_overlap
        L.igd_hip_group_support_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                 C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_group_enrich_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int] + \
            [C.c_void_p] * 8
        L.igd_hip_coverage_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_int, C.c_void_p, C.c_void_p]
        L.igd_hip_member_words.argtypes = [C.c_void_p]
        L.igd_hip_member_words.restype = C.c_int64
        L.igd_hip_member_grid.argtypes = [C.c_int64]
        L.igd_hip_member_grid.restype = C.c_int32
        L.igd_hip_fisher_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.igd_hip_enrich_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # igd_hip_enrich_sets' arguments, nhit, unhit, min_overlap
        L.igd_hip_enrich_sets_ov.argtypes = L.igd_hip_enrich_sets.argtypes + [C.c_void_p] * 3
        # sets restricted to the universe: db, ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, bits, size
        L.igd_hip_restrict_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        # ..., nu, v, rule, support, usupport, size, pvalue_log, odds_ratio, bits, nhit, unhit
        L.igd_hip_enrich_restricted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
        L.igd_hip_restrict_grid.argtypes = [C.c_int64]
        L.igd_hip_restrict_grid.restype = C.c_int32
        L.igd_hip_fisher_grid.argtypes = [C.c_int64]
        L.igd_hip_fisher_grid.restype = C.c_int32
        L.igd_hip_enrich_ranks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_rank_grid.argtypes = [C.c_int64]
        L.igd_hip_rank_grid.restype = C.c_int32
        L.igd_hip_rank_lds_cols.argtypes = []
        L.igd_hip_rank_lds_cols.restype = C.c_int32
        # dataset co-occurrence: db, ichr, qs, qe, nq, v, rule, cooc, nhit
        L.igd_hip_cooccur.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int,
                                      C.c_void_p, C.c_void_p]
        # db, bits, nrows, nW, cols / db, a, m, b, n, nwords32, out
        L.igd_hip_bits_transpose.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.igd_hip_bitrows_gram.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.igd_hip_gram_tile.argtypes = []
        L.igd_hip_gram_tile.restype = C.c_int32
        L.igd_hip_gram_kstep.argtypes = []
        L.igd_hip_gram_kstep.restype = C.c_int32
        L.igd_hip_gram_slices.argtypes = [C.c_int64, C.c_int64, C.c_int64]
        L.igd_hip_gram_slices.restype = C.c_int64
        # permutation null: db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, min, max
        L.igd_hip_permute_support.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_uint64,
                                              C.c_int64, C.c_int32, C.c_int] + [C.c_void_p] * 7
        L.igd_hip_permute_support_ov.argtypes = L.igd_hip_permute_support.argtypes + [C.c_void_p]
        # db, ichr, qs, qe, nq, ctg_len, nctg, mode, seed, p0, np, out_qs, out_qe / db, rows, nrows, ncols, observed, 6 outputs
        L.igd_hip_permute_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int,
                                              C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        L.igd_hip_perm_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p] + [C.c_void_p] * 6
        L.igd_hip_permute_grid.argtypes = [C.c_int64]
        L.igd_hip_permute_grid.restype = C.c_int32
        # the same inside a workspace: the last argument is a const igd_hip_workspace * (NULL: the entry above)
        L.igd_hip_permute_support_ws.argtypes = L.igd_hip_permute_support_ov.argtypes + [C.c_void_p]
        L.igd_hip_permute_regions_ws.argtypes = L.igd_hip_permute_regions.argtypes + [C.c_void_p]
        # support under rigid shifts: db, ichr, qs, qe, nq, ctg_len, nctg, offsets, nshift, out_qs, out_qe / db, ichr, qs, qe, nq,
        # ctg_len, offsets, nshift, v, rule, shifted, min_overlap
        L.igd_hip_shift_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_int64, C.c_void_p, C.c_void_p]
        L.igd_hip_shift_support.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_int32, C.c_int, C.c_void_p, C.c_void_p]
        # the three nulls by resampling: db, ichr, qs, qe, nq, pool_ichr, pool_qs, pool_qe, npool, seed, nperm, then the entry's own
        # arguments behind nperm; the generator alone: db, pool_ichr, pool_qs, pool_qe, npool, nq, seed, p0, np, out_ichr, out_qs, out_qe
        rs = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int64]
        L.igd_hip_permute_support_rs.argtypes = rs + [C.c_int32, C.c_int] + [C.c_void_p] * 8
        L.igd_hip_permute_nearest_rs.argtypes = rs + [C.c_int32, C.c_int32] + [C.c_void_p] * 3
        L.igd_hip_permute_bp_rs.argtypes = rs + [C.c_int32, C.c_int] + [C.c_void_p] * 4
        L.igd_hip_resample_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64,
                                               C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_membership.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_membership_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # nearest record per dataset: db, ichr, qs, qe, nq, window, v, dist, dmin / ..., set_off, nsets, window, v, n_within,
        # n_overlap, sum_dist / device pointers, ..., d_dist, d_dmin, stream
        L.igd_hip_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.igd_hip_nearest_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_nearest_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
        # the signed forms: as igd_hip_nearest / igd_hip_nearest_dev; the histogram: ..., set_off, nsets, window, v, edges, ne, hist
        L.igd_hip_nearest_signed.argtypes = L.igd_hip_nearest.argtypes
        L.igd_hip_nearest_signed_dev.argtypes = L.igd_hip_nearest_dev.argtypes
        L.igd_hip_nearest_hist.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_void_p]
        # the flanks: db, ichr, qs, qe, nq, window, measure, v, up, down, upmin, downmin [, stream]; the relative-distance
        # histogram: ..., set_off, nsets, window, measure, v, nbins, hist
        L.igd_hip_flank.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_flank_dev.argtypes = L.igd_hip_flank.argtypes + [C.c_void_p]
        L.igd_hip_flank_reldist.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int,
                                            C.c_int32, C.c_int32, C.c_void_p]
        # merged region sets: db, ichr, qs, qe, set_off, nsets, gap, m_ichr, m_qs, m_qe, m_off, m_count, n_dropped / device pointers,
        # ..., nsets, n, gap, ..., stream; merged base pairs per dataset: db, v, rule, file_bp; the table: db, ichr, qs, qe, set_off,
        # nsets, v, rule, inter, set_bp, file_bp, n_merged, n_dropped
        L.igd_hip_merge_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_merge_sets_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_dataset_bp.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_void_p]
        L.igd_hip_dataset_bp_computed.argtypes = [C.c_void_p]
        L.igd_hip_dataset_bp_computed.restype = C.c_int64
        L.igd_hip_jaccard_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # the permutation null of the base-pair overlap: db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, inter, set_bp,
        # n_merged, n_dropped / pc, nq
        L.igd_hip_permute_bp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_uint64,
                                         C.c_int64, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_permute_bp_ws.argtypes = L.igd_hip_permute_bp.argtypes + [C.c_void_p]
        L.igd_hip_merge_slices_per_row.argtypes = [C.c_int64, C.c_int64]
        L.igd_hip_merge_slices_per_row.restype = C.c_int64
        # the fused route and the permutation null of the distances: as igd_hip_nearest_sets / db, ichr, qs, qe, nq, ctg_len, mode,
        # seed, nperm, window, v, n_within, n_overlap, sum_dist
        L.igd_hip_nearest_sets_fused.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_permute_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_uint64,
                                              C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_permute_nearest_ws.argtypes = L.igd_hip_permute_nearest.argtypes + [C.c_void_p]
        L.igd_hip_nearest_fused_max_files.argtypes = []
        L.igd_hip_nearest_fused_max_files.restype = C.c_int32
        L.igd_hip_nearest_fused_grid.argtypes = [C.c_int64]
        L.igd_hip_nearest_fused_grid.restype = C.c_int32
        L.igd_hip_nearest_grid.argtypes = [C.c_int64]
        L.igd_hip_nearest_grid.restype = C.c_int32
        # values of the overlapping records: db, ichr, qs, qe, nq, op, v, count, agg / ..., set_off, nsets, op, v, n_hit, pairs,
        # agg_sum / device pointers, ..., d_count, d_agg, stream
        L.igd_hip_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int32, C.c_void_p, C.c_void_p]
        L.igd_hip_map_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_map_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
        L.igd_hip_map_grid.argtypes = [C.c_int64]
        L.igd_hip_map_grid.restype = C.c_int32
        # the fused route of the values and their permutation null: as igd_hip_map_sets / db, ichr, qs, qe, nq, ctg_len, mode, seed,
        # nperm, op, v, n_hit, pairs, agg_sum [, ws] / the resampling form
        L.igd_hip_map_sets_fused.argtypes = L.igd_hip_map_sets.argtypes
        L.igd_hip_permute_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_uint64,
                                          C.c_int64, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_permute_map_ws.argtypes = L.igd_hip_permute_map.argtypes + [C.c_void_p]
        L.igd_hip_permute_map_rs.argtypes = rs + [C.c_int, C.c_int32] + [C.c_void_p] * 3
        L.igd_hip_map_fused_max_files.argtypes = [C.c_int]
        L.igd_hip_map_fused_max_files.restype = C.c_int32
        L.igd_hip_map_fused_grid.argtypes = [C.c_int64]
        L.igd_hip_map_fused_grid.restype = C.c_int32
        # the y of the reductions' grid: ncols (nFiles + 1 for the nearest family, nFiles for map), nslices
        L.igd_hip_reduce_grid_y.argtypes = [C.c_int64, C.c_int64]
        L.igd_hip_reduce_grid_y.restype = C.c_int32
        # TEST-ONLY, igd_sortscan.hpp on host arrays: device, in, n, out, total / device, keys, vals, n, bits
        L.igd_hip_test_exclusive_scan.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.igd_hip_test_radix_sort_pairs.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        L.igd_hip_search_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_search_runs_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_hip_max_batch.restype = C.c_int64
        L.igd_hip_build_flags.restype = C.c_uint
        L.igd_hip_build_wrong_counts.restype = C.c_uint
        L.igd_hip_sync.argtypes = [C.c_void_p, C.c_void_p]
        L.igd_hip_sync_spin.argtypes = [C.c_void_p, C.c_void_p]
        L.igd_hip_enumerate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.POINTER(C.POINTER(HipHit)), i64p]
        L.igd_hip_free.argtypes = [C.c_void_p]
        L.igd_hip_enumerate_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                               C.c_void_p, ENUM_SINK, C.c_void_p, i64p]
        L.igd_hip_enumerate_stream8.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                C.c_void_p, ENUM_SINK8, C.c_void_p, i64p]
        L.igd_hip_hit8_idx_bits.argtypes = [C.c_void_p]
        L.igd_hip_batch_traffic.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_int32, C.c_int, C.c_int, C.POINTER(HipTraffic)]
        L.igd_hip_measure_rates.argtypes = [C.c_int, C.POINTER(C.c_double)]
        L.igd_hip_seqpare_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
        L.igd_hip_batch_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_int32, C.c_int, C.POINTER(HipStats)]
        L.igd_hip_hitmap.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, i64p]
        L.igd_hip_profile_begin.argtypes = [C.c_void_p, C.c_int]
        L.igd_hip_profile_end.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double)]
        L.igd_hip_profile_sampling.argtypes = [C.c_void_p, C.c_int]
        L.igd_hip_scan_kernel_name.restype = C.c_char_p
        L.igd_hip_last_scan_kernel.restype = C.c_char_p
        L.igd_hip_last_scan_kernel.argtypes = [C.c_void_p]
        # TEST-ONLY: db, out int64[n], n -> words filled
        L.igd_hip_last_batch_routes.argtypes = [C.c_void_p, i64p, C.c_int]
        L.igd_hip_route_constants.argtypes = [C.c_void_p, i64p, C.c_int]
        L.igd_hip_seqpare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
        L.igd_hip_create.argtypes = [C.POINTER(HipCreateDesc), C.c_int, C.POINTER(HipCreated)]
        L.igd_hip_created_free.argtypes = [C.POINTER(HipCreated)]
        _hip = L
    return _hip


def create_arrays(nbp, gtype, nctg, ctg, start, end, value, file, device=0):
    """igd_hip_create on numpy int32 arrays -> dict(nTile, nCnt, records[nRecords, 4|3])."""
    import numpy as np
    L = hip()
    arrs = [np.ascontiguousarray(a, dtype=np.int32) if a is not None else None for a in (ctg, start, end, value, file)]
    p = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrs]
    d = HipCreateDesc(int(nbp), int(gtype), int(nctg), len(arrs[0]), p[0], p[1], p[2], p[3], p[4], None, -1)
    out = HipCreated()
    rc = L.igd_hip_create(C.byref(d), int(device), C.byref(out))
    if rc != 0:
        raise RuntimeError("igd_hip_create failed (%d): %s" % (rc, L.igd_hip_last_error().decode()))
    try:
        w = 3 if gtype == 0 else 4
        ntile = np.ctypeslib.as_array(C.cast(out.nTile, C.POINTER(C.c_int32)), (max(int(nctg), 1),))[:nctg].copy()
        ncnt = np.ctypeslib.as_array(C.cast(out.nCnt, C.POINTER(C.c_int32)), (max(int(out.nTiles), 1),))[:out.nTiles].copy()
        if out.nRecords > 0:
            recs = np.ctypeslib.as_array(C.cast(out.records, C.POINTER(C.c_int32)), (int(out.nRecords), w)).copy()
        else:
            recs = np.zeros((0, w), np.int32)
    finally:
        L.igd_hip_created_free(C.byref(out))
    return {"nTile": ntile, "nCnt": ncnt, "records": recs}


def _bind_core(L):
    L.igdc_open.restype = C.POINTER(CoreDb)
    L.igdc_open.argtypes = [C.c_char_p]
    L.igdc_index_path.restype = C.c_void_p
    L.igdc_index_path.argtypes = [C.c_char_p]
    L.igdc_load_index.argtypes = [C.POINTER(CoreDb), C.c_char_p]
    L.igdc_close.argtypes = [C.POINTER(CoreDb)]
    L.igdc_get_id.argtypes = [C.POINTER(CoreDb), C.c_char_p]
    L.igdc_get_id.restype = C.c_int32
    L.igdc_attach_path.argtypes = [C.POINTER(CoreDb), C.c_char_p, C.c_int]
    L.igdc_parse_bed.restype = C.c_void_p
    L.igdc_parse_bed.argtypes = [C.c_char_p, i32p, i32p, C.c_int]
    L.igdc_read_queries.argtypes = [C.POINTER(CoreDb), C.c_char_p, C.c_int, C.POINTER(CoreQueries)]
    L.igdc_queries_free.argtypes = [C.POINTER(CoreQueries)]
    # support counts on the host (igd_hostpath.c): db, map (igdc_map_open), ichr, qs, qe, nq, v, rule, support, nhit
    L.igdc_map_open.restype = C.c_void_p
    L.igdc_map_open.argtypes = [C.c_void_p, C.c_int]
    L.igdc_map_close.argtypes = [C.c_void_p]
    L.igdc_support_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int,
                                    C.c_void_p, C.POINTER(C.c_int64)]
    # pair counts on the host: db, map, ichr, qs, qe, nq, v, rule, hits, total; the `_ov` twins take a pointer to an
    # igd_hip_min_overlap (NULL: no threshold) after the plain function's arguments
    L.igdc_search_host.argtypes = L.igdc_support_host.argtypes
    L.igdc_search_host_ov.argtypes = L.igdc_search_host.argtypes + [C.c_void_p]
    L.igdc_support_host_ov.argtypes = L.igdc_support_host.argtypes + [C.c_void_p]
    # support per group of datasets on the host: db, map, ichr, qs, qe, nq, grp_off, grp_idx, ngroups, v, rule, gsupport, gnhit,
    # min_overlap
    L.igdc_group_support_host_ov.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
    # covered base pairs on the host: the same arguments, coverage and covered in place of support and nhit
    L.igdc_coverage_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int,
                                     C.c_void_p, C.POINTER(C.c_int64)]
    # per-query membership rows on the host: ..., rule, bits (uint32[nq, nW]), nfiles_hit (int32[nq] or NULL), nhit
    L.igdc_membership_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int,
                                       C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    # Fisher's exact test on the host: a, b, c, d (int64[ncell]), ncell, pvalue_log, odds_ratio (double[ncell], may be NULL)
    L.igdc_fisher_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    # ranks and q-values on the host: support, pvalue_log, odds_ratio ([nrows, ncols], may be NULL), nrows, ncols, qvalue_log,
    # rnk_sup, rnk_pv, rnk_or, max_rnk, mean_rnk (may be NULL)
    L.igdc_rank_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    # sets restricted to a universe on the host: ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, bits, size
    L.igdc_restrict_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_void_p, C.c_void_p]
    # db, map, the same, v, rule, support, usupport, size, pvalue_log, odds_ratio, bits, nhit, unhit
    L.igdc_enrich_restricted_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
    # dataset co-occurrence on the host: db, map, ichr, qs, qe, nq, v, rule, cooc (int64[nfiles, nfiles]), nhit
    L.igdc_cooccur_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int,
                                    C.c_void_p, C.POINTER(C.c_int64)]
    # a (uint32[m, nwords32]), m, b (uint32[n, nwords32] or NULL: symmetric), n, nwords32, out (int64[m, n])
    L.igdc_bitrows_gram_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    # permutation null on the host: ichr, qs, qe, nq, ctg_len, nctg, mode, seed, p0, np, out_qs, out_qe
    L.igdc_permute_regions_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int, C.c_uint64,
                                            C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.igdc_permute_first_bad.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]
    L.igdc_permute_first_bad.restype = C.c_int64
    # db, map, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, min, max
    L.igdc_permute_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_uint64,
                                    C.c_int64, C.c_int32, C.c_int] + [C.c_void_p] * 7
    L.igdc_permute_host_ov.argtypes = L.igdc_permute_host.argtypes + [C.c_void_p]
    # observed, sum, sumsq, n_ge, n_le, nperm, n, mean, sd, z, nlog10_p_upper, nlog10_p_lower
    L.igdc_perm_summary.argtypes = [C.c_void_p] * 5 + [C.c_int64, C.c_int64] + [C.c_void_p] * 5
    # nearest record per dataset on the host: db, map, ichr, qs, qe, nq, window, v, dist, dmin / ..., set_off, nsets, window, v,
    # n_within, n_overlap, sum_dist / n_within, sum_dist, n, mean
    L.igdc_nearest_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p]
    L.igdc_nearest_sets_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.igdc_nearest_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    # the signed rows: as igdc_nearest_host; the histogram: db, map, ichr, qs, qe, set_off, nsets, window, v, edges, ne, hist
    L.igdc_nearest_signed_host.argtypes = L.igdc_nearest_host.argtypes
    L.igdc_nearest_hist_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    # the flanks: db, map, ichr, qs, qe, nq, window, measure, v, up, down, upmin, downmin; the relative-distance histogram: db,
    # map, ichr, qs, qe, set_off, nsets, window, measure, v, nbins, hist
    L.igdc_flank_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.igdc_flank_reldist_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_int, C.c_int32, C.c_int32, C.c_void_p]
    # merged region sets and the base-pair Jaccard on the host: db, ichr, qs, qe, set_off, nsets, gap, m_ichr, m_qs, m_qe, m_off,
    # m_count, n_dropped / db, map, v, rule, file_bp / db, map, ichr, qs, qe, set_off, nsets, v, rule, inter, set_bp, file_bp,
    # n_merged, n_dropped / inter, set_bp, file_bp, nsets, ncols, jaccard, set_fraction, file_fraction
    L.igdc_merge_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.igdc_dataset_bp_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_void_p]
    L.igdc_jaccard_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.igdc_jaccard_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    # values of the overlapping records on the host: db, map, ichr, qs, qe, nq, op, v, count, agg / ..., set_off, nsets, op, v,
    # n_hit, pairs, agg_sum / n_hit, pairs, agg_sum, n, op, mean_region, mean_pair
    L.igdc_map_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int32, C.c_void_p,
                                C.c_void_p]
    L.igdc_map_sets_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
    L.igdc_map_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    # permutation null of the distances on the host: db, map, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, window, v, n_within,
    # n_overlap, sum_dist / n_within, sum_dist, nperm, ncols, the twelve outputs
    L.igdc_permute_nearest_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                            C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.igdc_perm_nearest_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 12
    # permutation null of the base-pair overlap on the host: db, map, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, inter,
    # set_bp, n_merged, n_dropped / inter, set_bp, file_bp, nperm, ncols, the fourteen outputs
    L.igdc_permute_bp_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                       C.c_uint64, C.c_int64, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.igdc_perm_bp_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 14
    # the workspace of the permutation nulls: ichr, a, b, n, ctg_len, nctg, out / table / table, ctg_len, nctg / table, ctg_len,
    # ichr, qs, qe, nq / table, ichr, qs, qe, nq / db, path, ctg_len, out; and the four host routes with the table behind them
    L.igdc_workspace_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(C.POINTER(HipWorkspace))]
    L.igdc_workspace_free.argtypes = [C.c_void_p]
    L.igdc_workspace_free.restype = None
    L.igdc_workspace_valid.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.igdc_workspace_first_unplaceable.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.igdc_workspace_first_unplaceable.restype = C.c_int64
    L.igdc_workspace_outside.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.igdc_workspace_outside.restype = C.c_int64
    L.igdc_read_workspace.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.POINTER(HipWorkspace))]
    L.igdc_permute_regions_host_ws.argtypes = L.igdc_permute_regions_host.argtypes + [C.c_void_p]
    L.igdc_permute_host_ws.argtypes = L.igdc_permute_host_ov.argtypes + [C.c_void_p]
    L.igdc_permute_nearest_host_ws.argtypes = L.igdc_permute_nearest_host.argtypes + [C.c_void_p]
    L.igdc_permute_bp_host_ws.argtypes = L.igdc_permute_bp_host.argtypes + [C.c_void_p]
    # support under rigid shifts on the host: ichr, qs, qe, nq, ctg_len, nctg, offsets, nshift, out_qs, out_qe / db, map, ichr, qs,
    # qe, nq, ctg_len, offsets, nshift, v, rule, shifted, min_overlap
    L.igdc_shift_regions_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p]
    L.igdc_shift_support_host_ov.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_int32, C.c_int, C.c_void_p, C.c_void_p]
    # the three nulls by resampling on the host: db, map, ichr, qs, qe, nq, pool_ichr, pool_qs, pool_qe, npool, seed, nperm, then the
    # entry's own arguments behind nperm; the generator alone: pool_ichr, pool_qs, pool_qe, npool, nq, seed, p0, np, out_ichr, out_qs, out_qe
    rs = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64,
          C.c_int64]
    L.igdc_permute_host_rs.argtypes = rs + [C.c_int32, C.c_int] + [C.c_void_p] * 8
    L.igdc_permute_nearest_host_rs.argtypes = rs + [C.c_int32, C.c_int32] + [C.c_void_p] * 3
    L.igdc_permute_bp_host_rs.argtypes = rs + [C.c_int32, C.c_int] + [C.c_void_p] * 4
    L.igdc_resample_regions_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.c_int64,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
    # permutation null of the values on the host: db, map, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, op, v, n_hit, pairs, agg_sum
    # [, ws] / the resampling form / n_hit, pairs, agg_sum, nperm, ncols, over_pairs, the twelve outputs
    L.igdc_permute_map_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                                        C.c_uint64, C.c_int64, C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.igdc_permute_map_host_ws.argtypes = L.igdc_permute_map_host.argtypes + [C.c_void_p]
    L.igdc_permute_map_host_rs.argtypes = rs + [C.c_int, C.c_int32] + [C.c_void_p] * 3
    L.igdc_perm_map_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int] + [C.c_void_p] * 12
    # db, path, len (int32[nCtg]), bad_line
    L.igdc_read_genome.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64)]
    return L


def cli():
    """libigd.so -- include/igd_search.h + include/igd_base.h (+ the igdc_* core)"""
    global _cli
    if _cli is None:
        hip()
        L = _bind_core(_load("libigd.so"))
        L.igd_search.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
        L.igd_engine_status.restype = C.c_int
        L.get_igdinfo.restype = C.c_void_p
        L.get_igdinfo.argtypes = [C.c_char_p]
        L.get_id.argtypes = [C.c_char_p]
        L.get_id.restype = C.c_int32
        L.parse_bed.restype = C.c_void_p
        L.parse_bed.argtypes = [C.c_char_p, i32p, i32p]
        L.bSearch.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.bSearch.restype = C.c_int32
        _cli = L
    return _cli


def pyabi():
    """libigd_py.so -- include/igd_py_abi.h"""
    global _py
    if _py is None:
        hip()
        L = _load("libigd_py.so")
        L.iGD_init.restype = C.c_void_p
        L.get_nFiles.argtypes = [C.c_void_p]
        L.get_nFiles.restype = C.c_int32
        L.open_iGD.argtypes = [C.c_void_p, C.c_char_p]
        L.close_iGD.argtypes = [C.c_void_p]
        L.create_iGD.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        L.get_overlaps.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, i64p]
        L.get_overlaps.restype = None
        L.getOverlaps.argtypes = [C.c_void_p, C.c_char_p, i64p]
        L.getOverlaps.restype = C.c_int64
        L.igd_engine_status.restype = C.c_int
        L.igd_engine_clear.restype = None
        _py = L
    return _py


def rabi():
    """libigdr.so -- include/igdr_abi.h (plain-C / .C entry points)"""
    global _r
    if _r is None:
        hip()
        L = _load("libigdr.so")
        L.open_iGD.restype = C.c_void_p
        L.open_iGD.argtypes = [C.c_char_p]
        L.close_iGD.argtypes = [C.c_void_p]
        L.get_overlaps32.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, i32p]
        L.igdr_search_n32.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), i32p, i32p, i32p]
        L.search_1.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), i32p, i32p, i64p]
        L.getOverlaps.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), i64p]
        L.igd_engine_status.restype = C.c_int
        L.igd_engine_clear.restype = None
        _r = L
    return _r


def synth():
    """libigd_synth.so -- tools/igd_synth.c"""
    global _synth
    if _synth is None:
        hip()
        L = _load("libigd_synth.so")
        L.igd_synth_db.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int,
                                   C.c_int, C.c_int32, C.c_int32, C.c_int, C.c_int]
        L.igd_synth_db_beds.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int, C.c_int,
                                        C.c_int32, C.c_int32]
        L.igd_synth_queries.argtypes = [C.c_int64, C.c_uint64, C.c_int, C.c_int32, C.c_int32, C.c_int,
                                        C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_synth_queries.restype = C.c_int64
        L.igd_synth_queries_slab.argtypes = [C.c_int64, C.c_uint64, C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_int64,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_synth_queries_slab.restype = C.c_int64
        L.igd_synth_write_bed.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.igd_synth_contig_name.restype = C.c_char_p
        L.igd_synth_contig_name.argtypes = [C.c_int, C.c_int]
        L.igd_synth_ncontigs.argtypes = [C.c_int]
        _synth = L
    return _synth


def free(ptr):
    C.CDLL(None).free(C.c_void_p(ptr))
