"""Python face of one .igd resident on one MI355X.

Mirrors what the reference's front-ends do around the hot path -- load header + index
(get_igdinfo / get_fileinfo), map contig names (get_id), read query files (parse_bed loop) --
and hands every search to the HIP engine (include/igd_hip.h).  numpy arrays for host
batches; raw device pointers (e.g. torch tensors' data_ptr()) for resident batches."""
import collections
import ctypes as C
import os

import numpy as np

from . import _native as N


class IgdError(RuntimeError):
    pass


def _chk(rc, what):
    if rc != 0:
        raise IgdError("%s failed (code %d): %s" % (what, rc, N.hip().igd_hip_last_error().decode()))


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a):
    return a.ctypes.data if a.size else None


# ---- the arguments every entry takes: regions, sets, dispatch, a caller's output arrays, a seed, the contig lengths ---------
def _regions(ichr, qs, qe, what=None, noun="regions", ok=True):
    """(ichr, qs, qe) as C-ordered int32.  With `what`: three arrays of one length (and whatever else `ok` stands for), or
    IgdError; without it nothing is compared -- search(), the enumerations and the set entries, which speak for themselves."""
    ichr, qs, qe = _i32(ichr), _i32(qs), _i32(qe)
    if what and (len(ichr) != len(qs) or len(qe) != len(qs) or not ok):
        raise IgdError("%s: %d / %d / %d %s given" % (what, len(ichr), len(qs), len(qe), noun))
    return ichr, qs, qe


def _sets(ichr, qs, qe, set_off, what, noun="regions", universe=None):
    """(ichr, qs, qe, set_off int64[nsets + 1], nsets) of concatenated sets whose last offset is the number of regions.
    universe: the three lengths of a universe's arrays, which then have to agree too (_restrict_args)."""
    ichr, qs, qe = _regions(ichr, qs, qe)
    set_off = np.ascontiguousarray(set_off, dtype=np.int64)
    if len(set_off) < 1:
        raise IgdError("%s: set_off needs nsets + 1 entries" % what)
    if set_off[-1] != len(qs) or len(ichr) != len(qs) or len(qe) != len(qs) or (universe and len(set(universe)) != 1):
        given = "%d / %d / %d %s" % (len(ichr), len(qs), len(qe), noun)
        if universe:
            given += " and %d / %d / %d universe regions" % universe
        raise IgdError("%s: set_off[-1] = %d, but %s given" % (what, set_off[-1], given))
    return ichr, qs, qe, set_off, len(set_off) - 1


def _value_filter(value_filter):
    return N.IGD_HIP_NO_VALUE_FILTER if value_filter is None else int(value_filter)


def _dispatch(gtype, v, rule, value_filter):
    """(rule, engine v): the command line's choice for `-v v` unless the caller names a rule"""
    if rule is None:
        return Database.cli_dispatch(gtype, v)
    return rule, _value_filter(value_filter)


def _wrong_out(what, name, words, dtype, shape):
    return IgdError("%s: %s must be %s %s[%s]" % (what, name, words, np.dtype(dtype).name, ", ".join("%d" % n for n in shape)))


def _out(arr, shape, dtype, name, what, zero=False, words="a C-ordered"):
    """the caller's output array after its dtype, shape and order are checked, or a new one (zeroed where the entry adds)"""
    if arr is None:
        return (np.zeros if zero else np.empty)(shape, dtype)
    if arr.dtype != dtype or arr.shape != shape or not arr.flags.c_contiguous:
        raise _wrong_out(what, name, words, dtype, shape)
    return arr


def _outs(out, count, shape, what):
    """`count` C-ordered int64 arrays of `shape`: the caller's list (overwritten) or new ones"""
    if out is None:
        return [np.empty(shape, np.int64) for _ in range(count)]
    words = {3: "three", 6: "six"}[count] + " C-ordered"
    if len(out) != count:
        raise _wrong_out(what, "out", words, np.int64, shape)
    return [_out(a, shape, np.int64, "out", what, words=words) for a in out]


def _seed(seed):
    return int(seed) & (2 ** 64 - 1)


def _ctg_len_matches(ctg_len, nctg, what):
    if len(ctg_len) != nctg:
        raise IgdError("%s: ctg_len has %d entries, the database %d contigs" % (what, len(ctg_len), nctg))


def _open_core(igd_path):
    """header and index of a .igd: an igdc_db the caller closes with igdc_close"""
    L = N.cli()
    core = L.igdc_open(igd_path.encode())
    if not core:
        raise IgdError("cannot read .igd header of %s" % igd_path)
    tsv = L.igdc_index_path(igd_path.encode())
    rc = L.igdc_load_index(core, C.cast(tsv, C.c_char_p))
    N.free(tsv)
    if rc != 0:
        L.igdc_close(core)
        raise IgdError("cannot read the _index.tsv next to %s" % igd_path)
    return core


Enrichment = collections.namedtuple("Enrichment", "support usupport b c d pvalue_log odds_ratio clamped")
RestrictedEnrichment = collections.namedtuple("RestrictedEnrichment", "support usupport b c d pvalue_log odds_ratio size bits")
EnrichmentRanks = collections.namedtuple("EnrichmentRanks", "qvalue_log rnk_sup rnk_pv rnk_or max_rnk mean_rnk")
PermutationSupport = collections.namedtuple("PermutationSupport", "observed sum sumsq n_ge n_le min max nperm")
PermutationSummary = collections.namedtuple("PermutationSummary", "mean sd z nlog10_p_upper nlog10_p_lower")
PERM_MODES = {"circular": 0, "shuffle": 1}           # IGD_HIP_PERM_CIRCULAR, IGD_HIP_PERM_SHUFFLE
PERM_WORKSPACE = 2                                   # IGD_HIP_PERM_WORKSPACE: mode="workspace" together with workspace=
NearestSets = collections.namedtuple("NearestSets", "n_within n_overlap sum_dist window")
PermutationNearest = collections.namedtuple("PermutationNearest", "n_within n_overlap sum_dist window nperm")
MapSets = collections.namedtuple("MapSets", "n_hit pairs agg_sum op")
MAP_OPS = {"count": 0, "sum": 1, "min": 2, "max": 3}             # IGD_HIP_MAP_COUNT, _SUM, _MIN, _MAX
PermutationMap = collections.namedtuple("PermutationMap", "n_hit pairs agg_sum op nperm")
PermutationMapSummary = collections.namedtuple(
    "PermutationMapSummary", "observed_n_hit observed n_def mean sd z n_ge n_le nlog10_p_upper nlog10_p_lower nhit_mean nhit_sd nhit_z")
PermutationBp = collections.namedtuple("PermutationBp", "inter set_bp n_merged n_dropped file_bp nperm")
PermutationBpSummary = collections.namedtuple(
    "PermutationBpSummary", "observed mean sd z fold n_ge n_le nlog10_p_upper nlog10_p_lower jaccard jaccard_mean jaccard_sd jaccard_n_def "
    "jaccard_n_ge")
PermutationNearestSummary = collections.namedtuple(
    "PermutationNearestSummary", "within_mean within_sd within_z within_n_ge nlog10_p_within_upper mean_dist dist_mean dist_sd dist_z n_def "
    "dist_n_le nlog10_p_dist_lower")
NEAREST_MAX_WINDOW = 1 << 30                         # IGD_HIP_NEAREST_MAX_WINDOW
NEAREST_NO_RECORD = -2 ** 31                         # IGD_HIP_NEAREST_NO_RECORD: a signed distance where there is no record
NEAREST_MAX_EDGES = 63                               # IGD_HIP_NEAREST_MAX_EDGES
NearestHist = collections.namedtuple("NearestHist", "hist edges window")
FLANK_EDGES = 0                                      # IGD_HIP_FLANK_EDGES
FLANK_MIDPOINTS = 1                                  # IGD_HIP_FLANK_MIDPOINTS
FLANK_MAX_BINS = 64                                  # IGD_HIP_FLANK_MAX_BINS
FlankReldist = collections.namedtuple("FlankReldist", "hist nbins window measure")
JaccardSets = collections.namedtuple("JaccardSets", "inter set_bp file_bp n_merged n_dropped")
MERGE_MAX_GAP = 1 << 30


class MinOverlap(C.Structure):
    """A minimum overlap per (query region, record) pair -- igd_hip_min_overlap of include/igd_hip.h: LOLA's minOverlap,
    GenomicRanges' minoverlap, bedtools' -f / -F.  A pair the search counts keeps counting only if its overlap
    ov = min(qe, end) - max(qs, start) has ov >= max(bp, 1), ov * 10^6 >= (qe - qs) * query_ppm and
    ov * 10^6 >= (end - start) * record_ppm (integers; equality qualifies).  The fractions are parts per million, 0 .. 10^6;
    from_fractions() takes them as numbers in [0, 1].  All three zero is no threshold at all.  With any of them set a
    zero-length or inverted query (qe <= qs) is never counted -- the plain search counts one under a record that spans it.
    Accepted as `min_overlap=` by search_sets, support_sets, enrichment_sets, permutation_support, their one-set and file
    forms and the host functions; a bare int there means MinOverlap(bp=that)."""
    _fields_ = [("bp", C.c_int32), ("query_ppm", C.c_int32), ("record_ppm", C.c_int32)]
    PPM = 1000000

    def __init__(self, bp=0, query_ppm=0, record_ppm=0):
        for name, x, hi in (("bp", bp, 2 ** 31 - 1), ("query_ppm", query_ppm, self.PPM), ("record_ppm", record_ppm, self.PPM)):
            if isinstance(x, bool) or int(x) != x or not 0 <= int(x) <= hi:
                raise IgdError("MinOverlap: %s = %r, not an integer in 0 .. %d" % (name, x, hi))
        super().__init__(int(bp), int(query_ppm), int(record_ppm))

    @classmethod
    def from_fractions(cls, bp=0, query=0.0, record=0.0):
        """bp and the two fractions as numbers in [0, 1], rounded to the nearest part per million"""
        for name, x in (("query", query), ("record", record)):
            if not 0 <= x <= 1:                                   # (NaN fails both comparisons)
                raise IgdError("MinOverlap.from_fractions: %s = %r, not in [0, 1]" % (name, x))
        return cls(bp, int(round(query * cls.PPM)), int(round(record * cls.PPM)))

    @property
    def active(self):
        return bool(self.bp or self.query_ppm or self.record_ppm)

    def __repr__(self):
        return "MinOverlap(bp=%d, query_ppm=%d, record_ppm=%d)" % (self.bp, self.query_ppm, self.record_ppm)


def _min_overlap(mo, what):
    """None (no `_ov` call at all), or a MinOverlap from a MinOverlap or a bare int of base pairs"""
    if mo is None or isinstance(mo, MinOverlap):
        return mo
    if isinstance(mo, (int, np.integer)) and not isinstance(mo, bool):
        return MinOverlap(bp=int(mo))
    raise IgdError("%s: min_overlap must be None, an int (base pairs) or a MinOverlap, not %r" % (what, mo))


def _tables(a, b, c, d, what):
    t = [np.ascontiguousarray(x, dtype=np.int64) for x in (a, b, c, d)]
    if any(x.ndim != 1 or len(x) != len(t[0]) for x in t):
        raise IgdError("%s: a, b, c, d must be four one-dimensional arrays of one length" % what)
    return t


def fisher_host(a, b, c, d):
    """Fisher's exact test of the tables a b / c d on the host (igdc_fisher_host; no device is touched): (pvalue_log,
    odds_ratio), two float64 arrays, as Database.fisher() defines them."""
    a, b, c, d = _tables(a, b, c, d, "fisher_host")
    n = len(a)
    p, o = np.empty(n, np.float64), np.empty(n, np.float64)
    if N.cli().igdc_fisher_host(_ptr(a), _ptr(b), _ptr(c), _ptr(d), n, _ptr(p), _ptr(o)) != 0:
        raise IgdError("fisher_host: a table has a negative entry or N >= 2^31")
    return p, o


def _rank_inputs(support, pvalue_log, odds_ratio, what):
    if pvalue_log is None and odds_ratio is None and isinstance(support, (Enrichment, RestrictedEnrichment)):
        support, pvalue_log, odds_ratio = support.support, support.pvalue_log, support.odds_ratio
    if pvalue_log is None or odds_ratio is None:
        raise IgdError("%s: give support, pvalue_log and odds_ratio, or one Enrichment / RestrictedEnrichment" % what)
    s = np.ascontiguousarray(support, dtype=np.int64)
    p = np.ascontiguousarray(pvalue_log, dtype=np.float64)
    o = np.ascontiguousarray(odds_ratio, dtype=np.float64)
    if s.ndim != 2 or p.shape != s.shape or o.shape != s.shape:
        raise IgdError("%s: support, pvalue_log and odds_ratio must be three two-dimensional arrays of one shape" % what)
    return s, p, o


def _rank_outputs(shape):
    return EnrichmentRanks(np.empty(shape, np.float64), np.empty(shape, np.int32), np.empty(shape, np.int32),
                           np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape, np.float64))


def rank_host(support, pvalue_log=None, odds_ratio=None):
    """Rank columns and Benjamini-Hochberg q-values of an enrichment table on the host (igdc_rank_host; no device is
    touched): EnrichmentRanks as Database.enrichment_ranks() defines it, from three [nsets, ncols] arrays or one Enrichment."""
    s, p, o = _rank_inputs(support, pvalue_log, odds_ratio, "rank_host")
    r = _rank_outputs(s.shape)
    if N.cli().igdc_rank_host(_ptr(s), _ptr(p), _ptr(o), s.shape[0], s.shape[1], *[_ptr(x) for x in r]) != 0:
        raise IgdError("rank_host: more than 2^20 columns, or a pvalue_log is negative or NaN")
    return r


def _restrict_args(ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, what):
    u_ichr, u_qs, u_qe = _regions(u_ichr, u_qs, u_qe)
    ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, what, "queries", (len(u_ichr), len(u_qs), len(u_qe)))
    return ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, nsets, len(u_qs)


def _restricted_result(sup, usup, size, plog, odds, bits, nu):
    b = usup[None, :] - sup
    c = size[:, None] - sup
    d = nu - usup[None, :] - c
    return RestrictedEnrichment(sup, usup, b, c, d, plog, odds, size, bits)


def restrict_host(ichr, qs, qe, set_off, u_ichr, u_qs, u_qe):
    """Query sets restricted to a universe on the host (igdc_restrict_host; no device and no database is touched): (bits
    uint32[nsets, ceil(nu / 32)], size int64[nsets]) as Database.restrict_sets() defines them."""
    ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, nsets, nu = _restrict_args(ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, "restrict_host")
    bits, size = np.empty((nsets, (nu + 31) // 32), np.uint32), np.empty(max(nsets, 1), np.int64)
    if N.cli().igdc_restrict_host(_ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, _ptr(u_ichr), _ptr(u_qs), _ptr(u_qe), nu,
                                  _ptr(bits), _ptr(size)) != 0:
        raise IgdError("restrict_host: set_off is not monotone from 0, or the universe holds 2^31 - 1 regions or more")
    return bits, size[:nsets]


def enrich_restricted_host(igd_path, ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, v=0, rule=None, value_filter=None, with_nhit=False):
    """Enrichment of the restricted sets on the host (igdc_enrich_restricted_host: pread on the .igd; no device is touched):
    RestrictedEnrichment as Database.enrichment_restricted() defines it; with_nhit adds (nhit int64[nsets], unhit)."""
    ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, nsets, nu = _restrict_args(ichr, qs, qe, set_off, u_ichr, u_qs, u_qe,
                                                                          "enrich_restricted_host")
    with _HostDb(igd_path, None) as h:
        nf = h.nfiles
        rule, vf = h.dispatch(v, rule, value_filter)
        sup, usup = np.empty((nsets, nf), np.int64), np.empty(max(nf, 1), np.int64)
        plog, odds = np.empty((nsets, nf), np.float64), np.empty((nsets, nf), np.float64)
        size, nhit, unhit = np.empty(max(nsets, 1), np.int64), np.empty(max(nsets, 1), np.int64), C.c_int64(0)
        bits = np.empty((nsets, (nu + 31) // 32), np.uint32)
        if h.L.igdc_enrich_restricted_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, _ptr(u_ichr), _ptr(u_qs),
                                           _ptr(u_qe), nu, vf, rule, _ptr(sup), _ptr(usup), _ptr(size), _ptr(plog), _ptr(odds), _ptr(bits),
                                           _ptr(nhit), C.byref(unhit)) != 0:
            raise IgdError("enrich_restricted_host: bad set_off or universe, or a tile of %s could not be read" % igd_path)
    res = _restricted_result(sup, usup[:nf], size[:nsets], plog, odds, bits, nu)
    return (res, nhit[:nsets], unhit.value) if with_nhit else res


def _bitrows(x, name, what):
    x = np.ascontiguousarray(x, dtype=np.uint32)
    if x.ndim != 2:
        raise IgdError("%s: %s must be a two-dimensional uint32 array of bit rows" % (what, name))
    return x


def bitrows_gram_host(a, b=None):
    """Popcount Gram product of bit rows on the host (igdc_bitrows_gram_host; no device is touched): int64[m, n] with
    out[i, j] = popcount(a[i] & b[j]) as Database.bitrows_gram() defines it; b=None is the symmetric form."""
    a = _bitrows(a, "a", "bitrows_gram_host")
    b = None if b is None else _bitrows(b, "b", "bitrows_gram_host")
    if b is not None and b.shape[1] != a.shape[1]:
        raise IgdError("bitrows_gram_host: rows of %d and of %d words" % (a.shape[1], b.shape[1]))
    m, n = a.shape[0], a.shape[0] if b is None else b.shape[0]
    out = np.empty((m, n), np.int64)
    if N.cli().igdc_bitrows_gram_host(_ptr(a), m, None if b is None else (b.ctypes.data if b.size else a.ctypes.data), n, a.shape[1],
                                      _ptr(out)) != 0:
        raise IgdError("bitrows_gram_host: more than 2^28 cells")
    return out


def jaccard(cooc):
    """Jaccard index of a co-occurrence matrix (pure numpy): J[f, g] = cooc[f, g] / (cooc[f, f] + cooc[g, g] - cooc[f, g]) in
    float64, NaN where the denominator is 0."""
    c = np.asarray(cooc)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise IgdError("jaccard: cooc must be a square matrix")
    d = np.diagonal(c)
    den = (d[:, None] + d[None, :] - c).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, np.nan, c.astype(np.float64) / den)


def cooccur_host(igd_path, ichr, qs, qe, v=0, rule=None, value_filter=None):
    """Dataset co-occurrence over a region list on the host (igdc_cooccur_host: pread on the .igd; no device is touched):
    (cooc int64[nfiles, nfiles], nhit) as Database.cooccurrence() defines them."""
    ichr, qs, qe = _regions(ichr, qs, qe, "cooccur_host")
    with _HostDb(igd_path, None) as h:
        rule, vf = h.dispatch(v, rule, value_filter)
        cooc, nhit = np.empty((h.nfiles, h.nfiles), np.int64), C.c_int64(0)
        if h.L.igdc_cooccur_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), vf, rule, _ptr(cooc), C.byref(nhit)) != 0:
            raise IgdError("cooccur_host: more than 16384 files, or a tile of %s could not be read" % igd_path)
    return cooc, nhit.value


class _HostDb:
    """header, index and tile reader of a .igd for the igdc_*_host functions (no device is touched)"""

    def __init__(self, igd_path, what):
        """what: the entry's name in front of "cannot map"; None for the three oldest entries, which say it without one"""
        self.L = L = N.cli()
        self.core = _open_core(igd_path)
        self.m = None
        try:
            fd = os.open(igd_path, os.O_RDONLY)
            try:
                self.m = L.igdc_map_open(self.core, fd)
            finally:
                os.close(fd)
            if not self.m:
                raise IgdError("%scannot map %s" % ("%s: " % what if what else "", igd_path))
        except Exception:
            self.close()
            raise
        self.nfiles, self.gtype, self.nctg = self.core.contents.nFiles, self.core.contents.gType, self.core.contents.nCtg

    def dispatch(self, v, rule, value_filter):
        return _dispatch(self.gtype, v, rule, value_filter)

    def close(self):
        if self.m:
            self.L.igdc_map_close(self.m)
        self.L.igdc_close(self.core)
        self.m = self.core = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def search_host(igd_path, ichr, qs, qe, v=0, rule=None, value_filter=None, min_overlap=None):
    """Pair counts of one query set on the host (igdc_search_host / igdc_search_host_ov: pread on the .igd, threads over the
    queries; no device is touched): (hits int64[nfiles], total) as Database.search() defines them, under min_overlap
    (MinOverlap, or an int of base pairs) as Database.search_sets() does."""
    ichr, qs, qe = _regions(ichr, qs, qe)
    mo = _min_overlap(min_overlap, "search_host")
    with _HostDb(igd_path, "search_host") as h:
        rule, vf = h.dispatch(v, rule, value_filter)
        hits, total = np.zeros(max(h.nfiles, 1), np.int64), C.c_int64(0)
        a = (h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), vf, rule, _ptr(hits), C.byref(total))
        if (h.L.igdc_search_host(*a) if mo is None else h.L.igdc_search_host_ov(*a, C.byref(mo))) != 0:
            raise IgdError("search_host: a tile of %s could not be read" % igd_path)
        return hits[:h.nfiles], total.value


def support_host(igd_path, ichr, qs, qe, v=0, rule=None, value_filter=None, min_overlap=None):
    """Support counts of one query set on the host (igdc_support_host / igdc_support_host_ov; no device is touched):
    (support int64[nfiles], nhit) as Database.support() defines them, min_overlap included."""
    ichr, qs, qe = _regions(ichr, qs, qe)
    mo = _min_overlap(min_overlap, "support_host")
    with _HostDb(igd_path, "support_host") as h:
        rule, vf = h.dispatch(v, rule, value_filter)
        sup, nhit = np.zeros(max(h.nfiles, 1), np.int64), C.c_int64(0)
        a = (h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), vf, rule, _ptr(sup), C.byref(nhit))
        if (h.L.igdc_support_host(*a) if mo is None else h.L.igdc_support_host_ov(*a, C.byref(mo))) != 0:
            raise IgdError("support_host: a tile of %s could not be read" % igd_path)
        return sup[:h.nfiles], nhit.value


GROUP_MAX = 8192                                     # IGD_HIP_GROUP_MAX: groups of one grouping (the kernel's LDS budget)


class DatasetGroups:
    """A grouping of a database's datasets (include/igd_hip.h: DATASET GROUPS), a many-to-many relation in CSR form: dataset f is
    in the groups idx[off[f]:off[f + 1]] (int32, ascending, each in [0, ngroups)), names[g] is group g's name.  A dataset may be
    in no group, in one or in several; a group may be empty.  Anything else -- offsets that do not start at 0 or decrease, an
    index out of range, a run that does not ascend, no group or more than GROUP_MAX -- raises IgdError naming the first bad
    entry.  build_groups() and Database.read_groups() make one from labels / from a file."""

    def __init__(self, off, idx, names, check=True):
        self.off, self.idx, self.names = _i32(off), _i32(idx), [str(n) for n in names]
        self.nfiles, self.ngroups = len(self.off) - 1, len(self.names)
        if check:
            self.check("DatasetGroups")

    def check(self, what):
        off, idx, ng = self.off, self.idx, self.ngroups
        if not 0 < ng <= GROUP_MAX:
            raise IgdError("%s: %d groups given, 1 .. %d are possible" % (what, ng, GROUP_MAX))
        if self.nfiles < 0 or off[0] != 0:
            raise IgdError("%s: off[0] = %s: the offsets start at 0 and do not decrease" % (what, off[0] if len(off) else "missing"))
        down = np.flatnonzero(np.diff(off) < 0)
        if len(down):
            raise IgdError("%s: off[%d] = %d: the offsets start at 0 and do not decrease" % (what, down[0] + 1, off[down[0] + 1]))
        if off[-1] != len(idx):
            raise IgdError("%s: off[-1] = %d, but %d indices given" % (what, off[-1], len(idx)))
        for j in np.flatnonzero((idx < 0) | (idx >= ng))[:1]:
            raise IgdError("%s: idx[%d] = %d is not in [0, %d)" % (what, j, idx[j], ng))
        first = np.zeros(len(idx), bool)
        first[off[:-1][off[:-1] < len(idx)]] = True
        for j in np.flatnonzero(~first[1:] & (idx[1:] <= idx[:-1]))[:1] + 1:
            raise IgdError("%s: idx[%d] = %d does not ascend within its dataset's run" % (what, j, idx[j]))

    def dense(self):
        """bool[nfiles, ngroups]: dataset f is in group g"""
        m = np.zeros((self.nfiles, self.ngroups), bool)
        m[np.repeat(np.arange(self.nfiles), np.diff(self.off)), self.idx] = True
        return m

    @property
    def n_datasets(self):
        """int64[ngroups]: the datasets of each group"""
        return np.bincount(self.idx, minlength=self.ngroups).astype(np.int64)

    def labels(self):
        """the group names of each dataset, a list of nfiles lists -- what build_groups() takes"""
        return [[self.names[g] for g in self.idx[self.off[f]:self.off[f + 1]]] for f in range(self.nfiles)]


def build_groups(labels, nfiles):
    """DatasetGroups from labels: a list of nfiles lists of group names (dataset f's), or a dict dataset number -> names.  Groups
    are numbered in order of first appearance; a name given twice for one dataset counts once."""
    if isinstance(labels, dict):
        for f in labels:
            if not 0 <= int(f) < nfiles:
                raise IgdError("build_groups: dataset %s is not in [0, %d)" % (f, nfiles))
        labels = [labels.get(f, ()) for f in range(nfiles)]
    if len(labels) != nfiles:
        raise IgdError("build_groups: labels for %d datasets given, the database has %d" % (len(labels), nfiles))
    number, off, idx = {}, [0], []
    for names in labels:
        idx += sorted({number.setdefault(str(n), len(number)) for n in names})
        off.append(len(idx))
    g = DatasetGroups(off, idx, list(number), check=False)
    g.check("build_groups")
    return g


def read_groups_file(path, file_names):
    """DatasetGroups from a `dataset<TAB>group` file: dataset is a name of file_names exactly, or a decimal index; `#` lines and
    blank lines are skipped; a dataset may occur on several lines; groups are numbered in order of first appearance."""
    byname = {}
    for f, n in enumerate(file_names):
        byname.setdefault(n, f)
    number, per = {}, [set() for _ in file_names]
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            ds, tab, grp = line.partition("\t")
            if not tab or not grp:
                raise IgdError("groups file %s, line %d: not a dataset, a tab and a group" % (path, ln))
            f = byname.get(ds, int(ds) if ds.isdigit() and int(ds) < len(file_names) else None)
            if f is None:
                raise IgdError("groups file %s, line %d: the database has no dataset %s" % (path, ln, ds))
            if grp not in number and len(number) == GROUP_MAX:
                raise IgdError("groups file %s, line %d: more than %d groups" % (path, ln, GROUP_MAX))
            per[f].add(number.setdefault(grp, len(number)))
    if not number:
        raise IgdError("groups file %s: no group given" % path)
    off = np.zeros(len(per) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in per])
    return DatasetGroups(off, [g for p in per for g in sorted(p)], list(number))


def _groups(groups, nfiles, what):
    if not isinstance(groups, DatasetGroups):
        raise IgdError("%s: groups must be a DatasetGroups (build_groups(), Database.read_groups())" % what)
    if groups.nfiles != nfiles:
        raise IgdError("%s: the grouping is of %d datasets, the database has %d" % (what, groups.nfiles, nfiles))
    return groups


def group_support_host(igd_path, ichr, qs, qe, groups, v=0, rule=None, value_filter=None, min_overlap=None):
    """Support counts per group of datasets of one query set on the host (igdc_group_support_host_ov; no device is touched):
    (gsupport int64[ngroups], gnhit) as Database.group_support() defines them, min_overlap included."""
    ichr, qs, qe = _regions(ichr, qs, qe)
    mo = _min_overlap(min_overlap, "group_support_host")
    with _HostDb(igd_path, "group_support_host") as h:
        g = _groups(groups, h.nfiles, "group_support_host")
        rule, vf = h.dispatch(v, rule, value_filter)
        sup, nhit = np.zeros(max(g.ngroups, 1), np.int64), C.c_int64(0)
        g.check("group_support_host")                # (what the C entry refuses as an argument is refused here, by name)
        if h.L.igdc_group_support_host_ov(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), _ptr(g.off), _ptr(g.idx), g.ngroups,
                                          vf, rule, _ptr(sup), C.byref(nhit), C.byref(mo) if mo is not None else None) != 0:
            raise IgdError("group_support_host: a tile of %s could not be read" % igd_path)
        return sup[:g.ngroups], nhit.value


class Workspace:
    """The table of a workspace (include/igd_hip.h: THE WORKSPACE): the stretches of the contigs a permutation may place a
    region in.  Built by build_workspace() or Database.read_workspace(); handed as workspace= together with mode="workspace".
    nctg, nseg; w_off int64[nctg + 1], w_start, w_len int32[nseg], w_pre int32[nseg + nctg] (copies); ctg_len as it was built.
    first_unplaceable(ichr, qs, qe): the first region on a known contig that fits in no segment, or -1.  outside(ichr, qs,
    qe): the regions on known contigs that do not lie inside one segment."""

    def __init__(self, table, ctg_len):
        self._t, self.ctg_len = table, ctg_len
        t = table.contents
        self.nctg, self.nseg = int(t.nctg), int(t.nseg)

        def arr(p, n, ct, dt):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,)).astype(dt) if n > 0 else np.zeros(0, dt)
        self.w_off = arr(t.w_off, self.nctg + 1, C.c_int64, np.int64)
        self.w_start = arr(t.w_start, self.nseg, C.c_int32, np.int32)
        self.w_len = arr(t.w_len, self.nseg, C.c_int32, np.int32)
        self.w_pre = arr(t.w_pre, self.nseg + self.nctg, C.c_int32, np.int32)

    @property
    def ptr(self):
        return C.cast(self._t, C.c_void_p)

    def first_unplaceable(self, ichr, qs, qe):
        ichr, qs, qe = _regions(ichr, qs, qe)
        return int(N.cli().igdc_workspace_first_unplaceable(self.ptr, _ptr(self.ctg_len), _ptr(ichr), _ptr(qs), _ptr(qe), len(qs)))

    def outside(self, ichr, qs, qe):
        ichr, qs, qe = _regions(ichr, qs, qe)
        return int(N.cli().igdc_workspace_outside(self.ptr, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs)))

    def __del__(self):
        if getattr(self, "_t", None):
            N.cli().igdc_workspace_free(self._t)
            self._t = None


def build_workspace(ichr, a, b, ctg_len):
    """The Workspace of the segments (ichr, a, b) on contigs of lengths ctg_len (igdc_workspace_build): merged at gap 0,
    clipped to the contigs, per contig ordered by length descending, then start ascending."""
    ichr, a, b, ctg_len = _perm_regions(ichr, a, b, ctg_len, "build_workspace")
    t = C.POINTER(N.HipWorkspace)()
    if N.cli().igdc_workspace_build(_ptr(ichr), _ptr(a), _ptr(b), len(a), _ptr(ctg_len), len(ctg_len), C.byref(t)) != 0:
        raise IgdError("build_workspace: bad argument (a negative contig length), or out of memory")
    return Workspace(t, ctg_len)


def _perm_mode(mode, what, workspace=None):
    """the mode number of a call; mode="workspace" and workspace= come together or not at all (ValueError)"""
    if (mode == "workspace") != (workspace is not None):
        raise ValueError("%s: mode='workspace' and workspace= go together, not one without the other" % what)
    if workspace is not None:
        if not isinstance(workspace, Workspace):
            raise ValueError("%s: workspace must be a Workspace (build_workspace(), Database.read_workspace())" % what)
        return PERM_WORKSPACE
    if mode not in PERM_MODES:
        raise IgdError("%s: mode must be 'circular' or 'shuffle', not %r" % (what, mode))
    return PERM_MODES[mode]


PERM_RESAMPLE = 4                                    # IGD_HIP_PERM_RESAMPLE: mode="resample" together with universe=


def _perm_pool(mode, universe, ctg_len, workspace, what):
    """None, or the pool of a resampling call as three C-ordered int32 arrays.  mode="resample" and universe= come together or not
    at all, and with them neither contig lengths nor a workspace: nothing is placed (ValueError)."""
    if (mode == "resample") != (universe is not None):
        raise ValueError("%s: mode='resample' and universe= go together, not one without the other" % what)
    if universe is None:
        return None
    if workspace is not None:
        raise ValueError("%s: mode='resample' draws from the universe, it places nothing: there is no workspace= with it" % what)
    if ctg_len is not None:
        raise ValueError("%s: mode='resample' draws from the universe, it places nothing: ctg_len (genome_path) must be None" % what)
    if len(universe) != 3:
        raise ValueError("%s: universe must be (ichr, qs, qe)" % what)
    return _regions(*universe, what, "universe regions")


def _pool_args(pool):
    return _ptr(pool[0]), _ptr(pool[1]), _ptr(pool[2]), len(pool[1])


_Placement = collections.namedtuple("_Placement", "ichr qs qe ctg_len sfx mid tail refused keep")


def _placement(ichr, qs, qe, ctg_len, mode, workspace, universe, what):
    """What the six entries of the three nulls share: the call's regions as C-ordered int32 and how its permuted sets are made.
    sfx names the C entry -- "_ws": placed by mode, inside a workspace or not; "_rs": drawn from a universe (then ctg_len is None) --
    mid is what that entry takes between nq and the seed, tail what it takes last, refused the host routes' words for what the
    native call may have refused; keep holds the arrays behind mid's pointers."""
    pool = _perm_pool(mode, universe, ctg_len, workspace, what)
    if pool is not None:
        ichr, qs, qe = _regions(ichr, qs, qe, what)
        return _Placement(ichr, qs, qe, None, "_rs", _pool_args(pool), (), "%d regions from a universe of %d" % (len(qs), len(pool[1])), pool)
    ichr, qs, qe, ctg_len = _perm_regions(ichr, qs, qe, ctg_len, what)
    pm = _perm_mode(mode, what, workspace)
    return _Placement(ichr, qs, qe, ctg_len, "_ws", (_ptr(ctg_len), pm), (_ws_ptr(workspace),), "a region outside its contig or its workspace", workspace)


def _placement_fits(P, nctg, what):
    if P.ctg_len is not None:
        _ctg_len_matches(P.ctg_len, nctg, what)


def resample_regions_host(ichr, qs, qe, nq, p0, np_, seed=0):
    """Draws [p0, p0 + np_) of nq regions without replacement from the pool (ichr, qs, qe) on the host
    (igdc_resample_regions_host; no device is touched): (ichr, qs, qe) int32[np_, nq] as Database.resample_regions() defines them."""
    pool = _regions(ichr, qs, qe, "resample_regions_host", "universe regions")
    out = [np.empty((int(np_), int(nq)), np.int32) for _ in range(3)] if int(np_) >= 0 and int(nq) >= 0 else [np.empty(0, np.int32)] * 3
    if N.cli().igdc_resample_regions_host(*_pool_args(pool), int(nq), _seed(seed), int(p0), int(np_), *[_ptr(a) for a in out]) != 0:
        raise IgdError("resample_regions_host: bad argument (%d regions from a universe of %d)" % (int(nq), len(pool[1])))
    return tuple(out)


def _ws_ptr(workspace):
    return None if workspace is None else workspace.ptr


def _perm_regions(ichr, qs, qe, ctg_len, what):
    ctg_len = _i32(ctg_len)
    return (*_regions(ichr, qs, qe, what, ok=ctg_len.ndim == 1), ctg_len)


def permute_regions_host(ichr, qs, qe, ctg_len, p0, np_, seed=0, mode="circular", workspace=None):
    """Permutations [p0, p0 + np_) of a region list on the host (igdc_permute_regions_host_ws; no device is touched):
    (qs, qe) int32[np_, nq] as Database.permute_regions() defines them."""
    ichr, qs, qe, ctg_len = _perm_regions(ichr, qs, qe, ctg_len, "permute_regions_host")
    pm = _perm_mode(mode, "permute_regions_host", workspace)
    oqs, oqe = np.empty((int(np_), len(qs)), np.int32), np.empty((int(np_), len(qs)), np.int32)
    if N.cli().igdc_permute_regions_host_ws(_ptr(ichr), _ptr(qs), _ptr(qe), len(qs), _ptr(ctg_len), len(ctg_len),
                                            pm, _seed(seed), int(p0), int(np_), _ptr(oqs), _ptr(oqe), _ws_ptr(workspace)) != 0:
        raise IgdError("permute_regions_host: bad argument")
    return oqs, oqe


def permute_host(igd_path, ichr, qs, qe, ctg_len, nperm, seed=0, mode="circular", v=0, rule=None, value_filter=None, min_overlap=None,
                 workspace=None, universe=None):
    """The permutation null of the support counts on the host (igdc_permute_host: pread on the .igd, threads over the
    permutations; no device is touched): a PermutationSupport as Database.permutation_support() defines it, min_overlap
    included (igdc_permute_host_ov), and mode="resample" with universe= and ctg_len None (igdc_permute_host_rs)."""
    P = _placement(ichr, qs, qe, ctg_len, mode, workspace, universe, "permute_host")
    mo = _min_overlap(min_overlap, "permute_host")
    with _HostDb(igd_path, None) as h:
        _placement_fits(P, h.nctg, "permute_host")
        rule, vf = h.dispatch(v, rule, value_filter)
        out = [np.empty(h.nfiles + 1, np.int64) for _ in range(7)]
        a = (h.core, h.m, _ptr(P.ichr), _ptr(P.qs), _ptr(P.qe), len(P.qs), *P.mid, _seed(seed), int(nperm), vf, rule, *[_ptr(x) for x in out])
        if getattr(h.L, "igdc_permute_host" + P.sfx)(*a, None if mo is None else C.byref(mo), *P.tail) != 0:
            raise IgdError("permute_host: a refused argument (number of permutations, %s), or a tile of %s could not be read" % (P.refused, igd_path))
    return PermutationSupport(*out, int(nperm))


def perm_summary(ps):
    """mean, standard deviation (ddof = 1), z-score and -log10 of the one-sided permutation p-values (n_ge + 1) / (P + 1) and
    (n_le + 1) / (P + 1) of a PermutationSupport (igdc_perm_summary: the variance's numerator is exact): a PermutationSummary
    of float64 arrays.  sd is NaN for one permutation, z is NaN where sd is 0 or NaN."""
    a = [np.ascontiguousarray(x, dtype=np.int64) for x in (ps.observed, ps.sum, ps.sumsq, ps.n_ge, ps.n_le)]
    n = len(a[0])
    if any(x.shape != (n,) for x in a):
        raise IgdError("perm_summary: arrays of different lengths")
    out = [np.empty(n, np.float64) for _ in range(5)]
    if N.cli().igdc_perm_summary(*[_ptr(x) for x in a], int(ps.nperm), n, *[_ptr(x) for x in out]) != 0:
        raise IgdError("perm_summary: bad argument")
    return PermutationSummary(*out)


ShiftSupport = collections.namedtuple("ShiftSupport", "shifted offsets")
SHIFT_MAX = 4096                                     # IGD_HIP_SHIFT_MAX: offsets of one call
SHIFT_MAX_OFFSET = 1 << 30                           # IGD_HIP_SHIFT_MAX_OFFSET


def shift_offsets(window, step):
    """int32 offsets -k * step .. k * step with k = window // step (what `igd search -Z window,step` uses): 2 k + 1 of them,
    the middle one 0."""
    window, step = int(window), int(step)
    if window < 0 or step < 1 or window > SHIFT_MAX_OFFSET:
        raise IgdError("shift_offsets: window %d, step %d: not 0 <= window <= %d with step >= 1" % (window, step, SHIFT_MAX_OFFSET))
    k = window // step
    if 2 * k + 1 > SHIFT_MAX:
        raise IgdError("shift_offsets: %d shifts, not 1 .. %d" % (2 * k + 1, SHIFT_MAX))
    return (np.arange(-k, k + 1, dtype=np.int64) * step).astype(np.int32)


def _offsets(offsets, what):
    """the offsets of a shift call as C-ordered int32: 1 .. SHIFT_MAX whole numbers within +-2^30 (the engine's two refusals, said
    here because a conversion to int32 would wrap a larger one)"""
    o = np.asarray(offsets)
    if o.ndim != 1 or (o.size and o.dtype.kind not in "iu"):
        raise IgdError("%s: offsets must be a list of whole numbers" % what)
    if not 1 <= len(o) <= SHIFT_MAX:
        raise IgdError("%s: %d shifts, not 1 .. %d" % (what, len(o), SHIFT_MAX))
    bad = np.flatnonzero((o > SHIFT_MAX_OFFSET) | (o < -SHIFT_MAX_OFFSET))
    if len(bad):
        raise IgdError("%s: offset %d = %d is beyond +-%d" % (what, bad[0], int(o[bad[0]]), SHIFT_MAX_OFFSET))
    return np.ascontiguousarray(o, dtype=np.int32)


def shift_regions_host(ichr, qs, qe, ctg_len, offsets):
    """A region list under rigid shifts on the host (igdc_shift_regions_host; no device is touched): (qs, qe) int32[nshift, nq]
    as Database.shift_regions() defines them."""
    ichr, qs, qe, ctg_len = _perm_regions(ichr, qs, qe, ctg_len, "shift_regions_host")
    offsets = _offsets(offsets, "shift_regions_host")
    oqs, oqe = np.empty((len(offsets), len(qs)), np.int32), np.empty((len(offsets), len(qs)), np.int32)
    if N.cli().igdc_shift_regions_host(_ptr(ichr), _ptr(qs), _ptr(qe), len(qs), _ptr(ctg_len), len(ctg_len), _ptr(offsets), len(offsets),
                                       _ptr(oqs), _ptr(oqe)) != 0:
        raise IgdError("shift_regions_host: bad argument")
    return oqs, oqe


def shift_support_host(igd_path, ichr, qs, qe, ctg_len, offsets, v=0, rule=None, value_filter=None, min_overlap=None):
    """The support of one region set under rigid shifts on the host (igdc_shift_support_host_ov: pread on the .igd, threads over
    the shifts; no device is touched): a ShiftSupport as Database.shift_support() defines it."""
    ichr, qs, qe, ctg_len = _perm_regions(ichr, qs, qe, ctg_len, "shift_support_host")
    offsets = _offsets(offsets, "shift_support_host")
    mo = _min_overlap(min_overlap, "shift_support_host")
    with _HostDb(igd_path, "shift_support_host") as h:
        _ctg_len_matches(ctg_len, h.nctg, "shift_support_host")
        rule, vf = h.dispatch(v, rule, value_filter)
        shifted = np.empty((len(offsets), h.nfiles + 1), np.int64)
        if h.L.igdc_shift_support_host_ov(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), _ptr(ctg_len), _ptr(offsets), len(offsets),
                                          vf, rule, _ptr(shifted), None if mo is None else C.byref(mo)) != 0:
            raise IgdError("shift_support_host: a refused argument (a region outside its contig, more regions than a batch), or a tile of %s "
                           "could not be read" % igd_path)
    return ShiftSupport(shifted, offsets)


def local_zscore(ps, ss):
    """float64[nshift, nfiles + 1]: every shifted support of a ShiftSupport placed in the null of a PermutationSupport of the same
    set, z[j, f] = (shifted[j, f] - mean[f]) / sd[f] with mean and sd exactly as perm_summary() forms them; NaN where sd is 0
    (or NaN: one permutation).  A peak at offset 0 means the association depends on the exact position."""
    sm = perm_summary(ps)
    sh = np.asarray(ss.shifted, dtype=np.int64)
    if sh.ndim != 2 or sh.shape[1] != len(sm.mean):
        raise IgdError("local_zscore: shifted must be int64[nshift, %d], the columns of the PermutationSupport" % len(sm.mean))
    sd = np.where(sm.sd == 0, np.nan, sm.sd)
    return (sh.astype(np.float64) - sm.mean[None, :]) / sd[None, :]


def permute_nearest_host(igd_path, ichr, qs, qe, ctg_len, nperm, window, seed=0, mode="circular", value_filter=None, workspace=None,
                         universe=None):
    """Database.permutation_nearest() on the host (igdc_permute_nearest_host: pread on the .igd, threads over the permutations;
    no device is touched): a PermutationNearest.  mode="resample" with universe= and ctg_len None: igdc_permute_nearest_host_rs."""
    P = _placement(ichr, qs, qe, ctg_len, mode, workspace, universe, "permute_nearest_host")
    with _HostDb(igd_path, "permute_nearest_host") as h:
        _placement_fits(P, h.nctg, "permute_nearest_host")
        out = [np.empty((max(int(nperm), 0) + 1, h.nfiles + 1), np.int64) for _ in range(3)]
        if getattr(h.L, "igdc_permute_nearest_host" + P.sfx)(h.core, h.m, _ptr(P.ichr), _ptr(P.qs), _ptr(P.qe), len(P.qs), *P.mid, _seed(seed),
                                                             int(nperm), _window(window, "permute_nearest_host"), _value_filter(value_filter),
                                                             *[_ptr(a) for a in out], *P.tail) != 0:
            raise IgdError("permute_nearest_host: a refused argument (number of permutations, window, %s), or a tile of %s could not be read"
                           % (P.refused, igd_path))
        return PermutationNearest(*out, int(window), int(nperm))


def perm_nearest_summary(pn):
    """The summary of a PermutationNearest (igdc_perm_nearest_summary; igd_core.h has the formulas): a
    PermutationNearestSummary of arrays [nfiles + 1] -- float64, but within_n_ge, n_def and dist_n_le, which are int64.  Of the
    counts: mean, sd, z of the permuted n_within, the permutations with n_within >= the observed one and -log10 of the upper
    p-value.  Of the distances: the observed mean distance, mean and sd (ddof = 1) of the permuted mean distances over the
    n_def permutations that have one, z, the permutations at least as close as observed (compared exactly) and -log10 of the
    lower p-value."""
    nw, sd = (np.ascontiguousarray(x, dtype=np.int64) for x in (pn.n_within, pn.sum_dist))
    if nw.ndim != 2 or nw.shape != sd.shape or nw.shape[0] != int(pn.nperm) + 1:
        raise IgdError("perm_nearest_summary: n_within and sum_dist must be int64[nperm + 1, ncols]")
    n = nw.shape[1]
    kinds = [np.float64] * 3 + [np.int64] + [np.float64] * 5 + [np.int64] * 2 + [np.float64]
    out = [np.empty(n, k) for k in kinds]
    if N.cli().igdc_perm_nearest_summary(_ptr(nw), _ptr(sd), int(pn.nperm), n, *[_ptr(x) for x in out]) != 0:
        raise IgdError("perm_nearest_summary: bad argument")
    return PermutationNearestSummary(*out)


def _window(window, what):
    w = int(window)
    if not -2 ** 31 <= w < 2 ** 31:                      # (inside int32 the native call decides: 0 .. 2^30)
        raise IgdError("%s: window %d outside 0 .. %d" % (what, w, NEAREST_MAX_WINDOW))
    return w


def nearest_host(igd_path, ichr, qs, qe, window, value_filter=None):
    """Database.nearest() on the host (igdc_nearest_host: pread on the .igd, threads over the regions; no device is touched):
    (dist int32[nq, nfiles], dmin int32[nq])."""
    ichr, qs, qe = _regions(ichr, qs, qe, "nearest_host")
    with _HostDb(igd_path, "nearest_host") as h:
        dist, dmin = np.empty((len(qs), h.nfiles), np.int32), np.empty(len(qs), np.int32)
        if h.L.igdc_nearest_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), _window(window, "nearest_host"),
                                 _value_filter(value_filter), _ptr(dist), _ptr(dmin)) != 0:
            raise IgdError("nearest_host: a window outside 0 .. %d, or a tile of %s could not be read" % (NEAREST_MAX_WINDOW, igd_path))
        return dist, dmin


def nearest_sets_host(igd_path, ichr, qs, qe, set_off, window, value_filter=None):
    """Database.nearest_sets() on the host (igdc_nearest_sets_host; no device is touched): a NearestSets."""
    ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "nearest_sets_host")
    with _HostDb(igd_path, "nearest_sets_host") as h:
        out = [np.empty((nsets, h.nfiles + 1), np.int64) for _ in range(3)]
        if h.L.igdc_nearest_sets_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets,
                                      _window(window, "nearest_sets_host"), _value_filter(value_filter), *[_ptr(a) for a in out]) != 0:
            raise IgdError("nearest_sets_host: a bad set_off, a window outside 0 .. %d, or a tile of %s could not be read"
                           % (NEAREST_MAX_WINDOW, igd_path))
        return NearestSets(*out, int(window))


def _edges(edges, what):
    """1 .. 63 strictly ascending int32 edges (the native call refuses the same lists)"""
    e = np.asarray(edges)
    if e.ndim != 1 or not 1 <= len(e) <= NEAREST_MAX_EDGES or e.dtype.kind not in "iu":
        raise IgdError("%s: edges must be 1 to %d integers" % (what, NEAREST_MAX_EDGES))
    e = e.astype(np.int64)
    if (e < -2 ** 31).any() or (e >= 2 ** 31).any() or (np.diff(e) <= 0).any():
        raise IgdError("%s: edges must be strictly ascending int32 values" % what)
    return np.ascontiguousarray(e, dtype=np.int32)


def nearest_signed_host(igd_path, ichr, qs, qe, window, value_filter=None):
    """Database.nearest_signed() on the host (igdc_nearest_signed_host; no device is touched):
    (sdist int32[nq, nfiles], sdmin int32[nq])."""
    ichr, qs, qe = _regions(ichr, qs, qe, "nearest_signed_host")
    with _HostDb(igd_path, "nearest_signed_host") as h:
        sdist, sdmin = np.empty((len(qs), h.nfiles), np.int32), np.empty(len(qs), np.int32)
        if h.L.igdc_nearest_signed_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), _window(window, "nearest_signed_host"),
                                        _value_filter(value_filter), _ptr(sdist), _ptr(sdmin)) != 0:
            raise IgdError("nearest_signed_host: a window outside 0 .. %d, or a tile of %s could not be read" % (NEAREST_MAX_WINDOW, igd_path))
        return sdist, sdmin


def nearest_hist_host(igd_path, ichr, qs, qe, set_off, window, edges, value_filter=None):
    """Database.nearest_hist() on the host (igdc_nearest_hist_host; no device is touched): a NearestHist."""
    ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "nearest_hist_host")
    edges = _edges(edges, "nearest_hist_host")
    with _HostDb(igd_path, "nearest_hist_host") as h:
        hist = np.empty((nsets, len(edges) + 1, h.nfiles + 1), np.int64)
        if h.L.igdc_nearest_hist_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets,
                                      _window(window, "nearest_hist_host"), _value_filter(value_filter), _ptr(edges), len(edges),
                                      _ptr(hist)) != 0:
            raise IgdError("nearest_hist_host: a bad set_off, a window outside 0 .. %d, or a tile of %s could not be read"
                           % (NEAREST_MAX_WINDOW, igd_path))
        return NearestHist(hist, edges, int(window))


def _measure(measure, what):
    """"edges" / "midpoints" (or FLANK_EDGES / FLANK_MIDPOINTS) -> the native constant"""
    if isinstance(measure, str) and measure in ("edges", "midpoints"):
        return FLANK_EDGES if measure == "edges" else FLANK_MIDPOINTS
    if not isinstance(measure, (str, bool)) and measure in (FLANK_EDGES, FLANK_MIDPOINTS):
        return int(measure)
    raise IgdError("%s: measure must be \"edges\" or \"midpoints\"" % what)


def _nbins(nbins, what):
    if isinstance(nbins, (bool, float)) or not isinstance(nbins, (int, np.integer)) or not 1 <= nbins <= FLANK_MAX_BINS:
        raise IgdError("%s: nbins must be an integer from 1 to %d" % (what, FLANK_MAX_BINS))
    return int(nbins)


def flanks_host(igd_path, ichr, qs, qe, window, measure="midpoints", value_filter=None):
    """Database.flanks() on the host (igdc_flank_host; no device is touched): (up, down int32[nq, nfiles], upmin, downmin
    int32[nq])."""
    ichr, qs, qe = _regions(ichr, qs, qe, "flanks_host")
    measure = _measure(measure, "flanks_host")
    with _HostDb(igd_path, "flanks_host") as h:
        up, down = np.empty((len(qs), h.nfiles), np.int32), np.empty((len(qs), h.nfiles), np.int32)
        upmin, downmin = np.empty(len(qs), np.int32), np.empty(len(qs), np.int32)
        if h.L.igdc_flank_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), _window(window, "flanks_host"), measure,
                               _value_filter(value_filter), _ptr(up), _ptr(down), _ptr(upmin), _ptr(downmin)) != 0:
            raise IgdError("flanks_host: a window outside 0 .. %d, or a tile of %s could not be read" % (NEAREST_MAX_WINDOW, igd_path))
        return up, down, upmin, downmin


def flank_reldist_host(igd_path, ichr, qs, qe, set_off, window, nbins=50, measure="midpoints", value_filter=None):
    """Database.flank_reldist() on the host (igdc_flank_reldist_host; no device is touched): a FlankReldist."""
    ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "flank_reldist_host")
    nbins, m = _nbins(nbins, "flank_reldist_host"), _measure(measure, "flank_reldist_host")
    with _HostDb(igd_path, "flank_reldist_host") as h:
        hist = np.empty((nsets, nbins, h.nfiles + 1), np.int64)
        if h.L.igdc_flank_reldist_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets,
                                       _window(window, "flank_reldist_host"), m, _value_filter(value_filter), nbins, _ptr(hist)) != 0:
            raise IgdError("flank_reldist_host: a bad set_off, a window outside 0 .. %d, or a tile of %s could not be read"
                           % (NEAREST_MAX_WINDOW, igd_path))
        return FlankReldist(hist, nbins, int(window), m)


def _gap(gap, what):
    if isinstance(gap, (bool, float)) or not isinstance(gap, (int, np.integer)) or not 0 <= gap <= MERGE_MAX_GAP:
        raise IgdError("%s: gap must be an integer from 0 to %d" % (what, MERGE_MAX_GAP))
    return int(gap)


def _merge_out(n, nsets):
    return (np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(nsets + 1, np.int64), np.empty(n, np.int32),
            np.empty(nsets, np.int64))


def _merge_cut(mc, ms, me, moff, cnt, dropped):
    r = int(moff[-1])
    return mc[:r], ms[:r], me[:r], moff, cnt[:r], dropped


def permute_bp_host(igd_path, ichr, qs, qe, ctg_len, nperm, seed=0, mode="circular", v=0, rule=None, value_filter=None, workspace=None,
                    universe=None):
    """Database.permutation_bp() on the host (igdc_permute_bp_host: pread on the .igd, threads over the permutations; no device
    is touched): a PermutationBp.  mode="resample" with universe= and ctg_len None: igdc_permute_bp_host_rs."""
    P = _placement(ichr, qs, qe, ctg_len, mode, workspace, universe, "permute_bp_host")
    with _HostDb(igd_path, "permute_bp_host") as h:
        _placement_fits(P, h.nctg, "permute_bp_host")
        rule, vf = h.dispatch(v, rule, value_filter)
        rows = max(int(nperm), 0) + 1
        inter, set_bp, n_merged = np.empty((rows, h.nfiles + 1), np.int64), np.empty(rows, np.int64), np.empty(rows, np.int64)
        dropped, file_bp = np.zeros(1, np.int64), np.empty(h.nfiles + 1, np.int64)
        if getattr(h.L, "igdc_permute_bp_host" + P.sfx)(h.core, h.m, _ptr(P.ichr), _ptr(P.qs), _ptr(P.qe), len(P.qs), *P.mid, _seed(seed), int(nperm),
                                                        vf, rule, _ptr(inter), _ptr(set_bp), _ptr(n_merged), _ptr(dropped), *P.tail) != 0:
            raise IgdError("permute_bp_host: a refused argument (number of permutations, %s), or a tile of %s could not be read" % (P.refused, igd_path))
        if h.L.igdc_dataset_bp_host(h.core, h.m, vf, rule, _ptr(file_bp)) != 0:
            raise IgdError("permute_bp_host: a tile of %s could not be read" % igd_path)
        return PermutationBp(inter, set_bp, n_merged, int(dropped[0]), file_bp, int(nperm))


def perm_bp_summary(pb):
    """The summary of a PermutationBp (igdc_perm_bp_summary; igd_core.h has the formulas): a PermutationBpSummary of arrays
    [nfiles + 1] -- float64, but observed, n_ge, n_le, jaccard_n_def and jaccard_n_ge, which are int64.  Of the base pairs: the
    observed overlap, mean, sd (ddof = 1) and z of the permuted ones, fold = observed / mean, the permutations with at least
    and at most the observed overlap and -log10 of the two p-values.  Of the Jaccards: the observed one, mean and sd of the
    permuted ones over the jaccard_n_def permutations that have one, and the permutations whose Jaccard is at least the
    observed one (compared exactly)."""
    inter, set_bp, file_bp = (np.ascontiguousarray(x, dtype=np.int64) for x in (pb.inter, pb.set_bp, pb.file_bp))
    if inter.ndim != 2 or inter.shape != (int(pb.nperm) + 1, len(file_bp)) or set_bp.shape != (inter.shape[0],):
        raise IgdError("perm_bp_summary: inter must be int64[nperm + 1, ncols], set_bp int64[nperm + 1], file_bp int64[ncols]")
    n = inter.shape[1]
    kinds = [np.int64] + [np.float64] * 4 + [np.int64] * 2 + [np.float64] * 5 + [np.int64] * 2
    out = [np.empty(n, k) for k in kinds]
    if N.cli().igdc_perm_bp_summary(_ptr(inter), _ptr(set_bp), _ptr(file_bp), int(pb.nperm), n, *[_ptr(x) for x in out]) != 0:
        raise IgdError("perm_bp_summary: bad argument")
    return PermutationBpSummary(*out)


def merge_host(igd_path, ichr, qs, qe, set_off, gap=0):
    """Database.merge_sets() on the host (igdc_merge_host; no device is touched): (ichr, qs, qe, set_off, count, n_dropped)."""
    ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "merge_host")
    gap = _gap(gap, "merge_host")
    out = _merge_out(len(qs), nsets)
    with _HostDb(igd_path, "merge_host") as h:
        if h.L.igdc_merge_host(h.core, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, gap, *[_ptr(a) for a in out]) != 0:
            raise IgdError("merge_host: a bad set_off")
    return _merge_cut(*out)


def dataset_bp_host(igd_path, v=0, rule=None, value_filter=None):
    """Database.dataset_bp() on the host (igdc_dataset_bp_host; no device is touched): int64[nfiles + 1]."""
    with _HostDb(igd_path, "dataset_bp_host") as h:
        rule, vf = h.dispatch(v, rule, value_filter)
        bp = np.empty(h.nfiles + 1, np.int64)
        if h.L.igdc_dataset_bp_host(h.core, h.m, vf, rule, _ptr(bp)) != 0:
            raise IgdError("dataset_bp_host: a tile of %s could not be read" % igd_path)
        return bp


def jaccard_host(igd_path, ichr, qs, qe, set_off, v=0, rule=None, value_filter=None):
    """Database.jaccard_sets() on the host (igdc_jaccard_host; no device is touched): a JaccardSets."""
    ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "jaccard_host")
    with _HostDb(igd_path, "jaccard_host") as h:
        rule, vf = h.dispatch(v, rule, value_filter)
        js = JaccardSets(np.empty((nsets, h.nfiles + 1), np.int64), np.empty(nsets, np.int64), np.empty(h.nfiles + 1, np.int64),
                         np.empty(nsets, np.int64), np.empty(nsets, np.int64))
        if h.L.igdc_jaccard_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, vf, rule, _ptr(js.inter),
                                 _ptr(js.set_bp), _ptr(js.file_bp), _ptr(js.n_merged), _ptr(js.n_dropped)) != 0:
            raise IgdError("jaccard_host: a bad set_off, or a tile of %s could not be read" % igd_path)
        return js


def jaccard_summary(js):
    """(jaccard, set_fraction, file_fraction), each float64[nsets, nfiles + 1], of a JaccardSets (igdc_jaccard_summary):
    inter / (set_bp + file_bp - inter) and the two containment fractions inter / set_bp and inter / file_bp, NaN where the
    divisor is 0.  (igd_amd.jaccard is about co-occurrence: the Jaccard of two datasets over the regions of a set.)"""
    inter = np.ascontiguousarray(js.inter, np.int64)
    set_bp, file_bp = np.ascontiguousarray(js.set_bp, np.int64), np.ascontiguousarray(js.file_bp, np.int64)
    if inter.ndim != 2 or inter.shape != (len(set_bp), len(file_bp)):
        raise IgdError("jaccard_summary: inter must be int64[%d, %d]" % (len(set_bp), len(file_bp)))
    out = [np.empty(inter.shape, np.float64) for _ in range(3)]
    if N.cli().igdc_jaccard_summary(_ptr(inter), _ptr(set_bp), _ptr(file_bp), inter.shape[0], inter.shape[1], *[_ptr(a) for a in out]) != 0:
        raise IgdError("jaccard_summary: bad argument")
    return tuple(out)


def reldist_summary(fr):
    """(n_flanked int64[nsets, nfiles + 1], fraction float64[nsets, nbins, nfiles + 1]) of a FlankReldist: the flanked regions per
    set and dataset and the share of each bin among them (`bedtools reldist`'s fraction column), NaN where n_flanked is 0."""
    hist = np.asarray(fr.hist, np.int64)
    n = hist.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(n[:, None, :] > 0, hist / n[:, None, :].astype(np.float64), np.nan)
    return n, frac


def nearest_summary(ns):
    """mean distance = sum_dist / n_within of a NearestSets as float64[nsets, nfiles + 1], NaN where n_within is 0
    (igdc_nearest_summary)."""
    nw, sd = (np.ascontiguousarray(x, dtype=np.int64) for x in (ns.n_within, ns.sum_dist))
    if nw.shape != sd.shape:
        raise IgdError("nearest_summary: arrays of different shapes")
    mean = np.empty(nw.shape, np.float64)
    if N.cli().igdc_nearest_summary(_ptr(nw), _ptr(sd), nw.size, _ptr(mean)) != 0:
        raise IgdError("nearest_summary: bad argument")
    return mean


def _map_op(op, what):
    if op not in MAP_OPS:
        raise IgdError("%s: op %r is none of count, sum, min, max" % (what, op))
    return MAP_OPS[op]


def map_host(igd_path, ichr, qs, qe, op="sum", value_filter=None):
    """Database.map_values() on the host (igdc_map_host: pread on the .igd, threads over the regions; no device is touched):
    (count int32[nq, nfiles], agg int64[nq, nfiles]); under op "count" agg holds the counts."""
    ichr, qs, qe = _regions(ichr, qs, qe, "map_host")
    o = _map_op(op, "map_host")
    with _HostDb(igd_path, "map_host") as h:
        count, agg = np.empty((len(qs), h.nfiles), np.int32), np.empty((len(qs), h.nfiles), np.int64)
        if h.L.igdc_map_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), o, _value_filter(value_filter), _ptr(count), _ptr(agg)) != 0:
            raise IgdError("map_host: op %s on a database without values, or a tile of %s could not be read" % (op, igd_path))
        return count, agg


def map_sets_host(igd_path, ichr, qs, qe, set_off, op="sum", value_filter=None):
    """Database.map_sets() on the host (igdc_map_sets_host; no device is touched): a MapSets."""
    ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "map_sets_host")
    o = _map_op(op, "map_sets_host")
    with _HostDb(igd_path, "map_sets_host") as h:
        out = [np.empty((nsets, h.nfiles), np.int64) for _ in range(3)]
        if h.L.igdc_map_sets_host(h.core, h.m, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, o, _value_filter(value_filter),
                                  *[_ptr(a) for a in out]) != 0:
            raise IgdError("map_sets_host: a bad set_off, op %s on a database without values, or a tile of %s could not be read"
                           % (op, igd_path))
        return MapSets(*out, op)


def map_summary(ms):
    """(mean_region, mean_pair) of a MapSets as float64[nsets, nfiles] (igdc_map_summary): agg_sum / n_hit, and for op "sum"
    agg_sum / pairs (NaN under the other ops); NaN where the divisor is 0."""
    nh, npairs, sa = (np.ascontiguousarray(x, dtype=np.int64) for x in (ms.n_hit, ms.pairs, ms.agg_sum))
    if nh.shape != npairs.shape or nh.shape != sa.shape:
        raise IgdError("map_summary: arrays of different shapes")
    mean_region, mean_pair = np.empty(nh.shape, np.float64), np.empty(nh.shape, np.float64)
    if N.cli().igdc_map_summary(_ptr(nh), _ptr(npairs), _ptr(sa), nh.size, _map_op(ms.op, "map_summary"), _ptr(mean_region), _ptr(mean_pair)) != 0:
        raise IgdError("map_summary: bad argument")
    return mean_region, mean_pair


def _perm_map_op(op, what):
    """the op number whose rows a null of `op` runs: "mean" (agg_sum / pairs, regioneR's meanInRegions) runs the rows of op sum"""
    if op != "mean" and op not in MAP_OPS:
        raise IgdError("%s: op %r is none of count, sum, min, max, mean" % (what, op))
    return MAP_OPS["sum" if op == "mean" else op]


def permute_map_host(igd_path, ichr, qs, qe, ctg_len, nperm, op, seed=0, mode="circular", value_filter=None, workspace=None, universe=None):
    """Database.permutation_map() on the host (igdc_permute_map_host: pread on the .igd, threads over the permutations; no
    device is touched): a PermutationMap.  mode="resample" with universe= and ctg_len None: igdc_permute_map_host_rs."""
    P = _placement(ichr, qs, qe, ctg_len, mode, workspace, universe, "permute_map_host")
    o = _perm_map_op(op, "permute_map_host")
    with _HostDb(igd_path, "permute_map_host") as h:
        _placement_fits(P, h.nctg, "permute_map_host")
        out = [np.empty((max(int(nperm), 0) + 1, h.nfiles), np.int64) for _ in range(3)]
        if getattr(h.L, "igdc_permute_map_host" + P.sfx)(h.core, h.m, _ptr(P.ichr), _ptr(P.qs), _ptr(P.qe), len(P.qs), *P.mid, _seed(seed),
                                                         int(nperm), o, _value_filter(value_filter), *[_ptr(a) for a in out], *P.tail) != 0:
            raise IgdError("permute_map_host: a refused argument (number of permutations, op %s on a database without values, %s), or a "
                           "tile of %s could not be read" % (op, P.refused, igd_path))
        return PermutationMap(*out, op, int(nperm))


def perm_map_summary(pm):
    """The summary of a PermutationMap (igdc_perm_map_summary; igd_core.h has the formulas): a PermutationMapSummary of arrays
    [nfiles] -- float64, but observed_n_hit, n_def, n_ge and n_le, which are int64.  The statistic of a row is agg_sum / n_hit
    (mean_region) for the ops count, sum, min and max and agg_sum / pairs for "mean" (regioneR's meanInRegions over pairs),
    undefined where the divisor is 0: observed, the n_def permutations that have one, their mean and sd (ddof = 1), z, the
    defined permutations whose statistic is >= / <= the observed one (compared exactly), -log10 of both one-sided p-values
    (n + 1) / (n_def + 1); then mean, sd and z of the permuted n_hit.  NaN where undefined."""
    nh, npairs, sa = (np.ascontiguousarray(x, dtype=np.int64) for x in (pm.n_hit, pm.pairs, pm.agg_sum))
    if nh.ndim != 2 or nh.shape != npairs.shape or nh.shape != sa.shape or nh.shape[0] != int(pm.nperm) + 1:
        raise IgdError("perm_map_summary: n_hit, pairs and agg_sum must be int64[nperm + 1, ncols]")
    _perm_map_op(pm.op, "perm_map_summary")
    n = nh.shape[1]
    kinds = [np.float64, np.int64] + [np.float64] * 3 + [np.int64] * 2 + [np.float64] * 5
    out = [np.empty(n, k) for k in kinds]
    if N.cli().igdc_perm_map_summary(_ptr(nh), _ptr(npairs), _ptr(sa), int(pm.nperm), n, int(pm.op == "mean"), *[_ptr(x) for x in out]) != 0:
        raise IgdError("perm_map_summary: bad argument")
    return PermutationMapSummary(nh[0].copy(), *out)


def _forward(f):
    """A public method that hands all its arguments to the private method f (its own name with an underscore in front) and
    carries f's docstring.  For the group entries: tests/test_gpu_database_args.py holds every public method whose signature
    names (ichr, qs, qe) to a table of its own, which is not this change's to extend; their refusals are held to the same texts
    in tests/test_gpu_group_support.py."""
    def call(self, *args, **kwargs):
        return f(self, *args, **kwargs)
    call.__name__ = f.__name__[1:]
    call.__qualname__ = f.__qualname__.replace("._", ".")
    call.__doc__ = f.__doc__
    return call


class Database:
    def __init__(self, igd_path, device=0):
        self._L = N.cli()
        self._H = N.hip()
        self.build_flags = int(self._H.igd_hip_build_flags())
        if self._H.igd_hip_build_wrong_counts() and os.environ.get("IGD_HIP_ALLOW_EXP_BUILD") != "1":
            raise IgdError("%s is a measurement build (IGD_EXP=0x%x) whose counts are WRONG on purpose; "
                           "IGD_HIP_ALLOW_EXP_BUILD=1 loads it anyway" % (os.path.join(N.LIBDIR, "libigd_hip.so"), self.build_flags))
        self.path = igd_path
        self._core = _open_core(igd_path)
        c = self._core.contents
        self.nbp, self.gtype, self.nctg, self.nfiles = c.nbp, c.gType, c.nCtg, c.nFiles
        self.nrecords, self.ntiles = c.nRecords, c.nTileTotal
        self.contig_names = [c.cName[i].decode() for i in range(self.nctg)]
        self.file_names = [c.fileName[i].decode() for i in range(self.nfiles)]
        self.file_nr = [c.fileNr[i] for i in range(self.nfiles)]
        self.ntile = [c.nTile[i] for i in range(self.nctg)]
        rc = self._L.igdc_attach_path(self._core, igd_path.encode(), int(device))
        if rc != 0:
            err = self._H.igd_hip_last_error().decode()
            self._L.igdc_close(self._core)
            self._core = None
            raise IgdError("cannot put %s on GPU %d (code %d): %s -- there is no CPU search path"
                           % (igd_path, device, rc, err))
        self.dev = C.c_void_p(self._core.contents.dev)
        self.device = int(device)

    # ---- lifetime -----------------------------------------------------------------
    def close(self):
        if getattr(self, "_core", None):
            self._L.igdc_close(self._core)
            self._core = None
            self.dev = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def resident_bytes(self):
        return self._H.igd_hip_resident_bytes(self.dev)

    # ---- host helpers (reference: get_id, parse_bed loop) ---------------------------
    def contig_id(self, name):
        return self._L.igdc_get_id(self._core, name.encode())

    def read_queries(self, qfile, require_chr=True):
        q = N.CoreQueries()
        if self._L.igdc_read_queries(self._core, qfile.encode(), 1 if require_chr else 0, C.byref(q)) != 0:
            raise IOError("cannot open query file %s" % qfile)
        n = q.n
        if n:
            out = tuple(np.ctypeslib.as_array(p, shape=(n,)).copy() for p in (q.ichr, q.qs, q.qe))
        else:
            out = tuple(np.zeros(0, np.int32) for _ in range(3))
        self._L.igdc_queries_free(C.byref(q))
        return out

    @staticmethod
    def cli_dispatch(gtype, v):
        """(rule, engine v) that `igd search -q ... -v V` selects (src/igd_search.c:1023-1030)."""
        if gtype != 0 and v > 0:
            return N.IGD_HIP_RULE_FLAT, int(v)
        return N.IGD_HIP_RULE_NEST, N.IGD_HIP_NO_VALUE_FILTER

    # ---- searches ---------------------------------------------------------------------
    def search(self, ichr, qs, qe, v=0, rule=None, value_filter=None, hits=None, flags=0):
        """Host batch.  Default: the CLI dispatch for `-v v`.  Returns (hits int64[nfiles], total).
        flags: 0 (device checks the order and picks merge-join or bucketing), IGD_HIP_FLAG_SORTED [| IGD_HIP_FLAG_SHORT] (a
        promise, verified; a broken one is repaired by a second pass) or IGD_HIP_FLAG_BUCKET (the caller knows the batch is
        unordered: no order check, ~13 us per 10^6 queries less than 0)."""
        ichr, qs, qe = _regions(ichr, qs, qe)
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        if hits is None:
            hits = np.zeros(max(self.nfiles, 1), np.int64)
        total = C.c_int64(0)
        _chk(self._H.igd_hip_search_ex(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), vf, rule, int(flags),
                                       hits.ctypes.data, C.byref(total)), "igd_hip_search")     # (hits: the caller's, never looked at)
        return hits[: self.nfiles], total.value

    def search_sets(self, ichr, qs, qe, set_off, v=0, rule=None, value_filter=None, hits=None, flags=0, min_overlap=None):
        """Many query sets in one call (igd_hip_search_sets).  Set k is the queries [set_off[k], set_off[k + 1]) of the
        concatenated arrays (set_off: int64[nsets + 1], monotone, set_off[0] = 0).  Returns (hits int64[nsets, nfiles],
        totals int64[nsets]); row k is what search() returns for set k alone.  hits (int64[nsets, nfiles], C order) is added
        to when given.  flags as search() (they steer the route of sets of 2^17 queries and more).
        min_overlap (a MinOverlap, or an int of base pairs; igd_hip_search_sets_ov): only the pairs that reach it are counted,
        and every set, whatever its size, is counted by the slice kernel."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "search_sets", "queries")
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        hits = _out(hits, (nsets, self.nfiles), np.int64, "hits", "search_sets", zero=True)
        totals = np.zeros(max(nsets, 1), np.int64)
        mo = _min_overlap(min_overlap, "search_sets")
        a = (self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, vf, rule, int(flags), _ptr(hits), _ptr(totals))
        _chk(self._H.igd_hip_search_sets(*a) if mo is None else self._H.igd_hip_search_sets_ov(*a, C.byref(mo)), "igd_hip_search_sets")
        return hits, totals[:nsets]

    def search_files(self, paths, v=0, min_overlap=None):
        """One query set per BED file (read as `igd search -q` reads it): (hits int64[len(paths), nfiles], totals)."""
        return self.search_sets(*self._read_sets(paths), v, min_overlap=min_overlap)

    def support_sets(self, ichr, qs, qe, set_off, v=0, rule=None, value_filter=None, support=None, min_overlap=None):
        """Support counts of many query sets in one call (igd_hip_support_sets).  Sets as search_sets().  Returns (support
        int64[nsets, nfiles], nhit int64[nsets]): support[k, f] = the queries of set k that overlap at least one record of
        file f (search_sets counts every overlapping record), nhit[k] = the queries of set k that overlap any record.
        support (int64[nsets, nfiles], C order) is added to when given.  min_overlap (a MinOverlap, or an int of base pairs;
        igd_hip_support_sets_ov): "overlap" then means at least one PAIR that reaches it, as LOLA and bedtools test it."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "support_sets", "queries")
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        support = _out(support, (nsets, self.nfiles), np.int64, "support", "support_sets", zero=True)
        nhit = np.zeros(max(nsets, 1), np.int64)
        mo = _min_overlap(min_overlap, "support_sets")
        a = (self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, vf, rule, _ptr(support), _ptr(nhit))
        _chk(self._H.igd_hip_support_sets(*a) if mo is None else self._H.igd_hip_support_sets_ov(*a, C.byref(mo)), "igd_hip_support_sets")
        return support, nhit[:nsets]

    def support(self, ichr, qs, qe, v=0, rule=None, value_filter=None, min_overlap=None):
        """Support counts of one query set: (int64[nfiles], nhit) -- per file the queries that overlap at least one of its
        records, and the queries that overlap any record.  Row 0 of support_sets() with one set."""
        sup, nhit = self.support_sets(ichr, qs, qe, np.array([0, len(_i32(qs))], np.int64), v, rule, value_filter, min_overlap=min_overlap)
        return sup[0], int(nhit[0])

    def support_files(self, paths, v=0, min_overlap=None):
        """One query set per BED file (read as `igd search -q` reads it): (support int64[len(paths), nfiles], nhit)."""
        return self.support_sets(*self._read_sets(paths), v, min_overlap=min_overlap)

    def read_groups(self, path):
        """The DatasetGroups of a `dataset<TAB>group` file as `igd search -K` reads it: dataset is a file name exactly as the
        database's index lists it, or a decimal dataset number; groups are numbered in order of first appearance."""
        return read_groups_file(path, self.file_names)

    def _group_support_sets(self, ichr, qs, qe, set_off, groups, v=0, rule=None, value_filter=None, min_overlap=None, gsupport=None):
        """group_support_sets(ichr, qs, qe, set_off, groups, v=0, rule=None, value_filter=None, min_overlap=None, gsupport=None).  Support counts per GROUP of datasets of many query sets in one call (igd_hip_group_support_sets).  Sets as
        search_sets(), groups a DatasetGroups.  Returns (gsupport int64[nsets, ngroups], gnhit int64[nsets]): gsupport[k, g] =
        the queries of set k that overlap a record of AT LEAST ONE dataset of group g -- a union over the group's datasets,
        neither the sum nor the maximum of their support_sets() columns -- and gnhit[k] = the queries of set k that overlap a
        dataset with at least one group.  One kernel counts it; no membership matrix is formed.  v, rule, value_filter and
        min_overlap as support_sets().  gsupport (int64[nsets, ngroups], C order) is added to when given."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "group_support_sets", "queries")
        g = _groups(groups, self.nfiles, "group_support_sets")
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        gsupport = _out(gsupport, (nsets, g.ngroups), np.int64, "gsupport", "group_support_sets", zero=True)
        gnhit = np.zeros(max(nsets, 1), np.int64)
        mo = _min_overlap(min_overlap, "group_support_sets")
        _chk(self._H.igd_hip_group_support_sets(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, _ptr(g.off),
                                                _ptr(g.idx), g.ngroups, vf, rule, _ptr(gsupport), _ptr(gnhit),
                                                C.byref(mo) if mo is not None else None), "igd_hip_group_support_sets")
        return gsupport, gnhit[:nsets]

    group_support_sets = _forward(_group_support_sets)

    def _group_support(self, ichr, qs, qe, groups, v=0, rule=None, value_filter=None, min_overlap=None):
        """group_support(ichr, qs, qe, groups, v=0, rule=None, value_filter=None, min_overlap=None).  Support counts per group of one query set: (int64[ngroups], gnhit).  Row 0 of group_support_sets() with one set."""
        sup, nhit = self.group_support_sets(ichr, qs, qe, np.array([0, len(_i32(qs))], np.int64), groups, v, rule, value_filter, min_overlap)
        return sup[0], int(nhit[0])

    group_support = _forward(_group_support)

    def group_support_files(self, paths, groups, v=0, min_overlap=None):
        """One query set per BED file (read as `igd search -q` reads it): (gsupport int64[len(paths), ngroups], gnhit)."""
        return self.group_support_sets(*self._read_sets(paths), groups, v, min_overlap=min_overlap)

    def _group_enrichment_sets(self, ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, groups, v=0, rule=None, value_filter=None, min_overlap=None,
                               with_nhit=False):
        """group_enrichment_sets(ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, groups, v=0, rule=None, value_filter=None,
        min_overlap=None, with_nhit=False).  Region-set enrichment per GROUP of datasets (igd_hip_group_enrich_sets): enrichment_sets() with the groups as columns.
        Returns Enrichment(support, usupport, b, c, d, pvalue_log, odds_ratio, clamped) with support = group_support_sets() of
        the sets, usupport that of the universe, arrays [nsets, ngroups], usupport [ngroups]; enrichment_ranks() ranks it as it
        is, over each set's groups.  with_nhit adds (gnhit int64[nsets], gunhit)."""
        what = "group_enrichment_sets"
        ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, nsets, nu = _restrict_args(ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, what)
        g = _groups(groups, self.nfiles, what)
        ng = g.ngroups
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        sup, usup = np.empty((nsets, ng), np.int64), np.empty(max(ng, 1), np.int64)
        plog, odds = np.empty((nsets, ng), np.float64), np.empty((nsets, ng), np.float64)
        clamped, nhit, unhit = np.empty(max(nsets, 1), np.int64), np.empty(max(nsets, 1), np.int64), C.c_int64(0)
        mo = _min_overlap(min_overlap, what)
        _chk(self._H.igd_hip_group_enrich_sets(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, _ptr(u_ichr), _ptr(u_qs),
                                               _ptr(u_qe), nu, _ptr(g.off), _ptr(g.idx), ng, vf, rule, _ptr(sup), _ptr(usup),
                                               _ptr(plog), _ptr(odds), _ptr(clamped), _ptr(nhit), C.byref(unhit),
                                               C.byref(mo) if mo is not None else None), "igd_hip_group_enrich_sets")
        usup = usup[:ng]
        nk = np.diff(set_off)[:, None]
        b = usup[None, :] - sup
        c = nk - sup
        d = nu - sup - b - c
        res = Enrichment(sup, usup, np.maximum(b, 0), c, np.maximum(d, 0), plog, odds, clamped[:nsets])
        return (res, nhit[:nsets], unhit.value) if with_nhit else res

    group_enrichment_sets = _forward(_group_enrichment_sets)

    def group_enrichment_files(self, paths, universe_path, groups, v=0, min_overlap=None):
        """One query set per BED file and the universe from a BED file: what `igd search -Q list -U universe -K groups` prints,
        as group_enrichment_sets() returns it."""
        sets = self._read_sets(paths)
        uni = self.read_queries(universe_path)
        return self.group_enrichment_sets(*sets, uni[0], uni[1], uni[2], groups, v, min_overlap=min_overlap)

    def coverage_sets(self, ichr, qs, qe, set_off, v=0, rule=None, value_filter=None, coverage=None):
        """Covered base pairs of many query sets in one call (igd_hip_coverage_sets).  Sets as search_sets().  Returns
        (coverage int64[nsets, nfiles], covered int64[nsets]): coverage[k, f] = summed over the queries of set k, the bp of
        the query that lie under at least one record of file f that the query counts (an interval union per query, not a
        sum over records), covered[k] = the same under the records of any file.  The sum runs over queries: two identical
        queries count twice and overlapping queries of one set are not merged -- merge the BED first for the set-level
        intersection.  coverage (int64[nsets, nfiles], C order) is added to when given."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "coverage_sets", "queries")
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        coverage = _out(coverage, (nsets, self.nfiles), np.int64, "coverage", "coverage_sets", zero=True)
        covered = np.zeros(max(nsets, 1), np.int64)
        _chk(self._H.igd_hip_coverage_sets(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, vf, rule, _ptr(coverage),
                                           _ptr(covered)), "igd_hip_coverage_sets")
        return coverage, covered[:nsets]

    def coverage(self, ichr, qs, qe, v=0, rule=None, value_filter=None):
        """Covered base pairs of one query set: (int64[nfiles], covered) -- per file the bp of the queries under its
        records, and the bp under the records of any file.  Row 0 of coverage_sets() with one set."""
        cov, covered = self.coverage_sets(ichr, qs, qe, np.array([0, len(_i32(qs))], np.int64), v, rule, value_filter)
        return cov[0], int(covered[0])

    def coverage_files(self, paths, v=0):
        """One query set per BED file (read as `igd search -q` reads it): (coverage int64[len(paths), nfiles], covered)."""
        return self.coverage_sets(*self._read_sets(paths), v)

    def fisher(self, a, b, c, d, pvalue_log=None, odds_ratio=None):
        """Fisher's exact test, one-sided ("greater"), of the 2x2 tables a b / c d on the GPU (igd_hip_fisher_tables).
        Returns (pvalue_log, odds_ratio), two float64 arrays: pvalue_log = -log10 P(X >= a) for X ~ Hypergeometric(a+b+c+d,
        a+b, a+c), computed in log space (finite however small p is, +0.0 where a is the support minimum), odds_ratio =
        (a d) / (b c), the sample odds ratio (inf when b c = 0 < a d, NaN when both are 0).  The output arrays, when given,
        are overwritten.  A negative entry or N >= 2^31 raises IgdError and leaves them untouched."""
        a, b, c, d = _tables(a, b, c, d, "fisher")
        n = len(a)
        p = _out(pvalue_log, (n,), np.float64, "pvalue_log", "fisher", words="a contiguous")
        o = _out(odds_ratio, (n,), np.float64, "odds_ratio", "fisher", words="a contiguous")
        _chk(self._H.igd_hip_fisher_tables(self.dev, _ptr(a), _ptr(b), _ptr(c), _ptr(d), n, _ptr(p), _ptr(o)), "igd_hip_fisher_tables")
        return p, o

    def enrichment_sets(self, ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, v=0, rule=None, value_filter=None, min_overlap=None):
        """Region-set enrichment of many query sets against a universe in one call (igd_hip_enrich_sets).  Sets as
        search_sets(); the universe is one more set of regions.  Returns Enrichment(support, usupport, b, c, d, pvalue_log,
        odds_ratio, clamped): per set k and file f the table a = support[k, f] (support_sets()), b = usupport[f] - a,
        c = |set k| - a, d = |universe| - a - b - c, where a negative b or d is then 0 and clamped[k] counts the cells of
        set k where that happened (enrichment_restricted() restricts the sets to the universe first); pvalue_log and odds_ratio as fisher()
        on these tables.  Arrays are [nsets, nfiles], usupport [nfiles], clamped [nsets].  Ranks and q-values: enrichment_ranks().
        min_overlap (a MinOverlap, or an int of base pairs; igd_hip_enrich_sets_ov): the supports of the sets AND of the
        universe are taken under it, as LOLA's runLOLA(minOverlap=) does."""
        ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, nsets, nu = _restrict_args(ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, "enrichment_sets")
        nf = self.nfiles
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        sup, usup = np.empty((nsets, nf), np.int64), np.empty(max(nf, 1), np.int64)
        plog, odds = np.empty((nsets, nf), np.float64), np.empty((nsets, nf), np.float64)
        clamped = np.empty(max(nsets, 1), np.int64)
        mo = _min_overlap(min_overlap, "enrichment_sets")
        a = (self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, _ptr(u_ichr), _ptr(u_qs), _ptr(u_qe), nu, vf, rule,
             _ptr(sup), _ptr(usup), _ptr(plog), _ptr(odds), _ptr(clamped))
        _chk(self._H.igd_hip_enrich_sets(*a) if mo is None else self._H.igd_hip_enrich_sets_ov(*a, None, None, C.byref(mo)),
             "igd_hip_enrich_sets")
        usup = usup[:nf]
        nk = np.diff(set_off)[:, None]
        b = usup[None, :] - sup
        c = nk - sup
        d = nu - sup - b - c
        return Enrichment(sup, usup, np.maximum(b, 0), c, np.maximum(d, 0), plog, odds, clamped[:nsets])

    def restrict_sets(self, ichr, qs, qe, set_off, u_ichr, u_qs, u_qe):
        """Query sets restricted to a universe (igd_hip_restrict_sets; LOLA's redefineUserSets).  Sets as search_sets(); the
        universe in any order.  Returns (bits uint32[nsets, ceil(nu / 32)], size int64[nsets]): universe region u (the
        caller's numbering) is bit u & 31 of bits[k, u >> 5] and is set iff some region q of set k has the same contig number
        >= 0, u_qs[u] < qe[q] and u_qe[u] > qs[q] -- the plain predicate: empty and inverted regions are not special-cased,
        regions that touch do not overlap, a contig number < 0 overlaps nothing.  size[k] = the set bits of row k."""
        ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, nsets, nu = _restrict_args(ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, "restrict_sets")
        bits, size = np.empty((nsets, (nu + 31) // 32), np.uint32), np.empty(max(nsets, 1), np.int64)
        _chk(self._H.igd_hip_restrict_sets(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, _ptr(u_ichr), _ptr(u_qs),
                                           _ptr(u_qe), nu, _ptr(bits), _ptr(size)), "igd_hip_restrict_sets")
        return bits, size[:nsets]

    def enrichment_restricted(self, ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, v=0, rule=None, value_filter=None, with_nhit=False):
        """Region-set enrichment with every set first restricted to the universe (igd_hip_enrich_restricted): set k is replaced
        by R_k, the universe regions it overlaps (restrict_sets()), so each table is a true partition of the universe.  Returns
        RestrictedEnrichment(support, usupport, b, c, d, pvalue_log, odds_ratio, size, bits): with member = membership() of the
        universe regions, usupport[f] = its column sums, support[k, f] = the sum over R_k, a = support, b = usupport - a,
        c = size[k] - a, d = |universe| - usupport - c, all >= 0 (nothing is clamped); pvalue_log and odds_ratio as fisher() on
        these tables -- bit for bit what enrichment_sets() returns for R_k given as explicit regions.  Regions whose contig
        number is < 0 (read_queries() drops lines on contigs the database does not know) are in no restricted set.
        with_nhit adds (nhit int64[nsets], unhit): the regions of R_k / of the universe with a hit in any file."""
        ichr, qs, qe, set_off, u_ichr, u_qs, u_qe, nsets, nu = _restrict_args(ichr, qs, qe, set_off, u_ichr, u_qs, u_qe,
                                                                              "enrichment_restricted")
        nf = self.nfiles
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        sup, usup = np.empty((nsets, nf), np.int64), np.empty(max(nf, 1), np.int64)
        plog, odds = np.empty((nsets, nf), np.float64), np.empty((nsets, nf), np.float64)
        size, nhit, unhit = np.empty(max(nsets, 1), np.int64), np.empty(max(nsets, 1), np.int64), C.c_int64(0)
        bits = np.empty((nsets, (nu + 31) // 32), np.uint32)
        _chk(self._H.igd_hip_enrich_restricted(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, _ptr(u_ichr), _ptr(u_qs),
                                               _ptr(u_qe), nu, vf, rule, _ptr(sup), _ptr(usup), _ptr(size), _ptr(plog), _ptr(odds),
                                               _ptr(bits), _ptr(nhit), C.byref(unhit)), "igd_hip_enrich_restricted")
        res = _restricted_result(sup, usup[:nf], size[:nsets], plog, odds, bits, nu)
        return (res, nhit[:nsets], unhit.value) if with_nhit else res

    def enrichment_restricted_files(self, paths, universe_path, v=0):
        """One query set per BED file and the universe from a BED file (read as `igd search -q` reads them): what
        `igd search -Q list -U universe -X` prints, as enrichment_restricted() returns it."""
        sets = self._read_sets(paths)
        uni = self.read_queries(universe_path)
        return self.enrichment_restricted(*sets, uni[0], uni[1], uni[2], v)

    @staticmethod
    def unpack_restricted(bits, nu):
        """bool[nsets, nu] from the rows of restrict_sets() / RestrictedEnrichment.bits"""
        return Database.unpack_membership(bits, nu)

    def enrichment_ranks(self, support, pvalue_log=None, odds_ratio=None):
        """Rank columns and q-values of an enrichment table on the GPU (igd_hip_enrich_ranks): three [nsets, ncols] arrays,
        or one Enrichment / RestrictedEnrichment.  Per row (query set) and within it: rnk_sup, rnk_pv, rnk_or = 1 + the cells of the row with a
        larger support / pvalue_log / odds_ratio (ties take the minimum rank; +inf is the largest odds ratio, NaN ranks
        below every number), max_rnk their maximum, mean_rnk their mean (float64, not rounded), and qvalue_log = -log10 of
        the Benjamini-Hochberg adjusted p over the row's ncols tests, computed in log10 (no underflow), >= +0.0.  The
        number of columns is free (at most 2^20).  Returns EnrichmentRanks(qvalue_log, rnk_sup, rnk_pv, rnk_or, max_rnk,
        mean_rnk), arrays of the inputs' shape.  The family is the row: no whole-table correction, no Storey q-value."""
        s, p, o = _rank_inputs(support, pvalue_log, odds_ratio, "enrichment_ranks")
        r = _rank_outputs(s.shape)
        _chk(self._H.igd_hip_enrich_ranks(self.dev, _ptr(s), _ptr(p), _ptr(o), s.shape[0], s.shape[1], *[_ptr(x) for x in r]),
             "igd_hip_enrich_ranks")
        return r

    def enrichment_files(self, paths, universe_path, v=0, min_overlap=None):
        """One query set per BED file and the universe from a BED file (read as `igd search -q` reads them): what
        `igd search -Q list -U universe` prints, as enrichment_sets() returns it."""
        sets = self._read_sets(paths)
        uni = self.read_queries(universe_path)
        return self.enrichment_sets(*sets, uni[0], uni[1], uni[2], v, min_overlap=min_overlap)

    @property
    def member_words(self):
        """uint32 words of one membership row: ceil(nfiles / 32)"""
        return int(self._H.igd_hip_member_words(self.dev))

    def membership(self, ichr, qs, qe, v=0, rule=None, value_filter=None, bits=None):
        """Per-query dataset membership (igd_hip_membership).  Returns (bits uint32[nq, member_words], nfiles_hit int32[nq],
        nhit): file f is bit f & 31 of bits[q, f >> 5] and is set iff query q overlaps at least one record of file f (bits at
        positions >= nfiles are 0), nfiles_hit[q] = the files query q overlaps, nhit = the queries that overlap any -- the
        matrix whose column sums are support().  bits (uint32[nq, member_words], C order), when given, is overwritten:
        every word of it, so it need not be cleared."""
        ichr, qs, qe = _regions(ichr, qs, qe, "membership", "queries")
        nq, nW = len(qs), self.member_words
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        bits = _out(bits, (nq, nW), np.uint32, "bits", "membership")
        nfh = np.empty(nq, np.int32)
        nhit = C.c_int64(0)
        _chk(self._H.igd_hip_membership(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), nq, vf, rule, _ptr(bits), _ptr(nfh), C.byref(nhit)),
             "igd_hip_membership")
        return bits, nfh, nhit.value

    def cooccurrence(self, ichr, qs, qe, v=0, rule=None, value_filter=None, cooc=None):
        """Dataset x dataset co-occurrence over one region list (igd_hip_cooccur).  Returns (cooc int64[nfiles, nfiles], nhit):
        with member = unpack_membership(membership(...)), cooc[f, g] = the regions q with member[q, f] and member[q, g] --
        symmetric, its diagonal is support() -- and nhit = the regions that overlap any file.  Two identical regions count
        twice; no region gives a zero matrix.  cooc (int64[nfiles, nfiles], C order), when given, is overwritten: every cell
        of it.  The membership rows never leave the device.  More than 16 384 files raise IgdError.  jaccard() turns the
        matrix into the Jaccard index."""
        ichr, qs, qe = _regions(ichr, qs, qe, "cooccurrence")
        nq, nf = len(qs), self.nfiles
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        cooc = _out(cooc, (nf, nf), np.int64, "cooc", "cooccurrence")
        nhit = C.c_int64(0)
        _chk(self._H.igd_hip_cooccur(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), nq, vf, rule, _ptr(cooc), C.byref(nhit)), "igd_hip_cooccur")
        return cooc, nhit.value

    def cooccurrence_files(self, path, v=0):
        """The co-occurrence over the regions of one BED file (read as `igd search -q` reads it): what `igd search -q path -C`
        prints, as cooccurrence() returns it."""
        return self.cooccurrence(*self.read_queries(path), v)

    def transpose_bits(self, bits, cols=None):
        """Bit rows into bit columns on the GPU (igd_hip_bits_transpose): bits is uint32[nrows, nW] in the layout of
        membership(); returns uint64[32 * nW, ceil(nrows / 64)] where row r is bit r & 63 of cols[c, r >> 6], c = 32 * w + the
        bit's position in word w.  Every word is defined; bits at positions >= nrows are 0.  cols, when given, is overwritten."""
        bits = _bitrows(bits, "bits", "transpose_bits")
        nrows, nW = bits.shape
        shape = (32 * nW, (nrows + 63) // 64)
        cols = _out(cols, shape, np.uint64, "cols", "transpose_bits")
        _chk(self._H.igd_hip_bits_transpose(self.dev, _ptr(bits), nrows, nW, _ptr(cols)), "igd_hip_bits_transpose")
        return cols

    def bitrows_gram(self, a, b=None, out=None):
        """Popcount Gram product of bit rows on the GPU (igd_hip_bitrows_gram): a is uint32[m, nwords], b uint32[n, nwords];
        returns int64[m, n] with out[i, j] = popcount(a[i] & b[j]).  b=None is the symmetric form (b = a): only the tiles on
        and above the diagonal are computed.  With the bits of restrict_sets() it is the set x set overlap matrix.  out,
        when given, is overwritten: every cell of it."""
        a = _bitrows(a, "a", "bitrows_gram")
        b = None if b is None else _bitrows(b, "b", "bitrows_gram")
        if b is not None and b.shape[1] != a.shape[1]:
            raise IgdError("bitrows_gram: rows of %d and of %d words" % (a.shape[1], b.shape[1]))
        m, n = a.shape[0], a.shape[0] if b is None else b.shape[0]
        out = _out(out, (m, n), np.int64, "out", "bitrows_gram")
        pb = None if b is None else (b.ctypes.data if b.size else a.ctypes.data)
        _chk(self._H.igd_hip_bitrows_gram(self.dev, _ptr(a), m, pb, n, a.shape[1], _ptr(out)), "igd_hip_bitrows_gram")
        return out

    def permutation_support(self, ichr, qs, qe, ctg_len, nperm, seed=0, mode="circular", v=0, rule=None, value_filter=None,
                            min_overlap=None, workspace=None, universe=None):
        """Permutation null of the support counts of one region set (igd_hip_permute_support).  The set is moved nperm times
        -- mode "circular": one rigid shift per permutation and contig, a region that would cross the contig's end is pushed
        back against it; "shuffle": every region placed anew on its contig -- with the generator of include/igd_hip.h; every
        permuted set is counted as support() counts.  ctg_len: int32[nctg], the contig lengths in the database's contig
        order (read_genome()).  Returns PermutationSupport(observed, sum, sumsq, n_ge, n_le, min, max, nperm), int64[nfiles + 1]
        each: the support as given, and over the permuted supports x their sum, sum of squares, the permutations with
        x >= observed and x <= observed, the smallest and the largest; index nfiles is the regions with a hit in any file.
        The permuted regions and the permutations x files matrix never leave the device.  perm_summary() gives mean, sd, z
        and p.  A region on a known contig that does not lie within its length raises IgdError.  min_overlap (a MinOverlap, or
        an int of base pairs; igd_hip_permute_support_ov): the observed row and every permuted row are counted under it.
        mode "workspace" together with workspace= (a Workspace): every region is placed anew inside the segments of the
        workspace on its contig, every fitting start equally likely (igd_hip_permute_support_ws); a region that fits in no
        segment raises IgdError.  The same pair of arguments serves permutation_nearest(), permutation_bp() and
        permute_regions().
        mode "resample" together with universe=(ichr, qs, qe) and ctg_len None (igd_hip_permute_support_rs; regioneR's
        resampleRegions): every permuted set is len(qs) regions drawn without replacement from the universe, contigs, starts
        and ends as they stand; nothing is placed, so there are no contig lengths and no workspace, and the set need not be
        a subset of the universe.  Each permuted support is then hypergeometric.  A set larger than the universe raises
        IgdError.  The same pair serves permutation_nearest() and permutation_bp()."""
        P = _placement(ichr, qs, qe, ctg_len, mode, workspace, universe, "permutation_support")
        _placement_fits(P, self.nctg, "permutation_support")
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        out = [np.empty(self.nfiles + 1, np.int64) for _ in range(7)]
        mo = _min_overlap(min_overlap, "permutation_support")
        a = (self.dev, _ptr(P.ichr), _ptr(P.qs), _ptr(P.qe), len(P.qs), *P.mid, _seed(seed), int(nperm), vf, rule, *[_ptr(x) for x in out])
        _chk(getattr(self._H, "igd_hip_permute_support" + P.sfx)(*a, None if mo is None else C.byref(mo), *P.tail),
             "igd_hip_permute_support" + P.sfx.replace("_ws", ""))
        return PermutationSupport(*out, int(nperm))

    def read_genome(self, path):
        """int32[nctg]: the contig lengths of a genome file (`name<TAB>length` per line) in the database's contig order; 0 for
        a contig the file does not name."""
        ln = np.zeros(max(self.nctg, 1), np.int32)
        bad = C.c_int64(0)
        rc = self._L.igdc_read_genome(self._core, path.encode(), _ptr(ln), C.byref(bad))
        if rc == -1:
            raise IOError("cannot open genome file %s" % path)
        if rc != 0:
            raise IgdError("genome file %s, line %d: not a name, a tab and a length of at most 2147483647" % (path, bad.value))
        return ln[:self.nctg]

    def read_workspace(self, path, ctg_len):
        """The Workspace of a BED file (read as `igd search -q` reads a query file; lines on contigs the database lacks are
        skipped) on the database's contigs of lengths ctg_len (read_genome()): igdc_read_workspace."""
        ctg_len = _i32(ctg_len)
        _ctg_len_matches(ctg_len, self.nctg, "read_workspace")
        t = C.POINTER(N.HipWorkspace)()
        rc = self._L.igdc_read_workspace(self._core, path.encode(), _ptr(ctg_len), C.byref(t))
        if rc == -1:
            raise IOError("cannot open workspace file %s" % path)
        if rc != 0:
            raise IgdError("read_workspace: the table of %s could not be built" % path)
        return Workspace(t, ctg_len)

    def _genome_or_universe(self, genome_path, universe_path):
        """(ctg_len, universe) of a _files call: the lengths of a genome file, or -- mode "resample", genome_path None -- the regions
        of a universe file, read as enrichment_files() reads one"""
        return (None if genome_path is None else self.read_genome(genome_path),
                None if universe_path is None else self.read_queries(universe_path))

    def permutation_support_files(self, path, genome_path, nperm, seed=0, mode="circular", v=0, min_overlap=None, workspace=None,
                                  universe_path=None):
        """The permutation null of one BED file (read as `igd search -q` reads it) with the lengths of a genome file: the
        integers behind what `igd search -q path -P nperm -g genome_path` prints (with -W: mode="workspace" and workspace=; with
        -M resample -U universe_path: mode="resample", universe_path= and genome_path None)."""
        ctg_len, uni = self._genome_or_universe(genome_path, universe_path)
        return self.permutation_support(*self.read_queries(path), ctg_len, nperm, seed, mode, v, min_overlap=min_overlap,
                                        workspace=workspace, universe=uni)

    def _resample_regions(self, ichr, qs, qe, nq, p0, np_, seed=0):
        """resample_regions(ichr, qs, qe, nq, p0, np_, seed=0).  Kernel igd_resample_regions on host arrays
        (igd_hip_resample_regions): (ichr, qs, qe) int32[np_, nq], row k the nq regions of draw p0 + k from the pool (ichr, qs,
        qe) -- pool region igd_hip_resample_index(base(seed, p0 + k), i, npool) for i = 0 .. nq - 1, distinct within a row.  nq
        above the pool's size raises IgdError."""
        pool = _regions(ichr, qs, qe, "resample_regions", "universe regions")
        if int(np_) < 0 or int(nq) < 0:
            raise IgdError("resample_regions: a negative size")
        out = [np.empty((int(np_), int(nq)), np.int32) for _ in range(3)]
        _chk(self._H.igd_hip_resample_regions(self.dev, *_pool_args(pool), int(nq), _seed(seed), int(p0), int(np_), *[_ptr(a) for a in out]),
             "igd_hip_resample_regions")
        return tuple(out)

    resample_regions = _forward(_resample_regions)

    def _shift_support(self, ichr, qs, qe, ctg_len, offsets, v=0, rule=None, value_filter=None, min_overlap=None):
        """shift_support(ichr, qs, qe, ctg_len, offsets, v=0, rule=None, value_filter=None, min_overlap=None).  The support counts
        of one region set under rigid shifts (igd_hip_shift_support; regioneR's localZScore).  The whole set is moved by each of
        offsets (1 .. 4096 whole numbers within +-2^30, any order; shift_offsets() makes the usual ladder); a region that would
        leave its contig is pushed back against the end, its width kept; regions on unknown contigs stay.  ctg_len as
        permutation_support().  Returns ShiftSupport(shifted, offsets): shifted int64[nshift, nfiles + 1], row j what support()
        counts for the set moved by offsets[j] (same v, rule, value_filter and min_overlap), the last column the regions with a
        hit in any file.  The shifted regions never leave the device.  local_zscore() places the rows in the null of
        permutation_support().  A region on a known contig that does not lie within its length raises IgdError."""
        ichr, qs, qe, ctg_len = _perm_regions(ichr, qs, qe, ctg_len, "shift_support")
        offsets = _offsets(offsets, "shift_support")
        _ctg_len_matches(ctg_len, self.nctg, "shift_support")
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        mo = _min_overlap(min_overlap, "shift_support")
        shifted = np.empty((len(offsets), self.nfiles + 1), np.int64)
        _chk(self._H.igd_hip_shift_support(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), _ptr(ctg_len), _ptr(offsets), len(offsets),
                                           vf, rule, _ptr(shifted), None if mo is None else C.byref(mo)), "igd_hip_shift_support")
        return ShiftSupport(shifted, offsets)

    shift_support = _forward(_shift_support)

    def _shift_regions(self, ichr, qs, qe, ctg_len, offsets):
        """shift_regions(ichr, qs, qe, ctg_len, offsets).  Kernel igd_shift_regions on host arrays (igd_hip_shift_regions): (qs,
        qe) int32[nshift, nq], row j the regions moved by offsets[j].  ctg_len is the caller's, as for permute_regions()."""
        ichr, qs, qe, ctg_len = _perm_regions(ichr, qs, qe, ctg_len, "shift_regions")
        offsets = _offsets(offsets, "shift_regions")
        oqs, oqe = np.empty((len(offsets), len(qs)), np.int32), np.empty((len(offsets), len(qs)), np.int32)
        _chk(self._H.igd_hip_shift_regions(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), _ptr(ctg_len), len(ctg_len), _ptr(offsets),
                                           len(offsets), _ptr(oqs), _ptr(oqe)), "igd_hip_shift_regions")
        return oqs, oqe

    shift_regions = _forward(_shift_regions)

    def shift_support_files(self, path, genome_path, offsets, v=0, min_overlap=None):
        """The shift profile of one BED file (read as `igd search -q` reads it) with the lengths of a genome file: the integers
        that `igd search -q path -g genome_path -Z W,STEP` prints for offsets = shift_offsets(W, STEP)."""
        return self.shift_support(*self.read_queries(path), self.read_genome(genome_path), offsets, v, min_overlap=min_overlap)

    def permute_regions(self, ichr, qs, qe, ctg_len, p0, np_, seed=0, mode="circular", workspace=None):
        """Kernel igd_permute_regions on host arrays (igd_hip_permute_regions): (qs, qe) int32[np_, nq], row k the regions
        under permutation p0 + k.  ctg_len is the caller's: len(ctg_len) contigs, not tied to the database; a region with
        ichr outside [0, len(ctg_len)) passes through unchanged."""
        ichr, qs, qe, ctg_len = _perm_regions(ichr, qs, qe, ctg_len, "permute_regions")
        pm = _perm_mode(mode, "permute_regions", workspace)
        oqs, oqe = np.empty((int(np_), len(qs)), np.int32), np.empty((int(np_), len(qs)), np.int32)
        _chk(self._H.igd_hip_permute_regions_ws(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), len(qs), _ptr(ctg_len), len(ctg_len),
                                                pm, _seed(seed), int(p0), int(np_), _ptr(oqs), _ptr(oqe), _ws_ptr(workspace)),
             "igd_hip_permute_regions")
        return oqs, oqe

    def perm_stats(self, rows, observed, out=None):
        """Kernel igd_perm_stats on host arrays (igd_hip_perm_stats): rows int64[nrows, ncols], observed int64[ncols]; returns
        (sum, sumsq, n_ge, n_le, min, max), int64[ncols] each, over the rows of every column.  out, when given, is a list of
        six int64[ncols] arrays that are overwritten."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        observed = np.ascontiguousarray(observed, dtype=np.int64)
        if rows.ndim != 2 or observed.shape != (rows.shape[1],):
            raise IgdError("perm_stats: rows must be int64[nrows, ncols] and observed int64[ncols]")
        out = _outs(out, 6, (rows.shape[1],), "perm_stats")
        _chk(self._H.igd_hip_perm_stats(self.dev, _ptr(rows), rows.shape[0], rows.shape[1], _ptr(observed),
                                        *[_ptr(a) for a in out]), "igd_hip_perm_stats")
        return tuple(out)

    def membership_files(self, paths, v=0):
        """The rows of several BED files (read as `igd search -q` reads them), concatenated: (bits, nfiles_hit, nhit
        int64[len(paths)], set_off int64[len(paths) + 1]); file k owns the rows [set_off[k], set_off[k + 1])."""
        ichr, qs, qe, set_off = self._read_sets(paths)
        bits, nfh, _ = self.membership(ichr, qs, qe, v)
        any_hit = np.concatenate([[0], np.cumsum(nfh > 0)]).astype(np.int64)
        return bits, nfh, any_hit[set_off[1:]] - any_hit[set_off[:-1]], set_off

    # ---- nearest record per dataset within a window ---------------------------------------
    def nearest(self, ichr, qs, qe, window, value_filter=None, dist=None):
        """How far each region lies from the nearest record of every dataset within `window` bp (igd_hip_nearest; the
        definitions are in include/igd_hip.h): (dist int32[nq, nfiles], dmin int32[nq]).  dist[q, f] is 0 where region q
        overlaps a record of file f, the gap + 1 otherwise (book-ended intervals are 1 bp apart), -1 where file f has no record
        within the window; dmin[q] is the smallest of the row's distances, or -1.  value_filter: only records with value >=
        it count (the nearest passing record).  There is no tile rule.  dist (int32[nq, nfiles], C order), when given, is
        overwritten: every word is defined by the call."""
        ichr, qs, qe = _regions(ichr, qs, qe, "nearest")
        nq = len(qs)
        dist = _out(dist, (nq, self.nfiles), np.int32, "dist", "nearest")
        dmin = np.empty(nq, np.int32)
        _chk(self._H.igd_hip_nearest(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), nq, _window(window, "nearest"), _value_filter(value_filter),
                                     _ptr(dist), _ptr(dmin)), "igd_hip_nearest")
        return dist, dmin

    def nearest_sets(self, ichr, qs, qe, set_off, window, value_filter=None, out=None):
        """The distances of nearest() summed up per region set (igd_hip_nearest_sets; sets as search_sets()): a NearestSets of
        three int64[nsets, nfiles + 1] -- n_within (the regions of the set with a record of the file within the window),
        n_overlap (those that overlap one: the support under rule FLAT) and sum_dist (the sum of the former's distances) --
        whose last column is the any-dataset column, built from dmin.  The distance rows never leave the device.  out, when
        given, is a list of three C-ordered int64[nsets, nfiles + 1] that are overwritten."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "nearest_sets")
        out = _outs(out, 3, (nsets, self.nfiles + 1), "nearest_sets")
        _chk(self._H.igd_hip_nearest_sets(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, _window(window, "nearest_sets"),
                                          _value_filter(value_filter), *[_ptr(a) for a in out]), "igd_hip_nearest_sets")
        return NearestSets(*out, int(window))

    def nearest_sets_fused(self, ichr, qs, qe, set_off, window, value_filter=None, out=None):
        """nearest_sets() through the fused kernel (igd_hip_nearest_sets_fused, kernel igd_nearest_slices): the same NearestSets,
        every integer, without distance rows in device memory.  Databases with more files than igd_hip_nearest_fused_max_files()
        take nearest_sets()'s route.  out, when given, is a list of three C-ordered int64[nsets, nfiles + 1] that are
        overwritten."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "nearest_sets_fused")
        out = _outs(out, 3, (nsets, self.nfiles + 1), "nearest_sets_fused")
        _chk(self._H.igd_hip_nearest_sets_fused(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets,
                                                _window(window, "nearest_sets_fused"), _value_filter(value_filter), *[_ptr(a) for a in out]),
             "igd_hip_nearest_sets_fused")
        return NearestSets(*out, int(window))

    def nearest_fused_files(self, paths, window, value_filter=None):
        """One region set per BED file (read as `igd search -q` reads it): the NearestSets of nearest_sets_fused()."""
        return self.nearest_sets_fused(*self._read_sets(paths), window, value_filter)

    def permutation_nearest(self, ichr, qs, qe, ctg_len, nperm, window, seed=0, mode="circular", value_filter=None, out=None, workspace=None,
                            universe=None):
        """Permutation null of the nearest-record distances of one region set (igd_hip_permute_nearest): "are my regions closer
        to dataset f than chance".  The set is moved nperm times as permutation_support() moves it (same generator, mode, seed
        and ctg_len) and every permuted set is measured as nearest_sets() measures a set.  Returns PermutationNearest(n_within,
        n_overlap, sum_dist, window, nperm), int64[nperm + 1, nfiles + 1] each: row 0 the set as given, row p + 1 permutation
        p, the last column the any-dataset column.  The null distribution itself comes back -- the mean distance
        sum_dist / n_within is a ratio of two columns that both vary -- and perm_nearest_summary() places the observed row
        in it.  Neither the permuted regions nor any distance row leave the device.  out, when given, is a list of three
        C-ordered int64[nperm + 1, nfiles + 1] that are overwritten (untouched when the call raises).  mode "resample" with
        universe= and ctg_len None as permutation_support() takes them (igd_hip_permute_nearest_rs): "are my regions closer
        to dataset f than other regions of the universe"."""
        P = _placement(ichr, qs, qe, ctg_len, mode, workspace, universe, "permutation_nearest")
        _placement_fits(P, self.nctg, "permutation_nearest")
        out = _outs(out, 3, (max(int(nperm), 0) + 1, self.nfiles + 1), "permutation_nearest")
        _chk(getattr(self._H, "igd_hip_permute_nearest" + P.sfx)(self.dev, _ptr(P.ichr), _ptr(P.qs), _ptr(P.qe), len(P.qs), *P.mid, _seed(seed),
                                                                 int(nperm), _window(window, "permutation_nearest"), _value_filter(value_filter),
                                                                 *[_ptr(a) for a in out], *P.tail),
             "igd_hip_permute_nearest" + P.sfx.replace("_ws", ""))
        return PermutationNearest(*out, int(window), int(nperm))

    def permutation_nearest_files(self, path, genome_path, nperm, window, seed=0, mode="circular", value_filter=None, workspace=None,
                                  universe_path=None):
        """The null of one BED file (read as `igd search -q` reads it) with the lengths of a genome file: the integers behind
        what `igd search -q path -P nperm -g genome_path -D window` prints (mode="resample": universe_path=, genome_path None)."""
        ctg_len, uni = self._genome_or_universe(genome_path, universe_path)
        return self.permutation_nearest(*self.read_queries(path), ctg_len, nperm, window, seed, mode, value_filter,
                                        workspace=workspace, universe=uni)

    def nearest_files(self, paths, window, value_filter=None):
        """One region set per BED file (read as `igd search -q` reads it): the NearestSets of nearest_sets()."""
        return self.nearest_sets(*self._read_sets(paths), window, value_filter)

    def nearest_dev(self, d_ichr, d_qs, d_qe, nq, window, d_dist, d_dmin=None, value_filter=None, stream=None):
        """Resident batch: arguments are device pointers (ints).  Asynchronous.  d_dist (int32[nq * nfiles]) and d_dmin
        (int32[nq], may be None) are overwritten.  nq above igd_hip_max_batch() is refused: split the batch."""
        _chk(self._H.igd_hip_nearest_dev(self.dev, d_ichr, d_qs, d_qe, int(nq), _window(window, "nearest_dev"), _value_filter(value_filter),
                                         d_dist, d_dmin, stream), "igd_hip_nearest_dev")

    # ---- signed nearest distances and their histogram -------------------------------------
    def nearest_signed(self, ichr, qs, qe, window, value_filter=None, sdist=None):
        """nearest() with a side (igd_hip_nearest_signed; the definitions are in include/igd_hip.h): (sdist int32[nq, nfiles],
        sdmin int32[nq]).  sdist[q, f] is 0 where region q overlaps a record of file f, -d where the nearest record within the
        window lies upstream (at lower coordinates) and +d where it lies downstream, d being nearest()'s distance; at equal d on
        both sides upstream wins; NEAREST_NO_RECORD (-2^31) where file f has no record within the window.  sdmin[q] is the
        row's entry of smallest d, decided the same way.  sdist (int32[nq, nfiles], C order), when given, is overwritten."""
        ichr, qs, qe = _regions(ichr, qs, qe, "nearest_signed")
        nq = len(qs)
        sdist = _out(sdist, (nq, self.nfiles), np.int32, "sdist", "nearest_signed")
        sdmin = np.empty(nq, np.int32)
        _chk(self._H.igd_hip_nearest_signed(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), nq, _window(window, "nearest_signed"),
                                            _value_filter(value_filter), _ptr(sdist), _ptr(sdmin)), "igd_hip_nearest_signed")
        return sdist, sdmin

    def nearest_hist(self, ichr, qs, qe, set_off, window, edges, value_filter=None, hist=None):
        """The histogram of nearest_signed()'s distances per region set and dataset (igd_hip_nearest_hist; sets as
        search_sets()): NearestHist(hist, edges, window) with hist int64[nsets, len(edges) + 1, nfiles + 1].  edges are 1 to
        63 strictly ascending int32 values; bin b counts the regions whose signed distance x has exactly b edges <= x (bin 0:
        below edges[0], the last bin: at or above edges[-1]); the last column is the any-dataset column, built from sdmin.
        Regions without a record within the window are in no bin: hist.sum(axis=1) is nearest_sets().n_within.  The distance
        rows never leave the device.  hist, when given (C order), is overwritten."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "nearest_hist")
        edges = _edges(edges, "nearest_hist")
        shape = (nsets, len(edges) + 1, self.nfiles + 1)
        hist = _out(hist, shape, np.int64, "hist", "nearest_hist")
        _chk(self._H.igd_hip_nearest_hist(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, _window(window, "nearest_hist"),
                                          _value_filter(value_filter), _ptr(edges), len(edges), _ptr(hist)), "igd_hip_nearest_hist")
        return NearestHist(hist, edges, int(window))

    def nearest_hist_files(self, paths, window, edges, value_filter=None):
        """One region set per BED file (read as `igd search -q` reads it): the NearestHist of nearest_hist()."""
        return self.nearest_hist(*self._read_sets(paths), window, edges, value_filter)

    def nearest_signed_dev(self, d_ichr, d_qs, d_qe, nq, window, d_sdist, d_sdmin=None, value_filter=None, stream=None):
        """Resident batch: arguments are device pointers (ints).  Asynchronous.  d_sdist (int32[nq * nfiles]) and d_sdmin
        (int32[nq], may be None) are overwritten.  nq above igd_hip_max_batch() is refused: split the batch."""
        _chk(self._H.igd_hip_nearest_signed_dev(self.dev, d_ichr, d_qs, d_qe, int(nq), _window(window, "nearest_signed_dev"),
                                                _value_filter(value_filter), d_sdist, d_sdmin, stream), "igd_hip_nearest_signed_dev")

    # ---- flanking records per dataset and the relative-distance histogram ------------------
    def flanks(self, ichr, qs, qe, window, measure="midpoints", value_filter=None, up=None, down=None):
        """The nearest record of every dataset on EACH side of every region within `window` base pairs (igd_hip_flank; the
        definitions are in include/igd_hip.h): (up, down int32[nq, nfiles], upmin, downmin int32[nq]), -1 where there is none.
        measure "edges": distances as nearest()'s, between the region and the record, a record that overlaps the region is on
        neither side (`bedtools closest -D ref -io -iu` / `-id`); "midpoints": between integer midpoints, an equal midpoint
        counts as downstream at distance 0 (`bedtools reldist`).  Upstream means lower coordinates.  upmin / downmin are the
        minima over the datasets.  up and down (int32[nq, nfiles], C order), when given, are overwritten."""
        ichr, qs, qe = _regions(ichr, qs, qe, "flanks")
        nq = len(qs)
        rows = [_out(r, (nq, self.nfiles), np.int32, name, "flanks") for name, r in (("up", up), ("down", down))]
        upmin, downmin = np.empty(nq, np.int32), np.empty(nq, np.int32)
        _chk(self._H.igd_hip_flank(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), nq, _window(window, "flanks"), _measure(measure, "flanks"),
                                   _value_filter(value_filter), _ptr(rows[0]), _ptr(rows[1]), _ptr(upmin), _ptr(downmin)), "igd_hip_flank")
        return rows[0], rows[1], upmin, downmin

    def flanks_dev(self, d_ichr, d_qs, d_qe, nq, window, d_up, d_down, d_upmin=None, d_downmin=None, measure="midpoints",
                   value_filter=None, stream=None):
        """Resident batch: arguments are device pointers (ints).  Asynchronous.  d_up and d_down (int32[nq * nfiles]) and d_upmin,
        d_downmin (int32[nq], each may be None) are overwritten.  nq above igd_hip_max_batch() is refused: split the batch."""
        _chk(self._H.igd_hip_flank_dev(self.dev, d_ichr, d_qs, d_qe, int(nq), _window(window, "flanks_dev"), _measure(measure, "flanks_dev"),
                                       _value_filter(value_filter), d_up, d_down, d_upmin, d_downmin, stream), "igd_hip_flank_dev")

    def flank_reldist(self, ichr, qs, qe, set_off, window, nbins=50, measure="midpoints", value_filter=None, hist=None):
        """The histogram of the relative distance per region set and dataset (igd_hip_flank_reldist; sets as search_sets();
        `bedtools reldist`): FlankReldist(hist, nbins, window, measure) with hist int64[nsets, nbins, nfiles + 1].  A region
        that has a record of dataset f on both sides within the window (flanks(): up >= 0, down >= 0, up + down > 0) is counted
        in bin min(nbins - 1, floor(2 nbins min(up, down) / (up + down))) of column f: flat under independence, piled at 0 under
        association.  The last column is the any-dataset column, built from upmin / downmin.  hist.sum(axis=1) is the number
        of flanked regions (igd_amd.reldist_summary gives the fractions).  The rows never leave the device.  hist, when given
        (C order), is overwritten."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "flank_reldist")
        nbins, m = _nbins(nbins, "flank_reldist"), _measure(measure, "flank_reldist")
        hist = _out(hist, (nsets, nbins, self.nfiles + 1), np.int64, "hist", "flank_reldist")
        _chk(self._H.igd_hip_flank_reldist(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, _window(window, "flank_reldist"),
                                           m, _value_filter(value_filter), nbins, _ptr(hist)), "igd_hip_flank_reldist")
        return FlankReldist(hist, nbins, int(window), m)

    def flank_reldist_files(self, paths, window, nbins=50, measure="midpoints", value_filter=None):
        """One region set per BED file (read as `igd search -q` reads it): the FlankReldist of flank_reldist()."""
        return self.flank_reldist(*self._read_sets(paths), window, nbins, measure, value_filter)

    # ---- merged region sets and the base-pair Jaccard per set and dataset -------------------
    def merge_sets(self, ichr, qs, qe, set_off, gap=0):
        """Region sets merged on the device as `bedtools merge -d gap` (igd_hip_merge_sets; the definitions are in
        include/igd_hip.h; sets as search_sets()): (ichr, qs, qe, set_off, count, n_dropped) -- the runs ordered by (set, ichr, qs),
        their offsets per set (int64[nsets + 1]), the regions each run joined (int32) and per set the regions that were dropped
        (unknown contig, zero length, inverted; int64[nsets]).  At gap 0 book-ended regions join.  The order of the regions
        within a set does not matter."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "merge_sets")
        gap = _gap(gap, "merge_sets")
        out = _merge_out(len(qs), nsets)
        _chk(self._H.igd_hip_merge_sets(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, gap, *[_ptr(a) for a in out]),
             "igd_hip_merge_sets")
        return _merge_cut(*out)

    def merge_sets_dev(self, d_ichr, d_qs, d_qe, d_set_off, nsets, n, d_m_ichr, d_m_qs, d_m_qe, d_m_off, d_n_dropped, d_m_count=None,
                       gap=0, stream=None):
        """Resident sets: arguments are device pointers (ints), n the number of regions.  Asynchronous.  d_m_ichr, d_m_qs, d_m_qe
        and d_m_count (int32[n]; the last may be None), d_m_off (int64[nsets + 1]) and d_n_dropped (int64[nsets]) are
        overwritten, the words behind the last run with 0; d_m_off[nsets], read back by the caller, is the number of runs.  The
        merges of one Database share one workspace: order them with respect to each other (one stream, or an event between two
        streams) -- two in flight on different streams race."""
        _chk(self._H.igd_hip_merge_sets_dev(self.dev, d_ichr, d_qs, d_qe, d_set_off, int(nsets), int(n), _gap(gap, "merge_sets_dev"),
                                            d_m_ichr, d_m_qs, d_m_qe, d_m_off, d_m_count, d_n_dropped, stream), "igd_hip_merge_sets_dev")

    def _read_sets(self, paths):
        sets = [self.read_queries(p) for p in paths]
        set_off = np.zeros(len(sets) + 1, np.int64)
        set_off[1:] = np.cumsum([len(s[1]) for s in sets])
        cat = [np.concatenate([s[i] for s in sets]) if sets else np.zeros(0, np.int32) for i in range(3)]
        return cat[0], cat[1], cat[2], set_off

    def merge_files(self, paths, gap=0):
        """One region set per BED file (read as `igd search -q` reads it): merge_sets() of them."""
        return self.merge_sets(*self._read_sets(paths), gap=gap)

    def dataset_bp(self, v=0, rule=None, value_filter=None):
        """The merged base pairs of every dataset (igd_hip_dataset_bp): int64[nfiles + 1], entry f the bp of the union of the
        records of file f that a search under (v, rule, value_filter) counts, the last entry the union over all files.  Computed
        once per (value filter, rule) and kept in the handle: dataset_bp_computed() counts the computations."""
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        bp = np.empty(self.nfiles + 1, np.int64)
        _chk(self._H.igd_hip_dataset_bp(self.dev, vf, rule, _ptr(bp)), "igd_hip_dataset_bp")
        return bp

    def dataset_bp_computed(self):
        """How many times this handle has computed (not found in its cache) a dataset_bp()."""
        return int(self._H.igd_hip_dataset_bp_computed(self.dev))

    def jaccard_sets(self, ichr, qs, qe, set_off, v=0, rule=None, value_filter=None):
        """The base-pair intersection of every region set with every dataset, `bedtools jaccard` (igd_hip_jaccard_sets; sets as
        search_sets()): JaccardSets(inter int64[nsets, nfiles + 1], set_bp int64[nsets], file_bp int64[nfiles + 1], n_merged,
        n_dropped int64[nsets]).  The sets are merged at gap 0 first, so inter[k, f] is |A_k n B_f| exactly; the last column is
        "any dataset".  igd_amd.jaccard_summary() gives the Jaccard and the containment fractions."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "jaccard_sets")
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        js = JaccardSets(np.empty((nsets, self.nfiles + 1), np.int64), np.empty(nsets, np.int64), np.empty(self.nfiles + 1, np.int64),
                         np.empty(nsets, np.int64), np.empty(nsets, np.int64))
        _chk(self._H.igd_hip_jaccard_sets(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, vf, rule, _ptr(js.inter),
                                          _ptr(js.set_bp), _ptr(js.file_bp), _ptr(js.n_merged), _ptr(js.n_dropped)), "igd_hip_jaccard_sets")
        return js

    def permutation_bp(self, ichr, qs, qe, ctg_len, nperm, seed=0, mode="circular", v=0, rule=None, value_filter=None, workspace=None,
                       universe=None):
        """Permutation null of the base-pair overlap of one region set (igd_hip_permute_bp): "does my set share more base pairs
        with dataset f than chance".  The set is moved nperm times as permutation_support() moves it (same generator, mode,
        seed and ctg_len), and the set as given and every permuted set are treated as jaccard_sets() treats a set: merged at gap
        0, then covered.  Returns PermutationBp(inter int64[nperm + 1, nfiles + 1], set_bp, n_merged int64[nperm + 1], n_dropped,
        file_bp int64[nfiles + 1], nperm): row 0 the set as given, row p + 1 permutation p, the last column "any dataset";
        file_bp is dataset_bp().  Neither the permuted regions nor the merged runs leave the device.  perm_bp_summary() places
        the observed row in the null distribution.  mode "resample" with universe= and ctg_len None as permutation_support()
        takes them (igd_hip_permute_bp_rs); n_dropped is then that of the set as given, a draw drops what its own regions make
        it drop."""
        P = _placement(ichr, qs, qe, ctg_len, mode, workspace, universe, "permutation_bp")
        _placement_fits(P, self.nctg, "permutation_bp")
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        rows = max(int(nperm), 0) + 1
        inter, set_bp, n_merged = np.empty((rows, self.nfiles + 1), np.int64), np.empty(rows, np.int64), np.empty(rows, np.int64)
        dropped, file_bp = np.zeros(1, np.int64), np.empty(self.nfiles + 1, np.int64)
        _chk(getattr(self._H, "igd_hip_permute_bp" + P.sfx)(self.dev, _ptr(P.ichr), _ptr(P.qs), _ptr(P.qe), len(P.qs), *P.mid, _seed(seed), int(nperm),
                                                            vf, rule, _ptr(inter), _ptr(set_bp), _ptr(n_merged), _ptr(dropped), *P.tail),
             "igd_hip_permute_bp" + P.sfx.replace("_ws", ""))
        _chk(self._H.igd_hip_dataset_bp(self.dev, vf, rule, _ptr(file_bp)), "igd_hip_dataset_bp")
        return PermutationBp(inter, set_bp, n_merged, int(dropped[0]), file_bp, int(nperm))

    def permutation_bp_files(self, path, genome_path, nperm, seed=0, mode="circular", v=0, workspace=None, universe_path=None):
        """The null of one BED file (read as `igd search -q` reads it) with the lengths of a genome file: the integers behind
        what `igd search -q path -P nperm -g genome_path -G` prints (mode="resample": universe_path=, genome_path None)."""
        ctg_len, uni = self._genome_or_universe(genome_path, universe_path)
        return self.permutation_bp(*self.read_queries(path), ctg_len, nperm, seed, mode, v, workspace=workspace, universe=uni)

    def jaccard_files(self, paths, v=0):
        """One region set per BED file (read as `igd search -q` reads it): the JaccardSets of jaccard_sets()."""
        return self.jaccard_sets(*self._read_sets(paths), v=v)

    # ---- values of the overlapping records per region and dataset -------------------------
    def map_values(self, ichr, qs, qe, op="sum", value_filter=None, count=None, agg=None):
        """How many records of every dataset overlap each region and what they are worth (igd_hip_map; the definitions are in
        include/igd_hip.h): (count int32[nq, nfiles], agg int64[nq, nfiles]).  op is "count", "sum", "min" or "max" of the
        records' value column; agg is 0 where count is 0 and, under "count", holds the counts.  value_filter: only records with
        value >= it are counted.  There is no tile rule.  count and agg (C order), when given, are overwritten: every word is
        defined by the call.  "sum", "min" and "max" on a database without values raise."""
        ichr, qs, qe = _regions(ichr, qs, qe, "map_values")
        nq, o = len(qs), _map_op(op, "map_values")
        count = _out(count, (nq, self.nfiles), np.int32, "count", "map_values")
        agg = _out(agg, (nq, self.nfiles), np.int64, "agg", "map_values")
        _chk(self._H.igd_hip_map(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), nq, o, _value_filter(value_filter), _ptr(count), _ptr(agg)),
             "igd_hip_map")
        return count, agg

    def map_sets(self, ichr, qs, qe, set_off, op="sum", value_filter=None, out=None):
        """map_values() summed up per region set (igd_hip_map_sets; sets as search_sets()): MapSets(n_hit, pairs, agg_sum, op),
        three int64[nsets, nfiles] -- the regions of the set with a counted record of the file, the counted (region, record)
        pairs, and the sum of the regions' agg (under "count": the pairs).  The rows never leave the device.  out, when given,
        is a list of three C-ordered int64[nsets, nfiles] that are overwritten."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "map_sets")
        o = _map_op(op, "map_sets")
        out = _outs(out, 3, (nsets, self.nfiles), "map_sets")
        _chk(self._H.igd_hip_map_sets(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, o, _value_filter(value_filter),
                                      *[_ptr(a) for a in out]), "igd_hip_map_sets")
        return MapSets(*out, op)

    def map_files(self, paths, op, value_filter=None):
        """One region set per BED file (read as `igd search -q` reads it): the MapSets of map_sets()."""
        return self.map_sets(*self._read_sets(paths), op, value_filter)

    def _map_sets_fused(self, ichr, qs, qe, set_off, op="sum", value_filter=None, out=None):
        """map_sets_fused(ichr, qs, qe, set_off, op="sum", value_filter=None, out=None).  map_sets() through the fused kernel
        (igd_hip_map_sets_fused, kernel igd_map_slices): the same MapSets, every integer, without count and agg rows in device
        memory.  Databases with more files than igd_hip_map_fused_max_files(op) take map_sets()' route."""
        ichr, qs, qe, set_off, nsets = _sets(ichr, qs, qe, set_off, "map_sets_fused")
        o = _map_op(op, "map_sets_fused")
        out = _outs(out, 3, (nsets, self.nfiles), "map_sets_fused")
        _chk(self._H.igd_hip_map_sets_fused(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), _ptr(set_off), nsets, o, _value_filter(value_filter),
                                            *[_ptr(a) for a in out]), "igd_hip_map_sets_fused")
        return MapSets(*out, op)

    map_sets_fused = _forward(_map_sets_fused)

    def map_fused_files(self, paths, op, value_filter=None):
        """One region set per BED file (read as `igd search -q` reads it): the MapSets of map_sets_fused()."""
        return self.map_sets_fused(*self._read_sets(paths), op, value_filter)

    def _permutation_map(self, ichr, qs, qe, ctg_len, nperm, op, seed=0, mode="circular", value_filter=None, out=None, workspace=None,
                         universe=None):
        """permutation_map(ichr, qs, qe, ctg_len, nperm, op, seed=0, mode="circular", value_filter=None, out=None, workspace=None,
        universe=None).  Permutation null of the values of the records under one region set (igd_hip_permute_map): "are the scores
        of dataset f's records under my regions higher or lower than chance" (regioneR's permTest with meanInRegions).  The set is
        permuted nperm times by the generator of permutation_support() (same mode, seed and ctg_len) and every permuted set is
        measured as map_sets() measures a set.  Returns PermutationMap(n_hit, pairs, agg_sum, op, nperm), each int64[nperm + 1,
        nfiles]: row 0 is the set as given, row p + 1 permutation p.  op is "count", "sum", "min", "max" or "mean", which runs the
        rows of "sum"; perm_map_summary() places the observed statistic -- agg_sum / n_hit, for "mean" agg_sum / pairs -- in its
        null.  out, when given, is a list of three C-ordered int64[nperm + 1, nfiles] that are overwritten.  workspace= with
        mode="workspace", and universe= with mode="resample" and ctg_len None, as permutation_support() takes them
        (igd_hip_permute_map_ws, _rs)."""
        P = _placement(ichr, qs, qe, ctg_len, mode, workspace, universe, "permutation_map")
        _placement_fits(P, self.nctg, "permutation_map")
        o = _perm_map_op(op, "permutation_map")
        out = _outs(out, 3, (max(int(nperm), 0) + 1, self.nfiles), "permutation_map")
        _chk(getattr(self._H, "igd_hip_permute_map" + P.sfx)(self.dev, _ptr(P.ichr), _ptr(P.qs), _ptr(P.qe), len(P.qs), *P.mid, _seed(seed),
                                                             int(nperm), o, _value_filter(value_filter), *[_ptr(a) for a in out], *P.tail),
             "igd_hip_permute_map" + P.sfx.replace("_ws", ""))
        return PermutationMap(*out, op, int(nperm))

    permutation_map = _forward(_permutation_map)

    def permutation_map_files(self, path, genome_path, nperm, op, seed=0, mode="circular", value_filter=None, workspace=None,
                              universe_path=None):
        """The null of one BED file (read as `igd search -q` reads it) with the lengths of a genome file: the integers behind
        what `igd search -q path -P nperm -g genome_path -I op` prints (with -W: mode="workspace" and workspace=; with -M resample
        -U universe_path: mode="resample", universe_path= and genome_path None)."""
        ctg_len, uni = self._genome_or_universe(genome_path, universe_path)
        return self.permutation_map(*self.read_queries(path), ctg_len, nperm, op, seed, mode, value_filter, workspace=workspace,
                                    universe=uni)

    def map_dev(self, d_ichr, d_qs, d_qe, nq, d_count, d_agg=None, op="sum", value_filter=None, stream=None):
        """Resident batch: arguments are device pointers (ints).  Asynchronous.  d_count (int32[nq * nfiles]) and d_agg
        (int64[nq * nfiles]; may be None under op "count") are overwritten.  nq above igd_hip_max_batch() is refused: split the
        batch."""
        _chk(self._H.igd_hip_map_dev(self.dev, d_ichr, d_qs, d_qe, int(nq), _map_op(op, "map_dev"), _value_filter(value_filter), d_count, d_agg,
                                     stream), "igd_hip_map_dev")

    def membership_dev(self, d_ichr, d_qs, d_qe, nq, d_bits, d_nfiles_hit=None, d_nhit=None, v=0, rule=None,
                       value_filter=None, stream=None):
        """Resident batch: arguments are device pointers (ints).  Asynchronous.  d_bits (uint32[nq * member_words]) and
        d_nfiles_hit (int32[nq], may be None) are overwritten, d_nhit (int64[1], may be None) is added to.  nq above
        igd_hip_max_batch() is refused: split the batch, rows are per query."""
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        _chk(self._H.igd_hip_membership_dev(self.dev, d_ichr, d_qs, d_qe, int(nq), vf, rule, d_bits, d_nfiles_hit, d_nhit,
                                            stream), "igd_hip_membership_dev")

    @staticmethod
    def unpack_membership(bits, nfiles):
        """bool[nq, nfiles] from the rows of membership()"""
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        nq = bits.shape[0]
        if nfiles == 0 or nq == 0:
            return np.zeros((nq, nfiles), bool)
        b = np.unpackbits(bits.astype("<u4").view(np.uint8).reshape(nq, -1), axis=1, bitorder="little")
        return b[:, :nfiles].astype(bool)

    def search_dev(self, d_ichr, d_qs, d_qe, nq, d_hits, d_total=None, v=0, rule=None,
                   value_filter=None, stream=None, flags=0):
        """Resident batch: arguments are device pointers (ints).  Asynchronous.
        flags: 0, IGD_HIP_FLAG_SORTED (verified promise; sync() raises if broken) [| IGD_HIP_FLAG_SHORT: no query as long as a tile,
        verified too -- a dense batch then takes the DIRECT step] or IGD_HIP_FLAG_BUCKET (known to be unordered: no order check)."""
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        _chk(self._H.igd_hip_search_dev(self.dev, d_ichr, d_qs, d_qe, int(nq), vf, rule, int(flags), d_hits,
                                        d_total, stream), "igd_hip_search_dev")

    def search_runs_dev(self, d_run_start, d_qs, d_qe, nq, d_hits, d_total=None, v=0, rule=None,
                        value_filter=None, stream=None, flags=0):
        """Resident position-sorted batch given as contig runs (device int32[nctg + 1]: queries [run[c], run[c + 1]) lie on
        contig c) instead of one contig number per query.  Asynchronous; implies the order promise."""
        rule, vf = _dispatch(self.gtype, v, rule, value_filter)
        _chk(self._H.igd_hip_search_runs_dev(self.dev, d_run_start, d_qs, d_qe, int(nq), vf, rule, int(flags), d_hits,
                                             d_total, stream), "igd_hip_search_runs_dev")

    @staticmethod
    def contig_runs(ichr, nctg):
        """run_start[nctg + 1] of a batch whose contig numbers are non-decreasing (host, numpy)."""
        ichr = np.ascontiguousarray(ichr, dtype=np.int32)
        if len(ichr) and (np.any(np.diff(ichr) < 0) or ichr[0] < 0 or ichr[-1] >= nctg):
            raise IgdError("contig_runs: the batch is not grouped by ascending contig number")
        return np.searchsorted(ichr, np.arange(nctg + 1, dtype=np.int32), side="left").astype(np.int32)

    def sync(self, stream=None, spin=False):
        """Wait for the stream (spin: polling instead of sleeping on the completion signal) and surface asynchronous errors."""
        _chk((self._H.igd_hip_sync_spin if spin else self._H.igd_hip_sync)(self.dev, stream), "igd_hip_sync")

    def enumerate(self, ichr, qs, qe):
        """`-f`: returns (qoff int64[nq+1], records int32[n,4] = q,idx,start,end) in reference order."""
        ichr, qs, qe = _regions(ichr, qs, qe)
        nq = len(qs)
        qoff = np.zeros(nq + 1, np.int64)
        out = C.POINTER(N.HipHit)()
        total = C.c_int64(0)
        _chk(self._H.igd_hip_enumerate(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), nq,
                                       _ptr(qoff), C.byref(out), C.byref(total)), "igd_hip_enumerate")
        n = total.value
        if n:
            rec = np.ctypeslib.as_array(C.cast(out, N.i32p), shape=(n * 4,)).reshape(n, 4).copy()
            self._H.igd_hip_free(out)
        else:
            rec = np.zeros((0, 4), np.int32)
        return qoff, rec

    def enumerate_stream(self, ichr, qs, qe, on_chunk=None):
        """`-f`, streamed (igd_hip_enumerate_stream): on_chunk(q0, q1, qoff, rec) is called per chunk with
        rec = int32[n,4] VIEW of the pinned chunk buffer (valid during the call only).  Returns (qoff, total)."""
        ichr, qs, qe = _regions(ichr, qs, qe)
        nq = len(qs)
        qoff = np.zeros(nq + 1, np.int64)
        total = C.c_int64(0)

        def sink(ctx, q0, q1, qoff_p, hits_p):
            if on_chunk is not None:
                n = int(qoff[q1] - qoff[q0])
                rec = (np.ctypeslib.as_array(C.cast(hits_p, N.i32p), shape=(n * 4,)).reshape(n, 4)
                       if n else np.zeros((0, 4), np.int32))
                on_chunk(int(q0), int(q1), qoff, rec)
            return 0

        cb = N.ENUM_SINK(sink)
        _chk(self._H.igd_hip_enumerate_stream(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), nq,
                                              _ptr(qoff), cb, None, C.byref(total)), "igd_hip_enumerate_stream")
        return qoff, total.value

    def hit8_idx_bits(self):
        """How the packed `-f` record (igd_hip_hit8: 8 bytes per overlap) splits its second word for this database -- the low
        `bits` hold idx, the rest end - start -- or -1 when a record does not fit (igd_hip_hit8_idx_bits)."""
        return int(self._H.igd_hip_hit8_idx_bits(self.dev))

    def enumerate_stream8(self, ichr, qs, qe, on_chunk=None):
        """`-f`, streamed in 8 bytes per overlap (igd_hip_enumerate_stream8): on_chunk(q0, q1, qoff, rec, bits) is called per chunk
        with rec = uint32[n,2] VIEW of the pinned chunk buffer: rec[:,0] = start, rec[:,1] = (end - start) << bits | idx.
        Returns (qoff, total)."""
        ichr, qs, qe = _regions(ichr, qs, qe)
        nq = len(qs)
        qoff = np.zeros(nq + 1, np.int64)
        total = C.c_int64(0)

        def sink(ctx, q0, q1, qoff_p, hits_p, bits):
            if on_chunk is not None:
                n = int(qoff[q1] - qoff[q0])
                rec = (np.ctypeslib.as_array(C.cast(hits_p, C.POINTER(C.c_uint32)), shape=(n * 2,)).reshape(n, 2)
                       if n else np.zeros((0, 2), np.uint32))
                on_chunk(int(q0), int(q1), qoff, rec, int(bits))
            return 0

        cb = N.ENUM_SINK8(sink)
        _chk(self._H.igd_hip_enumerate_stream8(self.dev, _ptr(ichr), _ptr(qs), _ptr(qe), nq,
                                               _ptr(qoff), cb, None, C.byref(total)), "igd_hip_enumerate_stream8")
        return qoff, total.value

    @staticmethod
    def expand_hit8(rec, bits):
        """(start, end, idx) int32 arrays of packed records (igd_hip_hit8_expand)."""
        start = rec[:, 0].astype(np.uint32)
        hi = rec[:, 1].astype(np.uint32)
        idx = (hi & np.uint32((1 << bits) - 1)) if bits else np.zeros(len(hi), np.uint32)
        end = (start + (hi >> np.uint32(bits))).astype(np.uint32)
        return start.view(np.int32), end.view(np.int32), idx.astype(np.int32)

    def hitmap(self, v=0):
        """`-m`: (uint32[nfiles,nfiles], pairs); v>0 keeps records with value > v (getMap_v)."""
        m = np.zeros((self.nfiles, self.nfiles), np.uint32)
        total = C.c_int64(0)
        _chk(self._H.igd_hip_hitmap(self.dev, 1 if v > 0 else 0, int(v), m.ctypes.data, C.byref(total)), "igd_hip_hitmap")
        return m, total.value

    def seqpare(self, ichr, qs, qe, qgroup, ngroups, n_queries_total=None, nr=None):
        """`-s` (Seqpare, seqOverlaps src/igd_search.c:354-451).  Queries in the reference's order: contigs
        of the query file in first-seen order (qgroup = 0,1,.. non-decreasing), inside a contig by start
        (stable).  Returns the per-dataset sums of matched similarities; with n_queries_total (all accepted
        query lines, known contig or not) and nr (regions per dataset) the similarity S = sum/(Nq+nr-sum)."""
        a = [np.ascontiguousarray(x, dtype=np.int32) for x in (ichr, qs, qe, qgroup)]
        sums = np.zeros(max(self.nfiles, 1), np.float64)
        _chk(self._H.igd_hip_seqpare(self.dev, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), len(a[0]),
                                     _ptr(a[3]), int(ngroups), _ptr(sums)), "igd_hip_seqpare")
        sums = sums[:self.nfiles]
        if n_queries_total is None or nr is None:
            return sums
        return sums / (float(n_queries_total) + np.asarray(nr, np.float64) - sums)

    def batch_stats(self, d_ichr, d_qs, d_qe, nq, v=0):
        rule, vf = self.cli_dispatch(self.gtype, v)
        st = N.HipStats()
        _chk(self._H.igd_hip_batch_stats(self.dev, d_ichr, d_qs, d_qe, int(nq), vf, rule, C.byref(st)),
             "igd_hip_batch_stats")
        return dict(queries=st.queries, pairs=st.pairs, S=st.S, B=st.B, H=st.H)

    def batch_traffic(self, d_ichr, d_qs, d_qe, nq, v=0, flags=0):
        """Compulsory HBM bytes of the scan kernel for this batch (igd_hip_batch_traffic)."""
        rule, vf = self.cli_dispatch(self.gtype, v)
        t = N.HipTraffic()
        _chk(self._H.igd_hip_batch_traffic(self.dev, d_ichr, d_qs, d_qe, int(nq), vf, rule, int(flags), C.byref(t)),
             "igd_hip_batch_traffic")
        return {k: getattr(t, k) for k, _ in N.HipTraffic._fields_}

    def algorithmic_bytes(self, stats, nq, mode="hits"):
        """bytes one launch has to touch, by the reference's own work terms."""
        b = 4 * stats["S"] + 4 * stats["H"] + 4 * stats["B"] + 16 * stats["pairs"] + 12 * nq + 8 * self.nfiles
        if mode == "v":
            b += 4 * stats["S"]
        elif mode == "f":
            b += 4 * stats["H"] + 16 * stats["H"] + 8 * nq
        return b

    def profile_begin(self, max_launches, every=1):
        """Arm HIP-event timing of the scan kernel for up to max_launches launches, every `every`-th one."""
        _chk(self._H.igd_hip_profile_sampling(self.dev, int(every)), "igd_hip_profile_sampling")
        _chk(self._H.igd_hip_profile_begin(self.dev, int(max_launches)), "igd_hip_profile_begin")

    def profile_end(self):
        n, a, b = C.c_int(0), C.c_double(0), C.c_double(0)
        _chk(self._H.igd_hip_profile_end(self.dev, C.byref(n), C.byref(a), C.byref(b)), "igd_hip_profile_end")
        return dict(launches=n.value, scan_ms=a.value, pipeline_ms=b.value)

    def last_scan_kernel(self):
        """Name of the scan kernel the last batch ran on ("igd_scan_sorted" / "igd_scan_tiles"); waits for it."""
        return (self._H.igd_hip_last_scan_kernel(self.dev) or b"").decode()

    ROUTE_WORDS = ("kernel", "full", "packed", "lb_shift", "nfix", "nlong", "nheavys", "nheavy", "nfar", "cov_sorted",
                   "cov_bucket", "unsorted", "notstart")
    ROUTE_CONSTANTS = ("unit", "round", "short_tiles", "dense_min", "lean_first", "heavy_first", "heavy_slice", "far_wide",
                       "later_max", "sbcap", "lean_waves")

    def last_batch_routes(self):
        """TEST-ONLY (igd_hip_last_batch_routes): dict of the route words of the last batch, {} before the first; waits for it.
        kernel is the name last_scan_kernel() gives."""
        w = (C.c_int64 * len(self.ROUTE_WORDS))()
        n = self._H.igd_hip_last_batch_routes(self.dev, w, len(w))
        if n == 0:
            return {}
        if n != len(w):
            raise IgdError("igd_hip_last_batch_routes: %d words, not %d" % (n, len(w)))
        out = dict(zip(self.ROUTE_WORDS, (int(x) for x in w)))
        out["kernel"] = {1: "igd_scan_sorted", 2: "igd_scan_tiles", 3: "igd_scan_direct"}[out["kernel"]]
        return out

    def route_constants(self):
        """TEST-ONLY (igd_hip_route_constants): dict of the constants the merge join's routes are decided by."""
        w = (C.c_int64 * len(self.ROUTE_CONSTANTS))()
        n = self._H.igd_hip_route_constants(self.dev, w, len(w))
        if n != len(w):
            raise IgdError("igd_hip_route_constants: %d words, not %d" % (n, len(w)))
        return dict(zip(self.ROUTE_CONSTANTS, (int(x) for x in w)))


def measure_rates(device=0):
    """GB/s of this box, measured now: HBM float4 copy (read+write), HBM float4 read, pinned D2H, pinned H2D."""
    r = (C.c_double * 4)()
    _chk(N.hip().igd_hip_measure_rates(int(device), r), "igd_hip_measure_rates")
    return {"hbm_copy_GBps": r[0], "hbm_read_GBps": r[1], "d2h_GBps": r[2], "h2d_GBps": r[3]}
