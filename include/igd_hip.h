/* igd_hip.h -- C ABI of the MI355X (gfx950) overlap-search engine.
 *
 * This is the device-side boundary that the three host flavours of the reference's
 * igd_search.h (include/igd_search.h, include/igd_py_abi.h, include/igdr_abi.h) are built
 * on.  Plain C: opaque handle, pointers and sizes only, no C++/torch types.
 *
 * What it replaces in the reference (databio/IGD, /root/reference):
 *   igd_hip_search / _dev    the per-query loops  getOverlaps   src/igd_search.c:696-719
 *                                                 getOverlaps_v src/igd_search.c:746-769
 *                                                 getOverlaps0  src/igd_search.c:202-225
 *                            over the kernels     get_overlaps   src/igd_search.c:454-534
 *                                                 get_overlaps_v src/igd_search.c:623-694
 *                                                 get_overlaps0  src/igd_search.c:30-112
 *                            and the hits[] accumulator          src/igd_search.c:925,491,524,654,684
 *   igd_hip_enumerate        getOverlaps_f1/_f0 src/igd_search.c:721-744,227-250 over
 *                            get_overlaps_f1/_f0 src/igd_search.c:537-620,114-200
 *   igd_hip_open             the per-tile fseek/fread of src/igd_search.c:469-476 (the whole
 *                            tile region is uploaded once, transposed AoS->SoA on the GPU)
 *
 * There is NO CPU fallback behind any of these entry points: without a usable HIP device
 * they return an error code and igd_hip_last_error() says why.
 */
#ifndef IGD_HIP_H
#define IGD_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IGD_HIP_OK          0
#define IGD_HIP_ERR_DEVICE  (-1)   /* no device / HIP runtime error          */
#define IGD_HIP_ERR_ARG     (-2)   /* bad argument                            */
#define IGD_HIP_ERR_NOMEM   (-3)   /* host or device allocation failed        */
#define IGD_HIP_ERR_UNSORTED (-4)  /* IGD_HIP_FLAG_SORTED promised, order violated */

/* Tile-visiting rules. */
#define IGD_HIP_RULE_NEST 0  /* get_overlaps / get_overlaps0 / _f0 / _f1: an EMPTY first tile
                                ends the query (loop nested in `if(nCnt[n1]>0)`, :468-532)   */
#define IGD_HIP_RULE_FLAT 1  /* get_overlaps_v: every tile n1..n2 visited (:635-691)          */

typedef struct igd_hip_db igd_hip_db;          /* opaque: one .igd resident on one GPU      */

/* Host description of an .igd (the header tables of iGD_t, src/igd_base.h:96-105, plus the
 * raw tile region of the file).  Nothing is retained after igd_hip_open returns. */
typedef struct {
    int32_t nbp;              /* tile width in bp                                           */
    int32_t gType;            /* 1: 16-byte {idx,start,end,value}; 0: 12-byte {idx,start,end}*/
    int32_t nCtg;
    int32_t nFiles;           /* length of hits[] (from _index.tsv)                          */
    const int32_t *nTile;     /* [nCtg]                                                     */
    const int32_t *nCnt;      /* contig-major, sum(nTile) entries (file order)               */
    const void *records;      /* host pointer: all tile records in file order (AoS), or NULL: */
    int64_t nRecords;         /* = sum(nCnt)                                                */
    int     fd;               /* records == NULL: read them from this descriptor ...         */
    int64_t fd_offset;        /* ... starting at this byte offset (header size of the .igd)  */
} igd_hip_desc;

/* One emitted overlap of the `-f` path: query number (position in the batch), then the
 * record as the reference prints it (src/igd_search.c:577,610). */
typedef struct { int32_t q, idx, start, end; } igd_hip_hit;

/* Exact work statistics of one batch under one rule -- the terms of the algorithmic byte
 * model.  Instrumentation; not part of a search. */
typedef struct {
    int64_t queries;  /* queries with a valid contig and n1 in range                         */
    int64_t pairs;    /* (query,tile) pairs with cnt>0 && qe > first start                   */
    int64_t S;        /* sum of scan lengths                                                */
    int64_t B;        /* sum of ceil(log2(cnt+1))                                           */
    int64_t H;        /* hits                                                               */
} igd_hip_stats;

int         igd_hip_device_count(void);               /* <=0: none usable                    */
const char *igd_hip_last_error(void);                 /* thread-local, never NULL            */

int  igd_hip_open(const igd_hip_desc *desc, int device, igd_hip_db **out);
void igd_hip_close(igd_hip_db *db);
int  igd_hip_device(const igd_hip_db *db);
int32_t igd_hip_nfiles(const igd_hip_db *db);
int64_t igd_hip_resident_bytes(const igd_hip_db *db); /* HBM held by the SoA image + tables  */

/* `v` of the search calls: records with value < v are not counted (get_overlaps_v's
 * `value>=v`, src/igd_search.c:652,682).  IGD_HIP_NO_VALUE_FILTER switches the predicate
 * off (get_overlaps).  Ignored for gType 0, which stores no value (:1024-1025).  Whether a
 * CLI `-v N` selects the filtered kernel (only N>0, :1027) is the HOST's decision. */
#define IGD_HIP_NO_VALUE_FILTER INT32_MIN

/* How the engine groups a batch's queries by tile (flags of the search calls):
 *   0                     the device decides: one pass checks whether the batch is ordered by
 *                         (contig index, start) -- a position-sorted BED -- and, if so, reads
 *                         the queries in place (merge join); otherwise it counting-sorts the
 *                         (query,tile) pairs.  Same result either way.
 *   IGD_HIP_FLAG_SORTED   the caller PROMISES that order, which skips enqueueing the bucket
 *                         kernels.  The promise is verified on the device: if it does not hold,
 *                         that batch adds nothing and igd_hip_sync returns IGD_HIP_ERR_UNSORTED.
 *                         The promise is (contig index, START) -- starts that decrease inside one
 *                         tile break it too, whichever step the batch takes (without the promise
 *                         such a batch is counted by the merge join's pairwise compares).
 *   IGD_HIP_FLAG_BUCKET   the caller KNOWS the batch is not in that order (the command line tool's
 *                         parser saw a line out of order): no order check, no merge-join launch,
 *                         always the counting sort.  Never wrong -- the counting sort takes any
 *                         order -- only slower than the merge join on a batch that is sorted after all. */
#define IGD_HIP_FLAG_SORTED 1
#define IGD_HIP_FLAG_BUCKET 2
/* Besides the exact start/end/idx/value arrays the engine keeps a compact tile-relative image
 * (6 bytes per record) that the counting kernels read when the tile width is <= 32768 and
 * nFiles <= 65536.  IGD_HIP_FLAG_EXACT makes a call read the exact arrays instead (tests). */
#define IGD_HIP_FLAG_EXACT 4
/* igd_hip_search_dev only: d_hits[] (and d_total) are cleared by the batch's first kernel before the
 * counts are added -- saves the caller a separate memset when it does not accumulate. */
#define IGD_HIP_FLAG_ZERO_FIRST 8
/* With IGD_HIP_FLAG_SORTED: the caller also states that no query is longer than one tile (qe - qs < nbp) -- what a
 * query file of peaks / regions is, and what the command line tool finds out while it parses.  A dense batch (>= 28 queries
 * per tile on average) then takes the DIRECT step: no per-query pre-pass, the scan kernel reads q_qs / q_qe itself
 * (engine/scan_direct.hpp).  VERIFIED like the order: a longer query is found where it is read and its later tiles are
 * walked exactly -- it costs time, never a count. */
#define IGD_HIP_FLAG_SHORT 16

/* Host-buffer search.  ichr[i] = contig index (as get_id returns; <0 or >=nCtg: skipped).
 * hits[0..nFiles) is caller-allocated and is ADDED to (reference semantics :491).
 * *total (may be NULL) receives the number of overlaps of this batch.  Blocking. */
int igd_hip_search(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                   int64_t nq, int32_t v, int rule, int64_t *hits, int64_t *total);
/* same with `flags`.  An IGD_HIP_FLAG_SORTED promise that the device finds broken is not an
 * error here: the call repeats that slice with the device choosing the grouping. */
int igd_hip_search_ex(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                      int64_t nq, int32_t v, int rule, int flags, int64_t *hits, int64_t *total);

/* Many query sets in one call.  Set k = queries [set_off[k], set_off[k+1]) (host int64[nsets+1], monotone, set_off[0]=0);
 * hits (host int64[nsets * nFiles], row-major) and totals (host int64[nsets], may be NULL) are ADDED to.  Row k equals
 * igd_hip_search_ex on set k alone.  flags as igd_hip_search_ex (they steer the large-set route only).  Blocking.
 * Sets of fewer than 2^17 queries are counted together by one kernel (a row of LDS counters per workgroup); larger ones go
 * through the batch pipeline of igd_hip_search_dev, one row each.  A bad set_off is IGD_HIP_ERR_ARG before any launch. */
int igd_hip_search_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                        const int64_t *set_off, int32_t nsets, int32_t v, int rule, int flags,
                        int64_t *hits, int64_t *totals);

/* Support counts of many query sets in one call.  Sets as igd_hip_search_sets.  With hits_q[] = what igd_hip_search_ex
 * adds for the batch that holds query q alone (same rule and v):
 *     support[k * nFiles + f] += the queries q of set k with hits_q[f] > 0
 *     nhit[k]                 += the queries q of set k with hits_q[f] > 0 for some f      (nhit may be NULL)
 * -- the "regions of the set that overlap at least one region of file f" of a region-set enrichment table, where
 * igd_hip_search_sets counts (query, record) pairs.  Two identical queries are two queries; support <= min(|set|, hits).
 * One kernel counts all sets, whatever their sizes (igd_sets_support: a wave owns a whole query and keeps one bit per
 * file); there is no batch-pipeline route.  Blocking.  A bad set_off is IGD_HIP_ERR_ARG before any launch. */
int igd_hip_support_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                         const int64_t *set_off, int32_t nsets, int32_t v, int rule, int64_t *support, int64_t *nhit);

/* MINIMUM OVERLAP PER PAIR (LOLA's minOverlap, GenomicRanges' minoverlap, bedtools' -f / -F): a threshold on every (query,
 * record) pair, taken by the `_ov` forms of the set counts, the support counts, the enrichment and the permutation null.
 *     min_bp       base pairs, >= 0
 *     ppm_query    fraction of the QUERY's length, in parts per million, 0 .. 1 000 000
 *     ppm_record   fraction of the RECORD's length, in parts per million, 0 .. 1 000 000
 * Anything outside these ranges is IGD_HIP_ERR_ARG.  A NULL pointer or {0, 0, 0} is INACTIVE: the `_ov` form then IS the
 * plain entry point -- the same kernels, the same results.  With any field non-zero the threshold is ACTIVE and narrows the
 * pairs the search counts (rule word, the skip of a record met in an earlier tile, value filter and idx < nFiles unchanged)
 * to those with
 *     ov = min(qe, end) - max(qs, start)                      (the record's own coordinates, in whichever tile it is met)
 *     ov >= max(min_bp, 1)  &&  ov * 10^6 >= (qe - qs) * ppm_query  &&  ov * 10^6 >= (end - start) * ppm_record
 * in 64-bit integers; equality qualifies.  ppm_query = 10^6: the query lies inside the record; ppm_record = 10^6: the record
 * lies inside the query; both: equal intervals.  A ZERO-LENGTH OR INVERTED QUERY (qe <= qs) has ov <= 0 with every record
 * and is never counted under an active threshold, although the plain predicate  start < qe && end > qs  counts it under a
 * record that spans both its ends.  The test is per pair: support is "at least one qualifying pair in the file", not a sum
 * of covered base pairs over a file's records.
 * igd_hip_min_overlap_need_q is the part of the test that depends on the query alone, max(min_bp, 1, ceil(lenq * ppm_query /
 * 10^6)), or -1 when no record can qualify (qe <= qs; a bound above 2^31 - 1): the kernels evaluate it once per query.
 * Records are taken to satisfy 0 <= start < end (every writer of the format drops the others). */
typedef struct { int32_t min_bp, ppm_query, ppm_record; } igd_hip_min_overlap;
#define IGD_HIP_PPM 1000000
#if defined(__HIPCC__)
#define IGD_HIP_OV_HD_ __host__ __device__
#else
#define IGD_HIP_OV_HD_
#endif
static inline int igd_hip_min_overlap_valid(const igd_hip_min_overlap *t)
{
    return !t || (t->min_bp >= 0 && t->ppm_query >= 0 && t->ppm_query <= IGD_HIP_PPM && t->ppm_record >= 0 && t->ppm_record <= IGD_HIP_PPM);
}
static inline int igd_hip_min_overlap_active(const igd_hip_min_overlap *t)
{
    return t && (t->min_bp | t->ppm_query | t->ppm_record) != 0;
}
static inline IGD_HIP_OV_HD_ int32_t igd_hip_min_overlap_need_q(int32_t min_bp, int32_t ppm_query, int32_t qs, int32_t qe)
{
    const int64_t lenq = (int64_t)qe - (int64_t)qs;
    if (lenq <= 0) return -1;
    int64_t need = (lenq * (int64_t)ppm_query + (IGD_HIP_PPM - 1)) / IGD_HIP_PPM;
    if (need < min_bp) need = min_bp;
    if (need < 1) need = 1;
    return need > (int64_t)INT32_MAX ? -1 : (int32_t)need;
}
/* the pair (qs, qe) x (start, end), already counted by the plain predicate, under need_q >= 1 and ppm_record */
static inline IGD_HIP_OV_HD_ int igd_hip_min_overlap_pair(int32_t need_q, int32_t ppm_record, int32_t qs, int32_t qe, int32_t start, int32_t end)
{
    const int64_t ov = (int64_t)(qe < end ? qe : end) - (int64_t)(qs > start ? qs : start);
    return ov >= need_q && ov * IGD_HIP_PPM >= ((int64_t)end - (int64_t)start) * (int64_t)ppm_record;
}
int igd_hip_search_sets_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                           const int64_t *set_off, int32_t nsets, int32_t v, int rule, int flags,
                           int64_t *hits, int64_t *totals, const igd_hip_min_overlap *min_overlap);
int igd_hip_support_sets_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                            const int64_t *set_off, int32_t nsets, int32_t v, int rule, int64_t *support, int64_t *nhit,
                            const igd_hip_min_overlap *min_overlap);
/* igd_hip_search_sets_ov under an active threshold cuts EVERY set into slices for the kernel (as the support counts do):
 * the batch pipeline takes no threshold, so `flags` and the 2^17 boundary have no effect then. */

/* Covered base pairs of many query sets in one call.  Sets as igd_hip_search_sets.  With R_q(f) = the records of file f
 * that igd_hip_search_ex counts for the batch that holds query q = (contig, qs, qe) alone (same rule and v):
 *     coverage[k * nFiles + f] += sum over the queries q of set k of | [qs, qe) n union of [start, end) over R_q(f) |
 *     covered[k]               += the same with the union taken over the records of ALL files     (covered may be NULL)
 * in base pairs: an interval union per query, not a sum over records.  The sum runs over queries: two identical queries
 * count twice and overlapping queries of one set are not merged (merge the BED first for the set-level intersection).
 * coverage > 0 exactly where igd_hip_support_sets' support > 0.  One kernel counts all sets, whatever their sizes
 * (igd_sets_coverage: a wave owns a whole query and keeps one frontier per file); there is no batch-pipeline route.
 * Blocking.  A bad set_off is IGD_HIP_ERR_ARG before any launch. */
int igd_hip_coverage_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                          const int64_t *set_off, int32_t nsets, int32_t v, int rule, int64_t *coverage, int64_t *covered);

/* Per-query dataset membership: which files each query overlaps.  With hits_q[] as above (the batch that holds query q
 * alone, same rule and v), row q of `bits` is igd_hip_member_words(db) = ceil(nFiles / 32) uint32 words:
 *     bit (f & 31) of bits[q * nW + (f >> 5)] = hits_q[f] > 0;      bits at positions >= nFiles are 0
 *     nfiles_hit[q] = the files f with hits_q[f] > 0 (the popcount of row q)               (nfiles_hit may be NULL)
 *     nhit         += the queries with any bit set (what igd_hip_support_sets adds to nhit)  (nhit may be NULL)
 * -- the region x dataset matrix whose column sums are the support counts.  Every word of every row and every
 * nfiles_hit[q] is DEFINED by the call (overwritten, not OR-ed or added to): the caller need not clear them.  A query on an
 * unknown contig, out of range or ended by rule NEST's empty first tile has an all-zero row; two identical queries have two
 * identical rows.  Queries go through the engine in chunks of at most igd_hip_max_batch() queries and a budget of device
 * bytes for the rows.  Blocking.  A bad argument is IGD_HIP_ERR_ARG before any launch, the caller's arrays untouched. */
int64_t igd_hip_member_words(const igd_hip_db *db);
int igd_hip_membership(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                       int32_t v, int rule, uint32_t *bits, int32_t *nfiles_hit, int64_t *nhit);
/* The same with device pointers on db's GPU, for a caller that keeps the matrix resident: enqueues on `stream` (a
 * hipStream_t; NULL = the engine's own stream) and returns without waiting.  d_bits (uint32[nq * nW]) and d_nfiles_hit
 * (int32[nq], may be NULL) are overwritten; d_nhit (int64[1], may be NULL) is ADDED to.  nq above igd_hip_max_batch() is
 * IGD_HIP_ERR_ARG: the caller splits the batch (rows are per query). */
int igd_hip_membership_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq,
                           int32_t v, int rule, uint32_t *d_bits, int32_t *d_nfiles_hit, int64_t *d_nhit, void *stream);
/* Workgroups (of four waves) the membership kernel is launched with for nq queries: a wave takes a second query only when
 * nq exceeds four times this number (tests). */
int32_t igd_hip_member_grid(int64_t nq);

/* Nearest record per dataset within a window: how far each region lies from the nearest record of every file, as
 * `bedtools closest -d` / `window` and GenomicRanges' distanceToNearest measure it.  THE DEFINITIONS (the one place: kernel
 * igd_nearest_rows, igdc_nearest_host and the tests' numpy reference agree on every integer).  For a region (c, qs, qe) and a
 * record (c, s, e, value) on the same contig
 *     d = 0                          if s < qe && e > qs       (the plain predicate, on the raw int32 coordinates)
 *     d = max(s - qe, qs - e) + 1    otherwise                 (book-ended intervals are 1 bp apart: bedtools' convention)
 * in 64-bit integers; d >= 1 in the second case, whatever the region looks like.
 *     window       W, 0 <= W <= IGD_HIP_NEAREST_MAX_WINDOW = 2^30; anything else is IGD_HIP_ERR_ARG.  A record is WITHIN THE
 *                  WINDOW iff d <= W, which is  s < qe + W && e > qs - W  in 64-bit arithmetic.
 *     dist[q][f]   min d over the records of file f within the window -- with a value filter v on a database that has
 *                  values, over those with value >= v: the nearest PASSING record -- or -1 when there is none.  int32.
 *     dmin[q]      the minimum over f of the dist[q][f] that are not -1, else -1.
 *     no rule      A distance is a property of the intervals, not of the reference's loop: there is no `rule` argument.  The
 *                  widened interval [max(qs - W, 0), min(qe + W, 2^31 - 1)) is walked under rule FLAT on the image
 *                  igd_hip_support_sets walks (the re-tiled copy when there is one); neither clamp changes which records are
 *                  within the window, records having 0 <= start < end.
 *     degenerate   A region on an unknown contig (c < 0 or c >= nCtg) has a row of -1.  Zero-length and inverted regions are
 *                  not special-cased: the formula is applied literally.
 *     sets         For set k = regions [set_off[k], set_off[k + 1]) each statistic is int64[nsets][nFiles + 1]; column nFiles is
 *                  the any-dataset column, built from dmin (as index nFiles of igd_hip_permute_support's arrays):
 *                      n_within[k][f]  = #{q : dist[q][f] >= 0}        n_overlap[k][f] = #{q : dist[q][f] == 0}
 *                      sum_dist[k][f]  = the sum of the non-negative dist[q][f]
 *     identities   n_overlap is the support of igd_hip_support_sets(..., IGD_HIP_RULE_FLAT) for every W, its last column that
 *                  call's nhit; with W = 0, n_within == n_overlap.
 * Every output is DEFINED by the call, as igd_hip_membership defines its rows: every word is written, nothing is added to.
 * igd_hip_nearest: dist is int32[nq * nFiles], dmin int32[nq] (may be NULL).  The regions go through in chunks of at most
 * igd_hip_max_batch() regions and 256 MiB of device rows (TEST-ONLY: IGD_HIP_NEAREST_ROW_BYTES lowers it).
 * igd_hip_nearest_sets: whole sets are taken while their three result rows fit the row budget of igd_hip_support_sets, their
 * regions go through in the chunks above (a set may be cut by a chunk), kernel igd_nearest_reduce adds every chunk's rows
 * into the three resident matrices; the rows never leave the device and the matrices are copied out once.  Any of the three
 * may be NULL.
 * igd_hip_nearest_dev: device pointers, one engine batch (nq above igd_hip_max_batch() is IGD_HIP_ERR_ARG), enqueued on
 * `stream` (NULL: the engine's own) without waiting; d_dist and d_dmin (may be NULL) are overwritten.
 * Blocking (but for _dev), one device.  IGD_HIP_ERR_ARG -- a missing array, a bad set_off, W out of range -- comes before
 * anything of the caller's is written.
 * Not done: an unbounded nearest, a minimum overlap, several devices, the permutation null of a distance statistic. */
#define IGD_HIP_NEAREST_MAX_WINDOW ((int32_t)1 << 30)
static inline IGD_HIP_OV_HD_ int igd_hip_nearest_window_valid(int64_t window) { return window >= 0 && window <= IGD_HIP_NEAREST_MAX_WINDOW; }
/* d of one (region, record) pair */
static inline IGD_HIP_OV_HD_ int64_t igd_hip_nearest_dist(int32_t qs, int32_t qe, int32_t start, int32_t end)
{
    if (start < qe && end > qs) return 0;
    const int64_t a = (int64_t)start - (int64_t)qe, b = (int64_t)qs - (int64_t)end;
    return (a > b ? a : b) + 1;
}
/* the widened interval the tiles are visited for: [max(qs - W, 0), min(qe + W, 2^31 - 1)) */
static inline IGD_HIP_OV_HD_ void igd_hip_nearest_widen(int32_t qs, int32_t qe, int32_t window, int32_t *ws, int32_t *we)
{
    const int64_t a = (int64_t)qs - (int64_t)window, b = (int64_t)qe + (int64_t)window;
    *ws = (int32_t)(a < 0 ? 0 : a);
    *we = (int32_t)(b > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : b);
}
int igd_hip_nearest(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t window, int32_t v,
                    int32_t *dist, int32_t *dmin);
int igd_hip_nearest_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                         int32_t nsets, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist);
int igd_hip_nearest_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq, int32_t window,
                        int32_t v, int32_t *d_dist, int32_t *d_dmin, void *stream);
/* Workgroups (of four waves) igd_nearest_rows is launched with for nq regions: a wave meets a second region only when nq
 * exceeds four times this number (tests). */
int32_t igd_hip_nearest_grid(int64_t nq);

/* Signed nearest distances and their histogram per set and dataset: on which side the nearest record lies
 * (`bedtools closest -D ref`) and how the distances are distributed (GenomicDistributions' calcFeatureDist).  THE DEFINITIONS
 * (the one place: kernels igd_nearest_rows<., ., true> and igd_nearest_hist, igdc_nearest_signed_host / igdc_nearest_hist_host
 * and the tests' numpy reference agree on every integer).  With d = igd_hip_nearest_dist(qs, qe, s, e) as above:
 *     side         with a = s - qe and b = qs - e in 64 bits, a record with d > 0 lies DOWNSTREAM if a >= b, else UPSTREAM.  The
 *                  formula is applied literally to zero-length and inverted regions.  There is no strand: upstream means lower
 *                  coordinates.
 *     key          2 d + (d > 0 && downstream), unsigned 32-bit (igd_hip_nearest_key).  d <= 2^30, so key <= 2^31 + 1 <
 *                  0xffffffff, which stays "none".  The nearest record of file f is the one of MINIMUM KEY over the records
 *                  within the window (d <= W; with a value filter the passing ones): at equal d on both sides upstream wins.
 *                  The minimum of a key does not depend on the order of the records.
 *     sdist[q][f]  int32: IGD_HIP_NEAREST_NO_RECORD = INT32_MIN when there is none; otherwise -(key >> 1) for an even non-zero
 *                  key, +(key >> 1) for an odd key, 0 for key 0 (igd_hip_nearest_key_decode).
 *     sdmin[q]     the same decoding of the minimum key over the files.
 *     identities   abs(sdist) == dist wherever dist >= 0, and sdist == NO_RECORD iff dist == -1; the same pair for sdmin, dmin.
 *     edges        int32[ne], strictly ascending, 1 <= ne <= IGD_HIP_NEAREST_MAX_EDGES = 63; anything else is IGD_HIP_ERR_ARG.
 *     bin(x)       #{k : edges[k] <= x}, in 0 .. ne: bin 0 is "below edges[0]", bin ne "at or above the last edge".
 *     hist         int64[nsets][ne + 1][nFiles + 1]: hist[k][b][f] = the regions q of set k with sdist[q][f] != NO_RECORD and
 *                  bin(sdist[q][f]) == b; column nFiles is built from sdmin.  Regions with no record within the window are in
 *                  no bin: hist.sum(axis = 1) == igd_hip_nearest_sets' n_within, and with edges = (0, 1) bin 1 is n_overlap.
 * igd_hip_nearest_signed / _signed_dev: the chunks, checks and "a call defines every word" of igd_hip_nearest / _dev; sdmin may
 * be NULL.  igd_hip_nearest_hist: the groups and chunks of igd_hip_nearest_sets -- whole sets are taken while (ne + 1) x
 * (nFiles + 1) words per set fit the row budget of igd_hip_support_sets, a set may be cut by a chunk, kernel igd_nearest_hist adds
 * every chunk's rows into the resident histogram; the rows never leave the device and hist is copied out once per group.
 * nsets == 0 writes nothing; without regions or without files every word of hist is 0.  IGD_HIP_ERR_ARG comes before anything
 * of the caller's is written.
 * Not done: an unbounded nearest, the permutation null of a bin, several devices. */
#define IGD_HIP_NEAREST_NO_RECORD INT32_MIN
#define IGD_HIP_NEAREST_MAX_EDGES 63
/* key of one (region, record) pair */
static inline IGD_HIP_OV_HD_ uint32_t igd_hip_nearest_key(int32_t qs, int32_t qe, int32_t start, int32_t end)
{
    if (start < qe && end > qs) return 0;
    const int64_t a = (int64_t)start - (int64_t)qe, b = (int64_t)qs - (int64_t)end;
    return a >= b ? (uint32_t)(2 * (a + 1) + 1) : (uint32_t)(2 * (b + 1));
}
/* sdist of a minimum key (0xffffffff: none) */
static inline IGD_HIP_OV_HD_ int32_t igd_hip_nearest_key_decode(uint32_t key)
{
    const int32_t d = (int32_t)(key >> 1);
    return key == 0xffffffffu ? IGD_HIP_NEAREST_NO_RECORD : (key & 1u) ? d : -d;
}
/* bin of x: the number of edges <= x */
static inline IGD_HIP_OV_HD_ int igd_hip_nearest_bin(const int32_t *edges, int ne, int32_t x)
{
    int b = 0;
    while (b < ne && edges[b] <= x) b++;
    return b;
}
/* 1 <= ne <= IGD_HIP_NEAREST_MAX_EDGES strictly ascending edges */
static inline int igd_hip_nearest_edges_valid(const int32_t *edges, int64_t ne)
{
    if (!edges || ne < 1 || ne > IGD_HIP_NEAREST_MAX_EDGES) return 0;
    for (int64_t k = 1; k < ne; k++) if (edges[k] <= edges[k - 1]) return 0;
    return 1;
}
int igd_hip_nearest_signed(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t window,
                           int32_t v, int32_t *sdist, int32_t *sdmin);
int igd_hip_nearest_signed_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq,
                               int32_t window, int32_t v, int32_t *d_sdist, int32_t *d_sdmin, void *stream);
int igd_hip_nearest_hist(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                         int32_t nsets, int32_t window, int32_t v, const int32_t *edges, int32_t ne, int64_t *hist);

/* Flanking records per dataset and the relative-distance histogram: the nearest record on EACH side of every region
 * (`bedtools closest -D ref -io -iu` / `-id`: the next gene on either side of a peak) and `bedtools reldist`, the relative-distance
 * test of GenometriCorr.  THE DEFINITIONS (the one place: kernels igd_flank_rows and igd_flank_reldist, igdc_flank_host /
 * igdc_flank_reldist_host and the tests' numpy reference agree on every integer).  A record (s, e) of file f is COUNTED for
 * region (qs, qe) under window W when igd_hip_nearest counts it: igd_hip_nearest_dist(qs, qe, s, e) <= W, and with a value filter
 * when value >= v.  Two measures, chosen per call:
 *     IGD_HIP_FLANK_EDGES      with d, a = s - qe and b = qs - e as above, a counted record with d > 0 is DOWNSTREAM if a >= b,
 *                              else UPSTREAM, at distance d; a record with d == 0 (overlapping) is on neither side.  W: 0 .. 2^30.
 *     IGD_HIP_FLANK_MIDPOINTS  mid(x, y) = floor((x + y) / 2) in 64 bits (an arithmetic shift: bedtools' integer midpoint) and
 *                              D = mid(s, e) - mid(qs, qe).  A counted record takes part only if |D| <= W (for a proper region
 *                              and record |D| <= W implies d <= W; the conjunction keeps the formula literal for zero-length and
 *                              inverted regions).  It is UPSTREAM at distance -D if D < 0 and DOWNSTREAM at distance D if
 *                              D >= 0: an equal midpoint is "right", as reldist's lower_bound.
 *     up[q][f]     int32: the minimum distance over the upstream records of file f that take part, -1 when there is none;
 *     down[q][f]   the same over the downstream ones.  Edges: both >= 1.  Midpoints: up >= 1, down >= 0.  Every value is <= 2^30,
 *                  so the unsigned word 0xffffffff stays "none" while minimising, as in igd_hip_nearest.
 *     upmin[q], downmin[q]   the minima over the files (-1: none).
 *     degenerate   the formulas are applied literally to zero-length and inverted regions; a region on an unknown contig has rows
 *                  of -1; there is no strand (upstream means lower coordinates); a minimum does not depend on record order.
 *     flanked      a pair (q, f) with up >= 0 && down >= 0 && up + down > 0 (igd_hip_flank_flanked).
 *     bin          of a flanked pair, for B bins, 1 <= B <= IGD_HIP_FLANK_MAX_BINS = 64:
 *                  min(B - 1, floor(2 B min(up, down) / (up + down))), 64-bit integer arithmetic, exact everywhere
 *                  (igd_hip_flank_bin).  The relative distance min / (up + down) lies in [0, 0.5]; B = 50 gives reldist's bins of
 *                  0.01, with 0.5 folded into the last.
 *     hist         int64[nsets][B][nFiles + 1]: hist[k][b][f] = the regions q of set k whose pair (q, f) is flanked and in bin b;
 *                  column nFiles is computed from upmin / downmin (any dataset).  hist.sum(axis = 1) is n_flanked.
 * igd_hip_flank: up and down are int32[nq * nFiles] (both required when there are files), upmin and downmin int32[nq] (either
 * may be NULL).  The regions go through in igd_hip_nearest's chunks with two rows per region: at most igd_hip_max_batch()
 * regions and IGD_HIP_NEAREST_ROW_BYTES / (8 nFiles) regions.  A call defines every word.
 * igd_hip_flank_dev: device pointers, one engine batch (nq above igd_hip_max_batch() is IGD_HIP_ERR_ARG), enqueued on `stream`
 * (NULL: the engine's own) without waiting; d_up and d_down are overwritten, d_upmin and d_downmin may each be NULL.
 * igd_hip_flank_reldist: the groups and chunks of igd_hip_nearest_hist -- whole sets are taken while B x (nFiles + 1) words per
 * set fit the row budget of igd_hip_support_sets, a set may be cut by a chunk, kernel igd_flank_reldist adds every chunk's rows
 * into the resident histogram; the rows never leave the device and hist is copied out once per group.  The histogram is built
 * from the two rows alone, so it serves both measures.  nsets == 0 writes nothing; without regions or without files every word
 * of hist is 0.
 * Blocking (but for _dev), one device.  IGD_HIP_ERR_ARG -- W out of range, a measure that is neither, B outside 1 .. 64, a
 * missing array, a bad set_off -- comes before anything of the caller's is written.
 * Not done: unbounded flanks, the permutation null of a bin, several devices. */
#define IGD_HIP_FLANK_EDGES 0
#define IGD_HIP_FLANK_MIDPOINTS 1
#define IGD_HIP_FLANK_MAX_BINS 64
#define IGD_HIP_FLANK_NEITHER 0
#define IGD_HIP_FLANK_UP 1
#define IGD_HIP_FLANK_DOWN 2
static inline IGD_HIP_OV_HD_ int igd_hip_flank_measure_valid(int measure) { return measure == IGD_HIP_FLANK_EDGES || measure == IGD_HIP_FLANK_MIDPOINTS; }
static inline IGD_HIP_OV_HD_ int igd_hip_flank_bins_valid(int64_t nbins) { return nbins >= 1 && nbins <= IGD_HIP_FLANK_MAX_BINS; }
static inline IGD_HIP_OV_HD_ int64_t igd_hip_flank_mid(int32_t x, int32_t y) { return ((int64_t)x + (int64_t)y) >> 1; }
/* the side of one COUNTED (region, record) pair -- IGD_HIP_FLANK_NEITHER, _UP or _DOWN -- and, on a side, its distance in *dist */
static inline IGD_HIP_OV_HD_ int igd_hip_flank_pair(int measure, int32_t window, int32_t qs, int32_t qe, int32_t start, int32_t end,
                                                    uint32_t *dist)
{
    if (measure == IGD_HIP_FLANK_MIDPOINTS) {
        const int64_t D = igd_hip_flank_mid(start, end) - igd_hip_flank_mid(qs, qe);
        if (D < -(int64_t)window || D > (int64_t)window) return IGD_HIP_FLANK_NEITHER;
        *dist = (uint32_t)(D < 0 ? -D : D);
        return D < 0 ? IGD_HIP_FLANK_UP : IGD_HIP_FLANK_DOWN;
    }
    if (start < qe && end > qs) return IGD_HIP_FLANK_NEITHER;
    const int64_t a = (int64_t)start - (int64_t)qe, b = (int64_t)qs - (int64_t)end;
    *dist = (uint32_t)((a >= b ? a : b) + 1);
    return a >= b ? IGD_HIP_FLANK_DOWN : IGD_HIP_FLANK_UP;
}
static inline IGD_HIP_OV_HD_ int igd_hip_flank_flanked(int32_t up, int32_t down) { return up >= 0 && down >= 0 && (int64_t)up + (int64_t)down > 0; }
/* bin of a flanked pair */
static inline IGD_HIP_OV_HD_ int igd_hip_flank_bin(int nbins, int32_t up, int32_t down)
{
    const int64_t m = up < down ? up : down, k = 2 * (int64_t)nbins * m / ((int64_t)up + (int64_t)down);
    return (int)(k < nbins - 1 ? k : nbins - 1);
}
int igd_hip_flank(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t window, int measure,
                  int32_t v, int32_t *up, int32_t *down, int32_t *upmin, int32_t *downmin);
int igd_hip_flank_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq, int32_t window,
                      int measure, int32_t v, int32_t *d_up, int32_t *d_down, int32_t *d_upmin, int32_t *d_downmin, void *stream);
int igd_hip_flank_reldist(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                          int32_t nsets, int32_t window, int measure, int32_t v, int32_t nbins, int64_t *hist);

/* Values of the overlapping records per region and dataset: how many records of every file lie under each region and what they
 * are worth -- `bedtools map -c 5 -o count,sum,min,max,mean`, the regions x datasets feature matrix.  THE DEFINITIONS (the one
 * place: kernel igd_map_rows, igdc_map_host and the tests' numpy reference agree on every integer).
 *     counted      A record (idx = f, s, e, val) is counted for region (c, qs, qe) iff it lies on contig c, s < qe && e > qs and,
 *                  with a value filter v on a database that has values (gType 1), val >= v.  Each record is counted once,
 *                  however many tiles hold a copy of it.  This is "distance 0" of igd_hip_nearest_dist.
 *     no rule      As igd_hip_nearest at W = 0: igd_hip_nearest_widen(qs, qe, 0), walked under rule FLAT on the image
 *                  igd_hip_support_sets walks.  An unknown contig has an empty row; zero-length and inverted regions are not
 *                  special-cased, the predicate decides.
 *     op           IGD_HIP_MAP_COUNT, _SUM, _MIN, _MAX; anything else is IGD_HIP_ERR_ARG.  SUM, MIN and MAX on a gType 0
 *                  database (no values) are IGD_HIP_ERR_ARG; COUNT works on both types.
 *     count[q][f]  the number of counted records, int32.
 *     agg[q][f]    the sum, minimum or maximum of val over the counted records, sign-extended to int64; the sum is exact in
 *                  64-bit two's complement.  0 where count is 0.  Under op COUNT agg may be NULL; when it is given it receives
 *                  the counts (agg_sum below is defined the same way).
 *     sets         For set k = regions [set_off[k], set_off[k + 1]) each statistic is int64[nsets][nFiles]:
 *                      n_hit[k][f] = #{q : count[q][f] > 0}      pairs[k][f] = the sum of count[q][f]
 *                      agg_sum[k][f] = the sum of agg[q][f]      (COUNT: equal to pairs)
 *                  igdc_map_summary (igd_core.h) derives mean_region = agg_sum / n_hit and, for SUM, mean_pair = agg_sum / pairs.
 *     identities   count > 0 iff igd_hip_nearest(W = 0).dist == 0; n_hit is igd_hip_nearest_sets(W = 0).n_overlap without its
 *                  last column; over regions with 0 <= qs that start inside the contig's tiles the column sums of count are the
 *                  hits of igd_hip_search under rule FLAT.
 * Every output is DEFINED by the call: every word is written, nothing is added to.
 * igd_hip_map: count is int32[nq * nFiles], agg int64[nq * nFiles].  The regions go through in chunks of at most
 * igd_hip_max_batch() regions and 256 MiB of device rows (TEST-ONLY: IGD_HIP_MAP_ROW_BYTES lowers it).
 * igd_hip_map_sets: whole sets are taken while their three result rows fit the row budget of igd_hip_support_sets, their regions
 * go through in the chunks above (a set may be cut by a chunk), kernel igd_map_reduce adds every chunk's rows into the three
 * resident matrices; the rows never leave the device and the matrices are copied out once per group.  Any of the three may be NULL.
 * igd_hip_map_dev: device pointers, one engine batch (nq above igd_hip_max_batch() is IGD_HIP_ERR_ARG), enqueued on `stream`
 * (NULL: the engine's own) without waiting; d_count and d_agg are overwritten.
 * Blocking (but for _dev), one device.  IGD_HIP_ERR_ARG -- a missing array, a bad set_off, an unknown op, a value op on gType 0
 * -- comes before anything of the caller's is written.  nFiles == 0: rows of no words.
 * Not done: an any-dataset column, a per-region mean array (it is agg / count on the caller's side), a minimum overlap, a
 * window, median and other order statistics, several devices. */
#define IGD_HIP_MAP_COUNT 0
#define IGD_HIP_MAP_SUM 1
#define IGD_HIP_MAP_MIN 2
#define IGD_HIP_MAP_MAX 3
static inline IGD_HIP_OV_HD_ int igd_hip_map_op_valid(int op) { return op >= IGD_HIP_MAP_COUNT && op <= IGD_HIP_MAP_MAX; }
int igd_hip_map(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int op, int32_t v, int32_t *count,
                int64_t *agg);
int igd_hip_map_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                     int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum);
int igd_hip_map_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq, int op, int32_t v,
                    int32_t *d_count, int64_t *d_agg, void *stream);
/* Workgroups (of four waves) igd_map_rows is launched with for nq regions: a wave meets a second region only when nq exceeds four
 * times this number (tests). */
int32_t igd_hip_map_grid(int64_t nq);

/* Merged region sets and the base-pair Jaccard per set and dataset: `bedtools merge -d gap` on the device, and per set k and
 * dataset f what `bedtools jaccard` reports -- |A_k n B_f|, |A_k u B_f| -- with one extra column nFiles for "any dataset".  THE
 * DEFINITIONS (the one place: the kernels igd_merge_*, igdc_merge_host / igdc_dataset_bp_host / igdc_jaccard_host and the
 * tests' reference agree on every integer).
 *     gap          0 <= gap <= IGD_HIP_MERGE_MAX_GAP = 2^30; anything else is IGD_HIP_ERR_ARG.
 *     takes part   A region (ichr, qs, qe) takes part iff 0 <= ichr < the database's contigs and qe > qs (igd_hip_merge_takes_part).
 *                  Regions on unknown contigs, zero-length and inverted regions are dropped; n_dropped[k] counts them per set.
 *     runs         Within set k the regions that take part are ordered by (ichr, qs, qe).  A region OPENS A RUN iff it is the
 *                  first of its (set, contig) or qs > E + gap in 64 bits, E being the maximum qe of all earlier regions of the
 *                  same (set, contig) (igd_hip_merge_opens; qs and E reach INT32_MAX, the sum does not wrap).  At gap 0
 *                  book-ended regions join, as in bedtools.  A run is (ichr, its first qs, its maximum qe).
 *     outputs      m_ichr, m_qs, m_qe: int32, capacity n = set_off[nsets], the runs ordered by (set, ichr, qs); m_off:
 *                  int64[nsets + 1], the runs of set k are [m_off[k], m_off[k + 1]); m_count (may be NULL): int32 per run, the
 *                  regions it joined (`merge -c 1 -o count`); n_dropped: int64[nsets].  Words of the capacity behind the
 *                  last run are 0.  The result does not depend on the order of the regions within a set.
 *     set_bp[k]    the sum of qe - qs over the runs of set k AT GAP 0 (the Jaccard is always taken at gap 0).
 *     inter[k][f]  int64[nsets][nFiles + 1]: for f < nFiles igd_hip_coverage_sets' coverage of the runs of set k, column nFiles
 *                  its covered[].  The runs are disjoint, so this is |A_k n B_f| exactly; B_f is the union of the records of
 *                  file f that the search counts under the rule and v given.
 *     file_bp[f]   int64[nFiles + 1]: |B_f|, column nFiles the union over all files.  It is igd_hip_coverage_sets over ONE set
 *                  that holds every tile of every contig of the database as one query, [t nbp, (t + 1) nbp) with the end capped
 *                  at INT32_MAX (igd_hip_tile_query): the queries partition the contig and coverage clips to the query, so the
 *                  sum is exact.  Kept in the handle per (v, rule) once computed; a gType-0 database has one entry per rule.
 *     jaccard      inter / (set_bp + file_bp - inter) as a double, NaN where the union is 0.  The engine returns integers
 *                  only; igdc_jaccard_value (igd_core.h) and igd_amd.jaccard_summary derive it.
 * igd_hip_merge_sets: host arrays in and out, blocking.  igd_hip_merge_sets_dev: device pointers, n = the number of regions
 * (d_set_off is resident, so the host cannot read it), enqueued on `stream` (NULL: the engine's own) without waiting; the
 * caller reads d_m_off[nsets] back to learn the number of runs.  Every merge of a handle works in the handle's ONE workspace:
 * calls on one handle -- both forms, and igd_hip_jaccard_sets -- must be ORDERED with respect to each other (the same stream, or an
 * event between two streams); two merges of one handle in flight on different streams race.  igd_hip_dataset_bp: file_bp as above.
 * igd_hip_dataset_bp_computed: how many times the handle has computed (not found) one.  igd_hip_jaccard_sets: inter, set_bp,
 * file_bp, n_merged[k] = the runs of set k, n_dropped.
 * Every output is DEFINED by the call.  nsets == 0 writes nothing (igd_hip_jaccard_sets: file_bp only); without regions the
 * offsets and counts are 0; nFiles == 0 leaves the any-dataset column, 0.  IGD_HIP_ERR_ARG -- a bad gap, a bad set_off, a
 * missing array, more than 2^30 regions -- comes before anything of the caller's is written.  One device.
 * Not done: strand, a gap on the Jaccard, Jaccard between two query sets, a permutation null, several devices. */
#define IGD_HIP_MERGE_MAX_GAP ((int64_t)1 << 30)
static inline IGD_HIP_OV_HD_ int igd_hip_merge_gap_valid(int64_t gap) { return gap >= 0 && gap <= IGD_HIP_MERGE_MAX_GAP; }
static inline IGD_HIP_OV_HD_ int igd_hip_merge_takes_part(int32_t nctg, int32_t ichr, int32_t qs, int32_t qe) { return ichr >= 0 && ichr < nctg && qe > qs; }
/* a region that is not the first of its (set, contig): E is the maximum end before it */
static inline IGD_HIP_OV_HD_ int igd_hip_merge_opens(int32_t qs, int32_t E, int64_t gap) { return (int64_t)qs > (int64_t)E + gap; }
/* tile t of a contig as a query; 0 when the tile begins at or behind INT32_MAX (no region can lie there) */
static inline IGD_HIP_OV_HD_ int igd_hip_tile_query(int32_t nbp, int64_t t, int32_t *ws, int32_t *we)
{
    const int64_t a = t * (int64_t)nbp, b = a + (int64_t)nbp;
    if (a >= (int64_t)INT32_MAX) return 0;
    *ws = (int32_t)a;
    *we = (int32_t)(b > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : b);
    return 1;
}
int igd_hip_merge_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                       int64_t gap, int32_t *m_ichr, int32_t *m_qs, int32_t *m_qe, int64_t *m_off, int32_t *m_count, int64_t *n_dropped);
int igd_hip_merge_sets_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, const int64_t *d_set_off,
                           int32_t nsets, int64_t n, int64_t gap, int32_t *d_m_ichr, int32_t *d_m_qs, int32_t *d_m_qe, int64_t *d_m_off,
                           int32_t *d_m_count, int64_t *d_n_dropped, void *stream);
int igd_hip_dataset_bp(igd_hip_db *db, int32_t v, int rule, int64_t *file_bp);
int64_t igd_hip_dataset_bp_computed(const igd_hip_db *db);
int igd_hip_jaccard_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                         int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *file_bp, int64_t *n_merged, int64_t *n_dropped);

/* The permutation null of the base-pair overlap: "does my region set share more base pairs with dataset f than chance" (GAT's
 * nucleotide overlap, regioneR's permTest with numOverlaps in bp).  THE DEFINITIONS (the one place: the kernels of
 * permute_bp_dev.hpp, igdc_permute_bp_host and the tests' reference agree on every integer).
 *     inputs       one set of nq regions; ctg_len, mode, seed and nperm exactly as for igd_hip_permute_support (the generator is
 *                  igd_hip_perm_place below; 0 <= s <= e <= L on known contigs; nperm 1 .. IGD_HIP_PERM_MAX; nq <=
 *                  igd_hip_max_batch(); no sum of squares is taken, so that call's sumsq guard does not apply); v and rule
 *                  as for igd_hip_jaccard_sets.
 *     rows         Row 0 is the set as given, row p + 1 the set under permutation p.  Every row is treated as
 *                  igd_hip_jaccard_sets treats a set: its regions are merged at gap 0 (igd_hip_merge_takes_part,
 *                  igd_hip_merge_opens; zero-length regions and regions on unknown contigs are dropped), and the runs are
 *                  covered as igd_hip_coverage_sets covers them.  Every row is merged ANEW: both modes can put a region
 *                  over another (`circular` pushes a region that would cross the contig's end back against it).
 *     inter        int64[nperm + 1][nFiles + 1]: column f is |row n union of the records of dataset f| in bp, column nFiles
 *                  the same against any dataset (the coverage stage's covered[]).
 *     set_bp       int64[nperm + 1]: the merged bp of the row; it varies per permutation, overlaps come and go.
 *     n_merged     int64[nperm + 1]: the runs of the row.
 *     n_dropped    one int64: the regions that take no part -- the same in every row, a permutation moves neither a
 *                  zero-length region onto a length nor a region onto a known contig.
 * Any output may be NULL; all are DEFINED by the call.  file_bp is igd_hip_dataset_bp and is not computed again.  The null
 * distribution itself comes back, not moments of it: with x in base pairs x^2 passes 2^63 from x = 3.04 x 10^9, one human
 * genome's worth; igdc_perm_bp_summary (igd_core.h) takes the summary on the host.
 * Chunks of pc permutations, pc * nq <= igd_hip_max_batch() and pc * nFiles * 8 <= the row budget of igd_hip_permute_support
 * (TEST-ONLY: IGD_HIP_PERM_ROW_BYTES); per chunk igd_permute_regions, the merge launches, igd_merge_slices, igd_sets_coverage,
 * igd_merge_row_bp and the copies, enqueued without a wait or a host copy in between: the merged runs stay on the device.
 * igd_hip_merge_slices_per_row: the slice slots every row gets when pc rows of nq regions are handed over (tests):
 * ceil(nq / L) with L = clamp(ceil(pc nq / 4096), 64, 4096), the slice length of igd_hip_coverage_sets for pc nq queries.
 * IGD_HIP_ERR_ARG before any launch, nothing of the caller's written: a missing array, no such rule or mode, nperm < 1 or >
 * IGD_HIP_PERM_MAX, nq > igd_hip_max_batch(), a region on a known contig outside 0 <= s <= e <= L.  nq == 0: all zeros;
 * nFiles == 0: inter is zeros, set_bp and n_merged are still the rows'.  Blocking, one device; ordered with the other merges
 * of the handle as igd_hip_merge_sets is.
 * Not done: several sets in one call, a gap other than 0, regions split at a contig's end, several devices,
 * igd_hip_jaccard_sets itself on the resident hand-over. */
int igd_hip_permute_bp(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                       int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged,
                       int64_t *n_dropped);
int64_t igd_hip_merge_slices_per_row(int64_t pc, int64_t nq);
/* Rows of workgroups (the grid's y) that the reductions over a slice table -- igd_nearest_reduce, igd_nearest_hist,
 * igd_flank_reldist, igd_map_reduce -- are launched with for nslices slices of a matrix of ncols columns (nFiles + 1 for the
 * nearest family, nFiles for igd_hip_map_sets): clamp(16384 / ceil(ncols / 64), 1, min(nslices, 65535)).  Workgroup (x, y) takes
 * the slices y, y + this number, ..: it meets a second slice only when nslices exceeds it (tests; TEST-ONLY: IGD_HIP_REDUCE_WGS
 * lowers the 16384, read once per process). */
int32_t igd_hip_reduce_grid_y(int64_t ncols, int64_t nslices);
/* TEST-ONLY: the two device primitives everything above is built on (igd_sortscan.hpp), on host arrays.  Both block, need no
 * handle, and free what they allocate.  They run the instantiations the engine itself uses, with workspaces of exactly the
 * promised sizes (hist 256 * nBlocks uint32, digitBase as many int64, sums ceil(len / SCAN_TILE) + 1 int64) and 256 guard
 * bytes behind every device array: IGD_HIP_ERR_DEVICE, igd_hip_last_error naming the array, when one of them was written.
 * igd_hip_test_exclusive_scan: out[i] = in[0] + .. + in[i - 1] and *total = the sum of all, in 64 bits.  n == 0 is IGD_HIP_OK
 * with *total = 0 and nothing else touched.
 * igd_hip_test_radix_sort_pairs: (keys, vals) sorted in place, stably, by the low 8 * ceil(bits / 8) bits of the key (the
 * engine's callers pass keys below 2^bits); bits == 0 and n == 0 leave both arrays as they are.
 * IGD_HIP_ERR_ARG with nothing written: n < 0 or n > 2^31, a null array, bits outside 0 .. 32, no such device. */
int igd_hip_test_exclusive_scan(int device, const uint32_t *in, int64_t n, int64_t *out, int64_t *total);
int igd_hip_test_radix_sort_pairs(int device, uint32_t *keys, uint32_t *vals, int64_t n, int bits);

/* The set statistics without the distance rows, and their permutation null (kernel igd_nearest_slices: the walk and table of
 * igd_nearest_rows, folded per region into LDS accumulators of the slice; nothing per region reaches memory).
 * igd_hip_nearest_sets_fused: the contract, checks and outputs of igd_hip_nearest_sets, every integer the same.  Groups of
 * whole sets within the row budget of igd_hip_support_sets, regions in chunks of igd_hip_max_batch(), one launch per chunk.
 * igd_hip_permute_nearest: "are my regions closer to dataset f than chance" (regioneR's permTest with meanDistance).  Each
 * output is int64[nperm + 1][nFiles + 1] (any may be NULL): row 0 the statistics of the set as given, row p + 1 those of
 * permutation p of THE GENERATOR below (igd_hip_perm_place; mode, seed and ctg_len as igd_hip_permute_support), column nFiles
 * the any-dataset column.  The null distribution itself comes back, not moments of it: the statistic of interest,
 * sum_dist / n_within, is a ratio of two columns that both vary per permutation (igdc_perm_nearest_summary, igd_core.h).
 * Chunks of pc permutations, pc * nq <= igd_hip_max_batch() and 3 * pc * (nFiles + 1) * 8 <= the row budget of
 * igd_hip_permute_support (TEST-ONLY: IGD_HIP_PERM_ROW_BYTES); per chunk igd_permute_regions, a memset, igd_nearest_slices
 * and a copy, enqueued without a wait.  IGD_HIP_ERR_ARG before any launch, nothing of the caller's written: W out of range, a
 * missing array, no such mode, nperm < 1 or > IGD_HIP_PERM_MAX, nq > igd_hip_max_batch(), a region on a known contig outside
 * 0 <= s <= e <= L.  nq == 0 or nFiles == 0: all zeros.  Blocking, one device.
 * Databases with more than igd_hip_nearest_fused_max_files() files take igd_nearest_rows + igd_nearest_reduce instead (there
 * is no wide form of the fused kernel); the results are the same.  igd_hip_nearest_fused_grid: workgroups the fused kernel is
 * launched with for nslices slices (tests: a workgroup takes a second slice only past this number).
 * Not done: several sets or a set list under the permutation, signed or unbounded distances, a minimum overlap, several devices. */
int igd_hip_nearest_sets_fused(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                               int32_t nsets, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist);
int igd_hip_permute_nearest(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                            int mode, uint64_t seed, int64_t nperm, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap,
                            int64_t *sum_dist);
int32_t igd_hip_nearest_fused_max_files(void);
int32_t igd_hip_nearest_fused_grid(int64_t nslices);

/* Fisher's exact test, one-sided ("greater"), of many 2x2 tables  a b / c d  in one call (kernel igd_fisher_cells).  With
 * N = a+b+c+d, K = a+b, n = a+c and X ~ Hypergeometric(N, K, n):
 *     pvalue_log[i] = -log10 P(X >= a)   a double >= 0, computed in log space: finite however small p is (a p of 10^-4609
 *                                        is 4609.06), exactly +0.0 when a is the support minimum max(0, n - (N - K)) or N = 0
 *     odds_ratio[i] = (a d) / (b c)      in double: the SAMPLE odds ratio (not the conditional maximum-likelihood estimate
 *                                        R's fisher.test reports); +inf when b c = 0 < a d, NaN when both products are 0
 * Both are DEFINED by the call (overwritten); odds_ratio may be NULL.  Blocking.  A table with a negative entry or with
 * N >= 2^31 is IGD_HIP_ERR_ARG before any launch, the caller's outputs untouched. */
int igd_hip_fisher_tables(igd_hip_db *db, const int64_t *a, const int64_t *b, const int64_t *c, const int64_t *d,
                          int64_t ncell, double *pvalue_log, double *odds_ratio);
/* Region-set enrichment of many query sets against a universe, in one call.  Sets as igd_hip_search_sets; the universe is
 * the nu regions u_ichr / u_qs / u_qe.  With support as igd_hip_support_sets defines it (same rule and v for the sets and
 * the universe), n_k = |set k| and n_U = nu, the table of set k and file f is
 *     a = support[k * nFiles + f]      b = usupport[f] - a      c = n_k - a      d = n_U - a - b - c  (= n_U - usupport[f] - c)
 * where a negative b or d is then set to 0 and clamped[k] counts the cells of set k where that happened (a set region
 * outside the universe, or a universe region under several set regions).  igd_hip_enrich_restricted restricts the sets to the
 * universe first; its tables are partitions of the universe and need no clamp.
 *     support[nsets * nFiles], usupport[nFiles]                     the counts (the universe is counted once)
 *     pvalue_log[nsets * nFiles], odds_ratio[nsets * nFiles]        as igd_hip_fisher_tables on these tables, bit for bit
 *     clamped[nsets]
 * All are DEFINED by the call, not added to; odds_ratio and clamped may be NULL.  One igd_hip_support_sets call over the
 * nsets + 1 sets, then the cell kernel on the resident counts.  Blocking.  The argument checks of igd_hip_support_sets
 * apply; a set that with the universe holds 2^31 regions or more is IGD_HIP_ERR_ARG.  On an error nothing of the caller's
 * is written.  One device.  Ranks and q-values of the table: igd_hip_enrich_ranks. */
int igd_hip_enrich_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                        int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu,
                        int32_t v, int rule, int64_t *support, int64_t *usupport, double *pvalue_log, double *odds_ratio,
                        int64_t *clamped);
/* The same, and the regions with a hit in any file: nhit[nsets] for the sets, *unhit for the universe (what
 * igd_hip_support_sets adds to nhit; here DEFINED; both may be NULL) -- the last line of `igd search -U`. */
int igd_hip_enrich_sets_nhit(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                             int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu,
                             int32_t v, int rule, int64_t *support, int64_t *usupport, double *pvalue_log, double *odds_ratio,
                             int64_t *clamped, int64_t *nhit, int64_t *unhit);
/* The same under a minimum overlap (igd_hip_min_overlap above): the supports of the sets AND of the universe are taken under
 * the threshold, as LOLA's runLOLA(minOverlap=) does; the tables, the Fisher cells and the clamp are formed as before. */
int igd_hip_enrich_sets_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                           int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu,
                           int32_t v, int rule, int64_t *support, int64_t *usupport, double *pvalue_log, double *odds_ratio,
                           int64_t *clamped, int64_t *nhit, int64_t *unhit, const igd_hip_min_overlap *min_overlap);
/* DATASET GROUPS: support and enrichment per group of datasets -- "how many of my regions lie under ANY track of this cell
 * type" -- which is a union over datasets: neither the sum nor the maximum of the per-dataset supports.
 * A grouping of the nFiles datasets into ngroups groups is a many-to-many relation in CSR form:
 *     grp_off   int32[nFiles + 1], grp_off[0] = 0, non-decreasing
 *     grp_idx   int32[grp_off[nFiles]], every entry in [0, ngroups), strictly ascending within one dataset's run
 * A dataset may be in no group, in one or in several; a group may be empty.  1 <= ngroups <= IGD_HIP_GROUP_MAX.
 * With F_q = the datasets f with hits_q[f] > 0 as igd_hip_support_sets defines it (same rule, v and minimum overlap):
 *     gsupport[k * ngroups + g] += the queries q of set k for which F_q holds a dataset of group g
 *     gnhit[k]                  += the queries q of set k for which F_q holds a dataset with at least one group  (may be NULL)
 * So: the identity grouping gives support and nhit of igd_hip_support_sets bit for bit; one group of all datasets gives nhit
 * in its only column; max over f in g of support[f] <= gsupport[g] <= min(sum over f in g of support[f], |set|); two identical
 * queries count twice; an empty group has a zero column; an unlabelled dataset changes nothing.
 * One kernel (igd_sets_group_support) counts all sets in the chunks of igd_hip_support_sets with rows of ngroups columns; the
 * table goes to the device once per call; no membership matrix exists anywhere.  Blocking.  A bad set_off, a bad grouping
 * (the message names the first bad entry) or ngroups outside 1 .. IGD_HIP_GROUP_MAX is IGD_HIP_ERR_ARG before any launch and
 * before anything of the caller's is written.  min_overlap may be NULL.
 * igd_hip_groups_first_bad is that check of the grouping, shared with the host route: 0, or which rule the first bad entry
 * breaks with its index in *at (an index into grp_off for IGD_HIP_GROUPS_BAD_OFF, into grp_idx otherwise). */
#define IGD_HIP_GROUP_MAX 8192
enum { IGD_HIP_GROUPS_OK = 0, IGD_HIP_GROUPS_BAD_OFF = 1, IGD_HIP_GROUPS_BAD_RANGE = 2, IGD_HIP_GROUPS_BAD_ORDER = 3, IGD_HIP_GROUPS_BAD_NULL = 4 };
static inline int igd_hip_groups_first_bad(int32_t nfiles, const int32_t *grp_off, const int32_t *grp_idx, int32_t ngroups, int64_t *at)
{
    if (grp_off[0] != 0) { *at = 0; return IGD_HIP_GROUPS_BAD_OFF; }
    for (int32_t f = 0; f < nfiles; f++) {
        if (grp_off[f + 1] < grp_off[f]) { *at = (int64_t)f + 1; return IGD_HIP_GROUPS_BAD_OFF; }
        if (grp_off[f + 1] > grp_off[f] && !grp_idx) { *at = grp_off[f]; return IGD_HIP_GROUPS_BAD_NULL; }
        for (int32_t j = grp_off[f]; j < grp_off[f + 1]; j++) {
            if (grp_idx[j] < 0 || grp_idx[j] >= ngroups) { *at = j; return IGD_HIP_GROUPS_BAD_RANGE; }
            if (j > grp_off[f] && grp_idx[j] <= grp_idx[j - 1]) { *at = j; return IGD_HIP_GROUPS_BAD_ORDER; }
        }
    }
    return IGD_HIP_GROUPS_OK;
}
int igd_hip_group_support_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                               int32_t nsets, const int32_t *grp_off, const int32_t *grp_idx, int32_t ngroups, int32_t v, int rule,
                               int64_t *gsupport, int64_t *gnhit, const igd_hip_min_overlap *min_overlap);
/* Enrichment per group: igd_hip_enrich_sets_ov with the groups as columns.  The table of set k and group g is a =
 * gsupport[k * ngroups + g], b = gusupport[g] - a, c = n_k - a, d = n_U - a - b - c, clamped as there.  gsupport[nsets *
 * ngroups], gusupport[ngroups], pvalue_log / odds_ratio[nsets * ngroups], clamped[nsets], gnhit[nsets] and *gunhit are DEFINED
 * by the call; odds_ratio, clamped, gnhit and gunhit may be NULL.  ONE igd_hip_group_support_sets call over nsets + 1 sets --
 * the universe last, counted once -- then the cell kernel.  Ranks and q-values over a set's groups: igd_hip_enrich_ranks with
 * ncols = ngroups.  The argument checks above apply, and those of igd_hip_enrich_sets. */
int igd_hip_group_enrich_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                              int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu,
                              const int32_t *grp_off, const int32_t *grp_idx, int32_t ngroups, int32_t v, int rule,
                              int64_t *gsupport, int64_t *gusupport, double *pvalue_log, double *odds_ratio, int64_t *clamped,
                              int64_t *gnhit, int64_t *gunhit, const igd_hip_min_overlap *min_overlap);
/* Query sets RESTRICTED to the universe (LOLA's redefineUserSets): each set is replaced by the universe regions it overlaps
 * before anything is counted, so every table is a true 2x2 partition of the universe.  Sets as igd_hip_enrich_sets; the
 * universe is the nu regions u_ichr / u_qs / u_qe in ANY order.
 *     R_k = { u : some region q of set k has ichr_q == u_ichr_u >= 0, u_qs_u < qe_q and u_qe_u > qs_q }
 * -- the plain predicate on the raw int32 numbers, the one the database search uses on records: empty and inverted regions on
 * either side are not special-cased ([5,5) lies "in" [0,10)), regions that touch do not overlap.  A region with ichr < 0
 * overlaps nothing: such a set region is dropped, such a universe region stays in n_U = nu and is in no R_k.  (A caller that
 * maps contig names the database does not know to -1, or drops such lines as the command line tool's reader does, therefore
 * never has a region on such a contig in a restricted set, although the join itself needs no database.)  Duplicate universe
 * regions are distinct members; duplicate set regions add nothing.
 *     bits[nsets * nUW], nUW = ceil(nu / 32)    region u (the caller's numbering) is bit u & 31 of word u >> 5 of row k;
 *                                               bits at positions >= nu are 0
 *     size[k] = |R_k|
 * Both are DEFINED by the call.  Kernel igd_restrict_bits (an interval join over the universe ordered by (ichr, start) with a
 * prefix maximum of the ends), in chunks of sets within a row budget.  Blocking.  The argument checks of igd_hip_enrich_sets
 * apply, and nu + 1 >= 2^31 is IGD_HIP_ERR_ARG; on an error nothing of the caller's is written. */
int igd_hip_restrict_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                          int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu,
                          uint32_t *bits, int64_t *size);
/* Region-set enrichment of the restricted sets.  With member[u][f] as igd_hip_membership defines it for the universe regions
 * (rule and v of this call):
 *     usupport[f]  = sum over u of member[u][f]               support[k * nFiles + f] = sum over u in R_k of member[u][f]
 *     nhit[k]      = the u in R_k with any file               *unhit = the same over the whole universe
 *     a = support   b = usupport[f] - a   c = size[k] - a   d = nu - usupport[f] - c
 * all four >= 0 by construction (d = nu - |R_k u H_f|): there is no clamp and no `clamped`.  pvalue_log and odds_ratio are
 * igd_fisher_cells' on these tables: passing R_k as explicit region lists (the universe's own triples) to igd_hip_enrich_sets
 * gives the same supports, tables and, bit for bit, statistics, with clamped == 0.
 * All outputs are DEFINED by the call; odds_ratio, bits, nhit and unhit may be NULL.  The database is walked once per universe
 * region however many sets there are (igd_hip_membership_dev in chunks; kernel igd_bits_support gathers the member rows of the
 * set bits).  Blocking, one device.  Checks as igd_hip_restrict_sets, before anything of the caller's is written. */
int igd_hip_enrich_restricted(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                              int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu,
                              int32_t v, int rule, int64_t *support, int64_t *usupport, int64_t *size, double *pvalue_log,
                              double *odds_ratio, uint32_t *bits, int64_t *nhit, int64_t *unhit);
/* Workgroups (of 256 lanes, one set region per lane at a time) the join kernel is launched with for nregions set regions: a
 * lane takes a second region only when nregions exceeds 256 times this number (tests). */
int32_t igd_hip_restrict_grid(int64_t nregions);
/* Workgroups (of four waves, one cell per wave at a time) the cell kernel is launched with for ncell cells: a wave takes a
 * second cell only when ncell exceeds four times this number (tests). */
int32_t igd_hip_fisher_grid(int64_t ncell);
/* Rank columns and Benjamini-Hochberg q-values of an enrichment table (kernel igd_rank_rows): the columns of a LOLA table
 * that igd_hip_enrich_sets leaves out.  The three inputs are matrices [nrows x ncols], row-major; a ROW is the ncols cells of
 * one query set and the unit of all work: ranks are taken, and the m = ncols tests corrected, within a row.  ncols is the
 * caller's and not tied to the database (at most IGD_HIP_RANK_MAX_COLS).
 *     rank[f] = 1 + #{g : x[g] > x[f]}     int32; ties take the MINIMUM rank (R: rank(-x, ties.method = "min"))
 *     rnk_sup ranks support (compared as 64-bit integers), rnk_pv pvalue_log, rnk_or odds_ratio, where +inf is the largest
 *     value, NaN ranks below every number and all NaN of a row tie (rank 1 + the number of non-NaN cells)
 *     max_rnk = the largest of the three (int32), mean_rnk = (rnk_sup + rnk_pv + rnk_or) / 3.0 (double, not rounded)
 *     qvalue_log: with r[f] = #{g : pvalue_log[g] >= pvalue_log[f]} and adj[f] = pvalue_log[f] + (log10 r[f] - log10 m),
 *                 qvalue_log[f] = max(+0.0, max{adj[g] : pvalue_log[g] <= pvalue_log[f]})
 *                 = -log10 of the Benjamini-Hochberg adjusted p, min(1, min over j >= i of m p_(j) / j), computed in log10
 *                 throughout: a pvalue_log of 4609.06 keeps a finite q.  It is a function of the cell's value alone (equal
 *                 pvalue_log give bit-equal q), never negative and never -0.0.
 * Any output may be NULL; an input may be NULL when no requested output needs it (max_rnk and mean_rnk need all three).
 * Every requested output is DEFINED by the call (overwritten).  Blocking, on the engine's stream, in chunks of whole rows of
 * at most 2^20 cells.  IGD_HIP_ERR_ARG, before anything of the caller's is written: a needed input is NULL, ncols >
 * IGD_HIP_RANK_MAX_COLS, a pvalue_log that is needed is negative or NaN.  nrows == 0 or ncols == 0 is IGD_HIP_OK and writes nothing.
 * The family is the row: no whole-table correction, no Storey q-value, no two-sided test. */
#define IGD_HIP_RANK_MAX_COLS (1 << 20)
int igd_hip_enrich_ranks(igd_hip_db *db, const int64_t *support, const double *pvalue_log, const double *odds_ratio,
                         int64_t nrows, int64_t ncols, double *qvalue_log, int32_t *rnk_sup, int32_t *rnk_pv,
                         int32_t *rnk_or, int32_t *max_rnk, double *mean_rnk);
/* Workgroups (one row per workgroup at a time) the rank kernel is launched with for nrows rows: a workgroup takes a second
 * row only when nrows exceeds this number; and the widest row whose sort the kernel keeps in LDS -- wider rows are sorted in
 * a global workspace (tests). */
int32_t igd_hip_rank_grid(int64_t nrows);
int32_t igd_hip_rank_lds_cols(void);
/* Dataset x dataset co-occurrence over one region list.  With member[q][f] as igd_hip_membership defines it for the nq regions
 * (rule and v of this call):
 *     cooc[f * nFiles + g] = #{ q : member[q][f] and member[q][g] }       int64, nFiles x nFiles, row-major
 *     *nhit                = the regions with any file (may be NULL)
 * The matrix is symmetric and its diagonal is the support of the region list (igd_hip_support_sets with one set).  Two
 * identical regions count twice.  Both outputs are DEFINED by the call, never added to; nq == 0 gives a zero matrix.  The
 * Jaccard index cooc[f][g] / (cooc[f][f] + cooc[g][g] - cooc[f][g]) is the caller's (igd_amd.jaccard).
 * The regions go through in the chunks of igd_hip_membership; per chunk igd_hip_membership_dev, kernel igd_bits_transpose (the
 * bit rows into bit columns) and kernel igd_bitrows_gram (popcounts of column pairs, symmetric form) adding into a resident
 * matrix: the rows never leave the device, the matrix is copied out once.  Blocking, one device.  IGD_HIP_ERR_ARG, before
 * anything of the caller's is written: a missing array, no such rule, more than IGD_COOCCUR_MAX_FILES files (the matrix
 * would be 2 GiB).  Not done: several sets in one call, weighted counts, several devices. */
#define IGD_COOCCUR_MAX_FILES 16384
int igd_hip_cooccur(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t v, int rule,
                    int64_t *cooc, int64_t *nhit);
/* The two kernels on host arrays (db names the device and owns the workspaces; its records are not read).
 * igd_hip_bits_transpose: bits is nrows rows of nW uint32 words (the layout of igd_hip_membership); cols receives 32 * nW
 * columns of ceil(nrows / 64) uint64 words, column c at cols + c * ceil(nrows / 64): row r is bit r & 63 of word r >> 6 of
 * column c = 32 * w + (the bit's position in word w).  Every word of cols is DEFINED; bits at positions >= nrows are 0.
 * igd_hip_bitrows_gram: out[i * n + j] = popcount(a_i AND b_j) over rows of nwords32 uint32 words, a = m rows, b = n rows;
 * b == NULL selects the symmetric form (b = a, n = m: only the tiles on and above the diagonal are computed and mirrored).
 * out[m * n] is DEFINED.  The rows are those of igd_hip_restrict_sets' bits: igd_hip_bitrows_gram(bits, nsets, NULL, ..) is the
 * set x set overlap matrix |R_j n R_k|.  IGD_HIP_ERR_ARG for a missing array, a negative size or more than 2^28 cells. */
int igd_hip_bits_transpose(igd_hip_db *db, const uint32_t *bits, int64_t nrows, int64_t nW, uint64_t *cols);
int igd_hip_bitrows_gram(igd_hip_db *db, const uint32_t *a, int64_t m, const uint32_t *b, int64_t n, int64_t nwords32, int64_t *out);
/* The decomposition of igd_bitrows_gram (tests): the edge of an output tile (one workgroup), the 64-bit words of a row that
 * one K-step stages, and the slices the word range of a launch is cut into for a = m rows, b = n rows (n == 0: the symmetric
 * form) of nwords32 uint32 words -- every slice is a multiple of the K-step long and adds into out with atomics. */
int32_t igd_hip_gram_tile(void);
int32_t igd_hip_gram_kstep(void);
int64_t igd_hip_gram_slices(int64_t m, int64_t n, int64_t nwords32);

/* Permutation null for region-set support: the set is moved around the genome nperm times, every permuted set is counted as
 * igd_hip_support_sets counts a set, and per file the observed support is placed among the permuted ones.  No universe.
 *
 * THE GENERATOR (the one definition: kernel igd_permute_regions, igdc_permute_regions_host and the tests' numpy reference
 * agree bit for bit).  All arithmetic is unsigned 64-bit modulo 2^64.
 *     G        = 0x9E3779B97F4A7C15
 *     mix64(z) : z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31
 *     r(p, k)  = mix64( mix64( mix64(seed + G) + (p + 1) * G ) + (k + 1) * G )        p = permutation number, k = key
 * A region (c, s, e) with 0 <= c < nctg, len = e - s, L = ctg_len[c]; valid input has 0 <= s <= e <= L and L >= 1.
 *     IGD_HIP_PERM_CIRCULAR  a rigid shift, one offset per permutation and contig: k = c;  s' = (s + r(p, c) mod L) mod L in 64
 *                            bits;  len == L: s' = 0;  otherwise s' + len > L: s' = L - len -- a region that would cross the
 *                            contig's end is pushed back against it: its width is kept, it is never split;  e' = s' + len.
 *     IGD_HIP_PERM_SHUFFLE   independent placement on the same contig: k = i, the region's position in the call's arrays;
 *                            s' = r(p, i) mod (L - len + 1);  e' = s' + len.
 * A region with c < 0 or c >= nctg overlaps nothing: it passes through unchanged and is not validated.  (So does, in the
 * kernels' generic entry alone, an invalid region on a known contig; igd_hip_permute_support refuses those.)  `mod` is biased
 * towards small offsets by at most 2^-32 (L < 2^31 against a 64-bit draw); nothing is done about it. */
#define IGD_HIP_PERM_CIRCULAR 0
#define IGD_HIP_PERM_SHUFFLE  1
#define IGD_HIP_PERM_MAX ((int64_t)1 << 20)          /* permutations of one call */
#if defined(__HIPCC__)
#define IGD_HIP_HD_ __host__ __device__
#else
#define IGD_HIP_HD_
#endif
static inline IGD_HIP_HD_ uint64_t igd_hip_perm_mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
/* mix64(mix64(seed + G) + (p + 1) * G): what r(p, k) shares between the keys of permutation p */
static inline IGD_HIP_HD_ uint64_t igd_hip_perm_base(uint64_t seed, uint64_t p)
{
    const uint64_t a = igd_hip_perm_mix64(seed + 0x9E3779B97F4A7C15ull);
    const uint64_t b = igd_hip_perm_mix64(a + (p + 1) * 0x9E3779B97F4A7C15ull);
    return b;
}
/* region i = (c, *s, *e) under permutation p (base = igd_hip_perm_base(seed, p)), in place */
static inline IGD_HIP_HD_ void igd_hip_perm_place(int mode, uint64_t base, int32_t c, int64_t i, const int32_t *ctg_len, int32_t nctg,
                                                  int32_t *s, int32_t *e)
{
    if (c < 0 || c >= nctg) return;
    const int64_t L = ctg_len[c], s0 = *s, len = (int64_t)*e - s0;
    if (L < 1 || s0 < 0 || len < 0 || s0 + len > L) return;
    const uint64_t k = mode == IGD_HIP_PERM_SHUFFLE ? (uint64_t)i : (uint64_t)c;
    const uint64_t r = igd_hip_perm_mix64(base + (k + 1) * 0x9E3779B97F4A7C15ull);
    int64_t t;
    if (mode == IGD_HIP_PERM_SHUFFLE) t = (int64_t)(r % (uint64_t)(L - len + 1));
    else {
        t = (int64_t)(((uint64_t)s0 + r % (uint64_t)L) % (uint64_t)L);
        if (len == L) t = 0;
        else if (t + len > L) t = L - len;
    }
    *s = (int32_t)t;
    *e = (int32_t)(t + len);
}
/* THE DRAW (the one definition: kernel igd_resample_regions, igdc_resample_regions_host and the tests' numpy reference agree bit
 * for bit).  A keyed bijection on [0, n), 1 <= n < 2^31: a four-round Feistel network on the smallest domain 2^(2h) >= n, walked
 * until it is back below n (cycle walking).  Unsigned 64-bit arithmetic, G, mix64 and igd_hip_perm_base as above.
 *     h      = the smallest integer >= 1 with 4^h >= n            (h <= 16; the domain 2^(2h) is below 4 n for n >= 2)
 *     mask   = 2^h - 1
 *     base   = igd_hip_perm_base(seed, p)
 *     F(j,R) = mix64(base + (((j + 1) << 32) + R + 1) * G) & mask                 j = 0 .. 3
 *     step(x): L = x >> h, R = x & mask;  four times, j = 0 .. 3: (L, R) <- (R, L ^ F(j, R));  return (L << h) | R
 *     igd_hip_resample_index(base, i, n):  y = step(i);  while (y >= n) y = step(y);  return y      -- needs i < n
 * IGD_HIP_PERM_RESAMPLE: draw i of permutation p is region igd_hip_resample_index(base(seed, p), i, npool) of a pool of npool
 * regions, i = 0 .. nq - 1, copied as it stands -- contig, start and end; nq regions drawn WITHOUT replacement
 * (regioneR::resampleRegions).  step is a bijection of the domain and i < n, so the walk returns to [0, n) and ends; it need not
 * end for a start i >= n, so every entry refuses nq > npool before anything is launched.  A four-round network is not a uniform
 * random permutation, least of all on tiny domains (n <= 4 has 2^(2h) = 4 points and at most 4^4 round-function tables); nothing
 * is done about it. */
#define IGD_HIP_PERM_RESAMPLE 4                      /* (3 is the engine's internal shift placement) */
static inline IGD_HIP_HD_ int igd_hip_resample_bits(uint64_t n)
{
    int h = 1;
    while (((uint64_t)1 << (2 * h)) < n) h++;
    return h;
}
static inline IGD_HIP_HD_ uint64_t igd_hip_resample_step(uint64_t base, uint64_t x, int h)
{
    const uint64_t mask = ((uint64_t)1 << h) - 1;
    uint64_t L = x >> h, R = x & mask;
    for (uint64_t j = 0; j < 4; j++) {
        const uint64_t f = igd_hip_perm_mix64(base + (((j + 1) << 32) + R + 1) * 0x9E3779B97F4A7C15ull) & mask;
        const uint64_t t = L ^ f;
        L = R;
        R = t;
    }
    return (L << h) | R;
}
/* h = igd_hip_resample_bits(n), taken once by a caller with many draws from one pool */
static inline IGD_HIP_HD_ uint64_t igd_hip_resample_walk(uint64_t base, uint64_t i, uint64_t n, int h)
{
    uint64_t y = igd_hip_resample_step(base, i, h);
    while (y >= n) y = igd_hip_resample_step(base, y, h);
    return y;
}
static inline IGD_HIP_HD_ uint64_t igd_hip_resample_index(uint64_t base, uint64_t i, uint64_t n)
{
    const int h = igd_hip_resample_bits(n);
    const uint64_t y = igd_hip_resample_walk(base, i, n, h);
    return y;
}
/* THE WORKSPACE (the one definition: kernel igd_permute_workspace, igdc_permute_regions_host_ws and the tests' numpy reference
 * agree bit for bit).  A workspace is a list of segments (c, a, b) on the contigs of the call: the stretches a region may be
 * placed in (GAT's workspace, regioneR's mask inverted, `bedtools shuffle -incl`).  It is merged at gap 0 by the rules of
 * igd_hip_merge_sets (igd_hip_merge_takes_part, igd_hip_merge_opens: touching segments join, zero-length and inverted ones
 * and those on unknown contigs are dropped) and then clipped to [0, ctg_len[c]]; what is left of a segment has length >= 1.
 * Per contig the merged segments are ordered by length descending, then start ascending.  THE TABLE of nseg segments:
 *     w_off[nctg + 1]        int64: the segments of contig c are w_off[c] .. w_off[c + 1] - 1; w_off[0] = 0, w_off[nctg] = nseg
 *     w_start[nseg], w_len[nseg]   int32, in that order
 *     w_pre[nseg + nctg]     int32, n + 1 entries per contig: w_pre[w_off[c] + c + j] = the sum of the first j lengths of contig
 *                            c, 0 <= j <= n = w_off[c + 1] - w_off[c].  Disjoint segments of one contig sum to at most
 *                            ctg_len[c] <= 2^31 - 1.
 * IGD_HIP_PERM_WORKSPACE places region i = (c, s, e), len = e - s, valid as above, with k = i and r = r(p, i) as SHUFFLE:
 *     kk   = the number of segments of contig c with w_len >= len (binary search in the descending lengths)
 *     F(j) = w_pre[w_off[c] + c + j] - j * (len - 1) in signed 64 bits, 0 <= j <= kk: the valid starts in the first j segments
 *            (each gives w_len - len + 1 >= 1, so F is strictly increasing);  T = F(kk)
 *     T == 0: the region fits nowhere and passes through unchanged (the three drivers refuse such a call)
 *     u = r mod T;  j = the one index with F(j) <= u < F(j + 1) (a second binary search);
 *     s' = w_start[w_off[c] + j] + (u - F(j));  e' = s' + len.
 * Every fitting start is equally likely up to the bias of `mod`, at most 2^-31 (T <= 2^32).  Regions on unknown contigs and
 * invalid regions pass through as under the other modes.  Two identities: a workspace of the one segment [0, L) per contig
 * gives SHUFFLE's output bit for bit, and every placed region lies inside one segment.
 * igd_hip_workspace_valid: 1 when a table can be trusted -- nctg as given, offsets from 0 to nseg and monotone, per contig
 * fewer than 2^31 segments, every length >= 1 and not above the one before it, 0 <= start and start + len <= ctg_len[c], w_pre
 * the sums just defined and never above ctg_len[c].  O(nseg).  With such a table igd_hip_perm_place_ws reads inside the four
 * arrays and returns a region on its contig whatever else the table holds; both searches take at most 32 steps. */
#define IGD_HIP_PERM_WORKSPACE 2
typedef struct igd_hip_workspace {
    int32_t nctg;
    int64_t nseg;
    const int64_t *w_off;
    const int32_t *w_start, *w_len, *w_pre;
} igd_hip_workspace;
static inline int igd_hip_workspace_valid(const igd_hip_workspace *ws, const int32_t *ctg_len, int32_t nctg)
{
    if (!ws || ws->nctg != nctg || nctg < 0 || ws->nseg < 0 || !ws->w_off || (nctg > 0 && (!ctg_len || !ws->w_pre)) ||
        (ws->nseg > 0 && (!ws->w_start || !ws->w_len)) || ws->w_off[0] != 0 || ws->w_off[nctg] != ws->nseg)
        return 0;
    for (int32_t c = 0; c < nctg; c++) {
        const int64_t o = ws->w_off[c], n = ws->w_off[c + 1] - o, L = ctg_len[c];
        if (n < 0 || n > (int64_t)INT32_MAX || o + n > ws->nseg) return 0;
        const int32_t *pre = ws->w_pre + o + c;
        int64_t sum = 0;
        if (pre[0] != 0) return 0;
        for (int64_t j = 0; j < n; j++) {
            const int64_t a = ws->w_start[o + j], l = ws->w_len[o + j];
            if (l < 1 || (j > 0 && l > (int64_t)ws->w_len[o + j - 1]) || a < 0 || a + l > L) return 0;
            sum += l;
            if (sum > L || (int64_t)pre[j + 1] != sum) return 0;
        }
    }
    return 1;
}
/* a mode the call can run (the engine and the host route ask here): the two free placements without a workspace,
 * IGD_HIP_PERM_WORKSPACE with one, IGD_HIP_PERM_RESAMPLE exactly when a pool is given and never with a workspace */
static inline int igd_hip_perm_mode_ok(int mode, int has_ws, int has_pool)
{
    if (has_pool || mode == IGD_HIP_PERM_RESAMPLE) return has_pool && !has_ws && mode == IGD_HIP_PERM_RESAMPLE;
    return has_ws ? mode == IGD_HIP_PERM_WORKSPACE : (mode == IGD_HIP_PERM_CIRCULAR || mode == IGD_HIP_PERM_SHUFFLE);
}
/* region i = (c, *s, *e) under permutation p (base = igd_hip_perm_base(seed, p)) inside the workspace, in place; 1 when the
 * region is on a known contig, valid, and fits in no segment (it is left as it was), 0 otherwise */
static inline IGD_HIP_HD_ int igd_hip_perm_place_ws(uint64_t base, int32_t c, int64_t i, const int32_t *ctg_len, int32_t nctg,
                                                    const int64_t *w_off, const int32_t *w_start, const int32_t *w_len, const int32_t *w_pre,
                                                    int32_t *s, int32_t *e)
{
    if (c < 0 || c >= nctg) return 0;
    const int64_t L = ctg_len[c], s0 = *s, len = (int64_t)*e - s0;
    if (L < 1 || s0 < 0 || len < 0 || s0 + len > L) return 0;
    const int64_t o = w_off[c], n = w_off[c + 1] - o;
    const int32_t *pre = w_pre + o + c;
    int64_t lo = 0, hi = n;                               /* kk: the first j with w_len[j] < len */
    for (int step = 0; step < 32 && lo < hi; step++) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)w_len[o + mid] >= len) lo = mid + 1; else hi = mid;
    }
    const int64_t kk = lo, T = (int64_t)pre[kk] - kk * (len - 1);
    if (T <= 0) return 1;
    const uint64_t r = igd_hip_perm_mix64(base + ((uint64_t)i + 1) * 0x9E3779B97F4A7C15ull);
    const int64_t u = (int64_t)(r % (uint64_t)T);
    lo = 0; hi = kk;                                      /* F(lo) <= u < F(hi) */
    for (int step = 0; step < 32 && hi - lo > 1; step++) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)pre[mid] - mid * (len - 1) <= u) lo = mid; else hi = mid;
    }
    const int64_t t = (int64_t)w_start[o + lo] + (u - ((int64_t)pre[lo] - lo * (len - 1)));
    *s = (int32_t)t;
    *e = (int32_t)(t + len);
    return 0;
}
/* The two questions every driver asks of a call's regions before it runs, the engine's and the host route's alike (host only).
 * igd_hip_perm_first_bad: the first region on a known contig that breaks L >= 1, 0 <= s <= e <= L; -1: none.
 * igd_hip_perm_first_unplaceable: the first such valid region that fits in no segment of its contig (T == 0 above) in a table
 * igd_hip_workspace_valid has passed for these contigs; -1: none. */
static inline int64_t igd_hip_perm_first_bad(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                                             int32_t nctg)
{
    for (int64_t i = 0; i < nq; i++) {
        const int32_t c = ichr[i];
        if (c < 0 || c >= nctg) continue;
        if (ctg_len[c] < 1 || qs[i] < 0 || qe[i] < qs[i] || qe[i] > ctg_len[c]) return i;
    }
    return -1;
}
static inline int64_t igd_hip_perm_first_unplaceable(const igd_hip_workspace *ws, const int32_t *ctg_len, const int32_t *ichr,
                                                     const int32_t *qs, const int32_t *qe, int64_t nq)
{
    for (int64_t i = 0; i < nq; i++) {
        int32_t s = qs[i], e = qe[i];
        if (igd_hip_perm_place_ws(0, ichr[i], i, ctg_len, ws->nctg, ws->w_off, ws->w_start, ws->w_len, ws->w_pre, &s, &e)) return i;
    }
    return -1;
}
/* The whole test on one device.  ctg_len is int32[number of contigs of db], in the database's contig order.  Index nFiles of
 * every output is the "any dataset" column: the regions with a hit in any file, what igd_hip_support_sets adds to nhit.
 *     observed[f] = support of the set as given                          sum[f], sumsq[f] = over the permutations, of x and x^2
 *     n_ge[f], n_le[f] = permutations with x >= observed[f], x <= observed[f]      pmin[f], pmax[f] = smallest, largest x
 * with x = the support of file f in one permuted set.  Each array is int64[nFiles + 1]; all but observed may be NULL; all are
 * DEFINED by the call.  The regions are uploaded once; the permutations go through in chunks of pc permutations with
 * pc * nq <= igd_hip_max_batch() and pc * nFiles * 8 <= the row budget of igd_hip_support_sets (TEST-ONLY: IGD_HIP_PERM_ROW_BYTES
 * lowers it): kernel igd_permute_regions into the staging arrays, one row per permutation through igd_sets_support (both
 * forms), kernel igd_perm_stats over the chunk's rows and totals into resident statistics.  The permuted regions and the
 * rows never leave the device.  Blocking.  IGD_HIP_ERR_ARG, before any launch and with nothing of the caller's written: a
 * missing array, no such rule or mode, nperm < 1 or > IGD_HIP_PERM_MAX, nq > igd_hip_max_batch(), nperm * nq^2 >= 2^63 (sumsq),
 * a region on a known contig that breaks 0 <= s <= e <= L, L >= 1 (igd_hip_last_error names the first one).
 * Not done: several sets in one call, regions split at the contig's end, several devices. */
int igd_hip_permute_support(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                            int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq,
                            int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax);
/* The same under a minimum overlap (igd_hip_min_overlap above): the observed row and every permuted row are counted under it. */
int igd_hip_permute_support_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                               int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq,
                               int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax, const igd_hip_min_overlap *min_overlap);
/* The two kernels on host arrays (db names the device and owns the workspaces; its records are not read).
 * igd_hip_permute_regions: permutations [p0, p0 + np) of nq regions into out_qs, out_qe (int32[np * nq], permutation-major);
 * nctg is the caller's, not tied to the database.  IGD_HIP_ERR_ARG for a missing array, no such mode, a negative size,
 * nq > igd_hip_max_batch() or more than 2^31 - 1 outputs.
 * igd_hip_perm_stats: rows is int64[nrows * ncols]; sum .. pmax (int64[ncols], each may be NULL) are DEFINED as above with
 * x = rows[r][col]; sums wrap modulo 2^64.  The rows go through in chunks of the same row budget, the statistics stay
 * resident between them.  IGD_HIP_ERR_ARG for a missing array or nrows < 1 or ncols < 1.
 * igd_hip_permute_grid: workgroups igd_permute_regions is launched with for n outputs (tests: a lane takes a second output
 * only when n exceeds the grid's lanes). */
int igd_hip_permute_regions(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                            int32_t nctg, int mode, uint64_t seed, int64_t p0, int64_t np, int32_t *out_qs, int32_t *out_qe);
int igd_hip_perm_stats(igd_hip_db *db, const int64_t *rows, int64_t nrows, int64_t ncols, const int64_t *observed, int64_t *sum,
                       int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax);
int32_t igd_hip_permute_grid(int64_t n);
/* The four entries above inside a workspace (THE WORKSPACE above; kernel igd_permute_workspace, the launch shape of
 * igd_permute_regions with the table read from device memory).  ws == NULL is the entry above, every refusal included: mode
 * IGD_HIP_PERM_WORKSPACE without a workspace stays IGD_HIP_ERR_ARG.  With a workspace the mode must be IGD_HIP_PERM_WORKSPACE;
 * the table is checked by igd_hip_workspace_valid against the call's ctg_len (the database's contigs for the three drivers)
 * and uploaded once per call into a buffer of the handle; everything behind the placement is the entry's own chain, unchanged.
 * IGD_HIP_ERR_ARG before any launch, nothing of the caller's written: an invalid table, a mode / workspace mismatch and, in the
 * three drivers, a valid region on a known contig that fits in no segment (igd_hip_last_error names the first one; the generic
 * entry passes it through unchanged).
 * Not done: a circular shift inside a workspace, segments weighted other than by length (isochores), truncating datasets to
 * the workspace, several sets in one call, several devices. */
int igd_hip_permute_regions_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                               int32_t nctg, int mode, uint64_t seed, int64_t p0, int64_t np, int32_t *out_qs, int32_t *out_qe,
                               const igd_hip_workspace *ws);
int igd_hip_permute_support_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                               int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq,
                               int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax, const igd_hip_min_overlap *min_overlap,
                               const igd_hip_workspace *ws);
int igd_hip_permute_nearest_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                               int mode, uint64_t seed, int64_t nperm, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap,
                               int64_t *sum_dist, const igd_hip_workspace *ws);
int igd_hip_permute_bp_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                          int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged,
                          int64_t *n_dropped, const igd_hip_workspace *ws);
/* The three nulls by RESAMPLING from a universe (THE DRAW above; kernel igd_resample_regions, the launch shape of
 * igd_permute_regions with three gathered loads per output).  Row 0 is the call's own nq regions, the set as given, which need
 * not come from the pool; row p + 1 is the nq pool regions of draw p, contigs included.  Nothing is placed, so there is no
 * ctg_len and no region is validated: a region on an unknown contig overlaps nothing, as everywhere.  The pool (pool_ichr,
 * pool_qs, pool_qe: int32[npool]) is uploaded once behind the call's regions; everything behind the generator is the entry's own
 * chain, unchanged, with the chunk rule unchanged.  For the support each permuted value is hypergeometric: the null Fisher's test
 * gives in closed form.  igd_hip_permute_bp_rs: n_dropped is that of the set as given; the draws' differ and are not reported.
 * IGD_HIP_ERR_ARG before any launch, nothing of the caller's written, in this order: the entry's own first check (min_overlap, the
 * window); a missing argument or no such rule; nperm outside 1 .. IGD_HIP_PERM_MAX; nq or npool above igd_hip_max_batch();
 * npool < nq (igd_hip_last_error names both); the support's nperm * nq^2 >= 2^63.  nq == 0 or nFiles == 0: the all-zero results
 * of the entries above, no device work.
 * igd_hip_resample_regions: the generator alone, the twin of igd_hip_permute_regions -- draws [p0, p0 + np) of nq regions into
 * out_ichr, out_qs, out_qe (int32[np * nq], draw-major); IGD_HIP_ERR_ARG for a missing array, a negative size, nq or npool above
 * igd_hip_max_batch(), npool < nq or more than 2^31 - 1 outputs.
 * Not done: strata of the pool (width- or GC-matched resampling), resampling for the shift profile, groups or set lists, several
 * devices. */
int igd_hip_resample_regions(igd_hip_db *db, const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool,
                             int64_t nq, uint64_t seed, int64_t p0, int64_t np, int32_t *out_ichr, int32_t *out_qs, int32_t *out_qe);
int igd_hip_permute_support_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                               int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq, int64_t *n_ge,
                               int64_t *n_le, int64_t *pmin, int64_t *pmax, const igd_hip_min_overlap *min_overlap);
int igd_hip_permute_nearest_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                               int64_t nperm, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist);
int igd_hip_permute_bp_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                          const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                          int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged, int64_t *n_dropped);

/* The set statistics of the overlapping records' values without the count and agg rows, and their permutation null: "are the
 * scores of dataset f's records under my regions higher or lower than under the same regions placed at random" (regioneR's
 * permTest with meanInRegions).  Kernel igd_map_slices: the walk and tables of igd_map_rows, folded per region into LDS
 * accumulators of the slice; nothing per region reaches memory.  THE STATISTICS are igd_hip_map_sets' (counted, op, n_hit, pairs,
 * agg_sum above), every integer the same.
 * igd_hip_map_sets_fused: the contract, checks and outputs of igd_hip_map_sets.  Groups of whole sets within the row budget of
 * igd_hip_support_sets, regions in chunks of igd_hip_max_batch(), no row workspace, one launch per chunk.
 * igd_hip_permute_map (_ws: inside a workspace; _rs: resampled from a universe -- the placements of the three nulls above, with
 * their arguments): each output is int64[nperm + 1][nFiles] (any may be NULL): row 0 the statistics of the set as given, row
 * p + 1 those of permutation p of THE GENERATOR (resp. THE DRAW).  The null distribution itself comes back, as
 * igd_hip_permute_nearest returns it: the statistics of interest are ratios of two columns that both vary per permutation --
 *     mean_region = agg_sum / n_hit   (COUNT, SUM, MIN, MAX: the mean over the regions with a record of the region's aggregate)
 *     mean_pair   = agg_sum / pairs   (SUM: the mean value of a counted record, meanInRegions over pairs)
 * -- undefined where the denominator is 0 (igdc_perm_map_summary, igd_core.h).  Chunks of pc permutations, pc * nq <=
 * igd_hip_max_batch() and 3 * pc * nFiles * 8 <= the row budget of igd_hip_permute_support (TEST-ONLY: IGD_HIP_PERM_ROW_BYTES);
 * the slice table is built and uploaded once; per chunk the generator, a memset of the three matrices, igd_map_slices and an
 * asynchronous copy of the chunk's rows, enqueued without a wait.
 * IGD_HIP_ERR_ARG before any launch, nothing of the caller's written, in this order: an unknown op or a value op on a gType 0
 * database (igd_hip_map's refusal); then the refusals of igd_hip_permute_nearest behind its window (resp. of the _ws and _rs
 * entries).  nq == 0 or nFiles == 0: all zeros.  Blocking, one device.
 * Databases with more than igd_hip_map_fused_max_files(op) files (163 840 B of LDS, the whole of a CU, over 28 (COUNT), 52 (MIN,
 * MAX) or 68 (SUM) bytes per file: 5 851, 3 150, 2 409; 0 for an unknown op) take igd_map_rows + igd_map_reduce instead, in
 * pieces within the row budget of igd_hip_map (there is no wide form of the fused kernel); the results are the same.
 * igd_hip_map_fused_grid: workgroups the fused kernel is launched with for nslices slices (tests: a workgroup takes a second
 * slice only past this number).
 * Not done: several sets or a set list under the permutation, a minimum overlap, a per-permutation median, several devices. */
int igd_hip_map_sets_fused(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                           int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum);
int igd_hip_permute_map(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                        int mode, uint64_t seed, int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum);
int igd_hip_permute_map_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                           int mode, uint64_t seed, int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum,
                           const igd_hip_workspace *ws);
int igd_hip_permute_map_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                           const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                           int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum);
int32_t igd_hip_map_fused_max_files(int op);
int32_t igd_hip_map_fused_grid(int64_t nslices);

/* Local z-score: the support of a region set under rigid shifts (regioneR's localZScore).  The whole set is moved by each of
 * nshift offsets and counted again; the host places every count in the null the permutation entries above produced.
 * THE SHIFT (the one definition: kernel igd_shift_regions, igdc_shift_regions_host and the tests' numpy reference agree on
 * every integer).  A region (c, s, e) on a known contig, L = ctg_len[c] >= 1, 0 <= s <= e <= L, len = e - s, under offset d:
 *     s' = min(max(s + d, 0), L - len) in signed 64 bits;  e' = s' + len
 * -- a region that would leave its contig is pushed back against the end, its width kept: IGD_HIP_PERM_CIRCULAR's rule at the
 * contig's end.  A region with c < 0 or c >= nctg passes through unchanged, and so does, in the generic entry alone, an invalid
 * region on a known contig.  Offsets are int32 with |d| <= IGD_HIP_SHIFT_MAX_OFFSET (the bound of -N's window), 1 ..
 * IGD_HIP_SHIFT_MAX of them per call, in any order, repeats allowed. */
#define IGD_HIP_SHIFT_MAX 4096
#define IGD_HIP_SHIFT_MAX_OFFSET ((int32_t)1 << 30)
/* region (c, *s, *e) under offset d, in place */
static inline IGD_HIP_HD_ void igd_hip_shift_place(int32_t d, int32_t c, const int32_t *ctg_len, int32_t nctg, int32_t *s, int32_t *e)
{
    if (c < 0 || c >= nctg) return;
    const int64_t L = ctg_len[c], s0 = *s, len = (int64_t)*e - s0;
    if (L < 1 || s0 < 0 || len < 0 || s0 + len > L) return;
    int64_t t = s0 + (int64_t)d;
    if (t < 0) t = 0;
    if (t > L - len) t = L - len;
    *s = (int32_t)t;
    *e = (int32_t)(t + len);
}
/* the first offset beyond +-IGD_HIP_SHIFT_MAX_OFFSET; -1: none (host only) */
static inline int64_t igd_hip_shift_first_bad(const int32_t *offsets, int64_t nshift)
{
    for (int64_t j = 0; j < nshift; j++)
        if (offsets[j] > IGD_HIP_SHIFT_MAX_OFFSET || offsets[j] < -IGD_HIP_SHIFT_MAX_OFFSET) return j;
    return -1;
}
/* igd_hip_shift_support: shifted is int64[nshift][nFiles + 1], DEFINED by the call.  Row j is exactly what igd_hip_support_sets_ov
 * counts for the set shifted by offsets[j] (same v, rule and min_overlap; NULL: no threshold); column nFiles is the regions with a
 * hit in any dataset, as in igd_hip_permute_support.  A row with offset 0 equals the support of the set as given; equal offsets
 * give equal rows.  ctg_len is int32[number of contigs of db].  The regions and the offsets are uploaded once; the shifts go
 * through the chunk driver of the permutation nulls, pc shifts per chunk with pc * nq <= igd_hip_max_batch() and pc * nFiles * 8
 * <= the row budget of igd_hip_permute_support: kernel igd_shift_regions into the staging arrays, one row per shift through
 * igd_sets_support, the rows copied into a buffer of the call; one wait at the end.  z-scores are the host's (igd_amd.local_zscore,
 * `igd search -Z`): no floating point runs on the device.  IGD_HIP_ERR_ARG before any launch, nothing of the caller's written,
 * checked in this order: min_overlap out of range; a missing argument or no such rule; nshift outside 1 .. IGD_HIP_SHIFT_MAX; an
 * offset beyond +-2^30 (igd_hip_last_error names the first); nq > igd_hip_max_batch(); the first region on a known contig that
 * breaks 0 <= s <= e <= L, L >= 1.  nq == 0 or nFiles == 0: all zeros, no device work.
 * igd_hip_shift_regions: the kernel on host arrays, the twin of igd_hip_permute_regions -- out_qs, out_qe are int32[nshift * nq],
 * shift-major; nctg is the caller's; chunked by igd_hip_max_batch(); the same refusals but the last (regions are not validated),
 * and more than 2^31 - 1 outputs.
 * Not done: the shift profile of the nearest distances and of the base pairs, several sets in one call, several devices. */
int igd_hip_shift_regions(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                          int32_t nctg, const int32_t *offsets, int64_t nshift, int32_t *out_qs, int32_t *out_qe);
int igd_hip_shift_support(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                          const int32_t *offsets, int64_t nshift, int32_t v, int rule, int64_t *shifted,
                          const igd_hip_min_overlap *min_overlap);

/* Device-resident search: all pointers are device pointers on db's GPU; d_hits
 * (int64[nFiles]) is ADDED to; d_total (int64[1], may be NULL) is ADDED to.  Enqueues on
 * `stream` (a hipStream_t; NULL = the engine's own stream) and returns without waiting.
 * nq must be <= igd_hip_max_batch().  One call at a time per database (shared workspace). */
int igd_hip_search_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs,
                       const int32_t *d_qe, int64_t nq, int32_t v, int rule, int flags,
                       int64_t *d_hits, int64_t *d_total, void *stream);
/* The same for a position-sorted batch given as contig RUNS instead of one contig number per query: d_run_start (device,
 * nCtg + 1 int32) with run_start[0] = 0, run_start[nCtg] = nq and the queries [run_start[c], run_start[c + 1]) lying on contig c
 * in non-decreasing order of start -- what a position-sorted BED is (the command line tool's reader keeps its queries that
 * way, igdc_queries_group_contigs).  The grouping kernel then reads 8 instead of 12 bytes per query.  Implies
 * IGD_HIP_FLAG_SORTED (IGD_HIP_FLAG_BUCKET is refused); a table that is not monotone or does not cover [0, nq), like queries out
 * of order, is a broken promise: the batch adds nothing and igd_hip_sync returns IGD_HIP_ERR_UNSORTED. */
int igd_hip_search_runs_dev(igd_hip_db *db, const int32_t *d_run_start, const int32_t *d_qs, const int32_t *d_qe,
                            int64_t nq, int32_t v, int rule, int flags, int64_t *d_hits, int64_t *d_total, void *stream);
int64_t igd_hip_max_batch(void);   /* queries per call of the host-buffer entry points (2^24; test-only IGD_HIP_MAX_BATCH lowers it) */
/* The rule behind igd_hip_max_batch(), in ONE place: the engine (igd_hip.hip) and the host flavours' lazy binding
 * (igd_hip_lazy.c, which answers without mapping the engine) both evaluate this -- they cannot drift apart. */
#define IGD_HIP_MAX_BATCH_DEFAULT ((int64_t)1 << 24)
static inline int64_t igd_hip_max_batch_rule(const char *env /* getenv("IGD_HIP_MAX_BATCH") or NULL */)
{
    long long x = 0;
    if (env && *env) { int neg = 0; const char *p = env; if (*p == '-') { neg = 1; p++; } while (*p >= '0' && *p <= '9' && x < ((long long)1 << 40)) x = x * 10 + (*p++ - '0'); if (neg) x = -x; }
    return x >= 1 && x < IGD_HIP_MAX_BATCH_DEFAULT ? (int64_t)x : IGD_HIP_MAX_BATCH_DEFAULT;
}
int  igd_hip_sync(igd_hip_db *db, void *stream);      /* wait + surface async errors         */
int  igd_hip_sync_spin(igd_hip_db *db, void *stream); /* the same, polling hipStreamQuery instead of sleeping on the signal */

/* Several devices driven by one process (the C host's form): the database resident on each device of the
 * group (igd_hip_open once per device; a device may be listed twice), a query set cut into contiguous slabs, one per device,
 * and the path's ONE exchange -- the sum of the per-device hits[nFiles] vectors, the reference's single accumulator
 * (src/igd_search.c:925,1032-1039) -- as an RCCL all-reduce (ncclInt64, ncclSum) on the engines' own streams, over xGMI.
 * librccl is mapped when the first group is created.  When it cannot be used (not loadable, communicator refused, a device
 * listed twice, IGD_MULTI_REDUCE=host) the vectors are added on the host; igd_hip_group_reduce_kind() returns "rccl" or
 * "host", igd_hip_group_reduce_note() the reason for "host"; IGD_MULTI_REDUCE=rccl makes create fail instead of falling back.
 * igd_hip_group_search: hits[] is ADDED to, *total = overlaps of the whole set.  Blocking.  The group does not own the
 * databases (destroy the group first, then close them). */
typedef struct igd_hip_group igd_hip_group;
int  igd_hip_group_create(igd_hip_db *const *dbs, int n, igd_hip_group **out);
void igd_hip_group_destroy(igd_hip_group *g);
const char *igd_hip_group_reduce_kind(const igd_hip_group *g);
const char *igd_hip_group_reduce_note(const igd_hip_group *g);
int  igd_hip_group_search(igd_hip_group *g, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                          int32_t v, int rule, int flags, int64_t *hits, int64_t *total);

/* `-f`: full enumeration in reference order (queries in batch order; per query tiles
 * ascending, record index DESCENDING inside a tile; rule NEST, no value filter).
 * qoff[0..nq] receives the exclusive scan of per-query counts; *out is malloc'd by the
 * callee (free with igd_hip_free) and holds qoff[nq] records.  Blocking. */
int  igd_hip_enumerate(igd_hip_db *db, const int32_t *ichr, const int32_t *qs,
                       const int32_t *qe, int64_t nq, int64_t *qoff, igd_hip_hit **out,
                       int64_t *total);
void igd_hip_free(void *p);

/* The same enumeration, STREAMED: the overlaps are produced in chunks of contiguous query ranges
 * (<= 32 MiB of records each, a whole query never split) and each chunk is handed to `sink` from
 * pinned host memory while the next chunks are being filled and copied -- the caller (the command
 * line tool's formatter, getOverlaps_f1 src/igd_search.c:721-744) works on chunk k while chunk k+1
 * crosses PCIe.  qoff[0..nq] is complete before the first sink call; a chunk covers queries [q0,q1),
 * `hits` points at overlap number qoff[q0] (so overlap h of the batch is hits[h - qoff[q0]]) and is
 * only valid during the call.  Chunks arrive in order and together cover [0,nq) exactly once, also
 * the queries without overlaps.  A non-zero return of the sink stops the enumeration.  Blocking. */
typedef int (*igd_hip_enum_sink)(void *ctx, int64_t q0, int64_t q1, const int64_t *qoff, const igd_hip_hit *hits);
int  igd_hip_enumerate_stream(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                              int64_t nq, int64_t *qoff, igd_hip_enum_sink sink, void *ctx, int64_t *total);

/* The same stream in HALF the bytes (round 6; `-f` is bound by the bytes that cross PCIe, 0.81 of the link at 16 per overlap):
 * one overlap = 8 bytes.  `q` is implied by qoff[]; start is kept whole; (end - start) and idx share the second word, split
 * per DATABASE: idx takes idx_bits = ceil(log2(nFiles)) low bits, the length the 32 - idx_bits above them (1900 files: 11 + 21
 * bits, lengths up to 2 097 151 bp).  igd_hip_hit8_idx_bits() returns that split, or -1 when a record of this database does not
 * fit it (a length of 2^(32 - idx_bits) or more, or end < start): such a database streams through igd_hip_enumerate_stream only.
 * Expansion: start = (int32_t)h.start, idx = h.lenidx & ((1u << idx_bits) - 1), end = start + (int32_t)(h.lenidx >> idx_bits)
 * (igd_hip_hit8_expand).  Order, chunking, qoff and the sink's contract are those of igd_hip_enumerate_stream. */
typedef struct { uint32_t start, lenidx; } igd_hip_hit8;
typedef int (*igd_hip_enum_sink8)(void *ctx, int64_t q0, int64_t q1, const int64_t *qoff, const igd_hip_hit8 *hits, int idx_bits);
int  igd_hip_hit8_idx_bits(igd_hip_db *db);
int  igd_hip_enumerate_stream8(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                               int64_t nq, int64_t *qoff, igd_hip_enum_sink8 sink, void *ctx, int64_t *total);
static inline igd_hip_hit igd_hip_hit8_expand(igd_hip_hit8 h, int idx_bits, int32_t q)
{
    igd_hip_hit r;
    r.q = q;
    r.start = (int32_t)h.start;
    r.idx = (int32_t)(idx_bits ? (h.lenidx & ((1u << idx_bits) - 1u)) : 0u);
    r.end = (int32_t)(h.start + (idx_bits < 32 ? (h.lenidx >> idx_bits) : 0u));
    return r;
}

/* `-m`: dataset x dataset hit map, getMap src/igd_search.c:772-826 (use_v = 0) and getMap_v
 * :829-886 (use_v = 1: both records need value > v, strictly).  hitmap is nFiles x nFiles uint32,
 * row-major, caller-allocated, ADDED to; *total (may be NULL) receives the number of pairs.
 * gType-1 databases only.  Blocking. */
int igd_hip_hitmap(igd_hip_db *db, int use_v, int32_t v, uint32_t *hitmap, int64_t *total);

/* Seqpare (`search -q f.bed -s`): seqOverlaps src/igd_search.c:354-451 over
 * seq_overlaps :253-352.  Queries as the reference orders them: the contigs of the query file in
 * first-seen order, inside a contig by start (ties in file order); qgroup[i] = number of the query's
 * contig in that order (0..nGroups-1, non-decreasing).  sums[m] (nFiles doubles) receives the sum of
 * the greedily matched similarities of dataset m, added up in the reference's order; the caller
 * finishes with sm = sums/(Nq + nr - sums) (:446-449).  gType-1 databases; one batch; blocking. */
int igd_hip_seqpare(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                    const int32_t *qgroup, int32_t nGroups, double *sums);
/* The same for a query file beyond one batch: the contigs of the file are passed range by range, in
 * order; sums[] is NOT cleared but continued, so the additions happen in the reference's order. */
int igd_hip_seqpare_add(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                        const int32_t *qgroup, int32_t nGroups, double *sums);

/* `igd create`: intervals -> the tile region of an .igd, on the GPU.
 * Replaces igd_add (src/igd_base.c:118-169: replicate into tiles start/nbp..(end-1)/nbp),
 * igd_saveT (:333-364: per-tile append in input order) and igd_save (:396-461: per-tile
 * radix_sort_intv, src/igd_base.h:196-249, then contig-major concatenation).  The records come
 * out in EXACTLY the reference's order, including its (unstable) order of equal starts.
 * Input: n intervals in input order (files in glob order, lines in file order), every one with
 * 0 <= start < end; ctg[] = contig numbers in first-seen order, file[] = index of the source
 * file (gdata_t.idx); value may be NULL (0).  Host arrays; nothing is retained.
 * Output: out_fd < 0 -> the records come back in pinned host memory (igd_hip_created.records);
 * out_fd >= 0 -> the engine writes the complete .igd (header of SURVEY.md App. A with ctgName[],
 * zero-padded to 40 bytes, then the tiles) to that descriptor through two pinned staging buffers,
 * device->host copies overlapping the write()s, and records stays NULL. */
typedef struct {
    int32_t nbp, gType, nCtg;
    int64_t n;
    const int32_t *ctg, *start, *end, *value, *file;
    const char *const *ctgName;   /* [nCtg], needed only with out_fd >= 0                       */
    int out_fd;
} igd_hip_create_desc;
typedef struct {
    int32_t *nTile;           /* [nCtg]   tiles per contig = 1 + max (end-1)/nbp               */
    int32_t *nCnt;            /* [nTiles] records per tile, contig-major (the header table)     */
    int64_t nTiles, nRecords;
    void *records;            /* nRecords x 16 (gType 1) or 12 (gType 0) bytes, file order, pinned */
} igd_hip_created;
int  igd_hip_create(const igd_hip_create_desc *d, int device, igd_hip_created *out);
void igd_hip_created_free(igd_hip_created *c);

/* What the loaded library was compiled as.  igd_hip_build_flags(): bits 0..23 = the IGD_EXP experiment mask of the build
 * (0 in a shipped library), bit 24 = IGD_EXP_NOMATCH.  igd_hip_build_wrong_counts(): the subset of those bits that make the
 * kernels give WRONG counts on purpose (section-by-section measurement builds, tools/valu_ab.sh).  igd_hip_open refuses
 * such a library unless IGD_HIP_ALLOW_EXP_BUILD=1 is set, and igd_amd.Database refuses it outright. */
unsigned igd_hip_build_flags(void);
unsigned igd_hip_build_wrong_counts(void);

/* Instrumentation ------------------------------------------------------------------- */
/* Exact algorithmic-work terms for a device-resident batch (blocking). */
int igd_hip_batch_stats(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs,
                        const int32_t *d_qe, int64_t nq, int32_t v, int rule,
                        igd_hip_stats *out);
/* COMPULSORY traffic of the dominant kernel for one batch: the bytes igd_scan_tiles cannot avoid moving
 * through HBM when every visited unit's records are read exactly once -- the denominator-free part of
 * a roofline fraction that stays <= 1 (the algorithmic bytes above price the REFERENCE's re-reads).
 * Runs the batch once (grouping as `flags` say) into scratch counters and then counts, on the device,
 * the units the scan kernel visited.  Blocking. */
typedef struct {
    int64_t units;          /* units (<= 320-record chunks of a tile) with at least one candidate query     */
    int64_t records;        /* records in them                                                            */
    int64_t record_bytes;   /* records x bytes per record of the image read (6 / 8 compact, 12 / 16 exact) */
    int64_t unit_bytes;     /* 48-byte descriptors of ALL units + the per-tile query ranges / marks read     */
    int64_t query_bytes;    /* per-query words the kernel reads, each once (4 B/query in the compact merge join) */
    int64_t slab_bytes;     /* the workgroups' private counter rows written at the end of the kernel       */
    int64_t total;          /* sum of the four                                                            */
} igd_hip_traffic;
int igd_hip_batch_traffic(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe,
                          int64_t nq, int32_t v, int rule, int flags, igd_hip_traffic *out);
/* What this box's memory system delivers to simple streaming kernels, measured now (GB/s, 1e9):
 * rates[0] float4 copy kernel, read+write bytes (the guide's 6.29 TB/s figure is this measurement);
 * rates[1] float4 read-only kernel; rates[2] pinned device->host copy; rates[3] pinned host->device. */
int igd_hip_measure_rates(int device, double rates[4]);
/* HIP-event timing of the launches made by igd_hip_search_dev on their own stream:
 * begin() arms up to max_launches slots, end() waits and returns the number of launches
 * seen plus the average duration (ms) of the dominant scan kernel and of the whole
 * pipeline (bucket + scan + reduce). */
int igd_hip_profile_begin(igd_hip_db *db, int max_launches);
int igd_hip_profile_end(igd_hip_db *db, int *n_launches, double *avg_scan_ms,
                        double *avg_pipeline_ms);
/* Time only every `every`-th launch (default 1): an event is a packet of its own in the stream between two kernels and
 * costs the job about as much as a small kernel (10^6-query steps: 104 -> 95 us when the pipeline pair is dropped,
 * another ~4 us for the scan pair), so a job that is itself being timed samples.  Sticky per database. */
int igd_hip_profile_sampling(igd_hip_db *db, int every);
/* Name of the dominant kernel as rocprofv3 --kernel-trace prints it (for profiles/). */
const char *igd_hip_scan_kernel_name(void);
/* ... and the one the last batch of `db` actually ran on: "igd_scan_sorted" (merge join over the compact image) or
 * "igd_scan_tiles" (bucket path, exact arrays).  Waits for the batch. */
const char *igd_hip_last_scan_kernel(igd_hip_db *db);
/* TEST-ONLY: which routes the last batch of `db` took.  Fills out[0 .. min(n, IGD_HIP_ROUTE_WORDS) - 1] and returns the number
 * of words filled; 0 before the first batch (or when the device cannot be read).  Waits for the batch.  The list counters are
 * those of the batch's own control words: they stand until the handle's next batch.  Word k of out[]: */
enum {
    IGD_HIP_ROUTE_KERNEL = 0,     /* scan kernel igd_hip_last_scan_kernel names: 1 igd_scan_sorted, 2 igd_scan_tiles, 3 igd_scan_direct */
    IGD_HIP_ROUTE_FULL,           /* igd_scan_sorted: 0 the lean (pairwise-only) build, 1 the full (rank method) build; -1 another kernel */
    IGD_HIP_ROUTE_PACKED,         /* 1: the compact image, 0: the exact arrays                                              */
    IGD_HIP_ROUTE_LBSHIFT,        /* log2(queries per later block) of the bounds pass: 8, 10 or 12; 0 when it did not run     */
    IGD_HIP_ROUTE_NFIX,           /* entries of the merge join's exact-walk list (WALK_FIRST, WALK_LAST)                   */
    IGD_HIP_ROUTE_NLONG,          /* entries of the bucket path's exact-walk list (WALK_FIRST, WALK_ALL)                   */
    IGD_HIP_ROUTE_NHEAVYS,        /* tiles listed for heavy_sorted_body (merge join's skew valve)                          */
    IGD_HIP_ROUTE_NHEAVY,         /* tiles listed for heavy_bucket_body (bucket path's skew valve)                         */
    IGD_HIP_ROUTE_NFAR,           /* units listed for far_units_body                                                       */
    IGD_HIP_ROUTE_COV_SORTED,     /* 1: long queries of the merge join wrote coverage differences (set 0)                  */
    IGD_HIP_ROUTE_COV_BUCKET,     /* 1: long queries of the bucket path wrote coverage differences (set 1)                 */
    IGD_HIP_ROUTE_UNSORTED,       /* 1: the bounds pass found the batch not ordered by tile                                */
    IGD_HIP_ROUTE_NOTSTART,       /* 1: ordered by tile, but not by start inside a tile (rank method off)                  */
    IGD_HIP_ROUTE_WORDS
};
int igd_hip_last_batch_routes(igd_hip_db *db, int64_t *out, int n);
/* TEST-ONLY: the constants the route tests derive their shapes from, filled and counted like the words above (no device access;
 * valid from igd_hip_open on).  Word k of out[]: */
enum {
    IGD_HIP_RCONST_UNIT = 0,      /* records per unit (register slots per lane x 64 lanes)                                 */
    IGD_HIP_RCONST_ROUND,         /* units a wave of the lean build reads the descriptors of at once                       */
    IGD_HIP_RCONST_SHORT_TILES,   /* a query over more tiles than this has its last tile walked exactly (WALK_LAST)        */
    IGD_HIP_RCONST_DENSE_MIN,     /* full build: first-tile queries of a tile from which the rank method counts            */
    IGD_HIP_RCONST_LEAN_FIRST,    /* lean build: more first-tile queries than this list the tile for heavy_sorted_body     */
    IGD_HIP_RCONST_HEAVY_FIRST,   /* full build: the same                                                                  */
    IGD_HIP_RCONST_HEAVY_SLICE,   /* queries per slice of a listed tile                                                    */
    IGD_HIP_RCONST_FAR_WIDE,      /* full build: a far unit whose candidates span this many later blocks is listed         */
    IGD_HIP_RCONST_LATER_MAX,     /* later-tile candidates that come with a unit's records; one more makes the unit far    */
    IGD_HIP_RCONST_SBCAP,         /* this handle: query starts of one tile a wave of the full build keeps in LDS           */
    IGD_HIP_RCONST_LEAN_WAVES,    /* this handle: waves of one launch of the lean build (units beyond ROUND x this: a second round) */
    IGD_HIP_RCONST_WORDS
};
int igd_hip_route_constants(igd_hip_db *db, int64_t *out, int n);

#ifdef __cplusplus
}
#endif
#endif
