/* igd_core.h -- host-side core shared by the three ABI flavours (CLI, Python handle, R).
 *
 * Internal header (not installed): the public faces are include/igd_search.h,
 * include/igd_py_abi.h and include/igdr_abi.h.  Everything here is plain C99; the only
 * thing it calls for the search itself is the HIP engine of include/igd_hip.h -- there is
 * no CPU search path in this library.
 *
 * Reference counterparts (databio/IGD, /root/reference):
 *   igdc_open           get_igdinfo  src/igd_base.c:269-323  (+ whole tile region, once)
 *   igdc_load_index     get_fileinfo src/igd_base.c:235-267
 *   igdc_get_id         get_id       src/igd_base.c:325-331  (khash str->int, src/khash.h)
 *   igdc_parse_bed      parse_bed    src/igd_base.c:53-72
 *   igdc_lines_*        ks_getuntil  src/kseq.h:82-130 over gzread (src/igd_base.h:192)
 *   igdc_read_queries   the read/parse/lookup part of getOverlaps src/igd_search.c:708-714
 */
#ifndef IGD_CORE_H
#define IGD_CORE_H
#include <stdint.h>
#include <stdio.h>
#include "igd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IGDC_MAX_DEVICES 16
typedef struct igdc_db {
    int32_t nbp, gType, nCtg, nFiles;
    int32_t *nTile;          /* [nCtg]                                                  */
    int32_t *nCntFlat;       /* sum(nTile), contig-major (file order)                   */
    int32_t **nCnt;          /* [nCtg] -> into nCntFlat                                 */
    int64_t *tBase;          /* byte offset in the .igd of every 64th tile (flat numbering): a per-tile table would be
                                1.5 MB of fresh pages at roadmap scale -- 0.75 ms of page faults at every open, as much as
                                the reference needs for its whole header -- for a number that is one short sum away   */
    void    *reserved_;
    char   **cName;          /* [nCtg], each a 40-byte buffer as stored in the file     */
    char   **fileName;       /* [nFiles]                                                */
    int32_t *fileNr;
    double  *fileMd;
    int64_t  nTileTotal, nRecords, dataOff;
    int32_t *dict;           /* open-addressing contig dictionary                        */
    int32_t  dictCap;
    igd_hip_db *dev;         /* the database resident on the GPU (NULL until attached)   */
    /* multi-GPU: the same database resident on further devices; dev == devs[0] */
    int32_t     ndev;
    igd_hip_db *devs[IGDC_MAX_DEVICES];
    igd_hip_group *grp;      /* the devices as one group: slabs + ONE RCCL all-reduce of hits[] (igd_hip_group_search) */
} igdc_db;

/* byte offset of tile j of contig c in the .igd (what the reference keeps as tIdx[c][j], src/igd_base.c:288-303) */
static inline int64_t igdc_tile_off(const igdc_db *db, int32_t c, int32_t j)
{
    const int64_t t = (db->nCnt[c] - db->nCntFlat) + j;
    int64_t n = 0;
    for (int64_t k = t & ~(int64_t)63; k < t; k++) n += db->nCntFlat[k];
    return db->tBase[t >> 6] + n * (db->gType == 0 ? 12 : 16);
}

/* header tables of an .igd (no tile data is read) */
igdc_db *igdc_open(const char *igd_path);
/* "<igd minus last .ext>_index.tsv" */
char    *igdc_index_path(const char *igd_path);
int      igdc_load_index(igdc_db *db, const char *tsv_path);
void     igdc_close(igdc_db *db);
int32_t  igdc_get_id(const igdc_db *db, const char *chrm);

/* Put the tile region on the GPU (igd_hip_open).  _path maps the file; _fp reads through an
 * already open stream (the CLI flavour's global fP).  Returns IGD_HIP_OK or an IGD_HIP_ERR_*. */
int igdc_attach_path(igdc_db *db, const char *igd_path, int device);
int igdc_attach_fp(igdc_db *db, FILE *fp, int device);
/* Multi-GPU, one process driving several devices: the database is replicated on
 * devices[0..n) (uploaded by n host threads at once; the same device may be listed twice), and
 * igdc_search_multi gives device r the r-th CONTIGUOUS slab of the batch (one host thread per
 * device), then adds the n per-device vectors of nFiles counts into hits[] -- the reference keeps one
 * hits[] for all queries and prints it once (src/igd_search.c:925,1032-1039); a sum of non-negative
 * integers, so any partition of the queries gives the identical vector.  The sum is the engine group's RCCL all-reduce
 * (ncclAllReduce of int64[nFiles] on every engine's stream, igd_hip_group_search); a host-side add of the n vectors only
 * where RCCL cannot be used (igd_hip.h).  "IGD_DEVICES=0,1,.." selects the devices for the command line tool. */
int igdc_attach_path_multi(igdc_db *db, const char *igd_path, const int *devices, int n);
int igdc_search_multi(igdc_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                      int32_t v, int rule, int flags, int64_t *hits, int64_t *total);
/* "0,1,2" -> devices[]; returns the count (0 when the variable is unset or empty) */
int igdc_devices_from_env(int *devices, int max);

/* ONE query interval without the GPU.  The reference answers `-r` / get_overlaps() by reading the one to few tiles the
 * interval touches (fseek/fread of cnt records, src/igd_search.c:469-476) -- a few KB -- while putting the database on
 * the GPU means uploading all of it (851 MB at roadmap scale) for a single wave's work: for the single-interval entry
 * points of the three flavours (`igd search -r`, get_overlaps*, search_1) the host therefore reads those tiles itself
 * (pread) and counts.  Batches -- query files, search_n -- never come here: they have no CPU path.
 * Semantics = the engine's (and the reference's, src/igd_search.c:454-534 / :623-694 / :30-112): rule NEST or FLAT,
 * hits are the records with lob <= start < qe && end > qs [&& value >= v], lob = the tile's start in later tiles.
 * `emit` (may be NULL) is called per overlap in the reference's -f order (tiles ascending, record index descending).
 * Returns the number of overlaps, or -1 on an I/O error. */
/* one overlap: dataset, start, end, and where the record sits -- its index inside tile `tile` of the contig */
typedef void (*igdc_emit_fn)(void *ctx, int32_t idx, int32_t start, int32_t end, int32_t in_tile, int32_t tile);
int64_t igdc_walk_one(const igdc_db *db, int fd, int32_t ichr, int32_t qs, int32_t qe, int32_t v, int use_v, int rule,
                      int64_t *hits, igdc_emit_fn emit, void *ctx);

/* SMALL query files on the host (igd_hostpath.c; product code).  The reference starts cheaply -- header only, then the
 * tiles a query touches (src/igd_base.c:269-323, src/igd_search.c:469-476) -- while the engine costs a fixed ~0.18 s of HIP
 * start-up and upload: files of at most igdc_host_limit() queries (IGD_HOST_MAX_QUERIES; 0 = every file goes to the GPU) are
 * counted with pread() on the .igd (per-thread tile buffers) by a few host threads, the reference's per-query algorithm.  NOT a
 * fallback: the choice depends on the number of queries only, never on whether a device is usable; larger files have
 * no CPU path.  The engine's own entry points (igd_hip.h) never come here. */
typedef struct igdc_map igdc_map;
int64_t   igdc_host_limit(void);                            /* counting searches: 25 000 queries per usable thread, <= 400 000 */
int64_t   igdc_host_limit_enum(void);                       /* `-f`: 25 000 per usable thread */
int       igdc_host_probably_small(const char *qfile);       /* by file size: parse it before starting the engine */
igdc_map *igdc_map_open(const igdc_db *db, int fd);           /* fd stays the caller's */
void      igdc_map_close(igdc_map *m);
/* hits[] is ADDED to; *total = overlaps of the batch.  v = IGD_HIP_NO_VALUE_FILTER: no filter.  0 on success. */
int igdc_search_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                     int64_t nq, int32_t v, int rule, int64_t *hits, int64_t *total);
/* Support counts: support[f] += the queries that overlap at least one record of file f (igdc_search_host adds every
 * overlapping record), *nhit (may be NULL) += the queries that overlap any record.  Same threading, rule and filter as
 * igdc_search_host; added to the caller's only if every tile could be read.  0 on success. */
int igdc_support_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                      int64_t nq, int32_t v, int rule, int64_t *support, int64_t *nhit);
/* Covered base pairs: coverage[f] += over the queries, the bp of [qs, qe) that lie under the union of file f's counted
 * records (an interval union per query, not a sum over records), *covered (may be NULL) += the same for the union over all
 * files.  Same records, threading, rule and filter as igdc_support_host; added to the caller's only if every tile could be
 * read.  0 on success. */
/* The two above and igdc_permute_host below under a minimum overlap per pair (include/igd_hip.h: igd_hip_min_overlap -- the same
 * inline predicate as the kernels'; NULL or all zero: inactive, the plain function; a field out of range: -1, nothing written).
 * The enrichment of `-U` on the host is these supports through igdc_fisher_host, so it needs no twin of its own. */
int igdc_search_host_ov(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                        int64_t nq, int32_t v, int rule, int64_t *hits, int64_t *total, const igd_hip_min_overlap *min_overlap);
int igdc_support_host_ov(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                         int64_t nq, int32_t v, int rule, int64_t *support, int64_t *nhit, const igd_hip_min_overlap *min_overlap);
/* Support counts per GROUP of datasets on the host (what igd_hip_group_support_sets computes for one set; include/igd_hip.h has
 * the grouping grp_off / grp_idx / ngroups and the definitions): gsupport[g] += the queries that overlap a record of at least one
 * dataset of group g, *gnhit (may be NULL) += the queries that overlap a dataset with at least one group.  Same records,
 * threading, rule, filter and minimum overlap (may be NULL) as igdc_support_host_ov.  0 on success; -1, nothing written, for a
 * bad argument -- a grouping that igd_hip_groups_first_bad refuses, ngroups outside 1 .. IGD_HIP_GROUP_MAX -- or when a tile
 * could not be read. */
int igdc_group_support_host_ov(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const int32_t *grp_off, const int32_t *grp_idx, int32_t ngroups, int32_t v, int rule, int64_t *gsupport,
                               int64_t *gnhit, const igd_hip_min_overlap *min_overlap);
int igdc_permute_host_ov(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                         const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed,
                         int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax,
                         const igd_hip_min_overlap *min_overlap);
int igdc_coverage_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                       int64_t nq, int32_t v, int rule, int64_t *coverage, int64_t *covered);
/* Per-query membership: row q of bits (ceil(nFiles / 32) uint32 words; file f = bit f & 31 of word f >> 5) says which
 * files query q overlaps, nfiles_hit[q] (may be NULL) = their number, *nhit (may be NULL) += the queries with any file.  Rows
 * and nfiles_hit are OVERWRITTEN, every word of them (the threads write disjoint rows straight into the caller's).  Same
 * records, threading, rule and filter as igdc_support_host.  0 on success, -1 if a tile could not be read (rows undefined). */
int igdc_membership_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                         int64_t nq, int32_t v, int rule, uint32_t *bits, int32_t *nfiles_hit, int64_t *nhit);
/* Fisher's exact test, one-sided ("greater"), of ncell tables a b / c d: pvalue_log = -log10 P(X >= a) for X ~
 * Hypergeometric(a+b+c+d, a+b, a+c), in log space (finite however small p is; +0.0 at the support minimum and for N = 0), and
 * odds_ratio (may be NULL) = (a d) / (b c), the sample odds ratio (+inf when b c = 0 < a d, NaN when both are 0) -- what
 * igd_hip_fisher_tables computes, on the calling thread with lgamma.  Outputs are OVERWRITTEN.  0 on success; -1, the
 * outputs untouched, for a negative entry or N >= 2^31. */
int igdc_fisher_host(const int64_t *a, const int64_t *b, const int64_t *c, const int64_t *d, int64_t ncell, double *pvalue_log,
                     double *odds_ratio);
/* Rank columns and Benjamini-Hochberg q-values of an enrichment table, row by row (a row = the ncols cells of one query
 * set = one family of tests): what igd_hip_enrich_ranks computes (include/igd_hip.h has the definitions), on the calling
 * thread with qsort and log10.  Any output may be NULL, and an input that no requested output needs; max_rnk and mean_rnk
 * need all three.  Outputs are OVERWRITTEN.  0 on success; -1, the outputs untouched, for a missing input, ncols > 2^20 or
 * a pvalue_log that is negative or NaN. */
int igdc_rank_host(const int64_t *support, const double *pvalue_log, const double *odds_ratio, int64_t nrows, int64_t ncols,
                   double *qvalue_log, int32_t *rnk_sup, int32_t *rnk_pv, int32_t *rnk_or, int32_t *max_rnk, double *mean_rnk);
/* Query sets restricted to a universe (what igd_hip_restrict_sets computes; include/igd_hip.h has the definitions): row k of
 * bits (ceil(nu / 32) uint32 words; universe region u, the caller's numbering, = bit u & 31 of word u >> 5) holds the universe
 * regions that some region of set k overlaps, size[k] their number.  Needs no database.  Outputs are OVERWRITTEN.  0 on
 * success; -1, the outputs untouched, for a bad set_off, a missing array or nu + 1 >= 2^31. */
int igdc_restrict_host(const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                       const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu, uint32_t *bits, int64_t *size);
/* Enrichment of the restricted sets (what igd_hip_enrich_restricted computes): igdc_restrict_host, igdc_membership_host over
 * the universe, the gather over the member rows of each set's bits, igdc_fisher_host on a = support, b = usupport - a,
 * c = size - a, d = nu - usupport - c.  Outputs are OVERWRITTEN; odds_ratio, bits, nhit and unhit may be NULL.  0 on success;
 * -1 for a bad argument (nothing written) or when a tile could not be read (outputs undefined). */
int igdc_enrich_restricted_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                                const int64_t *set_off, int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe,
                                int64_t nu, int32_t v, int rule, int64_t *support, int64_t *usupport, int64_t *size, double *pvalue_log,
                                double *odds_ratio, uint32_t *bits, int64_t *nhit, int64_t *unhit);
/* Dataset x dataset co-occurrence over one region list (what igd_hip_cooccur computes; include/igd_hip.h has the definitions):
 * cooc[f * nFiles + g] = the regions that overlap a record of file f and one of file g, *nhit (may be NULL) = the regions with
 * any file.  Both are DEFINED by the call.  igdc_membership_host in chunks, a transpose into bit columns, popcounts of the
 * column pairs with threads over the rows.  0 on success; -1 for a bad argument or more than IGD_COOCCUR_MAX_FILES files
 * (nothing written), or when a tile could not be read (outputs undefined). */
int igdc_cooccur_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                      int32_t v, int rule, int64_t *cooc, int64_t *nhit);
/* out[i * n + j] = popcount(a_i AND b_j) over rows of nwords32 uint32 words (what igd_hip_bitrows_gram computes): a = m rows,
 * b = n rows, b == NULL: the symmetric form (b = a, n = m).  out is DEFINED.  Needs no database.  0, or -1 (nothing written)
 * for a missing array, a negative size or more than 2^28 cells. */
int igdc_bitrows_gram_host(const uint32_t *a, int64_t m, const uint32_t *b, int64_t n, int64_t nwords32, int64_t *out);
/* Permutation null of region-set support on the host (what igd_hip_permute_support computes; include/igd_hip.h has the generator,
 * the outputs -- nFiles + 1 words each, all but observed may be NULL, all DEFINED -- and the refusals).  igdc_permute_regions_host
 * is kernel igd_permute_regions: permutations [p0, p0 + np) of nq regions into out_qs, out_qe (int32[np * nq]); nctg is the
 * caller's.  igdc_permute_host counts the set with igdc_support_host and every permuted set with the same per-query walk,
 * threads over the permutations.  0 on success; -1 for a refused argument (nothing written) or when a tile could not be
 * read (nothing written).  igdc_permute_first_bad: the first region on a known contig that breaks 0 <= s <= e <= L, L >= 1,
 * or -1. */
int igdc_permute_regions_host(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len, int32_t nctg,
                              int mode, uint64_t seed, int64_t p0, int64_t np, int32_t *out_qs, int32_t *out_qe);
int64_t igdc_permute_first_bad(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len, int32_t nctg);
int igdc_permute_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                      const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed,
                      int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax);
/* Per column f of n, with P = nperm permutations:
 *     mean = sum / P          sd = sqrt((P * sumsq - sum^2) / (P * (P - 1)))   (the numerator exact in 128 bits; NaN when P = 1)
 *     z = (observed - mean) / sd   (NaN when sd is 0 or NaN)
 *     p_upper = (n_ge + 1) / (P + 1),  p_lower = (n_le + 1) / (P + 1), reported as -log10
 * Every output may be NULL.  Needs no database.  0, or -1 for a missing input or nperm < 1. */
int igdc_perm_summary(const int64_t *observed, const int64_t *sum, const int64_t *sumsq, const int64_t *n_ge, const int64_t *n_le,
                      int64_t nperm, int64_t n, double *mean, double *sd, double *z, double *nlog10_p_upper, double *nlog10_p_lower);
/* Nearest record per dataset within a window (what igd_hip_nearest and igd_hip_nearest_sets compute; include/igd_hip.h has the
 * definitions): dist (int32[nq * nFiles]) and dmin (int32[nq], may be NULL); n_within, n_overlap, sum_dist (int64[nsets *
 * (nFiles + 1)], each may be NULL; column nFiles from dmin).  Every output is OVERWRITTEN, every word of it.  Each region is
 * widened by the window, visits its tiles under rule FLAT with the prefix skip and keeps one minimum per file; threads run
 * over the regions.  0 on success; -1 for a missing array, a bad set_off or a window outside 0 .. 2^30 (nothing written), or
 * when a tile could not be read (outputs undefined). */
int igdc_nearest_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                      int32_t window, int32_t v, int32_t *dist, int32_t *dmin);
int igdc_nearest_sets_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                           const int64_t *set_off, int32_t nsets, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap,
                           int64_t *sum_dist);
/* Signed nearest distances and their histogram (what igd_hip_nearest_signed and igd_hip_nearest_hist compute; include/igd_hip.h
 * has the definitions): sdist (int32[nq * nFiles]) and sdmin (int32[nq], may be NULL), IGD_HIP_NEAREST_NO_RECORD where there is
 * no record; hist (int64[nsets * (ne + 1) * (nFiles + 1)], column nFiles from sdmin).  The walk of igdc_nearest_host with
 * igd_hip_nearest_key minimised instead of d, threads over the regions.  0 on success; -1 as above, and for edges that are not
 * 1 .. IGD_HIP_NEAREST_MAX_EDGES strictly ascending values (nothing written). */
int igdc_nearest_signed_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                             int32_t window, int32_t v, int32_t *sdist, int32_t *sdmin);
int igdc_nearest_hist_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                           const int64_t *set_off, int32_t nsets, int32_t window, int32_t v, const int32_t *edges, int32_t ne,
                           int64_t *hist);
/* Flanking records per dataset and the relative-distance histogram (what igd_hip_flank and igd_hip_flank_reldist compute;
 * include/igd_hip.h has the definitions): up and down (int32[nq * nFiles] each, both required when there are files), upmin and
 * downmin (int32[nq], each may be NULL), -1 where there is none; hist (int64[nsets * nbins * (nFiles + 1)], column nFiles from
 * upmin / downmin).  The walk of igdc_nearest_host with two words per file, threads over the regions.  0 on success; -1 as
 * above, and for a measure that is neither IGD_HIP_FLANK_EDGES nor IGD_HIP_FLANK_MIDPOINTS or nbins outside 1 ..
 * IGD_HIP_FLANK_MAX_BINS (nothing written). */
int igdc_flank_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                    int32_t window, int measure, int32_t v, int32_t *up, int32_t *down, int32_t *upmin, int32_t *downmin);
int igdc_flank_reldist_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                            const int64_t *set_off, int32_t nsets, int32_t window, int measure, int32_t v, int32_t nbins, int64_t *hist);
/* Merged region sets and the base-pair Jaccard (what igd_hip_merge_sets, igd_hip_dataset_bp and igd_hip_jaccard_sets compute;
 * include/igd_hip.h has the definitions): a sort and a sweep per set, threads over the sets; file_bp and the intersections
 * through igdc_coverage_host, threads over the tiles and the runs.  igdc_merge_host needs the database only for its number of
 * contigs.  Every output is OVERWRITTEN, every word of it.  0 on success; -1 for a missing array, a bad set_off, a gap outside
 * 0 .. 2^30 (nothing written), or when a tile could not be read (outputs undefined).  The host route keeps no file_bp between
 * calls. */
int igdc_merge_host(const igdc_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                    int64_t gap, int32_t *m_ichr, int32_t *m_qs, int32_t *m_qe, int64_t *m_off, int32_t *m_count, int64_t *n_dropped);
int igdc_dataset_bp_host(const igdc_db *db, const igdc_map *m, int32_t v, int rule, int64_t *file_bp);
int igdc_jaccard_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                      const int64_t *set_off, int32_t nsets, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *file_bp,
                      int64_t *n_merged, int64_t *n_dropped);
/* inter / (set_bp + file_bp - inter), NaN where the union is 0; and over inter[nsets][ncols], set_bp[nsets], file_bp[ncols] the
 * Jaccard and the two containment fractions inter / set_bp and inter / file_bp (doubles, NaN where the divisor is 0; each may
 * be NULL).  Need no database.  0, or -1 for a missing input. */
double igdc_jaccard_value(int64_t inter, int64_t set_bp, int64_t file_bp);
int igdc_jaccard_summary(const int64_t *inter, const int64_t *set_bp, const int64_t *file_bp, int64_t nsets, int64_t ncols, double *jaccard,
                         double *set_fraction, double *file_fraction);
/* mean[i] = sum_dist[i] / n_within[i] as a double, NaN where n_within[i] = 0.  Needs no database.  0, or -1 for a missing array. */
int igdc_nearest_summary(const int64_t *n_within, const int64_t *sum_dist, int64_t n, double *mean);
/* Values of the overlapping records per region and dataset (what igd_hip_map and igd_hip_map_sets compute; include/igd_hip.h has
 * the definitions and the ops): count (int32[nq * nFiles]) and agg (int64[nq * nFiles]; under op COUNT it may be NULL and
 * receives the counts when it is not); n_hit, pairs, agg_sum (int64[nsets * nFiles], each may be NULL).  Every output is
 * OVERWRITTEN, every word of it.  Each region visits its tiles under rule FLAT with the prefix skip, as igdc_nearest_host at
 * W = 0; threads run over the regions.  0 on success; -1 for a missing array, a bad set_off, an unknown op or a value op on a
 * gType 0 database (nothing written), or when a tile could not be read (outputs undefined). */
int igdc_map_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int op,
                  int32_t v, int32_t *count, int64_t *agg);
int igdc_map_sets_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                       const int64_t *set_off, int32_t nsets, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum);
/* mean_region[i] = agg_sum[i] / n_hit[i] and, under op SUM, mean_pair[i] = agg_sum[i] / pairs[i] (the mean value of a counted
 * record; NaN under the other ops), as doubles, NaN where the divisor is 0.  mean_pair may be NULL.  Needs no database.  0, or
 * -1 for a missing array or an unknown op. */
int igdc_map_summary(const int64_t *n_hit, const int64_t *pairs, const int64_t *agg_sum, int64_t n, int op, double *mean_region,
                     double *mean_pair);
/* Permutation null of the nearest-record distances on the host (what igd_hip_permute_nearest computes; include/igd_hip.h): each
 * output is int64[(nperm + 1) * (nFiles + 1)] (may be NULL), row 0 the set as given, row p + 1 permutation p of
 * igdc_permute_regions_host's generator counted as igdc_nearest_sets_host counts a set; threads run over the rows.  0; -1 for a
 * refused argument (igdc_permute_host's but the sumsq guard, and a window outside 0 .. 2^30) or when a tile could not be read
 * -- nothing is written then. */
int igdc_permute_nearest_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                              const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t window, int32_t v,
                              int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist);
/* The summary of such a null distribution, per column f of ncols; n_within and sum_dist are int64[(nperm + 1) * ncols].  With
 * P = nperm, nw_0 / sd_0 the observed row and nw_p / sd_p the permuted rows:
 *     counts      within_mean, within_sd, within_z: igdc_perm_summary's formulas over nw_p (the variance's numerator exact in 128
 *                 bits; sd NaN when P = 1, z NaN when sd is 0 or NaN); within_n_ge = #{p : nw_p >= nw_0};
 *                 nlog10_p_within_upper = -log10((within_n_ge + 1) / (P + 1))
 *     distances   mean_dist = sd_0 / nw_0 (NaN when nw_0 = 0); n_def = #{p : nw_p > 0}; dist_mean and dist_sd over
 *                 m_p = sd_p / nw_p of those permutations, in doubles, two passes in permutation order (dist_mean NaN when
 *                 n_def = 0; dist_sd divides by n_def - 1 and is NaN when n_def < 2); dist_z = (mean_dist - dist_mean) / dist_sd,
 *                 NaN when nw_0 = 0 or the sd is 0 or NaN; dist_n_le = #{p : nw_p > 0 and sd_p * nw_0 <= sd_0 * nw_p}, compared
 *                 exactly in 128 bits -- a permutation with nothing within the window is not "as close" -- and 0 when nw_0 = 0;
 *                 nlog10_p_dist_lower = -log10((dist_n_le + 1) / (P + 1))
 * within_n_ge, n_def and dist_n_le are int64[ncols], the others double[ncols]; every output may be NULL.  Needs no database.
 * 0, or -1 for a missing input or nperm < 1. */
int igdc_perm_nearest_summary(const int64_t *n_within, const int64_t *sum_dist, int64_t nperm, int64_t ncols, double *within_mean,
                              double *within_sd, double *within_z, int64_t *within_n_ge, double *nlog10_p_within_upper, double *mean_dist,
                              double *dist_mean, double *dist_sd, double *dist_z, int64_t *n_def, int64_t *dist_n_le,
                              double *nlog10_p_dist_lower);
/* Permutation null of the base-pair overlap on the host (what igd_hip_permute_bp computes; include/igd_hip.h): inter is
 * int64[(nperm + 1) * (nFiles + 1)], set_bp and n_merged int64[nperm + 1], n_dropped one word (each may be NULL); row 0 the set as
 * given, row p + 1 permutation p of igdc_permute_regions_host's generator, every row merged by igdc_merge_host at gap 0 and its
 * runs covered by igdc_coverage_host; threads run over the rows.  0; -1 for a refused argument (igdc_permute_host's but the
 * sumsq guard) or when a tile could not be read -- nothing is written then. */
int igdc_permute_bp_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                         const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter,
                         int64_t *set_bp, int64_t *n_merged, int64_t *n_dropped);
/* The summary of such a null distribution, per column f of ncols; inter is int64[(nperm + 1) * ncols], set_bp int64[nperm + 1],
 * file_bp int64[ncols] (igd_hip_dataset_bp).  With P = nperm, x_0 the observed row and x_p the permuted rows of column f:
 *     base pairs  observed = x_0; mean, sd, z: igdc_perm_summary's formulas over x_p (sum and sum of squares exact in 128 bits
 *                 -- x^2 alone passes 2^63 from 3.04 x 10^9 bp; sd NaN when P = 1, z NaN when sd is 0 or NaN);
 *                 fold = x_0 / mean, NaN when the mean is 0; n_ge = #{p : x_p >= x_0}, n_le = #{p : x_p <= x_0};
 *                 nlog10_p_upper = -log10((n_ge + 1) / (P + 1)), nlog10_p_lower = -log10((n_le + 1) / (P + 1))
 *     Jaccard     u_r = set_bp[r] + file_bp[f] - x_r, the union of row r; jaccard = x_0 / u_0 (NaN when u_0 = 0);
 *                 jaccard_n_def = #{p : u_p != 0}; jaccard_mean and jaccard_sd over j_p = x_p / u_p of those permutations, in
 *                 doubles, two passes in permutation order (mean NaN when n_def = 0; sd divides by n_def - 1, NaN when
 *                 n_def < 2); jaccard_n_ge = #{p : u_p != 0 and x_p * u_0 >= x_0 * u_p}, compared exactly in 128 bits (the
 *                 products reach about 2^77) -- a ratio over 0 is not defined and counts on neither side -- and 0 when u_0 = 0
 * observed, n_ge, n_le, jaccard_n_def and jaccard_n_ge are int64[ncols], the others double[ncols]; every output may be NULL.
 * Needs no database.  0, or -1 for a missing input or nperm < 1. */
int igdc_perm_bp_summary(const int64_t *inter, const int64_t *set_bp, const int64_t *file_bp, int64_t nperm, int64_t ncols,
                         int64_t *observed, double *mean, double *sd, double *z, double *fold, int64_t *n_ge, int64_t *n_le,
                         double *nlog10_p_upper, double *nlog10_p_lower, double *jaccard, double *jaccard_mean, double *jaccard_sd,
                         int64_t *jaccard_n_def, int64_t *jaccard_n_ge);
/* The workspace of the permutation nulls (include/igd_hip.h: THE WORKSPACE has the definition of the table), shared by the
 * host route and the engine's callers.
 * igdc_workspace_build: the table of the n segments (ichr, a, b) on nctg contigs of lengths ctg_len: merged at gap 0 through
 * igdc_merge_host, clipped to the contigs, ordered and summed; *out is one allocation, freed by igdc_workspace_free.  0; -1 for
 * a missing array, a negative length or no memory (nothing allocated).  A workspace without a segment is a table like any other.
 * igdc_workspace_valid: igd_hip_workspace_valid as a symbol of the library.
 * igdc_workspace_first_unplaceable: the first valid region on a known contig that fits in no segment of its contig (T == 0),
 * or -1; the table must be valid for ctg_len.
 * igdc_workspace_outside: the regions on known contigs that do not lie inside one segment (s >= a and e <= b; an inverted
 * region lies in none), or -1 without memory.  Information only: nothing refuses on it.
 * igdc_read_workspace: a BED file through igdc_read_queries (the command line's rule for `-q`; lines on contigs the
 * database lacks are dropped), built for the database's contigs.  0; -1 when the file cannot be opened; -2 when the table
 * could not be built.
 * The _ws routes are the four host routes above with the table as their last argument: NULL is the route above; with a table
 * the mode must be IGD_HIP_PERM_WORKSPACE, and -1 (nothing written) is also an invalid table and, in the three drivers, a region
 * on a known contig that fits in no segment. */
int igdc_workspace_build(const int32_t *ichr, const int32_t *a, const int32_t *b, int64_t n, const int32_t *ctg_len, int32_t nctg,
                         igd_hip_workspace **out);
void igdc_workspace_free(igd_hip_workspace *ws);
int igdc_workspace_valid(const igd_hip_workspace *ws, const int32_t *ctg_len, int32_t nctg);
int64_t igdc_workspace_first_unplaceable(const igd_hip_workspace *ws, const int32_t *ctg_len, const int32_t *ichr, const int32_t *qs,
                                         const int32_t *qe, int64_t nq);
int64_t igdc_workspace_outside(const igd_hip_workspace *ws, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq);
int igdc_read_workspace(const igdc_db *db, const char *path, const int32_t *ctg_len, igd_hip_workspace **out);
int igdc_permute_regions_host_ws(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len, int32_t nctg,
                                 int mode, uint64_t seed, int64_t p0, int64_t np, int32_t *out_qs, int32_t *out_qe,
                                 const igd_hip_workspace *ws);
int igdc_permute_host_ws(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                         const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed,
                         int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax,
                         const igd_hip_min_overlap *min_overlap, const igd_hip_workspace *ws);
int igdc_permute_nearest_host_ws(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                 const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t window, int32_t v,
                                 int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist, const igd_hip_workspace *ws);
int igdc_permute_bp_host_ws(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                            const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter,
                            int64_t *set_bp, int64_t *n_merged, int64_t *n_dropped, const igd_hip_workspace *ws);
/* The three nulls by resampling from a universe on the host (what igd_hip_permute_*_rs and igd_hip_resample_regions compute;
 * include/igd_hip.h has THE DRAW, the outputs and the refusals).  igdc_resample_regions_host is kernel igd_resample_regions: draws
 * [p0, p0 + np) of nq regions from the pool into out_ichr, out_qs, out_qe (int32[np * nq], draw-major).  The _rs forms are the _ws
 * forms with a pool in the place of ctg_len, mode and workspace: row 0 is the set as given, a row r > 0 is filled by draw r - 1
 * instead of the generator, and walked with the drawn contigs.  0 on success; -1 for a refused argument -- the engine's
 * refusals -- or when a tile could not be read (nothing written). */
int igdc_resample_regions_host(const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, int64_t nq,
                               uint64_t seed, int64_t p0, int64_t np, int32_t *out_ichr, int32_t *out_qs, int32_t *out_qe);
int igdc_permute_host_rs(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                         const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                         int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le,
                         int64_t *pmin, int64_t *pmax, const igd_hip_min_overlap *min_overlap);
int igdc_permute_nearest_host_rs(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                 const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                                 int64_t nperm, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist);
int igdc_permute_bp_host_rs(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                            const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                            int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged, int64_t *n_dropped);
/* Permutation null of the overlapping records' values on the host (what igd_hip_permute_map, _ws and _rs compute;
 * include/igd_hip.h): each output is int64[(nperm + 1) * nFiles] (may be NULL), row 0 the set as given, row p + 1 permutation p
 * of igdc_permute_regions_host's generator (_rs: draw p of the pool) measured as igdc_map_sets_host measures a set; threads run
 * over the rows.  0; -1 for a refused argument (an unknown op, a value op on a gType 0 database, then igdc_permute_nearest_host's
 * but the window) or when a tile could not be read -- nothing is written then. */
int igdc_permute_map_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                          const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs,
                          int64_t *agg_sum);
int igdc_permute_map_host_ws(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                             const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int op, int32_t v, int64_t *n_hit,
                             int64_t *pairs, int64_t *agg_sum, const igd_hip_workspace *ws);
int igdc_permute_map_host_rs(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                             const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                             int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum);
/* The summary of such a null distribution, per column f of ncols; n_hit, pairs and agg_sum are int64[(nperm + 1) * ncols].  The
 * statistic of row r is m_r = a_r / d_r with a = agg_sum and d = n_hit (over_pairs = 0: mean_region) or d = pairs (over_pairs
 * != 0: mean_pair, regioneR's meanInRegions over pairs); it is undefined where d_r = 0.  With P = nperm and row 0 the observed one:
 *     statistic   observed = m_0 (NaN when d_0 = 0); n_def = #{p : d_p > 0}; mean and sd over m_p of those permutations, in
 *                 doubles, two passes in permutation order (mean NaN when n_def = 0; sd divides by n_def - 1 and is NaN when
 *                 n_def < 2: igdc_perm_nearest_summary's convention); z = (observed - mean) / sd, NaN when d_0 = 0 or the sd is 0
 *                 or NaN; n_ge = #{p : d_p > 0 and m_p >= m_0}, n_le the same with <=, compared exactly as a_p d_0 against
 *                 a_0 d_p in 128 bits (a tie counts in both), both 0 when d_0 = 0; nlog10_p_upper = -log10((n_ge + 1) /
 *                 (n_def + 1)), nlog10_p_lower the same of n_le: NaN when d_0 = 0, 0 when n_def = 0
 *     counts      nhit_mean, nhit_sd, nhit_z: igdc_perm_summary's formulas over the permuted n_hit
 * n_def, n_ge and n_le are int64[ncols], the others double[ncols]; every output may be NULL.  Needs no database.  0, or -1 for a
 * missing input or nperm < 1. */
int igdc_perm_map_summary(const int64_t *n_hit, const int64_t *pairs, const int64_t *agg_sum, int64_t nperm, int64_t ncols, int over_pairs,
                          double *observed, int64_t *n_def, double *mean, double *sd, double *z, int64_t *n_ge, int64_t *n_le,
                          double *nlog10_p_upper, double *nlog10_p_lower, double *nhit_mean, double *nhit_sd, double *nhit_z);
/* The support of a region set under rigid shifts on the host (what igd_hip_shift_regions and igd_hip_shift_support compute;
 * include/igd_hip.h has THE SHIFT, the outputs and the refusals).  igdc_shift_regions_host is kernel igd_shift_regions: nq regions
 * under each of nshift offsets into out_qs, out_qe (int32[nshift * nq], shift-major); nctg is the caller's.
 * igdc_shift_support_host_ov: shifted is int64[nshift * (nFiles + 1)], DEFINED; row j is the set moved by offsets[j], walked with
 * the per-query code of igdc_support_host_ov (min_overlap NULL: no threshold); threads run over the rows as in igdc_permute_host.
 * 0 on success; -1 for a refused argument -- the engine's refusals -- or when a tile could not be read (nothing written). */
int igdc_shift_regions_host(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len, int32_t nctg,
                            const int32_t *offsets, int64_t nshift, int32_t *out_qs, int32_t *out_qe);
int igdc_shift_support_host_ov(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const int32_t *ctg_len, const int32_t *offsets, int64_t nshift, int32_t v, int rule, int64_t *shifted,
                               const igd_hip_min_overlap *min_overlap);
/* A genome file, lines `name<TAB>length`: len[c] = the length of contig c of the database (int32[nCtg]); lines of contigs the
 * database does not know are ignored, contigs the file does not name get 0.  0; -1 when the file cannot be opened; -2 for a
 * line of a known contig without a length or with one that is negative or above 2^31 - 1 (*bad_line, may be NULL, = its
 * number from 1). */
int igdc_read_genome(const igdc_db *db, const char *path, int32_t *len, int64_t *bad_line);
/* `-f` (rule NEST, the reference's order): qoff[0..nq] offsets, *out malloc'd (free()), entries as igd_hip_enumerate's */
int igdc_enumerate_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                        int64_t nq, int64_t *qoff, igd_hip_hit **out, int64_t *total);

/* handle flavours: small batch and no engine resident -> host; else the engine, attached (igdc_attach_path) when first needed.
 * Returns IGD_HIP_OK or the engine's error code. */
int igdc_search_auto(igdc_db *db, const char *path, int device, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                     int64_t nq, int32_t v, int rule, int flags, int64_t *hits, int64_t *total);

/* BED line -> (contig, start, end).  Mutates `line`.  require_chr=1 is the CLI rule
 * (name starts with "chr", shorter than 40, end > 0: src/igd_base.c:69); require_chr=0 is
 * the rule of the Python/R forks (>= 3 fields: src_py/igd_base.c:44). */
char *igdc_parse_bed(char *line, int32_t *st, int32_t *en, int require_chr);

/* '\n'-separated lines of a plain or gzip file */
typedef struct igdc_lines igdc_lines;
igdc_lines *igdc_lines_open(const char *path);
char       *igdc_lines_next(igdc_lines *r, int64_t *len);   /* NULL at end; buffer is reused */
void        igdc_lines_close(igdc_lines *r);

/* accepted queries of one file, as arrays */
typedef struct {
    int64_t n, cap;
    int32_t *ichr, *qs, *qe;
    int32_t unsorted;        /* 0 while every pushed query was >= the previous by (contig, start) */
    int32_t max_len;         /* largest qe - qs pushed (0 for an empty set): queries shorter than a tile let a dense sorted
                              * file take the engine's DIRECT step (IGD_HIP_FLAG_SHORT, verified on the device) */
} igdc_queries;
/* the engine flags a parsed query set earns: IGD_HIP_FLAG_SORTED when it is ordered, + IGD_HIP_FLAG_SHORT when no query is
 * as long as a tile of `nbp` bp */
int  igdc_queries_flags(const igdc_queries *q, int32_t nbp);
/* returns 0, or -1 when the file cannot be opened.  Lines whose contig is not in the
 * database are dropped here (the reference drops them in get_overlaps, :456-457). */
int  igdc_read_queries(const igdc_db *db, const char *qfile, int require_chr, igdc_queries *out);
void igdc_queries_free(igdc_queries *q);
/* every contig ONE run ordered by start, only the runs out of contig order (a sorted BED with another chromosome order
 * than the database's): put the runs into contig order, clear q->unsorted, return 1; otherwise 0.  Hits-only searches. */
int  igdc_queries_group_contigs(igdc_queries *q, int32_t nCtg);
int  igdc_queries_push(igdc_queries *q, int32_t ichr, int32_t qs, int32_t qe);

#ifdef __cplusplus
}
#endif
#endif
