/* igd_hip_lazy.c -- the host flavours' door to the HIP engine: libigd_hip.so is mapped when the FIRST engine function is
 * called, not when the process starts.
 *
 * Why: libigd_hip.so needs libamdhip64 and a dozen ROCm libraries; mapping and initialising them costs ~13 ms of every
 * process start (measured: `igd` without arguments 13.0 ms, the reference 1.1 ms) -- more than the reference needs for a
 * whole `igd search -q` of 10^3 queries (6 ms).  The entry points that never touch the GPU -- `-r`, get_overlaps*, small
 * query files (igd_hostpath.c), the header loaders -- should not pay it.  So libigd.so / libigd_py.so / libigdr.so do NOT
 * link -ligd_hip: they carry these trampolines, one per engine function the host code calls (include/igd_hip.h), which
 * dlopen "libigd_hip.so" from the directory this library was loaded from and forward.
 *
 * Not a fallback of any kind: if the engine library cannot be loaded every trampoline fails loudly -- the int-returning
 * ones with IGD_HIP_ERR_DEVICE, igd_hip_last_error() with dlopen's reason -- and the callers report it like any other
 * engine failure ("no CPU search path").
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "igd_hip.h"

static void *g_lib = NULL;
static char g_why[600] = "";
static pthread_once_t g_once = PTHREAD_ONCE_INIT;

static void load_engine(void)
{
    Dl_info di;
    char path[4096];
    path[0] = 0;
    if (dladdr((void *)load_engine, &di) && di.dli_fname) {
        const char *slash = strrchr(di.dli_fname, '/');
        if (slash && (size_t)(slash - di.dli_fname) + 32 < sizeof path) {
            memcpy(path, di.dli_fname, (size_t)(slash - di.dli_fname) + 1);
            strcpy(path + (slash - di.dli_fname) + 1, "libigd_hip.so");
        }
    }
    if (path[0]) g_lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!g_lib) {
        const char *e1 = dlerror();
        snprintf(g_why, sizeof g_why, "the HIP engine library could not be loaded (%s)", e1 ? e1 : path);
        g_lib = dlopen("libigd_hip.so", RTLD_NOW | RTLD_LOCAL);      /* the loader's search path (LD_LIBRARY_PATH, rpath) */
    }
}

static void *engine_sym(const char *name)
{
    pthread_once(&g_once, load_engine);
    return g_lib ? dlsym(g_lib, name) : NULL;
}

/* the engine is mapped already?  (the command line tool leaves through _exit() only when it is: igd_main.c) */
int igd_hip_lazy_loaded(void) { return g_lib != NULL; }

/* `fn`, the engine's function of this name, or NULL: its type is the header's declaration of `name` (include/igd_hip.h) and the
 * symbol looked up is the same identifier, so neither can drift from the trampoline that forwards to it -- the compiler holds
 * the trampoline's definition, the forwarded call and the header against each other */
#define RESOLVE(name)                                     \
    static __typeof__(&name) fn = NULL;                   \
    if (!fn) fn = (__typeof__(&name))engine_sym(#name)

const char *igd_hip_last_error(void)
{
    RESOLVE(igd_hip_last_error);
    return fn ? fn() : g_why;
}

void igd_hip_set_error_(const char *msg)
{
    RESOLVE(igd_hip_set_error_);
    if (fn) fn(msg);
}

int igd_hip_device_count(void)
{
    RESOLVE(igd_hip_device_count);
    return fn ? fn() : 0;
}

/* Answered here, without mapping the engine: a small `search -q -f` asks for the step of its loop before it knows that the
 * host path takes the file (the question alone cost the 13 ms this file exists to avoid).  Same rule as the
 * engine's max_batch(): 2^24 queries, lowered by the TEST-ONLY variable IGD_HIP_MAX_BATCH. */
int64_t igd_hip_max_batch(void)
{
    return igd_hip_max_batch_rule(getenv("IGD_HIP_MAX_BATCH"));    /* (include/igd_hip.h: the one definition) */
}

int igd_hip_open(const igd_hip_desc *desc, int device, igd_hip_db **out)
{
    RESOLVE(igd_hip_open);
    return fn ? fn(desc, device, out) : IGD_HIP_ERR_DEVICE;
}

void igd_hip_close(igd_hip_db *db)
{
    if (!db) return;                                   /* closing nothing must not map the engine */
    RESOLVE(igd_hip_close);
    if (fn) fn(db);
}

int32_t igd_hip_nfiles(const igd_hip_db *db)
{
    if (!db) return 0;
    RESOLVE(igd_hip_nfiles);
    return fn ? fn(db) : 0;
}

int igd_hip_search(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t v, int rule,
                   int64_t *hits, int64_t *total)
{
    RESOLVE(igd_hip_search);
    return fn ? fn(db, ichr, qs, qe, nq, v, rule, hits, total) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_search_ex(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t v, int rule,
                      int flags, int64_t *hits, int64_t *total)
{
    RESOLVE(igd_hip_search_ex);
    return fn ? fn(db, ichr, qs, qe, nq, v, rule, flags, hits, total) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_search_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                        int32_t v, int rule, int flags, int64_t *hits, int64_t *totals)
{
    RESOLVE(igd_hip_search_sets);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, v, rule, flags, hits, totals) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_support_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                         int32_t v, int rule, int64_t *support, int64_t *nhit)
{
    RESOLVE(igd_hip_support_sets);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, v, rule, support, nhit) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_search_sets_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                           int32_t v, int rule, int flags, int64_t *hits, int64_t *totals, const igd_hip_min_overlap *min_overlap)
{
    RESOLVE(igd_hip_search_sets_ov);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, v, rule, flags, hits, totals, min_overlap) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_support_sets_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                            int32_t v, int rule, int64_t *support, int64_t *nhit, const igd_hip_min_overlap *min_overlap)
{
    RESOLVE(igd_hip_support_sets_ov);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, v, rule, support, nhit, min_overlap) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_coverage_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                          int32_t v, int rule, int64_t *coverage, int64_t *covered)
{
    RESOLVE(igd_hip_coverage_sets);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, v, rule, coverage, covered) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_merge_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                       int64_t gap, int32_t *m_ichr, int32_t *m_qs, int32_t *m_qe, int64_t *m_off, int32_t *m_count, int64_t *n_dropped)
{
    RESOLVE(igd_hip_merge_sets);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, gap, m_ichr, m_qs, m_qe, m_off, m_count, n_dropped) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_merge_sets_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, const int64_t *d_set_off,
                           int32_t nsets, int64_t n, int64_t gap, int32_t *d_m_ichr, int32_t *d_m_qs, int32_t *d_m_qe, int64_t *d_m_off,
                           int32_t *d_m_count, int64_t *d_n_dropped, void *stream)
{
    RESOLVE(igd_hip_merge_sets_dev);
    return fn ? fn(db, d_ichr, d_qs, d_qe, d_set_off, nsets, n, gap, d_m_ichr, d_m_qs, d_m_qe, d_m_off, d_m_count, d_n_dropped, stream)
              : IGD_HIP_ERR_DEVICE;
}

int igd_hip_dataset_bp(igd_hip_db *db, int32_t v, int rule, int64_t *file_bp)
{
    RESOLVE(igd_hip_dataset_bp);
    return fn ? fn(db, v, rule, file_bp) : IGD_HIP_ERR_DEVICE;
}

int64_t igd_hip_dataset_bp_computed(const igd_hip_db *db)
{
    if (!db) return 0;
    RESOLVE(igd_hip_dataset_bp_computed);
    return fn ? fn(db) : 0;
}

int igd_hip_jaccard_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                         int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *file_bp, int64_t *n_merged, int64_t *n_dropped)
{
    RESOLVE(igd_hip_jaccard_sets);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, v, rule, inter, set_bp, file_bp, n_merged, n_dropped) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_bp(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                       int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged,
                       int64_t *n_dropped)
{
    RESOLVE(igd_hip_permute_bp);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, inter, set_bp, n_merged, n_dropped) : IGD_HIP_ERR_DEVICE;
}

int64_t igd_hip_merge_slices_per_row(int64_t pc, int64_t nq)
{
    RESOLVE(igd_hip_merge_slices_per_row);
    return fn ? fn(pc, nq) : 0;
}

int64_t igd_hip_member_words(const igd_hip_db *db)
{
    if (!db) return 0;
    RESOLVE(igd_hip_member_words);
    return fn ? fn(db) : 0;
}

int32_t igd_hip_member_grid(int64_t nq)
{
    RESOLVE(igd_hip_member_grid);
    return fn ? fn(nq) : 0;
}

int igd_hip_membership(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t v, int rule,
                       uint32_t *bits, int32_t *nfiles_hit, int64_t *nhit)
{
    RESOLVE(igd_hip_membership);
    return fn ? fn(db, ichr, qs, qe, nq, v, rule, bits, nfiles_hit, nhit) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_membership_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq, int32_t v,
                           int rule, uint32_t *d_bits, int32_t *d_nfiles_hit, int64_t *d_nhit, void *stream)
{
    RESOLVE(igd_hip_membership_dev);
    return fn ? fn(db, d_ichr, d_qs, d_qe, nq, v, rule, d_bits, d_nfiles_hit, d_nhit, stream) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_nearest(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t window, int32_t v,
                    int32_t *dist, int32_t *dmin)
{
    RESOLVE(igd_hip_nearest);
    return fn ? fn(db, ichr, qs, qe, nq, window, v, dist, dmin) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_nearest_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                         int32_t nsets, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist)
{
    RESOLVE(igd_hip_nearest_sets);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, window, v, n_within, n_overlap, sum_dist) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_nearest_hist(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                         int32_t nsets, int32_t window, int32_t v, const int32_t *edges, int32_t ne, int64_t *hist)
{
    RESOLVE(igd_hip_nearest_hist);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, window, v, edges, ne, hist) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_flank_reldist(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                          int32_t nsets, int32_t window, int measure, int32_t v, int32_t nbins, int64_t *hist)
{
    RESOLVE(igd_hip_flank_reldist);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, window, measure, v, nbins, hist) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_map(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int op, int32_t v, int32_t *count,
                int64_t *agg)
{
    RESOLVE(igd_hip_map);
    return fn ? fn(db, ichr, qs, qe, nq, op, v, count, agg) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_map_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                     int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    RESOLVE(igd_hip_map_sets);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, op, v, n_hit, pairs, agg_sum) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_enrich_sets_nhit(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                             int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu, int32_t v, int rule,
                             int64_t *support, int64_t *usupport, double *pvalue_log, double *odds_ratio, int64_t *clamped, int64_t *nhit,
                             int64_t *unhit)
{
    RESOLVE(igd_hip_enrich_sets_nhit);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, v, rule, support, usupport, pvalue_log, odds_ratio, clamped,
                   nhit, unhit)
              : IGD_HIP_ERR_DEVICE;
}

int igd_hip_enrich_sets_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                           int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu, int32_t v, int rule,
                           int64_t *support, int64_t *usupport, double *pvalue_log, double *odds_ratio, int64_t *clamped, int64_t *nhit,
                           int64_t *unhit, const igd_hip_min_overlap *min_overlap)
{
    RESOLVE(igd_hip_enrich_sets_ov);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, v, rule, support, usupport, pvalue_log, odds_ratio, clamped,
                   nhit, unhit, min_overlap)
              : IGD_HIP_ERR_DEVICE;
}

int igd_hip_group_support_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                               int32_t nsets, const int32_t *grp_off, const int32_t *grp_idx, int32_t ngroups, int32_t v, int rule,
                               int64_t *gsupport, int64_t *gnhit, const igd_hip_min_overlap *min_overlap)
{
    RESOLVE(igd_hip_group_support_sets);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, grp_off, grp_idx, ngroups, v, rule, gsupport, gnhit, min_overlap) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_group_enrich_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                              int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu,
                              const int32_t *grp_off, const int32_t *grp_idx, int32_t ngroups, int32_t v, int rule, int64_t *gsupport,
                              int64_t *gusupport, double *pvalue_log, double *odds_ratio, int64_t *clamped, int64_t *gnhit,
                              int64_t *gunhit, const igd_hip_min_overlap *min_overlap)
{
    RESOLVE(igd_hip_group_enrich_sets);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, grp_off, grp_idx, ngroups, v, rule, gsupport, gusupport,
                   pvalue_log, odds_ratio, clamped, gnhit, gunhit, min_overlap)
              : IGD_HIP_ERR_DEVICE;
}

int igd_hip_restrict_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                          int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu, uint32_t *bits,
                          int64_t *size)
{
    RESOLVE(igd_hip_restrict_sets);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, bits, size) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_enrich_restricted(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                              int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu, int32_t v, int rule,
                              int64_t *support, int64_t *usupport, int64_t *size, double *pvalue_log, double *odds_ratio, uint32_t *bits,
                              int64_t *nhit, int64_t *unhit)
{
    RESOLVE(igd_hip_enrich_restricted);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, v, rule, support, usupport, size, pvalue_log, odds_ratio,
                   bits, nhit, unhit)
              : IGD_HIP_ERR_DEVICE;
}

int32_t igd_hip_restrict_grid(int64_t nregions)
{
    RESOLVE(igd_hip_restrict_grid);
    return fn ? fn(nregions) : 0;
}

int igd_hip_enrich_ranks(igd_hip_db *db, const int64_t *support, const double *pvalue_log, const double *odds_ratio, int64_t nrows,
                         int64_t ncols, double *qvalue_log, int32_t *rnk_sup, int32_t *rnk_pv, int32_t *rnk_or, int32_t *max_rnk,
                         double *mean_rnk)
{
    RESOLVE(igd_hip_enrich_ranks);
    return fn ? fn(db, support, pvalue_log, odds_ratio, nrows, ncols, qvalue_log, rnk_sup, rnk_pv, rnk_or, max_rnk, mean_rnk)
              : IGD_HIP_ERR_DEVICE;
}

int32_t igd_hip_rank_grid(int64_t nrows)
{
    RESOLVE(igd_hip_rank_grid);
    return fn ? fn(nrows) : 0;
}

int32_t igd_hip_rank_lds_cols(void)
{
    RESOLVE(igd_hip_rank_lds_cols);
    return fn ? fn() : 0;
}

int igd_hip_cooccur(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t v, int rule,
                    int64_t *cooc, int64_t *nhit)
{
    RESOLVE(igd_hip_cooccur);
    return fn ? fn(db, ichr, qs, qe, nq, v, rule, cooc, nhit) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_bits_transpose(igd_hip_db *db, const uint32_t *bits, int64_t nrows, int64_t nW, uint64_t *cols)
{
    RESOLVE(igd_hip_bits_transpose);
    return fn ? fn(db, bits, nrows, nW, cols) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_bitrows_gram(igd_hip_db *db, const uint32_t *a, int64_t m, const uint32_t *b, int64_t n, int64_t nwords32, int64_t *out)
{
    RESOLVE(igd_hip_bitrows_gram);
    return fn ? fn(db, a, m, b, n, nwords32, out) : IGD_HIP_ERR_DEVICE;
}

int32_t igd_hip_gram_tile(void)
{
    RESOLVE(igd_hip_gram_tile);
    return fn ? fn() : 0;
}

int32_t igd_hip_gram_kstep(void)
{
    RESOLVE(igd_hip_gram_kstep);
    return fn ? fn() : 0;
}

int64_t igd_hip_gram_slices(int64_t m, int64_t n, int64_t nwords32)
{
    RESOLVE(igd_hip_gram_slices);
    return fn ? fn(m, n, nwords32) : 0;
}

int igd_hip_permute_support(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                            int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq,
                            int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax)
{
    RESOLVE(igd_hip_permute_support);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_support_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                               int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq,
                               int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax, const igd_hip_min_overlap *min_overlap)
{
    RESOLVE(igd_hip_permute_support_ov);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax, min_overlap)
              : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_regions(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                            int32_t nctg, int mode, uint64_t seed, int64_t p0, int64_t np, int32_t *out_qs, int32_t *out_qe)
{
    RESOLVE(igd_hip_permute_regions);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, nctg, mode, seed, p0, np, out_qs, out_qe) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_perm_stats(igd_hip_db *db, const int64_t *rows, int64_t nrows, int64_t ncols, const int64_t *observed, int64_t *sum,
                       int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax)
{
    RESOLVE(igd_hip_perm_stats);
    return fn ? fn(db, rows, nrows, ncols, observed, sum, sumsq, n_ge, n_le, pmin, pmax) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_nearest_sets_fused(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                               int32_t nsets, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist)
{
    RESOLVE(igd_hip_nearest_sets_fused);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, window, v, n_within, n_overlap, sum_dist) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_nearest(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                            int mode, uint64_t seed, int64_t nperm, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap,
                            int64_t *sum_dist)
{
    RESOLVE(igd_hip_permute_nearest);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, window, v, n_within, n_overlap, sum_dist) : IGD_HIP_ERR_DEVICE;
}

int32_t igd_hip_nearest_fused_max_files(void)
{
    RESOLVE(igd_hip_nearest_fused_max_files);
    return fn ? fn() : 0;
}

int32_t igd_hip_nearest_fused_grid(int64_t nslices)
{
    RESOLVE(igd_hip_nearest_fused_grid);
    return fn ? fn(nslices) : 0;
}

int32_t igd_hip_permute_grid(int64_t n)
{
    RESOLVE(igd_hip_permute_grid);
    return fn ? fn(n) : 0;
}

int igd_hip_permute_regions_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                               int32_t nctg, int mode, uint64_t seed, int64_t p0, int64_t np, int32_t *out_qs, int32_t *out_qe,
                               const igd_hip_workspace *ws)
{
    RESOLVE(igd_hip_permute_regions_ws);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, nctg, mode, seed, p0, np, out_qs, out_qe, ws) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_support_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                               int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq,
                               int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax, const igd_hip_min_overlap *min_overlap,
                               const igd_hip_workspace *ws)
{
    RESOLVE(igd_hip_permute_support_ws);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax, min_overlap, ws)
              : IGD_HIP_ERR_DEVICE;
}

int igd_hip_shift_regions(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                          int32_t nctg, const int32_t *offsets, int64_t nshift, int32_t *out_qs, int32_t *out_qe)
{
    RESOLVE(igd_hip_shift_regions);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, nctg, offsets, nshift, out_qs, out_qe) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_shift_support(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                          const int32_t *offsets, int64_t nshift, int32_t v, int rule, int64_t *shifted,
                          const igd_hip_min_overlap *min_overlap)
{
    RESOLVE(igd_hip_shift_support);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, offsets, nshift, v, rule, shifted, min_overlap) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_nearest_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                               int mode, uint64_t seed, int64_t nperm, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap,
                               int64_t *sum_dist, const igd_hip_workspace *ws)
{
    RESOLVE(igd_hip_permute_nearest_ws);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, window, v, n_within, n_overlap, sum_dist, ws) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_bp_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                          int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged,
                          int64_t *n_dropped, const igd_hip_workspace *ws)
{
    RESOLVE(igd_hip_permute_bp_ws);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, inter, set_bp, n_merged, n_dropped, ws) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_resample_regions(igd_hip_db *db, const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool,
                             int64_t nq, uint64_t seed, int64_t p0, int64_t np, int32_t *out_ichr, int32_t *out_qs, int32_t *out_qe)
{
    RESOLVE(igd_hip_resample_regions);
    return fn ? fn(db, pool_ichr, pool_qs, pool_qe, npool, nq, seed, p0, np, out_ichr, out_qs, out_qe) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_support_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                               int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq, int64_t *n_ge,
                               int64_t *n_le, int64_t *pmin, int64_t *pmax, const igd_hip_min_overlap *min_overlap)
{
    RESOLVE(igd_hip_permute_support_rs);
    return fn ? fn(db, ichr, qs, qe, nq, pool_ichr, pool_qs, pool_qe, npool, seed, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax,
                   min_overlap)
              : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_nearest_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                               int64_t nperm, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist)
{
    RESOLVE(igd_hip_permute_nearest_rs);
    return fn ? fn(db, ichr, qs, qe, nq, pool_ichr, pool_qs, pool_qe, npool, seed, nperm, window, v, n_within, n_overlap, sum_dist)
              : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_bp_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                          const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                          int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged, int64_t *n_dropped)
{
    RESOLVE(igd_hip_permute_bp_rs);
    return fn ? fn(db, ichr, qs, qe, nq, pool_ichr, pool_qs, pool_qe, npool, seed, nperm, v, rule, inter, set_bp, n_merged, n_dropped)
              : IGD_HIP_ERR_DEVICE;
}

int igd_hip_map_sets_fused(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                           int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    RESOLVE(igd_hip_map_sets_fused);
    return fn ? fn(db, ichr, qs, qe, set_off, nsets, op, v, n_hit, pairs, agg_sum) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_map(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                        int mode, uint64_t seed, int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    return igd_hip_permute_map_ws(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, op, v, n_hit, pairs, agg_sum, NULL);
}

int igd_hip_permute_map_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                           int mode, uint64_t seed, int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum,
                           const igd_hip_workspace *ws)
{
    RESOLVE(igd_hip_permute_map_ws);
    return fn ? fn(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, op, v, n_hit, pairs, agg_sum, ws) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_permute_map_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                           const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                           int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    RESOLVE(igd_hip_permute_map_rs);
    return fn ? fn(db, ichr, qs, qe, nq, pool_ichr, pool_qs, pool_qe, npool, seed, nperm, op, v, n_hit, pairs, agg_sum) : IGD_HIP_ERR_DEVICE;
}

int32_t igd_hip_map_fused_max_files(int op)
{
    RESOLVE(igd_hip_map_fused_max_files);
    return fn ? fn(op) : 0;
}

int32_t igd_hip_map_fused_grid(int64_t nslices)
{
    RESOLVE(igd_hip_map_fused_grid);
    return fn ? fn(nslices) : 0;
}

int igd_hip_enumerate_stream(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int64_t *qoff,
                             igd_hip_enum_sink sink, void *ctx, int64_t *total)
{
    RESOLVE(igd_hip_enumerate_stream);
    return fn ? fn(db, ichr, qs, qe, nq, qoff, sink, ctx, total) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_enumerate_stream8(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int64_t *qoff,
                              igd_hip_enum_sink8 sink, void *ctx, int64_t *total)
{
    RESOLVE(igd_hip_enumerate_stream8);
    return fn ? fn(db, ichr, qs, qe, nq, qoff, sink, ctx, total) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_hit8_idx_bits(igd_hip_db *db)
{
    if (!db) return -1;
    RESOLVE(igd_hip_hit8_idx_bits);
    return fn ? fn(db) : -1;
}

int igd_hip_hitmap(igd_hip_db *db, int use_v, int32_t v, uint32_t *hitmap, int64_t *total)
{
    RESOLVE(igd_hip_hitmap);
    return fn ? fn(db, use_v, v, hitmap, total) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_seqpare_add(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *qgroup,
                        int32_t nGroups, double *sums)
{
    RESOLVE(igd_hip_seqpare_add);
    return fn ? fn(db, ichr, qs, qe, nq, qgroup, nGroups, sums) : IGD_HIP_ERR_DEVICE;
}

int igd_hip_create(const igd_hip_create_desc *d, int device, igd_hip_created *out)
{
    RESOLVE(igd_hip_create);
    return fn ? fn(d, device, out) : IGD_HIP_ERR_DEVICE;
}

void igd_hip_created_free(igd_hip_created *c)
{
    RESOLVE(igd_hip_created_free);
    if (fn) fn(c);
}

int igd_hip_group_create(igd_hip_db *const *dbs, int n, igd_hip_group **out)
{
    RESOLVE(igd_hip_group_create);
    return fn ? fn(dbs, n, out) : IGD_HIP_ERR_DEVICE;
}

void igd_hip_group_destroy(igd_hip_group *g)
{
    if (!g) return;
    RESOLVE(igd_hip_group_destroy);
    if (fn) fn(g);
}

const char *igd_hip_group_reduce_kind(const igd_hip_group *g)
{
    RESOLVE(igd_hip_group_reduce_kind);
    return fn ? fn(g) : "";
}

const char *igd_hip_group_reduce_note(const igd_hip_group *g)
{
    RESOLVE(igd_hip_group_reduce_note);
    return fn ? fn(g) : "";
}

int igd_hip_group_search(igd_hip_group *g, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t v, int rule,
                         int flags, int64_t *hits, int64_t *total)
{
    RESOLVE(igd_hip_group_search);
    return fn ? fn(g, ichr, qs, qe, nq, v, rule, flags, hits, total) : IGD_HIP_ERR_DEVICE;
}

/* TEST-ONLY accessors (include/igd_hip.h): a caller that links a host flavour reads the last batch's routes through these */
int igd_hip_last_batch_routes(igd_hip_db *db, int64_t *out, int n)
{
    if (!db) return 0;
    RESOLVE(igd_hip_last_batch_routes);
    return fn ? fn(db, out, n) : 0;
}

int igd_hip_route_constants(igd_hip_db *db, int64_t *out, int n)
{
    if (!db) return 0;
    RESOLVE(igd_hip_route_constants);
    return fn ? fn(db, out, n) : 0;
}
