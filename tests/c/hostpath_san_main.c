/* hostpath_san_main.c -- harness for tests/test_hostpath_io_host.py: every entry of the host route (igd_hostpath.c) once on a
 * small database, a short run of each permutation driver, and at the end the same database after its file has been cut to
 * nothing under the open map (every tile read fails: the entries must answer -1 and free what they hold).  Compiled with
 * igd_core.c, igd_hostpath.c and igd_hip_lazy.c under the host sanitizers; needs no engine library.
 * usage: hostpath_san <db.igd (a copy: it is truncated)>   -> prints "hostpath_san ok <digest>", the same for any thread count */
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "igd_core.h"

static unsigned long long H = 1469598103934665603ULL;
static void mix(const void *p, size_t bytes)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < bytes; i++) H = (H ^ b[i]) * 1099511628211ULL;
}
static int fails = 0;
#define WANT(rc, call) do { if ((call) != (rc)) { fprintf(stderr, "line %d: %s did not answer %d\n", __LINE__, #call, rc); fails++; } } while (0)

enum { NQ = 9000, NP = 600, NPOOL = NP + 7, NPERM = 30, NSETS = 6, LEN = 1 << 30 };

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    igdc_db *db = igdc_open(argv[1]);
    if (!db) return 3;
    char *tsv = igdc_index_path(argv[1]);
    igdc_load_index(db, tsv);
    free(tsv);
    const int fd = open(argv[1], O_RDONLY);
    igdc_map *m = fd >= 0 ? igdc_map_open(db, fd) : NULL;
    if (fd >= 0) close(fd);
    if (!m) return 4;
    const int64_t nf = db->nFiles, nC = nf + 1, nW = (nf + 31) / 32;

    /* regions: whole contigs, short ones, an inverted one, unknown contigs; NQ is enough for five threads */
    int32_t *ichr = malloc(sizeof(int32_t) * NQ), *qs = malloc(sizeof(int32_t) * NQ), *qe = malloc(sizeof(int32_t) * NQ);
    uint64_t x = 88172645463325252ULL;
    for (int i = 0; i < NQ; i++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        ichr[i] = (int32_t)(x % 10) - 1;                        /* -1 .. 8 */
        qs[i] = i % 16 == 0 ? 0 : (int32_t)((x >> 8) % 3000000);
        qe[i] = i % 16 == 0 ? LEN : qs[i] + (int32_t)((x >> 40) % 50000) - 5;
    }
    const int64_t set_off[NSETS + 1] = {0, 0, 3000, 3000, 7000, NQ, NQ};
    const igd_hip_min_overlap mo = {5, 100000, 0};
    int64_t *a64 = calloc((size_t)(NQ * (nf + 1) + 64 * nC * NSETS + nf * nf + (NPERM + 1) * nC * 3), sizeof(int64_t)), tot = 0;
    int32_t *a32 = calloc((size_t)(2 * NQ * (nf + nW + 1) + 4 * NQ), sizeof(int32_t)), *b32 = a32 + NQ * (nf + nW + 1), *c32 = b32 + NQ * (nf + nW + 1);
    double *f64 = calloc((size_t)(2 * NSETS * nf + 1), sizeof(double));
#define MIX64(n) mix(a64, sizeof(int64_t) * (size_t)(n))

    for (int rule = 0; rule < 2; rule++) {
        const int32_t v = rule ? 300 : IGD_HIP_NO_VALUE_FILTER;
        WANT(0, igdc_search_host(db, m, ichr, qs, qe, NQ, v, rule, a64, &tot)); MIX64(nf); mix(&tot, 8);
        WANT(0, igdc_search_host_ov(db, m, ichr, qs, qe, NQ, v, rule, a64, &tot, &mo)); MIX64(nf); mix(&tot, 8);
        WANT(0, igdc_support_host(db, m, ichr, qs, qe, NQ, v, rule, a64, &tot)); MIX64(nf); mix(&tot, 8);
        WANT(0, igdc_support_host_ov(db, m, ichr, qs, qe, NQ, v, rule, a64, &tot, &mo)); MIX64(nf); mix(&tot, 8);
        WANT(0, igdc_coverage_host(db, m, ichr, qs, qe, NQ, v, rule, a64, &tot)); MIX64(nf); mix(&tot, 8);
        WANT(0, igdc_membership_host(db, m, ichr, qs, qe, NQ, v, rule, (uint32_t *)a32, c32, &tot)); mix(a32, 4 * (size_t)(NQ * nW)); mix(c32, 4 * NQ);
        WANT(0, igdc_cooccur_host(db, m, ichr, qs, qe, NQ, v, rule, a64, &tot)); MIX64(nf * nf);
        WANT(0, igdc_dataset_bp_host(db, m, v, rule, a64)); MIX64(nC);
        WANT(0, igdc_jaccard_host(db, m, ichr, qs, qe, set_off, NSETS, v, rule, a64, a64 + NSETS * nC, a64 + (NSETS + 1) * nC, a64 + (NSETS + 2) * nC,
                                  a64 + (NSETS + 3) * nC + NSETS));
        MIX64(NSETS * nC);
        WANT(0, igdc_enrich_restricted_host(db, m, ichr, qs, qe, set_off, NSETS, ichr, qs, qe, NQ, v, rule, a64, a64 + NSETS * nf, a64 + (NSETS + 1) * nf,
                                            f64, f64 + NSETS * nf, NULL, NULL, &tot));
        MIX64(NSETS * nf); mix(f64, 8 * (size_t)(NSETS * nf));
    }
    {
        int64_t *qoff = malloc(sizeof(int64_t) * (NQ + 1));
        igd_hip_hit *out = NULL;
        WANT(0, igdc_enumerate_host(db, m, ichr, qs, qe, NQ, qoff, &out, &tot));
        mix(qoff, 8 * (NQ + 1)); mix(out, sizeof(igd_hip_hit) * (size_t)tot);
        free(out); free(qoff);
    }
    const int32_t edges[3] = {-1000, 0, 1000};
    for (int32_t window = 0; window <= 20000; window += 20000) {
        WANT(0, igdc_nearest_host(db, m, ichr, qs, qe, NQ, window, IGD_HIP_NO_VALUE_FILTER, a32, c32)); mix(a32, 4 * (size_t)(NQ * nf)); mix(c32, 4 * NQ);
        WANT(0, igdc_nearest_signed_host(db, m, ichr, qs, qe, NQ, window, 300, a32, c32)); mix(a32, 4 * (size_t)(NQ * nf)); mix(c32, 4 * NQ);
        WANT(0, igdc_nearest_sets_host(db, m, ichr, qs, qe, set_off, NSETS, window, 300, a64, a64 + NSETS * nC, a64 + 2 * NSETS * nC)); MIX64(3 * NSETS * nC);
        WANT(0, igdc_nearest_hist_host(db, m, ichr, qs, qe, set_off, NSETS, window, IGD_HIP_NO_VALUE_FILTER, edges, 3, a64)); MIX64(4 * NSETS * nC);
        for (int measure = 0; measure < 2; measure++) {
            WANT(0, igdc_flank_host(db, m, ichr, qs, qe, NQ, window, measure, IGD_HIP_NO_VALUE_FILTER, a32, b32, c32, c32 + NQ));
            mix(a32, 4 * (size_t)(NQ * nf)); mix(b32, 4 * (size_t)(NQ * nf)); mix(c32, 8 * NQ);
            WANT(0, igdc_flank_reldist_host(db, m, ichr, qs, qe, set_off, NSETS, window, measure, IGD_HIP_NO_VALUE_FILTER, 10, a64)); MIX64(10 * NSETS * nC);
        }
    }
    for (int op = 0; op < 4; op++) {
        WANT(0, igdc_map_host(db, m, ichr, qs, qe, NQ, op, IGD_HIP_NO_VALUE_FILTER, a32, a64)); mix(a32, 4 * (size_t)(NQ * nf)); MIX64(NQ * nf);
        WANT(0, igdc_map_sets_host(db, m, ichr, qs, qe, set_off, NSETS, op, 300, a64, a64 + NSETS * nf, a64 + 2 * NSETS * nf)); MIX64(3 * NSETS * nf);
    }
    {
        int32_t *mr = malloc(sizeof(int32_t) * 4 * NQ);
        int64_t moff[NSETS + 1], dropped[NSETS];
        WANT(0, igdc_merge_host(db, ichr, qs, qe, set_off, NSETS, 100, mr, mr + NQ, mr + 2 * NQ, moff, mr + 3 * NQ, dropped));
        mix(mr, 16 * NQ); mix(moff, sizeof moff); mix(dropped, sizeof dropped);
        free(mr);
        WANT(0, igdc_bitrows_gram_host((const uint32_t *)ichr, 300, NULL, 0, 30, a64)); MIX64(300 * 300 <= NQ * (nf + 1) ? 300 * 300 : 0);
    }

    /* the permutation drivers: NP regions inside their contigs, both free placements and a workspace of two segments per contig */
    int32_t ctg_len[64], seg_c[128], seg_a[128], seg_b[128];
    const int32_t nctg = db->nCtg <= 64 ? db->nCtg : 0;
    for (int c = 0; c < 64; c++) {
        ctg_len[c] = 4000000;
        seg_c[2 * c] = seg_c[2 * c + 1] = c;
        seg_a[2 * c] = 0; seg_b[2 * c] = 2000000; seg_a[2 * c + 1] = 2100000; seg_b[2 * c + 1] = 4000000;
    }
    int32_t *ps = malloc(sizeof(int32_t) * NP), *pe = malloc(sizeof(int32_t) * NP), *po = malloc(sizeof(int32_t) * 4 * NP);
    for (int i = 0; i < NP; i++) { ps[i] = qs[i] < 1900000 ? qs[i] : 2100000 + qs[i] % 1000000; pe[i] = ps[i] + 1 + (qs[i] & 1023); }
    igd_hip_workspace *ws = NULL;
    WANT(0, igdc_workspace_build(seg_c, seg_a, seg_b, 2 * nctg, ctg_len, nctg, &ws));
    for (int mode = 0; mode < 3 && nctg > 0; mode++) {
        const igd_hip_workspace *w = mode == IGD_HIP_PERM_WORKSPACE ? ws : NULL;
        WANT(0, igdc_permute_regions_host_ws(ichr, ps, pe, NP, ctg_len, nctg, mode, 5, 0, 2, po, po + 2 * NP, w)); mix(po, 16 * NP);
        WANT(0, igdc_permute_host_ws(db, m, ichr, ps, pe, NP, ctg_len, mode, 5, NPERM, IGD_HIP_NO_VALUE_FILTER, mode & 1, a64, a64 + nC, a64 + 2 * nC,
                                     a64 + 3 * nC, a64 + 4 * nC, a64 + 5 * nC, a64 + 6 * nC, mode ? &mo : NULL, w));
        MIX64(7 * nC);
        WANT(0, igdc_permute_nearest_host_ws(db, m, ichr, ps, pe, NP, ctg_len, mode, 5, NPERM, 5000, IGD_HIP_NO_VALUE_FILTER, a64, a64 + (NPERM + 1) * nC,
                                             a64 + 2 * (NPERM + 1) * nC, w));
        MIX64(3 * (NPERM + 1) * nC);
        WANT(0, igdc_permute_bp_host_ws(db, m, ichr, ps, pe, NP, ctg_len, mode, 5, NPERM, 300, 1, a64, a64 + (NPERM + 1) * nC, a64 + (NPERM + 1) * nC + 64,
                                        &tot, w));
        MIX64((NPERM + 1) * nC);
        WANT(0, igdc_permute_map_host_ws(db, m, ichr, ps, pe, NP, ctg_len, mode, 5, NPERM, mode + 1, 300, a64, a64 + (NPERM + 1) * nf,
                                         a64 + 2 * (NPERM + 1) * nf, w));
        MIX64(3 * (NPERM + 1) * nf);
    }
    /* the same four nulls by resampling: draws of NP regions from a pool a few regions larger (the first NPOOL regions above,
     * unknown contigs and the inverted region included: a draw is copied as it stands), and the generator alone */
    WANT(0, igdc_resample_regions_host(ichr, qs, qe, NPOOL, NP, 5, 0, 1, po, po + NP, po + 2 * NP)); mix(po, 12 * NP);
    WANT(0, igdc_permute_host_rs(db, m, ichr, ps, pe, NP, ichr, qs, qe, NPOOL, 5, NPERM, IGD_HIP_NO_VALUE_FILTER, 1, a64, a64 + nC, a64 + 2 * nC,
                                 a64 + 3 * nC, a64 + 4 * nC, a64 + 5 * nC, a64 + 6 * nC, &mo));
    MIX64(7 * nC);
    WANT(0, igdc_permute_nearest_host_rs(db, m, ichr, ps, pe, NP, ichr, qs, qe, NPOOL, 5, NPERM, 5000, 300, a64, a64 + (NPERM + 1) * nC,
                                         a64 + 2 * (NPERM + 1) * nC));
    MIX64(3 * (NPERM + 1) * nC);
    WANT(0, igdc_permute_bp_host_rs(db, m, ichr, ps, pe, NP, ichr, qs, qe, NPOOL, 5, NPERM, IGD_HIP_NO_VALUE_FILTER, 0, a64, a64 + (NPERM + 1) * nC,
                                    a64 + (NPERM + 1) * nC + 64, &tot));
    MIX64((NPERM + 1) * nC + 128); mix(&tot, 8);
    WANT(0, igdc_permute_map_host_rs(db, m, ichr, ps, pe, NP, ichr, qs, qe, NPOOL, 5, NPERM, IGD_HIP_MAP_SUM, IGD_HIP_NO_VALUE_FILTER, a64,
                                     a64 + (NPERM + 1) * nf, a64 + 2 * (NPERM + 1) * nf));
    MIX64(3 * (NPERM + 1) * nf);
    /* the set under NPERM rigid shifts, to both sides and past the contig ends, and the shifted regions alone */
    int32_t offsets[NPERM];
    for (int j = 0; j < NPERM; j++) offsets[j] = (j - NPERM / 2) * 300000;
    if (nctg > 0) {
        WANT(0, igdc_shift_regions_host(ichr, ps, pe, NP, ctg_len, nctg, offsets, 2, po, po + 2 * NP)); mix(po, 16 * NP);
        WANT(0, igdc_shift_support_host_ov(db, m, ichr, ps, pe, NP, ctg_len, offsets, NPERM, 300, 0, a64, &mo)); MIX64(NPERM * nC);
    }

    /* the file is cut under the open map: no tile can be read any more */
    if (truncate(argv[1], 0) != 0) return 5;
    WANT(-1, igdc_search_host(db, m, ichr, qs, qe, NQ, IGD_HIP_NO_VALUE_FILTER, 0, a64, &tot));
    WANT(-1, igdc_coverage_host(db, m, ichr, qs, qe, NQ, IGD_HIP_NO_VALUE_FILTER, 1, a64, &tot));
    WANT(-1, igdc_membership_host(db, m, ichr, qs, qe, NQ, IGD_HIP_NO_VALUE_FILTER, 0, (uint32_t *)a32, c32, &tot));
    {
        int64_t *qoff = malloc(sizeof(int64_t) * (NQ + 1));
        igd_hip_hit *out = NULL;
        WANT(-1, igdc_enumerate_host(db, m, ichr, qs, qe, NQ, qoff, &out, &tot));
        free(qoff);
    }
    WANT(-1, igdc_nearest_sets_host(db, m, ichr, qs, qe, set_off, NSETS, 100, IGD_HIP_NO_VALUE_FILTER, a64, NULL, NULL));
    WANT(-1, igdc_flank_reldist_host(db, m, ichr, qs, qe, set_off, NSETS, 100, 0, IGD_HIP_NO_VALUE_FILTER, 10, a64));
    WANT(-1, igdc_map_sets_host(db, m, ichr, qs, qe, set_off, NSETS, 0, IGD_HIP_NO_VALUE_FILTER, a64, NULL, NULL));
    WANT(-1, igdc_jaccard_host(db, m, ichr, qs, qe, set_off, NSETS, IGD_HIP_NO_VALUE_FILTER, 0, a64, a64 + NSETS * nC, a64 + (NSETS + 1) * nC,
                               a64 + (NSETS + 2) * nC, a64 + (NSETS + 3) * nC + NSETS));
    if (nctg > 0) {
        WANT(-1, igdc_permute_host(db, m, ichr, ps, pe, NP, ctg_len, 1, 5, NPERM, IGD_HIP_NO_VALUE_FILTER, 0, a64, NULL, NULL, NULL, NULL, NULL, NULL));
        WANT(-1, igdc_permute_nearest_host(db, m, ichr, ps, pe, NP, ctg_len, 1, 5, NPERM, 5000, IGD_HIP_NO_VALUE_FILTER, a64, NULL, NULL));
        WANT(-1, igdc_permute_bp_host(db, m, ichr, ps, pe, NP, ctg_len, 0, 5, NPERM, IGD_HIP_NO_VALUE_FILTER, 0, a64, NULL, NULL, NULL));
        WANT(-1, igdc_permute_map_host_rs(db, m, ichr, ps, pe, NP, ichr, qs, qe, NPOOL, 5, NPERM, IGD_HIP_MAP_COUNT, IGD_HIP_NO_VALUE_FILTER, a64, NULL,
                                          NULL));
        WANT(-1, igdc_shift_support_host_ov(db, m, ichr, ps, pe, NP, ctg_len, offsets, NPERM, IGD_HIP_NO_VALUE_FILTER, 0, a64, NULL));
    }

    igdc_workspace_free(ws);
    free(ps); free(pe); free(po);
    free(ichr); free(qs); free(qe); free(a64); free(a32); free(f64);
    igdc_map_close(m);
    igdc_close(db);
    if (fails) return 1;
    printf("hostpath_san ok %llu\n", H);
    return 0;
}
