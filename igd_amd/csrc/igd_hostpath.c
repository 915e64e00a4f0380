/* igd_hostpath.c -- SMALL query files answered on the host (product code; nothing of oracle/ is used or linked).
 *
 * Why this exists.  The reference starts cheaply: get_igdinfo reads the header only (src/igd_base.c:269-323) and
 * get_overlaps freads just the tiles a query touches (src/igd_search.c:469-476), so `igd search -q` on a file of 10^3
 * queries takes it 6 ms.  Bringing up the HIP runtime and uploading the whole tile region costs a fixed ~0.18 s
 *  whatever the file holds -- 30 x the reference's time at 10^3 queries.  The GPU pays off
 * above ~10^5 queries.  So the three flavours' query-FILE entry points (getOverlaps*, search_n, `-q`, `-f`) count
 * files of at most igdc_host_limit() queries here, like the single-interval entry points already do
 * (igdc_walk_one, igd_core.c), and take the engine for everything larger.
 *
 * What this is NOT: a fallback.  The choice depends on the number of queries and the host's thread count
 * (igdc_host_limit: the same file can take different paths on different hosts, with identical output), never on whether
 * a GPU is present; a file above the limit has no CPU path and fails loudly without a usable device (tests/test_host.py),
 * IGD_HOST_MAX_QUERIES=0 sends every file to the engine (all `-m gpu` parity tests run that way), and the engine's
 * own entry points (include/igd_hip.h, igd_amd.Database, bench.py) never come here.
 *
 * Algorithm = the reference's per query (src/igd_search.c:454-534 rule NEST, :623-694 rule FLAT): in every visited
 * tile bisect the start-sorted records for the last one with start < qe (:479-487 / bSearch src/igd_base.c:74-94),
 * walk back from there testing end > qs [&& value >= v] (:489-493), in later tiles stop at the first record that
 * starts before the tile (:510-511).  Tiles are read with pread() into per-thread buffers (igdc_map holds the file
 * descriptor only; the page cache serves repeats), the
 * queries are split into contiguous ranges over a few threads with private hits[] that are added up at the end
 * (hits[] is a sum over queries).
 */
#define _GNU_SOURCE
#include "igd_core.h"

#include <fcntl.h>
#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

/* Where the engine takes over.  The host route exists for SMALL query files -- a search of 10^3 .. 10^5 lines should not pay
 * the accelerator's start-up (HIP runtime + 851 MB through PCIe: 0.18 s at best, 0.4-0.5 s in many runs, LABNOTES R5-3) --
 * not to carry the product's headline workloads on CPU threads.  Round 6: the limit is back at
 * the conservative round-4 value, 25 000 queries per usable thread (<= 400 000), the same as `-f`'s.  Round 5's model
 * (engine F + n * 7 ns against host 0.03 s + n * 0.55 us / T, crossing at ~280 000 * T) assumed the engine route's BEST start-up
 * and threads that scale; on a host where they do not (1.4 us per query whatever T) it sent 2e6-query files to a 2.8 s host
 * route.  With this limit the worst case of the model's error is ~0.1 s either way, and a 10^6-query file -- BASELINE config 2
 * -- is counted by the MI355X.  IGD_HOST_MAX_QUERIES overrides it (0: every file goes to the GPU).  The LIMIT is frozen
 * (the code of this file is not): bench.py times every size on BOTH routes and labels who counted. */
static int64_t host_threads_usable(void)
{
    long t = sysconf(_SC_NPROCESSORS_ONLN);
    if (t > 16) t = 16;
    if (t < 2) t = 2;
    return t;
}
static int64_t host_limit_env(void)
{
    const char *e = getenv("IGD_HOST_MAX_QUERIES");
    if (e && *e) {
        const long long x = atoll(e);
        return x < 0 ? 0 : (int64_t)x;
    }
    return -1;
}
int64_t igdc_host_limit(void)
{
    const int64_t e = host_limit_env();
    if (e >= 0) return e;
    return 25000 * host_threads_usable();
}
int64_t igdc_host_limit_enum(void) { return igdc_host_limit(); }

/* a query file of `bytes` bytes can be expected to hold at most the limit's number of lines (a BED3 line of a human
 * genome is 18-26 bytes; gzip shrinks it about four times): parse it BEFORE the engine is started, then decide */
int igdc_host_probably_small(const char *qfile)
{
    const int64_t lim = igdc_host_limit();
    if (lim <= 0 || !qfile) return 0;
    struct stat st;
    if (stat(qfile, &st) != 0 || !S_ISREG(st.st_mode)) return 0;
    const size_t L = strlen(qfile);
    const int gz = L > 3 && strcmp(qfile + L - 3, ".gz") == 0;
    return (int64_t)st.st_size <= lim * (gz ? 6 : 24);
}

/* The tile region is read with pread into a per-thread buffer that keeps the last tile (position-sorted query files ask
 * for the same tile again and again; the reference keeps one tile too, src/igd_search.c:469-476).  Measured against a
 * read-only mapping of the file: the mapping pays a page fault per touched 4 KiB page -- 49 ms for 10^4 queries on five
 * threads, which contend for the address space's lock -- where one pread per tile pays a system call (8 ms). */
struct igdc_map {
    int fd;
    int64_t bytes;
};

igdc_map *igdc_map_open(const igdc_db *db, int fd)
{
    if (!db || fd < 0) return NULL;
    const int64_t recBytes = db->gType == 0 ? 12 : 16;
    const int64_t need = db->dataOff + recBytes * db->nRecords;
    struct stat st;
    if (fstat(fd, &st) != 0 || (int64_t)st.st_size < need || need <= 0) return NULL;
    igdc_map *m = (igdc_map *)malloc(sizeof *m);
    if (!m) return NULL;
    m->fd = dup(fd);
    m->bytes = need;
    if (m->fd < 0) { free(m); return NULL; }
    return m;
}

void igdc_map_close(igdc_map *m)
{
    if (!m) return;
    close(m->fd);
    free(m);
}

typedef struct { int32_t *buf; size_t cap; int32_t ichr, tile; int failed; } tilebuf;
static const int32_t *tile_records(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t j, int32_t cnt)
{
    if (tb->ichr == ichr && tb->tile == j) return tb->buf;
    const size_t bytes = (size_t)cnt * (db->gType == 0 ? 12u : 16u);
    if (bytes > tb->cap) {
        free(tb->buf);
        tb->cap = bytes + bytes / 2 + 4096;
        tb->buf = (int32_t *)malloc(tb->cap);
        if (!tb->buf) { tb->cap = 0; tb->failed = 1; tb->ichr = -1; return NULL; }
    }
    size_t done = 0;
    const int64_t off = igdc_tile_off(db, ichr, j);
    while (done < bytes) {
        const ssize_t got = pread(m->fd, (char *)tb->buf + done, bytes - done, (off_t)(off + (int64_t)done));
        if (got <= 0) { tb->failed = 1; tb->ichr = -1; return NULL; }
        done += (size_t)got;
    }
    tb->ichr = ichr; tb->tile = j;
    return tb->buf;
}

/* number of records of a start-sorted tile with start < qe (the reference's bisections, :479-487, bSearch) */
static inline int32_t below(const int32_t *rec, int w, int32_t cnt, int32_t qe)
{
    int32_t lo = 0, hi = cnt;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (rec[(size_t)mid * (size_t)w + 1] < qe) lo = mid + 1; else hi = mid;
    }
    return lo;
}

/* a worker's tile buffer: opened empty; closing frees it and reports whether a tile could not be read */
static void tb_open(tilebuf *tb)
{
    memset(tb, 0, sizeof *tb);
    tb->ichr = -1;
}
static int tb_close(tilebuf *tb)
{
    free(tb->buf);
    tb->buf = NULL;
    return tb->failed;
}

/* ---- THE tile walk: the one place that knows how the reference visits the tiles of an interval -----------------------------
 * The tiles of [lo, hi) on contig ichr, and in each the COUNTED records: start < hi (the bisection), end > lo, value >= v under
 * a filter, a dataset number the database has (the reference indexes hits[] unchecked, :491), and in a tile after the first
 * only records that start inside the tile (the prefix skip, :510-511: the others were met in an earlier tile).  WALK_BACK
 * scans each tile down from the bisection, as the reference does (:489-493, :522-526); WALK_FORWARD scans the same records
 * up from the prefix skip, so that they come in non-decreasing start order over the whole walk.  nest is rule NEST's exit on
 * an empty first tile (:468).  On a tile that cannot be read the walk stops with tb->failed set and answers 0; otherwise 1.
 * What is done with a counted record is the visitor's business.  The walker is forced inline and every caller passes a
 * function by name, so the visitor is a constant where the walk is expanded and is inlined into the scan loop (LABNOTES has
 * the check of the object code): a new host twin writes a visitor, not an eighth copy of this. */
typedef void (*walk_visit)(void *ctx, const int32_t *r);
enum { WALK_BACK = 0, WALK_FORWARD = 1 };

static inline int counted(const int32_t *r, int32_t lo, int32_t v, int use_v, int32_t nf)
{
    return r[2] > lo && (!use_v || r[3] >= v) && r[0] >= 0 && r[0] < nf;
}

static inline __attribute__((always_inline)) int walk_tiles(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t lo,
                                                            int32_t hi, int32_t v, int use_v, int nest, int dir, walk_visit visit, void *ctx)
{
    if (ichr < 0 || ichr >= db->nCtg) return 1;                            /* :456-457 */
    const int32_t nbp = db->nbp, mT = db->nTile[ichr] - 1;
    const int32_t n1 = lo / nbp;                                           /* C division, as :459 */
    int32_t n2 = (int32_t)((uint32_t)hi - 1u) / nbp;                       /* (hi-1)/nbp with the reference's wrap */
    if (n1 < 0 || n1 > mT) return 1;                                       /* (no record ends behind the contig's last tile) */
    if (n2 > mT) n2 = mT;
    if (nest && db->nCnt[ichr][n1] == 0) return 1;                         /* :468 */
    const int w = db->gType == 0 ? 3 : 4;
    const int32_t nf = db->nFiles;
    for (int32_t j = n1; j <= (n2 > n1 ? n2 : n1); j++) {
        const int32_t cnt = db->nCnt[ichr][j];
        if (cnt <= 0) continue;
        const int32_t *rec = tile_records(db, m, tb, ichr, j, cnt);
        if (!rec) return 0;
        const int32_t tile0 = (int32_t)((uint32_t)nbp * (uint32_t)j), stop = below(rec, w, cnt, hi);
        if (dir == WALK_FORWARD) {
            for (int32_t i = j == n1 ? 0 : below(rec, w, cnt, tile0); i < stop; i++) {
                const int32_t *r = rec + (size_t)i * (size_t)w;
                if (counted(r, lo, v, use_v, nf)) visit(ctx, r);
            }
        } else {
            const int64_t lob = j == n1 ? INT64_MIN : (int64_t)tile0;
            for (int32_t i = stop - 1; i >= 0; i--) {
                const int32_t *r = rec + (size_t)i * (size_t)w;
                if ((int64_t)r[1] < lob) break;                            /* met in an earlier tile (:510-511) */
                if (counted(r, lo, v, use_v, nf)) visit(ctx, r);
            }
        }
    }
    return 1;
}

/* ---- the visitors: one per kind of answer.  Each one_* function sets up its row BEFORE the walk (an unknown contig still
 * gives a defined row) and returns what the walk had when it stopped. */

/* pair counts: hits may be NULL (count only); emit appends (idx,start,end) triples in the reference's -f order.
 * mo: an ACTIVE minimum overlap per pair (include/igd_hip.h: igd_hip_min_overlap; the host flavours pass NULL for an inactive
 * one), the same inline predicate as the kernels': need_q once per query, the pair test on every record the walk counts */
typedef struct { igd_hip_hit *v; int64_t n, cap; int failed; } hitvec;
static inline void hv_push(hitvec *o, int32_t q, const int32_t *r)
{
    if (o->n == o->cap) {
        const int64_t nc = o->cap ? 2 * o->cap : 4096;
        igd_hip_hit *nv = (igd_hip_hit *)realloc(o->v, sizeof(igd_hip_hit) * (size_t)nc);
        if (!nv) { o->failed = 1; return; }
        o->v = nv; o->cap = nc;
    }
    igd_hip_hit *h = &o->v[o->n++];
    h->q = q; h->idx = r[0]; h->start = r[1]; h->end = r[2];
}

typedef struct { int32_t qs, qe, need, qno; const igd_hip_min_overlap *mo; int64_t *hits; hitvec *emit; int64_t total; } pairs_ctx;
static inline void visit_pairs(void *ctx, const int32_t *r)
{
    pairs_ctx *c = (pairs_ctx *)ctx;
    if (c->mo && !igd_hip_min_overlap_pair(c->need, c->mo->ppm_record, c->qs, c->qe, r[1], r[2])) return;
    if (c->hits) c->hits[r[0]]++;
    if (c->emit) hv_push(c->emit, c->qno, r);
    c->total++;
}
static inline int64_t one_query(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t qs, int32_t qe, int32_t v,
                                int use_v, int rule, int64_t *hits, hitvec *emit, int32_t qno, const igd_hip_min_overlap *mo)
{
    pairs_ctx c = {qs, qe, mo ? igd_hip_min_overlap_need_q(mo->min_bp, mo->ppm_query, qs, qe) : 0, qno, mo, hits, emit, 0};
    if (c.need < 0) return 0;                                              /* qe <= qs: no record qualifies */
    walk_tiles(db, m, tb, ichr, qs, qe, v, use_v, rule == IGD_HIP_RULE_NEST, WALK_BACK, visit_pairs, &c);
    return c.total;
}

/* support counts (igdc_support_host): a file counts once per query.  last[f] holds the stamp of the last query that counted
 * file f (stamp = query number + 1; 0 = none yet).  Returns 1 if the query overlaps any record. */
typedef struct { int32_t qs, qe, need; const igd_hip_min_overlap *mo; int64_t *support, *last, stamp; int any; } support_ctx;
static inline void visit_support(void *ctx, const int32_t *r)
{
    support_ctx *c = (support_ctx *)ctx;
    if (c->mo && !igd_hip_min_overlap_pair(c->need, c->mo->ppm_record, c->qs, c->qe, r[1], r[2])) return;
    c->any = 1;
    if (c->last[r[0]] != c->stamp) { c->last[r[0]] = c->stamp; c->support[r[0]]++; }
}
static inline int one_query_support(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t qs, int32_t qe, int32_t v,
                                    int use_v, int rule, int64_t *support, int64_t *last, int64_t stamp, const igd_hip_min_overlap *mo)
{
    support_ctx c = {qs, qe, mo ? igd_hip_min_overlap_need_q(mo->min_bp, mo->ppm_query, qs, qe) : 0, mo, support, last, stamp, 0};
    if (c.need < 0) return 0;
    walk_tiles(db, m, tb, ichr, qs, qe, v, use_v, rule == IGD_HIP_RULE_NEST, WALK_BACK, visit_support, &c);
    return c.any;
}

/* support counts per group of datasets (igdc_group_support_host_ov; include/igd_hip.h has the grouping): one_query_support with
 * one stamp per GROUP -- a counted record of dataset f visits the groups goff[f] .. goff[f + 1] of gidx, and a group counts once
 * per query however many of its datasets the query meets.  Returns 1 if the query met a dataset with at least one group. */
typedef struct {
    int32_t qs, qe, need; const igd_hip_min_overlap *mo; const int32_t *goff, *gidx; int64_t *gsupport, *last, stamp; int any;
} group_support_ctx;
static inline void visit_group_support(void *ctx, const int32_t *r)
{
    group_support_ctx *c = (group_support_ctx *)ctx;
    if (c->mo && !igd_hip_min_overlap_pair(c->need, c->mo->ppm_record, c->qs, c->qe, r[1], r[2])) return;
    for (int32_t j = c->goff[r[0]]; j < c->goff[r[0] + 1]; j++) {
        const int32_t g = c->gidx[j];
        c->any = 1;
        if (c->last[g] != c->stamp) { c->last[g] = c->stamp; c->gsupport[g]++; }
    }
}
static inline int one_query_group_support(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t qs, int32_t qe, int32_t v,
                                          int use_v, int rule, const int32_t *goff, const int32_t *gidx, int64_t *gsupport, int64_t *last,
                                          int64_t stamp, const igd_hip_min_overlap *mo)
{
    group_support_ctx c = {qs, qe, mo ? igd_hip_min_overlap_need_q(mo->min_bp, mo->ppm_query, qs, qe) : 0, mo, goff, gidx, gsupport, last, stamp, 0};
    if (c.need < 0) return 0;
    walk_tiles(db, m, tb, ichr, qs, qe, v, use_v, rule == IGD_HIP_RULE_NEST, WALK_BACK, visit_group_support, &c);
    return c.any;
}

/* membership rows (igdc_membership_host): a counted record sets its file's bit in the query's row (zeroed here first).
 * Returns the number of files met. */
typedef struct { uint32_t *row; int n; } member_ctx;
static inline void visit_member(void *ctx, const int32_t *r)
{
    member_ctx *c = (member_ctx *)ctx;
    const uint32_t bit = 1u << (r[0] & 31);
    if (!(c->row[r[0] >> 5] & bit)) { c->row[r[0] >> 5] |= bit; c->n++; }
}
static inline int one_query_member(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t qs, int32_t qe, int32_t v,
                                   int use_v, int rule, uint32_t *row, int32_t nW)
{
    member_ctx c = {row, 0};
    memset(row, 0, sizeof(uint32_t) * (size_t)nW);
    walk_tiles(db, m, tb, ichr, qs, qe, v, use_v, rule == IGD_HIP_RULE_NEST, WALK_BACK, visit_member, &c);
    return c.n;
}

/* covered base pairs (igdc_coverage_host): the walk FORWARD, so the counted records come in non-decreasing start order (a tile
 * is sorted by start, a later tile skips start < its own, every record of an earlier tile starts before it).  front[f] = file f
 * is covered up to here under this query; last[f] = the stamp of the last query that met file f, as in one_query_support
 * (another stamp: the frontier is the query's start).  A record adds what it covers beyond the frontier: coverage[f] +=
 * | [qs, qe) n union of f's counted records |.  Returns the same for the union over all files. */
typedef struct { int32_t qs, qe; int64_t *coverage, *last, *front, stamp, all, covered; } coverage_ctx;
static inline void visit_coverage(void *ctx, const int32_t *r)
{
    coverage_ctx *c = (coverage_ctx *)ctx;
    const int64_t lo = r[1] > c->qs ? r[1] : c->qs, hi = r[2] < c->qe ? r[2] : c->qe;
    if (c->last[r[0]] != c->stamp) { c->last[r[0]] = c->stamp; c->front[r[0]] = c->qs; }
    const int64_t from = lo > c->front[r[0]] ? lo : c->front[r[0]];
    if (hi > from) c->coverage[r[0]] += hi - from;
    if (hi > c->front[r[0]]) c->front[r[0]] = hi;
    const int64_t afrom = lo > c->all ? lo : c->all;
    if (hi > afrom) c->covered += hi - afrom;
    if (hi > c->all) c->all = hi;
}
static inline int64_t one_query_coverage(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t qs, int32_t qe,
                                         int32_t v, int use_v, int rule, int64_t *coverage, int64_t *last, int64_t *front, int64_t stamp)
{
    coverage_ctx c = {qs, qe, coverage, last, front, stamp, qs, 0};        /* all: the frontier over all files (64 bits: no wrap) */
    walk_tiles(db, m, tb, ichr, qs, qe, v, use_v, rule == IGD_HIP_RULE_NEST, WALK_FORWARD, visit_coverage, &c);
    return c.covered;
}

/* nearest record per dataset within a window (include/igd_hip.h has the definitions).  One region: its row is set to -1, the
 * interval is widened by the window (igd_hip_nearest_widen), the tiles of the widened interval are walked without rule NEST's
 * exit, and every counted record lowers row[idx] to its d, computed from the region as given (igd_hip_nearest_dist).  Returns
 * the minimum over the files, or -1.  one_region_keys is that on unsigned words, 0xffffffff (= -1) for "none": with sgn it
 * minimises igd_hip_nearest_key instead of d, and one_region_nearest_signed decodes the row and the minimum
 * (igd_hip_nearest_key_decode). */
typedef struct { int32_t qs, qe; int sgn; uint32_t *row, best; } keys_ctx;
static inline void visit_keys(void *ctx, const int32_t *r)
{
    keys_ctx *c = (keys_ctx *)ctx;
    const uint32_t d = c->sgn ? igd_hip_nearest_key(c->qs, c->qe, r[1], r[2]) : (uint32_t)igd_hip_nearest_dist(c->qs, c->qe, r[1], r[2]);
    if (d < c->row[r[0]]) c->row[r[0]] = d;
    if (d < c->best) c->best = d;
}
static inline uint32_t one_region_keys(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t qs, int32_t qe,
                                       int32_t window, int32_t v, int use_v, int sgn, uint32_t *row)
{
    keys_ctx c = {qs, qe, sgn, row, 0xffffffffu};
    int32_t ws, we;
    for (int32_t f = 0; f < db->nFiles; f++) row[f] = 0xffffffffu;
    igd_hip_nearest_widen(qs, qe, window, &ws, &we);
    walk_tiles(db, m, tb, ichr, ws, we, v, use_v, 0, WALK_BACK, visit_keys, &c);
    return c.best;
}
static inline int32_t one_region_nearest(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t qs, int32_t qe,
                                         int32_t window, int32_t v, int use_v, int32_t *row)
{
    return (int32_t)one_region_keys(db, m, tb, ichr, qs, qe, window, v, use_v, 0, (uint32_t *)row);
}
static inline int32_t one_region_nearest_signed(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t qs, int32_t qe,
                                                int32_t window, int32_t v, int use_v, int32_t *row)
{
    const uint32_t best = one_region_keys(db, m, tb, ichr, qs, qe, window, v, use_v, 1, (uint32_t *)row);
    for (int32_t f = 0; f < db->nFiles; f++) row[f] = igd_hip_nearest_key_decode((uint32_t)row[f]);
    return igd_hip_nearest_key_decode(best);
}

/* flanking records per dataset (include/igd_hip.h has the definitions).  One region: one_region_keys' walk -- the same tiles,
 * the same counted records -- with two unsigned words per file, 0xffffffff (= -1) for "none": igd_hip_flank_pair says on which
 * side a counted record lies and how far, and it lowers that side's word.  The minima over the files go to *upmin, *downmin. */
typedef struct { int32_t qs, qe, window; int measure; uint32_t *up, *down, upmin, downmin; } flank_ctx;
static inline void visit_flanks(void *ctx, const int32_t *r)
{
    flank_ctx *c = (flank_ctx *)ctx;
    uint32_t d = 0;
    const int side = igd_hip_flank_pair(c->measure, c->window, c->qs, c->qe, r[1], r[2], &d);
    if (side == IGD_HIP_FLANK_NEITHER) return;
    uint32_t *row = side == IGD_HIP_FLANK_UP ? c->up : c->down, *best = side == IGD_HIP_FLANK_UP ? &c->upmin : &c->downmin;
    if (d < row[r[0]]) row[r[0]] = d;
    if (d < *best) *best = d;
}
static inline void one_region_flanks(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t qs, int32_t qe,
                                     int32_t window, int measure, int32_t v, int use_v, uint32_t *up, uint32_t *down, uint32_t *upmin,
                                     uint32_t *downmin)
{
    flank_ctx c = {qs, qe, window, measure, up, down, 0xffffffffu, 0xffffffffu};
    int32_t ws, we;
    for (int32_t f = 0; f < db->nFiles; f++) up[f] = down[f] = 0xffffffffu;
    igd_hip_nearest_widen(qs, qe, window, &ws, &we);
    walk_tiles(db, m, tb, ichr, ws, we, v, use_v, 0, WALK_BACK, visit_flanks, &c);
    *upmin = c.upmin; *downmin = c.downmin;
}

/* values of the overlapping records per region and dataset (include/igd_hip.h has the definitions).  One region: its rows are
 * set to 0, the tiles of igd_hip_nearest_widen(qs, qe, 0) are walked as one_region_keys walks them, and every counted record
 * adds 1 to count[idx] and folds its value into agg[idx] (NULL under COUNT: nothing). */
typedef struct { int op; int32_t *count; int64_t *agg; } map_ctx;
static inline void visit_map(void *ctx, const int32_t *r)
{
    map_ctx *c = (map_ctx *)ctx;
    const int32_t f = r[0];
    if (c->op != IGD_HIP_MAP_COUNT) {
        const int64_t val = r[3];
        if (c->op == IGD_HIP_MAP_SUM) c->agg[f] = (int64_t)((uint64_t)c->agg[f] + (uint64_t)val);
        else if (c->count[f] == 0 || (c->op == IGD_HIP_MAP_MIN ? val < c->agg[f] : val > c->agg[f])) c->agg[f] = val;
    }
    c->count[f]++;
}
static inline void one_region_map(const igdc_db *db, const igdc_map *m, tilebuf *tb, int32_t ichr, int32_t qs, int32_t qe, int op,
                                  int32_t v, int use_v, int32_t *count, int64_t *agg)
{
    map_ctx c = {op, count, agg};
    const int32_t nf = db->nFiles;
    int32_t ws, we;
    for (int32_t f = 0; f < nf; f++) count[f] = 0;
    if (agg) for (int32_t f = 0; f < nf; f++) agg[f] = 0;
    igd_hip_nearest_widen(qs, qe, 0, &ws, &we);
    if (!walk_tiles(db, m, tb, ichr, ws, we, v, use_v, 0, WALK_BACK, visit_map, &c)) return;
    if (agg && op == IGD_HIP_MAP_COUNT) for (int32_t f = 0; f < nf; f++) agg[f] = count[f];
}

/* ---- threads ---------------------------------------------------------------------------------------------------------------
 * run_threads: T jobs of one type, `size` bytes apart: jobs 1 .. T-1 on new threads, job 0 on the caller; a thread that could
 * not be created has its job run here, inline.  Returns when all are done.  How many threads a call is worth is the caller's
 * rule (host_threads, capped by what there is to share out). */
#define HOST_MAX_THREADS 64
static int host_threads(int64_t nq)
{
    const char *e = getenv("IGD_HOST_THREADS");
    long t = e && *e ? atol(e) : 0;
    if (t <= 0) {
        t = sysconf(_SC_NPROCESSORS_ONLN);
        if (t > 16) t = 16;
    }
    const int64_t byWork = (nq + 2047) / 2048;      /* a thread is worth starting for ~2000 queries (~3 ms of counting) */
    if (t > byWork) t = (long)byWork;
    if (t > HOST_MAX_THREADS) t = HOST_MAX_THREADS;
    return t < 1 ? 1 : (int)t;
}

static void run_threads(void *(*run)(void *), void *jobs, size_t size, int T)
{
    pthread_t th[HOST_MAX_THREADS];
    int started[HOST_MAX_THREADS];
    for (int k = 1; k < T; k++) {
        void *job = (char *)jobs + (size_t)k * size;
        started[k] = pthread_create(&th[k], NULL, run, job) == 0;
        if (!started[k]) run(job);
    }
    run(jobs);
    for (int k = 1; k < T; k++) if (started[k]) pthread_join(th[k], NULL);
}

/* ---- the job of one thread of a query-split entry: queries [lo, hi) of the caller's arrays, answered as `kind` says --------- */
enum { JOB_PAIRS, JOB_SUPPORT, JOB_COVERAGE, JOB_MEMBER, JOB_NEAREST, JOB_FLANK, JOB_MAP, JOB_GROUP_SUPPORT };
typedef struct {
    int kind;
    const igdc_db *db; const igdc_map *m;
    const int32_t *ichr, *qs, *qe;
    int64_t lo, hi;
    int32_t v; int use_v, rule;
    int64_t total;          /* out: PAIRS pairs, SUPPORT, GROUP_SUPPORT and MEMBER queries with a hit, COVERAGE base pairs under any file */
    int io_failed;          /* out: a tile could not be read */
    int64_t *hits;          /* PAIRS hits[] (may be NULL), SUPPORT support[], COVERAGE coverage[], GROUP_SUPPORT gsupport[] */
    int64_t *last, *front;  /* SUPPORT, COVERAGE, GROUP_SUPPORT: the stamps; COVERAGE: the frontiers */
    const igd_hip_min_overlap *mo;      /* PAIRS, SUPPORT, GROUP_SUPPORT: an active minimum overlap, or NULL */
    const int32_t *goff, *gidx;         /* GROUP_SUPPORT: the grouping (grp_off, grp_idx) */
    int64_t *qcnt;          /* PAIRS: per-query counts (enumeration; may be NULL) */
    hitvec out; int want_out;
    uint32_t *bits;         /* MEMBER: the caller's rows, nW words each; nfh: its nfiles_hit[] or NULL */
    int32_t *nfh, nW;
    int32_t window; int sgn, measure, op;           /* NEAREST window, sgn; FLANK window, measure; MAP op */
    int32_t *rowa, *rowb, *mina, *minb;             /* NEAREST dist, -, dmin, -; FLANK up, down, upmin, downmin; MAP count; */
    int64_t *agg;                                   /* MAP agg or NULL; rows of nFiles words per query, mins may be NULL */
} host_job;

static void job_init(host_job *J, int kind, const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                     int64_t lo, int64_t hi, int32_t v, int rule)
{
    memset(J, 0, sizeof *J);
    J->kind = kind; J->db = db; J->m = m; J->ichr = ichr; J->qs = qs; J->qe = qe;
    J->lo = lo; J->hi = hi;
    J->v = v; J->use_v = v != IGD_HIP_NO_VALUE_FILTER && db->gType == 1;   /* gType 0 stores no value (:1024-1025) */
    J->rule = rule;
}

/* T jobs over nq queries in contiguous ranges; the caller adds what its kind needs */
static void jobs_split(host_job *job, int T, int kind, const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs,
                       const int32_t *qe, int64_t nq, int32_t v, int rule)
{
    for (int k = 0; k < T; k++) job_init(&job[k], kind, db, m, ichr, qs, qe, nq * k / T, nq * (k + 1) / T, v, rule);
}

static void *host_run(void *arg)
{
    host_job *J = (host_job *)arg;
    const igdc_db *db = J->db;
    const igdc_map *m = J->m;
    const int32_t *ichr = J->ichr, *qs = J->qs, *qe = J->qe, v = J->v;
    const int use_v = J->use_v, rule = J->rule;
    const size_t nf = (size_t)db->nFiles;
    int64_t tot = 0;
    tilebuf tb;
    tb_open(&tb);
    switch (J->kind) {
    case JOB_PAIRS:
        for (int64_t i = J->lo; i < J->hi; i++) {
            const int64_t n = one_query(db, m, &tb, ichr[i], qs[i], qe[i], v, use_v, rule, J->hits, J->want_out ? &J->out : NULL, (int32_t)i, J->mo);
            if (J->qcnt) J->qcnt[i] = n;
            tot += n;
        }
        break;
    case JOB_SUPPORT:
        for (int64_t i = J->lo; i < J->hi; i++)
            tot += one_query_support(db, m, &tb, ichr[i], qs[i], qe[i], v, use_v, rule, J->hits, J->last, i + 1, J->mo);
        break;
    case JOB_GROUP_SUPPORT:
        for (int64_t i = J->lo; i < J->hi; i++)
            tot += one_query_group_support(db, m, &tb, ichr[i], qs[i], qe[i], v, use_v, rule, J->goff, J->gidx, J->hits, J->last, i + 1, J->mo);
        break;
    case JOB_COVERAGE:
        for (int64_t i = J->lo; i < J->hi; i++)
            tot += one_query_coverage(db, m, &tb, ichr[i], qs[i], qe[i], v, use_v, rule, J->hits, J->last, J->front, i + 1);
        break;
    case JOB_MEMBER:
        for (int64_t i = J->lo; i < J->hi; i++) {
            const int n = one_query_member(db, m, &tb, ichr[i], qs[i], qe[i], v, use_v, rule, J->bits + (size_t)i * (size_t)J->nW, J->nW);
            if (J->nfh) J->nfh[i] = n;
            tot += n > 0;
        }
        break;
    case JOB_NEAREST:
        for (int64_t i = J->lo; i < J->hi; i++) {
            int32_t *row = J->rowa + (size_t)i * nf;
            const int32_t d = J->sgn ? one_region_nearest_signed(db, m, &tb, ichr[i], qs[i], qe[i], J->window, v, use_v, row)
                                     : one_region_nearest(db, m, &tb, ichr[i], qs[i], qe[i], J->window, v, use_v, row);
            if (J->mina) J->mina[i] = d;
        }
        break;
    case JOB_FLANK:
        for (int64_t i = J->lo; i < J->hi; i++) {
            uint32_t um, dm;
            one_region_flanks(db, m, &tb, ichr[i], qs[i], qe[i], J->window, J->measure, v, use_v, (uint32_t *)J->rowa + (size_t)i * nf,
                              (uint32_t *)J->rowb + (size_t)i * nf, &um, &dm);
            if (J->mina) J->mina[i] = (int32_t)um;
            if (J->minb) J->minb[i] = (int32_t)dm;
        }
        break;
    case JOB_MAP:
        for (int64_t i = J->lo; i < J->hi; i++)
            one_region_map(db, m, &tb, ichr[i], qs[i], qe[i], J->op, v, use_v, J->rowa + (size_t)i * nf, J->agg ? J->agg + (size_t)i * nf : NULL);
        break;
    }
    J->total = tot;
    J->io_failed = tb_close(&tb);
    return NULL;
}

/* runs the jobs; nonzero if a tile could not be read; *tot (may be NULL) = the sum of the jobs' totals */
static int jobs_run(host_job *job, int T, int64_t *tot)
{
    int bad = 0;
    int64_t sum = 0;
    run_threads(host_run, job, sizeof *job, T);
    for (int k = 0; k < T; k++) { bad |= job[k].io_failed; sum += job[k].total; }
    if (tot) *tot = sum;
    return bad;
}

/* the entries whose answer is a sum over queries (pair counts, support counts, covered base pairs, group support counts): every
 * thread counts into nvec private vectors of ncols + 1 words -- the answer, then the stamps, then the frontiers -- and the
 * answers are ADDED to out[] only if every tile could be read.  ncols is nFiles, or the number of groups with the grouping goff /
 * gidx behind it (JOB_GROUP_SUPPORT).  0 and *tot = the sum of the threads' totals, or -1 with out[] as it was. */
static int run_private_cols(int kind, int nvec, int32_t ncols, const int32_t *goff, const int32_t *gidx, const igdc_db *db, const igdc_map *m,
                            const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t v, int rule,
                            const igd_hip_min_overlap *mo, int64_t *out, int64_t *tot)
{
    const int T = host_threads(nq);
    const size_t nf1 = (size_t)ncols + 1;
    host_job job[HOST_MAX_THREADS];
    int64_t *priv = (int64_t *)calloc((size_t)T * (size_t)nvec * nf1, sizeof(int64_t));
    if (!priv) return -1;
    jobs_split(job, T, kind, db, m, ichr, qs, qe, nq, v, rule);
    for (int k = 0; k < T; k++) {
        job[k].hits = priv + (size_t)k * (size_t)nvec * nf1;
        if (nvec > 1) job[k].last = job[k].hits + nf1;
        if (nvec > 2) job[k].front = job[k].last + nf1;
        job[k].mo = mo;
        job[k].goff = goff; job[k].gidx = gidx;
    }
    const int bad = jobs_run(job, T, tot);
    for (int k = 0; k < T && !bad; k++)
        for (int32_t f = 0; f < ncols; f++) out[f] += job[k].hits[f];
    free(priv);
    return bad ? -1 : 0;
}
static int run_private(int kind, int nvec, const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                       int64_t nq, int32_t v, int rule, const igd_hip_min_overlap *mo, int64_t *out, int64_t *tot)
{
    return run_private_cols(kind, nvec, db->nFiles, NULL, NULL, db, m, ichr, qs, qe, nq, v, rule, mo, out, tot);
}

int igdc_search_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                     int64_t nq, int32_t v, int rule, int64_t *hits, int64_t *total)
{
    return igdc_search_host_ov(db, m, ichr, qs, qe, nq, v, rule, hits, total, NULL);
}

int igdc_search_host_ov(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                        int64_t nq, int32_t v, int rule, int64_t *hits, int64_t *total, const igd_hip_min_overlap *min_overlap)
{
    if (!db || !m || !hits || nq < 0 || !igd_hip_min_overlap_valid(min_overlap)) return -1;
    int64_t tot = 0;
    if (run_private(JOB_PAIRS, 1, db, m, ichr, qs, qe, nq, v, rule, igd_hip_min_overlap_active(min_overlap) ? min_overlap : NULL, hits, &tot) != 0)
        return -1;
    if (total) *total = tot;
    return 0;
}

int igdc_support_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                      int64_t nq, int32_t v, int rule, int64_t *support, int64_t *nhit)
{
    return igdc_support_host_ov(db, m, ichr, qs, qe, nq, v, rule, support, nhit, NULL);
}

int igdc_support_host_ov(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                         int64_t nq, int32_t v, int rule, int64_t *support, int64_t *nhit, const igd_hip_min_overlap *min_overlap)
{
    if (!db || !m || !support || nq < 0 || !igd_hip_min_overlap_valid(min_overlap)) return -1;
    int64_t tot = 0;
    if (run_private(JOB_SUPPORT, 2, db, m, ichr, qs, qe, nq, v, rule, igd_hip_min_overlap_active(min_overlap) ? min_overlap : NULL, support, &tot) != 0)
        return -1;
    if (nhit) *nhit += tot;
    return 0;
}

int igdc_group_support_host_ov(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const int32_t *grp_off, const int32_t *grp_idx, int32_t ngroups, int32_t v, int rule, int64_t *gsupport,
                               int64_t *gnhit, const igd_hip_min_overlap *min_overlap)
{
    int64_t at = 0, tot = 0;
    if (!db || !m || !gsupport || nq < 0 || !grp_off || ngroups <= 0 || ngroups > IGD_HIP_GROUP_MAX || !igd_hip_min_overlap_valid(min_overlap) ||
        igd_hip_groups_first_bad(db->nFiles, grp_off, grp_idx, ngroups, &at) != IGD_HIP_GROUPS_OK)
        return -1;
    if (run_private_cols(JOB_GROUP_SUPPORT, 2, ngroups, grp_off, grp_idx, db, m, ichr, qs, qe, nq, v, rule,
                         igd_hip_min_overlap_active(min_overlap) ? min_overlap : NULL, gsupport, &tot) != 0)
        return -1;
    if (gnhit) *gnhit += tot;
    return 0;
}

int igdc_coverage_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                       int64_t nq, int32_t v, int rule, int64_t *coverage, int64_t *covered)
{
    if (!db || !m || !coverage || nq < 0) return -1;
    int64_t tot = 0;
    if (run_private(JOB_COVERAGE, 3, db, m, ichr, qs, qe, nq, v, rule, NULL, coverage, &tot) != 0) return -1;
    if (covered) *covered += tot;
    return 0;
}

int igdc_membership_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                         int64_t nq, int32_t v, int rule, uint32_t *bits, int32_t *nfiles_hit, int64_t *nhit)
{
    if (!db || !m || nq < 0 || (nq > 0 && !bits)) return -1;
    const int T = host_threads(nq);
    host_job job[HOST_MAX_THREADS];
    uint32_t none = 0;                       /* (a database without files: rows of no words) */
    /* rows are disjoint per query: every thread writes its queries' rows straight into the caller's */
    jobs_split(job, T, JOB_MEMBER, db, m, ichr, qs, qe, nq, v, rule);
    for (int k = 0; k < T; k++) { job[k].bits = bits ? bits : &none; job[k].nfh = nfiles_hit; job[k].nW = (db->nFiles + 31) / 32; }
    int64_t tot = 0;
    if (jobs_run(job, T, &tot)) return -1;
    if (nhit) *nhit += tot;
    return 0;
}

int igdc_enumerate_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                        int64_t nq, int64_t *qoff, igd_hip_hit **out, int64_t *total)
{
    if (!db || !m || !qoff || !out || nq < 0 || nq > INT32_MAX) return -1;
    *out = NULL;
    const int T = host_threads(nq);
    host_job job[HOST_MAX_THREADS];
    jobs_split(job, T, JOB_PAIRS, db, m, ichr, qs, qe, nq, IGD_HIP_NO_VALUE_FILTER, IGD_HIP_RULE_NEST);      /* -f: rule NEST, no filter */
    for (int k = 0; k < T; k++) { job[k].qcnt = qoff; job[k].want_out = 1; }       /* counts first, turned into offsets below */
    int failed = jobs_run(job, T, NULL);
    int64_t tot = 0;
    for (int k = 0; k < T; k++) { tot += job[k].out.n; failed |= job[k].out.failed; }
    igd_hip_hit *all = failed ? NULL : (igd_hip_hit *)malloc(sizeof(igd_hip_hit) * (size_t)(tot ? tot : 1));
    if (!all) failed = 1;
    int64_t at = 0;
    for (int k = 0; k < T; k++) {
        if (!failed && job[k].out.n) memcpy(all + at, job[k].out.v, sizeof(igd_hip_hit) * (size_t)job[k].out.n);
        at += job[k].out.n;
        free(job[k].out.v);
    }
    if (failed) return -1;
    int64_t run = 0;
    for (int64_t i = 0; i < nq; i++) { const int64_t c = qoff[i]; qoff[i] = run; run += c; }
    qoff[nq] = run;
    *out = all;
    if (total) *total = tot;
    return 0;
}

/* ---- region sets: the offsets' check and the loop over chunks of regions ---------------------------------------------------
 * set_off_bad: nsets >= 0 offsets from 0 that never fall, and the region arrays if there is a region. */
static int set_off_bad(const int64_t *set_off, int32_t nsets, const int32_t *ichr, const int32_t *qs, const int32_t *qe)
{
    if (nsets < 0 || (nsets > 0 && (!set_off || set_off[0] != 0))) return 1;
    for (int32_t k = 0; k < nsets; k++)
        if (set_off[k + 1] < set_off[k]) return 1;
    return nsets > 0 && set_off[nsets] > 0 && (!ichr || !qs || !qe);
}


/* Fisher's exact test of 2x2 tables on the host: what igd_fisher_cells (engine/fisher_dev.hpp) computes, by the same scheme
 * -- log space, nine log-factorials per term added in the same pairs, the tail summed from the side on which it decays in
 * steps of 64 terms until a step's first term is below the first one by 45 -- with the C library's lgamma, on the calling
 * thread.  The statistics of `-U` when the supports were counted on the host. */
/* libm by weak reference: the libraries link -lm (Makefile), but this file is also compiled into test harnesses whose
 * link lines are fixed and do not name it.  Every process that reaches here has libm mapped (the HIP engine and the
 * sanitizer runtimes need it); a process that has not is answered with -1, not with a crash. */
#pragma weak exp
#pragma weak log
#pragma weak log1p
#pragma weak lgamma_r
#define FISHER_STOP 45.0
#define FISHER_LN10 2.302585092994045684
static double lfact(int64_t x)
{
    int sign;
    return lgamma_r((double)x + 1.0, &sign);
}
static double fisher_plog(int64_t a, int64_t b, int64_t c, int64_t d)
{
    const int64_t N = a + b + c + d, K = a + b, n = a + c;
    const int64_t lo = a - d > 0 ? a - d : 0, hi = n < K ? n : K;
    if (N == 0 || a <= lo) return 0.0;
    const int64_t mode = ((n + 1) * (K + 1)) / (N + 2);
    const int up = a > mode;
    const double lfK = lfact(K), lfNK = lfact(N - K), lfn = lfact(n), tail5 = lfact(N - n) - lfact(N);
    const int64_t k0 = up ? a : a - 1, rest = N - K - n;
    double tFirst = 0.0, S = 0.0;
    for (int64_t base = 0;; base += 64) {
        double t0 = 0.0, acc = 0.0;
        for (int j = 0; j < 64; j++) {
            const int64_t k = up ? k0 + base + j : k0 - base - j;
            if (up ? k > hi : k < lo) break;
            const double t = ((lfK - lfact(K - k)) + (lfNK - lfact(rest + k))) + (((lfn - lfact(n - k)) - lfact(k)) + tail5);
            if (j == 0) { t0 = t; if (base == 0) tFirst = t; }
            acc += exp(t - tFirst);
        }
        S += acc;
        if (t0 < tFirst - FISHER_STOP) break;
        if (up ? k0 + base + 64 > hi : k0 - base - 64 < lo) break;
    }
    double lp = tFirst + log(S);
    if (!up) {
        double L = exp(lp);
        if (!(L < 1.0)) L = 0x1.fffffffffffffp-1;
        lp = log1p(-L);
    }
    const double r = -lp / FISHER_LN10;
    return r > 0.0 ? r : 0.0;
}

int igdc_fisher_host(const int64_t *a, const int64_t *b, const int64_t *c, const int64_t *d, int64_t ncell, double *pvalue_log,
                     double *odds_ratio)
{
    if (ncell < 0 || (ncell > 0 && (!a || !b || !c || !d || !pvalue_log))) return -1;
    if (!exp || !log || !log1p || !lgamma_r) return -1;
    const int64_t lim = (int64_t)1 << 31;
    for (int64_t i = 0; i < ncell; i++)
        if (a[i] < 0 || b[i] < 0 || c[i] < 0 || d[i] < 0 || a[i] >= lim || b[i] >= lim || c[i] >= lim || d[i] >= lim ||
            a[i] + b[i] + c[i] + d[i] >= lim)
            return -1;
    for (int64_t i = 0; i < ncell; i++) {
        pvalue_log[i] = fisher_plog(a[i], b[i], c[i], d[i]);
        if (odds_ratio) {
            const double ad = (double)a[i] * (double)d[i], bc = (double)b[i] * (double)c[i];
            odds_ratio[i] = bc == 0.0 ? (ad > 0.0 ? INFINITY : NAN) : ad / bc;
        }
    }
    return 0;
}

/* Ranks and Benjamini-Hochberg q-values of an enrichment table on the host: what igd_rank_rows (engine/rank_dev.hpp)
 * computes, by the same scheme -- per row and column a 64-bit key whose unsigned order is the column's, the cells sorted by
 * descending key (equal keys by column), the start of a cell's tie run its rank - 1, the end of the run r, and q the maximum
 * of adj = p + (log10 r - log10 m) from the small end, clamped at +0.0 -- on the calling thread.  The ranks and q of `-U -R`
 * when the supports were counted on the host.  log10 by weak reference, as the Fisher test's functions above. */
#pragma weak log10
typedef struct { uint64_t key; uint32_t idx; } rank_cell;
static int rank_cell_cmp(const void *x, const void *y)
{
    const rank_cell *a = (const rank_cell *)x, *b = (const rank_cell *)y;
    if (a->key != b->key) return a->key > b->key ? -1 : 1;
    return a->idx < b->idx ? -1 : a->idx > b->idx;
}
static uint64_t rank_bits(double x)
{
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return b;
}
static uint64_t rank_key_or(double x)
{
    if (x != x) return 0;                                 /* NaN: below -inf */
    const uint64_t b = x == 0.0 ? 0 : rank_bits(x);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
/* sorts cell[0..m) and stores rank[idx]; with q also the q-values (the keys are then the bits of pvalue_log >= +0.0) */
static void rank_row(rank_cell *cell, int64_t m, int32_t *rank, double *q)
{
    qsort(cell, (size_t)m, sizeof *cell, rank_cell_cmp);
    if (rank) {
        int64_t start = 0;
        for (int64_t j = 0; j < m; j++) {
            if (j > 0 && cell[j].key != cell[j - 1].key) start = j;
            rank[cell[j].idx] = (int32_t)(start + 1);
        }
    }
    if (q) {
        const double log10m = log10((double)m);
        double adj = 0.0, best = -INFINITY;
        for (int64_t j = m - 1; j >= 0; j--) {
            if (j == m - 1 || cell[j + 1].key != cell[j].key) {      /* the end of a tie run: r = j + 1 */
                double p;
                memcpy(&p, &cell[j].key, sizeof p);
                adj = p + (log10((double)(j + 1)) - log10m);
            }
            if (adj > best) best = adj;
            q[cell[j].idx] = best > 0.0 ? best : 0.0;
        }
    }
}

int igdc_rank_host(const int64_t *support, const double *pvalue_log, const double *odds_ratio, int64_t nrows, int64_t ncols,
                   double *qvalue_log, int32_t *rnk_sup, int32_t *rnk_pv, int32_t *rnk_or, int32_t *max_rnk, double *mean_rnk)
{
    const int mm = max_rnk || mean_rnk;
    const int doSup = rnk_sup || mm, doPv = rnk_pv || qvalue_log || mm, doOr = rnk_or || mm;
    if (nrows < 0 || ncols < 0 || ncols > ((int64_t)1 << 20)) return -1;
    if (nrows == 0 || ncols == 0 || (!doSup && !doPv && !doOr)) return 0;
    if ((doSup && !support) || (doPv && !pvalue_log) || (doOr && !odds_ratio) || nrows > INT64_MAX / ncols) return -1;
    if (qvalue_log && !log10) return -1;
    if (doPv)
        for (int64_t i = 0; i < nrows * ncols; i++)
            if (!(pvalue_log[i] >= 0.0)) return -1;
    const int64_t m = ncols;
    rank_cell *cell = (rank_cell *)malloc(sizeof(rank_cell) * (size_t)m);
    int32_t *tmp = (int32_t *)malloc(sizeof(int32_t) * 3 * (size_t)m);     /* the row's three ranks, for max and mean */
    if (!cell || !tmp) { free(cell); free(tmp); return -1; }
    for (int64_t r = 0; r < nrows; r++) {
        const int64_t o = r * m;
        int32_t *rs = rnk_sup ? rnk_sup + o : tmp, *rp = rnk_pv ? rnk_pv + o : tmp + m, *ro = rnk_or ? rnk_or + o : tmp + 2 * m;
        if (doSup) {
            for (int64_t c = 0; c < m; c++) { cell[c].key = (uint64_t)support[o + c] ^ 0x8000000000000000ull; cell[c].idx = (uint32_t)c; }
            rank_row(cell, m, rs, NULL);
        }
        if (doOr) {
            for (int64_t c = 0; c < m; c++) { cell[c].key = rank_key_or(odds_ratio[o + c]); cell[c].idx = (uint32_t)c; }
            rank_row(cell, m, ro, NULL);
        }
        if (doPv) {
            for (int64_t c = 0; c < m; c++) { cell[c].key = pvalue_log[o + c] == 0.0 ? 0 : rank_bits(pvalue_log[o + c]); cell[c].idx = (uint32_t)c; }
            rank_row(cell, m, rp, qvalue_log ? qvalue_log + o : NULL);
        }
        if (mm)
            for (int64_t c = 0; c < m; c++) {
                const int32_t a = rs[c], b = rp[c], d = ro[c];
                if (max_rnk) max_rnk[o + c] = a > b ? (a > d ? a : d) : (b > d ? b : d);
                if (mean_rnk) mean_rnk[o + c] = (double)(a + b + d) / 3.0;
            }
    }
    free(cell); free(tmp);
    return 0;
}

/* Query sets restricted to the universe on the host: what igd_restrict_bits (engine/restrict_dev.hpp) computes, by the same
 * scheme -- the universe regions with ichr >= 0 ordered by (ichr, start) unless they come that way, per contig the prefix
 * maximum of the ends, per set region a bisection for the first start >= qe and a walk back while the prefix maximum is above
 * qs -- on the calling thread.  The restricted sets of `-U -X` when the supports are counted on the host. */
typedef struct { uint64_t key; int32_t idx; } restrict_ent;
static int restrict_ent_cmp(const void *x, const void *y)
{
    const restrict_ent *a = (const restrict_ent *)x, *b = (const restrict_ent *)y;
    if (a->key != b->key) return a->key < b->key ? -1 : 1;
    return a->idx < b->idx ? -1 : a->idx > b->idx;
}
static int restrict_args_bad(const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                             const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu)
{
    return nsets == INT32_MAX || nu < 0 || nu + 1 >= ((int64_t)1 << 31) || (nu > 0 && (!u_ichr || !u_qs || !u_qe)) ||
           set_off_bad(set_off, nsets, ichr, qs, qe);
}

int igdc_restrict_host(const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                       const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu, uint32_t *bits, int64_t *size)
{
    if (restrict_args_bad(ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu)) return -1;
    const int64_t nUW = (nu + 31) / 32;
    if (nsets > 0 && (!size || (nUW > 0 && !bits))) return -1;
    if (nsets == 0) return 0;
    /* the universe regions with a contig, by (ichr, start), ties in the caller's order */
    restrict_ent *ent = (restrict_ent *)malloc(sizeof(restrict_ent) * (size_t)(nu + 1));
    int32_t *us = (int32_t *)malloc(sizeof(int32_t) * 5 * (size_t)(nu + 1));
    if (!ent || !us) { free(ent); free(us); return -1; }
    int32_t *ue = us + nu, *pm = ue + nu, *cval = pm + nu, *cbeg = cval + nu;      /* (cbeg: at most nv + 1 <= nu + 1 entries) */
    int64_t nv = 0;
    int sorted = 1;
    for (int64_t u = 0; u < nu; u++) {
        if (u_ichr[u] < 0) continue;
        ent[nv].key = ((uint64_t)(uint32_t)u_ichr[u] << 32) | (uint64_t)((uint32_t)u_qs[u] ^ 0x80000000u);
        ent[nv].idx = (int32_t)u;
        if (nv > 0 && ent[nv].key < ent[nv - 1].key) sorted = 0;
        nv++;
    }
    if (!sorted) qsort(ent, (size_t)nv, sizeof *ent, restrict_ent_cmp);
    int32_t nc = 0;
    for (int64_t p = 0; p < nv; p++) {
        const int32_t u = ent[p].idx;
        const int first = p == 0 || u_ichr[ent[p - 1].idx] != u_ichr[u];
        if (first) { cval[nc] = u_ichr[u]; cbeg[nc] = (int32_t)p; nc++; }
        us[p] = u_qs[u]; ue[p] = u_qe[u];
        pm[p] = first || u_qe[u] > pm[p - 1] ? u_qe[u] : pm[p - 1];
    }
    cbeg[nc] = (int32_t)nv;
    if (nUW) memset(bits, 0, sizeof(uint32_t) * (size_t)nsets * (size_t)nUW);
    for (int32_t k = 0; k < nsets; k++) {
        uint32_t *row = bits + (size_t)k * (size_t)nUW;
        int64_t n = 0;
        for (int64_t i = set_off[k]; i < set_off[k + 1]; i++) {
            const int32_t c = ichr[i], s = qs[i], e = qe[i];
            if (c < 0) continue;
            int32_t lo = 0, hi = nc;
            while (lo < hi) { const int32_t m = (lo + hi) >> 1; if (cval[m] < c) lo = m + 1; else hi = m; }
            if (lo >= nc || cval[lo] != c) continue;
            const int32_t s0 = cbeg[lo];
            int32_t a = s0, b = cbeg[lo + 1];
            while (a < b) { const int32_t m = a + ((b - a) >> 1); if (us[m] < e) a = m + 1; else b = m; }
            for (int32_t p = a - 1; p >= s0 && pm[p] > s; p--)
                if (ue[p] > s) {
                    const int32_t u = ent[p].idx;
                    const uint32_t bit = 1u << (u & 31);
                    if (!(row[u >> 5] & bit)) { row[u >> 5] |= bit; n++; }
                }
        }
        size[k] = n;
    }
    free(ent); free(us);
    return 0;
}

/* Enrichment of the restricted sets on the host: igdc_restrict_host, igdc_membership_host over the universe (in the caller's
 * order), the gather support[k][f] = sum over u in R_k of member[u][f], then igdc_fisher_host on a = support, b = usupport - a,
 * c = size - a, d = nu - usupport - c -- what igd_hip_enrich_restricted computes (include/igd_hip.h has the definitions).
 * Outputs are OVERWRITTEN; odds_ratio, bits, nhit and unhit may be NULL.  0 on success; -1 for a bad argument (nothing written)
 * or when a tile could not be read (outputs undefined). */
int igdc_enrich_restricted_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                                const int64_t *set_off, int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe,
                                int64_t nu, int32_t v, int rule, int64_t *support, int64_t *usupport, int64_t *size, double *pvalue_log,
                                double *odds_ratio, uint32_t *bits, int64_t *nhit, int64_t *unhit)
{
    if (!db || !m || restrict_args_bad(ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu)) return -1;
    const int64_t nF = db->nFiles, nW = (nF + 31) / 32, nUW = (nu + 31) / 32;
    const size_t cells = (size_t)nsets * (size_t)nF;
    if ((nF > 0 && !usupport) || (nsets > 0 && (!size || (nF > 0 && (!support || !pvalue_log))))) return -1;
    uint32_t *own = bits ? NULL : (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)nsets * (size_t)nUW + 1));
    uint32_t *rb = bits ? bits : own;
    uint32_t *member = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)nu * (size_t)nW + 1));
    int32_t *nfh = (int32_t *)malloc(sizeof(int32_t) * ((size_t)nu + 1));
    int64_t *tb = (int64_t *)malloc(sizeof(int64_t) * (3 * cells + 1)), *tc = tb ? tb + cells : NULL, *td = tb ? tc + cells : NULL;
    int rc = rb && member && nfh && tb ? 0 : -1;
    int64_t uh = 0;
    if (rc == 0) rc = igdc_restrict_host(ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, rb, size);
    if (rc == 0 && nu > 0) rc = igdc_membership_host(db, m, u_ichr, u_qs, u_qe, nu, v, rule, member, nfh, &uh);
    if (rc == 0) {
        for (int64_t f = 0; f < nF; f++) usupport[f] = 0;
        for (int64_t u = 0; u < nu; u++)
            for (int64_t w = 0; w < nW; w++)
                for (uint32_t x = member[u * nW + w]; x; x &= x - 1) usupport[w * 32 + __builtin_ctz(x)]++;
        if (cells) memset(support, 0, sizeof(int64_t) * cells);
        for (int32_t k = 0; k < nsets; k++) {
            int64_t *row = support + (size_t)k * (size_t)nF, h = 0;
            for (int64_t uw = 0; uw < nUW; uw++)
                for (uint32_t y = rb[(size_t)k * (size_t)nUW + (size_t)uw]; y; y &= y - 1) {
                    const int64_t u = uw * 32 + __builtin_ctz(y);
                    h += nfh[u] > 0;
                    for (int64_t w = 0; w < nW; w++)
                        for (uint32_t x = member[u * nW + w]; x; x &= x - 1) row[w * 32 + __builtin_ctz(x)]++;
                }
            if (nhit) nhit[k] = h;
            for (int64_t f = 0; f < nF; f++) {
                const size_t i = (size_t)k * (size_t)nF + (size_t)f;
                tb[i] = usupport[f] - row[f];
                tc[i] = size[k] - row[f];
                td[i] = nu - usupport[f] - tc[i];
            }
        }
        if (unhit) *unhit = uh;
        if (cells) rc = igdc_fisher_host(support, tb, tc, td, (int64_t)cells, pvalue_log, odds_ratio);
    }
    free(own); free(member); free(nfh); free(tb);
    return rc;
}

/* Popcount Gram product of bit rows on the host: what igd_bitrows_gram (engine/cooccur_dev.hpp) computes.  Rows of nwords32
 * uint32 words `stride` words apart; b == a selects the symmetric form: the cells on and above the diagonal are counted and
 * mirrored.  out (leading dimension ldo) is ADDED to.  Threads take the rows of a interleaved (row i, i + T, ..: the triangle
 * of the symmetric form is shared out evenly); the mirror cell (j, i) of a pair i < j is written by the owner of row i alone. */
typedef struct { const uint32_t *a, *b; int64_t m, n, stride, nw, ldo; int64_t *out; int k, T; } gram_job;
static inline int64_t and_popc(const uint32_t *x, const uint32_t *y, int64_t nw)
{
    int64_t c = 0, w = 0;
    for (; w + 2 <= nw; w += 2) {
        uint64_t p, q;
        memcpy(&p, x + w, 8); memcpy(&q, y + w, 8);
        c += __builtin_popcountll(p & q);
    }
    if (w < nw) c += __builtin_popcount(x[w] & y[w]);
    return c;
}
static void *gram_run(void *p)
{
    const gram_job *J = (const gram_job *)p;
    const int sym = J->a == J->b;
    for (int64_t i = J->k; i < J->m; i += J->T)
        for (int64_t j = sym ? i : 0; j < J->n; j++) {
            const int64_t c = and_popc(J->a + i * J->stride, J->b + j * J->stride, J->nw);
            J->out[i * J->ldo + j] += c;
            if (sym && j != i) J->out[j * J->ldo + i] += c;
        }
    return NULL;
}
static void gram_host(const uint32_t *a, int64_t m, const uint32_t *b, int64_t n, int64_t stride, int64_t nw, int64_t *out, int64_t ldo)
{
    if (m <= 0 || n <= 0) return;
    const double work = (double)m * (double)n * (double)(nw + 1) / 1024.0;     /* a thread per ~2 x 10^6 word pairs */
    const int T = host_threads(work > 1e15 ? (int64_t)1e15 : (int64_t)work);
    gram_job job[HOST_MAX_THREADS];
    for (int k = 0; k < T; k++) {
        job[k].a = a; job[k].b = b; job[k].m = m; job[k].n = n; job[k].stride = stride; job[k].nw = nw; job[k].ldo = ldo;
        job[k].out = out; job[k].k = k; job[k].T = T;
    }
    run_threads(gram_run, job, sizeof job[0], T);
}

int igdc_bitrows_gram_host(const uint32_t *a, int64_t m, const uint32_t *b, int64_t n, int64_t nwords32, int64_t *out)
{
    if (!b) n = m;
    if (m < 0 || n < 0 || nwords32 < 0 || (m > 0 && n > 0 && !out) || (m > 0 && nwords32 > 0 && !a) ||
        (m > 0 && n > ((int64_t)1 << 28) / m))
        return -1;
    if (m == 0 || n == 0) return 0;
    memset(out, 0, sizeof(int64_t) * (size_t)m * (size_t)n);
    if (nwords32 > 0) gram_host(a, m, b ? b : a, n, nwords32, nwords32, out, n);
    return 0;
}

/* Dataset x dataset co-occurrence on the host: what igd_hip_cooccur computes (include/igd_hip.h has the definitions) --
 * igdc_membership_host in chunks of COOCCUR_CHUNK regions, the chunk's rows transposed word-wise into one bit column per
 * file (region r of the chunk = bit r & 31 of word r >> 5), and the popcounts of the column pairs on and above the diagonal
 * added to the matrix and its mirror.  cooc and *nhit are DEFINED by the call.  0 on success; -1 for a bad argument (nothing
 * written) or when a tile could not be read (outputs undefined). */
#define COOCCUR_CHUNK ((int64_t)1 << 16)
int igdc_cooccur_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                      int32_t v, int rule, int64_t *cooc, int64_t *nhit)
{
    if (!db || !m || nq < 0 || (nq > 0 && (!ichr || !qs || !qe)) || (db->nFiles > 0 && !cooc) || db->nFiles > IGD_COOCCUR_MAX_FILES ||
        (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT))
        return -1;
    const int64_t nF = db->nFiles, nW = (nF + 31) / 32;
    if (nF > 0) memset(cooc, 0, sizeof(int64_t) * (size_t)nF * (size_t)nF);
    if (nhit) *nhit = 0;
    if (nF == 0 || nq == 0) return 0;
    const int64_t step = nq < COOCCUR_CHUNK ? nq : COOCCUR_CHUNK, cw = 2 * ((step + 63) / 64);
    uint32_t *bits = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)step * (size_t)nW);
    uint32_t *cols = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)nF * (size_t)cw);
    int rc = bits && cols ? 0 : -1;
    int64_t hit = 0;
    for (int64_t c0 = 0; c0 < nq && rc == 0; c0 += step) {
        const int64_t n = nq - c0 < step ? nq - c0 : step;
        rc = igdc_membership_host(db, m, ichr + c0, qs + c0, qe + c0, n, v, rule, bits, NULL, &hit);
        if (rc != 0) break;
        memset(cols, 0, sizeof(uint32_t) * (size_t)nF * (size_t)cw);
        for (int64_t r = 0; r < n; r++)
            for (int64_t w = 0; w < nW; w++)
                for (uint32_t x = bits[r * nW + w]; x; x &= x - 1)
                    cols[(w * 32 + __builtin_ctz(x)) * cw + (r >> 5)] |= 1u << (r & 31);
        gram_host(cols, nF, cols, nF, cw, (n + 31) / 32, cooc, nF);
    }
    free(bits); free(cols);
    if (rc == 0 && nhit) *nhit = hit;
    return rc;
}

/* ---- the permutation nulls on the host: what the igd_hip_permute_* entries compute (include/igd_hip.h has the generator and
 * the definitions) -----------------------------------------------------------------------------------------------------------
 * Five statistics have one: support (igdc_permute_host*), support under rigid shifts (igdc_shift_support_host_ov), nearest
 * distances, record values and base pairs (further down, each behind the statistic it permutes).  They share ONE value that says
 * how a permuted row is made (perm_place, below) and ONE driver that shares the rows out over threads (stripe_drive); a statistic
 * adds its refusals, its result buffer, its row function and the copy-out.  The generators alone are igdc_permute_regions_host
 * (kernel igd_permute_regions), igdc_shift_regions_host and igdc_resample_regions_host.  All outputs are DEFINED. */
/* THE PLACEMENT of a call.  Exactly one of four ways: mode CIRCULAR or SHUFFLE on the contigs (ws, offsets and pool NULL), mode
 * WORKSPACE inside the checked table ws, a rigid shift by offsets[r - 1] (the shift entries; mode and seed unused), or mode
 * RESAMPLE, a draw from pool (no ctg_len: nothing is placed).  Every exported entry builds one from its loose arguments in one
 * line; everything below that takes the value. */
typedef struct { const int32_t *ichr, *qs, *qe; int64_t npool; } perm_pool;
typedef struct {
    const int32_t *ctg_len;
    int mode; uint64_t seed;
    const igd_hip_workspace *ws;
    const int32_t *offsets;
    const perm_pool *pool;
} perm_place;

/* the generator's placement itself, on checked arguments: permutations p0 .. p0 + np - 1 of the set */
static void perm_regions_fill(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t nctg, const perm_place *pl,
                              int64_t p0, int64_t np, int32_t *out_qs, int32_t *out_qe)
{
    const igd_hip_workspace *ws = pl->ws;
    for (int64_t p = 0; p < np; p++) {
        const uint64_t base = igd_hip_perm_base(pl->seed, (uint64_t)(p0 + p));
        int32_t *os = out_qs + p * nq, *oe = out_qe + p * nq;
        for (int64_t i = 0; i < nq; i++) {
            os[i] = qs[i]; oe[i] = qe[i];
            if (ws) (void)igd_hip_perm_place_ws(base, ichr[i], i, pl->ctg_len, nctg, ws->w_off, ws->w_start, ws->w_len, ws->w_pre, &os[i], &oe[i]);
            else igd_hip_perm_place(pl->mode, base, ichr[i], i, pl->ctg_len, nctg, &os[i], &oe[i]);
        }
    }
}

int igdc_permute_regions_host_ws(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len, int32_t nctg,
                                 int mode, uint64_t seed, int64_t p0, int64_t np, int32_t *out_qs, int32_t *out_qe,
                                 const igd_hip_workspace *ws)
{
    if (nq < 0 || np < 0 || p0 < 0 || nctg < 0 || (nctg > 0 && !ctg_len) || (nq > 0 && (!ichr || !qs || !qe)) ||
        (nq > 0 && np > 0 && (!out_qs || !out_qe)) || !igd_hip_perm_mode_ok(mode, ws != NULL, 0) ||
        (ws && !igd_hip_workspace_valid(ws, ctg_len, nctg)))
        return -1;
    const perm_place pl = {ctg_len, mode, seed, ws, NULL, NULL};
    perm_regions_fill(ichr, qs, qe, nq, nctg, &pl, p0, np, out_qs, out_qe);
    return 0;
}

int igdc_permute_regions_host(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len, int32_t nctg,
                              int mode, uint64_t seed, int64_t p0, int64_t np, int32_t *out_qs, int32_t *out_qe)
{
    return igdc_permute_regions_host_ws(ichr, qs, qe, nq, ctg_len, nctg, mode, seed, p0, np, out_qs, out_qe, NULL);
}

/* the shift placement (include/igd_hip.h: THE SHIFT), on checked arguments: the set under each of nshift offsets */
static void shift_regions_fill(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len, int32_t nctg,
                               const int32_t *offsets, int64_t nshift, int32_t *out_qs, int32_t *out_qe)
{
    for (int64_t j = 0; j < nshift; j++) {
        int32_t *os = out_qs + j * nq, *oe = out_qe + j * nq;
        for (int64_t i = 0; i < nq; i++) {
            os[i] = qs[i]; oe[i] = qe[i];
            igd_hip_shift_place(offsets[j], ichr[i], ctg_len, nctg, &os[i], &oe[i]);
        }
    }
}

/* the refusals the two shift entries share with the engine's: the arrays, the number of shifts, every offset, the batch limit */
static int shift_args_bad(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len, int32_t nctg,
                          const int32_t *offsets, int64_t nshift)
{
    return nq < 0 || nctg < 0 || (nq > 0 && (!ichr || !qs || !qe)) || (nctg > 0 && !ctg_len) || !offsets || nshift < 1 ||
           nshift > IGD_HIP_SHIFT_MAX || igd_hip_shift_first_bad(offsets, nshift) >= 0 || nq > igd_hip_max_batch();
}

int igdc_shift_regions_host(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len, int32_t nctg,
                            const int32_t *offsets, int64_t nshift, int32_t *out_qs, int32_t *out_qe)
{
    if (shift_args_bad(ichr, qs, qe, nq, ctg_len, nctg, offsets, nshift) || (nq > 0 && (!out_qs || !out_qe)) ||
        (nq > 0 && nshift > (int64_t)INT32_MAX / nq))
        return -1;
    shift_regions_fill(ichr, qs, qe, nq, ctg_len, nctg, offsets, nshift, out_qs, out_qe);
    return 0;
}

/* The pool of a resampling call (include/igd_hip.h: THE DRAW) and the draws themselves, on checked arguments (nq <= npool): draw i
 * of permutation p0 + p is pool region igd_hip_resample_index(base, i, npool), copied as it stands. */
static void resample_regions_fill(const perm_pool *pool, int64_t nq, uint64_t seed, int64_t p0, int64_t np, int32_t *out_ichr,
                                  int32_t *out_qs, int32_t *out_qe)
{
    const int h = igd_hip_resample_bits((uint64_t)pool->npool);
    for (int64_t p = 0; p < np; p++) {
        const uint64_t base = igd_hip_perm_base(seed, (uint64_t)(p0 + p));
        for (int64_t i = 0; i < nq; i++) {
            const uint64_t k = igd_hip_resample_walk(base, (uint64_t)i, (uint64_t)pool->npool, h);
            out_ichr[p * nq + i] = pool->ichr[k];
            out_qs[p * nq + i] = pool->qs[k];
            out_qe[p * nq + i] = pool->qe[k];
        }
    }
}

/* the pool's own refusals, the engine's: the arrays, the batch limit, fewer regions than are drawn */
static int pool_bad(const perm_pool *pool, int64_t nq)
{
    return pool->npool < 0 || (pool->npool > 0 && (!pool->ichr || !pool->qs || !pool->qe)) || pool->npool > igd_hip_max_batch() ||
           pool->npool < nq;
}

int igdc_resample_regions_host(const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, int64_t nq,
                               uint64_t seed, int64_t p0, int64_t np, int32_t *out_ichr, int32_t *out_qs, int32_t *out_qe)
{
    const perm_pool pool = {pool_ichr, pool_qs, pool_qe, npool};
    if (nq < 0 || np < 0 || p0 < 0 || nq > igd_hip_max_batch() || pool_bad(&pool, nq) || (nq > 0 && np > 0 && (!out_ichr || !out_qs || !out_qe)) ||
        (nq > 0 && np > (int64_t)INT32_MAX / nq))
        return -1;
    resample_regions_fill(&pool, nq, seed, p0, np, out_ichr, out_qs, out_qe);
    return 0;
}

/* ---- the workspace table (include/igd_hip.h: THE WORKSPACE) ---------------------------------------------------------------
 * igdc_workspace_build: the segments through igdc_merge_host at gap 0 (one set; it needs a database only for the number of
 * contigs), the runs clipped to [0, ctg_len[c]], per contig ordered by length descending then start ascending, and summed.  The
 * table and its four arrays are ONE allocation (igdc_workspace_free). */
typedef struct { int32_t c, a, l; } ws_seg;
static int ws_seg_cmp(const void *x, const void *y)
{
    const ws_seg *p = (const ws_seg *)x, *q = (const ws_seg *)y;
    if (p->c != q->c) return p->c < q->c ? -1 : 1;
    if (p->l != q->l) return p->l > q->l ? -1 : 1;
    return p->a < q->a ? -1 : p->a > q->a;
}

int igdc_workspace_build(const int32_t *ichr, const int32_t *a, const int32_t *b, int64_t n, const int32_t *ctg_len, int32_t nctg,
                         igd_hip_workspace **out)
{
    if (!out || n < 0 || nctg < 0 || (nctg > 0 && !ctg_len) || (n > 0 && (!ichr || !a || !b))) return -1;
    for (int32_t c = 0; c < nctg; c++) if (ctg_len[c] < 0) return -1;
    igdc_db d;
    memset(&d, 0, sizeof d);
    d.nCtg = nctg;
    const int64_t off[2] = {0, n};
    int64_t moff[2] = {0, 0}, dropped = 0, m = 0;
    int32_t *mr = (int32_t *)malloc((size_t)(n > 0 ? n : 1) * 3 * sizeof *mr);
    ws_seg *g = (ws_seg *)malloc((size_t)(n > 0 ? n : 1) * sizeof *g);
    if (!mr || !g || igdc_merge_host(&d, ichr, a, b, off, 1, 0, mr, mr + n, mr + 2 * n, moff, NULL, &dropped) != 0) { free(mr); free(g); return -1; }
    for (int64_t r = 0; r < moff[1]; r++) {
        const int32_t c = mr[r];
        const int64_t L = ctg_len[c], lo = mr[n + r] < 0 ? 0 : mr[n + r], hi = mr[2 * n + r] > L ? L : mr[2 * n + r];
        if (hi - lo < 1) continue;
        g[m].c = c; g[m].a = (int32_t)lo; g[m].l = (int32_t)(hi - lo);
        m++;
    }
    free(mr);
    qsort(g, (size_t)m, sizeof *g, ws_seg_cmp);
    /* the struct, then w_off (8-byte words), then the three 32-bit arrays */
    const size_t bytes = sizeof(igd_hip_workspace) + ((size_t)nctg + 1) * 8 + ((size_t)m * 3 + (size_t)nctg + 1) * 4;
    char *blk = (char *)malloc(bytes);
    if (!blk) { free(g); return -1; }
    igd_hip_workspace *ws = (igd_hip_workspace *)blk;
    int64_t *w_off = (int64_t *)(blk + sizeof(igd_hip_workspace));
    int32_t *w_start = (int32_t *)(w_off + nctg + 1), *w_len = w_start + m, *w_pre = w_len + m;
    int64_t at = 0;
    for (int32_t c = 0; c < nctg; c++) {
        int64_t sum = 0;
        w_off[c] = at;
        w_pre[at + c] = 0;
        for (; at < m && g[at].c == c; at++) {
            w_start[at] = g[at].a; w_len[at] = g[at].l;
            sum += g[at].l;
            w_pre[at + c + 1] = (int32_t)sum;
        }
    }
    w_off[nctg] = m;
    free(g);
    ws->nctg = nctg; ws->nseg = m; ws->w_off = w_off; ws->w_start = w_start; ws->w_len = w_len; ws->w_pre = w_pre;
    *out = ws;
    return 0;
}

void igdc_workspace_free(igd_hip_workspace *ws) { free(ws); }

int igdc_workspace_valid(const igd_hip_workspace *ws, const int32_t *ctg_len, int32_t nctg) { return igd_hip_workspace_valid(ws, ctg_len, nctg); }

int64_t igdc_workspace_first_unplaceable(const igd_hip_workspace *ws, const int32_t *ctg_len, const int32_t *ichr, const int32_t *qs,
                                         const int32_t *qe, int64_t nq)
{
    return igd_hip_perm_first_unplaceable(ws, ctg_len, ichr, qs, qe, nq);
}

static int ws_span_cmp(const void *x, const void *y)
{
    const int32_t *p = (const int32_t *)x, *q = (const int32_t *)y;
    return p[0] < q[0] ? -1 : p[0] > q[0];
}

int64_t igdc_workspace_outside(const igd_hip_workspace *ws, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq)
{
    if (!ws || nq < 0 || (nq > 0 && (!ichr || !qs || !qe))) return -1;
    /* per contig the segments as (start, end) ordered by start: they are disjoint, so the one that can hold a region is the
     * last that starts at or before it */
    int32_t *sp = (int32_t *)malloc(((size_t)ws->nseg + 1) * 2 * sizeof *sp);
    if (!sp) return -1;
    for (int64_t j = 0; j < ws->nseg; j++) { sp[2 * j] = ws->w_start[j]; sp[2 * j + 1] = ws->w_start[j] + ws->w_len[j]; }
    for (int32_t c = 0; c < ws->nctg; c++) qsort(sp + 2 * ws->w_off[c], (size_t)(ws->w_off[c + 1] - ws->w_off[c]), 2 * sizeof *sp, ws_span_cmp);
    int64_t out = 0;
    for (int64_t i = 0; i < nq; i++) {
        const int32_t c = ichr[i];
        if (c < 0 || c >= ws->nctg) continue;
        int64_t lo = ws->w_off[c], hi = ws->w_off[c + 1];          /* the first segment that starts behind qs[i] */
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (sp[2 * mid] <= qs[i]) lo = mid + 1; else hi = mid;
        }
        out += !(lo > ws->w_off[c] && qe[i] >= qs[i] && qe[i] <= sp[2 * (lo - 1) + 1]);
    }
    free(sp);
    return out;
}

int igdc_read_workspace(const igdc_db *db, const char *path, const int32_t *ctg_len, igd_hip_workspace **out)
{
    igdc_queries q;
    if (!db || !path || !out) return -1;
    if (igdc_read_queries(db, path, 1, &q) != 0) return -1;
    const int rc = igdc_workspace_build(q.ichr, q.qs, q.qe, q.n, ctg_len, db->nCtg, out);
    igdc_queries_free(&q);
    return rc == 0 ? 0 : -2;
}

/* igd_hip_perm_first_bad (include/igd_hip.h) as a symbol of the library */
int64_t igdc_permute_first_bad(const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len, int32_t nctg)
{
    return igd_hip_perm_first_bad(ichr, qs, qe, nq, ctg_len, nctg);
}

/* the refusals the nulls share (each adds its own in front): the set and the contig lengths, a mode the call can run, the
 * number of permutations, the generator's bounds on the regions, and under a workspace a table that is valid for the database's
 * contigs and has a segment for every region on a known contig */
static int perm_args_bad(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                         int64_t nperm, const perm_place *pl)
{
    const int32_t *ctg_len = pl->ctg_len;
    const igd_hip_workspace *ws = pl->ws;
    /* resampling: nothing is placed, so there are no contig lengths and no region is validated; the pool has its own bounds */
    if (pl->pool || pl->mode == IGD_HIP_PERM_RESAMPLE)
        return !igd_hip_perm_mode_ok(pl->mode, ws != NULL, pl->pool != NULL) || !db || !m || nq < 0 || (nq > 0 && (!ichr || !qs || !qe)) ||
               nperm < 1 || nperm > IGD_HIP_PERM_MAX || nq > igd_hip_max_batch() || pool_bad(pl->pool, nq);
    return !db || !m || nq < 0 || (nq > 0 && (!ichr || !qs || !qe)) || (!ctg_len && db->nCtg > 0) || !igd_hip_perm_mode_ok(pl->mode, ws != NULL, 0) ||
           nperm < 1 || nperm > IGD_HIP_PERM_MAX || nq > igd_hip_max_batch() || igdc_permute_first_bad(ichr, qs, qe, nq, ctg_len, db->nCtg) >= 0 ||
           (ws && (!igd_hip_workspace_valid(ws, ctg_len, db->nCtg) || igdc_workspace_first_unplaceable(ws, ctg_len, ichr, qs, qe, nq) >= 0));
}

/* ---- THE null driver: the one place that shares the rows of a null out over threads ----------------------------------------
 * Row 0 is the set as given, row r > 0 what the placement makes of it for r - 1 (permutation, draw or shift r - 1), filled into
 * the thread's own arrays.  A statistic declares its thread's job with a perm_stripe as the FIRST member, asks stripe_threads
 * how many there will be, sets its own fields of job[0 .. T) and calls stripe_drive, which gives every thread its arrays (the
 * permuted set, `extra` words of the statistic's choosing, the drawn contigs under a pool) and a tile buffer, runs thread k of
 * T over the rows first + k, first + k + T, .. below nrows, each handed to the statistic's row function until one answers
 * nonzero (a tile that could not be read), and frees what it took.  Results, their copy-out, the statistic's own refusals and
 * whether the threads run at all at an empty shape stay with the statistic. */
typedef int (*perm_row_fn)(void *job, int64_t r, const int32_t *s, const int32_t *e);
typedef struct {
    const igdc_db *db; const igdc_map *m;
    const int32_t *ichr, *qs, *qe;
    int64_t nq, first, nrows;
    perm_place pl;
    perm_row_fn row;
    int32_t *ps, *pe, *pc, *extra;      /* the permuted set; the drawn contigs (pool only); the statistic's words */
    const int32_t *rowc;                /* the contigs of the row in hand: ichr, or pc for a draw */
    tilebuf tb;                         /* for the row functions that walk tiles themselves */
    int k, T, failed;
} perm_stripe;

static void *stripe_run(void *job)
{
    perm_stripe *S = (perm_stripe *)job;
    tb_open(&S->tb);
    for (int64_t r = S->first + S->k; r < S->nrows && !S->failed; r += S->T) {
        const int32_t *s = S->qs, *e = S->qe;
        S->rowc = S->ichr;
        if (r > 0) {
            if (S->pl.pool) {
                resample_regions_fill(S->pl.pool, S->nq, S->pl.seed, r - 1, 1, S->pc, S->ps, S->pe);
                S->rowc = S->pc;
            }
            else if (S->pl.offsets) shift_regions_fill(S->ichr, S->qs, S->qe, S->nq, S->pl.ctg_len, S->db->nCtg, S->pl.offsets + (r - 1), 1, S->ps, S->pe);
            else perm_regions_fill(S->ichr, S->qs, S->qe, S->nq, S->db->nCtg, &S->pl, r - 1, 1, S->ps, S->pe);
            s = S->ps; e = S->pe;
        }
        if (S->row(job, r, s, e)) S->failed = 1;
    }
    tb_close(&S->tb);
    return NULL;
}

/* the threads a null of `rows` permuted rows over nq regions is worth: never more than there are rows */
static int stripe_threads(int64_t nq, int64_t rows)
{
    const int T = host_threads(nq * rows > 0 ? nq * rows : 1);
    return T > rows ? (int)rows : T;
}

/* T jobs of `size` bytes at `jobs` (T from stripe_threads(nq, nrows - first)), each thread with 2 nq + extra words of its own.
 * 0, or -1 when memory could not be had or a row function failed. */
static int stripe_drive(void *jobs, size_t size, int T, int64_t extra, const igdc_db *db, const igdc_map *m, const int32_t *ichr,
                        const int32_t *qs, const int32_t *qe, int64_t nq, const perm_place *pl, int64_t first, int64_t nrows, perm_row_fn row)
{
    const size_t per = 2 * (size_t)nq + (size_t)extra;
    int32_t *w = (int32_t *)malloc(sizeof(int32_t) * ((size_t)T * per + 1));
    int32_t *pc = pl->pool ? (int32_t *)malloc(sizeof(int32_t) * ((size_t)T * (size_t)nq + 1)) : NULL;
    int rc = w && (pc || !pl->pool) ? 0 : -1;
    for (int k = 0; k < T && rc == 0; k++) {
        perm_stripe *S = (perm_stripe *)((char *)jobs + (size_t)k * size);
        S->db = db; S->m = m; S->ichr = ichr; S->qs = qs; S->qe = qe;
        S->nq = nq; S->first = first; S->nrows = nrows; S->pl = *pl; S->row = row;
        S->ps = w + (size_t)k * per; S->pe = S->ps + nq; S->extra = S->pe + nq;
        S->pc = pc ? pc + (size_t)k * (size_t)nq : NULL; S->rowc = ichr;
        S->k = k; S->T = T; S->failed = 0;
    }
    if (rc == 0) {
        run_threads(stripe_run, jobs, size, T);
        for (int k = 0; k < T; k++) if (((perm_stripe *)((char *)jobs + (size_t)k * size))->failed) rc = -1;
    }
    free(w); free(pc);
    return rc;
}

/* igdc_permute_host's thread: rows 1 .. nperm, each walked with the per-query code of igdc_support_host and folded into the
 * thread's own statistics */
typedef struct {
    perm_stripe s;
    int32_t v; int rule;
    const int64_t *observed;
    int64_t *acc;           /* sum, sumsq, n_ge, n_le, min, max: nFiles + 1 words each */
    int64_t *row, *last;
    const igd_hip_min_overlap *mo;      /* an active minimum overlap, or NULL */
} perm_job;

static int perm_row(void *job, int64_t r, const int32_t *s, const int32_t *e)
{
    perm_job *P = (perm_job *)job;
    const int64_t nF = P->s.db->nFiles, nC = nF + 1;
    (void)r;
    memset(P->row, 0, sizeof(int64_t) * (size_t)nC);
    memset(P->last, 0, sizeof(int64_t) * (size_t)nC);
    host_job J;
    job_init(&J, JOB_SUPPORT, P->s.db, P->s.m, P->s.rowc, s, e, 0, P->s.nq, P->v, P->rule);
    J.hits = P->row; J.last = P->last; J.mo = P->mo;
    host_run(&J);
    if (J.io_failed) return 1;
    P->row[nF] = J.total;
    for (int64_t f = 0; f < nC; f++) {
        const int64_t x = P->row[f];
        P->acc[f] += x;
        P->acc[nC + f] += x * x;
        P->acc[2 * nC + f] += x >= P->observed[f];
        P->acc[3 * nC + f] += x <= P->observed[f];
        if (x < P->acc[4 * nC + f]) P->acc[4 * nC + f] = x;
        if (x > P->acc[5 * nC + f]) P->acc[5 * nC + f] = x;
    }
    return 0;
}

int igdc_permute_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                      const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed,
                      int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax)
{
    return igdc_permute_host_ws(db, m, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax, NULL, NULL);
}

int igdc_permute_host_ov(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                         const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed,
                         int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax,
                         const igd_hip_min_overlap *min_overlap)
{
    return igdc_permute_host_ws(db, m, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax,
                                min_overlap, NULL);
}

/* the body of the igdc_permute_host entries: the set as given through igdc_support_host_ov, then rows 1 .. nperm */
static int permute_host_run(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                            const perm_place *pl, int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq,
                            int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax, const igd_hip_min_overlap *min_overlap)
{
    const igd_hip_min_overlap *mo = igd_hip_min_overlap_active(min_overlap) ? min_overlap : NULL;
    if (!igd_hip_min_overlap_valid(min_overlap) || !observed || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT) ||
        perm_args_bad(db, m, ichr, qs, qe, nq, nperm, pl) ||
        (unsigned __int128)nperm * (unsigned __int128)nq * (unsigned __int128)nq >= (unsigned __int128)1 << 63)
        return -1;
    const int64_t nF = db->nFiles, nC = nF + 1;
    const int T = stripe_threads(nq, nperm);
    /* per thread: 6 statistics, row and stamps (8 nC words); + the observed row */
    int64_t *w = (int64_t *)calloc((size_t)T * 8 * (size_t)nC + (size_t)nC, sizeof(int64_t));
    int rc = w ? 0 : -1;
    int64_t *obs = w ? w + (size_t)T * 8 * (size_t)nC : NULL;
    if (rc == 0 && nq > 0) rc = igdc_support_host_ov(db, m, ichr, qs, qe, nq, v, rule, obs, &obs[nF], mo);
    perm_job job[HOST_MAX_THREADS];
    for (int k = 0; k < T && rc == 0; k++) {
        job[k].v = v; job[k].rule = rule; job[k].observed = obs; job[k].mo = mo;
        job[k].acc = w + (size_t)k * 8 * (size_t)nC;
        job[k].row = job[k].acc + 6 * nC; job[k].last = job[k].row + nC;
        for (int64_t f = 0; f < nC; f++) { job[k].acc[4 * nC + f] = INT64_MAX; job[k].acc[5 * nC + f] = INT64_MIN; }
    }
    if (rc == 0) rc = stripe_drive(job, sizeof job[0], T, 0, db, m, ichr, qs, qe, nq, pl, 1, nperm + 1, perm_row);
    if (rc == 0) {
        int64_t *a0 = job[0].acc;
        for (int k = 1; k < T; k++)
            for (int64_t f = 0; f < nC; f++) {
                const int64_t *a = job[k].acc;
                for (int s = 0; s < 4; s++) a0[s * nC + f] += a[s * nC + f];
                if (a[4 * nC + f] < a0[4 * nC + f]) a0[4 * nC + f] = a[4 * nC + f];
                if (a[5 * nC + f] > a0[5 * nC + f]) a0[5 * nC + f] = a[5 * nC + f];
            }
        int64_t *const out[6] = {sum, sumsq, n_ge, n_le, pmin, pmax};
        memcpy(observed, obs, sizeof(int64_t) * (size_t)nC);
        for (int s = 0; s < 6; s++) if (out[s]) memcpy(out[s], a0 + s * nC, sizeof(int64_t) * (size_t)nC);
    }
    free(w);
    return rc;
}

int igdc_permute_host_ws(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                         const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed,
                         int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax,
                         const igd_hip_min_overlap *min_overlap, const igd_hip_workspace *ws)
{
    const perm_place pl = {ctg_len, mode, seed, ws, NULL, NULL};
    return permute_host_run(db, m, ichr, qs, qe, nq, &pl, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax, min_overlap);
}

int igdc_permute_host_rs(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                         const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                         int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le,
                         int64_t *pmin, int64_t *pmax, const igd_hip_min_overlap *min_overlap)
{
    const perm_pool pool = {pool_ichr, pool_qs, pool_qe, npool};
    const perm_place pl = {NULL, IGD_HIP_PERM_RESAMPLE, seed, NULL, NULL, &pool};
    return permute_host_run(db, m, ichr, qs, qe, nq, &pl, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax, min_overlap);
}

/* igdc_shift_support_host_ov's thread: rows 1 .. nshift of the stripe (row r is the set moved by offsets[r - 1]), each walked
 * with the per-query code of igdc_support_host and written as row r - 1 of the call's own matrix */
typedef struct {
    perm_stripe s;
    int32_t v; int rule;
    int64_t *out, *last;                /* the call's matrix, nFiles + 1 words per row; the thread's stamps */
    const igd_hip_min_overlap *mo;      /* an active minimum overlap, or NULL */
} shift_job;

static int shift_row(void *job, int64_t r, const int32_t *s, const int32_t *e)
{
    shift_job *P = (shift_job *)job;
    const int64_t nF = P->s.db->nFiles, nC = nF + 1;
    int64_t *row = P->out + (r - 1) * nC;
    memset(row, 0, sizeof(int64_t) * (size_t)nC);
    memset(P->last, 0, sizeof(int64_t) * (size_t)nC);
    host_job J;
    job_init(&J, JOB_SUPPORT, P->s.db, P->s.m, P->s.rowc, s, e, 0, P->s.nq, P->v, P->rule);
    J.hits = row; J.last = P->last; J.mo = P->mo;
    host_run(&J);
    if (J.io_failed) return 1;
    row[nF] = J.total;
    return 0;
}

int igdc_shift_support_host_ov(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const int32_t *ctg_len, const int32_t *offsets, int64_t nshift, int32_t v, int rule, int64_t *shifted,
                               const igd_hip_min_overlap *min_overlap)
{
    const igd_hip_min_overlap *mo = igd_hip_min_overlap_active(min_overlap) ? min_overlap : NULL;
    if (!igd_hip_min_overlap_valid(min_overlap) || !db || !m || !shifted || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT) ||
        shift_args_bad(ichr, qs, qe, nq, ctg_len, db->nCtg, offsets, nshift) || igdc_permute_first_bad(ichr, qs, qe, nq, ctg_len, db->nCtg) >= 0)
        return -1;
    const int64_t nF = db->nFiles, nC = nF + 1;
    if (nq == 0 || nF == 0) {
        memset(shifted, 0, sizeof(int64_t) * (size_t)(nshift * nC));
        return 0;
    }
    const perm_place pl = {ctg_len, 0, 0, NULL, offsets, NULL};
    const int T = stripe_threads(nq, nshift);
    /* the call's matrix, then per thread the stamps (nC words) */
    int64_t *w = (int64_t *)calloc((size_t)(nshift + T) * (size_t)nC, sizeof(int64_t));
    int rc = w ? 0 : -1;
    shift_job job[HOST_MAX_THREADS];
    for (int k = 0; k < T && rc == 0; k++) {
        job[k].v = v; job[k].rule = rule; job[k].mo = mo;
        job[k].out = w; job[k].last = w + (size_t)(nshift + k) * (size_t)nC;
    }
    if (rc == 0) rc = stripe_drive(job, sizeof job[0], T, 0, db, m, ichr, qs, qe, nq, &pl, 1, nshift + 1, shift_row);
    if (rc == 0) memcpy(shifted, w, sizeof(int64_t) * (size_t)(nshift * nC));
    free(w);
    return rc;
}

/* mean, sd, z and the two one-sided permutation p-values (as -log10) of n columns; igd_core.h has the formulas.  sqrt by
 * weak reference, as log10 above.  0, or -1 without a C math library. */
#pragma weak sqrt
int igdc_perm_summary(const int64_t *observed, const int64_t *sum, const int64_t *sumsq, const int64_t *n_ge, const int64_t *n_le,
                       int64_t nperm, int64_t n, double *mean, double *sd, double *z, double *nlog10_p_upper, double *nlog10_p_lower)
{
    const double P = (double)nperm, nan = __builtin_nan("");
    if (!sqrt || !log10 || nperm < 1 || n < 0 || (n > 0 && (!observed || !sum || !sumsq || !n_ge || !n_le))) return -1;
    for (int64_t f = 0; f < n; f++) {
        const double mu = (double)sum[f] / P;
        double s = nan;
        if (nperm > 1) {
            const __int128 num = (__int128)nperm * (__int128)sumsq[f] - (__int128)sum[f] * (__int128)sum[f];
            s = sqrt((double)num / (P * (P - 1.0)));
        }
        if (mean) mean[f] = mu;
        if (sd) sd[f] = s;
        if (z) z[f] = (s != s || s == 0.0) ? nan : ((double)observed[f] - mu) / s;
        if (nlog10_p_upper) nlog10_p_upper[f] = 0.0 - log10((double)(n_ge[f] + 1) / (P + 1.0));
        if (nlog10_p_lower) nlog10_p_lower[f] = 0.0 - log10((double)(n_le[f] + 1) / (P + 1.0));
    }
    return 0;
}

/* ---- nearest record per dataset within a window: the entries (one_region_keys has the walk) ------------------------------ */
static int nearest_rows_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                             int32_t window, int32_t v, int sgn, int32_t *dist, int32_t *dmin)
{
    if (!db || !m || nq < 0 || !igd_hip_nearest_window_valid(window) || (nq > 0 && (!ichr || !qs || !qe || (!dist && db->nFiles > 0)))) return -1;
    const int T = host_threads(nq);
    host_job job[HOST_MAX_THREADS];
    int32_t none = 0;                        /* (a database without files: rows of no words) */
    /* rows are disjoint per region: every thread writes its regions' rows straight into the caller's */
    jobs_split(job, T, JOB_NEAREST, db, m, ichr, qs, qe, nq, v, 0);
    for (int k = 0; k < T; k++) { job[k].window = window; job[k].sgn = sgn; job[k].rowa = dist ? dist : &none; job[k].mina = dmin; }
    return jobs_run(job, T, NULL) ? -1 : 0;
}

int igdc_nearest_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                      int32_t window, int32_t v, int32_t *dist, int32_t *dmin)
{
    return nearest_rows_host(db, m, ichr, qs, qe, nq, window, v, 0, dist, dmin);
}

int igdc_nearest_signed_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                             int32_t window, int32_t v, int32_t *sdist, int32_t *sdmin)
{
    return nearest_rows_host(db, m, ichr, qs, qe, nq, window, v, 1, sdist, sdmin);
}

/* ---- per-set statistics of per-region rows: the loop over chunks of regions ----------------------------------------------
 * The rows of a whole set list need not fit in memory, so they are computed for chunks of regions -- as many as HOST_ROW_BYTES
 * hold (IGD_HOST_ROW_BYTES overrides it: for tests of the seam) -- by the entry's row computer, and every region of the chunk
 * is handed with its set to the entry's fold.  The set index runs along with the regions; empty sets are passed over.  A *_sets
 * entry is its refusals, a row computer and a fold. */
#define HOST_ROW_BYTES ((int64_t)32 << 20)
typedef int (*chunk_rows_fn)(void *ctx, int64_t c0, int64_t n);        /* the rows of regions [c0, c0 + n); 0 or -1 */
typedef void (*chunk_fold_fn)(void *ctx, int32_t set, int64_t i);       /* region i of the chunk belongs to `set` */

static int64_t chunk_regions(int64_t bytes_per_region, int64_t nq)
{
    const char *e = getenv("IGD_HOST_ROW_BYTES");
    const long long x = e && *e ? atoll(e) : 0;
    const int64_t chunk = (x > 0 ? (int64_t)x : HOST_ROW_BYTES) / bytes_per_region;
    return chunk < 1 ? 1 : chunk > nq ? nq : chunk;
}

static int set_chunks(const int64_t *set_off, int32_t nsets, int64_t chunk, chunk_rows_fn rows, chunk_fold_fn fold, void *ctx)
{
    const int64_t nq = nsets > 0 ? set_off[nsets] : 0;
    int32_t k = 0;
    for (int64_t c0 = 0; c0 < nq; c0 += chunk) {
        const int64_t n = nq - c0 < chunk ? nq - c0 : chunk;
        const int rc = rows(ctx, c0, n);
        if (rc != 0) return rc;
        for (int64_t i = 0; i < n; i++) {
            while (set_off[k + 1] <= c0 + i) k++;                          /* (empty sets are passed over) */
            fold(ctx, k, i);
        }
    }
    return 0;
}

/* igdc_nearest_sets_host and igdc_nearest_hist_host: the (signed) distance rows of a chunk, each word counted into its set's
 * three statistics, or into its bin of its set's histogram */
typedef struct {
    const igdc_db *db; const igdc_map *m;
    const int32_t *ichr, *qs, *qe;
    int32_t window, v; int sgn;
    int32_t *dist, *dmin;                           /* the chunk's rows */
    int64_t *n_within, *n_overlap, *sum_dist;       /* nearest_sets' outputs (each may be NULL) */
    const int32_t *edges; int32_t ne; int64_t *hist;
} nearest_sets_ctx;

static int nearest_sets_rows(void *ctx, int64_t c0, int64_t n)
{
    nearest_sets_ctx *c = (nearest_sets_ctx *)ctx;
    return nearest_rows_host(c->db, c->m, c->ichr + c0, c->qs + c0, c->qe + c0, n, c->window, c->v, c->sgn, c->dist, c->dmin);
}
static void nearest_sets_fold(void *ctx, int32_t k, int64_t i)
{
    nearest_sets_ctx *c = (nearest_sets_ctx *)ctx;
    const int64_t nf = c->db->nFiles, nC = nf + 1;
    const int32_t *row = c->dist + (size_t)i * (size_t)nf;
    const size_t o = (size_t)k * (size_t)nC;
    for (int64_t f = 0; f < nC; f++) {
        const int32_t d = f < nf ? row[f] : c->dmin[i];
        if (d < 0) continue;
        if (c->n_within) c->n_within[o + f]++;
        if (c->n_overlap && d == 0) c->n_overlap[o + f]++;
        if (c->sum_dist) c->sum_dist[o + f] += d;
    }
}
static void nearest_hist_fold(void *ctx, int32_t k, int64_t i)
{
    nearest_sets_ctx *c = (nearest_sets_ctx *)ctx;
    const int64_t nf = c->db->nFiles, nC = nf + 1;
    const int32_t *row = c->dist + (size_t)i * (size_t)nf;
    int64_t *h = c->hist + (size_t)k * (size_t)(c->ne + 1) * (size_t)nC;
    for (int64_t f = 0; f < nC; f++) {
        const int32_t x = f < nf ? row[f] : c->dmin[i];
        if (x != IGD_HIP_NEAREST_NO_RECORD) h[(size_t)igd_hip_nearest_bin(c->edges, c->ne, x) * (size_t)nC + (size_t)f]++;
    }
}
/* allocates the chunk's rows, runs the chunks with `fold`, frees */
static int nearest_sets_run(nearest_sets_ctx *c, const int64_t *set_off, int32_t nsets, chunk_fold_fn fold)
{
    const int64_t nf = c->db->nFiles, chunk = chunk_regions(4 * (nf > 0 ? nf : 1), nsets > 0 ? set_off[nsets] : 0);
    c->dist = (int32_t *)malloc(sizeof(int32_t) * (size_t)(chunk * nf + 1));
    c->dmin = (int32_t *)malloc(sizeof(int32_t) * (size_t)(chunk + 1));
    const int rc = c->dist && c->dmin ? set_chunks(set_off, nsets, chunk, nearest_sets_rows, fold, c) : -1;
    free(c->dist); free(c->dmin);
    return rc;
}

int igdc_nearest_sets_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                           const int64_t *set_off, int32_t nsets, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap,
                           int64_t *sum_dist)
{
    if (!db || !m || !igd_hip_nearest_window_valid(window) || set_off_bad(set_off, nsets, ichr, qs, qe)) return -1;
    nearest_sets_ctx c = {db, m, ichr, qs, qe, window, v, 0, NULL, NULL, n_within, n_overlap, sum_dist, NULL, 0, NULL};
    int64_t *outs[3] = {n_within, n_overlap, sum_dist};
    for (int i = 0; i < 3; i++) if (outs[i]) memset(outs[i], 0, sizeof(int64_t) * (size_t)nsets * (size_t)(db->nFiles + 1));
    return nearest_sets_run(&c, set_off, nsets, nearest_sets_fold);
}

int igdc_nearest_hist_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                           const int64_t *set_off, int32_t nsets, int32_t window, int32_t v, const int32_t *edges, int32_t ne,
                           int64_t *hist)
{
    if (!db || !m || !igd_hip_nearest_window_valid(window) || !igd_hip_nearest_edges_valid(edges, ne) || (nsets > 0 && !hist) ||
        set_off_bad(set_off, nsets, ichr, qs, qe)) return -1;
    nearest_sets_ctx c = {db, m, ichr, qs, qe, window, v, 1, NULL, NULL, NULL, NULL, NULL, edges, ne, hist};
    if (nsets > 0) memset(hist, 0, sizeof(int64_t) * (size_t)nsets * (size_t)(ne + 1) * (size_t)(db->nFiles + 1));
    return nearest_sets_run(&c, set_off, nsets, nearest_hist_fold);
}

/* ---- flanking records per dataset and the relative-distance histogram: the entries (one_region_flanks has the walk) ------ */
int igdc_flank_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                    int32_t window, int measure, int32_t v, int32_t *up, int32_t *down, int32_t *upmin, int32_t *downmin)
{
    if (!db || !m || nq < 0 || !igd_hip_nearest_window_valid(window) || !igd_hip_flank_measure_valid(measure) ||
        (nq > 0 && (!ichr || !qs || !qe || ((!up || !down) && db->nFiles > 0)))) return -1;
    const int T = host_threads(nq);
    host_job job[HOST_MAX_THREADS];
    int32_t none[2] = {0, 0};                /* (a database without files: rows of no words) */
    /* rows are disjoint per region: every thread writes its regions' rows straight into the caller's */
    jobs_split(job, T, JOB_FLANK, db, m, ichr, qs, qe, nq, v, 0);
    for (int k = 0; k < T; k++) {
        job[k].window = window; job[k].measure = measure;
        job[k].rowa = up ? up : &none[0]; job[k].rowb = down ? down : &none[1]; job[k].mina = upmin; job[k].minb = downmin;
    }
    return jobs_run(job, T, NULL) ? -1 : 0;
}

/* the two rows of a chunk of regions (igdc_flank_host), each flanked pair counted into its bin of its set's histogram */
typedef struct {
    const igdc_db *db; const igdc_map *m;
    const int32_t *ichr, *qs, *qe;
    int32_t window, v, nbins; int measure;
    int32_t *up, *down, *upmin, *downmin;           /* the chunk's rows */
    int64_t *hist;
} reldist_ctx;

static int reldist_rows(void *ctx, int64_t c0, int64_t n)
{
    reldist_ctx *c = (reldist_ctx *)ctx;
    return igdc_flank_host(c->db, c->m, c->ichr + c0, c->qs + c0, c->qe + c0, n, c->window, c->measure, c->v, c->up, c->down, c->upmin, c->downmin);
}
static void reldist_fold(void *ctx, int32_t k, int64_t i)
{
    reldist_ctx *c = (reldist_ctx *)ctx;
    const int64_t nf = c->db->nFiles, nC = nf + 1;
    int64_t *h = c->hist + (size_t)k * (size_t)c->nbins * (size_t)nC;
    for (int64_t f = 0; f < nC; f++) {
        const int32_t u = f < nf ? c->up[(size_t)i * (size_t)nf + (size_t)f] : c->upmin[i];
        const int32_t d = f < nf ? c->down[(size_t)i * (size_t)nf + (size_t)f] : c->downmin[i];
        if (igd_hip_flank_flanked(u, d)) h[(size_t)igd_hip_flank_bin(c->nbins, u, d) * (size_t)nC + (size_t)f]++;
    }
}

int igdc_flank_reldist_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                            const int64_t *set_off, int32_t nsets, int32_t window, int measure, int32_t v, int32_t nbins, int64_t *hist)
{
    if (!db || !m || !igd_hip_nearest_window_valid(window) || !igd_hip_flank_measure_valid(measure) || !igd_hip_flank_bins_valid(nbins) ||
        (nsets > 0 && !hist) || set_off_bad(set_off, nsets, ichr, qs, qe)) return -1;
    const int64_t nf = db->nFiles, chunk = chunk_regions(8 * (nf > 0 ? nf : 1), nsets > 0 ? set_off[nsets] : 0);
    int32_t *rows = (int32_t *)malloc(sizeof(int32_t) * (size_t)(2 * chunk * nf + 1)), *mins = (int32_t *)malloc(sizeof(int32_t) * (size_t)(2 * chunk + 1));
    if (!rows || !mins) { free(rows); free(mins); return -1; }
    reldist_ctx c = {db, m, ichr, qs, qe, window, v, nbins, measure, rows, rows + chunk * nf, mins, mins + chunk, hist};
    if (nsets > 0) memset(hist, 0, sizeof(int64_t) * (size_t)nsets * (size_t)nbins * (size_t)(nf + 1));
    const int rc = set_chunks(set_off, nsets, chunk, reldist_rows, reldist_fold, &c);
    free(rows); free(mins);
    return rc;
}

int igdc_nearest_summary(const int64_t *n_within, const int64_t *sum_dist, int64_t n, double *mean)
{
    if (n < 0 || (n > 0 && (!n_within || !sum_dist || !mean))) return -1;
    for (int64_t i = 0; i < n; i++) mean[i] = n_within[i] > 0 ? (double)sum_dist[i] / (double)n_within[i] : __builtin_nan("");
    return 0;
}

/* ---- values of the overlapping records per region and dataset: the entries (one_region_map has the walk) ----------------- */
static int map_op_ok(const igdc_db *db, int op) { return igd_hip_map_op_valid(op) && (op == IGD_HIP_MAP_COUNT || db->gType == 1); }

int igdc_map_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int op,
                  int32_t v, int32_t *count, int64_t *agg)
{
    if (!db || !m || nq < 0 || !map_op_ok(db, op)) return -1;
    if (nq > 0 && (!ichr || !qs || !qe || (db->nFiles > 0 && (!count || (!agg && op != IGD_HIP_MAP_COUNT))))) return -1;
    const int T = host_threads(nq);
    host_job job[HOST_MAX_THREADS];
    int32_t none = 0;                        /* (a database without files: rows of no words) */
    /* rows are disjoint per region: every thread writes its regions' rows straight into the caller's */
    jobs_split(job, T, JOB_MAP, db, m, ichr, qs, qe, nq, v, 0);
    for (int k = 0; k < T; k++) { job[k].op = op; job[k].rowa = count ? count : &none; job[k].agg = db->nFiles > 0 ? agg : NULL; }
    return jobs_run(job, T, NULL) ? -1 : 0;
}

/* the count and agg rows of a chunk of regions (igdc_map_host), each region with a record counted into its set's sums */
typedef struct {
    const igdc_db *db; const igdc_map *m;
    const int32_t *ichr, *qs, *qe;
    int op; int32_t v;
    int32_t *count; int64_t *agg;                   /* the chunk's rows */
    int64_t *n_hit, *pairs, *agg_sum;               /* (each may be NULL) */
} map_sets_ctx;

static int map_sets_rows(void *ctx, int64_t c0, int64_t n)
{
    map_sets_ctx *c = (map_sets_ctx *)ctx;
    return igdc_map_host(c->db, c->m, c->ichr + c0, c->qs + c0, c->qe + c0, n, c->op, c->v, c->count, c->agg);
}
static void map_sets_fold(void *ctx, int32_t k, int64_t i)
{
    map_sets_ctx *c = (map_sets_ctx *)ctx;
    const int64_t nf = c->db->nFiles;
    const size_t r = (size_t)i * (size_t)nf, o = (size_t)k * (size_t)nf;
    for (int64_t f = 0; f < nf; f++) {
        if (c->count[r + f] == 0) continue;
        if (c->n_hit) c->n_hit[o + f]++;
        if (c->pairs) c->pairs[o + f] += c->count[r + f];
        if (c->agg_sum) c->agg_sum[o + f] = (int64_t)((uint64_t)c->agg_sum[o + f] + (uint64_t)c->agg[r + f]);
    }
}

int igdc_map_sets_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                       const int64_t *set_off, int32_t nsets, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    if (!db || !m || nsets < 0 || !map_op_ok(db, op) || set_off_bad(set_off, nsets, ichr, qs, qe)) return -1;
    const int64_t nf = db->nFiles, chunk = chunk_regions(12 * (nf > 0 ? nf : 1), nsets > 0 ? set_off[nsets] : 0);
    int32_t *count = (int32_t *)malloc(sizeof(int32_t) * (size_t)(chunk * nf + 1));
    int64_t *agg = (int64_t *)malloc(sizeof(int64_t) * (size_t)(chunk * nf + 1));
    if (!count || !agg) { free(count); free(agg); return -1; }
    map_sets_ctx c = {db, m, ichr, qs, qe, op, v, count, agg, n_hit, pairs, agg_sum};
    int64_t *outs[3] = {n_hit, pairs, agg_sum};
    for (int i = 0; i < 3; i++) if (outs[i]) memset(outs[i], 0, sizeof(int64_t) * (size_t)nsets * (size_t)nf);
    const int rc = set_chunks(set_off, nsets, chunk, map_sets_rows, map_sets_fold, &c);
    free(count); free(agg);
    return rc;
}

int igdc_map_summary(const int64_t *n_hit, const int64_t *pairs, const int64_t *agg_sum, int64_t n, int op, double *mean_region,
                     double *mean_pair)
{
    if (n < 0 || !igd_hip_map_op_valid(op) || (n > 0 && (!n_hit || !pairs || !agg_sum || !mean_region))) return -1;
    for (int64_t i = 0; i < n; i++) {
        mean_region[i] = n_hit[i] > 0 ? (double)agg_sum[i] / (double)n_hit[i] : __builtin_nan("");
        if (mean_pair) mean_pair[i] = op == IGD_HIP_MAP_SUM && pairs[i] > 0 ? (double)agg_sum[i] / (double)pairs[i] : __builtin_nan("");
    }
    return 0;
}

/* ---- permutation null of the nearest-record distances (what igd_hip_permute_nearest computes) ----------------------------
 * Row 0 is the set as given, row p + 1 permutation p of igdc_permute_regions_host's generator (stripe_run); a row is
 * igdc_nearest_sets_host's walk over its regions (one_region_nearest) summed into the three statistics.  Each thread has its
 * own permuted arrays, distance row and tile buffer; the rows are disjoint.  Everything is computed into a buffer and copied out
 * at the end: -1 (a refused argument, a tile that could not be read) writes nothing. */
typedef struct {
    perm_stripe s;
    int32_t window, v; int use_v;
    int64_t *res;           /* three matrices of nrows x (nFiles + 1) */
} pnear_job;

static int pnear_row(void *job, int64_t r, const int32_t *s, const int32_t *e)
{
    pnear_job *P = (pnear_job *)job;
    const int64_t nF = P->s.db->nFiles, nC = nF + 1;
    int64_t *nw = P->res + r * nC, *no = nw + P->s.nrows * nC, *sd = no + P->s.nrows * nC;
    int32_t *row = P->s.extra;                                             /* one distance row */
    for (int64_t i = 0; i < P->s.nq && !P->s.tb.failed; i++) {
        const int32_t dm = one_region_nearest(P->s.db, P->s.m, &P->s.tb, P->s.rowc[i], s[i], e[i], P->window, P->v, P->use_v, row);
        if (dm < 0) continue;                                          /* (no record within the window: the row is all -1) */
        for (int64_t f = 0; f < nC; f++) {
            const int32_t d = f < nF ? row[f] : dm;
            if (d < 0) continue;
            nw[f]++;
            no[f] += d == 0;
            sd[f] += d;
        }
    }
    return P->s.tb.failed;
}

int igdc_permute_nearest_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                              const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t window, int32_t v,
                              int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist)
{
    return igdc_permute_nearest_host_ws(db, m, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, window, v, n_within, n_overlap, sum_dist, NULL);
}

/* the body of the igdc_permute_nearest_host entries: per thread a distance row of nFiles words */
static int permute_nearest_host_run(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                    const perm_place *pl, int64_t nperm, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap,
                                    int64_t *sum_dist)
{
    if (!igd_hip_nearest_window_valid(window) || perm_args_bad(db, m, ichr, qs, qe, nq, nperm, pl)) return -1;
    const int64_t nF = db->nFiles, nC = nF + 1, R = nperm + 1;
    const int T = stripe_threads(nq, R);
    int64_t *res = (int64_t *)calloc((size_t)(3 * R * nC), sizeof(int64_t));
    int rc = res ? 0 : -1;
    pnear_job job[HOST_MAX_THREADS];
    for (int k = 0; k < T; k++) {
        job[k].window = window; job[k].v = v; job[k].use_v = v != IGD_HIP_NO_VALUE_FILTER && db->gType == 1;
        job[k].res = res;
    }
    if (rc == 0 && nq > 0 && nF > 0) rc = stripe_drive(job, sizeof job[0], T, nF, db, m, ichr, qs, qe, nq, pl, 0, R, pnear_row);
    if (rc == 0) {
        int64_t *const out[3] = {n_within, n_overlap, sum_dist};
        for (int s = 0; s < 3; s++) if (out[s]) memcpy(out[s], res + (size_t)s * (size_t)(R * nC), sizeof(int64_t) * (size_t)(R * nC));
    }
    free(res);
    return rc;
}

int igdc_permute_nearest_host_ws(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                 const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t window, int32_t v,
                                 int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist, const igd_hip_workspace *ws)
{
    const perm_place pl = {ctg_len, mode, seed, ws, NULL, NULL};
    return permute_nearest_host_run(db, m, ichr, qs, qe, nq, &pl, nperm, window, v, n_within, n_overlap, sum_dist);
}

int igdc_permute_nearest_host_rs(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                 const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                                 int64_t nperm, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist)
{
    const perm_pool pool = {pool_ichr, pool_qs, pool_qe, npool};
    const perm_place pl = {NULL, IGD_HIP_PERM_RESAMPLE, seed, NULL, NULL, &pool};
    return permute_nearest_host_run(db, m, ichr, qs, qe, nq, &pl, nperm, window, v, n_within, n_overlap, sum_dist);
}

/* the summary of a null distribution of distance statistics; igd_core.h has the formulas */
int igdc_perm_nearest_summary(const int64_t *n_within, const int64_t *sum_dist, int64_t nperm, int64_t ncols, double *within_mean,
                              double *within_sd, double *within_z, int64_t *within_n_ge, double *nlog10_p_within_upper, double *mean_dist,
                              double *dist_mean, double *dist_sd, double *dist_z, int64_t *n_def, int64_t *dist_n_le,
                              double *nlog10_p_dist_lower)
{
    const double P = (double)nperm, nan = __builtin_nan("");
    if (!sqrt || !log10 || nperm < 1 || ncols < 0 || (ncols > 0 && (!n_within || !sum_dist))) return -1;
    for (int64_t f = 0; f < ncols; f++) {
        const int64_t nw0 = n_within[f], sd0 = sum_dist[f];
        /* counts: igdc_perm_summary's formulas */
        __int128 sum = 0, sumsq = 0;
        int64_t nge = 0, ndef = 0, nle = 0;
        for (int64_t p = 1; p <= nperm; p++) {
            const int64_t x = n_within[p * ncols + f];
            sum += x;
            sumsq += (__int128)x * (__int128)x;
            nge += x >= nw0;
        }
        const double mu = (double)sum / P;
        double s = nan;
        if (nperm > 1) s = sqrt((double)((__int128)nperm * sumsq - sum * sum) / (P * (P - 1.0)));
        if (within_mean) within_mean[f] = mu;
        if (within_sd) within_sd[f] = s;
        if (within_z) within_z[f] = (s != s || s == 0.0) ? nan : ((double)nw0 - mu) / s;
        if (within_n_ge) within_n_ge[f] = nge;
        if (nlog10_p_within_upper) nlog10_p_within_upper[f] = 0.0 - log10((double)(nge + 1) / (P + 1.0));
        /* distances: m_p = sd_p / nw_p over the permutations with nw_p > 0, two passes in permutation order */
        const double md = nw0 > 0 ? (double)sd0 / (double)nw0 : nan;
        double acc = 0.0;
        for (int64_t p = 1; p <= nperm; p++) {
            const int64_t nwp = n_within[p * ncols + f], sdp = sum_dist[p * ncols + f];
            if (nwp <= 0) continue;
            ndef++;
            acc += (double)sdp / (double)nwp;
            if (nw0 > 0 && (__int128)sdp * (__int128)nw0 <= (__int128)sd0 * (__int128)nwp) nle++;
        }
        const double dmu = ndef > 0 ? acc / (double)ndef : nan;
        double ds = nan;
        if (ndef > 1) {
            double ss = 0.0;
            for (int64_t p = 1; p <= nperm; p++) {
                const int64_t nwp = n_within[p * ncols + f];
                if (nwp <= 0) continue;
                const double t = (double)sum_dist[p * ncols + f] / (double)nwp - dmu;
                ss += t * t;
            }
            ds = sqrt(ss / (double)(ndef - 1));
        }
        if (mean_dist) mean_dist[f] = md;
        if (dist_mean) dist_mean[f] = dmu;
        if (dist_sd) dist_sd[f] = ds;
        if (dist_z) dist_z[f] = (nw0 <= 0 || ds != ds || ds == 0.0) ? nan : (md - dmu) / ds;
        if (n_def) n_def[f] = ndef;
        if (dist_n_le) dist_n_le[f] = nle;
        if (nlog10_p_dist_lower) nlog10_p_dist_lower[f] = 0.0 - log10((double)(nle + 1) / (P + 1.0));
    }
    return 0;
}

/* ---- permutation null of the overlapping records' values (what igd_hip_permute_map computes) ------------------------------
 * Row 0 is the set as given, row p + 1 permutation p of the generator or draw p of the pool (stripe_run); a row is
 * igdc_map_sets_host's row computer over its regions (one_region_map) summed into the three statistics as map_sets_fold sums a
 * region.  Each thread has its own permuted arrays, count and agg row and tile buffer; the rows are disjoint.  Everything is
 * computed into a buffer and copied out at the end: -1 (a refused argument, a tile that could not be read) writes nothing. */
typedef struct {
    perm_stripe s;
    int op; int32_t v; int use_v;
    int64_t *res;           /* three matrices of nrows x nFiles */
    int64_t *agg;           /* one agg row (under COUNT it receives the counts: agg_sum IS pairs) */
} pmap_job;

static int pmap_row(void *job, int64_t r, const int32_t *s, const int32_t *e)
{
    pmap_job *P = (pmap_job *)job;
    const int64_t nF = P->s.db->nFiles;
    int32_t *count = P->s.extra;                                           /* one count row */
    map_sets_ctx c = {P->s.db, P->s.m, NULL, NULL, NULL, P->op, P->v, count, P->agg, P->res, P->res + P->s.nrows * nF,
                      P->res + 2 * P->s.nrows * nF};
    for (int64_t i = 0; i < P->s.nq && !P->s.tb.failed; i++) {
        one_region_map(P->s.db, P->s.m, &P->s.tb, P->s.rowc[i], s[i], e[i], P->op, P->v, P->use_v, count, P->agg);
        if (!P->s.tb.failed) map_sets_fold(&c, (int32_t)r, 0);
    }
    return P->s.tb.failed;
}

/* the body of the igdc_permute_map_host entries: per thread a count row of nFiles words and an agg row of nFiles 64-bit words */
static int permute_map_host_run(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                const perm_place *pl, int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    if (!db || !map_op_ok(db, op) || perm_args_bad(db, m, ichr, qs, qe, nq, nperm, pl)) return -1;
    const int64_t nF = db->nFiles, R = nperm + 1;
    const int T = stripe_threads(nq, R);
    int64_t *res = (int64_t *)calloc((size_t)(3 * R * nF) + 1, sizeof(int64_t));
    int64_t *a = (int64_t *)malloc(sizeof(int64_t) * ((size_t)T * (size_t)nF + 1));
    int rc = res && a ? 0 : -1;
    pmap_job job[HOST_MAX_THREADS];
    for (int k = 0; k < T && rc == 0; k++) {
        job[k].op = op; job[k].v = v; job[k].use_v = v != IGD_HIP_NO_VALUE_FILTER && db->gType == 1;
        job[k].res = res; job[k].agg = a + (size_t)k * (size_t)nF;
    }
    if (rc == 0 && nq > 0 && nF > 0) rc = stripe_drive(job, sizeof job[0], T, nF, db, m, ichr, qs, qe, nq, pl, 0, R, pmap_row);
    if (rc == 0) {
        int64_t *const out[3] = {n_hit, pairs, agg_sum};
        for (int s = 0; s < 3; s++) if (out[s]) memcpy(out[s], res + (size_t)s * (size_t)(R * nF), sizeof(int64_t) * (size_t)(R * nF));
    }
    free(res); free(a);
    return rc;
}

int igdc_permute_map_host_ws(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                             const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int op, int32_t v, int64_t *n_hit,
                             int64_t *pairs, int64_t *agg_sum, const igd_hip_workspace *ws)
{
    const perm_place pl = {ctg_len, mode, seed, ws, NULL, NULL};
    return permute_map_host_run(db, m, ichr, qs, qe, nq, &pl, nperm, op, v, n_hit, pairs, agg_sum);
}

int igdc_permute_map_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                          const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs,
                          int64_t *agg_sum)
{
    return igdc_permute_map_host_ws(db, m, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, op, v, n_hit, pairs, agg_sum, NULL);
}

int igdc_permute_map_host_rs(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                             const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                             int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    const perm_pool pool = {pool_ichr, pool_qs, pool_qe, npool};
    const perm_place pl = {NULL, IGD_HIP_PERM_RESAMPLE, seed, NULL, NULL, &pool};
    return permute_map_host_run(db, m, ichr, qs, qe, nq, &pl, nperm, op, v, n_hit, pairs, agg_sum);
}

/* the summary of a null distribution of value statistics; igd_core.h has the formulas */
int igdc_perm_map_summary(const int64_t *n_hit, const int64_t *pairs, const int64_t *agg_sum, int64_t nperm, int64_t ncols, int over_pairs,
                          double *observed, int64_t *n_def, double *mean, double *sd, double *z, int64_t *n_ge, int64_t *n_le,
                          double *nlog10_p_upper, double *nlog10_p_lower, double *nhit_mean, double *nhit_sd, double *nhit_z)
{
    const double P = (double)nperm, nan = __builtin_nan("");
    const int64_t *den = over_pairs ? pairs : n_hit;
    if (!sqrt || !log10 || nperm < 1 || ncols < 0 || (ncols > 0 && (!n_hit || !agg_sum || !den))) return -1;
    for (int64_t f = 0; f < ncols; f++) {
        /* the counts: igdc_perm_summary's formulas over the permuted n_hit */
        __int128 sum = 0, sumsq = 0;
        for (int64_t p = 1; p <= nperm; p++) {
            const int64_t x = n_hit[p * ncols + f];
            sum += x;
            sumsq += (__int128)x * (__int128)x;
        }
        const double mu = (double)sum / P;
        double s = nan;
        if (nperm > 1) s = sqrt((double)((__int128)nperm * sumsq - sum * sum) / (P * (P - 1.0)));
        if (nhit_mean) nhit_mean[f] = mu;
        if (nhit_sd) nhit_sd[f] = s;
        if (nhit_z) nhit_z[f] = (s != s || s == 0.0) ? nan : ((double)n_hit[f] - mu) / s;
        /* the statistic: m_p = a_p / d_p over the permutations with d_p > 0, two passes in permutation order; m_p against m_0 is
         * a_p d_0 against a_0 d_p, exact in 128 bits (both denominators are positive) */
        const int64_t a0 = agg_sum[f], d0 = den[f];
        const double m0 = d0 > 0 ? (double)a0 / (double)d0 : nan;
        int64_t ndef = 0, nge = 0, nle = 0;
        double acc = 0.0;
        for (int64_t p = 1; p <= nperm; p++) {
            const int64_t ap = agg_sum[p * ncols + f], dp = den[p * ncols + f];
            if (dp <= 0) continue;
            ndef++;
            acc += (double)ap / (double)dp;
            if (d0 > 0) {
                const __int128 l = (__int128)ap * (__int128)d0, r = (__int128)a0 * (__int128)dp;
                nge += l >= r;
                nle += l <= r;
            }
        }
        const double dmu = ndef > 0 ? acc / (double)ndef : nan;
        double ds = nan;
        if (ndef > 1) {
            double ss = 0.0;
            for (int64_t p = 1; p <= nperm; p++) {
                const int64_t dp = den[p * ncols + f];
                if (dp <= 0) continue;
                const double t = (double)agg_sum[p * ncols + f] / (double)dp - dmu;
                ss += t * t;
            }
            ds = sqrt(ss / (double)(ndef - 1));
        }
        if (observed) observed[f] = m0;
        if (n_def) n_def[f] = ndef;
        if (mean) mean[f] = dmu;
        if (sd) sd[f] = ds;
        if (z) z[f] = (d0 <= 0 || ds != ds || ds == 0.0) ? nan : (m0 - dmu) / ds;
        if (n_ge) n_ge[f] = nge;
        if (n_le) n_le[f] = nle;
        if (nlog10_p_upper) nlog10_p_upper[f] = d0 > 0 ? 0.0 - log10((double)(nge + 1) / (double)(ndef + 1)) : nan;
        if (nlog10_p_lower) nlog10_p_lower[f] = d0 > 0 ? 0.0 - log10((double)(nle + 1) / (double)(ndef + 1)) : nan;
    }
    return 0;
}

/* The handle flavours' batches (Python search_n / search_1, R search_nr / getOverlaps): on the host while the batch is
 * small and no engine is resident, otherwise on the engine, which is attached at the first batch that needs it -- the
 * moment the reference would do its first fseek/fread (src/igd_search.c:469-476); open_iGD reads the header only, like
 * the reference's (src_py/igd_base.c, IGDr/src/igd_base.c open_iGD). */
int igdc_search_auto(igdc_db *db, const char *path, int device, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                     int64_t nq, int32_t v, int rule, int flags, int64_t *hits, int64_t *total)
{
    if (total) *total = 0;
    if (!db || !hits || nq < 0) return IGD_HIP_ERR_ARG;
    if (nq == 0) return IGD_HIP_OK;
    if (!db->dev && nq <= igdc_host_limit() && path) {
        const int fd = open(path, O_RDONLY);
        igdc_map *m = fd >= 0 ? igdc_map_open(db, fd) : NULL;
        if (fd >= 0) close(fd);
        if (m) {
            const int rc = igdc_search_host(db, m, ichr, qs, qe, nq, v, rule, hits, total);
            igdc_map_close(m);
            if (rc == 0) return IGD_HIP_OK;
        }
    }
    if (!db->dev) {
        const int rc = path ? igdc_attach_path(db, path, device) : IGD_HIP_ERR_ARG;
        if (rc != IGD_HIP_OK) return rc;
    }
    return igd_hip_search_ex(db->dev, ichr, qs, qe, nq, v, rule, flags, hits, total);
}

/* ---- merged region sets and the base-pair Jaccard (include/igd_hip.h has the definitions) -------------------------------
 * Per set: the regions that take part, sorted by (ichr, qs, qe), one sweep with the running maximum of the ends.  The runs of
 * set k are built at its own place [set_off[k], ..) of scratch arrays, threads over the sets; one serial pass packs them. */
typedef struct { int32_t c, s, e; } merge_reg;
static int merge_reg_cmp(const void *a, const void *b)
{
    const merge_reg *x = (const merge_reg *)a, *y = (const merge_reg *)b;
    if (x->c != y->c) return x->c < y->c ? -1 : 1;
    if (x->s != y->s) return x->s < y->s ? -1 : 1;
    return x->e < y->e ? -1 : x->e > y->e;
}

typedef struct {
    const igdc_db *db;
    const int32_t *ichr, *qs, *qe;
    const int64_t *set_off;
    int32_t k0, k1;
    int64_t gap;
    merge_reg *regs;            /* [n] scratch: set k sorts at set_off[k] */
    int32_t *rc, *rs, *re, *rn; /* [n] the runs of set k from set_off[k] on */
    int64_t *nrun, *n_dropped;  /* [nsets] */
} merge_job;

static void *merge_run(void *arg)
{
    merge_job *J = (merge_job *)arg;
    for (int32_t k = J->k0; k < J->k1; k++) {
        const int64_t a = J->set_off[k], b = J->set_off[k + 1];
        merge_reg *g = J->regs + a;
        int64_t m = 0, r = -1;
        for (int64_t i = a; i < b; i++)
            if (igd_hip_merge_takes_part(J->db->nCtg, J->ichr[i], J->qs[i], J->qe[i])) {
                g[m].c = J->ichr[i]; g[m].s = J->qs[i]; g[m].e = J->qe[i];
                m++;
            }
        qsort(g, (size_t)m, sizeof *g, merge_reg_cmp);
        for (int64_t i = 0; i < m; i++) {
            if (r < 0 || g[i].c != J->rc[a + r] || igd_hip_merge_opens(g[i].s, J->re[a + r], J->gap)) {
                r++;
                J->rc[a + r] = g[i].c; J->rs[a + r] = g[i].s; J->re[a + r] = g[i].e; J->rn[a + r] = 1;
            } else {
                if (g[i].e > J->re[a + r]) J->re[a + r] = g[i].e;
                J->rn[a + r]++;
            }
        }
        J->nrun[k] = r + 1;
        J->n_dropped[k] = (b - a) - m;
    }
    return NULL;
}

int igdc_merge_host(const igdc_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                    int64_t gap, int32_t *m_ichr, int32_t *m_qs, int32_t *m_qe, int64_t *m_off, int32_t *m_count, int64_t *n_dropped)
{
    if (!db || !igd_hip_merge_gap_valid(gap) || (nsets > 0 && (!m_off || !n_dropped)) || set_off_bad(set_off, nsets, ichr, qs, qe)) return -1;
    const int64_t n = nsets > 0 ? set_off[nsets] : 0;
    if (n > 0 && (!m_ichr || !m_qs || !m_qe)) return -1;
    if (nsets == 0) return 0;
    merge_reg *regs = (merge_reg *)malloc((size_t)(n > 0 ? n : 1) * sizeof *regs);
    int32_t *runs = (int32_t *)malloc((size_t)(n > 0 ? n : 1) * 4 * sizeof *runs);
    int64_t *nrun = (int64_t *)calloc((size_t)nsets, sizeof *nrun);
    if (!regs || !runs || !nrun) { free(regs); free(runs); free(nrun); return -1; }
    int T = host_threads(n);
    if (T > nsets) T = nsets;
    merge_job job[HOST_MAX_THREADS];
    for (int t = 0; t < T; t++) {
        merge_job *J = &job[t];
        J->db = db; J->ichr = ichr; J->qs = qs; J->qe = qe; J->set_off = set_off; J->gap = gap;
        J->k0 = (int32_t)((int64_t)nsets * t / T); J->k1 = (int32_t)((int64_t)nsets * (t + 1) / T);
        J->regs = regs; J->rc = runs; J->rs = runs + n; J->re = runs + 2 * n; J->rn = runs + 3 * n;
        J->nrun = nrun; J->n_dropped = n_dropped;
    }
    run_threads(merge_run, job, sizeof job[0], T);
    int64_t at = 0;
    for (int32_t k = 0; k < nsets; k++) {
        const int64_t a = set_off[k];
        m_off[k] = at;
        for (int64_t r = 0; r < nrun[k]; r++, at++) {
            m_ichr[at] = runs[a + r]; m_qs[at] = runs[n + a + r]; m_qe[at] = runs[2 * n + a + r];
            if (m_count) m_count[at] = runs[3 * n + a + r];
        }
    }
    m_off[nsets] = at;
    for (; at < n; at++) {                                /* the rest of the capacity is defined too */
        m_ichr[at] = 0; m_qs[at] = 0; m_qe[at] = 0;
        if (m_count) m_count[at] = 0;
    }
    free(regs); free(runs); free(nrun);
    return 0;
}

/* file_bp[f], f <= nFiles: igdc_coverage_host over every tile of every contig as one query (igd_hip_tile_query); nothing is
 * kept between calls -- the host route has no handle of its own to keep it in */
int igdc_dataset_bp_host(const igdc_db *db, const igdc_map *m, int32_t v, int rule, int64_t *file_bp)
{
    if (!db || !m || !file_bp || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) return -1;
    int64_t nq = 0;
    for (int32_t c = 0; c < db->nCtg; c++) nq += db->nTile[c];
    int32_t *q = (int32_t *)malloc((size_t)(nq > 0 ? nq : 1) * 3 * sizeof *q);
    if (!q) return -1;
    int64_t k = 0;
    for (int32_t c = 0; c < db->nCtg; c++)
        for (int64_t t = 0; t < db->nTile[c]; t++) {
            int32_t ws, we;
            if (!igd_hip_tile_query(db->nbp, t, &ws, &we)) break;
            q[k] = c; q[nq + k] = ws; q[2 * nq + k] = we;
            k++;
        }
    for (int32_t f = 0; f <= db->nFiles; f++) file_bp[f] = 0;
    const int rc = igdc_coverage_host(db, m, q, q + nq, q + 2 * nq, k, v, rule, file_bp, file_bp + db->nFiles);
    free(q);
    return rc;
}

int igdc_jaccard_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                      const int64_t *set_off, int32_t nsets, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *file_bp,
                      int64_t *n_merged, int64_t *n_dropped)
{
    if (!db || !m || !file_bp || (nsets > 0 && (!inter || !set_bp || !n_merged || !n_dropped)) ||
        (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT) || set_off_bad(set_off, nsets, ichr, qs, qe)) return -1;
    const int64_t n = nsets > 0 ? set_off[nsets] : 0, nF = db->nFiles;
    int rc = igdc_dataset_bp_host(db, m, v, rule, file_bp);
    if (rc != 0 || nsets == 0) return rc;
    int32_t *mr = (int32_t *)malloc((size_t)(n > 0 ? n : 1) * 3 * sizeof *mr);
    int64_t *moff = (int64_t *)malloc(((size_t)nsets + 1) * sizeof *moff);
    if (!mr || !moff) { free(mr); free(moff); return -1; }
    rc = igdc_merge_host(db, ichr, qs, qe, set_off, nsets, 0, mr, mr + n, mr + 2 * n, moff, NULL, n_dropped);
    for (int32_t k = 0; rc == 0 && k < nsets; k++) {
        const int64_t a = moff[k], b = moff[k + 1];
        int64_t *row = inter + (int64_t)k * (nF + 1), bp = 0;
        for (int64_t f = 0; f <= nF; f++) row[f] = 0;
        for (int64_t r = a; r < b; r++) bp += (int64_t)mr[2 * n + r] - (int64_t)mr[n + r];
        set_bp[k] = bp;
        n_merged[k] = b - a;
        rc = igdc_coverage_host(db, m, mr + a, mr + n + a, mr + 2 * n + a, b - a, v, rule, row, row + nF);
    }
    free(mr); free(moff);
    return rc;
}

/* jaccard[i] = inter / (set_bp + file_bp - inter), set_fraction[i] = inter / set_bp, file_fraction[i] = inter / file_bp, doubles, NaN
 * where the divisor is 0; i = k * ncols + f over inter[nsets][ncols], set_bp[nsets], file_bp[ncols] */
double igdc_jaccard_value(int64_t inter, int64_t set_bp, int64_t file_bp)
{
    const int64_t u = set_bp + file_bp - inter;
    return u != 0 ? (double)inter / (double)u : NAN;
}
int igdc_jaccard_summary(const int64_t *inter, const int64_t *set_bp, const int64_t *file_bp, int64_t nsets, int64_t ncols, double *jaccard,
                         double *set_fraction, double *file_fraction)
{
    if (nsets < 0 || ncols < 0 || (nsets > 0 && ncols > 0 && (!inter || !set_bp || !file_bp))) return -1;
    for (int64_t k = 0; k < nsets; k++)
        for (int64_t f = 0; f < ncols; f++) {
            const int64_t i = k * ncols + f;
            if (jaccard) jaccard[i] = igdc_jaccard_value(inter[i], set_bp[k], file_bp[f]);
            if (set_fraction) set_fraction[i] = set_bp[k] != 0 ? (double)inter[i] / (double)set_bp[k] : NAN;
            if (file_fraction) file_fraction[i] = file_bp[f] != 0 ? (double)inter[i] / (double)file_bp[f] : NAN;
        }
    return 0;
}

/* ---- permutation null of the base-pair overlap (what igd_hip_permute_bp computes; include/igd_hip.h has the definitions) --
 * Row 0 is the set as given, row p + 1 permutation p of igdc_permute_regions_host's generator (stripe_run); a row is
 * igdc_jaccard_host's treatment of one set: igdc_merge_host at gap 0, then igdc_coverage_host over the runs.  Each thread has
 * its own permuted arrays and run arrays; the rows are disjoint.  Everything is computed into a buffer and copied out at the
 * end: -1 (a refused argument, a tile that could not be read) writes nothing. */
typedef struct {
    perm_stripe s;
    int32_t v; int rule;
    int64_t *inter, *set_bp, *n_merged, *dropped;   /* nrows x (nFiles + 1), nrows, nrows, nrows */
} pbp_job;

static int pbp_row(void *job, int64_t r, const int32_t *s, const int32_t *e)
{
    pbp_job *P = (pbp_job *)job;
    const igdc_db *db = P->s.db;
    const int64_t nF = db->nFiles, nq = P->s.nq, off[2] = {0, nq};
    int32_t *mr = P->s.extra;                                              /* the runs (3 x nq) */
    int64_t moff[2], bp = 0;
    if (igdc_merge_host(db, P->s.rowc, s, e, off, 1, 0, mr, mr + nq, mr + 2 * nq, moff, NULL, &P->dropped[r]) != 0) return 1;
    for (int64_t i = 0; i < moff[1]; i++) bp += (int64_t)mr[2 * nq + i] - (int64_t)mr[nq + i];
    P->set_bp[r] = bp;
    P->n_merged[r] = moff[1];
    int64_t *row = P->inter + r * (nF + 1);
    return igdc_coverage_host(db, P->s.m, mr, mr + nq, mr + 2 * nq, moff[1], P->v, P->rule, row, row + nF) != 0;
}

int igdc_permute_bp_host(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                         const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter,
                         int64_t *set_bp, int64_t *n_merged, int64_t *n_dropped)
{
    return igdc_permute_bp_host_ws(db, m, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, inter, set_bp, n_merged, n_dropped, NULL);
}

/* the body of the igdc_permute_bp_host entries: per thread the runs of a row, 3 nq words */
static int permute_bp_host_run(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const perm_place *pl, int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged,
                               int64_t *n_dropped)
{
    if ((rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT) || perm_args_bad(db, m, ichr, qs, qe, nq, nperm, pl)) return -1;
    const int64_t nF = db->nFiles, nC = nF + 1, R = nperm + 1;
    const int T = stripe_threads(nq, R);
    int64_t *res = (int64_t *)calloc((size_t)(R * nC + 3 * R), sizeof(int64_t));
    int rc = res ? 0 : -1;
    pbp_job job[HOST_MAX_THREADS];
    for (int k = 0; k < T && rc == 0; k++) {
        job[k].v = v; job[k].rule = rule;
        job[k].inter = res; job[k].set_bp = res + R * nC; job[k].n_merged = job[k].set_bp + R; job[k].dropped = job[k].n_merged + R;
    }
    if (rc == 0 && nq > 0) rc = stripe_drive(job, sizeof job[0], T, 3 * nq, db, m, ichr, qs, qe, nq, pl, 0, R, pbp_row);
    if (rc == 0) {
        if (inter) memcpy(inter, res, sizeof(int64_t) * (size_t)(R * nC));
        if (set_bp) memcpy(set_bp, res + R * nC, sizeof(int64_t) * (size_t)R);
        if (n_merged) memcpy(n_merged, res + R * nC + R, sizeof(int64_t) * (size_t)R);
        if (n_dropped) *n_dropped = res[R * nC + 2 * R];
    }
    free(res);
    return rc;
}

int igdc_permute_bp_host_ws(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                            const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter,
                            int64_t *set_bp, int64_t *n_merged, int64_t *n_dropped, const igd_hip_workspace *ws)
{
    const perm_place pl = {ctg_len, mode, seed, ws, NULL, NULL};
    return permute_bp_host_run(db, m, ichr, qs, qe, nq, &pl, nperm, v, rule, inter, set_bp, n_merged, n_dropped);
}

int igdc_permute_bp_host_rs(const igdc_db *db, const igdc_map *m, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                            const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                            int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged, int64_t *n_dropped)
{
    const perm_pool pool = {pool_ichr, pool_qs, pool_qe, npool};
    const perm_place pl = {NULL, IGD_HIP_PERM_RESAMPLE, seed, NULL, NULL, &pool};
    return permute_bp_host_run(db, m, ichr, qs, qe, nq, &pl, nperm, v, rule, inter, set_bp, n_merged, n_dropped);
}

/* the summary of a null distribution of base-pair overlaps; igd_core.h has the formulas */
int igdc_perm_bp_summary(const int64_t *inter, const int64_t *set_bp, const int64_t *file_bp, int64_t nperm, int64_t ncols,
                         int64_t *observed, double *mean, double *sd, double *z, double *fold, int64_t *n_ge, int64_t *n_le,
                         double *nlog10_p_upper, double *nlog10_p_lower, double *jaccard, double *jaccard_mean, double *jaccard_sd,
                         int64_t *jaccard_n_def, int64_t *jaccard_n_ge)
{
    const double P = (double)nperm, nan = __builtin_nan("");
    if (!sqrt || !log10 || nperm < 1 || ncols < 0 || (ncols > 0 && (!inter || !set_bp || !file_bp))) return -1;
    for (int64_t f = 0; f < ncols; f++) {
        const int64_t x0 = inter[f], u0 = set_bp[0] + file_bp[f] - x0;
        /* base pairs: igdc_perm_summary's formulas, the sums exact in 128 bits */
        __int128 sum = 0, sumsq = 0;
        int64_t nge = 0, nle = 0;
        for (int64_t p = 1; p <= nperm; p++) {
            const int64_t x = inter[p * ncols + f];
            sum += x;
            sumsq += (__int128)x * (__int128)x;
            nge += x >= x0;
            nle += x <= x0;
        }
        const double mu = (double)sum / P;
        double s = nan;
        if (nperm > 1) s = sqrt((double)((__int128)nperm * sumsq - sum * sum) / (P * (P - 1.0)));
        if (observed) observed[f] = x0;
        if (mean) mean[f] = mu;
        if (sd) sd[f] = s;
        if (z) z[f] = (s != s || s == 0.0) ? nan : ((double)x0 - mu) / s;
        if (fold) fold[f] = mu != 0.0 ? (double)x0 / mu : nan;
        if (n_ge) n_ge[f] = nge;
        if (n_le) n_le[f] = nle;
        if (nlog10_p_upper) nlog10_p_upper[f] = 0.0 - log10((double)(nge + 1) / (P + 1.0));
        if (nlog10_p_lower) nlog10_p_lower[f] = 0.0 - log10((double)(nle + 1) / (P + 1.0));
        /* Jaccards: j_p = x_p / u_p over the permutations with u_p != 0, two passes in permutation order */
        int64_t ndef = 0, jge = 0;
        double acc = 0.0;
        for (int64_t p = 1; p <= nperm; p++) {
            const int64_t xp = inter[p * ncols + f], up = set_bp[p] + file_bp[f] - xp;
            if (up == 0) continue;
            ndef++;
            acc += (double)xp / (double)up;
            if (u0 != 0 && (__int128)xp * (__int128)u0 >= (__int128)x0 * (__int128)up) jge++;
        }
        const double jmu = ndef > 0 ? acc / (double)ndef : nan;
        double js = nan;
        if (ndef > 1) {
            double ss = 0.0;
            for (int64_t p = 1; p <= nperm; p++) {
                const int64_t xp = inter[p * ncols + f], up = set_bp[p] + file_bp[f] - xp;
                if (up == 0) continue;
                const double t = (double)xp / (double)up - jmu;
                ss += t * t;
            }
            js = sqrt(ss / (double)(ndef - 1));
        }
        if (jaccard) jaccard[f] = igdc_jaccard_value(x0, set_bp[0], file_bp[f]);
        if (jaccard_mean) jaccard_mean[f] = jmu;
        if (jaccard_sd) jaccard_sd[f] = js;
        if (jaccard_n_def) jaccard_n_def[f] = ndef;
        if (jaccard_n_ge) jaccard_n_ge[f] = jge;
    }
    return 0;
}
