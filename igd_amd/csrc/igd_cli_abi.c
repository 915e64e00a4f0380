/* igd_cli_abi.c -- the CLI/libigd flavour of the reference ABI (include/igd_search.h,
 * include/igd_base.h) on top of the host core (igd_core.c) and the HIP engine (igd_hip.h).
 *
 * Every function keeps the name, prototype, return value and silent-failure behaviour of
 * its counterpart in /root/reference/src/igd_search.c / igd_base.c (lines cited at each
 * definition).  What differs is how the answer is computed: the whole tile region is put on
 * the GPU once and every call -- single query or query file -- is one batch for the engine.
 * There is no CPU search here.  A library must not end its host process (it may be a Python or R
 * interpreter): if no HIP device is usable, the call prints why on stderr, returns the way the
 * reference's silent failures return (src/igd_search.c:457,462,701-702: 0 / hits untouched) and
 * igd_engine_status() is non-zero from then on; only `igd_search` -- the body of the command line
 * tool -- turns that into a non-zero return value instead of printing a table of zeros.
 */
#define _GNU_SOURCE
#include <fcntl.h>
#include <pthread.h>
#include <stdlib.h>
#include <unistd.h>
#include <string.h>
#include <sysexits.h>

#include <time.h>

#include "igd_search.h"
#include "igd_core.h"
#include "igd_create_host.h"
#include "../../include/igd_create.h"

/* IGD_TIMING=1: wall-clock phases of `igd search` on stderr (stdout stays the reference's) */
static double now_s(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}
static int timing_on(void) { const char *e = getenv("IGD_TIMING"); return e && *e && *e != '0'; }
static void phase(const char *name, double *t0)
{
    if (!timing_on()) return;
    double t = now_s();
    fprintf(stderr, "[igd timing] %-28s %8.1f ms\n", name, 1e3 * (t - *t0));
    *t0 = t;
}

/* process-wide state of this flavour (reference: src/igd.c:14-19) */
void     *hc = NULL;
iGD_t    *IGD = NULL;
gdata_t  *gData = NULL;
gdata0_t *gData0 = NULL;
int32_t   preIdx = 0, preChr = 0, tile_size = 16384;
FILE     *fP = NULL;

/* our side of an iGD_t handed out by get_igdinfo */
static igdc_db *g_core = NULL;       /* header tables + dictionary + device handle        */
static iGD_t   *g_core_of = NULL;    /* the iGD_t that g_core mirrors                      */
static char    *g_core_path = NULL;

/* The database the search functions work on.  In the reference everything is one program and
 * `IGD` is THE global (src/igd.c:15).  When this library is a shared object and the calling
 * program defines its own `IGD` (as src/igd.c does) without exporting it, the program's variable
 * and ours are different objects and ours stays NULL: then the handle last returned by
 * get_igdinfo() is the database -- which is what the program stored in its `IGD` anyway. */
static iGD_t *cur_igd(void)
{
    return (IGD && IGD == g_core_of) ? IGD : g_core_of;
}

static int device_from_env(void)
{
    const char *e = getenv("IGD_DEVICE");
    return e && *e ? atoi(e) : 0;
}

static int g_fail_rc = 0;            /* code of the first engine failure of this process (0: none) */
static int g_usage_rc = 0;           /* a refusal found in the input files of `-P .. -W` (exit code EX_USAGE; 0: none) */

int igd_engine_status(void) { return g_fail_rc; }

static void engine_failed(const char *where, int rc)
{
    if (rc == IGD_HIP_ERR_ARG || rc == IGD_HIP_ERR_NOMEM)
        fprintf(stderr, "igd: %s: the GPU engine refused the request (code %d): %s\n", where, rc, igd_hip_last_error());
    else
        fprintf(stderr, "igd: %s: GPU engine unavailable (code %d): %s\n"
                        "igd: this build has no CPU search path.\n", where, rc, igd_hip_last_error());
    if (!g_fail_rc) g_fail_rc = rc ? rc : IGD_HIP_ERR_DEVICE;
}

/* The engine for the current IGD, created at the first search call: this is the moment the
 * reference would do its first fseek/fread on fP (src/igd_search.c:469-476). */
static igd_hip_db *engine(void)
{
    iGD_t *G = cur_igd();
    if (!G || !g_core) {
        fprintf(stderr, "igd: search called before get_igdinfo()\n");
        if (!g_fail_rc) g_fail_rc = IGD_HIP_ERR_ARG;
        return NULL;
    }
    if (g_core->dev && igd_hip_nfiles(g_core->dev) == G->nFiles) return g_core->dev;
    g_core->nFiles = G->nFiles;          /* hits[] is sized from the TSV (:923-925) */
    double t0 = now_s();
    /* the path is preferred when known (pipelined pread + upload); fP serves callers that only
     * opened the stream themselves.  IGD_DEVICES=0,1,..: the database goes to every listed GPU and
     * query files are searched in contiguous slabs, one per device (igdc_search_multi) */
    int devs[IGDC_MAX_DEVICES];
    const int nd = g_core_path ? igdc_devices_from_env(devs, IGDC_MAX_DEVICES) : 0;
    /* (IGD_MULTI_REDUCE=rccl with ONE listed device still goes through the group: a one-rank communicator and all-reduce --
     * how the RCCL call-site is exercised on a one-GPU box, tests/test_gpu_multidev.py) */
    const char *mr = getenv("IGD_MULTI_REDUCE");
    const int group = nd > 1 || (nd == 1 && mr && !strcmp(mr, "rccl"));
    int rc = group ? igdc_attach_path_multi(g_core, g_core_path, devs, nd)
           : g_core_path ? igdc_attach_path(g_core, g_core_path, nd == 1 ? devs[0] : device_from_env())
                         : igdc_attach_fp(g_core, fP, device_from_env());
    if (rc != IGD_HIP_OK) { engine_failed("open", rc); return NULL; }
    phase("database -> GPU", &t0);
    return g_core->dev;
}

/* ------------------------------- base ------------------------------------------------- */
char *parse_bed(char *s, int32_t *st_, int32_t *en_)                /* src/igd_base.c:53-72 */
{
    return igdc_parse_bed(s, st_, en_, 1);
}

int32_t bSearch(gdata_t *g, int32_t t0, int32_t tc, int32_t qe)    /* src/igd_base.c:74-94 */
{
    /* last index in [t0,tc] whose start < qe; -1 when there is none */
    if (tc < t0 || g[t0].start >= qe) return -1;
    int32_t lo = t0, hi = tc;            /* invariant: g[lo].start < qe */
    while (lo < hi) {
        int32_t mid = lo + (hi - lo + 1) / 2;
        if (g[mid].start < qe) lo = mid; else hi = mid - 1;
    }
    return lo;
}

int32_t get_id(const char *chrm)                                   /* src/igd_base.c:325-331 */
{
    return igdc_get_id(hc ? (const igdc_db *)hc : g_core, chrm);
}

info_t *get_fileinfo(char *ifName, int32_t *nFiles)                /* src/igd_base.c:235-267 */
{
    igdc_db tmp;
    memset(&tmp, 0, sizeof tmp);
    if (igdc_load_index(&tmp, ifName) != 0) {
        printf("file not found:%s\n", ifName);
        return NULL;
    }
    info_t *fi = (info_t *)malloc(sizeof(info_t) * (size_t)(tmp.nFiles + 1));
    for (int32_t i = 0; i < tmp.nFiles; i++) {
        fi[i].fileName = tmp.fileName[i];      /* ownership moves to the caller, as strdup'd */
        fi[i].nr = tmp.fileNr[i];
        fi[i].md = tmp.fileMd[i];
    }
    *nFiles = tmp.nFiles;
    free(tmp.fileName); free(tmp.fileNr); free(tmp.fileMd);
    return fi;
}

iGD_t *get_igdinfo(char *igdFile)                                  /* src/igd_base.c:269-323 */
{
    igdc_db *core = igdc_open(igdFile);
    if (!core) {
        printf("Can't open file %s", igdFile);
        return NULL;
    }
    /* hand out the tables in the allocation shape the reference's callers free
     * (src/igd_search.c:1067-1076: nTile, each nCnt[i]/tIdx[i], the arrays, then IGD) */
    iGD_t *g = (iGD_t *)calloc(1, sizeof *g);
    const int32_t m = core->nCtg;
    g->nbp = core->nbp; g->gType = core->gType; g->nCtg = m;
    g->nTile = (int32_t *)malloc(sizeof(int32_t) * (size_t)(m + 1));
    g->nCnt = (int32_t **)malloc(sizeof(int32_t *) * (size_t)(m + 1));
    g->tIdx = (int64_t **)malloc(sizeof(int64_t *) * (size_t)(m + 1));
    g->cName = (char **)malloc(sizeof(char *) * (size_t)(m + 1));
    const int64_t recBytes = core->gType == 0 ? 12 : 16;
    int64_t loc = core->dataOff;                               /* tile offsets: the running sum of src/igd_base.c:288-303 */
    for (int32_t c = 0; c < m; c++) {
        const int32_t k = core->nTile[c];
        g->nTile[c] = k;
        g->nCnt[c] = (int32_t *)malloc(((size_t)k + 1) * sizeof(int32_t));
        g->tIdx[c] = (int64_t *)malloc(((size_t)k + 1) * sizeof(int64_t));
        memcpy(g->nCnt[c], core->nCnt[c], sizeof(int32_t) * (size_t)k);
        g->nCnt[c][k] = 0; g->tIdx[c][k] = 0;
        for (int32_t j = 0; j < k; j++) { g->tIdx[c][j] = loc; loc += recBytes * (int64_t)core->nCnt[c][j]; }
        g->cName[c] = (char *)malloc(40);
        memcpy(g->cName[c], core->cName[c], 40);
    }
    if (g_core) igdc_close(g_core);
    free(g_core_path);
    g_core = core;
    g_core_of = g;
    g_core_path = strdup(igdFile);
    hc = core;                         /* the dictionary lives in the core */
    tile_size = core->nbp;
    return g;
}

/* ------------------------------- one query -------------------------------------------- */
/* Single intervals (`-r`, get_overlaps*): while no engine is resident the host reads the interval's own tiles, like the
 * reference does (:469-476), instead of uploading the whole database for one wave of work (igdc_walk_one, igd_core.h) */
static int one_query_fd(void)
{
    if (g_core && g_core->dev) return -1;                     /* the database is on the GPU already: ask it */
    if (g_core_path) return open(g_core_path, O_RDONLY);
    return fP ? dup(fileno(fP)) : -1;
}

static int32_t one_query(const char *chrm, int32_t qs, int32_t qe, int32_t v, int rule, int64_t *hits)
{
    int32_t ichr = get_id(chrm);
    if (ichr < 0) return 0;                                   /* :456-457 */
    if (g_core && cur_igd()) {
        const int fd = one_query_fd();
        if (fd >= 0) {
            g_core->nFiles = cur_igd()->nFiles;
            const int64_t n = igdc_walk_one(g_core, fd, ichr, qs, qe, v, v != IGD_HIP_NO_VALUE_FILTER, rule, hits, NULL, NULL);
            close(fd);
            if (n >= 0) return (int32_t)n;
        }
    }
    igd_hip_db *dev = engine();
    if (!dev) return 0;
    int64_t total = 0;
    int rc = igd_hip_search(dev, &ichr, &qs, &qe, 1, v, rule, hits, &total);
    if (rc != IGD_HIP_OK) { engine_failed("search", rc); return 0; }
    return (int32_t)total;
}

int32_t get_overlaps(char *chrm, int32_t qs, int32_t qe, int64_t *hits)      /* :454-534 */
{
    one_query(chrm, qs, qe, IGD_HIP_NO_VALUE_FILTER, IGD_HIP_RULE_NEST, hits);
    return 0;                           /* the reference's nols is never incremented (:533) */
}

int32_t get_overlaps0(char *chrm, int32_t qs, int32_t qe, int64_t *hits)     /* :30-112 */
{
    one_query(chrm, qs, qe, IGD_HIP_NO_VALUE_FILTER, IGD_HIP_RULE_NEST, hits);
    return 0;
}

int32_t get_overlaps_v(char *chrm, int32_t qs, int32_t qe, int32_t v, int64_t *hits) /* :623-694 */
{
    /* the driver calls this only for v>0 (:1027); any v keeps the predicate value>=v */
    return one_query(chrm, qs, qe, v, IGD_HIP_RULE_FLAT, hits);
}

/* ------------------------------- query files ------------------------------------------ */
/* the query file is parsed (host threads) while the database goes to the GPU (first search only) */
typedef struct { const char *qFile; igdc_queries q; int rc; } parse_job;
static void *parse_run(void *arg)
{
    parse_job *J = (parse_job *)arg;
    J->rc = igdc_read_queries(g_core, J->qFile, 1, &J->q);
    return NULL;
}

/* `-O N -A F -B F`: a minimum overlap per (query region, record) pair (include/igd_hip.h: igd_hip_min_overlap), for the plain
 * `-q` / `-Q` counts, `-u`, `-U` [-R] and `-P`.  g_mo is NULL without them; the routines below hand it to the `_ov` entry points,
 * which take NULL as "no threshold". */
static igd_hip_min_overlap g_mo_val = {0, 0, 0};
static const igd_hip_min_overlap *g_mo = NULL;

/* a decimal fraction in [0, 1] with at most six places -> parts per million, exactly (digits only: no strtod); -1: refused */
static int32_t parse_ppm(const char *a)
{
    int32_t whole = 0, frac = 0;
    int nw = 0, nf = 0;
    for (; *a >= '0' && *a <= '9'; a++, nw++) {
        if (nw >= 1) return -1;                       /* one digit before the point: 0 or 1 */
        whole = *a - '0';
    }
    if (*a == '.') {
        for (a++; *a >= '0' && *a <= '9'; a++, nf++) {
            if (nf >= 6) return -1;
            frac = frac * 10 + (*a - '0');
        }
        if (nf == 0 && nw == 0) return -1;
    } else if (nw == 0) return -1;
    if (*a) return -1;
    for (; nf < 6; nf++) frac *= 10;
    if (whole > 1 || (whole == 1 && frac != 0)) return -1;
    return whole * IGD_HIP_PPM + frac;
}

/* a file of at most igdc_host_limit() queries, while no engine is resident: counted on the host (igd_hostpath.c) */
static igdc_map *host_map_lim(int64_t nq, int64_t lim)
{
    if (!g_core || g_core->dev || nq > lim) return NULL;
    const int fd = g_core_path ? open(g_core_path, O_RDONLY) : (fP ? dup(fileno(fP)) : -1);
    if (fd < 0) return NULL;
    g_core->nFiles = cur_igd()->nFiles;          /* hits[] is sized from the TSV (:923-925) */
    igdc_map *m = igdc_map_open(g_core, fd);
    close(fd);
    return m;
}

/* ------------------------------- shared by the table commands of `igd search` ---------- */
/* the dispatch of `-q` on gType and -v (:1023-1030): returns the value filter and stores the tile rule (NULL: the command has none) */
static int32_t q_dispatch(int32_t v, int *rule)
{
    const int byValue = IGD->gType != 0 && v > 0;
    if (rule) *rule = byValue ? IGD_HIP_RULE_FLAT : IGD_HIP_RULE_NEST;
    return byValue ? v : IGD_HIP_NO_VALUE_FILTER;
}

/* The route of a table command.  While no engine is resident and at most igdc_host_limit() regions are asked about, the host
 * answers from the mapped database (igd_hostpath.c); otherwise, and after a read error there, the engine does (IGD_DEVICES with
 * several devices: the first one, as -Q).  The two calls are the command's own:
 *     cli_route R;
 *     if (route_host(&R, regions)) route_host_end(&R, igdc_x_host(g_core, R.hm, ..) == 0, "<host label>");
 *     if (route_engine(&R, gate)) route_engine_end(&R, "x", igd_hip_x(R.dev, ..), "<engine label>");
 * `gate` is the command's reason to ask the engine at all (for most: regions > 0).  An engine failure is reported here and leaves
 * g_fail_rc set: the command prints no table then, as `-q`. */
typedef struct { igdc_map *hm; igd_hip_db *dev; int onHost; double t0; } cli_route;

static int route_host(cli_route *R, int64_t regions)
{
    R->dev = NULL; R->onHost = 0;
    R->hm = host_map_lim(regions, igdc_host_limit());
    R->t0 = now_s();
    return R->hm != NULL;
}

static int route_host_end(cli_route *R, int ok, const char *label)
{
    igdc_map_close(R->hm);
    R->hm = NULL;
    if ((R->onHost = ok)) phase(label, &R->t0);
    return ok;
}

static int route_engine(cli_route *R, int gate)
{
    if (R->onHost || !gate) return 0;
    R->dev = engine();
    R->t0 = now_s();
    return R->dev != NULL;
}

static void route_engine_end(cli_route *R, const char *name, int rc, const char *label)
{
    if (rc != IGD_HIP_OK) engine_failed(name, rc);
    phase(label, &R->t0);
}

/* The query files of a command: the one of `-q` (no "Query set" lines), else those of the `-Q` list -- one per line, blank lines
 * skipped, a trailing CR stripped. */
typedef struct { char **paths; int32_t n; int setLines; char *one; } cli_paths;

static char **read_list(const char *listName, int32_t *n_out)
{
    char **paths = NULL;
    int32_t n = 0, cap = 0;
    *n_out = -1;
    igdc_lines *r = igdc_lines_open(listName);
    if (!r) { printf("Cannot open query list %s\n", listName); return NULL; }
    char *line;
    int64_t len;
    while ((line = igdc_lines_next(r, &len)) != NULL) {
        size_t L = strlen(line);
        while (L > 0 && (line[L - 1] == '\r' || line[L - 1] == '\n')) line[--L] = '\0';
        if (L == 0) continue;
        if (n == cap) { cap = cap ? 2 * cap : 64; paths = (char **)realloc(paths, sizeof(char *) * (size_t)cap); }
        paths[n++] = strdup(line);
    }
    igdc_lines_close(r);
    *n_out = n;
    return paths;
}

static int paths_open(cli_paths *P, char *qfName, const char *listName)      /* 0: the list cannot be opened (said on stdout) */
{
    memset(P, 0, sizeof *P);
    if (qfName) { P->one = qfName; P->paths = &P->one; P->n = 1; return 1; }
    P->setLines = 1;
    P->paths = read_list(listName, &P->n);
    return P->n >= 0;
}

static void paths_close(cli_paths *P)
{
    if (!P->setLines) return;
    for (int32_t k = 0; k < P->n; k++) free(P->paths[k]);
    free(P->paths);
}

/* The query sets of a command: every file read by igdc_read_queries (an unreadable one is an empty set) and, once sets_cat() is
 * asked for them, the sets' accepted lines concatenated with their offsets -- what the `_sets` entry points take. */
typedef struct {
    char **paths; int32_t n; int setLines;
    igdc_queries *q; int64_t nq;                 /* per set, and the regions of all sets */
    int32_t *ichr, *qs, *qe; int64_t *off;       /* sets_cat() */
} cli_sets;

static void sets_load(cli_sets *S, const cli_paths *P)
{
    char **paths = P->paths;
    const int32_t n = P->n;
    memset(S, 0, sizeof *S);
    S->paths = paths; S->n = n; S->setLines = P->setLines;
    igdc_queries *q = S->q = (igdc_queries *)calloc((size_t)n + 1, sizeof(igdc_queries));
    for (int32_t k = 0; k < n; k++) {
        if (igdc_read_queries(g_core, paths[k], 1, &q[k]) != 0) memset(&q[k], 0, sizeof q[k]);   /* unreadable: an empty set */
        S->nq += q[k].n;
    }
}

static void sets_cat(cli_sets *S)
{
    if (S->off) return;
    const igdc_queries *q = S->q;
    const int32_t n = S->n;
    int32_t *ichr = (int32_t *)malloc(sizeof(int32_t) * (size_t)(S->nq + 1)), *qs = (int32_t *)malloc(sizeof(int32_t) * (size_t)(S->nq + 1));
    int32_t *qe = (int32_t *)malloc(sizeof(int32_t) * (size_t)(S->nq + 1));
    int64_t *off = (int64_t *)malloc(sizeof(int64_t) * ((size_t)n + 1));
    off[0] = 0;
    for (int32_t k = 0; k < n; k++) {
        if (q[k].n) {
            memcpy(ichr + off[k], q[k].ichr, sizeof(int32_t) * (size_t)q[k].n);
            memcpy(qs + off[k], q[k].qs, sizeof(int32_t) * (size_t)q[k].n);
            memcpy(qe + off[k], q[k].qe, sizeof(int32_t) * (size_t)q[k].n);
        }
        off[k + 1] = off[k] + q[k].n;
    }
    S->ichr = ichr; S->qs = qs; S->qe = qe; S->off = off;
}

static void sets_free(cli_sets *S)
{
    for (int32_t k = 0; k < S->n; k++) igdc_queries_free(&S->q[k]);
    free(S->q); free(S->ichr); free(S->qs); free(S->qe); free(S->off);
}

static void sets_title(const cli_sets *S, int32_t k)                         /* the line that opens the block of set k under -Q */
{
    if (S->setLines) printf("Query set %d: %s\n", (int)k, S->paths[k]);
}

static int64_t file_query(const char *qFile, int32_t v, int rule, int64_t *hits)
{
    if (!g_core || !cur_igd()) { engine(); return 0; }
    parse_job J;
    J.qFile = qFile; J.rc = -1;
    double t0 = now_s();
    pthread_t th;
    /* a file that is probably small is parsed first and the engine is only started if it turns out not to be */
    const int threaded = !(g_core->dev) && !igdc_host_probably_small(qFile) && pthread_create(&th, NULL, parse_run, &J) == 0;
    if (threaded) { engine(); pthread_join(th, NULL); }
    else parse_run(&J);
    if (J.rc != 0) return 0;                                         /* :701-702 */
    igdc_queries q = J.q;
    phase(threaded ? "database -> GPU  ||  read + parse queries" : "read + parse queries", &t0);
    int64_t total = 0;
    if (q.unsorted && igdc_queries_group_contigs(&q, g_core->nCtg))       /* a sorted BED, chromosomes in another order */
        phase("contig runs put into the database's order", &t0);
    else if (q.unsorted && timing_on())                                   /* one out-of-place line is enough */
        fprintf(stderr, "[igd timing] the query file is not position-sorted: the engine groups it (bucket path)\n");
    igdc_map *hm = q.n > 0 ? host_map_lim(q.n, igdc_host_limit()) : NULL;
    int onHost = 0;
    if (hm) {
        onHost = igdc_search_host_ov(g_core, hm, q.ichr, q.qs, q.qe, q.n, v, rule, hits, &total, g_mo) == 0;   // (fails only on a read error: hits[] untouched)
        igdc_map_close(hm);
        if (onHost) phase("search on the host (small file)", &t0);
        else total = 0;
    }
    if (!onHost && q.n > 0) {
        igd_hip_db *dev = engine();
        t0 = now_s();
        /* position-sorted BED (the common case): tell the engine, it verifies on the device */
        /* under a minimum overlap the file is ONE set of the sets route (the batch pipeline takes no threshold; first device) */
        const int64_t one[2] = {0, q.n};
        int rc = !dev ? IGD_HIP_OK
               : g_mo ? igd_hip_search_sets_ov(dev, q.ichr, q.qs, q.qe, one, 1, v, rule, 0, hits, &total, g_mo)
               : g_core->grp ? igdc_search_multi(g_core, q.ichr, q.qs, q.qe, q.n, v, rule, igdc_queries_flags(&q, g_core->nbp), hits, &total)
               : igd_hip_search_ex(dev, q.ichr, q.qs, q.qe, q.n, v, rule, igdc_queries_flags(&q, g_core->nbp), hits, &total);
        if (rc != IGD_HIP_OK) { engine_failed("search", rc); total = 0; }
        phase("search (H2D + kernels + D2H)", &t0);
    }
    igdc_queries_free(&q);
    return total;
}

int64_t getOverlaps(char *qFile, int64_t *hits)                              /* :696-719 */
{
    file_query(qFile, IGD_HIP_NO_VALUE_FILTER, IGD_HIP_RULE_NEST, hits);
    return 0;                           /* sum of get_overlaps returns = 0 */
}

int64_t getOverlaps0(char *qFile, int64_t *hits)                             /* :202-225 */
{
    file_query(qFile, IGD_HIP_NO_VALUE_FILTER, IGD_HIP_RULE_NEST, hits);
    return 0;
}

int64_t getOverlaps_v(char *qFile, int64_t *hits, int32_t v)                 /* :746-769 */
{
    return file_query(qFile, v, IGD_HIP_RULE_FLAT, hits);
}

/* ------------------------------- Seqpare (-s) ------------------------------------------ */
/* seqOverlaps, src/igd_search.c:354-451.  The query file is read like readBED reads it
 * (src/igd_base.c:628-649: parse_bed's accept rule, ailist_add drops uint32 start > end), contigs in
 * first-seen order, each contig's queries ordered by start with ties in file order (the reference's
 * qsort(compare_qstart) is glibc's stable merge sort).  Enumeration, grouping, the greedy matching
 * and the ordered double sums run on the GPU (igd_hip_seqpare); here only sm/(Nq + nr - sm). */
typedef struct { char *name; int32_t id; int32_t *qs, *qe; int64_t n, cap; } sq_ctg;

static void sq_sort(int32_t *qs, int32_t *qe, int64_t n)
{
    if (n < 2) return;
    int32_t *ts = (int32_t *)malloc(sizeof(int32_t) * (size_t)n), *te = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
    int32_t *as = qs, *ae = qe, *bs = ts, *be = te;
    for (int64_t w = 1; w < n; w <<= 1) {
        for (int64_t lo = 0; lo < n; lo += 2 * w) {
            const int64_t mid = lo + w < n ? lo + w : n, hi = lo + 2 * w < n ? lo + 2 * w : n;
            int64_t i = lo, j = mid, k = lo;
            while (i < mid && j < hi) {
                if (as[j] < as[i]) { bs[k] = as[j]; be[k++] = ae[j++]; }
                else { bs[k] = as[i]; be[k++] = ae[i++]; }
            }
            while (i < mid) { bs[k] = as[i]; be[k++] = ae[i++]; }
            while (j < hi) { bs[k] = as[j]; be[k++] = ae[j++]; }
        }
        int32_t *x = as; as = bs; bs = x;
        x = ae; ae = be; be = x;
    }
    if (as != qs) { memcpy(qs, as, sizeof(int32_t) * (size_t)n); memcpy(qe, ae, sizeof(int32_t) * (size_t)n); }
    free(ts); free(te);
}

void seqOverlaps(char *qFile, double *sm)
{
    iGD_t *G = cur_igd();
    if (!G) return;
    const int32_t nfiles = G->nFiles;
    for (int32_t m = 0; m < nfiles; m++) sm[m] = 0.0;
    igdc_lines *r = igdc_lines_open(qFile);
    if (!r) return;                                           /* the reference dereferences NULL here */
    sq_ctg *ctg = NULL;
    int32_t nctg = 0, mctg = 0;
    int64_t Nq = 0;
    char *line;
    while ((line = igdc_lines_next(r, NULL)) != NULL) {
        int32_t st, en;
        char *name = igdc_parse_bed(line, &st, &en, 1);
        if (!name || (uint32_t)st > (uint32_t)en) continue;
        int32_t k = nctg - 1;                                  /* BED files are grouped by contig */
        while (k >= 0 && strcmp(ctg[k].name, name) != 0) k--;
        if (k < 0) {
            if (nctg == mctg) { mctg = mctg ? 2 * mctg : 32; ctg = (sq_ctg *)realloc(ctg, sizeof(sq_ctg) * (size_t)mctg); }
            k = nctg++;
            ctg[k].name = strdup(name); ctg[k].id = get_id(name);
            ctg[k].qs = ctg[k].qe = NULL; ctg[k].n = ctg[k].cap = 0;
        }
        sq_ctg *c = &ctg[k];
        if (c->n == c->cap) {
            c->cap = c->cap ? 2 * c->cap : 64;
            c->qs = (int32_t *)realloc(c->qs, sizeof(int32_t) * (size_t)c->cap);
            c->qe = (int32_t *)realloc(c->qe, sizeof(int32_t) * (size_t)c->cap);
        }
        c->qs[c->n] = st; c->qe[c->n] = en; c->n++;
        Nq++;
    }
    igdc_lines_close(r);
    int64_t n = 0;
    for (int32_t k = 0; k < nctg; k++) if (ctg[k].id >= 0) n += ctg[k].n;
    int32_t *ichr = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n ? n : 1)), *qs = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n ? n : 1));
    int32_t *qe = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n ? n : 1)), *grp = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n ? n : 1));
    int64_t at = 0;
    int32_t ng = 0;
    for (int32_t k = 0; k < nctg; k++) {
        if (ctg[k].id < 0) continue;                          /* unknown contig: counts in Nq, overlaps nothing */
        sq_sort(ctg[k].qs, ctg[k].qe, ctg[k].n);
        for (int64_t i = 0; i < ctg[k].n; i++, at++) { ichr[at] = ctg[k].id; qs[at] = ctg[k].qs[i]; qe[at] = ctg[k].qe[i]; grp[at] = ng; }
        ng++;
    }
    double *sums = (double *)calloc((size_t)nfiles + 1, sizeof(double));
    /* The (query contig, dataset) groups are independent, so a query file beyond one engine batch (2^24
     * queries, 2^32 overlaps; the reference has no limit) goes contig range by contig range; the engine
     * continues the running double sums (igd_hip_seqpare_add), so the order of additions stays the reference's. */
    igd_hip_db *dev = n > 0 ? engine() : NULL;
    int failed = n > 0 && !dev;
    for (int32_t g0 = 0; g0 < ng && !failed;) {
        int64_t a0 = 0, a1;
        while (a0 < n && grp[a0] < g0) a0++;
        int32_t g1 = g0;
        a1 = a0;
        while (g1 < ng) {                                      /* as many whole contigs as fit one batch */
            int64_t e = a1;
            while (e < n && grp[e] == g1) e++;
            if (g1 > g0 && e - a0 > igd_hip_max_batch()) break;
            a1 = e; g1++;
        }
        for (;;) {
            for (int64_t i = a0; i < a1; i++) grp[i] -= g0;    /* group numbers of the call start at 0 */
            const int rc = igd_hip_seqpare_add(dev, ichr + a0, qs + a0, qe + a0, a1 - a0, grp + a0, g1 - g0, sums);
            for (int64_t i = a0; i < a1; i++) grp[i] += g0;
            if (rc == IGD_HIP_OK) break;
            if (rc == IGD_HIP_ERR_ARG && g1 - g0 > 1) {          /* too many overlaps for one call: fewer contigs */
                g1 = g0 + (g1 - g0) / 2;
                a1 = a0;
                while (a1 < n && grp[a1] < g1) a1++;
                continue;
            }
            engine_failed("seqpare", rc);
            failed = 1;
            break;
        }
        g0 = g1;
    }
    for (int32_t m = 0; m < nfiles; m++) sm[m] = sums[m] / ((double)Nq + G->finfo[m].nr - sums[m]);   /* :446-449 */
    free(sums); free(ichr); free(qs); free(qe); free(grp);
    for (int32_t k = 0; k < nctg; k++) { free(ctg[k].name); free(ctg[k].qs); free(ctg[k].qe); }
    free(ctg);
}

/* ------------------------------- full enumeration (-f) -------------------------------- */
typedef struct { char *buf; size_t n, cap; } obuf;
static void ob_str(obuf *o, const char *s, size_t L) { memcpy(o->buf + o->n, s, L); o->n += L; }

/* Prints what get_overlaps_f1/_f0 print for each query of the batch, in order
 * ("Query %s, %i, %i: \n" at :548, one "%i\t %i\t %i\t %s\n" per overlap at :577,:610).  The engine
 * streams the overlaps in chunks of contiguous query ranges (igd_hip_enumerate_stream); the text of a
 * chunk (35 bytes per overlap: > 1 GB for 10^6 queries) is formatted by several threads, each into its
 * own buffer for a contiguous range of queries, and written out in order -- while the next chunk is
 * being filled on the GPU and copied over PCIe. */
typedef struct {
    const igdc_queries *q; char **names; const iGD_t *G; const size_t *flen;
    int64_t q0;                       /* first query of the engine call this block belongs to   */
    const int64_t *qoff; const igd_hip_hit *hit;   /* hit[h - hbase] = overlap h of the call    */
    const igd_hip_hit8 *hit8; int bits;            /* ... or the packed stream (8 bytes per overlap; bits = those of idx) */
    int64_t hbase;
    int64_t i0, i1;                   /* queries [i0, i1) of that call                           */
    obuf o;
} fmt_job;

static const char DIGIT2[201] =
    "00010203040506070809101112131415161718192021222324252627282930313233343536373839"
    "40414243444546474849505152535455565758596061626364656667686970717273747576777879"
    "8081828384858687888990919293949596979899";
static inline void ob_uint(obuf *o, uint32_t u)
{
    char t[12];
    int k = 12;
    while (u >= 100) { const uint32_t r = u % 100; u /= 100; k -= 2; memcpy(t + k, DIGIT2 + 2 * r, 2); }
    if (u >= 10) { k -= 2; memcpy(t + k, DIGIT2 + 2 * u, 2); }
    else t[--k] = (char)('0' + u);
    memcpy(o->buf + o->n, t + k, (size_t)(12 - k));
    o->n += (size_t)(12 - k);
}
static inline void ob_int(obuf *o, int32_t x)
{
    if (x < 0) { o->buf[o->n++] = '-'; ob_uint(o, 0u - (uint32_t)x); }
    else ob_uint(o, (uint32_t)x);
}

static void *fmt_run(void *arg)
{
    fmt_job *J = (fmt_job *)arg;
    obuf *o = &J->o;
    const iGD_t *G = J->G;
    for (int64_t i = J->i0; i < J->i1; i++) {
        const int32_t c = J->q->ichr[J->q0 + i], qs = J->q->qs[J->q0 + i], qe = J->q->qe[J->q0 + i];
        const int32_t n1 = qs / G->nbp;
        if (n1 > G->nTile[c] - 1 || n1 < 0) continue;           /* :544-545 */
        const char *nm = J->names[J->q0 + i];
        ob_str(o, "Query ", 6);
        ob_str(o, nm, strlen(nm));
        ob_str(o, ", ", 2); ob_int(o, qs); ob_str(o, ", ", 2); ob_int(o, qe);
        ob_str(o, ": \n", 3);
        uint32_t k = 0;
        if (J->hit8) {                                            /* start | (end - start) << bits | idx: expanded while it is printed */
            const igd_hip_hit8 *h = J->hit8 + (J->qoff[i] - J->hbase), *he = J->hit8 + (J->qoff[i + 1] - J->hbase);
            const int bits = J->bits;
            const uint32_t fmask = bits ? (1u << bits) - 1u : 0u;
            for (; h < he; h++, k++) {
                const uint32_t f = h->lenidx & fmask;
                const int32_t st = (int32_t)h->start, en = (int32_t)(h->start + (h->lenidx >> bits));
                ob_uint(o, k); ob_str(o, "\t ", 2); ob_int(o, st); ob_str(o, "\t ", 2);
                ob_int(o, en); ob_str(o, "\t ", 2); ob_str(o, G->finfo[f].fileName, J->flen[f]); o->buf[o->n++] = '\n';
            }
            continue;
        }
        const igd_hip_hit *h = J->hit + (J->qoff[i] - J->hbase), *he = J->hit + (J->qoff[i + 1] - J->hbase);
        for (; h < he; h++, k++) {
            const int32_t f = h->idx;
            ob_uint(o, k); ob_str(o, "\t ", 2); ob_int(o, h->start); ob_str(o, "\t ", 2);
            ob_int(o, h->end); ob_str(o, "\t ", 2); ob_str(o, G->finfo[f].fileName, J->flen[f]); o->buf[o->n++] = '\n';
        }
    }
    return NULL;
}

typedef struct {
    const igdc_queries *q; char **names; const iGD_t *G; const size_t *flen; size_t maxL;
    int64_t q0; int nt;
    obuf keep[64];                    /* the formatting threads' text buffers, kept from chunk to chunk: fresh 100 MB
                                         allocations per chunk would spend the time in page faults, not in formatting */
} print_ctx;

/* igd_hip_enum_sink / igd_hip_enum_sink8: one chunk = queries [b0,b1) of the call, its overlaps in pinned memory */
static int print_chunk_any(void *ctx, int64_t b0, int64_t b1, const int64_t *qoff, const igd_hip_hit *hit, const igd_hip_hit8 *hit8, int bits);
static int print_chunk(void *ctx, int64_t b0, int64_t b1, const int64_t *qoff, const igd_hip_hit *hit)
{
    return print_chunk_any(ctx, b0, b1, qoff, hit, NULL, 0);
}
static int print_chunk8(void *ctx, int64_t b0, int64_t b1, const int64_t *qoff, const igd_hip_hit8 *hit8, int bits)
{
    return print_chunk_any(ctx, b0, b1, qoff, NULL, hit8, bits);
}
static int print_chunk_any(void *ctx, int64_t b0, int64_t b1, const int64_t *qoff, const igd_hip_hit *hit, const igd_hip_hit8 *hit8, int bits)
{
    print_ctx *P = (print_ctx *)ctx;
    const int nt = P->nt;
    fmt_job job[64];
    pthread_t th[64];
    int started[64];
    int used = 0;
    int64_t i0 = b0;
    for (int t = 0; t < nt && i0 < b1; t++) {                    /* equal shares of the chunk's overlaps (+queries) */
        int64_t i1 = b1;
        if (t + 1 < nt) {
            const int64_t want = qoff[b0] + b0 + (qoff[b1] - qoff[b0] + (b1 - b0)) * (t + 1) / nt;
            int64_t lo = i0, hi = b1;                            /* largest i1 with qoff[i1] + i1 <= want */
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo + 1) / 2;
                if (qoff[mid] + mid <= want) lo = mid; else hi = mid - 1;
            }
            i1 = lo > i0 ? lo : i0 + 1;
        }
        fmt_job *J = &job[used];
        J->q = P->q; J->names = P->names; J->G = P->G; J->flen = P->flen; J->q0 = P->q0; J->qoff = qoff; J->hit = hit; J->hit8 = hit8; J->bits = bits;
        J->hbase = qoff[b0];
        J->i0 = i0; J->i1 = i1;
        const size_t need = (size_t)(i1 - i0) * 96 + (size_t)(qoff[i1] - qoff[i0]) * (40 + P->maxL) + 64;
        if (need > P->keep[used].cap) {
            free(P->keep[used].buf);
            P->keep[used].cap = need + need / 4;
            P->keep[used].buf = (char *)malloc(P->keep[used].cap);
        }
        J->o = P->keep[used];
        J->o.n = 0;
        if (!J->o.buf) { P->keep[used].cap = 0; for (int k = 0; k < used; k++) if (started[k]) pthread_join(th[k], NULL); return 1; }
        /* a thread that cannot be started is simply run here */
        started[used] = used > 0 && pthread_create(&th[used], NULL, fmt_run, J) == 0;
        if (used > 0 && !started[used]) fmt_run(J);
        used++;
        i0 = i1;
    }
    if (used > 0) fmt_run(&job[0]);
    for (int t = 0; t < used; t++) {
        if (started[t]) pthread_join(th[t], NULL);
        if (job[t].o.n) fwrite(job[t].o.buf, 1, job[t].o.n, stdout);
    }
    return 0;
}

static int64_t enumerate_and_print(const igdc_queries *q, char **names)
{
    if (q->n == 0) return 0;
    igdc_map *hm = host_map_lim(q->n, igdc_host_limit_enum());
    igd_hip_db *dev = hm ? NULL : engine();
    if (!hm && !dev) return 0;
    iGD_t *G = cur_igd();
    int64_t *qoff = (int64_t *)malloc(sizeof(int64_t) * (size_t)(q->n + 1));
    int64_t total = 0, grand = 0;
    size_t *flen = (size_t *)malloc(sizeof(size_t) * (size_t)(G->nFiles + 1));
    size_t maxL = 0;
    for (int32_t f = 0; f < G->nFiles; f++) { flen[f] = strlen(G->finfo[f].fileName); if (flen[f] > maxL) maxL = flen[f]; }
    long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
    const char *ev = getenv("IGD_PRINT_THREADS");
    int nt = ev && atoi(ev) > 0 ? atoi(ev) : (ncpu > 32 ? 32 : (ncpu < 1 ? 1 : (int)ncpu));
    if (nt > 64) nt = 64;
    const int64_t step = igd_hip_max_batch();
    fflush(stdout);
    print_ctx P;
    P.q = q; P.names = names; P.G = G; P.flen = flen; P.maxL = maxL; P.nt = nt;
    memset(P.keep, 0, sizeof P.keep);
    int onHost = 0;
    if (hm) {                                                    /* small file: the overlaps come from the host, the text as always */
        igd_hip_hit *hit = NULL;
        P.q0 = 0;
        if (igdc_enumerate_host(g_core, hm, q->ichr, q->qs, q->qe, q->n, qoff, &hit, &total) == 0) {
            print_chunk(&P, 0, q->n, qoff, hit);
            grand = total;
            onHost = 1;
        }
        free(hit);
        igdc_map_close(hm);
        if (!onHost) dev = engine();                             /* (a read error on the host path: the engine reads the file its own way) */
    }
    if (!onHost && dev)
    for (int64_t q0 = 0; q0 < q->n; q0 += step) {
        int64_t m = q->n - q0 < step ? q->n - q0 : step;
        P.q0 = q0;
        /* 8 bytes per overlap over PCIe when the database's records fit them (igd_hip_hit8), else 16 */
        int rc = (!getenv("IGD_ENUM_HIT16") && igd_hip_hit8_idx_bits(dev) >= 0)
                     ? igd_hip_enumerate_stream8(dev, q->ichr + q0, q->qs + q0, q->qe + q0, m, qoff, print_chunk8, &P, &total)
                     : igd_hip_enumerate_stream(dev, q->ichr + q0, q->qs + q0, q->qe + q0, m, qoff, print_chunk, &P, &total);
        if (rc != IGD_HIP_OK) { engine_failed("enumerate", rc); break; }
        grand += total;
    }
    for (int t = 0; t < 64; t++) free(P.keep[t].buf);
    free(flen);
    free(qoff);
    return grand;
}

static int64_t file_enumerate(const char *qFile)
{
    if (!g_core || !cur_igd()) { engine(); return 0; }
    igdc_lines *r = igdc_lines_open(qFile);
    if (!r) return 0;
    igdc_queries q;
    memset(&q, 0, sizeof q);
    char **names = NULL;
    int64_t ncap = 0;
    char *line;
    while ((line = igdc_lines_next(r, NULL)) != NULL) {
        int32_t st, en;
        char *chrm = igdc_parse_bed(line, &st, &en, 1);
        if (!chrm) continue;
        int32_t id = igdc_get_id(g_core, chrm);
        if (id < 0) continue;
        if (q.n == ncap) {
            ncap = ncap ? ncap * 2 : 4096;
            names = (char **)realloc(names, sizeof(char *) * (size_t)ncap);
        }
        names[q.n] = g_core->cName[id];    /* the accepted name equals the stored one */
        igdc_queries_push(&q, id, st, en);
    }
    igdc_lines_close(r);
    int64_t total = enumerate_and_print(&q, names);
    igdc_queries_free(&q);
    free(names);
    return total;
}

int64_t getOverlaps_f1(char *qFile) { return file_enumerate(qFile); }        /* :721-744 */
int64_t getOverlaps_f0(char *qFile) { return file_enumerate(qFile); }        /* :227-250 */

typedef struct { int32_t k; const iGD_t *G; } emit_ctx;
static void emit_line(void *ctx, int32_t idx, int32_t start, int32_t end, int32_t in_tile, int32_t tile)
{
    (void)in_tile; (void)tile;
    emit_ctx *E = (emit_ctx *)ctx;
    printf("%i\t %i\t %i\t %s\n", E->k++, start, end, E->G->finfo[idx].fileName);          /* :577,:610 */
}

static int32_t one_enumerate(char *chrm, int32_t qs, int32_t qe)
{
    int32_t ichr = get_id(chrm);
    if (ichr < 0) return 0;
    if (g_core && cur_igd()) {                                /* `-r ... -f`: the interval's own tiles, on the host */
        const iGD_t *G = cur_igd();
        const int32_t n1 = qs / G->nbp;
        const int fd = one_query_fd();
        if (fd >= 0) {
            if (n1 > G->nTile[ichr] - 1 || n1 < 0) { close(fd); return 0; }              /* :544-545 */
            g_core->nFiles = G->nFiles;
            printf("Query %s, %i, %i: \n", chrm, qs, qe);                                 /* :548 */
            emit_ctx E;
            E.k = 0; E.G = G;
            const int64_t n = igdc_walk_one(g_core, fd, ichr, qs, qe, 0, 0, IGD_HIP_RULE_NEST, NULL, emit_line, &E);
            close(fd);
            if (n >= 0) return (int32_t)n;
        }
    }
    igdc_queries q;
    memset(&q, 0, sizeof q);
    igdc_queries_push(&q, ichr, qs, qe);
    char *name = chrm;
    int64_t total = enumerate_and_print(&q, &name);
    igdc_queries_free(&q);
    return (int32_t)total;
}

/* seq_overlaps, src/igd_search.c:253-352: Seqpare's per-query helper -- every overlap of ONE interval appended to the
 * caller's list with its similarity st / (qlen + rlen - st) in single precision (the reference's order of operations) and
 * the reference's identity of a record: (index inside its tile, FIRST tile of the query) -- idx_t = n1 also for records
 * met in later tiles (:291,:337).  One interval: answered on the host from the interval's own tiles, like get_overlaps;
 * rule NEST (everything is nested in `if(tmpi>0)`, :266), 16-byte records (the reference reads gdata_t unconditionally).
 * The list grows by the reference's EXPAND rule (src/igd_base.h:262-265), so `mm` matches as well. */
typedef struct { overlaps_t *olp; float qlen; int32_t qs, qe, n1; int failed; } seq_ctx;
static void emit_seq(void *ctx, int32_t idx, int32_t start, int32_t end, int32_t in_tile, int32_t tile)
{
    seq_ctx *S = (seq_ctx *)ctx;
    overlaps_t *o = S->olp;
    (void)tile;
    if (S->failed) return;
    if (o->nn == o->mm) {
        const int32_t m = o->mm ? o->mm + (2 + o->mm / 8) : 16;
        overlap_t *p = (overlap_t *)realloc(o->olist, sizeof(overlap_t) * (size_t)m);
        if (!p) { S->failed = 1; return; }
        o->olist = p; o->mm = m;
    }
    const float st = (float)((S->qe < end ? S->qe : end) - (S->qs > start ? S->qs : start));
    const float rlen = (float)(end - start);
    overlap_t *p = &o->olist[o->nn++];
    p->idx_g = in_tile; p->idx_f = idx; p->idx_t = S->n1;
    p->sm = st / (S->qlen + rlen - st);
}

void seq_overlaps(char *chrm, int32_t qs, int32_t qe, overlaps_t *olp)
{
    const int32_t ichr = get_id(chrm);
    if (ichr < 0 || !olp || !g_core || !cur_igd()) return;                  /* :257-258 */
    const iGD_t *G = cur_igd();
    if (G->gType == 0) return;                                              /* 12-byte records: the reference would misread them */
    int fd = g_core_path ? open(g_core_path, O_RDONLY) : (fP ? dup(fileno(fP)) : -1);
    if (fd < 0) return;
    seq_ctx S;
    S.olp = olp; S.qlen = (float)(qe - qs); S.qs = qs; S.qe = qe; S.n1 = qs / G->nbp; S.failed = 0;
    g_core->nFiles = G->nFiles > 0 ? G->nFiles : INT32_MAX;  /* (no hits[] is indexed here; a caller may not have read the index file) */
    (void)igdc_walk_one(g_core, fd, ichr, qs, qe, 0, 0, IGD_HIP_RULE_NEST, NULL, emit_seq, &S);
    g_core->nFiles = G->nFiles;
    close(fd);
}

int32_t get_overlaps_f1(char *chrm, int32_t qs, int32_t qe) { return one_enumerate(chrm, qs, qe); } /* :537-620 */
int32_t get_overlaps_f0(char *chrm, int32_t qs, int32_t qe) { return one_enumerate(chrm, qs, qe); } /* :114-200 */

/* ------------------------------- hit map (-m) ----------------------------------------- */
static int64_t hit_map(uint32_t **hitmap, int use_v, int32_t v)
{
    igd_hip_db *dev = engine();
    if (!dev) return 0;
    const int32_t n = cur_igd()->nFiles;
    uint32_t *flat = (uint32_t *)calloc((size_t)n * (size_t)n + 1, sizeof(uint32_t));
    int64_t total = 0;
    int rc = igd_hip_hitmap(dev, use_v, v, flat, &total);
    if (rc != IGD_HIP_OK) { engine_failed("hitmap", rc); free(flat); return 0; }
    for (int32_t a = 0; a < n; a++)
        for (int32_t b = 0; b < n; b++) hitmap[a][b] += flat[(size_t)a * (size_t)n + (size_t)b];
    free(flat);
    /* the reference prints a progress counter every 1000 tiles while it works (:783-784) */
    int64_t tiles = 0;
    for (int32_t c = 0; c < cur_igd()->nCtg; c++) tiles += cur_igd()->nTile[c];
    for (int64_t m = 1000; m <= tiles; m += 1000) printf("%i\n", (int)m);
    return total;
}
int64_t getMap(uint32_t **hitmap) { return hit_map(hitmap, 0, 0); }                  /* :772-826 */
int64_t getMap_v(uint32_t **hitmap, int32_t v) { return hit_map(hitmap, 1, v); }      /* :829-886 */

/* ------------------------------- `igd search -Q <list>` ------------------------------- */
/* One query set per line of `list` (blank lines skipped, a trailing CR stripped).  For each set in list order: the line
 * "Query set <k>: <path>" and then exactly what `igd search <db> -q <path> [-v N]` prints for that file.  When all the sets
 * together hold at most igdc_host_limit() queries every file takes the `-q` route in turn (the host's for small files);
 * otherwise all of them are counted by ONE engine call (igd_hip_search_sets) on one device. */
static void print_hits_table(const int64_t *hits)
{
    printf("index\t number of regions\t number of hits\t File_name\n");
    int64_t total = 0;
    for (int32_t i = 0; i < IGD->nFiles; i++) {
        if (hits[i] > 0)
            printf("%i\t%i\t%lld\t%s\n", i, IGD->finfo[i].nr, (long long)hits[i], IGD->finfo[i].fileName);
        total += hits[i];
    }
    printf("Total: %lld\n", (long long)total);
}

static void count_file(char *qFile, int32_t v, int64_t *hits)                /* the counts of `-q` for one file (:1023-1030) */
{
    if (IGD->gType == 0) getOverlaps0(qFile, hits);
    else if (v > 0) getOverlaps_v(qFile, hits, v);
    else getOverlaps(qFile, hits);
}

static void search_sets(const cli_paths *P, int32_t v, int64_t *hits)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    const int32_t nfiles = IGD->nFiles, n = P->n;
    int rule;
    const int32_t ev = q_dispatch(v, &rule);
    cli_sets S;
    sets_load(&S, P);
    if (S.nq <= igdc_host_limit()) {
        /* every file through the `-q` route (it reads the file again: one code path for the text of a block) */
        for (int32_t k = 0; k < n && !g_fail_rc; k++) {
            memset(hits, 0, sizeof(int64_t) * (size_t)nfiles);
            sets_title(&S, k);
            count_file(S.paths[k], v, hits);
            if (!g_fail_rc) print_hits_table(hits);     /* (as `-q`: no table after an engine failure) */
        }
    } else {
        int64_t *rows = (int64_t *)calloc((size_t)n * (size_t)nfiles + 1, sizeof(int64_t));
        sets_cat(&S);
        double t0 = now_s();
        igd_hip_db *dev = engine();                   /* (IGD_DEVICES with several devices: the first one; -Q is one device) */
        if (dev) {
            const int rc = igd_hip_search_sets_ov(dev, S.ichr, S.qs, S.qe, S.off, n, ev, rule, 0, rows, NULL, g_mo);
            if (rc != IGD_HIP_OK) engine_failed("search", rc);
            phase("search of the query sets (H2D + kernels + D2H)", &t0);
        }
        for (int32_t k = 0; k < n && !g_fail_rc; k++) {
            sets_title(&S, k);
            print_hits_table(rows + (size_t)k * (size_t)nfiles);
        }
        free(rows);
    }
    sets_free(&S);
}

/* ------------------------------- `-K groups.tsv`: the tables of `-u` and `-U [-R]` per GROUP of datasets ----------------- */
/* One `dataset<TAB>group` pair per line: dataset is a file name exactly as the index lists it, or else a decimal dataset
 * number; the group's name is the rest of the line; `#` lines and blank lines are skipped; a dataset may occur on several
 * lines; groups are numbered in order of first appearance.  The relation is kept as include/igd_hip.h defines a grouping
 * (off, idx: CSR, ascending within a dataset's run), with the groups' names and their numbers of datasets.  g_grp.ng == 0:
 * no -K, and every table below is per dataset as it always was. */
typedef struct { int32_t ng, *off, *idx, *nds; char **names; } cli_groups;
static cli_groups g_grp = {0, NULL, NULL, NULL, NULL};

static void groups_free(void)
{
    for (int32_t g = 0; g < g_grp.ng; g++) free(g_grp.names[g]);
    free(g_grp.off); free(g_grp.idx); free(g_grp.nds); free(g_grp.names);
    memset(&g_grp, 0, sizeof g_grp);
}

static int pair_cmp(const void *a, const void *b)
{
    const int32_t *x = (const int32_t *)a, *y = (const int32_t *)b;
    return x[0] != y[0] ? (x[0] < y[0] ? -1 : 1) : x[1] != y[1] ? (x[1] < y[1] ? -1 : 1) : 0;
}

/* 0, or EX_USAGE after one "Not supported" line that names the file and, where there is one, the line */
static int groups_read(const char *path)
{
    FILE *fp = fopen(path, "r");
    if (!fp) { printf("Not supported: -K %s (cannot open the groups file)\n", path); return EX_USAGE; }
    const int32_t nf = IGD->nFiles;
    int32_t *pairs = NULL;
    int64_t npair = 0, cap = 0, lineno = 0;
    char *line = NULL;
    size_t lcap = 0;
    const char *why = NULL;
    g_grp.names = (char **)calloc((size_t)IGD_HIP_GROUP_MAX, sizeof(char *));
    while (!why && getline(&line, &lcap, fp) >= 0) {
        lineno++;
        size_t n = strlen(line);
        while (n && (line[n - 1] == '\n' || line[n - 1] == '\r')) line[--n] = '\0';
        size_t blank = 0;
        while (line[blank] == ' ' || line[blank] == '\t' || line[blank] == '\v' || line[blank] == '\f') blank++;
        if (line[blank] == '\0' || line[0] == '#') continue;
        char *tab = strchr(line, '\t');
        if (!tab || tab[1] == '\0') { why = "not a dataset, a tab and a group"; break; }
        *tab = '\0';
        const char *grp = tab + 1;
        int32_t f = -1;
        for (int32_t i = 0; i < nf && f < 0; i++) if (strcmp(IGD->finfo[i].fileName, line) == 0) f = i;
        if (f < 0 && line[0] != '\0' && strspn(line, "0123456789") == strlen(line) && strlen(line) < 10 && atol(line) < nf) f = (int32_t)atol(line);
        if (f < 0) { why = "the database has no such dataset"; break; }
        int32_t g = -1;
        for (int32_t i = 0; i < g_grp.ng && g < 0; i++) if (strcmp(g_grp.names[i], grp) == 0) g = i;
        if (g < 0) {
            if (g_grp.ng == IGD_HIP_GROUP_MAX) { why = "more than 8192 groups"; break; }
            g = g_grp.ng++;
            g_grp.names[g] = strdup(grp);
        }
        if (npair == cap) { cap = cap ? 2 * cap : 1024; pairs = (int32_t *)realloc(pairs, sizeof(int32_t) * 2 * (size_t)cap); }
        pairs[2 * npair] = f; pairs[2 * npair + 1] = g;
        npair++;
    }
    free(line);
    fclose(fp);
    if (!why && g_grp.ng == 0) { printf("Not supported: -K %s (the file names no group)\n", path); free(pairs); groups_free(); return EX_USAGE; }
    if (why) {
        printf("Not supported: -K %s, line %lld: %s\n", path, (long long)lineno, why);
        free(pairs);
        groups_free();
        return EX_USAGE;
    }
    qsort(pairs, (size_t)npair, 2 * sizeof(int32_t), pair_cmp);
    g_grp.off = (int32_t *)calloc((size_t)nf + 1, sizeof(int32_t));
    g_grp.idx = (int32_t *)calloc((size_t)npair + 1, sizeof(int32_t));
    g_grp.nds = (int32_t *)calloc((size_t)g_grp.ng, sizeof(int32_t));
    int32_t m = 0;
    for (int64_t i = 0; i < npair; i++) {
        if (i > 0 && pairs[2 * i] == pairs[2 * i - 2] && pairs[2 * i + 1] == pairs[2 * i - 1]) continue;     /* the same pair twice */
        g_grp.idx[m++] = pairs[2 * i + 1];
        g_grp.off[pairs[2 * i] + 1]++;
        g_grp.nds[pairs[2 * i + 1]]++;
    }
    for (int32_t f = 0; f < nf; f++) g_grp.off[f + 1] += g_grp.off[f];
    free(pairs);
    return 0;
}

/* the columns of the `-u` and `-U` tables: the datasets, or under -K the groups (their number of datasets where a dataset's
 * number of regions stands, their name where its file name stands) */
static int32_t table_cols(void) { return g_grp.ng ? g_grp.ng : IGD->nFiles; }
static int32_t col_count(int32_t i) { return g_grp.ng ? g_grp.nds[i] : IGD->finfo[i].nr; }
static const char *col_name(int32_t i) { return g_grp.ng ? g_grp.names[i] : IGD->finfo[i].fileName; }

/* ------------------------------- `igd search -q F -u` / `-Q <list> -u` ----------------- */
/* Support counts: per database file the number of QUERY REGIONS that overlap at least one of its records, where the table
 * of `-q` counts (query, record) pairs -- the count a region-set enrichment table is made of.  The table keeps the shape
 * of `-q`'s (third column: the support; last line: the query regions with any hit, of the accepted query lines).  Rule and
 * filter are `-q`'s dispatch for -v.  Route (cli_route, which this and the commands below share): igdc_support_host on the
 * host, ONE igd_hip_support_sets call on the engine. */
static void print_support_table(const int64_t *sup, int64_t nhit, int64_t nq)
{
    printf(g_grp.ng ? "index\t number of datasets\t number of query regions\t Group_name\n"
                    : "index\t number of regions\t number of query regions\t File_name\n");
    for (int32_t i = 0; i < table_cols(); i++)
        if (sup[i] > 0) printf("%i\t%i\t%lld\t%s\n", i, col_count(i), (long long)sup[i], col_name(i));
    printf("Query regions with a hit: %lld of %lld\n", (long long)nhit, (long long)nq);
}

/* `-b`: the same table with the covered base pairs in the third column (igdc_coverage_host / igd_hip_coverage_sets): per
 * database file the bp of the query regions that lie under its records, an interval union per query region.  Last line:
 * the bp under the records of any file, of the bp of the accepted query lines with end > start. */
static void print_coverage_table(const int64_t *cov, int64_t covered, int64_t qbp)
{
    printf("index\t number of regions\t covered bp\t File_name\n");
    for (int32_t i = 0; i < IGD->nFiles; i++)
        if (cov[i] > 0) printf("%i\t%i\t%lld\t%s\n", i, IGD->finfo[i].nr, (long long)cov[i], IGD->finfo[i].fileName);
    printf("Query bp with a hit: %lld of %lld\n", (long long)covered, (long long)qbp);
}

static void support_files(const cli_paths *P, int32_t v, int bp)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    const int32_t nfiles = table_cols(), n = P->n;    /* (under -K: the groups, and bp is 0) */
    const cli_groups *K = g_grp.ng ? &g_grp : NULL;
    int rule;
    const int32_t ev = q_dispatch(v, &rule);
    cli_sets S;
    sets_load(&S, P);
    const igdc_queries *q = S.q;
    int64_t *rows = (int64_t *)calloc((size_t)n * (size_t)nfiles + 1, sizeof(int64_t));
    int64_t *nhit = (int64_t *)calloc((size_t)n + 1, sizeof(int64_t));
    cli_route R;
    if (route_host(&R, S.nq)) {                       /* set by set: no concatenation on this route */
        int ok = 1;
        for (int32_t k = 0; k < n && ok; k++)
            if (q[k].n > 0)
                ok = (bp ? igdc_coverage_host(g_core, R.hm, q[k].ichr, q[k].qs, q[k].qe, q[k].n, ev, rule,
                                              rows + (size_t)k * (size_t)nfiles, &nhit[k])
                         : K ? igdc_group_support_host_ov(g_core, R.hm, q[k].ichr, q[k].qs, q[k].qe, q[k].n, K->off, K->idx, K->ng, ev, rule,
                                                          rows + (size_t)k * (size_t)nfiles, &nhit[k], g_mo)
                         : igdc_support_host_ov(g_core, R.hm, q[k].ichr, q[k].qs, q[k].qe, q[k].n, ev, rule,
                                                rows + (size_t)k * (size_t)nfiles, &nhit[k], g_mo)) == 0;
        if (!route_host_end(&R, ok, bp ? "covered base pairs on the host (small files)" : "support counts on the host (small files)")) {
            memset(rows, 0, sizeof(int64_t) * (size_t)n * (size_t)nfiles);      /* (the sets before the read error were counted) */
            memset(nhit, 0, sizeof(int64_t) * (size_t)n);
        }
    }
    if (!R.onHost && S.nq > 0) sets_cat(&S);
    if (route_engine(&R, S.nq > 0))
        route_engine_end(&R, bp ? "coverage" : "support",
                         bp ? igd_hip_coverage_sets(R.dev, S.ichr, S.qs, S.qe, S.off, n, ev, rule, rows, nhit)
                            : K ? igd_hip_group_support_sets(R.dev, S.ichr, S.qs, S.qe, S.off, n, K->off, K->idx, K->ng, ev, rule, rows, nhit, g_mo)
                            : igd_hip_support_sets_ov(R.dev, S.ichr, S.qs, S.qe, S.off, n, ev, rule, rows, nhit, g_mo),
                         bp ? "covered base pairs of the query sets (H2D + kernel + D2H)" : "support counts of the query sets (H2D + kernel + D2H)");
    for (int32_t k = 0; k < n && !g_fail_rc; k++) {   /* (as `-q`: no table after an engine failure) */
        sets_title(&S, k);
        if (bp) {
            int64_t qbp = 0;                          /* (64 bits: a line may span 2^32 - 1 bp) */
            for (int64_t i = 0; i < q[k].n; i++)
                if (q[k].qe[i] > q[k].qs[i]) qbp += (int64_t)q[k].qe[i] - (int64_t)q[k].qs[i];
            print_coverage_table(rows + (size_t)k * (size_t)nfiles, nhit[k], qbp);
        } else
            print_support_table(rows + (size_t)k * (size_t)nfiles, nhit[k], q[k].n);
    }
    sets_free(&S);
    free(rows); free(nhit);
}

/* ------------------------------- `igd search -q F -J` / `-Q <list> -J` ----------------- */
/* Base-pair Jaccard (include/igd_hip.h has the definitions): the query set is merged at gap 0, and per database file the table
 * gives the bp of the intersection with the union of the file's records, the bp of the union of the two, the Jaccard, the
 * fraction of the set's bp inside the file (set_fraction) and the file's merged bp; every file has a line.  Last line: the
 * same against the records of any file.  A ratio over 0 is printed as NA.  Rule and filter are `-q`'s dispatch for -v.
 * Route: igdc_jaccard_host, or ONE igd_hip_jaccard_sets call. */
static void print_ratio(int64_t num, int64_t den)
{
    if (den != 0) printf("%.6f", (double)num / (double)den);
    else printf("NA");
}

static void print_jaccard_table(const int64_t *inter, int64_t set_bp, const int64_t *file_bp, int64_t n_merged, int64_t n_dropped)
{
    const int32_t nf = IGD->nFiles;
    printf("index\tintersection\tunion\tjaccard\tset_fraction\tfile_bp\tFile\n");
    for (int32_t i = 0; i < nf; i++) {
        const int64_t u = set_bp + file_bp[i] - inter[i];
        printf("%i\t%lld\t%lld\t", i, (long long)inter[i], (long long)u);
        print_ratio(inter[i], u);
        printf("\t");
        print_ratio(inter[i], set_bp);
        printf("\t%lld\t%s\n", (long long)file_bp[i], IGD->finfo[i].fileName);
    }
    printf("Any dataset: %lld of %lld bp in %lld merged regions (%lld dropped); jaccard ", (long long)inter[nf], (long long)set_bp,
           (long long)n_merged, (long long)n_dropped);
    print_ratio(inter[nf], set_bp + file_bp[nf] - inter[nf]);
    printf("\n");
}

static void jaccard_files(const cli_paths *P, int32_t v)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    const size_t nc = (size_t)IGD->nFiles + 1;
    const int32_t n = P->n;
    int rule;
    const int32_t ev = q_dispatch(v, &rule);
    cli_sets S;
    sets_load(&S, P);
    sets_cat(&S);
    int64_t *inter = (int64_t *)calloc((size_t)(n ? n : 1) * nc, sizeof(int64_t));
    int64_t *file_bp = (int64_t *)calloc(nc, sizeof(int64_t));
    int64_t *per = (int64_t *)calloc(3 * (size_t)(n ? n : 1), sizeof(int64_t)), *set_bp = per, *n_merged = per + n, *n_dropped = per + 2 * (size_t)n;
    cli_route R;
    if (route_host(&R, S.nq))
        route_host_end(&R, igdc_jaccard_host(g_core, R.hm, S.ichr, S.qs, S.qe, S.off, n, ev, rule, inter, set_bp, file_bp, n_merged, n_dropped) == 0,
                       "base-pair Jaccard on the host (small files)");
    if (route_engine(&R, 1))                              /* no gate on the regions: the table needs file_bp of every dataset, also for empty sets */
        route_engine_end(&R, "jaccard", igd_hip_jaccard_sets(R.dev, S.ichr, S.qs, S.qe, S.off, n, ev, rule, inter, set_bp, file_bp, n_merged, n_dropped),
                         "base-pair Jaccard of the query sets (merge + coverage)");
    for (int32_t k = 0; k < n && !g_fail_rc; k++) {       /* (as `-q`: no table after an engine failure) */
        sets_title(&S, k);
        print_jaccard_table(inter + (size_t)k * nc, set_bp[k], file_bp, n_merged[k], n_dropped[k]);
    }
    sets_free(&S);
    free(inter); free(file_bp); free(per);
}

/* ------------------------------- `igd search -q F -U <universe>` / `-Q <list> -U <universe>` ----------------- */
/* Region-set enrichment: per query set and database file the 2x2 table of a one-sided Fisher exact test against a
 * background universe, the LOLA table.  With the supports of `-u` (same rule and -v filter for sets and universe), n_k
 * accepted lines in the set and n_U in the universe:
 *     a = support of the set      b = u - a  (u = support of the universe)      c = n_k - a      d = n_U - a - b - c
 * a negative b or d is printed and tested as 0 and counted in "clamped cells" (a set region outside the universe, or a
 * universe region under several set regions; `-X` below restricts the sets to the universe first).  oddsRatio = (a d) / (b c), the
 * sample odds ratio; pValueLog = -log10 P(X >= a), X ~ Hypergeometric(a+b+c+d, a+b, a+c).  One row per file with a > 0.
 * Route, the universe's lines counted with the sets': igdc_support_host and igdc_fisher_host, or ONE igd_hip_enrich_sets_nhit call.
 * With `-R` six more columns follow the file name: rnkSup, rnkPV, rnkOR -- the file's rank among ALL files of the set, those
 * with a = 0 included, by support, pValueLog and oddsRatio (ties take the minimum rank) -- maxRnk, meanRnk and qValueLog,
 * -log10 of the Benjamini-Hochberg adjusted p over the set's nFiles tests (include/igd_hip.h: igd_hip_enrich_ranks).  They come
 * from igdc_rank_host where the supports came from the host, otherwise from igd_hip_enrich_ranks.  Lines and their order are
 * those without `-R`.
 * With `-X` every set is first replaced by the universe regions it overlaps (igd_hip_restrict_sets has the definition; LOLA's
 * redefineUserSets): n_k becomes size[k] = the number of those regions, the supports are sums over them, every table is a
 * partition of the universe (b = u - a, c = size[k] - a, d = n_U - u - c, nothing to clamp), and the last line reads
 *     Restricted regions with a hit: <nhit> of <size> (from <n> query regions); universe regions: <n_U>
 * Lines of the set or the universe whose contig the database does not know are dropped by the reader, as everywhere: they
 * are in no restricted set and not in n_U.  Route: igdc_enrich_restricted_host, or ONE igd_hip_enrich_restricted call.  `-X`
 * without `-U` is refused. */
/* b, c, d and the clamp count of every cell from the definitions (printed on both routes; the host route tests them) */
static void enrich_tables(const int64_t *rows, const int64_t *urow, const igdc_queries *q, int64_t nU, int32_t n, int32_t nfiles,
                          int64_t *tb, int64_t *tc, int64_t *td, int64_t *clamped)
{
    for (int32_t k = 0; k < n; k++) {
        clamped[k] = 0;
        for (int32_t f = 0; f < nfiles; f++) {
            const size_t i = (size_t)k * (size_t)nfiles + (size_t)f;
            const int64_t b = urow[f] - rows[i], c = q[k].n - rows[i], d = nU - rows[i] - b - c;
            if (b < 0 || d < 0) clamped[k]++;
            tb[i] = b < 0 ? 0 : b; tc[i] = c; td[i] = d < 0 ? 0 : d;
        }
    }
}

/* -X: b, c, d of every cell from the restricted supports and sizes; nothing is clamped */
static void enrich_tables_restricted(const int64_t *rows, const int64_t *urow, const int64_t *size, int64_t nU, int32_t n, int32_t nfiles,
                                     int64_t *tb, int64_t *tc, int64_t *td)
{
    for (int32_t k = 0; k < n; k++)
        for (int32_t f = 0; f < nfiles; f++) {
            const size_t i = (size_t)k * (size_t)nfiles + (size_t)f;
            tb[i] = urow[f] - rows[i];
            tc[i] = size[k] - rows[i];
            td[i] = nU - urow[f] - tc[i];
        }
}

static void enrich_files(const cli_paths *P, const char *uniName, int32_t v, int ranks, int restricted)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    const int32_t nfiles = table_cols(), n = P->n;    /* (under -K: the groups, and restricted is 0) */
    const cli_groups *K = g_grp.ng ? &g_grp : NULL;
    int rule;
    const int32_t ev = q_dispatch(v, &rule);
    igdc_queries uq;
    memset(&uq, 0, sizeof uq);
    if (igdc_read_queries(g_core, uniName, 1, &uq) != 0 || uq.n == 0) {
        printf("Cannot read universe file %s, or it holds no region\n", uniName);
        igdc_queries_free(&uq);
        return;
    }
    cli_sets S;
    sets_load(&S, P);
    const igdc_queries *q = S.q;
    const size_t cells = (size_t)n * (size_t)nfiles;
    int64_t *rows = (int64_t *)calloc(cells + 1, sizeof(int64_t)), *urow = (int64_t *)calloc((size_t)nfiles + 1, sizeof(int64_t));
    int64_t *nhit = (int64_t *)calloc((size_t)n + 1, sizeof(int64_t)), unhit = 0;
    int64_t *tb = (int64_t *)calloc(3 * cells + 1, sizeof(int64_t)), *tc = tb + cells, *td = tc + cells;
    int64_t *clamped = (int64_t *)calloc((size_t)n + 1, sizeof(int64_t)), *size = (int64_t *)calloc((size_t)n + 1, sizeof(int64_t));
    double *plog = (double *)calloc(2 * cells + 1, sizeof(double)), *odds = plog + cells;
    /* -R: q and mean, then the four int32 columns */
    double *qlog = ranks ? (double *)calloc(4 * cells + 1, sizeof(double)) : NULL, *rmean = ranks ? qlog + cells : NULL;
    int32_t *rsup = ranks ? (int32_t *)(rmean + cells) : NULL, *rpv = ranks ? rsup + cells : NULL, *ror = ranks ? rpv + cells : NULL;
    int32_t *rmax = ranks ? ror + cells : NULL;
    cli_route R;
    if (route_host(&R, S.nq + uq.n)) {
        int ok;
        if (restricted) {
            sets_cat(&S);
            ok = igdc_enrich_restricted_host(g_core, R.hm, S.ichr, S.qs, S.qe, S.off, n, uq.ichr, uq.qs, uq.qe, uq.n, ev, rule, rows, urow, size,
                                             plog, odds, NULL, nhit, &unhit) == 0;
            if (ok) enrich_tables_restricted(rows, urow, size, uq.n, n, nfiles, tb, tc, td);
        } else {
            ok = (K ? igdc_group_support_host_ov(g_core, R.hm, uq.ichr, uq.qs, uq.qe, uq.n, K->off, K->idx, K->ng, ev, rule, urow, &unhit, g_mo)
                    : igdc_support_host_ov(g_core, R.hm, uq.ichr, uq.qs, uq.qe, uq.n, ev, rule, urow, &unhit, g_mo)) == 0;
            for (int32_t k = 0; k < n && ok; k++)
                if (q[k].n > 0)
                    ok = (K ? igdc_group_support_host_ov(g_core, R.hm, q[k].ichr, q[k].qs, q[k].qe, q[k].n, K->off, K->idx, K->ng, ev, rule,
                                                         rows + (size_t)k * (size_t)nfiles, &nhit[k], g_mo)
                            : igdc_support_host_ov(g_core, R.hm, q[k].ichr, q[k].qs, q[k].qe, q[k].n, ev, rule, rows + (size_t)k * (size_t)nfiles,
                                                   &nhit[k], g_mo)) == 0;
            if (ok) {
                enrich_tables(rows, urow, q, uq.n, n, nfiles, tb, tc, td, clamped);
                ok = igdc_fisher_host(rows, tb, tc, td, (int64_t)cells, plog, odds) == 0;
            }
        }
        if (ok && ranks) ok = igdc_rank_host(rows, plog, odds, n, nfiles, qlog, rsup, rpv, ror, rmax, rmean) == 0;
        if (!route_host_end(&R, ok, restricted ? "restricted sets, membership of the universe and Fisher tests on the host (small files)"
                                               : "support counts and Fisher tests on the host (small files)")) {
            memset(rows, 0, sizeof(int64_t) * cells);                           /* (what was counted before the read error) */
            memset(urow, 0, sizeof(int64_t) * (size_t)nfiles);
            memset(nhit, 0, sizeof(int64_t) * (size_t)n);
            unhit = 0;
        }
    }
    if (!R.onHost) sets_cat(&S);
    if (route_engine(&R, 1)) {                        /* (no gate: the universe holds a region) */
        const int rc = restricted
                           ? igd_hip_enrich_restricted(R.dev, S.ichr, S.qs, S.qe, S.off, n, uq.ichr, uq.qs, uq.qe, uq.n, ev, rule, rows, urow, size,
                                                       plog, odds, NULL, nhit, &unhit)
                           : K ? igd_hip_group_enrich_sets(R.dev, S.ichr, S.qs, S.qe, S.off, n, uq.ichr, uq.qs, uq.qe, uq.n, K->off, K->idx, K->ng, ev,
                                                           rule, rows, urow, plog, odds, NULL, nhit, &unhit, g_mo)
                           : igd_hip_enrich_sets_ov(R.dev, S.ichr, S.qs, S.qe, S.off, n, uq.ichr, uq.qs, uq.qe, uq.n, ev, rule, rows, urow, plog,
                                                    odds, NULL, nhit, &unhit, g_mo);
        if (rc == IGD_HIP_OK && restricted) enrich_tables_restricted(rows, urow, size, uq.n, n, nfiles, tb, tc, td);
        else if (rc == IGD_HIP_OK) enrich_tables(rows, urow, q, uq.n, n, nfiles, tb, tc, td, clamped);
        route_engine_end(&R, "enrichment", rc, restricted ? "enrichment of the restricted sets (join + membership of the universe + gather + Fisher kernel)"
                                                          : "enrichment of the query sets (H2D + support kernel + Fisher kernel + D2H)");
        if (ranks && rc == IGD_HIP_OK)
            route_engine_end(&R, "enrichment ranks", igd_hip_enrich_ranks(R.dev, rows, plog, odds, n, nfiles, qlog, rsup, rpv, ror, rmax, rmean),
                             "ranks and q-values of the enrichment table (H2D + rank kernel + D2H)");
    }
    for (int32_t k = 0; k < n && !g_fail_rc; k++) {   /* (as `-q`: no table after an engine failure) */
        sets_title(&S, k);
        printf("index\t number of %s\t support\t b\t c\t d\t oddsRatio\t pValueLog\t %s%s\n", K ? "datasets" : "regions", K ? "Group_name" : "File_name",
               ranks ? "\t rnkSup\t rnkPV\t rnkOR\t maxRnk\t meanRnk\t qValueLog" : "");
        for (int32_t f = 0; f < nfiles; f++) {
            const size_t i = (size_t)k * (size_t)nfiles + (size_t)f;
            if (rows[i] <= 0) continue;
            printf("%i\t%i\t%lld\t%lld\t%lld\t%lld\t%.4f\t%.4f\t%s", f, col_count(f), (long long)rows[i], (long long)tb[i],
                   (long long)tc[i], (long long)td[i], odds[i], plog[i], col_name(f));
            if (ranks) printf("\t%d\t%d\t%d\t%d\t%.2f\t%.4f", (int)rsup[i], (int)rpv[i], (int)ror[i], (int)rmax[i], rmean[i], qlog[i]);
            printf("\n");
        }
        if (restricted)
            printf("Restricted regions with a hit: %lld of %lld (from %lld query regions); universe regions: %lld\n", (long long)nhit[k],
                   (long long)size[k], (long long)q[k].n, (long long)uq.n);
        else
            printf("Query regions with a hit: %lld of %lld; universe regions: %lld; clamped cells: %lld\n", (long long)nhit[k],
                   (long long)q[k].n, (long long)uq.n, (long long)clamped[k]);
    }
    sets_free(&S);
    igdc_queries_free(&uq);
    free(rows); free(urow); free(nhit); free(tb); free(clamped); free(size); free(plog); free(qlog);
}

/* ------------------------------- `igd search -q F -w` / `-Q <list> -w` ----------------- */
/* Per-query membership: one line per accepted query line, in input order,
 *     contig \t start \t end \t n \t list
 * with the database's name of the contig (`.`: it has no such contig), the number n of datasets the region overlaps and
 * their indices, ascending and comma-separated (`.` when n is 0) -- the rows of the matrix whose column sums `-u` prints;
 * then `-u`'s last line.  Rule and filter are `-q`'s dispatch for -v.  Routing as `-u`: at most igdc_host_limit() queries in
 * all go through igdc_membership_host, more through igd_hip_membership on one device.  The queries are taken in chunks of
 * at most MEMBER_CHUNK_QUERIES queries and MEMBER_CHUNK_BYTES of rows, and the text leaves in pieces of about
 * MEMBER_TEXT_BYTES: a file of 10^6 lines never holds the whole matrix or the whole text. */
#define MEMBER_CHUNK_QUERIES ((int64_t)1 << 16)
#define MEMBER_CHUNK_BYTES ((int64_t)64 << 20)
#define MEMBER_TEXT_BYTES ((size_t)1 << 20)

typedef struct { char *s; size_t n, cap; } textbuf;

static int text_room(textbuf *t, size_t more)
{
    if (t->n + more <= t->cap) return 1;
    size_t nc = t->cap ? t->cap : (size_t)1 << 16;
    while (nc < t->n + more) nc *= 2;
    char *ns = (char *)realloc(t->s, nc);
    if (!ns) return 0;
    t->s = ns; t->cap = nc;
    return 1;
}

static void text_flush(textbuf *t)
{
    if (t->n) fwrite(t->s, 1, t->n, stdout);
    t->n = 0;
}

static size_t put_uint(char *p, uint32_t x)
{
    char d[12];
    size_t k = 0;
    do { d[k++] = (char)('0' + x % 10); x /= 10; } while (x);
    for (size_t i = 0; i < k; i++) p[i] = d[k - 1 - i];
    return k;
}

/* the lines of the queries [a, b) of one file from their rows */
static int member_lines(textbuf *t, const igdc_queries *q, int64_t a, int64_t b, const uint32_t *bits, const int32_t *nfh, int32_t nW)
{
    for (int64_t i = a; i < b; i++) {
        const uint32_t *row = bits + (size_t)(i - a) * (size_t)nW;
        const int32_t c = q->ichr[i], n = nfh[i - a];
        const char *name = (c >= 0 && c < IGD->nCtg) ? IGD->cName[c] : ".";
        if (!text_room(t, strlen(name) + 64 + (size_t)n * 11)) return 0;
        t->n += (size_t)sprintf(t->s + t->n, "%s\t%d\t%d\t%d\t", name, (int)q->qs[i], (int)q->qe[i], (int)n);
        if (n == 0) t->s[t->n++] = '.';
        int first = 1;
        for (int32_t w = 0; w < nW; w++)
            for (uint32_t x = row[w]; x; x &= x - 1) {
                if (!first) t->s[t->n++] = ',';
                first = 0;
                t->n += put_uint(t->s + t->n, (uint32_t)w * 32u + (uint32_t)__builtin_ctz(x));
            }
        t->s[t->n++] = '\n';
        if (t->n >= MEMBER_TEXT_BYTES) text_flush(t);
    }
    return 1;
}

static void membership_files(const cli_paths *P, int32_t v)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    const int32_t nfiles = IGD->nFiles, nW = (nfiles + 31) / 32, n = P->n;
    int rule;
    const int32_t ev = q_dispatch(v, &rule);
    cli_sets S;
    sets_load(&S, P);
    const igdc_queries *q = S.q;
    int64_t step = MEMBER_CHUNK_BYTES / ((int64_t)(nW ? nW : 1) * 4);
    step = step < 1 ? 1 : step > MEMBER_CHUNK_QUERIES ? MEMBER_CHUNK_QUERIES : step;
    /* (not a cli_route: the rows are asked for chunk by chunk, and a read error moves the remaining chunks to the engine) */
    igdc_map *hm = host_map_lim(S.nq, igdc_host_limit());
    igd_hip_db *dev = NULL;
    if (!hm && S.nq > 0 && !(dev = engine())) {       /* no device: nothing of the table is printed */
        sets_free(&S);
        return;
    }
    uint32_t *bits = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)step * (size_t)(nW ? nW : 1));
    int32_t *nfh = (int32_t *)malloc(sizeof(int32_t) * (size_t)step);
    textbuf t = {NULL, 0, 0};
    double t0 = now_s();
    for (int32_t k = 0; k < n && !g_fail_rc; k++) {
        if (S.setLines && text_room(&t, strlen(S.paths[k]) + 64))        /* (sets_title(), into the text buffer) */
            t.n += (size_t)sprintf(t.s + t.n, "Query set %d: %s\n", (int)k, S.paths[k]);
        int64_t nhit = 0;
        for (int64_t a = 0; a < q[k].n && !g_fail_rc; a += step) {
            const int64_t b = a + step < q[k].n ? a + step : q[k].n;
            int done = 0;
            if (hm) {
                done = igdc_membership_host(g_core, hm, q[k].ichr + a, q[k].qs + a, q[k].qe + a, b - a, ev, rule, bits, nfh, &nhit) == 0;
                if (!done) { igdc_map_close(hm); hm = NULL; }     /* (a read error: the engine reads the file its own way) */
            }
            if (!done) {
                if (!dev) dev = engine();
                if (!dev) break;
                const int rc = igd_hip_membership(dev, q[k].ichr + a, q[k].qs + a, q[k].qe + a, b - a, ev, rule, bits, nfh, &nhit);
                if (rc != IGD_HIP_OK) { engine_failed("membership", rc); break; }
            }
            if (!member_lines(&t, &q[k], a, b, bits, nfh, nW)) { fprintf(stderr, "igd: out of memory\n"); break; }
        }
        if (!g_fail_rc && text_room(&t, 96))
            t.n += (size_t)sprintf(t.s + t.n, "Query regions with a hit: %lld of %lld\n", (long long)nhit, (long long)q[k].n);
    }
    text_flush(&t);
    phase(hm ? "membership rows on the host (small files)" : "membership rows of the query files (H2D + kernel + D2H + text)", &t0);
    if (hm) igdc_map_close(hm);
    sets_free(&S);
    free(bits); free(nfh); free(t.s);
}

/* ------------------------------- `igd search -q F -C` ----------------------------------- */
/* Dataset co-occurrence over the regions of one query file: the header
 *     index_a \t index_b \t support_a \t support_b \t both \t jaccard \t File_a \t File_b
 * and one line per pair of datasets a < b that at least one region overlaps both of, in ascending (a, b): the regions that
 * overlap a, that overlap b, that overlap both, and the Jaccard index both / (support_a + support_b - both) as %.6f; then
 * `-u`'s last line.  Rule and filter are `-q`'s dispatch for -v.  Route: igdc_cooccur_host, or igd_hip_cooccur.  The text leaves
 * in pieces of about MEMBER_TEXT_BYTES. */
static void cooccur_file(char *path, int32_t v)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    const int32_t nfiles = IGD->nFiles;
    if (nfiles > IGD_COOCCUR_MAX_FILES) {
        printf("Not supported: -C with more than %d datasets\n", (int)IGD_COOCCUR_MAX_FILES);
        return;
    }
    int rule;
    const int32_t ev = q_dispatch(v, &rule);
    igdc_queries q;
    if (igdc_read_queries(g_core, path, 1, &q) != 0) memset(&q, 0, sizeof q);                  /* unreadable: an empty set */
    int64_t *cooc = (int64_t *)calloc((size_t)nfiles * (size_t)nfiles + 1, sizeof(int64_t));
    int64_t nhit = 0;
    if (!cooc) { fprintf(stderr, "igd: out of memory\n"); igdc_queries_free(&q); return; }
    cli_route R;
    if (route_host(&R, q.n))
        route_host_end(&R, igdc_cooccur_host(g_core, R.hm, q.ichr, q.qs, q.qe, q.n, ev, rule, cooc, &nhit) == 0, "co-occurrence on the host (small files)");
    if (route_engine(&R, q.n > 0))
        route_engine_end(&R, "co-occurrence", igd_hip_cooccur(R.dev, q.ichr, q.qs, q.qe, q.n, ev, rule, cooc, &nhit),
                         "co-occurrence of the query file (H2D + membership + transpose + Gram kernels + D2H)");
    if (!g_fail_rc) {
        textbuf t = {NULL, 0, 0};
        int ok = text_room(&t, 128);
        if (ok) t.n += (size_t)sprintf(t.s + t.n, "index_a\tindex_b\tsupport_a\tsupport_b\tboth\tjaccard\tFile_a\tFile_b\n");
        for (int32_t a = 0; a < nfiles && ok; a++) {
            const int64_t sa = cooc[(size_t)a * (size_t)nfiles + (size_t)a];
            if (sa == 0) continue;
            const char *na = IGD->finfo[a].fileName;
            for (int32_t b = a + 1; b < nfiles && ok; b++) {
                const int64_t both = cooc[(size_t)a * (size_t)nfiles + (size_t)b];
                if (both <= 0) continue;
                const int64_t sb = cooc[(size_t)b * (size_t)nfiles + (size_t)b];
                const char *nb = IGD->finfo[b].fileName;
                ok = text_room(&t, strlen(na) + strlen(nb) + 160);
                if (!ok) break;
                t.n += (size_t)sprintf(t.s + t.n, "%d\t%d\t%lld\t%lld\t%lld\t%.6f\t%s\t%s\n", (int)a, (int)b, (long long)sa, (long long)sb,
                                       (long long)both, (double)both / (double)(sa + sb - both), na, nb);
                if (t.n >= MEMBER_TEXT_BYTES) text_flush(&t);
            }
        }
        if (ok && text_room(&t, 96))
            t.n += (size_t)sprintf(t.s + t.n, "Query regions with a hit: %lld of %lld\n", (long long)nhit, (long long)q.n);
        else fprintf(stderr, "igd: out of memory\n");
        text_flush(&t);
        free(t.s);
    }
    igdc_queries_free(&q);
    free(cooc);
}

/* ------------------------------- the options of `igd search` ----------------------------- */
/* What search_parse makes of argv, read by search_check and by the commands.  `given` has one bit per option (O_x; B(x)), and
 * behind those the facts that the parse derives from the order and from the values (F_x; F(x)), so that a row of RULES can ask
 * for either in one mask.  A valued option's bit says that a value was met, except -L and -r, which count bare too. */
enum { O_f = 1, O_m, O_s, O_u, O_b, O_w, O_X, O_C, O_G, O_E, O_R, O_J, O_q, O_r, O_v, O_Q, O_U, O_P, O_g, O_S, O_M, O_O, O_A, O_B, O_N,
       O_H, O_L, O_V, O_D, O_W, O_K, O_Z, O_o, O_I, O_COUNT,
       F_q = O_COUNT, F_r, F_m, F_s,      /* the mode: the last of -q, -r, -m and -s (-s does not count after -r) */
       F_PERSET,                          /* -u, -b and -w have their sets: mode -q, or -Q with no mode at all */
       F_MINOV,                           /* -O, -A or -B */
       F_RESAMPLE,                        /* -P and -M resample */
       F_BAD_P, F_BAD_M, F_BAD_Z, F_BAD_D, F_BAD_N, F_BAD_V, F_BAD_L, F_BAD_H,       /* the value does not parse (-M: neither circular nor shuffle) */
       F_L_BARE,                          /* -L without a value */
       F_V_BLIND,                         /* -V with an op other than count on a database without values */
       F_BAD_I, F_I_BLIND,                /* the same two facts of -I */
       F_COUNT };
_Static_assert(F_COUNT <= 64, "the options and facts of igd search share one 64-bit mask");
#define B(x) (1ULL << O_##x)
#define F(x) (1ULL << F_##x)

typedef struct {
    uint64_t given;
    char *val[O_COUNT];                   /* the value of a valued option (-r: the contig), or NULL */
    int mode, cmd;                        /* F_q, F_r, F_m, F_s or 0; the CMD_ that search_check chose */
    /* every value parsed once */
    int32_t v, qs, qe;                    /* -v; -r's start and end */
    long long np;                         /* -P (0: none) */
    uint64_t seed;                        /* -S */
    int pmode;                            /* IGD_HIP_PERM_: -W's, -M resample's, or -M's */
    int32_t distW, nearW, flankBins;      /* -D (-1: none), -N, -L */
    int32_t histEdges[IGD_HIP_NEAREST_MAX_EDGES];
    int histNe, mapOp, inOp;              /* -H; -V's and -I's index in MAP_OPS (-1: none) */
    int32_t *shiftOff;                    /* -Z: malloc'd offsets */
    int nShift;
} cli_opts;

/* ------------------------------- `igd search -q F -P N -g genome` ------------------------ */
/* Permutation null of the support counts of one query file: the regions are shifted along their contigs (-M circular, the
 * default: one offset per permutation and contig) or placed anew on them (-M shuffle) N times, seed -S (default 0); the
 * contig lengths come from the genome file (`name<TAB>length`).  The header
 *     index \t observed \t mean \t sd \t z \t n_ge \t n_le \t nlog10_p_upper \t nlog10_p_lower \t File
 * and one line per dataset: the support of the file as given, mean and standard deviation of the permuted supports, the
 * z-score, the permutations with a support >= / <= the observed one and -log10 of (n + 1) / (N + 1) for both (floats as
 * %.6f); then `-u`'s last line followed by the same seven statistics of the regions with a hit in any dataset.  Rule and
 * filter are `-q`'s dispatch for -v.  Route, decided on regions x (N + 1) and with no gate on them: igdc_permute_host, or
 * igd_hip_permute_support.  A region outside its contig's length, or on a contig the genome file lacks, ends the run with a
 * message that names the line. */
/* `-D W` switches the statistic from support to distance (permute_nearest_table below); window < 0: the support. */
static void permute_nearest_table(const igdc_queries *q, const int32_t *len, int64_t nperm, uint64_t seed, int pmode, int32_t ev, int32_t window);
/* `-W workspace.bed` places the regions inside a workspace (include/igd_hip.h: THE WORKSPACE; pmode is IGD_HIP_PERM_WORKSPACE then
 * and -M is refused): the file is read as a query file is, built into the table once (igdc_read_workspace) and handed to the _ws
 * form of the statistic's route; the three tables keep their layout.  A workspace without a usable segment and a region that
 * fits in no segment of its contig end the run with a message (the latter names the line) and exit code EX_USAGE; regions that
 * do not lie inside the workspace as given are counted on stderr and the run goes on.  g_ws: the table of the run, or NULL. */
static const igd_hip_workspace *g_ws = NULL;
/* `-M resample -U universe.bed` draws every permuted set from the universe instead of placing it (include/igd_hip.h: THE DRAW;
 * pmode is IGD_HIP_PERM_RESAMPLE then, -g and -W are refused): the universe is read as `-U` reads it everywhere, there is no genome
 * file and no region is held against a contig's length, and the statistic's route is the _rs form; the three tables keep their
 * layout.  A set larger than the universe ends the run with a message on stderr and exit code EX_USAGE; the set need not be a subset
 * of the universe.  g_pool: the universe of the run, or NULL. */
static const igdc_queries *g_pool = NULL;
/* `-G` switches it to base pairs (permute_bp_table below); it takes no sum of squares on the device, so the guard on it does not apply. */
static void permute_bp_table(const igdc_queries *q, const int32_t *len, int64_t nperm, uint64_t seed, int pmode, int32_t ev, int rule);
/* `-I op` switches it to the values of the overlapping records (permute_map_table below); opName: the index in MAP_OPS. */
static void permute_map_table(const igdc_queries *q, const int32_t *len, int64_t nperm, uint64_t seed, int pmode, int32_t ev, int opName);
/* `-Z W,STEP` prints the shift profile of the support instead (shift_table below): nshift > 0 offsets; nperm may be 0 then. */
static void shift_table(const igdc_queries *q, const int32_t *len, const int32_t *offsets, int nshift, int64_t nperm, uint64_t seed, int pmode,
                        int32_t ev, int rule);
static void permute_file(const cli_opts *o)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    char *path = o->val[O_q];
    const char *genome = o->val[O_g], *wsName = o->val[O_W], *uniName = o->pmode == IGD_HIP_PERM_RESAMPLE ? o->val[O_U] : NULL;
    const int64_t nperm = o->np;
    const uint64_t seed = o->seed;
    const int pmode = o->pmode, gbp = (o->given & B(G)) != 0;
    const int32_t v = o->v, window = o->distW;
    const int32_t nfiles = IGD->nFiles, nC = nfiles + 1;
    int rule;
    const int32_t ev = q_dispatch(v, &rule);
    int32_t *len = (int32_t *)calloc((size_t)g_core->nCtg + 1, sizeof(int32_t));
    int64_t bad = 0;
    const int grc = !len ? -1 : uniName ? 0 : igdc_read_genome(g_core, genome, len, &bad);   /* (resampling: no genome file) */
    if (grc == -1) { printf("Cannot open genome file %s\n", genome); free(len); return; }
    if (grc != 0) {
        printf("Genome file %s, line %lld: not a name, a tab and a length of at most 2147483647\n", genome, (long long)bad);
        free(len);
        return;
    }
    /* the accepted lines as igdc_read_queries accepts them, read here so that a refusal can name its line */
    igdc_queries q;
    memset(&q, 0, sizeof q);
    int64_t no = 0, *lineOf = NULL, lineCap = 0;                             /* -W: the line of every accepted region */
    igd_hip_workspace *ws = NULL;
    igdc_queries uq;                                                         /* -M resample: the universe */
    memset(&uq, 0, sizeof uq);
    igdc_lines *r = igdc_lines_open(path);
    char *line;
    while (r && (line = igdc_lines_next(r, NULL)) != NULL) {
        int32_t st, en;
        no++;
        char *chrm = igdc_parse_bed(line, &st, &en, 1);
        if (!chrm) continue;
        const int32_t id = igdc_get_id(g_core, chrm);
        if (id < 0) continue;
        if (uniName) {                                                       /* (nothing is placed: no region is held against a length) */
            if (igdc_queries_push(&q, id, st, en) != 0) { fprintf(stderr, "igd: out of memory\n"); goto done; }
            continue;
        }
        if (len[id] < 1) {
            printf("%s, line %lld: contig %s is not in the genome file %s\n", path, (long long)no, g_core->cName[id], genome);
            goto done;
        }
        if (st < 0 || en < st || en > len[id]) {
            printf("%s, line %lld: region %s:%d-%d does not lie on its contig of length %d\n", path, (long long)no, g_core->cName[id],
                   (int)st, (int)en, (int)len[id]);
            goto done;
        }
        if (wsName && q.n == lineCap) {
            int64_t *grown = (int64_t *)realloc(lineOf, sizeof(int64_t) * (size_t)(lineCap ? 2 * lineCap : 1024));
            if (!grown) { fprintf(stderr, "igd: out of memory\n"); goto done; }
            lineOf = grown; lineCap = lineCap ? 2 * lineCap : 1024;
        }
        if (igdc_queries_push(&q, id, st, en) != 0) { fprintf(stderr, "igd: out of memory\n"); goto done; }
        if (wsName) lineOf[q.n - 1] = no;
    }
    if (wsName) {
        const int wrc = igdc_read_workspace(g_core, wsName, len, &ws);
        if (wrc == -1) { printf("Cannot open workspace file %s\n", wsName); goto done; }
        if (wrc != 0) { fprintf(stderr, "igd: out of memory\n"); goto done; }
        if (ws->nseg == 0) {
            printf("Workspace file %s: no usable segment on a contig of the database\n", wsName);
            g_usage_rc = 1;
            goto done;
        }
        const int64_t bad_i = igdc_workspace_first_unplaceable(ws, len, q.ichr, q.qs, q.qe, q.n);
        if (bad_i >= 0) {
            printf("%s, line %lld: region %s:%d-%d fits in no segment of the workspace %s on its contig\n", path, (long long)lineOf[bad_i],
                   g_core->cName[q.ichr[bad_i]], (int)q.qs[bad_i], (int)q.qe[bad_i], wsName);
            g_usage_rc = 1;
            goto done;
        }
        const int64_t outside = igdc_workspace_outside(ws, q.ichr, q.qs, q.qe, q.n);
        if (outside > 0) fprintf(stderr, "%lld of %lld regions do not lie inside the workspace\n", (long long)outside, (long long)q.n);
        g_ws = ws;
    }
    if (uniName) {
        if (igdc_read_queries(g_core, uniName, 1, &uq) != 0 || uq.n == 0) {
            printf("Cannot read universe file %s, or it holds no region\n", uniName);
            goto done;
        }
        if (q.n > uq.n) {
            fprintf(stderr, "Not supported: -M resample with a set of %lld regions, more than the %lld of the universe %s\n", (long long)q.n,
                    (long long)uq.n, uniName);
            g_usage_rc = 1;
            goto done;
        }
        if (uq.n > igd_hip_max_batch()) {
            fprintf(stderr, "Not supported: -M resample with a universe of %lld regions, more than %lld\n", (long long)uq.n,
                    (long long)igd_hip_max_batch());
            g_usage_rc = 1;
            goto done;
        }
        g_pool = &uq;
    }
    if (q.n > igd_hip_max_batch() ||
        (window < 0 && !gbp && o->inOp < 0 && (unsigned __int128)nperm * (unsigned __int128)q.n * (unsigned __int128)q.n >= (unsigned __int128)1 << 63)) {
        printf("Not supported: -P %lld with %lld regions\n", (long long)nperm, (long long)q.n);
        goto done;
    }
    if (o->nShift > 0) shift_table(&q, len, o->shiftOff, o->nShift, nperm, seed, pmode, ev, rule);
    else if (gbp) permute_bp_table(&q, len, nperm, seed, pmode, ev, rule);
    else if (o->inOp >= 0) permute_map_table(&q, len, nperm, seed, pmode, ev, o->inOp);
    else if (window >= 0) permute_nearest_table(&q, len, nperm, seed, pmode, ev, window);
    else {
        int64_t *st7 = (int64_t *)calloc(7 * (size_t)nC, sizeof(int64_t));
        double *fl = (double *)calloc(5 * (size_t)nC, sizeof(double));
        if (!st7 || !fl) { fprintf(stderr, "igd: out of memory\n"); free(st7); free(fl); goto done; }
        int64_t *obs = st7, *sum = obs + nC, *ssq = sum + nC, *nge = ssq + nC, *nle = nge + nC, *mn = nle + nC, *mx = mn + nC;
        cli_route R;
        if (route_host(&R, q.n * (nperm + 1)))
            route_host_end(&R, (g_pool ? igdc_permute_host_rs(g_core, R.hm, q.ichr, q.qs, q.qe, q.n, g_pool->ichr, g_pool->qs, g_pool->qe, g_pool->n, seed,
                                                              nperm, ev, rule, obs, sum, ssq, nge, nle, mn, mx, g_mo)
                                       : igdc_permute_host_ws(g_core, R.hm, q.ichr, q.qs, q.qe, q.n, len, pmode, seed, nperm, ev, rule, obs, sum, ssq, nge, nle, mn, mx, g_mo, g_ws)) == 0,
                           "permutation null on the host (small files)");
        if (route_engine(&R, 1))
            route_engine_end(&R, "permutation null",
                             g_pool ? igd_hip_permute_support_rs(R.dev, q.ichr, q.qs, q.qe, q.n, g_pool->ichr, g_pool->qs, g_pool->qe, g_pool->n, seed, nperm, ev,
                                                                 rule, obs, sum, ssq, nge, nle, mn, mx, g_mo)
                                    : igd_hip_permute_support_ws(R.dev, q.ichr, q.qs, q.qe, q.n, len, pmode, seed, nperm, ev, rule, obs, sum, ssq, nge, nle, mn, mx, g_mo, g_ws),
                             "permutation null of the query file (H2D + permute, support and statistics kernels + D2H)");
        if (!g_fail_rc && igdc_perm_summary(obs, sum, ssq, nge, nle, nperm, nC, fl, fl + nC, fl + 2 * nC, fl + 3 * nC, fl + 4 * nC) == 0) {
            printf("index\tobserved\tmean\tsd\tz\tn_ge\tn_le\tnlog10_p_upper\tnlog10_p_lower\tFile\n");
            for (int32_t i = 0; i < nfiles; i++)
                printf("%d\t%lld\t%.6f\t%.6f\t%.6f\t%lld\t%lld\t%.6f\t%.6f\t%s\n", (int)i, (long long)obs[i], fl[i], fl[nC + i], fl[2 * nC + i],
                       (long long)nge[i], (long long)nle[i], fl[3 * nC + i], fl[4 * nC + i], IGD->finfo[i].fileName);
            const int32_t a = nfiles;
            printf("Query regions with a hit: %lld of %lld\t%.6f\t%.6f\t%.6f\t%lld\t%lld\t%.6f\t%.6f\n", (long long)obs[a], (long long)q.n, fl[a],
                   fl[nC + a], fl[2 * nC + a], (long long)nge[a], (long long)nle[a], fl[3 * nC + a], fl[4 * nC + a]);
        }
        free(st7); free(fl);
    }
done:
    if (r) igdc_lines_close(r);
    igdc_queries_free(&q);
    g_ws = NULL;
    g_pool = NULL;
    igdc_queries_free(&uq);
    igdc_workspace_free(ws);
    free(lineOf);
    free(len);
}

/* ------------------------------- `igd search -q F -g genome -Z W,STEP [-P N]` ---------- */
/* Local z-score: the support of every dataset with the whole query file moved rigidly by each offset (include/igd_hip.h: THE
 * SHIFT).  Without -P the header `index \t File \t shift_<d> ..` and one line per dataset with the integer supports, then a line
 * `any \t -` with the regions that have a hit in any dataset.  With -P N the columns observed, mean and sd (%.6f; `NA` for the sd
 * of one permutation) of -P's null stand in front, and every shift is printed as z = (support - mean) / sd, %.4f, `NA` where sd
 * is 0 or undefined.  The file, the genome file and the workspace are read and checked by permute_file.  Route, decided on
 * regions x (shifts + N + 1): igdc_shift_support_host_ov and igdc_permute_host_ws, or igd_hip_shift_support and
 * igd_hip_permute_support_ws. */
static void shift_table(const igdc_queries *q, const int32_t *len, const int32_t *offsets, int nshift, int64_t nperm, uint64_t seed, int pmode,
                        int32_t ev, int rule)
{
    const int32_t nfiles = IGD->nFiles, nC = nfiles + 1;
    int64_t *sh = (int64_t *)calloc((size_t)nshift * (size_t)nC, sizeof(int64_t));
    int64_t *st7 = (int64_t *)calloc(7 * (size_t)nC, sizeof(int64_t));
    double *fl = (double *)calloc(2 * (size_t)nC, sizeof(double));
    if (!sh || !st7 || !fl) { fprintf(stderr, "igd: out of memory\n"); free(sh); free(st7); free(fl); return; }
    int64_t *obs = st7, *sum = obs + nC, *ssq = sum + nC, *nge = ssq + nC, *nle = nge + nC, *mn = nle + nC, *mx = mn + nC;
    cli_route R;
    if (route_host(&R, q->n * ((int64_t)nshift + (nperm > 0 ? nperm + 1 : 0))))
        route_host_end(&R, igdc_shift_support_host_ov(g_core, R.hm, q->ichr, q->qs, q->qe, q->n, len, offsets, nshift, ev, rule, sh, g_mo) == 0 &&
                               (nperm < 1 || igdc_permute_host_ws(g_core, R.hm, q->ichr, q->qs, q->qe, q->n, len, pmode, seed, nperm, ev, rule, obs, sum,
                                                                  ssq, nge, nle, mn, mx, g_mo, g_ws) == 0),
                       "shift profile on the host (small files)");
    if (route_engine(&R, 1)) {
        int rc = igd_hip_shift_support(R.dev, q->ichr, q->qs, q->qe, q->n, len, offsets, nshift, ev, rule, sh, g_mo);
        if (rc == IGD_HIP_OK && nperm > 0)
            rc = igd_hip_permute_support_ws(R.dev, q->ichr, q->qs, q->qe, q->n, len, pmode, seed, nperm, ev, rule, obs, sum, ssq, nge, nle, mn, mx, g_mo, g_ws);
        route_engine_end(&R, "shift profile", rc, "shift profile of the query file (H2D + shift and support kernels + D2H)");
    }
    if (!g_fail_rc && (nperm < 1 || igdc_perm_summary(obs, sum, ssq, nge, nle, nperm, nC, fl, fl + nC, NULL, NULL, NULL) == 0)) {
        printf("index\tFile%s", nperm > 0 ? "\tobserved\tmean\tsd" : "");
        for (int j = 0; j < nshift; j++) printf("\tshift_%d", (int)offsets[j]);
        printf("\n");
        for (int32_t i = 0; i <= nfiles; i++) {               /* (i = nfiles: the any-dataset column) */
            const double mean = fl[i], sd = fl[nC + i];
            if (i < nfiles) printf("%d\t%s", (int)i, IGD->finfo[i].fileName);
            else printf("any\t-");
            if (nperm > 0) {
                printf("\t%lld\t%.6f", (long long)obs[i], mean);
                if (sd == sd) printf("\t%.6f", sd); else printf("\tNA");
            }
            for (int j = 0; j < nshift; j++) {
                const int64_t x = sh[(size_t)j * (size_t)nC + (size_t)i];
                if (nperm < 1) printf("\t%lld", (long long)x);
                else if (sd != sd || sd == 0.0) printf("\tNA");
                else printf("\t%.4f", ((double)x - mean) / sd);
            }
            printf("\n");
        }
    }
    free(sh); free(st7); free(fl);
}

/* `-Z W,STEP`: the offsets -k STEP .. k STEP, k = W / STEP, into a malloc'd array; 0 for anything but two whole numbers with
 * 0 <= W <= 2^30, STEP >= 1 and at most IGD_HIP_SHIFT_MAX shifts */
static int parse_shifts(const char *arg, int32_t **offsets)
{
    char *end = NULL;
    if (arg[0] < '0' || arg[0] > '9') return 0;
    const long long w = strtoll(arg, &end, 10);
    if (*end != ',' || end[1] < '0' || end[1] > '9' || w > (long long)IGD_HIP_SHIFT_MAX_OFFSET) return 0;
    const char *p = end + 1;
    const long long step = strtoll(p, &end, 10);
    if (*end || step < 1) return 0;
    const long long k = w / step;
    if (2 * k + 1 > IGD_HIP_SHIFT_MAX) return 0;
    int32_t *o = (int32_t *)malloc(sizeof(int32_t) * (size_t)(2 * k + 1));
    if (!o) return 0;
    for (long long j = -k; j <= k; j++) o[j + k] = (int32_t)(j * step);
    *offsets = o;
    return (int)(2 * k + 1);
}

/* ------------------------------- `igd search -q F -N <bp>` / `-Q <list> -N <bp>` ------- */
/* Nearest record per dataset within a window (include/igd_hip.h has the definitions): per database file the query regions
 * with a record of the file within W bp (n_within), those that overlap one (n_overlap) and the mean distance of the former
 * (mean_dist, `NA` where there is none); one line per dataset, then the same for "any dataset".  -v keeps the records with
 * value >= v, as everywhere; there is no tile rule.  Route: igdc_nearest_sets_host, or ONE igd_hip_nearest_sets call. */
static void print_mean(const char *before, int64_t n_within, double mean, const char *after)
{
    if (n_within > 0) printf("%s%.2f%s", before, mean, after);
    else printf("%sNA%s", before, after);
}

static void nearest_files(const cli_paths *P, int32_t v, int32_t window)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    const int32_t nfiles = IGD->nFiles, n = P->n;
    const size_t nC = (size_t)nfiles + 1;
    const int32_t ev = q_dispatch(v, NULL);
    cli_sets S;
    sets_load(&S, P);
    sets_cat(&S);
    const igdc_queries *q = S.q;
    int64_t *st3 = (int64_t *)calloc(3 * (size_t)(n ? n : 1) * nC, sizeof(int64_t));
    double *mean = (double *)malloc(sizeof(double) * (size_t)(n ? n : 1) * nC);
    int64_t *nw = st3, *no = st3 + (size_t)n * nC, *sd = st3 + 2 * (size_t)n * nC;
    cli_route R;
    if (route_host(&R, S.nq))
        route_host_end(&R, igdc_nearest_sets_host(g_core, R.hm, S.ichr, S.qs, S.qe, S.off, n, window, ev, nw, no, sd) == 0,
                       "nearest records on the host (small files)");
    if (route_engine(&R, S.nq > 0))
        route_engine_end(&R, "nearest", igd_hip_nearest_sets(R.dev, S.ichr, S.qs, S.qe, S.off, n, window, ev, nw, no, sd),
                         "nearest records of the query sets (H2D + kernels + D2H)");
    if (!g_fail_rc) igdc_nearest_summary(nw, sd, (int64_t)n * (int64_t)nC, mean);
    for (int32_t k = 0; k < n && !g_fail_rc; k++) {   /* (as `-q`: no table after an engine failure) */
        const size_t o = (size_t)k * nC;
        sets_title(&S, k);
        printf("index\tn_within\tn_overlap\tmean_dist\tFile\n");
        for (int32_t i = 0; i < nfiles; i++) {
            printf("%d\t%lld\t%lld", (int)i, (long long)nw[o + i], (long long)no[o + i]);
            print_mean("\t", nw[o + i], mean[o + i], "\t");
            printf("%s\n", IGD->finfo[i].fileName);
        }
        printf("Regions with a dataset within %d bp: %lld of %lld; overlapping: %lld", (int)window, (long long)nw[o + nfiles], (long long)q[k].n,
               (long long)no[o + nfiles]);
        print_mean("; mean distance ", nw[o + nfiles], mean[o + nfiles], "\n");
    }
    sets_free(&S);
    free(st3); free(mean);
}

/* ------------------------------- `igd search -q F -N <bp> -H e1,e2,..` / `-Q <list> -N <bp> -H ..` ------- */
/* Histogram of the signed nearest distances (include/igd_hip.h has the definitions): per database file the query regions with
 * a record of the file within W bp (n_within) and their number per bin of the signed distance -- negative: the nearest record
 * lies upstream -- under the columns `<e1`, `[e1,e2)`, .., `>=e_ne`; one line per dataset, then the same for "any dataset".
 * -v, routing and the layout of -Q blocks as -N: the host answers with igdc_nearest_hist_host, the engine with ONE
 * igd_hip_nearest_hist call. */
static int parse_edges(const char *arg, int32_t *edges)                     /* the number of edges, or -1 for a refused list */
{
    int ne = 0;
    for (const char *p = arg;;) {
        char *end = NULL;
        if (p[0] != '-' && (p[0] < '0' || p[0] > '9')) return -1;           /* (strtoll's leading blanks and '+' are not the list's) */
        const long long x = strtoll(p, &end, 10);                           /* (out of range: LLONG_MIN / LLONG_MAX, refused below) */
        if (end == p || (*end != ',' && *end != '\0') || x < (long long)INT32_MIN || x > (long long)INT32_MAX) return -1;
        if (ne == IGD_HIP_NEAREST_MAX_EDGES || (ne > 0 && (int32_t)x <= edges[ne - 1])) return -1;
        edges[ne++] = (int32_t)x;
        if (*end == '\0') return ne;
        p = end + 1;
    }
}

/* the lines under the header of -H's and -L's table: per dataset, and then for "any dataset", the sum of the bins and the bins */
static void print_hist_rows(const int64_t *h, size_t nB, int32_t window, int64_t nq)
{
    const int32_t nfiles = IGD->nFiles;
    const size_t nC = (size_t)nfiles + 1;
    for (int32_t i = 0; i <= nfiles; i++) {           /* (i = nfiles: the any-dataset column) */
        int64_t nw = 0;
        for (size_t b = 0; b < nB; b++) nw += h[b * nC + (size_t)i];
        if (i < nfiles) printf("%d\t%lld", (int)i, (long long)nw);
        else printf("Any dataset within %d bp: %lld of %lld", (int)window, (long long)nw, (long long)nq);
        for (size_t b = 0; b < nB; b++) printf("\t%lld", (long long)h[b * nC + (size_t)i]);
        if (i < nfiles) printf("\t%s\n", IGD->finfo[i].fileName);
        else printf("\n");
    }
}

static void nearest_hist_files(const cli_paths *P, int32_t v, int32_t window, const int32_t *edges, int ne)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    const int32_t n = P->n;
    const size_t nC = (size_t)IGD->nFiles + 1, nB = (size_t)ne + 1;
    const int32_t ev = q_dispatch(v, NULL);
    cli_sets S;
    sets_load(&S, P);
    sets_cat(&S);
    int64_t *hist = (int64_t *)calloc((size_t)(n ? n : 1) * nB * nC, sizeof(int64_t));
    cli_route R;
    if (route_host(&R, S.nq))
        route_host_end(&R, igdc_nearest_hist_host(g_core, R.hm, S.ichr, S.qs, S.qe, S.off, n, window, ev, edges, ne, hist) == 0,
                       "histogram of the nearest distances on the host (small files)");
    if (route_engine(&R, S.nq > 0))
        route_engine_end(&R, "nearest histogram", igd_hip_nearest_hist(R.dev, S.ichr, S.qs, S.qe, S.off, n, window, ev, edges, ne, hist),
                         "histogram of the nearest distances of the query sets (H2D + kernels + D2H)");
    for (int32_t k = 0; k < n && !g_fail_rc; k++) {   /* (as `-q`: no table after an engine failure) */
        sets_title(&S, k);
        printf("index\tn_within\t<%d", (int)edges[0]);
        for (int b = 1; b < ne; b++) printf("\t[%d,%d)", (int)edges[b - 1], (int)edges[b]);
        printf("\t>=%d\tFile\n", (int)edges[ne - 1]);
        print_hist_rows(hist + (size_t)k * nB * nC, nB, window, S.q[k].n);
    }
    sets_free(&S);
    free(hist);
}

/* ------------------------------- `igd search -q F -N <bp> -L <bins> [-E]` / `-Q <list> -N <bp> -L ..` ------- */
/* Histogram of the relative distance (include/igd_hip.h has the definitions; `bedtools reldist`): per database file the query
 * regions that have a record of the file on BOTH sides within W bp (n_flanked) and their number per bin of min(up, down) /
 * (up + down), under the bins' lower bounds k / (2 B); one line per dataset, then the same for "any dataset".  The distances
 * are measured between midpoints, with -E between edges.  -v, routing and the layout of -Q blocks as -N: the host answers with
 * igdc_flank_reldist_host, the engine with ONE igd_hip_flank_reldist call. */
static void flank_reldist_files(const cli_paths *P, int32_t v, int32_t window, int measure, int32_t nbins)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    const int32_t n = P->n;
    const size_t nC = (size_t)IGD->nFiles + 1, nB = (size_t)nbins;
    const int32_t ev = q_dispatch(v, NULL);
    cli_sets S;
    sets_load(&S, P);
    sets_cat(&S);
    int64_t *hist = (int64_t *)calloc((size_t)(n ? n : 1) * nB * nC, sizeof(int64_t));
    cli_route R;
    if (route_host(&R, S.nq))
        route_host_end(&R, igdc_flank_reldist_host(g_core, R.hm, S.ichr, S.qs, S.qe, S.off, n, window, measure, ev, nbins, hist) == 0,
                       "histogram of the relative distances on the host (small files)");
    if (route_engine(&R, S.nq > 0))
        route_engine_end(&R, "relative-distance histogram", igd_hip_flank_reldist(R.dev, S.ichr, S.qs, S.qe, S.off, n, window, measure, ev, nbins, hist),
                         "histogram of the relative distances of the query sets (H2D + kernels + D2H)");
    for (int32_t k = 0; k < n && !g_fail_rc; k++) {   /* (as `-q`: no table after an engine failure) */
        sets_title(&S, k);
        printf("index\tn_flanked");
        for (int b = 0; b < nbins; b++) printf("\t%.4f", (double)b / (double)(2 * nbins));
        printf("\tFile\n");
        print_hist_rows(hist + (size_t)k * nB * nC, nB, window, S.q[k].n);
    }
    sets_free(&S);
    free(hist);
}

/* ------------------------------- `igd search -q F -V <op>` / `-Q <list> -V <op>` ------- */
/* Values of the overlapping records per dataset (include/igd_hip.h has the definitions): per database file the query regions
 * with a counted record (n_hit), the counted (region, record) pairs (pairs) and a mean -- of the per-region count, sum, minimum
 * or maximum over the regions with a hit (mean_region) or, for `mean`, of the values over the pairs (op SUM, mean_pair); `NA`
 * where the divisor is 0.  One line per dataset, then the pairs of all datasets and the datasets with a hit.  -v keeps the
 * records with value >= v, as everywhere; there is no tile rule.  Route: igdc_map_sets_host, or ONE igd_hip_map_sets call. */
static const char *const MAP_OPS[] = {"count", "sum", "min", "max", "mean"};
static const int MAP_OP_OF[] = {IGD_HIP_MAP_COUNT, IGD_HIP_MAP_SUM, IGD_HIP_MAP_MIN, IGD_HIP_MAP_MAX, IGD_HIP_MAP_SUM};

static void map_files(const cli_paths *P, int32_t v, int opName)
{
    if (!g_core || !cur_igd()) { engine(); return; }
    const int op = MAP_OP_OF[opName], perPair = opName == 4;
    const int32_t nfiles = IGD->nFiles, n = P->n;
    const size_t nC = (size_t)nfiles;
    const int32_t ev = q_dispatch(v, NULL);
    cli_sets S;
    sets_load(&S, P);
    sets_cat(&S);
    int64_t *st3 = (int64_t *)calloc(3 * (size_t)(n ? n : 1) * nC + 1, sizeof(int64_t));
    double *mean = (double *)malloc(sizeof(double) * (2 * (size_t)(n ? n : 1) * nC + 1));
    int64_t *nh = st3, *np = st3 + (size_t)n * nC, *sa = st3 + 2 * (size_t)n * nC;
    double *meanPair = mean + (size_t)n * nC;
    cli_route R;
    if (route_host(&R, S.nq))
        route_host_end(&R, igdc_map_sets_host(g_core, R.hm, S.ichr, S.qs, S.qe, S.off, n, op, ev, nh, np, sa) == 0,
                       "values of the overlapping records on the host (small files)");
    if (route_engine(&R, S.nq > 0))
        route_engine_end(&R, "map", igd_hip_map_sets(R.dev, S.ichr, S.qs, S.qe, S.off, n, op, ev, nh, np, sa),
                         "values of the overlapping records of the query sets (H2D + kernels + D2H)");
    if (!g_fail_rc) igdc_map_summary(nh, np, sa, (int64_t)n * (int64_t)nC, op, mean, meanPair);
    for (int32_t k = 0; k < n && !g_fail_rc; k++) {   /* (as `-q`: no table after an engine failure) */
        const size_t o = (size_t)k * nC;
        int64_t all = 0, withHit = 0;
        sets_title(&S, k);
        printf("index\tn_hit\tpairs\tmean_%s\tFile\n", MAP_OPS[opName]);
        for (int32_t i = 0; i < nfiles; i++) {
            printf("%d\t%lld\t%lld", (int)i, (long long)nh[o + i], (long long)np[o + i]);
            print_mean("\t", perPair ? np[o + i] : nh[o + i], perPair ? meanPair[o + i] : mean[o + i], "\t");
            printf("%s\n", IGD->finfo[i].fileName);
            all += np[o + i];
            withHit += nh[o + i] > 0;
        }
        printf("Pairs: %lld; datasets with a hit: %lld of %d\n", (long long)all, (long long)withHit, (int)nfiles);
    }
    sets_free(&S);
    free(st3); free(mean);
}

/* ------------------------------- `igd search -q F -P N -g genome -D <bp>` --------------- */
/* Permutation null of the nearest-record distances (include/igd_hip.h: igd_hip_permute_nearest; igd_core.h:
 * igdc_perm_nearest_summary has the columns): "are my regions closer to dataset f than chance".  The header
 *     index n_within mean_dist within_mean within_sd within_z nlog10_p_within_upper dist_mean dist_sd dist_z n_def dist_n_le
 *     nlog10_p_dist_lower File                                                                       (tab-separated)
 * and one line per dataset; floats as %.6f, mean_dist and dist_mean as %.2f as under -N, NaN as NA; then -N's last line for
 * the set as given, followed by the same statistics (within_mean .. nlog10_p_dist_lower) of the any-dataset column.  Routing
 * as -P: regions x (N + 1) against igdc_host_limit(). */
static void print_na(const char *fmt, double x, const char *after)
{
    if (x != x) printf("NA%s", after);
    else { printf(fmt, x); printf("%s", after); }
}

static void permute_nearest_table(const igdc_queries *q, const int32_t *len, int64_t nperm, uint64_t seed, int pmode, int32_t ev, int32_t window)
{
    const int32_t nfiles = IGD->nFiles;
    const size_t nC = (size_t)nfiles + 1, R = (size_t)nperm + 1;
    int64_t *st3 = (int64_t *)calloc(3 * R * nC + 3 * nC, sizeof(int64_t));
    double *fl = (double *)calloc(9 * nC, sizeof(double));
    if (!st3 || !fl) { fprintf(stderr, "igd: out of memory\n"); free(st3); free(fl); return; }
    int64_t *nw = st3, *no = nw + R * nC, *sd = no + R * nC, *nge = sd + R * nC, *ndef = nge + nC, *nle = ndef + nC;
    double *wm = fl, *ws = wm + nC, *wz = ws + nC, *pu = wz + nC, *md = pu + nC, *dm = md + nC, *ds = dm + nC, *dz = ds + nC, *pl = dz + nC;
    cli_route Rt;
    if (route_host(&Rt, q->n * (nperm + 1)))
        route_host_end(&Rt, (g_pool ? igdc_permute_nearest_host_rs(g_core, Rt.hm, q->ichr, q->qs, q->qe, q->n, g_pool->ichr, g_pool->qs, g_pool->qe, g_pool->n,
                                                                   seed, nperm, window, ev, nw, no, sd)
                                    : igdc_permute_nearest_host_ws(g_core, Rt.hm, q->ichr, q->qs, q->qe, q->n, len, pmode, seed, nperm, window, ev, nw, no, sd, g_ws)) == 0,
                       "permutation null of the distances on the host (small files)");
    if (route_engine(&Rt, 1))
        route_engine_end(&Rt, "permutation null of the distances",
                         g_pool ? igd_hip_permute_nearest_rs(Rt.dev, q->ichr, q->qs, q->qe, q->n, g_pool->ichr, g_pool->qs, g_pool->qe, g_pool->n, seed, nperm,
                                                             window, ev, nw, no, sd)
                                : igd_hip_permute_nearest_ws(Rt.dev, q->ichr, q->qs, q->qe, q->n, len, pmode, seed, nperm, window, ev, nw, no, sd, g_ws),
                         "permutation null of the distances (H2D + permute and fused nearest kernels + D2H)");
    if (!g_fail_rc && igdc_perm_nearest_summary(nw, sd, nperm, (int64_t)nC, wm, ws, wz, nge, pu, md, dm, ds, dz, ndef, nle, pl) == 0) {
        printf("index\tn_within\tmean_dist\twithin_mean\twithin_sd\twithin_z\tnlog10_p_within_upper\tdist_mean\tdist_sd\tdist_z\tn_def\tdist_n_le\t"
               "nlog10_p_dist_lower\tFile\n");
        for (int32_t i = 0; i <= nfiles; i++) {
            if (i < nfiles) {
                printf("%d\t%lld\t", (int)i, (long long)nw[i]);
                print_na("%.2f", md[i], "\t");
            } else {
                printf("Regions with a dataset within %d bp: %lld of %lld; overlapping: %lld", (int)window, (long long)nw[i], (long long)q->n,
                       (long long)no[i]);
                print_mean("; mean distance ", nw[i], md[i], "\t");
            }
            print_na("%.6f", wm[i], "\t"); print_na("%.6f", ws[i], "\t"); print_na("%.6f", wz[i], "\t"); print_na("%.6f", pu[i], "\t");
            print_na("%.2f", dm[i], "\t"); print_na("%.6f", ds[i], "\t"); print_na("%.6f", dz[i], "\t");
            printf("%lld\t%lld\t", (long long)ndef[i], (long long)nle[i]);
            print_na("%.6f", pl[i], i < nfiles ? "\t" : "\n");
            if (i < nfiles) printf("%s\n", IGD->finfo[i].fileName);
        }
    }
    free(st3); free(fl);
}

/* ------------------------------- `igd search -q F -P N -g genome -I <op>` -------------- */
/* Permutation null of the values of the overlapping records (include/igd_hip.h: igd_hip_permute_map; igd_core.h:
 * igdc_perm_map_summary has the columns): "are the scores of dataset f's records under my regions higher or lower than chance"
 * (regioneR's meanInRegions).  -I is to -V what -D is to -N.  The statistic is -V's mean: of the per-region count, sum, minimum
 * or maximum over the regions with a hit, or, for `mean`, of the values over the pairs (the rows of op SUM).  The header
 *     index observed_n_hit observed_mean_<op> n_def mean sd z n_ge n_le mlog10p_ge mlog10p_le nhit_mean nhit_sd nhit_z File
 * (tab-separated) and one line per dataset; floats as %.6f, NaN as NA.  -v keeps the records with value >= v, as everywhere;
 * there is no tile rule.  Routing as -P: regions x (N + 1) against igdc_host_limit(). */
static void permute_map_table(const igdc_queries *q, const int32_t *len, int64_t nperm, uint64_t seed, int pmode, int32_t ev, int opName)
{
    const int op = MAP_OP_OF[opName], perPair = opName == 4;
    const int32_t nfiles = IGD->nFiles;
    const size_t nC = (size_t)nfiles, R = (size_t)nperm + 1;
    int64_t *st3 = (int64_t *)calloc(3 * R * nC + 3 * nC + 1, sizeof(int64_t));
    double *fl = (double *)calloc(9 * nC + 1, sizeof(double));
    if (!st3 || !fl) { fprintf(stderr, "igd: out of memory\n"); free(st3); free(fl); return; }
    int64_t *nh = st3, *np = nh + R * nC, *sa = np + R * nC, *ndef = sa + R * nC, *nge = ndef + nC, *nle = nge + nC;
    double *ob = fl, *mu = ob + nC, *sd = mu + nC, *z = sd + nC, *pu = z + nC, *pl = pu + nC, *hm = pl + nC, *hs = hm + nC, *hz = hs + nC;
    cli_route Rt;
    if (route_host(&Rt, q->n * (nperm + 1)))
        route_host_end(&Rt, (g_pool ? igdc_permute_map_host_rs(g_core, Rt.hm, q->ichr, q->qs, q->qe, q->n, g_pool->ichr, g_pool->qs, g_pool->qe, g_pool->n,
                                                               seed, nperm, op, ev, nh, np, sa)
                                    : igdc_permute_map_host_ws(g_core, Rt.hm, q->ichr, q->qs, q->qe, q->n, len, pmode, seed, nperm, op, ev, nh, np, sa, g_ws)) == 0,
                       "permutation null of the values on the host (small files)");
    if (route_engine(&Rt, 1))
        route_engine_end(&Rt, "permutation null of the values",
                         g_pool ? igd_hip_permute_map_rs(Rt.dev, q->ichr, q->qs, q->qe, q->n, g_pool->ichr, g_pool->qs, g_pool->qe, g_pool->n, seed, nperm,
                                                         op, ev, nh, np, sa)
                                : igd_hip_permute_map_ws(Rt.dev, q->ichr, q->qs, q->qe, q->n, len, pmode, seed, nperm, op, ev, nh, np, sa, g_ws),
                         "permutation null of the values (H2D + permute and fused map kernels + D2H)");
    if (!g_fail_rc && igdc_perm_map_summary(nh, np, sa, nperm, (int64_t)nC, perPair, ob, ndef, mu, sd, z, nge, nle, pu, pl, hm, hs, hz) == 0) {
        printf("index\tobserved_n_hit\tobserved_mean_%s\tn_def\tmean\tsd\tz\tn_ge\tn_le\tmlog10p_ge\tmlog10p_le\tnhit_mean\tnhit_sd\tnhit_z\tFile\n",
               MAP_OPS[opName]);
        for (int32_t i = 0; i < nfiles; i++) {
            printf("%d\t%lld\t", (int)i, (long long)nh[i]);
            print_na("%.6f", ob[i], "\t");
            printf("%lld\t", (long long)ndef[i]);
            print_na("%.6f", mu[i], "\t"); print_na("%.6f", sd[i], "\t"); print_na("%.6f", z[i], "\t");
            printf("%lld\t%lld\t", (long long)nge[i], (long long)nle[i]);
            print_na("%.6f", pu[i], "\t"); print_na("%.6f", pl[i], "\t");
            print_na("%.6f", hm[i], "\t"); print_na("%.6f", hs[i], "\t"); print_na("%.6f", hz[i], "\t");
            printf("%s\n", IGD->finfo[i].fileName);
        }
    }
    free(st3); free(fl);
}

/* ------------------------------- `igd search -q F -P N -g genome -G` ------------------- */
/* Permutation null of the base-pair overlap (include/igd_hip.h: igd_hip_permute_bp; igd_core.h: igdc_perm_bp_summary has the
 * columns): "does my region set share more base pairs with dataset f than chance".  -G is to -J what -D is to -N.  The header
 *     index observed_bp mean sd z fold n_ge n_le nlog10_p_upper nlog10_p_lower jaccard jaccard_mean File     (tab-separated)
 * and one line per dataset; floats as %.6f, NaN as NA; then -J's last line for the set as given (without its Jaccard),
 * followed by the same statistics (mean .. jaccard_mean) of the any-dataset column.  Rule and filter are `-q`'s dispatch for
 * -v.  Routing as -P: regions x (N + 1) against igdc_host_limit(). */
static void permute_bp_table(const igdc_queries *q, const int32_t *len, int64_t nperm, uint64_t seed, int pmode, int32_t ev, int rule)
{
    const int32_t nfiles = IGD->nFiles;
    const size_t nC = (size_t)nfiles + 1, R = (size_t)nperm + 1;
    int64_t *st = (int64_t *)calloc(R * nC + 2 * R + 1 + 4 * nC, sizeof(int64_t));
    double *fl = (double *)calloc(9 * nC, sizeof(double));
    if (!st || !fl) { fprintf(stderr, "igd: out of memory\n"); free(st); free(fl); return; }
    int64_t *inter = st, *sbp = inter + R * nC, *nm = sbp + R, *nd = nm + R, *fbp = nd + 1, *obs = fbp + nC, *nge = obs + nC, *nle = nge + nC;
    double *mu = fl, *sd = mu + nC, *z = sd + nC, *fold = z + nC, *pu = fold + nC, *pl = pu + nC, *jac = pl + nC, *jm = jac + nC, *js = jm + nC;
    cli_route Rt;
    if (route_host(&Rt, q->n * (nperm + 1)))
        route_host_end(&Rt, (g_pool ? igdc_permute_bp_host_rs(g_core, Rt.hm, q->ichr, q->qs, q->qe, q->n, g_pool->ichr, g_pool->qs, g_pool->qe, g_pool->n, seed,
                                                              nperm, ev, rule, inter, sbp, nm, nd)
                                    : igdc_permute_bp_host_ws(g_core, Rt.hm, q->ichr, q->qs, q->qe, q->n, len, pmode, seed, nperm, ev, rule, inter, sbp, nm, nd, g_ws)) == 0 &&
                           igdc_dataset_bp_host(g_core, Rt.hm, ev, rule, fbp) == 0,
                       "permutation null of the base-pair overlap on the host (small files)");
    if (route_engine(&Rt, 1)) {
        int rc = g_pool ? igd_hip_permute_bp_rs(Rt.dev, q->ichr, q->qs, q->qe, q->n, g_pool->ichr, g_pool->qs, g_pool->qe, g_pool->n, seed, nperm, ev, rule,
                                                inter, sbp, nm, nd)
                        : igd_hip_permute_bp_ws(Rt.dev, q->ichr, q->qs, q->qe, q->n, len, pmode, seed, nperm, ev, rule, inter, sbp, nm, nd, g_ws);
        if (rc == IGD_HIP_OK) rc = igd_hip_dataset_bp(Rt.dev, ev, rule, fbp);
        route_engine_end(&Rt, "permutation null of the base-pair overlap", rc,
                         "permutation null of the base-pair overlap (H2D + permute, merge, hand-over and coverage kernels + D2H)");
    }
    if (!g_fail_rc && igdc_perm_bp_summary(inter, sbp, fbp, nperm, (int64_t)nC, obs, mu, sd, z, fold, nge, nle, pu, pl, jac, jm, js, NULL, NULL) == 0) {
        printf("index\tobserved_bp\tmean\tsd\tz\tfold\tn_ge\tn_le\tnlog10_p_upper\tnlog10_p_lower\tjaccard\tjaccard_mean\tFile\n");
        for (int32_t i = 0; i <= nfiles; i++) {
            if (i < nfiles) printf("%d\t%lld\t", (int)i, (long long)obs[i]);
            else printf("Any dataset: %lld of %lld bp in %lld merged regions (%lld dropped)\t", (long long)obs[i], (long long)sbp[0], (long long)nm[0],
                        (long long)nd[0]);
            print_na("%.6f", mu[i], "\t"); print_na("%.6f", sd[i], "\t"); print_na("%.6f", z[i], "\t"); print_na("%.6f", fold[i], "\t");
            printf("%lld\t%lld\t", (long long)nge[i], (long long)nle[i]);
            print_na("%.6f", pu[i], "\t"); print_na("%.6f", pl[i], "\t"); print_na("%.6f", jac[i], "\t");
            print_na("%.6f", jm[i], i < nfiles ? "\t" : "\n");
            if (i < nfiles) printf("%s\n", IGD->finfo[i].fileName);
        }
    }
    free(st); free(fl);
}

/* ------------------------------- `igd search` ----------------------------------------- */
static int usage_search(void)
{
    fprintf(stderr,
            "igd (MI355X build), search usage:\n"
            "  igd search <igd database file> [options]\n"
            "    -q <query file>            BED or BED.gz\n"
            "    -r <chrN start end>        a single region\n"
            "    -v <signal value 0-1000>   keep records with value >= v\n"
            "    -f                         print every overlap (with -q or -r)\n"
            "    -m                         dataset x dataset hit map, written to -o <name> (default Hitsmap)\n"
            "    -c                         accepted, no effect\n"
            "    -s                         Seqpare similarity of the query file with every dataset\n"
            "    -Q <list file>             one query file per line: the table of -q for each of them\n"
            "    -u                         with -q or -Q: count query regions with a hit, once per dataset (support)\n"
            "    -b                         with -q or -Q: base pairs of the query regions covered by each dataset\n"
            "    -w                         with -q or -Q: per query region, the datasets it overlaps (membership)\n"
            "    -U <universe file>         with -q or -Q: enrichment of each query set against the universe, per dataset the\n"
            "                               2x2 table of the supports, the sample odds ratio and -log10 p of a one-sided\n"
            "                               Fisher exact test (the sets as given; -X restricts them to the universe)\n"
            "    -X                         with -U: each set is first replaced by the universe regions it overlaps, so every\n"
            "                               table is a partition of the universe (number of regions of the set = their number)\n"
            "    -C                         with -q: dataset x dataset co-occurrence over the query regions, per pair of datasets\n"
            "                               the regions that overlap each, both, and the Jaccard index\n"
            "    -P <permutations>          with -q and -g: permutation null of the support counts -- the regions are moved along\n"
            "                               their contigs N times; per dataset observed, mean, sd, z and both one-sided p\n"
            "    -g <genome file>           with -P: the contig lengths, one name<TAB>length per line\n"
            "    -S <seed>  -M <mode>       with -P: the seed (default 0); circular (default: one rigid shift per contig) or\n"
            "                               shuffle (every region placed anew on its contig)\n"
            "    -M resample -U <universe>  with -P, without -g: every permuted set is as many regions as the query file holds, drawn\n"
            "                               without replacement from the universe file (contig, start and end as they stand);\n"
            "                               with -D or -G the null of the distances or of the base pairs, tables as under -P\n"
            "    -O <bp>  -A <F>  -B <F>    minimum overlap of a counted (query region, record) pair: at least <bp> base pairs,\n"
            "                               the fraction F of the query region (-A), of the record (-B); F is a decimal in [0, 1]\n"
            "                               with at most six places.  With -q or -Q alone, -u, -U [-R] and -P\n"
            "    -N <bp>                    with -q or -Q: per dataset, the query regions with a record within <bp> base pairs (0 to\n"
            "                               1073741824), those that overlap one, and the mean distance to the nearest record\n"
            "    -H <e1,e2,...>             with -N: instead, per dataset the regions with a record within <bp> and their number per\n"
            "                               bin of the SIGNED distance to the nearest record (negative: it lies upstream); 1 to 63\n"
            "                               ascending integer edges, bins <e1, [e1,e2), .., >=e_last\n"
            "    -L <bins> [-E]             with -N: instead, per dataset the regions with a record on BOTH sides within <bp> and their\n"
            "                               number per bin of the relative distance min(up, down) / (up + down) in [0, 0.5], as\n"
            "                               bedtools reldist (1 to 64 bins; 50: its bins of 0.01); distances between midpoints,\n"
            "                               with -E between edges\n"
            "    -V <op>                    with -q or -Q: per dataset, the query regions with an overlapping record, the overlapping\n"
            "                               (region, record) pairs and the mean over those regions of the records' count, sum, min\n"
            "                               or max of the value column; mean: the mean value over the pairs\n"
            "    -D <bp>                    with -P: the null of the distances instead -- per dataset the regions with a record within\n"
            "                               <bp> base pairs (0 to 1073741824) and their mean distance to the nearest one, each\n"
            "                               placed among the permuted sets' (mean, sd, z, one-sided p)\n"
            "    -G                         with -P: the null of the base-pair overlap instead -- per dataset the base pairs the merged\n"
            "                               regions share with it (as -J) placed among the permuted sets' (mean, sd, z, fold, both\n"
            "                               one-sided p) and the Jaccard with the mean permuted one\n"
            "    -W <workspace file>        with -P: the regions are placed inside the segments of this BED file (centromeres, gaps and\n"
            "                               blacklisted stretches left out), every fitting start equally likely; instead of -M\n"
            "    -Z <W>,<STEP>              local z-score, with -q and -g: the support of every dataset with the whole file moved by\n"
            "                               -k STEP .. k STEP base pairs (k = W / STEP, at most 4096 shifts; a region is pushed back\n"
            "                               against its contig's ends); with -P each count as a z-score in the null of -P\n"
            "    -R                         with -U: six more columns, the dataset's rank within the set by support, p and odds\n"
            "                               ratio, their maximum and mean, and -log10 of the Benjamini-Hochberg q-value\n"
            "  environment: IGD_DEVICE=<n> selects the GPU (default 0); IGD_DEVICES=0,1,.. searches a query file on\n"
            "               several GPUs (database replicated, contiguous query slabs, per-dataset counts summed)\n");
    return EX_OK;
}

/* `-P <permutations>`: 1 when the argument is a whole number in 1 .. IGD_HIP_PERM_MAX */
static int parse_perm_count(const char *arg, long long *np)
{
    char *end = NULL;
    *np = strtoll(arg, &end, 10);
    return end != arg && !*end && *np >= 1 && *np <= (long long)IGD_HIP_PERM_MAX;
}

/* `-N <bp>`, `-D <bp>`: 1 with the window in *w when the argument is a whole number in 0 .. 2^30 */
static int parse_window(const char *arg, int32_t *w)
{
    char *end = NULL;
    const long long ww = strtoll(arg, &end, 10);
    if (end == arg || *end || ww < 0 || ww > (long long)IGD_HIP_NEAREST_MAX_WINDOW) return 0;
    *w = (int32_t)ww;
    return 1;
}

/* `-M <mode>`: circular (also without -M) or shuffle; -1: neither */
static int parse_perm_mode(const char *arg)
{
    if (!arg || strcmp(arg, "circular") == 0) return IGD_HIP_PERM_CIRCULAR;
    return strcmp(arg, "shuffle") == 0 ? IGD_HIP_PERM_SHUFFLE : -1;
}

/* `-O <bp>`, `-A <F>`, `-B <F>` (a minimum overlap per pair, see g_mo) into g_mo_val; 0 after the refusal of a missing or malformed value */
static int parse_min_overlap(const char *a, const char *arg)
{
    char *end = NULL;
    const long long bpv = a[1] == 'O' && arg ? strtoll(arg, &end, 10) : -1;
    const int32_t ppm = a[1] != 'O' && arg ? parse_ppm(arg) : -1;
    if (a[1] == 'O' ? (!end || end == arg || *end || bpv < 0 || bpv > INT32_MAX) : ppm < 0) {
        printf("Not supported: %s %s (%s)\n", a, arg ? arg : "",
               a[1] == 'O' ? "a number of base pairs, 0 to 2147483647" : "a decimal fraction in [0, 1] with at most six places");
        return 0;
    }
    if (a[1] == 'O') g_mo_val.min_bp = (int32_t)bpv;
    else if (a[1] == 'A') g_mo_val.ppm_query = ppm;
    else g_mo_val.ppm_record = ppm;
    return 1;
}

/* How an answer of the command line leaves: the older refusals on stdout with exit code 0, the newer ones as usage errors, those
 * of -Z and -M resample on stderr with nothing on stdout.  In RULES the same column also holds what is no refusal: the groups file
 * of -K is read at that place, or a command is taken. */
enum { OLD = 1, NEW, ERR, GROUPS, CMD_PERMUTE, CMD_JACCARD, CMD_MAP, CMD_NEAREST, CMD_COOCCUR, CMD_ENRICH, CMD_FULL, CMD_MEMBERS, CMD_SUPPORT,
       CMD_COUNT, CMD_REGION, CMD_HITMAP, CMD_SEQPARE, CMD_SETS, CMD_USAGE };
#define NS "Not supported: "

static int say(int how, const char *text, const char *arg, const char *tail)
{
    fprintf(how == ERR ? stderr : stdout, "%s%s%s\n", text, arg ? arg : "", tail ? tail : "");
    return how == OLD ? EX_OK : EX_USAGE;
}

/* One row per option.  words: the words of its value.  STEP: the parse steps over the value; without it the value is looked at
 * again as an option.  BARE: the option counts without its value too.  EAGER: parsed and refused where it stands
 * (parse_min_overlap).  AFTER_R: does not set the mode after -r.  mode: the mode it sets.  miss, how: the answer to a missing
 * value, given where it is met; none: the option is ignored then.  Words that are no row (-c among them) are ignored. */
enum { STEP = 1, BARE = 2, EAGER = 4, AFTER_R = 8 };
#define OPT(x, ...) {.name = "-" #x, .id = O_##x, .words = __VA_ARGS__}
static const struct { const char *name; int id, words, flags, mode; const char *miss; int how; } OPTS[] = {
    OPT(f, 0), OPT(u, 0), OPT(b, 0), OPT(w, 0), OPT(X, 0), OPT(C, 0), OPT(G, 0), OPT(E, 0), OPT(R, 0), OPT(J, 0),
    OPT(m, 0, 0, F_m),
    OPT(s, 0, AFTER_R, F_s),
    OPT(q, 1, 0, F_q, "No query file.", OLD),
    OPT(r, 3, BARE, F_r),
    OPT(v, 1),
    OPT(Q, 1),
    OPT(o, 1),
    OPT(U, 1, 0, 0, "No universe file.", OLD),
    OPT(P, 1, 0, 0, "No number of permutations.", OLD),
    OPT(g, 1, 0, 0, "No genome file.", OLD),
    OPT(S, 1, 0, 0, "No seed.", OLD),
    OPT(M, 1, 0, 0, "No mode.", OLD),
    OPT(W, 1, 0, 0, NS "-W without a workspace file", NEW),
    OPT(N, 1, STEP, 0, "No window.", OLD),                  /* (the window is not an option: "-N -5" is a refused window) */
    OPT(H, 1, STEP, 0, NS "-H without a list of edges", NEW),
    OPT(L, 1, STEP | BARE),
    OPT(V, 1, STEP, 0, NS "-V without an op (count, sum, min, max or mean)", NEW),
    OPT(D, 1, STEP, 0, NS "-D without a window", NEW),
    OPT(I, 1, STEP, 0, NS "-I without an op (count, sum, min, max or mean)", NEW),
    OPT(K, 1, STEP, 0, NS "-K without a groups file", NEW),
    OPT(Z, 1, STEP, 0, NS "-Z without W,STEP", ERR),
    OPT(O, 1, STEP | EAGER), OPT(A, 1, STEP | EAGER), OPT(B, 1, STEP | EAGER),
};

/* argv into *o.  -1, or the exit code after the answer to a missing or (-O, -A, -B) refused value */
static int search_parse(cli_opts *o, int argc, char **argv)                  /* :931-971 */
{
    for (int i = 3; i < argc; i++) {
        size_t k = 0;
        while (k < sizeof OPTS / sizeof *OPTS && strcmp(argv[i], OPTS[k].name) != 0) k++;
        if (k == sizeof OPTS / sizeof *OPTS) continue;
        const int id = OPTS[k].id, flags = OPTS[k].flags, have = i + OPTS[k].words < argc;
        if (flags & EAGER) { if (!parse_min_overlap(argv[i], have ? argv[i + 1] : NULL)) return EX_USAGE; }
        else if (!have && OPTS[k].miss) return say(OPTS[k].how, OPTS[k].miss, NULL, NULL);
        else if (!have && !(flags & BARE)) continue;
        o->given |= 1ULL << id;
        if (!have) continue;
        if (OPTS[k].words) o->val[id] = argv[i + 1];
        if (id == O_r) { o->qs = atoi(argv[i + 2]); o->qe = atoi(argv[i + 3]); }
        if (OPTS[k].mode && !((flags & AFTER_R) && o->mode == F_r)) o->mode = OPTS[k].mode;
        if (flags & STEP) i += OPTS[k].words;
    }
    if (o->mode) o->given |= 1ULL << o->mode;
    if (o->mode == F_q || (!o->mode && (o->given & B(Q)))) o->given |= F(PERSET);
    if (o->given & (B(O) | B(A) | B(B))) o->given |= F(MINOV);
    const char *a;
    o->v = o->val[O_v] ? atoi(o->val[O_v]) : 0;
    o->seed = o->val[O_S] ? (uint64_t)strtoull(o->val[O_S], NULL, 10) : 0;
    if ((a = o->val[O_P]) && !parse_perm_count(a, &o->np)) { o->np = 0; o->given |= F(BAD_P); }
    o->pmode = o->val[O_W] ? IGD_HIP_PERM_WORKSPACE : parse_perm_mode(o->val[O_M]);
    if (parse_perm_mode(o->val[O_M]) < 0) o->given |= F(BAD_M);
    if (o->val[O_P] && o->val[O_M] && strcmp(o->val[O_M], "resample") == 0) { o->given |= F(RESAMPLE); o->pmode = IGD_HIP_PERM_RESAMPLE; }
    o->distW = -1;
    if ((a = o->val[O_D]) && !parse_window(a, &o->distW)) o->given |= F(BAD_D);
    if ((a = o->val[O_N]) && !parse_window(a, &o->nearW)) o->given |= F(BAD_N);
    if ((a = o->val[O_L])) {
        char *end = NULL;
        const long long nb = strtoll(a, &end, 10);
        if (a[0] < '0' || a[0] > '9' || *end || !igd_hip_flank_bins_valid(nb)) o->given |= F(BAD_L);
        else o->flankBins = (int32_t)nb;
    } else if (o->given & B(L)) o->given |= F(L_BARE);
    if ((a = o->val[O_H]) && (o->histNe = parse_edges(a, o->histEdges)) < 1) o->given |= F(BAD_H);
    o->mapOp = -1;
    for (int k = 0; (a = o->val[O_V]) && k < 5; k++) if (strcmp(a, MAP_OPS[k]) == 0) o->mapOp = k;
    if (a && o->mapOp < 0) o->given |= F(BAD_V);
    if (a && o->mapOp > 0 && IGD->gType == 0) o->given |= F(V_BLIND);
    o->inOp = -1;
    for (int k = 0; (a = o->val[O_I]) && k < 5; k++) if (strcmp(a, MAP_OPS[k]) == 0) o->inOp = k;
    if (a && o->inOp < 0) o->given |= F(BAD_I);
    if (a && o->inOp > 0 && IGD->gType == 0) o->given |= F(I_BLIND);
    if ((a = o->val[O_Z]) && (o->nShift = parse_shifts(a, &o->shiftOff)) < 1) o->given |= F(BAD_Z);
    return -1;
}

/* What `igd search` answers, as ONE ordered list: the first row that applies is the answer.  A row applies when every option and
 * fact of `all` is given, one of `any` (where there is an `any`) and none of `none`; so "-X together with .." rows keep their
 * partners in `any`, "-X without .." rows in `none`.  The answer is a refusal -- the sentence as it is printed, with the value
 * of option `arg` and `tail` behind it where the sentence quotes one -- or a command.  The order is the behaviour: where two
 * refusals apply the earlier one answers (-J -P 5: -J's sentence, not -P's), and a command that stands ahead of a refusal wins
 * over it (-q F -f -w -u prints every overlap).  The letters of a sentence stand in an order of their own; the mask beside it is what decides. */
#define OTHER (B(m) | B(s) | B(r))
#define QSET (F(q) | B(Q))                /* -q or -Q names the query sets */
#define RULE(a, y, n, ...) {.all = (a), .any = (y), .none = (n), .how = __VA_ARGS__}
static const struct { uint64_t all, any, none; int how; const char *text; int arg; const char *tail; } RULES[] = {
    /* -I: the null of the values.  A block of its own ahead of every older row, so that no older sentence and no older mask
     * changes; behind it a command line with -I falls through to the rows of -M resample, -W and -P as they stand */
    RULE(B(I), 0, B(P), NEW, NS "-I without -P"),
    RULE(B(I), B(D) | B(G) | B(V) | B(N) | B(H) | B(L) | B(E) | B(J) | B(Z) | B(K) | B(Q) | B(u) | B(b) | B(w) | B(R) | B(X) | B(C) | B(f) | OTHER | F(MINOV),
         0, NEW, NS "-I together with -D, -G, -V, -N, -H, -L, -E, -J, -Z, -K, -Q, -u, -b, -w, -R, -X, -C, -f, -m, -s, -r, -O, -A or -B"),
    RULE(B(I) | B(U), 0, F(RESAMPLE), NEW, NS "-I with -U but without -M resample"),
    RULE(B(I), F(BAD_I), 0, NEW, NS "-I ", O_I, " (count, sum, min, max or mean)"),
    RULE(B(I), F(I_BLIND), 0, NEW, NS "-I ", O_I, " on a database without values (gType 0); -I count works there"),
    /* -Z: the shift profile */
    RULE(B(Z), B(Q), 0, ERR, NS "-Z together with -Q"),
    RULE(B(Z), B(u) | B(U) | B(b) | B(J) | B(w) | B(C) | B(N) | B(V) | B(K) | OTHER | B(f) | B(R) | B(X) | B(H) | B(L) | B(E), 0, ERR,
     NS "-Z together with -u, -U, -b, -J, -w, -C, -N, -V, -K, -m, -s, -r, -f, -R, -X, -H, -L or -E"),
    RULE(B(Z), B(D) | B(G), 0, ERR, NS "-Z together with -D or -G (the shift profile is the support's)"),
    RULE(B(Z), 0, B(g), ERR, NS "-Z without -g"),
    RULE(B(Z), 0, F(q), ERR, NS "-Z without -q"),
    RULE(B(Z), B(S) | B(M) | B(W), B(P), ERR, NS "-Z with -S, -M or -W but without -P"),
    RULE(B(Z) | B(W) | B(M), 0, 0, ERR, NS "-W together with -M (the workspace is the placement)"),
    RULE(B(Z), F(BAD_P), 0, ERR, NS "-Z with a number of permutations outside 1 to 1048576"),
    RULE(B(Z) | B(P), F(BAD_M), 0, ERR, NS "-Z with a -M that is neither circular nor shuffle"),
    RULE(B(Z), F(BAD_Z), 0, ERR, NS "-Z W,STEP needs 0 <= W <= 1073741824, STEP >= 1 and at most 4096 shifts, not ", O_Z),
    RULE(B(Z), 0, 0, CMD_PERMUTE),
    /* -P -M resample: the one -P that takes -U, so it stands ahead of -G and -D, which refuse -U */
    RULE(F(RESAMPLE), 0, B(U), ERR, NS "-M resample without -U"),
    RULE(F(RESAMPLE), B(g) | B(W), 0, ERR, NS "-M resample together with -g or -W (the universe is the placement)"),
    RULE(F(RESAMPLE), B(Q) | B(R) | B(X) | B(K) | B(Z), 0, ERR, NS "-M resample together with -Q, -R, -X, -K or -Z"),
    RULE(F(RESAMPLE), B(u) | B(b) | B(w) | B(C) | B(f) | OTHER | B(J) | B(V) | B(N) | B(H) | B(L) | B(E), 0, ERR,
     NS "-M resample together with -u, -b, -w, -C, -f, -m, -s, -r, -J, -V, -N, -H, -L or -E"),
    RULE(F(RESAMPLE) | B(D) | B(G), 0, 0, ERR, NS "-M resample together with both -D and -G"),
    RULE(F(RESAMPLE) | F(MINOV), B(D) | B(G), 0, ERR, NS "-M resample -D or -G together with -O, -A or -B"),
    RULE(F(RESAMPLE), 0, F(q), ERR, NS "-M resample without -q"),
    RULE(F(RESAMPLE), F(BAD_P), 0, ERR, NS "-M resample with a number of permutations outside 1 to 1048576"),
    RULE(F(RESAMPLE), F(BAD_D), 0, ERR, NS "-D ", O_D, " (a window of 0 to 1073741824 base pairs)"),
    RULE(F(RESAMPLE), 0, 0, CMD_PERMUTE),
    /* -K: groups of datasets; the file is read, and refused for what it holds, once the options stand */
    RULE(B(K), B(b) | B(w) | B(X) | B(C) | B(P) | B(D) | B(G) | B(W) | B(J) | B(V) | B(N) | B(H) | B(L) | B(E) | B(f) | OTHER, 0, NEW,
     NS "-K together with -b, -w, -X, -C, -P, -D, -G, -W, -J, -V, -N, -H, -L, -E, -f, -m, -s or -r"),
    RULE(B(K), 0, B(u) | B(U), NEW, NS "-K without -u or -U"),
    RULE(B(K), 0, QSET, NEW, NS "-K without -q or -Q"),
    RULE(B(K), 0, 0, GROUPS),
    /* -W: a workspace */
    RULE(B(W), 0, B(P), NEW, NS "-W without -P"),
    RULE(B(W) | B(M), 0, 0, NEW, NS "-W together with -M (the workspace is the placement)"),
    /* -G: the null of the base pairs */
    RULE(B(G), 0, B(P), NEW, NS "-G without -P"),
    RULE(B(G), B(D) | B(J) | F(MINOV) | B(N) | B(H) | B(L) | B(E) | B(V) | B(Q) | B(u) | B(b) | B(w) | B(U) | B(R) | B(X) | B(C) | B(f) | OTHER, 0, NEW,
     NS "-G together with -D, -J, -O, -A, -B, -N, -H, -L, -E, -V, -Q, -u, -b, -w, -U, -R, -X, -C, -f, -m, -s or -r"),
    RULE(B(G), 0, B(g), NEW, NS "-G -P without -g"),
    RULE(B(G), 0, F(q), NEW, NS "-G -P without -q"),
    RULE(B(G), F(BAD_P), 0, NEW, NS "-G with a number of permutations outside 1 to 1048576"),
    RULE(B(G), F(BAD_M), 0, NEW, NS "-G with a -M that is neither circular nor shuffle"),
    /* -J: base-pair Jaccard */
    RULE(B(J), B(u) | B(b) | B(w) | B(U) | B(R) | B(X) | B(C) | B(P) | B(D) | B(N) | B(H) | B(L) | B(E) | B(V) | B(f) | OTHER | F(MINOV), 0, NEW,
     NS "-J together with -u, -b, -w, -U, -R, -X, -C, -P, -D, -N, -H, -L, -E, -V, -f, -m, -s, -r, -O, -A or -B"),
    RULE(B(J), 0, QSET, NEW, NS "-J without -q or -Q"),
    /* -V: values of the overlapping records */
    RULE(B(V), B(u) | B(b) | B(w) | B(U) | B(R) | B(X) | B(C) | B(P) | B(D) | B(N) | B(f) | OTHER | F(MINOV), 0, NEW,
     NS "-V together with -u, -b, -w, -U, -R, -X, -C, -P, -D, -N, -f, -m, -s, -r, -O, -A or -B"),
    RULE(B(V), 0, QSET, NEW, NS "-V without -q or -Q"),
    RULE(B(V), F(BAD_V), 0, NEW, NS "-V ", O_V, " (count, sum, min, max or mean)"),
    RULE(B(V), F(V_BLIND), 0, NEW, NS "-V ", O_V, " on a database without values (gType 0); -V count works there"),
    /* -L, -E: relative distances */
    RULE(B(E), 0, B(L), NEW, NS "-E without -L"),
    RULE(B(L), 0, B(N), NEW, NS "-L without -N"),
    RULE(B(L), B(H) | B(P) | B(D) | F(MINOV), 0, NEW, NS "-L together with -H, -P, -D, -O, -A or -B"),
    RULE(B(L), F(L_BARE), 0, NEW, NS "-L without a number of bins"),
    RULE(B(L), F(BAD_L), 0, NEW, NS "-L ", O_L, " (1 to 64 bins)"),
    /* -H: signed distances */
    RULE(B(H), 0, B(N), NEW, NS "-H without -N"),
    RULE(B(H), B(P) | B(D), 0, NEW, NS "-H together with -P or -D"),
    RULE(B(H), F(BAD_H), 0, NEW, NS "-H ", O_H, " (1 to 63 ascending integer edges, each within int32, separated by commas)"),
    /* -D: the null of the distances */
    RULE(B(D), 0, B(P), NEW, NS "-D without -P"),
    RULE(B(D), B(N) | F(MINOV) | B(Q) | B(u) | B(b) | B(w) | B(U) | B(R) | B(X) | B(C) | B(f) | OTHER, 0, NEW,
     NS "-D together with -N, -O, -A, -B, -Q, -u, -b, -w, -U, -R, -X, -C, -f, -m, -s or -r"),
    RULE(B(D), 0, B(g), NEW, NS "-D -P without -g"),
    RULE(B(D), 0, F(q), NEW, NS "-D -P without -q"),
    RULE(B(D), F(BAD_P), 0, NEW, NS "-D with a number of permutations outside 1 to 1048576"),
    RULE(B(D), F(BAD_M), 0, NEW, NS "-D with a -M that is neither circular nor shuffle"),
    RULE(B(D), F(BAD_D), 0, NEW, NS "-D ", O_D, " (a window of 0 to 1073741824 base pairs)"),
    /* -N: nearest records (the older wording, and exit code 0) */
    RULE(B(N), B(u) | B(b) | B(w) | B(U) | B(R) | B(X) | B(C) | B(P) | B(f) | OTHER | F(MINOV), 0, OLD,
     NS "-N together with -u, -b, -w, -U, -R, -X, -C, -P, -f, -m, -s, -r, -O, -A or -B"),
    RULE(B(N), 0, QSET, OLD, NS "-N without -q or -Q"),
    RULE(B(N), F(BAD_N), 0, OLD, NS "-N ", O_N, " (a window of 0 to 1073741824 base pairs)"),
    /* -O, -A, -B: a minimum overlap */
    RULE(F(MINOV), B(b) | B(w) | B(X) | B(C) | B(f) | OTHER, 0, NEW, NS "-O, -A or -B together with -b, -w, -X, -C, -f, -m, -s or -r, or without -q or -Q"),
    RULE(F(MINOV), 0, QSET, NEW, NS "-O, -A or -B together with -b, -w, -X, -C, -f, -m, -s or -r, or without -q or -Q"),
    /* the commands, and the older refusals between them */
    RULE(0, B(g) | B(S) | B(M), B(P), OLD, NS "-g, -S or -M without -P"),
    RULE(B(J), 0, 0, CMD_JACCARD),
    RULE(B(V), 0, 0, CMD_MAP),
    RULE(B(N), 0, 0, CMD_NEAREST),
    RULE(B(P), B(Q) | B(u) | B(b) | B(w) | B(U) | B(R) | B(X) | B(C) | B(f) | OTHER, 0, OLD, NS "-P together with -Q, -u, -b, -w, -U, -R, -X, -C, -f, -m, -s or -r"),
    RULE(B(P), 0, B(g), OLD, NS "-P without -g"),
    RULE(B(P), 0, F(q), OLD, NS "-P without -q"),
    RULE(B(P), F(BAD_P), 0, OLD, NS "-P ", O_P, " (1 to 1048576 permutations)"),
    RULE(B(P), F(BAD_M), 0, OLD, NS "-M ", O_M, " (circular or shuffle)"),
    RULE(B(P), 0, 0, CMD_PERMUTE),
    RULE(B(C), B(Q) | B(u) | B(b) | B(w) | B(U) | B(R) | B(X) | B(f) | OTHER, 0, OLD, NS "-C together with -Q, -u, -b, -w, -U, -R, -X, -f, -m, -s or -r"),
    RULE(B(C), 0, F(q), OLD, NS "-C without -q"),
    RULE(B(C), 0, 0, CMD_COOCCUR),
    RULE(B(R), 0, B(U), OLD, NS "-R without -U"),
    RULE(B(X), 0, B(U), OLD, NS "-X without -U"),
    RULE(B(U), B(b) | B(w) | B(f) | OTHER, 0, OLD, NS "-U together with -b, -w, -f, -m, -s or -r"),
    RULE(B(U), QSET, 0, CMD_ENRICH),
    RULE(B(f), 0, F(q) | F(r), OLD, "Not supported -f option"),
    RULE(B(f), 0, 0, CMD_FULL),
    RULE(F(PERSET) | B(w), B(u) | B(b), 0, OLD, NS "-w together with -u or -b"),
    RULE(F(PERSET) | B(w), 0, 0, CMD_MEMBERS),
    RULE(F(PERSET) | B(u) | B(b), 0, 0, OLD, NS "-b together with -u"),
    RULE(F(PERSET), B(u) | B(b), 0, CMD_SUPPORT),
    RULE(F(q), 0, 0, CMD_COUNT),
    RULE(F(r), 0, 0, CMD_REGION),
    RULE(F(m), 0, 0, CMD_HITMAP),
    RULE(F(s), 0, 0, CMD_SEQPARE),
    RULE(B(Q), 0, 0, CMD_SETS),                       /* only where the reference's own parse leaves nothing to do */
    RULE(0, 0, 0, CMD_USAGE),
};
_Static_assert(IGD_HIP_PERM_MAX == 1048576 && IGD_HIP_NEAREST_MAX_WINDOW == 1073741824 && IGD_HIP_SHIFT_MAX_OFFSET == 1073741824 &&
               IGD_HIP_SHIFT_MAX == 4096 && IGD_HIP_FLANK_MAX_BINS == 64 && IGD_HIP_NEAREST_MAX_EDGES == 63, "RULES spells these limits out");

/* The first row of RULES that applies: the exit code after its refusal, or -1 with the command in o->cmd */
static int search_check(cli_opts *o)
{
    for (size_t k = 0;; k++) {
        if ((o->given & RULES[k].all) != RULES[k].all || (RULES[k].any && !(o->given & RULES[k].any)) || (o->given & RULES[k].none)) continue;
        const int how = RULES[k].how;
        if (how == GROUPS) {
            const int rc = groups_read(o->val[O_K]);
            if (rc) return rc;
        } else if (how >= CMD_PERMUTE) {
            o->cmd = how;
            return -1;
        } else return say(how, RULES[k].text, RULES[k].arg ? o->val[RULES[k].arg] : NULL, RULES[k].tail);
    }
}

/* `-m`: the dataset x dataset hit map into the file `name` (-o; default Hitsmap) */
static void hitmap_file(int32_t v, const char *name)                         /* :996-1022 */
{
    const int32_t nfiles = IGD->nFiles;
    char out[64] = "";
    if (name) strncpy(out, name, sizeof out - 1);
    if (IGD->gType != 1) {
        printf("igd: -m needs a database created with 16-byte records (gType 1)\n");
        return;
    }
    uint32_t **hitmap = (uint32_t **)malloc(sizeof(uint32_t *) * (size_t)(nfiles + 1));
    for (int32_t i = 0; i < nfiles; i++) hitmap[i] = (uint32_t *)calloc((size_t)nfiles + 1, sizeof(uint32_t));
    if (v > 0) getMap_v(hitmap, v); else getMap(hitmap);
    if (strlen(out) < 2) strcpy(out, "Hitsmap");
    FILE *fo = g_fail_rc ? NULL : fopen(out, "w");
    if (g_fail_rc) ;                                /* no matrix of zeros after an engine failure */
    else if (!fo) printf("Can't open file %s\n", out);
    else {
        static char obuf[1 << 20];
        setvbuf(fo, obuf, _IOFBF, sizeof obuf);
        fprintf(fo, "%u\t%u\t%u\n", (unsigned)nfiles, (unsigned)nfiles, (unsigned)v);
        for (int32_t i = 0; i < nfiles; i++) {
            for (int32_t j = 0; j < nfiles; j++) fprintf(fo, "%u\t", hitmap[i][j]);
            fprintf(fo, "\n");
        }
        fclose(fo);
    }
    for (int32_t i = 0; i < nfiles; i++) free(hitmap[i]);
    free(hitmap);
}

/* The command that search_check chose */
static void search_run(const cli_opts *o, int64_t *hits)
{
    const int32_t nfiles = IGD->nFiles, v = o->v;
    char *qfName = o->val[O_q] ? o->val[O_q] : (char *)"", *chrm = o->val[O_r];
    /* the query files of the per-set commands: -q's when it is the mode, else the -Q list's; opened by the command that reads them */
    char *const oneFile = o->mode == F_q ? qfName : NULL, *const listName = o->val[O_Q];
    cli_paths P;
    memset(&P, 0, sizeof P);
    int64_t total;
    switch (o->cmd) {
    case CMD_PERMUTE: permute_file(o); break;
    case CMD_JACCARD: if (paths_open(&P, oneFile, listName)) jaccard_files(&P, v); break;
    case CMD_MAP: if (paths_open(&P, oneFile, listName)) map_files(&P, v, o->mapOp); break;
    case CMD_NEAREST:
        if (!paths_open(&P, oneFile, listName)) break;
        if (o->given & B(L)) flank_reldist_files(&P, v, o->nearW, o->given & B(E) ? IGD_HIP_FLANK_EDGES : IGD_HIP_FLANK_MIDPOINTS, o->flankBins);
        else if (o->given & B(H)) nearest_hist_files(&P, v, o->nearW, o->histEdges, o->histNe);
        else nearest_files(&P, v, o->nearW);
        break;
    case CMD_COOCCUR: cooccur_file(qfName, v); break;
    case CMD_ENRICH: if (paths_open(&P, oneFile, listName)) enrich_files(&P, o->val[O_U], v, (o->given & B(R)) != 0, (o->given & B(X)) != 0); break;
    case CMD_FULL:                                                            /* :975-995 */
        if (o->mode == F_q) total = IGD->gType == 0 ? getOverlaps_f0(qfName) : getOverlaps_f1(qfName);
        else total = IGD->gType == 0 ? get_overlaps_f0(chrm, o->qs, o->qe) : get_overlaps_f1(chrm, o->qs, o->qe);
        if (!g_fail_rc) printf("Total overlaps: %lld\n", (long long)total);
        break;
    case CMD_MEMBERS: if (paths_open(&P, oneFile, listName)) membership_files(&P, v); break;
    case CMD_SUPPORT: if (paths_open(&P, oneFile, listName)) support_files(&P, v, (o->given & B(b)) != 0); break;
    case CMD_COUNT:                                                           /* :1023-1040 */
        count_file(qfName, v, hits);
        if (!g_fail_rc) print_hits_table(hits);
        break;
    case CMD_REGION:                                                          /* :1041-1053 */
        if (IGD->gType == 0) get_overlaps0(chrm, o->qs, o->qe, hits);
        else if (v > 0) get_overlaps_v(chrm, o->qs, o->qe, v, hits);
        else get_overlaps(chrm, o->qs, o->qe, hits);
        if (!g_fail_rc) printf("index\t number of regions\t number of hits\t File_name\n");
        for (int32_t i = 0; i < nfiles && !g_fail_rc; i++)
            printf("%i\t%i\t%lld\t%s\n", i, IGD->finfo[i].nr, (long long)hits[i], IGD->finfo[i].fileName);
        break;
    case CMD_HITMAP: hitmap_file(v, o->val[O_o]); break;
    case CMD_SEQPARE:                                                         /* :1054-1061 */
        if (IGD->gType != 1) printf("igd: -s needs a database created with 16-byte records (gType 1)\n");
        else {
            double *sm = (double *)malloc(sizeof(double) * (size_t)(nfiles + 1));
            seqOverlaps(qfName, sm);
            if (!g_fail_rc) printf("index\t number of regions\t similarity\t dataset name\n");
            for (int32_t i = 0; i < nfiles && !g_fail_rc; i++)
                printf("%i\t%i\t%10.6f\t%s\n", i, IGD->finfo[i].nr, sm[i], IGD->finfo[i].fileName);
            free(sm);
        }
        break;
    case CMD_SETS: if (paths_open(&P, oneFile, listName)) search_sets(&P, v, hits); break;
    default: usage_search();
    }
    paths_close(&P);
}

int igd_search(int argc, char **argv)                                        /* :889-1079 */
{
    if (argc < 4) return usage_search();
    char *igdName = argv[2];
    size_t L = strlen(igdName);
    if (L < 4 || strcmp(igdName + L - 4, ".igd") != 0) {                      /* :894-898 */
        printf("%s is not an igd database", igdName);
        return EX_OK;
    }
    FILE *probe = fopen(igdName, "rb");
    if (!probe) {                                                             /* :899-903 */
        printf("%s does not exist", igdName);
        return EX_OK;
    }
    fclose(probe);

    double t0 = now_s();
    IGD = get_igdinfo(igdName);
    if (!IGD) return EX_OK;
    phase("header", &t0);
    /* from here on every way out is the release below: refusal, usage, success and engine failure alike */
    int rc = EX_OK;
    int64_t *hits = NULL;
    cli_opts o;
    memset(&o, 0, sizeof o);
    char *tsv = igdc_index_path(igdName);
    {   /* fname = path without extension; the reference strcpy's into 64 bytes (:916-922) */
        size_t stem = strlen(tsv) - strlen("_index.tsv");
        if (stem > sizeof IGD->fname - 1) stem = sizeof IGD->fname - 1;
        memcpy(IGD->fname, igdName, stem);
        IGD->fname[stem] = '\0';
    }
    IGD->finfo = get_fileinfo(tsv, &IGD->nFiles);
    free(tsv);
    if (IGD->finfo) {
        hits = (int64_t *)calloc((size_t)IGD->nFiles + 1, sizeof(int64_t));
        g_mo_val.min_bp = g_mo_val.ppm_query = g_mo_val.ppm_record = 0;
        groups_free();
        if ((rc = search_parse(&o, argc, argv)) < 0) rc = search_check(&o);
        if (rc < 0) {
            if ((o.given & F(MINOV)) && igd_hip_min_overlap_active(&g_mo_val)) g_mo = &g_mo_val;  /* (all three zero: no threshold) */
            fP = fopen(igdName, "rb");                                        /* :974 */
            search_run(&o, hits);
            /* the reference's exit code is always 0; an engine failure (message already on stderr) is the one
             * thing this tool reports through it, instead of printing a table of zeros */
            rc = g_fail_rc ? EX_UNAVAILABLE : g_usage_rc ? EX_USAGE : EX_OK;
        }
    }

    /* release everything, in the shape get_igdinfo/get_fileinfo handed it out (:1066-1078), and leave the process as a first
     * call finds it */
    groups_free();
    free(o.shiftOff);
    free(hits);
    if (fP) { fclose(fP); fP = NULL; }
    free(IGD->nTile);
    for (int32_t c = 0; c < IGD->nCtg; c++) {
        free(IGD->nCnt[c]); free(IGD->tIdx[c]); free(IGD->cName[c]);
    }
    for (int32_t i = 0; IGD->finfo && i < IGD->nFiles; i++) free(IGD->finfo[i].fileName);
    free(IGD->nCnt); free(IGD->tIdx); free(IGD->cName); free(IGD->finfo);
    free(IGD);
    IGD = NULL;
    if (g_core) { igdc_close(g_core); g_core = NULL; g_core_of = NULL; hc = NULL; }
    free(g_core_path); g_core_path = NULL;
    g_mo = NULL; g_ws = NULL; g_pool = NULL;
    g_usage_rc = 0;
    return rc;
}

/* ---- create_igd*, src/igd_create.h:10-14 --------------------------------------------------- */
static void create_with(char *iPath, char *oPath, char *igdName, int mode)
{
    igdc_create_opts o;
    o.ipath = iPath; o.opath = oPath; o.name = igdName;
    o.nbp = tile_size > 0 ? tile_size : 16384;            /* igd_init, src/igd_base.c:522 */
    o.mode = mode; o.msg = IGDC_MSG_CLI;
    o.linebuf = mode == IGDC_CREATE_GTYPE0 ? 256 : 1024;
    const char *dv = getenv("IGD_DEVICE");
    o.device = dv ? atoi(dv) : 0;
    const int rc = igdc_create(&o);
    if (rc < 0) {
        fprintf(stderr, "igd create: no usable GPU (%d): %s\n", rc, igd_hip_last_error());
        if (!g_fail_rc) g_fail_rc = rc;
    }
}
void create_igd(char *iPath, char *oPath, char *igdName) { create_with(iPath, oPath, igdName, IGDC_CREATE_GLOB); }
void create_igd0(char *iPath, char *oPath, char *igdName) { create_with(iPath, oPath, igdName, IGDC_CREATE_GTYPE0); }
void create_igd_f(char *iPath, char *oPath, char *igdName) { create_with(iPath, oPath, igdName, IGDC_CREATE_LIST); }
void create_igd_bed4(char *iPath, char *oPath, char *igdName) { create_with(iPath, oPath, igdName, IGDC_CREATE_BED4); }
