// engine/host_permute.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_permute_support / igd_hip_permute_regions / igd_hip_perm_stats: the permutation null of region-set support
// ------------------------------------------------------------------------------------------
// What the nulls (here, host_permute_nearest.hpp, host_permute_map.hpp, host_permute_bp.hpp, host_shift.hpp) share is written
// once, here.  ONE value, PermSpec, says how the rows of a call are made -- free placement, workspace, draw from a pool, rigid
// shifts -- and is what every exported entry builds from its loose arguments and hands on: to the refusals (perm_args_refused),
// to the upload of the call's regions, contig lengths, table, offsets or pool (perm_place_upload, which answers with the device
// side of the same thing, PermPlace), and to the chunk driver (run_perm_chunks), which launches the generator (permute_launch)
// per chunk.  A statistic adds the bytes of device rows one permutation costs, the workspaces it grows, and what it counts from a
// chunk of rows.  The entries that return the generated regions themselves share perm_regions_home.
// The support: the set as given is counted first, one row through igd_sets_support, copied on the device into `observed`
// (db->d_pmStat holds observed and the six statistics, nFiles + 1 words each; word nFiles is the any-dataset column, the
// kernel's nhit total).  Then the permutations in the driver's chunks, pc * nFiles * 8 <= perm_row_bytes() (the rows of
// igd_hip_search_sets): the slice table -- one row per permutation, each row cut as igd_hip_support_sets cuts a set; built and
// uploaded once, a shorter last chunk uses a prefix of it -- drives ONE launch of igd_sets_support, and igd_perm_stats folds the
// chunk's rows and totals into the statistics.  7 x (nFiles + 1) words come back behind the last chunk, into a buffer of this
// file that is copied to the caller's behind the driver's wait: on an error nothing is written.

// The TEST-ONLY variable IGD_HIP_PERM_ROW_BYTES (read once per process, as IGD_HIP_RESTRICT_ROW_BYTES) lowers the row budget of
// a chunk so that small fixtures cross the seam between two chunks.
static int64_t perm_row_bytes(void)
{
    static const int64_t m = env_positive("IGD_HIP_PERM_ROW_BYTES", sets_row_bytes());
    return m;
}

// workgroups igd_permute_regions is launched with for n outputs: a lane takes a second one only when n exceeds the grid's lanes
extern "C" int32_t igd_hip_permute_grid(int64_t n) { return items_grid(n, IGD_SETS_WG); }

// The third placement kind, internal to the engine: the set moved rigidly by offsets[p] (igd_hip_shift_place; host_shift.hpp drives
// it through run_perm_chunks with its offset table).  No public mode: igd_hip_perm_mode_ok refuses it for the nulls.
#define IGD_PERM_PLACE_SHIFT 3

// The pool of a resampling call (THE DRAW of include/igd_hip.h): host arrays of npool regions.  No pool: every other mode.
struct PermPool {
    const int32_t *ichr, *qs, *qe;
    int64_t npool;
};

// HOW THE ROWS OF ONE CALL ARE MADE, as the caller gave it (host pointers): nperm permutations, draws or shifts.  Exactly one of
// ws (mode IGD_HIP_PERM_WORKSPACE), offsets (mode IGD_PERM_PLACE_SHIFT: nperm of them, the seed is not read) and pool (mode
// IGD_HIP_PERM_RESAMPLE: no ctg_len) is set, or none (the two free placements).
struct PermSpec {
    const int32_t *ctg_len;
    int mode; uint64_t seed; int64_t nperm;
    const igd_hip_workspace *ws;
    const int32_t *offsets;
    const PermPool *pool;
};

// true, g_err set: the table is not valid for these contigs or -- drivers only, behind their own check of the regions -- a
// region on a known contig fits in no segment
static bool perm_ws_refused(const char *who, const igd_hip_workspace *ws, const int32_t *ctg_len, int32_t nctg, const int32_t *ichr,
                            const int32_t *qs, const int32_t *qe, int64_t nq, bool mustFit)
{
    if (!ws) return false;
    if (!igd_hip_workspace_valid(ws, ctg_len, nctg)) {
        snprintf(g_err, sizeof g_err, "%s: the workspace table is not valid for the %d contigs of the call", who, (int)nctg);
        return true;
    }
    const int64_t i = mustFit ? igd_hip_perm_first_unplaceable(ws, ctg_len, ichr, qs, qe, nq) : -1;
    if (i >= 0)
        snprintf(g_err, sizeof g_err, "%s: region %lld = (%d, %d, %d) fits in no segment of the workspace on its contig", who, (long long)i,
                 (int)ichr[i], (int)qs[i], (int)qe[i]);
    return i >= 0;
}

// THE REFUSALS OF THE THREE DRIVERS, in this order: a missing argument (extraBad: what else the driver calls one -- a missing
// output, no such rule), a mode the call cannot run, the number of permutations, more regions than a batch, the first region
// off its contig, a workspace table that is not valid for the database's contigs, the first region in no segment.  true, g_err
// set, prefixed with `who`.  Each driver has its own check in front (min_overlap, the window); the support's bound on the sum of
// squares runs BEHIND this function, so a call that also has one of the last three faults is now told of that fault instead.
// With a pool (mode IGD_HIP_PERM_RESAMPLE) nothing is placed: no contig lengths are asked for and no region is validated; the
// pool's size is held against the batch and against nq instead.
static bool perm_args_refused(const char *who, const igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                              const PermSpec &sp, bool extraBad)
{
    const auto [ctg_len, mode, seed, nperm, ws, offsets, pool] = sp;
    const bool poolBad = pool && (pool->npool < 0 || (pool->npool > 0 && (!pool->ichr || !pool->qs || !pool->qe)));
    if (!db || nq < 0 || extraBad || (nq > 0 && (!ichr || !qs || !qe)) || (!pool && !ctg_len && db->nCtg > 0) || poolBad ||
        !igd_hip_perm_mode_ok(mode, ws != nullptr, pool != nullptr)) {
        snprintf(g_err, sizeof g_err, "%s: bad argument", who);
        return true;
    }
    if (nperm < 1 || nperm > IGD_HIP_PERM_MAX) {
        snprintf(g_err, sizeof g_err, "%s: %lld permutations, not 1 .. %lld", who, (long long)nperm, (long long)IGD_HIP_PERM_MAX);
        return true;
    }
    if (nq > max_batch()) {
        snprintf(g_err, sizeof g_err, "%s: %lld regions, more than %lld", who, (long long)nq, (long long)max_batch());
        return true;
    }
    if (pool) {
        if (pool->npool > max_batch())
            snprintf(g_err, sizeof g_err, "%s: a pool of %lld regions, more than %lld", who, (long long)pool->npool, (long long)max_batch());
        else if (pool->npool < nq)
            snprintf(g_err, sizeof g_err, "%s: %lld regions cannot be drawn without replacement from a pool of %lld", who, (long long)nq,
                     (long long)pool->npool);
        return pool->npool > max_batch() || pool->npool < nq;
    }
    const int64_t i = igd_hip_perm_first_bad(ichr, qs, qe, nq, ctg_len, db->nCtg);
    if (i >= 0) {
        snprintf(g_err, sizeof g_err, "%s: region %lld = (%d, %d, %d) does not lie on its contig of length %lld", who, (long long)i,
                 (int)ichr[i], (int)qs[i], (int)qe[i], (long long)ctg_len[ichr[i]]);
        return true;
    }
    return perm_ws_refused(who, ws, ctg_len, db->nCtg, ichr, qs, qe, nq, true);
}

// THE PLACEMENT OF ONE CALL, written once for the two launch sites (run_perm_chunks, igd_hip_permute_regions_ws): the call's nq
// regions and nctg contig lengths on the device (db->d_pmReg), the mode and, under IGD_HIP_PERM_WORKSPACE, the table (db->d_pmWs);
// under IGD_PERM_PLACE_SHIFT the offsets, behind the contig lengths in db->d_pmReg; under IGD_HIP_PERM_RESAMPLE the pool's three
// arrays in the same place.
struct PermPlace {
    const int32_t *rC, *rS, *rE, *rL;
    int64_t nq;
    int32_t nctg;
    int mode;
    const int64_t *wOff;
    const int32_t *wStart, *wLen, *wPre;
    const int32_t *offs;
    const int32_t *pC, *pS, *pE;
    int64_t npool;
};

// the pool's three arrays to `at` (device, 3 * npool words) on the engine's stream, and into the placement
static int perm_pool_upload(igd_hip_db *db, const PermPool &pool, int32_t *at, PermPlace *pl)
{
    const int64_t n = pool.npool;
    pl->pC = at; pl->pS = at + n; pl->pE = at + 2 * n; pl->npool = n;
    if (n == 0) return IGD_HIP_OK;
    HIPCHK(hipMemcpyAsync(at, pool.ichr, (size_t)n * 4, hipMemcpyHostToDevice, db->stream));
    HIPCHK(hipMemcpyAsync(at + n, pool.qs, (size_t)n * 4, hipMemcpyHostToDevice, db->stream));
    HIPCHK(hipMemcpyAsync(at + 2 * n, pool.qe, (size_t)n * 4, hipMemcpyHostToDevice, db->stream));
    return IGD_HIP_OK;
}

// both buffers grown, then on the engine's stream the table of a checked workspace (without one only the mode is kept) and the
// regions with the nctg contig lengths; the offsets of a shift call (sp.nperm of them) or the pool of a resampling call go up last
static int perm_place_upload(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t nctg,
                             const PermSpec &sp, PermPlace *pl)
{
    const auto [ctg_len, mode, seed, nperm, ws, offsets, pool] = sp;
    const int64_t nshift = offsets ? nperm : 0;
    const int64_t nc = ws ? ws->nctg : 0, ns = ws ? ws->nseg : 0;
    hipStream_t st = db->stream;
    int rc = dev_grow(db, &db->d_pmReg, &db->pmRegCap, 3 * nq + nctg + nshift + (pool ? 3 * pool->npool : 0));
    if (rc == IGD_HIP_OK && ws) rc = dev_grow(db, &db->d_pmWs, &db->pmWsCap, 2 * (nc + 1) + 3 * ns + nc + 1);
    if (rc != IGD_HIP_OK) return rc;
    int32_t *rC = db->d_pmReg, *rS = rC + nq, *rE = rS + nq, *rL = rE + nq;
    *pl = PermPlace{rC, rS, rE, rL, nq, nctg, mode, nullptr, nullptr, nullptr, nullptr, nshift > 0 ? rL + nctg : nullptr, nullptr, nullptr, nullptr, 0};
    if (ws) {
        int64_t *dOff = (int64_t *)db->d_pmWs;
        int32_t *dStart = db->d_pmWs + 2 * (nc + 1), *dLen = dStart + ns, *dPre = dLen + ns;
        HIPCHK(hipMemcpyAsync(dOff, ws->w_off, (size_t)(nc + 1) * 8, hipMemcpyHostToDevice, st));
        if (ns > 0) {
            HIPCHK(hipMemcpyAsync(dStart, ws->w_start, (size_t)ns * 4, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(dLen, ws->w_len, (size_t)ns * 4, hipMemcpyHostToDevice, st));
        }
        if (ns + nc > 0) HIPCHK(hipMemcpyAsync(dPre, ws->w_pre, (size_t)(ns + nc) * 4, hipMemcpyHostToDevice, st));
        pl->wOff = dOff; pl->wStart = dStart; pl->wLen = dLen; pl->wPre = dPre;
    }
    HIPCHK(hipMemcpyAsync(rC, ichr, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(rS, qs, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(rE, qe, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    if (nctg > 0) HIPCHK(hipMemcpyAsync(rL, ctg_len, (size_t)nctg * 4, hipMemcpyHostToDevice, st));
    if (nshift > 0) HIPCHK(hipMemcpyAsync(rL + nctg, offsets, (size_t)nshift * 4, hipMemcpyHostToDevice, st));
    if (pool) return perm_pool_upload(db, *pool, rL + nctg + nshift, pl);
    return IGD_HIP_OK;
}

// `total` outputs (permutations from p0 on, nq regions each) by the kernel of the call's placement; under IGD_PERM_PLACE_SHIFT
// permutation p is the shift by offsets[p] and the seed is not read; under IGD_HIP_PERM_RESAMPLE the outputs are pool regions, the
// call's own are not read and oC is always written
static int permute_launch(igd_hip_db *db, const PermPlace &pl, u64 seed, u64 p0, int64_t total, int32_t *oC, int32_t *oS, int32_t *oE)
{
    const unsigned grid = (unsigned)igd_hip_permute_grid(total);
    if (pl.mode == IGD_HIP_PERM_RESAMPLE)
        igd_resample_regions<<<grid, IGD_SETS_WG, 0, db->stream>>>(pl.pC, pl.pS, pl.pE, (unsigned)pl.npool, (unsigned)pl.nq, seed, p0, (unsigned)total,
                                                                 oC, oS, oE);
    else if (pl.mode == IGD_PERM_PLACE_SHIFT)
        igd_shift_regions<<<grid, IGD_SETS_WG, 0, db->stream>>>(pl.rC, pl.rS, pl.rE, (unsigned)pl.nq, pl.rL, pl.nctg, pl.offs, (unsigned)p0,
                                                              (unsigned)total, oC, oS, oE);
    else if (pl.mode == IGD_HIP_PERM_WORKSPACE)
        igd_permute_workspace<<<grid, IGD_SETS_WG, 0, db->stream>>>(pl.rC, pl.rS, pl.rE, (unsigned)pl.nq, pl.rL, pl.nctg, pl.wOff, pl.wStart, pl.wLen,
                                                                  pl.wPre, seed, p0, (unsigned)total, oC, oS, oE);
    else
        igd_permute_regions<<<grid, IGD_SETS_WG, 0, db->stream>>>(pl.rC, pl.rS, pl.rE, (unsigned)pl.nq, pl.rL, pl.nctg, pl.mode, seed, p0,
                                                                (unsigned)total, oC, oS, oE);
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

// The generator alone, for the entries that return the regions themselves (igd_hip_permute_regions_ws, igd_hip_resample_regions,
// igd_hip_shift_regions), behind their uploads and ensure_qstage(pc * nq): permutations [p0, p0 + np) of the placement, pc per
// launch into the staging arrays, each chunk copied back behind its launch into home[] (the call's own buffers, np * nq words
// each; contigs, starts, ends -- home[0] == nullptr: no contigs are generated); ONE wait, then the caller's arrays out[].
static int perm_regions_home(igd_hip_db *db, const PermPlace &pl, u64 seed, int64_t p0, int64_t np, int64_t pc, int32_t *const home[3],
                             int32_t *const out[3])
{
    const int64_t nq = pl.nq;
    int32_t *const stage[3] = {home[0] ? db->d_qc : nullptr, db->d_qs, db->d_qe};
    hipStream_t st = db->stream;
    for (int64_t a = 0; a < np; a += pc) {
        const int64_t n = np - a < pc ? np - a : pc;
        const int rc = permute_launch(db, pl, seed, (u64)(p0 + a), n * nq, stage[0], stage[1], stage[2]);
        if (rc != IGD_HIP_OK) return rc;
        for (int i = 0; i < 3; i++)
            if (home[i]) HIPCHK(hipMemcpyAsync(home[i] + a * nq, stage[i], (size_t)(n * nq) * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    for (int i = 0; i < 3; i++)
        if (home[i]) memcpy(out[i], home[i], (size_t)(np * nq) * 4);
    return IGD_HIP_OK;
}

// the host slice table of a chunk of pc rows of nq staged regions: row r cut as igd_hip_support_sets cuts a set (the support, the
// fused nearest kernel); a shorter chunk uses a prefix of it
static std::vector<SetSlice> perm_row_slices(int64_t pc, int64_t nq, int64_t sliceLen)
{
    std::vector<SetSlice> slices;
    slices.reserve((size_t)(pc * ((nq + sliceLen - 1) / sliceLen)));
    for (int64_t r = 0; r < pc; r++) push_slices(slices, (int32_t)r, r * nq, (r + 1) * nq, sliceLen, 0);
    return slices;
}

// The chunk driver of the three nulls (the arguments are checked, nq > 0).  A chunk holds pc permutations: pc * nq <=
// igd_hip_max_batch() (the staging arrays of igd_hip_search) and, unless rowBytes is 0, pc * rowBytes <= perm_row_bytes(); at
// least one, at most nperm.  prepare(pc, sliceLen, perRow) grows the statistic's own workspaces for such a chunk, cut into
// slices of sliceLen = sets_slice_len(pc * nq) regions, perRow of them per row; it enqueues nothing.  Then the staging arrays and
// the placement's two buffers are grown -- every dev_grow of the call is over before its first upload -- and the regions, the
// contig lengths and the table go up once.  count(c, s, e, rows, r0) enqueues what the statistic does with `rows` rows of nq
// resident regions each, rows [r0, r0 + rows) of the null: first the set as given (r0 == 0, one row: the regions themselves;
// this call also uploads what every chunk reads, and adds what the statistic does once behind row 0), then per chunk the
// generator's output in the staging arrays (r0 = 1 + p0); the call with r0 + rows == nperm + 1 is the last.  Everything is on the
// engine's stream without a wait in between, unless count waits itself; ONE wait at the end, behind which the callers write
// their results.  sp.offsets: the table of mode IGD_PERM_PLACE_SHIFT, nperm entries -- "permutation" p is then the set shifted
// by offsets[p], and the caller's count has nothing to do with the set as given.  sp.pool (mode IGD_HIP_PERM_RESAMPLE, which has
// no ctg_len): its regions go up behind the call's, and permutation p is a draw from it.
template <typename Prepare, typename Count>
static int run_perm_chunks(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const PermSpec &sp,
                           int64_t rowBytes, Prepare &&prepare, Count &&count)
{
    const int64_t nperm = sp.nperm;
    HIPCHK(hipSetDevice(db->device));
    int64_t pc = max_batch() / nq;
    const int64_t byRows = rowBytes > 0 ? perm_row_bytes() / rowBytes : pc;
    if (byRows < pc) pc = byRows < 1 ? 1 : byRows;
    if (nperm < pc) pc = nperm;
    const int64_t sliceLen = sets_slice_len(pc * nq);
    const int64_t perRow = (nq + sliceLen - 1) / sliceLen;                // slices of one permutation
    int rc = prepare(pc, sliceLen, perRow);
    if (rc == IGD_HIP_OK) rc = ensure_qstage(db, pc * nq);
    PermPlace pl;
    if (rc == IGD_HIP_OK) rc = perm_place_upload(db, ichr, qs, qe, nq, sp.pool ? 0 : db->nCtg, sp, &pl);
    if (rc == IGD_HIP_OK) rc = count(pl.rC, pl.rS, pl.rE, (int64_t)1, (int64_t)0);      // the set as given
    for (int64_t p0 = 0; rc == IGD_HIP_OK && p0 < nperm; p0 += pc) {
        const int64_t n = nperm - p0 < pc ? nperm - p0 : pc;
        rc = permute_launch(db, pl, (u64)sp.seed, (u64)p0, n * nq, db->d_qc, db->d_qs, db->d_qe);
        if (rc == IGD_HIP_OK) rc = count(db->d_qc, db->d_qs, db->d_qe, n, 1 + p0);
    }
    if (rc != IGD_HIP_OK) return rc;
    HIPCHK(hipStreamSynchronize(db->stream));
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

// igd_perm_stats over nrows rows (device) into the six arrays at d_st; d_tot: see permute_dev.hpp
static int perm_stats_launch(igd_hip_db *db, const int64_t *d_rows, const int64_t *d_tot, int64_t nrows, int64_t ncols,
                             const long long *d_obs, long long *d_st)
{
    const int64_t gx = (ncols + IGD_WAVE - 1) / IGD_WAVE, waves = IGD_SETS_WG / IGD_WAVE;
    int64_t gy = (nrows + waves - 1) / waves;
    const int64_t room = IGD_SETS_GRID / gx > 1 ? IGD_SETS_GRID / gx : 1;
    if (gy > room) gy = room;
    if (gy > IGD_PERM_STATS_ROWS_Y) gy = IGD_PERM_STATS_ROWS_Y;
    igd_perm_stats<<<dim3((unsigned)gx, (unsigned)gy), IGD_SETS_WG, 0, db->stream>>>((const long long *)d_rows, (const long long *)d_tot, nrows,
                                                                                  ncols, d_obs, d_st);
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

static int perm_stats_init(igd_hip_db *db, long long *d_st, int64_t ncols)
{
    const int64_t g = (6 * ncols + IGD_SETS_WG - 1) / IGD_SETS_WG;
    igd_perm_stats_init<<<(unsigned)(g < IGD_SETS_GRID ? g : IGD_SETS_GRID), IGD_SETS_WG, 0, db->stream>>>(d_st, ncols);
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

// the six statistics of a call whose every permuted value is 0 against observed 0 (no region, or no file)
static void perm_all_zero(int64_t *res, int64_t nC, int64_t nperm)
{
    for (int64_t f = 0; f < nC; f++) {
        res[f] = res[nC + f] = res[2 * nC + f] = res[5 * nC + f] = res[6 * nC + f] = 0;
        res[3 * nC + f] = res[4 * nC + f] = nperm;
    }
}

// res = observed, sum, sumsq, n_ge, n_le, min, max, nC words each -> the caller's arrays
static void perm_copy_out(const int64_t *res, int64_t nC, int64_t *const out[7])
{
    for (int a = 0; a < 7; a++)
        if (out[a]) memcpy(out[a], res + a * nC, (size_t)nC * 8);
}

// the body of igd_hip_permute_support_ws and, with a pool and no ctg_len, of igd_hip_permute_support_rs
static int permute_support_run(const char *who, igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const PermSpec &sp, int32_t v, int rule, int64_t *observed, int64_t *sum, int64_t *sumsq, int64_t *n_ge,
                               int64_t *n_le, int64_t *pmin, int64_t *pmax, const igd_hip_min_overlap *min_overlap)
{
    const int64_t nperm = sp.nperm;
    if (!igd_hip_min_overlap_valid(min_overlap)) {
        snprintf(g_err, sizeof g_err, "%s: min_overlap (%d bp, %d ppm, %d ppm) out of range", who, (int)min_overlap->min_bp,
                 (int)min_overlap->ppm_query, (int)min_overlap->ppm_record);
        return IGD_HIP_ERR_ARG;
    }
    const bool ov = igd_hip_min_overlap_active(min_overlap);
    const MinOv mo = min_ov_of(min_overlap);
    if (perm_args_refused(who, db, ichr, qs, qe, nq, sp, !observed || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)))
        return IGD_HIP_ERR_ARG;
    if ((unsigned __int128)nperm * (unsigned __int128)nq * (unsigned __int128)nq >= (unsigned __int128)1 << 63) {
        snprintf(g_err, sizeof g_err, "%s: %lld permutations of %lld regions: the sum of squares may pass 2^63", who, (long long)nperm,
                 (long long)nq);
        return IGD_HIP_ERR_ARG;
    }
    const int64_t nF = db->nFiles, nC = nF + 1;
    int64_t *const out[7] = {observed, sum, sumsq, n_ge, n_le, pmin, pmax};
    std::vector<int64_t> res((size_t)(7 * nC));
    if (nq == 0 || nF == 0) {
        perm_all_zero(res.data(), nC, nperm);
        perm_copy_out(res.data(), nC, out);
        return IGD_HIP_OK;
    }

    const SliceImage im = slice_image(db, rule, v);
    const int64_t maxGrid = support_max_grid(db);
    hipStream_t st = db->stream;
    std::vector<SetSlice> slices;
    int64_t perRow = 0;
    auto prepare = [&](int64_t pc, int64_t sliceLen, int64_t perRow_) -> int {
        perRow = perRow_;
        slices = perm_row_slices(pc, nq, sliceLen);
        int rc = dev_grow(db, &db->d_pmStat, &db->pmStatCap, 7 * nC);
        if (rc == IGD_HIP_OK) rc = sets_ws(db, pc * nF, pc, pc * perRow);
        if (rc == IGD_HIP_OK) rc = ensure_support_bits(db, maxGrid);
        return rc;
    };
    // `rows` zeroed rows counted from the query arrays (c, s, e): rows * perRow slices, a prefix of the table.  Row 0 becomes
    // `observed` and opens the statistics; a chunk is folded into them, and the last one sends them home.
    auto count = [&](const int32_t *c, const int32_t *s, const int32_t *e, int64_t rows, int64_t r0) -> int {
        const int ns = (int)(rows * perRow);
        const int grid = ns < maxGrid ? ns : (int)maxGrid;
        long long *dObs = db->d_pmStat, *dSt = dObs + nC;
        if (r0 == 0) HIPCHK(hipMemcpyAsync(db->d_setSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(db->d_setRows, 0, (size_t)(rows * nF) * 8, st));
        HIPCHK(hipMemsetAsync(db->d_setTot, 0, (size_t)rows * 8, st));
        int rc = support_launch(db, im, c, s, e, ns, grid, v, ov, mo);
        if (rc != IGD_HIP_OK) return rc;
        if (r0 == 0) {
            HIPCHK(hipMemcpyAsync(dObs, db->d_setRows, (size_t)nF * 8, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(dObs + nF, db->d_setTot, 8, hipMemcpyDeviceToDevice, st));
            return perm_stats_init(db, dSt, nC);
        }
        if ((rc = perm_stats_launch(db, db->d_setRows, db->d_setTot, rows, nC, dObs, dSt)) != IGD_HIP_OK) return rc;
        if (r0 + rows == nperm + 1) HIPCHK(hipMemcpyAsync(res.data(), db->d_pmStat, (size_t)(7 * nC) * 8, hipMemcpyDeviceToHost, st));
        return IGD_HIP_OK;
    };
    const int rc = run_perm_chunks(db, ichr, qs, qe, nq, sp, nF * 8, prepare, count);
    if (rc != IGD_HIP_OK) return rc;
    perm_copy_out(res.data(), nC, out);
    return IGD_HIP_OK;
}

extern "C" int igd_hip_permute_support_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                          const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule,
                                          int64_t *observed, int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin,
                                          int64_t *pmax, const igd_hip_min_overlap *min_overlap, const igd_hip_workspace *ws)
{
    const PermSpec sp{ctg_len, mode, seed, nperm, ws, nullptr, nullptr};
    return permute_support_run("igd_hip_permute_support", db, ichr, qs, qe, nq, sp, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax,
                               min_overlap);
}

extern "C" int igd_hip_permute_support_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                          const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool,
                                          uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *observed, int64_t *sum,
                                          int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax,
                                          const igd_hip_min_overlap *min_overlap)
{
    const PermPool pool{pool_ichr, pool_qs, pool_qe, npool};
    const PermSpec sp{nullptr, IGD_HIP_PERM_RESAMPLE, seed, nperm, nullptr, nullptr, &pool};
    return permute_support_run("igd_hip_permute_support_rs", db, ichr, qs, qe, nq, sp, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax,
                               min_overlap);
}

extern "C" int igd_hip_permute_support_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                          const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule,
                                          int64_t *observed, int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin,
                                          int64_t *pmax, const igd_hip_min_overlap *min_overlap)
{
    return igd_hip_permute_support_ws(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax,
                                      min_overlap, nullptr);
}

extern "C" int igd_hip_permute_support(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                       const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t v, int rule,
                                       int64_t *observed, int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin,
                                       int64_t *pmax)
{
    return igd_hip_permute_support_ov(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, observed, sum, sumsq, n_ge, n_le, pmin, pmax,
                                      nullptr);
}

extern "C" int igd_hip_permute_regions_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                          const int32_t *ctg_len, int32_t nctg, int mode, uint64_t seed, int64_t p0, int64_t np,
                                          int32_t *out_qs, int32_t *out_qe, const igd_hip_workspace *ws)
{
    if (!db || nq < 0 || np < 0 || p0 < 0 || nctg < 0 || (nctg > 0 && !ctg_len) || (nq > 0 && (!ichr || !qs || !qe)) ||
        (nq > 0 && np > 0 && (!out_qs || !out_qe)) || !igd_hip_perm_mode_ok(mode, ws != nullptr, 0) ||
        nq > max_batch() || (nq > 0 && np > (int64_t)INT32_MAX / nq)) {
        snprintf(g_err, sizeof g_err, "igd_hip_permute_regions: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (perm_ws_refused("igd_hip_permute_regions", ws, ctg_len, nctg, ichr, qs, qe, nq, false)) return IGD_HIP_ERR_ARG;
    if (nq == 0 || np == 0) return IGD_HIP_OK;
    const int64_t pc = max_batch() / nq < np ? max_batch() / nq : np;
    std::vector<int32_t> hs((size_t)(np * nq)), he((size_t)(np * nq));
    HIPCHK(hipSetDevice(db->device));
    int rc = ensure_qstage(db, pc * nq);
    PermPlace pl;
    if (rc == IGD_HIP_OK) rc = perm_place_upload(db, ichr, qs, qe, nq, nctg, PermSpec{ctg_len, mode, seed, np, ws, nullptr, nullptr}, &pl);
    if (rc != IGD_HIP_OK) return rc;
    int32_t *const home[3] = {nullptr, hs.data(), he.data()}, *const out[3] = {nullptr, out_qs, out_qe};
    return perm_regions_home(db, pl, (u64)seed, p0, np, pc, home, out);
}

extern "C" int igd_hip_permute_regions(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                       const int32_t *ctg_len, int32_t nctg, int mode, uint64_t seed, int64_t p0, int64_t np,
                                       int32_t *out_qs, int32_t *out_qe)
{
    return igd_hip_permute_regions_ws(db, ichr, qs, qe, nq, ctg_len, nctg, mode, seed, p0, np, out_qs, out_qe, nullptr);
}

// the generator of the resampling null alone: draws [p0, p0 + np) of nq regions from the pool, chunked as igd_hip_permute_regions
extern "C" int igd_hip_resample_regions(igd_hip_db *db, const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe,
                                        int64_t npool, int64_t nq, uint64_t seed, int64_t p0, int64_t np, int32_t *out_ichr, int32_t *out_qs,
                                        int32_t *out_qe)
{
    if (!db || nq < 0 || np < 0 || p0 < 0 || npool < 0 || (npool > 0 && (!pool_ichr || !pool_qs || !pool_qe)) ||
        (nq > 0 && np > 0 && (!out_ichr || !out_qs || !out_qe)) || nq > max_batch() || npool > max_batch() ||
        (nq > 0 && np > (int64_t)INT32_MAX / nq)) {
        snprintf(g_err, sizeof g_err, "igd_hip_resample_regions: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (npool < nq) {
        snprintf(g_err, sizeof g_err, "igd_hip_resample_regions: %lld regions cannot be drawn without replacement from a pool of %lld",
                 (long long)nq, (long long)npool);
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0 || np == 0) return IGD_HIP_OK;
    const int64_t pc = max_batch() / nq < np ? max_batch() / nq : np;
    std::vector<int32_t> h((size_t)(3 * np * nq));
    int32_t *hc = h.data(), *hs = hc + np * nq, *he = hs + np * nq;
    HIPCHK(hipSetDevice(db->device));
    int rc = ensure_qstage(db, pc * nq);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_pmReg, &db->pmRegCap, 3 * npool);
    if (rc != IGD_HIP_OK) return rc;
    PermPlace pl{nullptr, nullptr, nullptr, nullptr, nq, 0, IGD_HIP_PERM_RESAMPLE, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    const PermPool pool{pool_ichr, pool_qs, pool_qe, npool};
    if ((rc = perm_pool_upload(db, pool, db->d_pmReg, &pl)) != IGD_HIP_OK) return rc;
    int32_t *const home[3] = {hc, hs, he}, *const out[3] = {out_ichr, out_qs, out_qe};
    return perm_regions_home(db, pl, (u64)seed, p0, np, pc, home, out);
}

extern "C" int igd_hip_perm_stats(igd_hip_db *db, const int64_t *rows, int64_t nrows, int64_t ncols, const int64_t *observed,
                                  int64_t *sum, int64_t *sumsq, int64_t *n_ge, int64_t *n_le, int64_t *pmin, int64_t *pmax)
{
    if (!db || !rows || !observed || nrows < 1 || ncols < 1 || ncols > ((int64_t)1 << 40) / nrows) {
        snprintf(g_err, sizeof g_err, "igd_hip_perm_stats: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    int64_t rc_ = perm_row_bytes() / (ncols * 8);
    const int64_t step = rc_ < 1 ? 1 : rc_ < nrows ? rc_ : nrows;
    std::vector<int64_t> res((size_t)(7 * ncols));
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    int rc = dev_grow(db, &db->d_pmStat, &db->pmStatCap, 7 * ncols);
    if (rc == IGD_HIP_OK) rc = sets_ws(db, step * ncols, step, 0);
    if (rc != IGD_HIP_OK) return rc;
    long long *dObs = db->d_pmStat, *dSt = dObs + ncols;
    HIPCHK(hipMemcpyAsync(dObs, observed, (size_t)ncols * 8, hipMemcpyHostToDevice, st));
    if ((rc = perm_stats_init(db, dSt, ncols)) != IGD_HIP_OK) return rc;
    for (int64_t r0 = 0; r0 < nrows; r0 += step) {
        const int64_t n = nrows - r0 < step ? nrows - r0 : step;
        HIPCHK(hipMemcpyAsync(db->d_setRows, rows + r0 * ncols, (size_t)(n * ncols) * 8, hipMemcpyHostToDevice, st));
        if ((rc = perm_stats_launch(db, db->d_setRows, nullptr, n, ncols, dObs, dSt)) != IGD_HIP_OK) return rc;
    }
    HIPCHK(hipMemcpyAsync(res.data(), db->d_pmStat, (size_t)(7 * ncols) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    int64_t *const out[7] = {nullptr, sum, sumsq, n_ge, n_le, pmin, pmax};
    perm_copy_out(res.data(), ncols, out);
    return IGD_HIP_OK;
}
