// engine/host_cooccur.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_cooccur, igd_hip_bits_transpose, igd_hip_bitrows_gram (cooccur_dev.hpp)
// ------------------------------------------------------------------------------------------
// The co-occurrence.  The regions go through in the CHUNKS of igd_hip_membership (run_region_chunks, host_common.hpp): at most
// igd_hip_max_batch() regions and member_row_bytes() of rows; the first chunk is the largest and every workspace is grown once,
// before the loop.  Per chunk, all on the engine's stream: the regions to the staging buffers, igd_hip_membership_dev
// into the handle's rows, igd_bits_transpose into the handle's columns (32 * nW columns of ceil(chunk / 64) words; the tail bits
// of a chunk's last word are 0, so a chunk end that is no multiple of 64 adds nothing), igd_bitrows_gram<true> over the first
// nFiles columns ADDING into the handle's matrix, which was zeroed once before the first chunk.  The rows never leave the
// device; the matrix and the hit counter are copied out once, behind the last chunk.
// The generic entries take host arrays: the rows go up with a pitched copy into rows of an even number of words (the pad word
// zeroed first), the matrix is zeroed on the stream, one launch, the result comes back.
// (IGD_COOCCUR_MAX_FILES = 16 384, include/igd_hip.h: the int64 matrix would be 2 GiB)
#define IGD_GRAM_MAX_CELLS ((int64_t)1 << 28)        // the generic entry's matrix: the same 2 GiB

// The TEST-ONLY variable IGD_HIP_COOCCUR_MAX_FILES (read once per process, as IGD_HIP_MEMBER_ROW_BYTES) lowers the limit so
// that the refusal is met by a small fixture.
static int64_t cooccur_max_files(void)
{
    static const int64_t m = std::min(env_positive("IGD_HIP_COOCCUR_MAX_FILES", IGD_COOCCUR_MAX_FILES), (int64_t)IGD_COOCCUR_MAX_FILES);
    return m;
}

// words per slice and slices of a Gram launch over `tiles` tiles and nw64 words
static void gram_plan(int64_t tiles, int64_t nw64, int64_t *sliceLen, int64_t *slices)
{
    int64_t s = tiles > 0 ? (IGD_GRAM_TARGET + tiles - 1) / tiles : 1;
    const int64_t cap = nw64 / IGD_GRAM_SLICE_MIN;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    int64_t len = (nw64 + s - 1) / s;
    len = (len + IGD_GRAM_KSTEP - 1) / IGD_GRAM_KSTEP * IGD_GRAM_KSTEP;
    if (len > IGD_GRAM_SLICE_MAX) len = IGD_GRAM_SLICE_MAX;
    if (len < IGD_GRAM_KSTEP) len = IGD_GRAM_KSTEP;
    *sliceLen = len;
    *slices = nw64 > 0 ? (nw64 + len - 1) / len : 1;
}

static int64_t gram_tiles(int64_t m, int64_t n, bool sym)
{
    const int64_t tm = (m + IGD_GRAM_TILE - 1) / IGD_GRAM_TILE, tn = (n + IGD_GRAM_TILE - 1) / IGD_GRAM_TILE;
    return sym ? tm * (tm + 1) / 2 : tm * tn;
}

extern "C" int32_t igd_hip_gram_tile(void) { return IGD_GRAM_TILE; }
extern "C" int32_t igd_hip_gram_kstep(void) { return IGD_GRAM_KSTEP; }
// slices of a launch for A = m rows, B = n rows (n == 0: the symmetric form, B == A) of nwords32 uint32 words
extern "C" int64_t igd_hip_gram_slices(int64_t m, int64_t n, int64_t nwords32)
{
    if (m <= 0 || n < 0 || nwords32 <= 0) return 0;
    int64_t len, s;
    gram_plan(gram_tiles(m, n ? n : m, n == 0), (nwords32 + 1) / 2, &len, &s);
    return s;
}

// one launch on the stream: out[m x n] (leading dimension n) += the Gram product of the resident rows; B == nullptr: symmetric
static int gram_launch(const u64 *A, int64_t m, const u64 *B, int64_t n, int64_t stride, int64_t nw64, u64 *out, hipStream_t st)
{
    const bool sym = B == nullptr;
    if (sym) n = m;
    if (m <= 0 || n <= 0 || nw64 <= 0) return IGD_HIP_OK;
    const int64_t tiles = gram_tiles(m, n, sym), tn = (n + IGD_GRAM_TILE - 1) / IGD_GRAM_TILE;
    int64_t len, slices;
    gram_plan(tiles, nw64, &len, &slices);
    if (tiles > INT32_MAX || slices > 65535) {
        snprintf(g_err, sizeof g_err, "igd_bitrows_gram: %lld tiles x %lld slices do not fit one grid", (long long)tiles, (long long)slices);
        return IGD_HIP_ERR_ARG;
    }
    const dim3 grid((unsigned)tiles, (unsigned)slices);
    if (sym) igd_bitrows_gram<true><<<grid, IGD_SETS_WG, 0, st>>>(A, m, A, n, stride, nw64, len, (int)tn, out, n);
    else igd_bitrows_gram<false><<<grid, IGD_SETS_WG, 0, st>>>(A, m, B, n, stride, nw64, len, (int)tn, out, n);
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

// one launch on the stream: the n resident rows of nW words into 32 * nW columns of ceil(n / 64) words
static int transpose_launch(const unsigned *bits, int64_t n, int64_t nW, u64 *cols, hipStream_t st)
{
    const int64_t cw = (n + 63) / 64;
    if (nW <= 0 || cw <= 0) return IGD_HIP_OK;
    const int64_t groups = (cw + IGD_TR_BLOCKS - 1) / IGD_TR_BLOCKS;
    if (nW > INT32_MAX || groups > INT32_MAX / nW) {
        snprintf(g_err, sizeof g_err, "igd_bits_transpose: %lld rows of %lld words do not fit one grid", (long long)n, (long long)nW);
        return IGD_HIP_ERR_ARG;
    }
    igd_bits_transpose<<<(unsigned)(groups * nW), IGD_SETS_WG, 0, st>>>(bits, n, (int)nW, cw, cols);
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

extern "C" int igd_hip_bits_transpose(igd_hip_db *db, const uint32_t *bits, int64_t nrows, int64_t nW, uint64_t *cols)
{
    const int64_t cw = nrows > 0 ? (nrows + 63) / 64 : 0;
    if (!db || nrows < 0 || nW < 0 || nW > ((int64_t)1 << 26) || (nrows > 0 && nW > 0 && (!bits || !cols)) ||
        (nW > 0 && nrows > INT64_MAX / 64 / nW)) {
        snprintf(g_err, sizeof g_err, "igd_hip_bits_transpose: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nrows == 0 || nW == 0) return IGD_HIP_OK;
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    int rc = dev_grow(db, &db->d_coA, &db->coACap, (nrows * nW + 1) / 2);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_coCols, &db->coColsCap, 32 * nW * cw);
    if (rc != IGD_HIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(db->d_coA, bits, (size_t)(nrows * nW) * 4, hipMemcpyHostToDevice, st));
    rc = transpose_launch((const unsigned *)db->d_coA, nrows, nW, db->d_coCols, st);
    if (rc != IGD_HIP_OK) return rc;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(cols, db->d_coCols, (size_t)(32 * nW * cw) * 8, hipMemcpyDeviceToHost));
    return IGD_HIP_OK;
}

// host rows of nwords32 uint32 words into resident rows of nw64 uint64 words (an odd nwords32: the pad word is zero)
static int gram_upload(igd_hip_db *db, u64 **d, int64_t *cap, const uint32_t *h, int64_t rows, int64_t nwords32, int64_t nw64, hipStream_t st)
{
    int rc = dev_grow(db, d, cap, rows * nw64);
    if (rc != IGD_HIP_OK) return rc;
    if (nwords32 & 1) {
        HIPCHK(hipMemsetAsync(*d, 0, (size_t)(rows * nw64) * 8, st));
        HIPCHK(hipMemcpy2DAsync(*d, (size_t)nw64 * 8, h, (size_t)nwords32 * 4, (size_t)nwords32 * 4, (size_t)rows, hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(hipMemcpyAsync(*d, h, (size_t)(rows * nw64) * 8, hipMemcpyHostToDevice, st));
    }
    return IGD_HIP_OK;
}

extern "C" int igd_hip_bitrows_gram(igd_hip_db *db, const uint32_t *a, int64_t m, const uint32_t *b, int64_t n, int64_t nwords32, int64_t *out)
{
    const bool sym = b == nullptr;
    if (sym) n = m;
    if (!db || m < 0 || n < 0 || nwords32 < 0 || nwords32 > ((int64_t)1 << 40) || (m > 0 && n > 0 && !out) ||
        (m > 0 && nwords32 > 0 && !a) || (m > 0 && n > IGD_GRAM_MAX_CELLS / m) ||
        (nwords32 > 0 && (m > ((int64_t)1 << 50) / nwords32 || n > ((int64_t)1 << 50) / nwords32))) {
        snprintf(g_err, sizeof g_err, "igd_hip_bitrows_gram: bad argument (at most 2^28 cells)");
        return IGD_HIP_ERR_ARG;
    }
    if (m == 0 || n == 0) return IGD_HIP_OK;
    if (nwords32 == 0) {
        memset(out, 0, (size_t)(m * n) * 8);
        return IGD_HIP_OK;
    }
    const int64_t nw64 = (nwords32 + 1) / 2;
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    int rc = gram_upload(db, &db->d_coA, &db->coACap, a, m, nwords32, nw64, st);
    if (rc == IGD_HIP_OK && !sym) rc = gram_upload(db, &db->d_coB, &db->coBCap, b, n, nwords32, nw64, st);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_coMat, &db->coMatCap, m * n);
    if (rc != IGD_HIP_OK) return rc;
    HIPCHK(hipMemsetAsync(db->d_coMat, 0, (size_t)(m * n) * 8, st));
    rc = gram_launch(db->d_coA, m, sym ? nullptr : db->d_coB, n, nw64, nw64, db->d_coMat, st);
    if (rc != IGD_HIP_OK) return rc;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, db->d_coMat, (size_t)(m * n) * 8, hipMemcpyDeviceToHost));
    return IGD_HIP_OK;
}

extern "C" int igd_hip_cooccur(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t v, int rule,
                               int64_t *cooc, int64_t *nhit)
{
    if (!db || nq < 0 || (nq > 0 && (!ichr || !qs || !qe)) || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT) ||
        (db->nFiles > 0 && !cooc)) {
        snprintf(g_err, sizeof g_err, "igd_hip_cooccur: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    const int64_t nF = db->nFiles, nW = (nF + 31) / 32;
    if (nF > cooccur_max_files()) {
        snprintf(g_err, sizeof g_err, "igd_hip_cooccur: %lld files, more than %lld", (long long)nF, (long long)cooccur_max_files());
        return IGD_HIP_ERR_ARG;
    }
    if (nF == 0 || nq == 0) {
        if (nF) memset(cooc, 0, (size_t)(nF * nF) * 8);
        if (nhit) *nhit = 0;
        return IGD_HIP_OK;
    }
    int64_t step = chunk_step(member_row_bytes(), nW * 4);
    if (nq < step) step = nq;

    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    int rc = dev_grow(db, &db->d_coMat, &db->coMatCap, nF * nF);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_coCols, &db->coColsCap, 32 * nW * ((step + 63) / 64));
    if (rc == IGD_HIP_OK) rc = ensure_qstage(db, step);       // (the first chunk is the largest: stage_queries never grows them)
    if (rc == IGD_HIP_OK) rc = ensure_member_ws(db, step * nW, step);
    if (rc != IGD_HIP_OK) return rc;
    HIPCHK(hipMemsetAsync(db->d_coMat, 0, (size_t)(nF * nF) * 8, st));
    HIPCHK(hipMemsetAsync(db->d_memHit, 0, 8, st));
    rc = run_region_chunks(db, ichr, qs, qe, nq, step, [&](int64_t, int64_t m, hipStream_t) {
        const int64_t cw = (m + 63) / 64;
        int rc2 = igd_hip_membership_dev(db, db->d_qc, db->d_qs, db->d_qe, m, v, rule, db->d_memBits, nullptr, (int64_t *)db->d_memHit, st);
        if (rc2 == IGD_HIP_OK) rc2 = transpose_launch(db->d_memBits, m, nW, db->d_coCols, st);
        if (rc2 == IGD_HIP_OK) rc2 = gram_launch(db->d_coCols, nF, nullptr, nF, cw, cw, db->d_coMat, st);
        return rc2;
    });
    if (rc != IGD_HIP_OK) return rc;
    unsigned long long h = 0;
    HIPCHK(hipMemcpy(&h, db->d_memHit, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cooc, db->d_coMat, (size_t)(nF * nF) * 8, hipMemcpyDeviceToHost));
    if (nhit) *nhit = (int64_t)h;
    return IGD_HIP_OK;
}
