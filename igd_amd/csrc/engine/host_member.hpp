// engine/host_member.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_membership / igd_hip_membership_dev: per query one bit row -- the files it overlaps (igd_member_rows, member_dev.hpp)
// ------------------------------------------------------------------------------------------
// The device form takes one engine batch of resident queries and writes resident rows: one launch (the wide form: a memset
// of the rows before it and, when nfiles_hit is wanted, igd_member_popc behind it), asynchronous on the caller's stream.
// The host form takes host arrays in CHUNKS of at most igd_hip_max_batch() queries AND at most IGD_MEMBER_ROW_BYTES of
// device rows (a database of 10^6 files has 125 KB rows: 2^24 of them would be 2 TB; chunk_step); run_region_chunks
// (host_common.hpp) stages the queries of a chunk, the body here runs the device form on the engine's stream and sends the
// rows back into the caller's array at their place -- rows are per query, so chunks need no merging.
// The image and the rule word are igd_hip_support_sets's (slice_image, host_common.hpp).
#define IGD_MEMBER_ROW_BYTES ((int64_t)256 << 20)    // device rows of one chunk (of the order of IGD_SETS_ROW_BYTES)

// The TEST-ONLY variable IGD_HIP_MEMBER_ROW_BYTES (read once per process, as IGD_HIP_MAX_BATCH) lowers the budget so that
// small fixtures cross the row seam.
static int64_t member_row_bytes(void)
{
    static const int64_t m = env_positive("IGD_HIP_MEMBER_ROW_BYTES", IGD_MEMBER_ROW_BYTES);
    return m;
}

extern "C" int64_t igd_hip_member_words(const igd_hip_db *db) { return db ? ((int64_t)db->nFiles + 31) / 32 : 0; }

// workgroups igd_member_rows is launched with for nq queries (each of IGD_SETS_WG / IGD_WAVE waves; a wave meets a second
// query only when nq exceeds the grid's waves)
extern "C" int32_t igd_hip_member_grid(int64_t nq) { return items_grid(nq, IGD_SETS_WG / IGD_WAVE); }

extern "C" int igd_hip_membership_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq,
                                      int32_t v, int rule, uint32_t *d_bits, int32_t *d_nfiles_hit, int64_t *d_nhit, void *stream)
{
    if (!db || nq < 0 || nq > max_batch() || (nq > 0 && (!d_ichr || !d_qs || !d_qe || !d_bits)) ||
        (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) {
        snprintf(g_err, sizeof g_err, "igd_hip_membership_dev: bad argument (batch limit %lld queries)", (long long)max_batch());
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0) return IGD_HIP_OK;
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = stream ? (hipStream_t)stream : db->stream;
    const int64_t nF = db->nFiles, nW = (nF + 31) / 32;
    if (nF == 0) {                                       // rows of no words; every query meets no file
        if (d_nfiles_hit) HIPCHK(hipMemsetAsync(d_nfiles_hit, 0, (size_t)nq * 4, st));
        return IGD_HIP_OK;
    }
    const SliceImage im = slice_image(db, rule, v);
    const bool lds = nF <= IGD_MEMBER_LDS_FILES;
    const int grid = igd_hip_member_grid(nq);
    const size_t ldsB = (size_t)(4 + (lds ? (IGD_SETS_WG / IGD_WAVE) * nW : 0)) * 4;
    const int n = (int)nq;
    if (!lds) HIPCHK(hipMemsetAsync(d_bits, 0, (size_t)(nq * nW) * 4, st));        // the wide form ORs into zeroed rows
    with_flags(im.useV, lds, [&](auto V, auto L) {
        igd_member_rows<V(), L()><<<grid, IGD_SETS_WG, ldsB, st>>>(im.view, d_ichr, d_qs, d_qe, n, im.krule, v, d_bits, d_nfiles_hit, (u64 *)d_nhit);
    });
    HIPCHK(hipGetLastError());
    if (!lds && d_nfiles_hit) {
        igd_member_popc<<<grid, IGD_SETS_WG, 0, st>>>(d_bits, n, (int)nW, d_nfiles_hit);
        HIPCHK(hipGetLastError());
    }
    return IGD_HIP_OK;
}

static int ensure_member_ws(igd_hip_db *db, int64_t words, int64_t rows)
{
    int rc = dev_grow(db, &db->d_memBits, &db->memBitsCap, words);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_memNf, &db->memNfCap, rows);
    if (rc == IGD_HIP_OK && !db->d_memHit) rc = dalloc(&db->d_memHit, (size_t)1, nullptr);
    return rc;
}

extern "C" int igd_hip_membership(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                  int32_t v, int rule, uint32_t *bits, int32_t *nfiles_hit, int64_t *nhit)
{
    if (!db || nq < 0 || (nq > 0 && (!ichr || !qs || !qe || !bits)) || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) {
        snprintf(g_err, sizeof g_err, "igd_hip_membership: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0) return IGD_HIP_OK;
    const int64_t nF = db->nFiles, nW = (nF + 31) / 32;
    if (nF == 0) {
        if (nfiles_hit) memset(nfiles_hit, 0, (size_t)nq * 4);
        return IGD_HIP_OK;
    }
    // the hit counter is per chunk: zeroed before the launch, copied out behind it, and the chunks' counts are added once the
    // driver has waited for the last of them
    const int64_t step = chunk_step(member_row_bytes(), nW * 4);
    std::vector<unsigned long long> hs((size_t)((nq + step - 1) / step), 0);
    const int rc = run_region_chunks(db, ichr, qs, qe, nq, step, [&](int64_t c0, int64_t m, hipStream_t st) {
        int rc2 = ensure_member_ws(db, m * nW, m);
        if (rc2 != IGD_HIP_OK) return rc2;
        HIPCHK(hipMemsetAsync(db->d_memHit, 0, 8, st));
        rc2 = igd_hip_membership_dev(db, db->d_qc, db->d_qs, db->d_qe, m, v, rule, db->d_memBits, nfiles_hit ? db->d_memNf : nullptr,
                                     (int64_t *)db->d_memHit, st);
        if (rc2 != IGD_HIP_OK) return rc2;
        HIPCHK(hipMemcpyAsync(bits + c0 * nW, db->d_memBits, (size_t)(m * nW) * 4, hipMemcpyDeviceToHost, st));
        if (nfiles_hit) HIPCHK(hipMemcpyAsync(nfiles_hit + c0, db->d_memNf, (size_t)m * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&hs[(size_t)(c0 / step)], db->d_memHit, 8, hipMemcpyDeviceToHost, st));
        return IGD_HIP_OK;
    });
    if (rc != IGD_HIP_OK) return rc;
    if (nhit) for (unsigned long long h : hs) *nhit += (int64_t)h;
    return IGD_HIP_OK;
}
