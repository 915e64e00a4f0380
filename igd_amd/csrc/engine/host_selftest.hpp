// engine/host_selftest.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// TEST-ONLY: igd_hip_test_exclusive_scan / igd_hip_test_radix_sort_pairs, the two primitives of igd_sortscan.hpp on host
// arrays (the definitions are in include/igd_hip.h).  No handle: a stream and the arrays of one call, freed before it returns.
// ------------------------------------------------------------------------------------------
// The entries call the instantiations the rest of this file uses, exclusive_scan<uint32_t, int64_t> and radix_sort_pairs, and
// size every workspace exactly as the comment above radix_sort_pairs promises.  Every device array has IGD_SELFTEST_GUARD
// bytes of IGD_SELFTEST_FILL directly behind its last element; they are read back after the run, so a kernel that writes
// past a promised size fails the call instead of landing in a neighbour's padding.
#define IGD_SELFTEST_GUARD 256
#define IGD_SELFTEST_FILL 0xa5
#define IGD_SELFTEST_MAX ((int64_t)1 << 31)

struct SelfTest {
    struct Arr { const char *name; char *p; size_t bytes; };
    hipStream_t st = nullptr;
    Arr a[8];
    int na = 0;
    ~SelfTest()
    {
        for (int k = 0; k < na; k++) (void)hipFree(a[k].p);
        if (st) (void)hipStreamDestroy(st);
    }
    int open(const char *who, int device)
    {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
            snprintf(g_err, sizeof g_err, "%s: no HIP device", who);
            return IGD_HIP_ERR_DEVICE;
        }
        if (device < 0 || device >= ndev) {
            snprintf(g_err, sizeof g_err, "%s: device out of range", who);
            return IGD_HIP_ERR_ARG;
        }
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return IGD_HIP_OK;
    }
    // count elements of *p and the guard behind them
    template <typename T>
    int take(T **p, const char *name, int64_t count)
    {
        const size_t bytes = (size_t)count * sizeof(T);
        char *m = nullptr;
        HIPCHK(hipMalloc(&m, bytes + IGD_SELFTEST_GUARD));
        a[na++] = Arr{name, m, bytes};
        HIPCHK(hipMemsetAsync(m + bytes, IGD_SELFTEST_FILL, IGD_SELFTEST_GUARD, st));
        *p = (T *)m;
        return IGD_HIP_OK;
    }
    // waits for the stream; IGD_HIP_ERR_DEVICE naming the first array whose guard changed
    int check(const char *who)
    {
        unsigned char g[IGD_SELFTEST_GUARD];
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < na; k++) {
            HIPCHK(hipMemcpy(g, a[k].p + a[k].bytes, IGD_SELFTEST_GUARD, hipMemcpyDeviceToHost));
            for (int b = 0; b < IGD_SELFTEST_GUARD; b++)
                if (g[b] != IGD_SELFTEST_FILL) {
                    snprintf(g_err, sizeof g_err, "%s: byte %d behind the %zu bytes of %s was written", who, b, a[k].bytes, a[k].name);
                    return IGD_HIP_ERR_DEVICE;
                }
        }
        return IGD_HIP_OK;
    }
};

extern "C" int igd_hip_test_exclusive_scan(int device, const uint32_t *in, int64_t n, int64_t *out, int64_t *total)
{
    static const char who[] = "igd_hip_test_exclusive_scan";
    if (n < 0 || n > IGD_SELFTEST_MAX || !in || !out || !total) {
        snprintf(g_err, sizeof g_err, "%s: bad argument (0 .. 2^31 elements, no null array)", who);
        return IGD_HIP_ERR_ARG;
    }
    if (n == 0) { *total = 0; return IGD_HIP_OK; }
    SelfTest t;
    int rc = t.open(who, device);
    if (rc != IGD_HIP_OK) return rc;
    uint32_t *dIn = nullptr;
    int64_t *dOut = nullptr, *dSums = nullptr, *dTot = nullptr;
    if ((rc = t.take(&dIn, "in", n)) != IGD_HIP_OK || (rc = t.take(&dOut, "out", n)) != IGD_HIP_OK ||
        (rc = t.take(&dSums, "sums", (n + SCAN_TILE - 1) / SCAN_TILE + 1)) != IGD_HIP_OK || (rc = t.take(&dTot, "total", 1)) != IGD_HIP_OK)
        return rc;
    HIPCHK(hipMemcpyAsync(dIn, in, (size_t)n * 4, hipMemcpyHostToDevice, t.st));
    HIPCHK((exclusive_scan<uint32_t, int64_t>(dIn, n, dOut, dSums, dTot, t.st)));
    if ((rc = t.check(who)) != IGD_HIP_OK) return rc;
    HIPCHK(hipMemcpy(out, dOut, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(total, dTot, 8, hipMemcpyDeviceToHost));
    return IGD_HIP_OK;
}

extern "C" int igd_hip_test_radix_sort_pairs(int device, uint32_t *keys, uint32_t *vals, int64_t n, int bits)
{
    static const char who[] = "igd_hip_test_radix_sort_pairs";
    if (n < 0 || n > IGD_SELFTEST_MAX || !keys || !vals || bits < 0 || bits > 32) {
        snprintf(g_err, sizeof g_err, "%s: bad argument (0 .. 2^31 pairs, 0 .. 32 bits, no null array)", who);
        return IGD_HIP_ERR_ARG;
    }
    if (n == 0) return IGD_HIP_OK;
    SelfTest t;
    int rc = t.open(who, device);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nh = rs_blocks(n) * 256;
    uint32_t *kA = nullptr, *vA = nullptr, *kB = nullptr, *vB = nullptr, *hist = nullptr;
    int64_t *dig = nullptr, *sums = nullptr, *tot = nullptr;
    if ((rc = t.take(&kA, "keys", n)) != IGD_HIP_OK || (rc = t.take(&vA, "vals", n)) != IGD_HIP_OK ||
        (rc = t.take(&kB, "the second key buffer", n)) != IGD_HIP_OK || (rc = t.take(&vB, "the second value buffer", n)) != IGD_HIP_OK ||
        (rc = t.take(&hist, "hist", nh)) != IGD_HIP_OK || (rc = t.take(&dig, "digitBase", nh)) != IGD_HIP_OK ||
        (rc = t.take(&sums, "sums", (nh + SCAN_TILE - 1) / SCAN_TILE + 1)) != IGD_HIP_OK || (rc = t.take(&tot, "total", 1)) != IGD_HIP_OK)
        return rc;
    HIPCHK(hipMemcpyAsync(kA, keys, (size_t)n * 4, hipMemcpyHostToDevice, t.st));
    HIPCHK(hipMemcpyAsync(vA, vals, (size_t)n * 4, hipMemcpyHostToDevice, t.st));
    HIPCHK(radix_sort_pairs(&kA, &vA, &kB, &vB, n, bits, hist, dig, sums, tot, t.st));      // (kA / vA: where the sorted pairs are now)
    if ((rc = t.check(who)) != IGD_HIP_OK) return rc;
    HIPCHK(hipMemcpy(keys, kA, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(vals, vA, (size_t)n * 4, hipMemcpyDeviceToHost));
    return IGD_HIP_OK;
}
