// igd_hip.hip -- MI355X (gfx950 / CDNA4) overlap-search engine behind include/igd_hip.h.
//
// Replaces, for a whole batch of queries at once, the reference's per-query kernels
//   get_overlaps    /root/reference/src/igd_search.c:454-534   (rule NEST)
//   get_overlaps_v  /root/reference/src/igd_search.c:623-694   (rule FLAT, value>=v)
//   get_overlaps0   /root/reference/src/igd_search.c:30-112    (12-byte records)
//   get_overlaps_f1 /root/reference/src/igd_search.c:537-620   (enumeration)
// and the hits[] accumulator (:925, :491, :524, :654, :684).
//
// Design (DESIGN.md has the long form).  The reference walks queries and, per query, seeks
// a tile, bisects it for the last start<qe and scans backwards testing end>qs.  Here the
// loop is turned inside out so that BOTH sides stream:
//   1. group the queries by tile.  Two ways, chosen ON THE DEVICE per batch:
//      a. queries already ordered by (contig, start) -- what a position-sorted BED gives:
//         k_query_bounds finds, in one pass and without atomics, the first query of every
//         tile (firstQ[]), verifies the order and leaves per query its READY-MADE compare word for
//         its first tile (qw0) and, for the 6 % that reach into later tiles, one more word, compacted
//         per block of 1024 queries (later[]); the scan kernel then reads the words of tile t's
//         queries, and of those of the up-to-3 tiles before it that reach it, with the tile's
//         records (a merge join: both sides stream, nothing is computed per candidate);
//      b. any other order: every (query, visited tile) pair is grouped by tile id without global
//         atomics (k_split_local -> k_split_fine_a/_b: LDS counting in two levels);
//         these kernels return at once when (a) holds.
//      The NEST/FLAT visiting rule and the "first tile" notion live entirely in this step.
//   2. scan:   igd_scan_sorted (a) / igd_scan_tiles (b) -- one wavefront owns one <=320-record chunk
//      ("unit") of one tile at a time.  It loads the unit's records once, coalesced, into 5 register
//      slots (record r*64+lane) -- by default from a compact 6-byte tile-relative image
//      (k_pack_units) -- keeps two units in flight, and runs through the tile's queries 64 at a
//      time across the lanes.  Each slot has a summary word (component-wise max of its 64 record
//      words, kept in the unit's descriptor); the queries that pass against it -- one vector compare
//      for all 64 -- are broadcast with v_readlane one at a time, and per query and slot the test
//            lob <= start < qe  &&  end > qs  [&& value >= v]
//      (lob = tile start for a non-first tile: the reference's tS prefix skip, :510-511; the
//      upper bound start<qe is what its bisection computes, :479-487) is one packed 16-bit max,
//      one compare and one add-with-carry into a per-record hit count; the counts go into a
//      per-workgroup LDS copy of hits[] (privatised counters).  Tiles with >= 32 queries are counted
//      by ranks instead (two bisections per query/record: see "rank" at igd_scan_sorted).
//   3. flush/reduce: each workgroup stores its LDS counters to its own slab row with plain
//      coalesced stores; k_reduce_slabs sums the rows into the caller's int64 hits[].  The same
//      launch walks, on the exact arrays, the few queries the scan leaves out (more than
//      IGD_SHORT_TILES tiles long, or needing exact starts: see k_pack_units), and shares out over
//      all its waves the tiles that were listed as too heavy for the one wave that owns them
//      (heavy_bucket_body / heavy_sorted_body: the skew valves).
//   `-f` (igd_enum_queries: query-major, streamed out in chunks) and `-m` (igd_hitmap_tiles) are separate kernels on the exact arrays;
//   Seqpare `-s` (igd_hip_seqpare) = the `-f` kernel emitting similarities + radix sorts into the
//   greedy order (igd_sortscan.hpp) + a wave-per-group matching kernel (k_seq_greedy).
// No MFMA anywhere: this is integer compare + count, bound by HBM / VALU issue, not by math.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <vector>
#include <algorithm>
#include <thread>
#include <mutex>
#include <time.h>
#include <unistd.h>

#include "igd_hip.h"
#include "igd_sortscan.hpp"

#define IGD_WAVE 64
#ifndef IGD_SLOTS
#define IGD_SLOTS 5                          // register slots per array per lane
#endif
#define IGD_CHUNK (IGD_WAVE * IGD_SLOTS)     // records per work chunk (320)
#define IGD_SHORT_TILES 4                    // queries spanning more tiles take the long path
#ifndef IGD_WPE
#define IGD_WPE 8                            // scan kernel: waves per SIMD the register budget is cut for
#endif
#ifndef IGD_WG
#define IGD_WG 1024                          // threads per scan workgroup (16 waves; 2 workgroups per CU)
#endif
#define IGD_MAX_BATCH ((long long)IGD_HIP_MAX_BATCH_DEFAULT)   // queries per device batch (include/igd_hip.h)
#define IGD_SCAN_ITEMS 16                    // elements per thread in the tile scan
#define IGD_SCAN_BLOCK 256
#define IGD_SCAN_TILE (IGD_SCAN_ITEMS * IGD_SCAN_BLOCK)
#ifndef IGD_TAIL_WGS
#define IGD_TAIL_WGS 256                     // workgroups (IGD_TAIL_WG threads) of the batch's last launch: one per CU -- with the ~100 registers of the
                                             // long queries' four-deep walks a CU holds one anyway, and a second round of workgroups cost every batch 1 us
#endif
#ifndef IGD_TAIL_WG
#define IGD_TAIL_WG 1024                     // ... in workgroups of 16 waves: what the long queries' work counts in a workgroup's LDS
                                             // leaves it as one global atomic per dataset, and 2048 workgroups of 4 waves made 3.9 x 10^6 of those
#endif
#ifndef IGD_REDUCE_SPLIT
#define IGD_REDUCE_SPLIT 4                   // row shares per column block of 64 files in k_reduce_slabs = additions per hits[f] and batch
                                             // (1900 files, 32-bit rows, the kernel by rocprofv3: 7.3 us with 1 share, 5.3 with 2, 4.8 with 4, 4.6 with 8,
                                             // taken with the partial sums added up before the tail; 4 and 8 are within the run-to-run spread of each
                                             // other and give the same step; adding up after the tail: 5.2 with 4)
#endif
static_assert(IGD_REDUCE_SPLIT >= 1 && IGD_REDUCE_SPLIT <= 32 && (IGD_REDUCE_SPLIT & (IGD_REDUCE_SPLIT - 1)) == 0, "IGD_REDUCE_SPLIT: a power of two, 1 .. 32");
#define IGD_REDUCE_DEPTH (512 / (IGD_REDUCE_SPLIT * (IGD_TAIL_WG / IGD_WAVE)))   // rows a lane asks for at a time: all of a wave's, of a slab of 512
static_assert(IGD_REDUCE_DEPTH >= 1, "IGD_REDUCE_DEPTH: column_share's loop would not advance");
#define IGD_PIPE_EVENTS 16                   // profiling: launches whose whole pipeline (not just the scan kernel) is timed
#define IGD_WINDOW_FILES 10240
#define IGD_MAX_WINDOWS 16                   // passes over the files of a database with more files than LDS counters
#define IGD_LDS_HITS_MAX_BYTES (120 * 1024)   // + 37 KiB of rank-method areas (igd_scan_sorted) stays below 160 KiB

typedef unsigned long long u64;

// measurement builds (-D...; also IGD_D_EXP, scan_direct.hpp): section costing, WRONG counts (igd_hip_open refuses them
// unless IGD_HIP_ALLOW_EXP_BUILD=1).  The forms of the kernels that lost an A/B are gone; LABNOTES.md keeps their figures.
#ifndef IGD_EXP_NOMATCH
#define IGD_EXP_NOMATCH 0     // measurement only: load everything, compare nothing (wrong results)
#endif

#ifndef IGD_EXP
#define IGD_EXP 0      // measurement-only builds (bits 1..512 and 8192 give WRONG counts): 1 no LDS flush, 2 no per-query compares,
                       // 4 no compares at all, 8 no later-tile queries, 64/128/256 rank method without term B / the searches of
                       // term A / prefix sums, 512 later-tile queries found but not searched, 8192 k_query_bounds without the
                       // compaction of the later-tile words; 0x10000 / 0x20000 the last launch without heavy_sorted_body /
                       // far_units_body, 0x40000 / 0x80000 k_query_bounds without the firstQ[] fill / the head and tail fill,
                       // 0x100000 / 0x200000 the last launch without the exact walks / the coverage sums, 0x800000 k_query_bounds
                       // without the lpos[] stores of short gaps (all WRONG counts).  (The time-stamp builds of rounds 2-5 -- bits 32,
                       // 1024, 0x400000, 0x1000000 -- left the source in round 6; their results are in LABNOTES.md.)
#endif

// ------------------------------------------------------------------------------------------
// error plumbing
static thread_local char g_err[512] = "";
static void set_err(const char *what, hipError_t e, const char *file, int line)
{
    snprintf(g_err, sizeof g_err, "%s: %s (%s:%d)", what, hipGetErrorString(e), file, line);
}
#define HIPCHK(call)                                                          \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) {                                               \
            set_err(#call, e_, __FILE__, __LINE__);                           \
            return IGD_HIP_ERR_DEVICE;                                        \
        }                                                                     \
    } while (0)

extern "C" const char *igd_hip_last_error(void) { return g_err; }
extern "C" void igd_hip_set_error_(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); }   // igd_create.hip

extern "C" int igd_hip_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_err("hipGetDeviceCount", e, __FILE__, __LINE__);
        return 0;
    }
    return n;
}

// Queries per engine call of the HOST-buffer entry points (igd_hip_search*, igd_hip_enumerate*, igd_hip_seqpare*) and the
// step of the command line tool's loops over longer query files.  IGD_MAX_BATCH in production; the TEST-ONLY variable
// IGD_HIP_MAX_BATCH (read once per process) lowers it so that every multi-batch seam -- the loop of igd_hip_search_ex, the
// `-f` and `-s` loops of igd_cli_abi.c -- is crossed by ordinary small fixtures (tests/test_gpu_batches.py).
static int64_t max_batch(void)
{
    static const int64_t m = []() -> int64_t {
        return igd_hip_max_batch_rule(getenv("IGD_HIP_MAX_BATCH"));      // (include/igd_hip.h: shared with igd_hip_lazy.c)
    }();
    return m;
}
extern "C" int64_t igd_hip_max_batch(void) { return max_batch(); }

// What this library was compiled as: bits 0..23 = IGD_EXP, bit 24 = IGD_EXP_NOMATCH.  A build with any bit of
// IGD_HIP_BUILD_WRONG_COUNTS gives WRONG counts on purpose (measurement of kernel sections): igd_hip_open refuses to
// work in such a build unless IGD_HIP_ALLOW_EXP_BUILD=1 says the caller knows (tools/valu_ab.sh does).
#define IGD_EXP_WRONG_BITS (1 | 2 | 4 | 8 | 64 | 128 | 256 | 512 | 8192 | 0x10000 | 0x20000 | 0x40000 | 0x80000 | 0x100000 | 0x200000 | 0x800000)
extern "C" unsigned igd_hip_build_flags(void) { return ((unsigned)IGD_EXP & 0xffffffu) | (IGD_EXP_NOMATCH ? 1u << 24 : 0u); }
extern "C" unsigned igd_hip_build_wrong_counts(void);     // (defined behind the engine's parts: igd_scan_direct's measurement bits count too)

// ------------------------------------------------------------------------------------------
// device view of one database (passed to kernels by value)
// One unit of scan work: a chunk of <= IGD_CHUNK records of one tile (48 bytes, three dwordx4 loads).
// Every tile has at least one unit; an empty tile gets a placeholder with n == 0 so that the
// long queries that START in it still have an owner in the sorted path.
struct __attribute__((aligned(16))) Unit {
    int64_t off;      // index of the unit's first record in the SoA arrays
    int32_t tile;     // global tile id
    int32_t n;        // records in this unit
    int32_t jf;       // (j << 4) | flags; j = tile index inside its contig;
                      // flag bit 0: first unit of its tile; bit k (1..3): tile j-k of the contig is EMPTY
    uint32_t W[6];    // compact image: summary word of each 64-record slot (k_pack_units): the component-wise
                      // maximum of the slot's record words = (65535 - smallest s') | largest e' << 16
    int32_t pre;      // compact image: the unit's records that start BEFORE its tile (s' = 0) -- the first `pre` of it, the tile
                      // being ordered by start; a tile covered from end to end counts the others without looking at them
};
#define UNIT_J(u) ((u).jf >> 4)
#define UNIT_FLAGS(u) ((u).jf & 15)

struct SpTuple { int32_t t, s, e; };     // split path: one (tile, qs, qe) pair on its way to its tile: 12 bytes, one dwordx3 access

struct DbView {
    int32_t nbp, shift, nCtg, nT, nUnits, nFiles;
    const Unit *units;
    const int32_t *start, *end, *idx, *value;   // SoA over all records, file order (exact)
    // compact tile-relative image of the same records (6 bytes each), see k_pack_units:
    const uint32_t *pse;                        // s' | e' << 16
    const uint16_t *px;                         // idx
    const uint32_t *pxv;                        // idx | value << 16 (only when every value fits 16 bits)
    const int64_t *tileOff;                     // [nT+1] record offset of each tile
    const int32_t *tileCnt;                     // [nT]
    const int32_t *tileBd;                      // [nT] tile start coordinate j*nbp (INT_MIN for j==0)
    const int32_t *ctgBase;                     // [nCtg] global tile id of the contig's tile 0
    const int32_t *ctgNTile;                    // [nCtg]
    const int32_t *tileUnit0;                   // [nT+1] number of each tile's first unit
    int32_t *cov;                               // workspace: 4 sets of coverage difference arrays (IGD_COV_*)
    const uint32_t *tileBits;                   // [(nT + 31) / 32] bit t: tile t holds records (what the grouping of an unordered batch asks of tileCnt[], 32 tiles per word)
    const int4 *tileD;                          // [nT] per tile: the records that start in the NEXT tile, the contig, the tiles left in it (k_tile_desc; null: no DIRECT step)
    // A database whose file is bucketed with another tile width than the image likes (-b 11..13, 16..19) is searched over a
    // RE-TILED copy: the same records in tiles of 2^14 bp (igd_hip_db::inner).  Which records a query counts does not depend on
    // the tile width -- every record that overlaps it, once -- with two exceptions that are properties of the FILE's tiles: a
    // query whose first tile lies outside the contig's tiles counts nothing (:462), and under rule NEST neither does one whose
    // first tile is empty (:468).  vshift >= 0 marks such a copy: log2 of the file's tile width; rNTile / rBase / rEmpty describe
    // the file's tiles (per contig: their number and the number of the first one; one bit per tile: it holds no record).
    int32_t vshift;
    const int32_t *rNTile, *rBase;
    const uint32_t *rEmpty;
    int32_t fileLo;                             // scan kernels, WIN builds: the pass counts the files [fileLo, fileLo + nFiles) (see igd_hip_db::winN)
};

struct igd_hip_db {
    int device;
    int32_t nbp, gType, nCtg, nFiles, nT;
    int64_t nRec;
    DbView v;
    // owned device memory of the image
    int32_t *d_start, *d_end, *d_idx, *d_value;
    uint32_t *d_pse;
    uint16_t *d_px;
    uint32_t *d_pxv;
    bool packed, packedV;         // compact image usable (nbp<=32768, nFiles<=65536) / values fit int16
    int64_t *d_tileOff;
    int32_t *d_tileCnt, *d_tileBd, *d_ctgBase, *d_ctgNTile, *d_tileUnit0;
    int32_t *d_heavy;             // [IGD_HEAVY_MAX] tiles of the batch with more pairs than a wave should take alone
    int32_t *d_far;               // [nUnits + 1] units the lean build of igd_scan_sorted leaves to far_units_body
    Unit *d_units;
    int32_t nUnits;
    int64_t resident;
    int32_t *d_firstQ, *d_pairN;  // [nT+1] first query of each tile (sorted path); pair counts copy
    int32_t *d_lpos;              // [nT+1] lpos[]: entries of its later block before query firstQ[t] (k_query_bounds)
    int32_t *d_cov;               // coverage of long queries (IGD_COV_*): 4 sets (path x batch parity) of { diff[nT + 2], coarse[(nT >> IGD_COV_SHIFT) + 2] }
    bool covStale;                // a batch returned an error after its first kernel: clear d_cov before the next one
    igd_hip_db *inner;            // the re-tiled copy the counting searches run on (file bucketed with -b 11..13 / 16..19), else null
    uint32_t *d_rEmpty;           // ... and its bitmap of the FILE's empty tiles
    int vnest;                    // (set on a re-tiled copy by the call that forwards to it: rule NEST of that call)
    int32_t *d_runIchr;           // igd_hip_search_runs_dev: contig numbers written out for the batches the RUNS build does not take
    int64_t runCap;
    int32_t *d_qw;                // [wsQueries] per-query word of the merge join (k_query_bounds: qw0)
    int32_t *d_later;               // [wsQueries + 1088] later[]: later-tile words, compacted per later block (compact image only)
    int32_t *d_spill;             // [nT+1] epoch stamps: a query covers the tile as a later tile
    int ldsSorted;                // dynamic LDS of igd_scan_sorted: counters + the waves' rank-method areas
    int32_t maxTileCnt;           // records of the fullest tile
    int sbCap;                    // igd_scan_sorted, rank method: query starts of one tile a wave keeps in LDS
    int32_t *d_laterHdr;         // laterHdr[]: int2 per later block (entries, last tile covered as a later tile)
    int lbShift;                  // log2(queries per later block) of the batch in flight
    int lastMode, lastPacked;     // of the last batch (igd_hip_last_scan_kernel)
    int lastRank;                 // build of igd_scan_sorted the last batch launched: 0 lean, 1 full (igd_hip_last_batch_routes)
    int forceRank;                // IGD_HIP_RANK at open (tests): 0 lean build, 1 full build, -1 the engine decides
    int forceDirect;              // IGD_HIP_DIRECT at open (tests): 1 every batch under IGD_HIP_FLAG_SORTED that can takes the DIRECT step, 0 none, -1 the engine decides
    int4 *d_tileD;                // DbView::tileD
    uint32_t *d_tileBits;         // DbView::tileBits
    int ldsDirect;                // dynamic LDS of igd_scan_direct
    int lastDirect;               // the last batch took the DIRECT step (igd_hip_last_scan_kernel)
    bool bigImage;                // the compact image is addressed with per-unit 64-bit bases (>= 2^30 tile records; IGD_HIP_BIG=1 at open: tests)
    bool timing;                  // IGD_TIMING at open: no getenv on the per-batch path
    // IGD_HIP_SPLIT_NOSTAGE / _NOBITS / _NOREGION at open (tests): the split path's fallbacks for what does not fit LDS, taken
    // by small fixtures too -- the unstaged fine walk, tileCnt[] gathers (bits or contig tables too large), tuples stored one by one
    bool splitNoStage, splitNoBits, splitNoRegion;
    uint32_t *d_spTable;          // split path: [nWG][nCoarse] offset | count << 16
    SpTuple *d_spT;               // regions: the pairs of each k_split_local workgroup, grouped by coarse bucket
    uint32_t *d_spSub;            // piled-up buckets: [nCoarse][SPF_S][2^spShift] pairs per (bucket, share, tile), then bucketBase[nCoarse], bucketLong[nCoarse]
    int spShift, spCoarse;        // coarse bucket = tile >> spShift; spShift < 0: split path not applicable
    char *arena;                  // one hipMalloc holds the whole resident image (carved by dalloc)
    size_t arenaSize, arenaUsed;
    int32_t epoch;                // batch counter: device-side flags are compared against it
    int32_t promised;             // != 0: a batch was launched under IGD_HIP_FLAG_SORTED since the last igd_hip_sync
    // per-batch workspace
    int32_t *d_pairCnt, *d_pairPos, *d_blockSums;
    void *d_pairs;                // int2[cap*K] (or int4 for the enumerate path)
    int2 *d_long, *d_fix;         // exact-walk lists: bucket path / merge-join path
    int32_t *d_ctl;               // control words (CTL_*)
    int64_t wsQueries;            // capacity in queries (merge-join arrays)
    int64_t wsBucket;             // capacity in queries of the bucket-path structures
    int pairBytes;
    u64 *d_slab;
    int grid, ldsBytes;
    bool ldsHits;
    int winN, nWin;               // files per window / windows (1: the files fit the LDS counters, or there are too many for windows)
    // `-f` streaming workspace (created by the first enumeration, kept)
    int64_t *d_qcount, *d_qoff, *d_enumBsum;
    int64_t enumQCap, enumChunkCap;          // capacity in queries / overlaps per chunk buffer
    igd_hip_hit *d_enumOut[2], *h_enumPin[2];
    bool enumPinned;
    int hit8State, hit8Bits;                 // igd_hip_hit8 (8 bytes per overlap): 0 not looked at yet, 1 fits (hit8Bits = bits of idx), 2 does not
    hipStream_t copyStream;
    hipEvent_t evFill[2], evCopy[2];
    // host-API staging
    int32_t *d_qc, *d_qs, *d_qe;
    int64_t qcap;
    int64_t *d_hits, *d_total;
    // igd_hip_search_sets (host_sets.hpp): the rows and totals of one chunk of sets, the slice table of its small sets.  These and
    // the workspaces below only grow: dev_grow (host_common.hpp)
    int64_t *d_setRows, *d_setTot;
    int64_t setRowCap, setTotCap;
    struct SetSlice *d_setSlices;
    int64_t setSliceCap;
    // igd_hip_support_sets (host_support.hpp), databases too wide for the LDS form: the waves' bitmap stripes (words)
    unsigned *d_supBits;
    int64_t supBitsCap;
    // igd_hip_coverage_sets (host_coverage.hpp), databases too wide for the LDS form: the waves' frontier stripes (64-bit
    // words) and the last tag a launch has handed out
    unsigned long long *d_covFront;
    int64_t covFrontCap;
    unsigned long long covTag;
    // igd_hip_membership (host_member.hpp): the bit rows, nfiles_hit[] and the hit counter of one chunk of queries
    unsigned *d_memBits;
    int32_t *d_memNf;
    unsigned long long *d_memHit;
    int64_t memBitsCap, memNfCap;
    // igd_hip_fisher_tables / igd_hip_enrich_sets (host_enrich.hpp): the tables and results of one chunk of cells (64-bit words);
    // igd_hip_enrich_ranks (host_rank.hpp) uses the same words for its chunk of rows
    int64_t *d_fisher;
    int64_t fisherCap;
    // igd_hip_restrict_sets / igd_hip_enrich_restricted (host_restrict.hpp): the ordered universe (ustart, uend, pmax, perm), the
    // contig table and set offsets, the bit rows of one chunk of sets and their popcounts
    int32_t *d_rsUni, *d_rsTab, *d_rsSize;
    unsigned *d_rsBits;
    int64_t rsUniCap, rsTabCap, rsSizeCap, rsBitsCap;
    // igd_hip_cooccur / igd_hip_bits_transpose / igd_hip_bitrows_gram (host_cooccur.hpp): the bit columns of one chunk of regions,
    // the matrix, and the generic entries' resident copies of the caller's rows (64-bit words)
    u64 *d_coCols, *d_coMat, *d_coA, *d_coB;
    int64_t coColsCap, coMatCap, coACap, coBCap;
    // perm_place_upload (host_permute.hpp), for run_perm_chunks -- the three permutation nulls -- and igd_hip_permute_regions: the
    // call's regions and contig lengths (ichr, qs, qe, ctg_len), behind them the offsets of a shift call (host_shift.hpp) or the pool of a resampling call.  igd_hip_permute_support / igd_hip_perm_stats: observed with the
    // six statistics (64-bit words)
    int32_t *d_pmReg;
    long long *d_pmStat;
    int64_t pmRegCap, pmStatCap;
    // perm_place_upload under a workspace (the _ws entries): the table of one call, as 32-bit words -- w_off (int64[nctg + 1], in
    // front: 8-byte aligned), then w_start, w_len and w_pre
    int32_t *d_pmWs;
    int64_t pmWsCap;
    // run_set_groups (host_nearest.hpp), the driver of igd_hip_nearest_sets(_fused), igd_hip_nearest_hist, igd_hip_flank_reldist and
    // igd_hip_map_sets: the result matrices of one group of sets (64-bit words) and the slice table of one chunk.  One pair for
    // all of them: every user runs on `stream` and waits before it returns.  igd_hip_permute_nearest keeps its chunk's matrices
    // and its slice table here too
    int64_t *d_grpStat;
    struct SetSlice *d_grpSlices;
    int64_t grpStatCap, grpSliceCap;
    // igd_hip_nearest / igd_hip_nearest_sets (host_nearest.hpp), igd_hip_flank (host_flank.hpp): the distance rows and dmin[] of one
    // chunk of regions
    int32_t *d_nrDist, *d_nrMin;
    int64_t nrDistCap, nrMinCap;
    // igd_hip_nearest_hist: the edges on the device
    int32_t *d_nrEdges;
    int64_t nrEdgesCap;
    // igd_hip_map / igd_hip_map_sets (host_map.hpp): the count and agg rows of one chunk of regions
    int32_t *d_mpCount;
    int64_t *d_mpAgg;
    int64_t mpCountCap, mpAggCap;
    // igd_hip_merge_sets / _dev (host_merge.hpp): every array of one merge, carved from one allocation (bytes)
    char *d_merge;
    int64_t mergeCap;
    // igd_hip_permute_bp (host_permute_bp.hpp; grown in its prepare, carved in its count): the runs of one chunk of rows (m_ichr,
    // m_qs, m_qe), and its 64-bit words: the regular set offsets, the run offsets, dropped, set_bp and n_merged per row
    int32_t *d_pbRun;
    int64_t *d_pbWord;
    int64_t pbRunCap, pbWordCap;
    // igd_hip_group_support_sets (host_group_support.hpp): the grouping of one call, grp_off[nFiles + 1] then grp_idx (32-bit words)
    int32_t *d_gsTab;
    int64_t gsTabCap;
    // igd_hip_dataset_bp: the tiles of every contig as the file has them (host copy), the merged base pairs per dataset that
    // have been computed so far, one entry per (v, rule), and how often one was computed
    struct BpEntry { int32_t v; int rule; std::vector<int64_t> bp; };
    std::vector<int32_t> hNTile;
    std::vector<BpEntry> bpCache;
    int64_t bpComputed;
    hipStream_t stream;
    // profiling
    std::vector<hipEvent_t> ev;   // 4 per launch: pipeline start, scan start, scan stop, pipeline stop
    int evMax, evUsed;
    hipEvent_t evStart, evStop;   // set while a timed launch of a promised-sorted batch is being enqueued: the scan kernel's own dispatch is
                                  // bracketed by them (hipExtLaunchKernel), not two event packets around it
    int evEvery, evSeen;          // every evEvery-th launch is timed (igd_hip_profile_sampling)
    bool evOn;
};


// ------------------------------------------------------------------------------------------
// The engine is ONE translation unit (the kernels are templates over the same views and the host code
// instantiates them), kept in parts by subject; each part is included exactly once, in this order.
#include "engine/upload.hpp"          // AoS -> SoA transposes of the .igd records at open
#include "engine/query_bounds.hpp"    // tile arithmetic, k_query_bounds (queries grouped by tile, fix list, coverage differences), k_count_pairs
#include "engine/split.hpp"           // unordered batches: two-level split into tile buckets (k_split_local / k_split_fine*), scans, scatter
#include "engine/compact_image.hpp"   // k_pack_units: the 6-byte tile-relative image and its unit descriptors
#include "engine/scan_tiles.hpp"      // igd_scan_tiles (bucket path) and its skew valve
#include "engine/scan_sorted.hpp"     // igd_scan_sorted: the merge join (pairwise and rank builds) -- the dominant kernel
#include "engine/scan_direct.hpp"     // dense sorted batches without a per-query pre-pass: k_tile_bounds, igd_scan_direct
#include "engine/tail.hpp"            // exact walks, coverage, k_reduce_slabs (last launch of a batch), k_sum_hits
#include "engine/enumerate_dev.hpp"   // `-f` enumeration kernels
#include "engine/hitmap_dev.hpp"      // `-m` hit map kernel
#include "engine/batch_stats_dev.hpp" // instrumentation: terms of the algorithmic byte model
#include "engine/sets_dev.hpp"        // igd_sets_count: many small query sets in one launch, one hits[] row per set
#include "engine/support_dev.hpp"     // igd_sets_support: the same walk, counting each (query, file) pair once
#include "engine/group_support_dev.hpp" // igd_sets_group_support: the same walk, one bit and one counter per GROUP of datasets -- the union over a group's files
#include "engine/coverage_dev.hpp"    // igd_sets_coverage: the same walk, one frontier per (query, file): covered base pairs
#include "engine/member_dev.hpp"      // igd_member_rows: the same walk, one bit row per query: which files it overlaps
#include "engine/fisher_dev.hpp"      // igd_fisher_cells: one wave per 2x2 table, the hypergeometric tail in log space
#include "engine/rank_dev.hpp"        // igd_rank_rows: one workgroup per table row, bitonic sort per column: ranks and BH q-values
#include "engine/restrict_dev.hpp"    // igd_restrict_bits, igd_bits_support: sets restricted to a universe -- the interval join and the gather over member rows
#include "engine/cooccur_dev.hpp"     // igd_bits_transpose, igd_bitrows_gram: bit rows into bit columns, popcount Gram product -- dataset co-occurrence
#include "engine/permute_dev.hpp"     // igd_permute_regions, igd_perm_stats: shifted / shuffled region sets, column statistics of a row matrix -- permutation null
#include "engine/permute_ws_dev.hpp"  // igd_permute_workspace: the same launch, regions placed inside a workspace by two binary searches in a resident table
#include "engine/shift_dev.hpp"       // igd_shift_regions: the same launch, the set moved rigidly by each offset of a resident table -- local z-score
#include "engine/resample_dev.hpp"    // igd_resample_regions: the same launch, each output a pool region drawn without replacement by a keyed bijection -- resampling null
#include "engine/nearest_dev.hpp"     // igd_nearest_rows, igd_nearest_reduce, igd_nearest_hist: the same walk over a widened interval, one (signed) distance row per region -- nearest record per dataset
#include "engine/flank_dev.hpp"       // igd_flank_rows, igd_flank_reldist: the same walk with two minima per region and dataset -- the nearest record on each side, the relative-distance histogram
#include "engine/nearest_fused_dev.hpp" // igd_nearest_slices: the same walk and table, folded into per-slice LDS accumulators -- the set statistics without the rows
#include "engine/map_dev.hpp"         // igd_map_rows, igd_map_reduce: the same walk with the value words, count and sum / min / max rows per region -- values of the overlapping records
#include "engine/map_fused_dev.hpp"   // igd_map_slices: the same walk and tables, folded into per-slice LDS accumulators -- the set statistics of the values without the rows
#include "engine/merge_dev.hpp"       // igd_merge_*: region sets merged as `bedtools merge` -- sort keys, segmented maximum scan of the ends, run heads and compaction
#include "engine/permute_bp_dev.hpp"  // igd_merge_row_offsets, igd_merge_slices, igd_merge_row_bp: the merged runs handed to igd_sets_coverage on the device -- permutation null of base-pair overlap
#include "engine/host_open.hpp"       // handles: allocation, close, pinned buffers, re-tiled copy, igd_hip_open
#include "engine/host_search.hpp"     // workspaces, launches, igd_hip_search_dev / _runs_dev / _search / _search_ex, sync
#include "engine/host_group.hpp"      // device groups of one process: native RCCL all-reduce of hits[]
#include "engine/host_enumerate.hpp"  // `-f` on the host side: chunked, double-buffered
#include "engine/seqpare.hpp"         // Seqpare `-s`: kernels and host
#include "engine/host_misc.hpp"       // igd_hip_hitmap, igd_hip_batch_stats
#include "engine/host_common.hpp"     // shared by the parts below: dev_grow, stage_queries, chunk_step, push_slices, slice_image, sets_check, with_flags; the drivers run_region_chunks and run_set_chunks
#include "engine/host_sets.hpp"       // igd_hip_search_sets: chunks of sets, small ones sliced, large ones through the batch pipeline
#include "engine/host_support.hpp"    // igd_hip_support_sets: chunks of sets, all of them sliced
#include "engine/host_coverage.hpp"   // igd_hip_coverage_sets: chunks of sets, all of them sliced
#include "engine/host_member.hpp"     // igd_hip_membership / _dev: a body of run_region_chunks, chunks of queries within a row budget, one launch each
#include "engine/host_enrich.hpp"     // igd_hip_fisher_tables / igd_hip_enrich_sets: chunks of cells, one launch each
#include "engine/host_group_support.hpp" // igd_hip_group_support_sets / igd_hip_group_enrich_sets: the same chunks with rows of nGroups columns, the table resident
#include "engine/host_rank.hpp"       // igd_hip_enrich_ranks: chunks of whole rows, one launch each
#include "engine/host_restrict.hpp"   // igd_hip_restrict_sets / igd_hip_enrich_restricted: chunks of sets x chunks of the universe
#include "engine/host_cooccur.hpp"    // igd_hip_cooccur / igd_hip_bits_transpose / igd_hip_bitrows_gram: chunks of regions, rows stay resident
#include "engine/host_permute.hpp"    // igd_hip_permute_support / igd_hip_permute_regions / igd_hip_perm_stats: chunks of permutations, rows stay resident
#include "engine/host_shift.hpp"      // igd_hip_shift_support / igd_hip_shift_regions: run_perm_chunks with the shift placement, the rows copied home
#include "engine/host_nearest.hpp"    // igd_hip_nearest / _dev / _sets, _signed / _signed_dev / _hist: a body of run_region_chunks; run_set_groups, the group driver of every resident set statistic, and its chunk functors
#include "engine/host_flank.hpp"      // igd_hip_flank / _dev / _reldist: the same two drivers with two rows per region
#include "engine/host_permute_nearest.hpp" // igd_hip_nearest_sets_fused / igd_hip_permute_nearest: run_set_groups with one fused launch per chunk, the null distribution of the distance statistics
#include "engine/host_map.hpp"        // igd_hip_map / _dev / _sets: the same two drivers, the set statistics stay resident
#include "engine/host_permute_map.hpp" // igd_hip_map_sets_fused / igd_hip_permute_map: run_set_groups with one fused launch per chunk, the null distribution of the value statistics
#include "engine/host_merge.hpp"      // igd_hip_merge_sets / _dev, igd_hip_dataset_bp, igd_hip_jaccard_sets: device merge, merged base pairs per dataset, the intersection table
#include "engine/host_permute_bp.hpp" // igd_hip_permute_bp: chunks of permutations, merged and covered without a host copy in between
#include "engine/host_selftest.hpp"   // TEST-ONLY: igd_hip_test_exclusive_scan / igd_hip_test_radix_sort_pairs: igd_sortscan.hpp on host arrays, guard bytes behind every device array
#include "engine/measure.hpp"         // instrumentation: compulsory traffic, streaming rates of the box, launch profile
extern "C" unsigned igd_hip_build_wrong_counts(void)
{
    return (((unsigned)IGD_EXP) & (unsigned)IGD_EXP_WRONG_BITS) | (IGD_EXP_NOMATCH ? 1u << 24 : 0u) | ((IGD_D_EXP & 47) ? 1u << 25 : 0u);
}
