/* Internal to the host side (not installed): what hm_api.cpp (context, arena,
 * the count driver, merges) and hm_stream_api.cpp (the streaming heatmap)
 * share.  Everything declared HM_INTERNAL is defined in hm_api.cpp and stays
 * out of the library's dynamic symbol table. */
#ifndef HM_CTX_H
#define HM_CTX_H

#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/heatmap_amd.h"
#include "hm_pipeline.h"

#define HM_INTERNAL __attribute__((visibility("hidden")))

struct HM_INTERNAL Buf {
    void* p = nullptr;
    size_t cap = 0;
};

/* per-call stage events: [0..4] stage boundaries, [5..] pairs around the
 * level >= 2 partition launches */
#define HM_NEV 12

#define HM_FALLBACK (-1)   /* internal status: this path cannot take the call, the caller's other path does */

struct hm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<Buf> bufs;
    unsigned long long* state = nullptr;      /* device: err, exotic count, slow, cursor, nslots, ... */
    unsigned long long* host_state = nullptr; /* pinned mirror */
    int last_levels = 0;                      /* partition levels of the last count (stats [7]) */
    uint32_t* host_aux = nullptr;             /* pinned: level-1 histogram / region sizes */
    int64_t last_err_index = -1;
    int last_err_kind = 0;
    int64_t last_slow = 0;
    double stage_us[9] = {0};              /* [8]: keys per aggregation work item (0: general path) */
    hipEvent_t ev[HM_NEV];
    /* plan-tuning knobs, read once from the environment at hm_ctx_create
     * (INTEGRATION.md): HM_SPREAD_MIN_KEYS, HM_RS_BIG_MIN */
    double spread_min_keys = 0;
    double spread_min_cold = 0;
    int sample_log2 = 18;              /* level-1 region sizing: ~2^sample_log2 sampled points */
    int debug_l1 = 0;                  /* HM_DEBUG_L1: report level-1 region overflows on stderr */
    int stage_timing = 1;              /* HM_STAGE_TIMING=0: no stage events (hm_last_stats stages read 0) */
    int contig = 1;                    /* HM_CONTIG=0: 3-level plans keep run-streaming at the last level */
    uint32_t ta_min = 16384;           /* HM_TA_MIN: smallest aggregation work item (keys) */
    uint32_t ta_items = 128;           /* HM_TA_ITEMS: items' worth of points a call must have before ta halves */
    /* a stream's tail cells: the count re-keys them under the batch's bucket
     * (read on the device from the stream state) before its last read-back */
    uint64_t* tail_keys = nullptr;
    const unsigned long long* tail_state = nullptr;
    int tail_cb = 0;
    int tail_done = 0;
    uint64_t rs_big_min = 0;
    /* hot tiles (hm_pipeline.h): HM_HOT=0 turns them off; a tile is hot with
     * >= 1/hot_inv_share of the sampled points and >= hot_min_keys estimated */
    int hot = 1;
    int hot_mid = 1;               /* HM_HOT_MID=0: no hot tiles in 3-level plans (zmax 19-21) */
    double hot_inv_share = 4096;   /* 2048 -> 4096: 291 -> 470 hot tiles on the bench cloud, -0.13 ms */
    double hot_min_keys = 65536;
    int run_shard_bits = -1;   /* HM_RUN_SHARD_BITS: level >= 2 run-counter shards (-1: by plan) */
};

enum {
    ST_ERR = 0,
    ST_XCOUNT = 1,
    ST_SLOW = 2,
    ST_CURSOR = 3,
    ST_NSLOTS = 4,
    ST_REDO = 5,
    ST_REDO_OUT = 6,
    ST_XCURSOR = 7,
    ST_OVERFLOW = 8,
    ST_NHOT = 9,          /* hot tiles of this call (k_hot_select; low 32 bits) */
    ST_L1TOTAL = 10,      /* level-1 regions' total capacity (k_l1_sizes) */
    ST_LTOT = 12,         /* 12..14: a partition level's run, key and bucket totals (its run scans),
                           * read back with the state in one copy */
    ST_COUNT = 16
};

/* named arena slots */
enum {
    B_KEYS_A, B_KEYS_B, B_RUNS_SH, B_FLAT_A, B_FLAT_B, B_EXCL_A, B_EXCL_B, B_CNT, B_SHOFF, B_NR, B_NRUNS,
    B_NKEYS, B_KEYBASE, B_VALS, B_PREFIX, B_PARTIAL, B_TOTAL, B_ROOT, B_REDO_IDX, B_REDO_ROWS, B_REDO_COLS,
    B_RUNBASE0,
    B_BK0 = B_RUNBASE0 + HM_MAX_LEVELS, /* 4 levels x 8 arrays */
    B_CHILD0 = B_BK0 + HM_MAX_LEVELS * 8,
    B_TOT0 = B_CHILD0 + HM_MAX_LEVELS,
    B_SLOTS = B_TOT0 + HM_MAX_LEVELS + 1,
    B_SLOTBKT, B_GSLOTS, B_SPCODES, B_DESC0,
    /* exotic list and the general path (hm_general.hip) */
    B_X_ROW = B_DESC0 + HM_MAX_LEVELS, B_X_COL, B_X_IDX, B_GEN_KA, B_GEN_KB, B_GEN_FLAG, B_GEN_IDX, B_GEN_C,
    B_GEN_KHA, B_GEN_KHB, B_GEN_HIST, B_GEN_ORAND, B_GL_GRP,
    B_L1_FILL, B_L1_RBASE, B_L1_RCAP, B_L1_HIST, B_L1_SMASK,
    B_RT_CNT, B_RT_OFF, B_MG_TABLE, B_MG_STATE, B_SEG, B_RS_BIG,
    B_HOT, B_HOT_COUNTS, B_HOT_PARENT, B_D2B, B_MB_CNT, B_MB_OFF, B_MB_KEYS, B_MB_COUNTS, B_MB_CNT2, B_MB_OFF2,
    B_MB_KEYS2, B_MB_COUNTS2, B_KEYS_C, B_HOT_FORCE, B_C2B, B_SEG2, B_CTOT, B_CBASE, B_CCUR, B_MG_PIECES,
    B_L1_SLOT,
    B_RS_B, B_RS_MX,   /* hm_raster_render: blurred counts, the two maxima */
    B_SEL_IDS, B_SEL_MAP,   /* a stream selection: the sorted group ids, the word per bucket slot */
    B_TOP_SCRATCH, B_TOP_KEYS, B_TOP_COUNTS,   /* cells_top: words, states and histograms; the collected records */
    B_COUNT
};

/* HM_OK, or HM_E_HIP with the error reported on stderr */
HM_INTERNAL int hip_fail(hipError_t e, const char* what);

#define HIPCHK(x)                                  \
    do {                                           \
        int _st = hip_fail((x), #x);               \
        if (_st != HM_OK) return _st;              \
    } while (0)

/* wait for the stream (HM_SYNC_SPIN_US > 0: poll that long first) */
HM_INTERNAL hipError_t hm_sync(hipStream_t s);

/* arena slot `slot` with room for `bytes`; arena_release: every slot freed
 * after an allocation failure, so the next call starts from an empty arena */
HM_INTERNAL int ensure(hm_ctx* c, int slot, size_t bytes, void** out);
HM_INTERNAL void arena_release(hm_ctx* c);

#define ENSURE(slot, bytes, ptr)                                         \
    do {                                                                 \
        void* _p = nullptr;                                              \
        int _st = ensure(ctx, (slot), (size_t)(bytes), &_p);             \
        if (_st != HM_OK) return _st;                                    \
        ptr = (decltype(ptr))_p;                                         \
    } while (0)

/* what the stream calls across the file boundary (defined in hm_api.cpp) */
HM_INTERNAL void ctx_copy_tuning(hm_ctx* d, const hm_ctx* c);
HM_INTERNAL int grouped_impl(hm_ctx* ctx, const double* lat, const double* lon, const int64_t* rows,
                             const int64_t* cols, const uint8_t* keep, const uint32_t* group, int64_t n, int zmin,
                             int zmax, int64_t* cells_out, int64_t capacity, int64_t* n_out, uint64_t* pkeys = nullptr,
                             uint64_t* pcounts = nullptr);
HM_INTERNAL int cells_merge(hm_ctx* ctx, const void* keys_in, const void* counts_in, int layout, int64_t n,
                            const int64_t* runs, int nruns, uint64_t* keys_out, uint64_t* counts_out, int64_t capacity,
                            int64_t* n_out);
/* the first min(n, k) of n device records in rank order (hm_cells_top without
 * its argument checks: n > 0, 1 <= k <= HM_TOP_MAX_K, outputs of min(n, k)
 * entries that do not overlap the inputs); asynchronous, no read-back */
HM_INTERNAL int cells_top(hm_ctx* ctx, const uint64_t* keys, const uint64_t* counts, int64_t n, int64_t k,
                          uint64_t* keys_out, uint64_t* counts_out);
HM_INTERNAL bool raster_args_ok(const int64_t* tiles, int ntiles, int bins_log2, int halo, int zlo, int zhi);

#endif
