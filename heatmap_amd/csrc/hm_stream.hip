/* Resident multi-zoom heatmap for streaming micro-batches (BASELINE config 5,
 * SURVEY.md 8f item 2).
 *
 * The reference recomputes its whole pyramid per Spark job (heatmap.py:152-158)
 * and keys every bin by user group and timespan label (heatmap.py:54-55,62-75).
 * A stream instead keeps every micro-batch's cells in HBM, log-structured:
 *
 *   bucket table  u64 keys {group u32 | period u32}, open addressing; a
 *                 bucket's id is its SLOT INDEX, so interning needs one CAS on
 *                 the key word and no value word.  Periods: an epoch hour
 *                 relative to the stream's base, "undated", or (rollup outputs)
 *                 a day / month / year / alltime label.
 *   cell log      {u64 key, u64 count} arrays: key = bucket << cb | cell, cell =
 *                 the pyramid index (4^z - 1)/3 + row * 2^z + col of a tile of
 *                 zoom z (cb bits: 43 at zmax 21).  A batch's count pass writes
 *                 its cells straight at the log's tail and k_stream_rekey adds
 *                 the bucket: ingest is an append (no hash-table probe per cell;
 *                 a 4 GB table insert took 0.4 ms per 10M-point batch).
 *
 * Per batch: k_stream_buckets interns each kept point's (group, hour) and
 * writes its bucket id; one count pass (hm_count when the batch has one
 * bucket, one per bucket for a few, else the grouped general path with the
 * bucket as group) writes the batch's cells at the tail.  Queries (rollups:
 * hour, day, month, year, alltime) relabel the log's cells to (group or all
 * groups, label) buckets (k_stream_relabel), sum equal keys with the bucketed
 * LDS merge (hm_cells_merge) and list them (k_stream_emit).  The log is
 * compacted (the same merge) when it fills up or its exact size is asked for.
 * A sliding window (hm_stream_window: the hours [lo, hi)) is one more relabel
 * rule on the same chain.  A viewport (hm_stream_view) swaps the relabel for
 * k_stream_view, which keeps only the cells inside a few rectangles, tested on
 * the key alone, so merge and emit see the viewport's cells, not the window's.
 * A raster (hm_stream_raster, k_stream_raster) is that filter followed by adds
 * into dense per-tile grids: equal cells meet in one bin, so nothing is merged.
 * Frames (hm_stream_raster_frames, k_stream_raster_frames) are the same pass
 * with each survivor sent to the grids of its own hour's frame.
 * A ranking (hm_stream_top) is a view whose merged cells go through the top-k
 * selection (hm_top.hip) before the emit, so k cells leave, not all of them;
 * a ranking of groups (hm_stream_top_groups) keys the survivors by group alone
 * (k_stream_view_groups) before the same merge and selection.
 * Distinct visitors (hm_stream_visitors) are a per-group view whose merged
 * (group, cell) records are folded once more, per cell, into points and a
 * count of groups (k_stream_visit_fold), and listed above a threshold
 * (k_stream_visit_emit): the k-anonymous cells of a selection.
 * Retention (hm_stream_expire, k_stream_expire)
 * filters the log into the alternate arrays and moves the surviving buckets
 * to a fresh bucket table, which frees the slots of the expired hours and of
 * every rollup label.  Forgetting (hm_stream_forget) is the same move for a
 * selection of (group, hour) buckets: k_stream_select judges every bucket slot
 * once and moves the buckets that stay, k_stream_forget filters the log through
 * the slot map it leaves; hm_stream_export_select lists the selected cells
 * instead (k_stream_export_select).  The state leaves and enters as cells: hm_stream_export
 * lists the compacted log with each cell's group and hour (k_stream_export,
 * one pass), hm_stream_import appends such cells at the tail under interned
 * buckets (k_stream_import: a snapshot restored, another stream merged in).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/heatmap_amd.h"
#include "hm_device.h"
#include "hm_pipeline.h"
#include "hm_table.h"
#include "hm_stream_dev.h"
#define HMS_SELECT_FN __device__ __forceinline__   /* hms_select_has on the device */
#include "hm_stream_select.h"
#define HM_VISIT_FN __device__ __forceinline__   /* hm_visit_judge on the device */
#include "hm_visit.h"

__device__ __forceinline__ uint64_t hms_pyr_off(int z) { return ((1ull << (2 * z)) - 1ull) / 3ull; }

/* hm_count key (zoom<<58 | row<<29 | col) -> pyramid cell index */
__device__ __forceinline__ uint64_t hms_cell(uint64_t k)
{
    const int z = (int)(k >> 58);
    const uint64_t r = (k >> 29) & 0x1FFFFFFFull, c = k & 0x1FFFFFFFull;
    return hms_pyr_off(z) + (r << z) + c;
}

__device__ __forceinline__ uint64_t hms_cell_key(uint64_t id, int zmin, int zmax)
{
    int z = zmin;
    while (z < zmax && id >= hms_pyr_off(z + 1)) z++;
    const uint64_t m = id - hms_pyr_off(z);
    return ((uint64_t)z << 58) | ((m >> z) << 29) | (m & ((1ull << z) - 1ull));
}

/* a bucket met by a wave: flagged with the batch epoch (a plain store -- the
 * waves of a batch start together, so a flag read-then-atomic would put
 * thousands of same-address atomics on one L2 channel); k_stream_collect
 * lists the flagged buckets afterwards */
__device__ __forceinline__ void hms_seen(const HmsBucketArgs& a, uint32_t b)
{
    if (b != HMS_NO_BUCKET && a.bflag[b] != a.epoch) a.bflag[b] = a.epoch;
}

/* Bucket of every kept point: (group or HMS_NOGROUP, hour - base or
 * HMS_UNDATED).  Each wave walks a contiguous range of the batch, HMS_WC
 * (key, bucket) pairs cached in registers (wave-uniform): a point whose key
 * is cached costs no probe and no atomic (a time-ordered batch is one key, a
 * batch of a few hours a few); a miss interns the key once for the wave
 * (ballot match) and evicts round-robin.  Also the list of the batch's
 * distinct buckets and their min/max.  Hours outside [base, base + 2^28) are
 * input errors (first index wins). */
#define HMS_WC 4
__global__ __launch_bounds__(256) void k_stream_buckets(HmsBucketArgs a)
{
    constexpr int U = 4;   /* points per lane per step, loads issued together */
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t per = ((a.n + waves - 1) / waves + 64 * U - 1) / (64 * U) * (64 * U);
    const uint64_t w0 = wave * per, w1 = min(w0 + per, a.n);
    uint32_t claimed = 0, full = 0;
    uint64_t ck[HMS_WC];
    uint32_t cb[HMS_WC];
#pragma unroll
    for (int c = 0; c < HMS_WC; c++) {
        ck[c] = HMS_EMPTY;
        cb[c] = HMS_NO_BUCKET;
    }
    uint32_t victim = 0;
    for (uint64_t i0 = w0; i0 < w1; i0 += 64 * U) {
        uint64_t key[U];
        bool kept[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = i0 + (uint64_t)u * 64 + lane;
            kept[u] = i < w1 && (!a.keep || a.keep[i]);
            const uint32_t h = (a.hour && i < w1) ? a.hour[i] : a.base;
            const uint32_t g = (a.group && i < w1) ? a.group[i] : HMS_NOGROUP;
            if (kept[u] && a.hour && (h < a.base || h - a.base >= HMS_MAX_HOUR_OFFSET)) {
                atomicMin(a.err_word, ((unsigned long long)i << 8) | (unsigned long long)HM_E_RANGE);
                kept[u] = false;
            }
            key[u] = ((uint64_t)g << 32) | (a.hour ? h - a.base : HMS_UNDATED);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            uint32_t mine = HMS_NO_BUCKET;
            bool hit = false;
#pragma unroll
            for (int c = 0; c < HMS_WC; c++)
                if (key[u] == ck[c]) {
                    mine = cb[c];
                    hit = true;
                }
            uint64_t pending = __ballot(kept[u] && !hit);
            while (pending) {
                const int leader = __ffsll((unsigned long long)pending) - 1;
                const uint64_t k0 = __shfl((unsigned long long)key[u], leader, 64);
                const uint64_t match = __ballot(kept[u] && key[u] == k0) & pending;
                uint32_t b = 0;
                if ((int)lane == leader) b = hms_intern(a.buckets, k0, &claimed);
                b = __shfl(b, leader, 64);
                if (lane == 0) hms_seen(a, b);
                full |= b == HMS_NO_BUCKET;
#pragma unroll
                for (int c = 0; c < HMS_WC; c++)
                    if (c == (int)victim) {
                        ck[c] = k0;
                        cb[c] = b;
                    }
                victim = (victim + 1) % HMS_WC;
                if ((match >> lane) & 1ull) mine = b;
                pending &= ~match;
            }
            const uint64_t i = i0 + (uint64_t)u * 64 + lane;
            if (kept[u] && a.out) a.out[i] = mine;
        }
    }
    const uint64_t cl = hms_wave_sum(claimed);
    if (lane == 0) {
        if (cl) atomicAdd(&a.state[HMS_ST_BUCKETS], (unsigned long long)cl);
        if (full) atomicAdd(&a.state[HMS_ST_BFULL], 1ull);
    }
}

/* the buckets flagged with this batch's epoch -> the batch's list (one
 * atomic per wave that finds any); HMS_ST_BMM receives one of them (THE one
 * when the batch has a single bucket) */
__global__ __launch_bounds__(256) void k_stream_collect(const uint32_t* __restrict__ bflag, uint64_t nb, uint32_t epoch,
                                                        uint32_t* __restrict__ list, unsigned long long* state)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63ull; i0 < nb; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool m = i < nb && bflag[i] == epoch;
        const uint64_t bal = __ballot(m);
        if (!bal) continue;
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(&state[HMS_ST_NLIST], (unsigned long long)__popcll(bal));
        first = __shfl(first, 0, 64);
        if (m) {
            list[first + hm_mbcnt(bal)] = (uint32_t)i;
            if (hm_mbcnt(bal) == 0) state[HMS_ST_BMM] = i;
        }
    }
}

/* the batch's distinct buckets -> their run index j (loc[bucket]) */
__global__ __launch_bounds__(256) void k_stream_batch_list(const uint32_t* __restrict__ list, uint32_t nlist,
                                                           uint32_t* __restrict__ loc)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nlist) loc[list[j]] = j;
}

/* points per run: the kept points of each of the batch's buckets, and (run
 * nparts) the points not kept; a block histogram over 4096-point chunks (a
 * thread's 16 bucket ids and keep bytes loaded before their run lookups),
 * one atomic per run */
__global__ __launch_bounds__(256) void k_stream_part_count(HmsScatterArgs a)
{
    __shared__ uint32_t h[HMS_MAX_PARTS + 1 + 64];
    const int tid = threadIdx.x;
    const uint32_t np = a.nparts + 1;
    if (tid < (int)np) h[tid] = 0;
    __syncthreads();
    const uint64_t chunk = 256 * 16;
    for (uint64_t c0 = (uint64_t)blockIdx.x * chunk; c0 < a.n; c0 += (uint64_t)gridDim.x * chunk) {
        uint32_t bid[16];
        bool kept[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint64_t i = c0 + (uint64_t)k * 256 + tid;
            bid[k] = i < a.n ? a.bids[i] : 0u;
            kept[k] = i < a.n && (!a.keep || a.keep[i]);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const bool in = c0 + (uint64_t)k * 256 + tid < a.n;
            const uint32_t part = in ? (kept[k] ? a.loc[bid[k]] : a.nparts) : 0u;
            hm_lds_count(h, HMS_MAX_PARTS + 1, part, in);
        }
    }
    __syncthreads();
    if (tid < (int)np && h[tid]) atomicAdd(&a.cursor[tid], (unsigned long long)h[tid]);
}

/* Gather a batch into bucket-contiguous runs (the partition path for batches
 * of a few buckets): run j = the kept points of the batch's j-th bucket, run
 * nparts = the points not kept (projected for their errors only).  Per block
 * chunk: LDS histogram, one global reservation per run, LDS slot claims. */
__global__ __launch_bounds__(256) void k_stream_scatter(HmsScatterArgs a)
{
    __shared__ uint32_t cur[HMS_MAX_PARTS + 1 + 64];   /* + 64 dummy words */
    __shared__ uint64_t base[HMS_MAX_PARTS + 1];
    const int tid = threadIdx.x;
    const uint32_t np = a.nparts + 1;
    const uint64_t chunk = 256 * 16;
    for (uint64_t c0 = (uint64_t)blockIdx.x * chunk; c0 < a.n; c0 += (uint64_t)gridDim.x * chunk) {
        if (tid < (int)np) cur[tid] = 0;
        __syncthreads();
        uint32_t part[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint64_t i = c0 + (uint64_t)k * 256 + tid;
            const bool in = i < a.n;
            const bool kept = in && (!a.keep || a.keep[i]);
            part[k] = in ? (kept ? a.loc[a.bids[i]] : a.nparts) : 0xFFFFFFFFu;
            hm_lds_count(cur, HMS_MAX_PARTS + 1, part[k], in);
        }
        __syncthreads();
        if (tid < (int)np) {
            const uint32_t c = cur[tid];
            base[tid] = a.start[tid] + (c ? atomicAdd(&a.cursor[tid], (unsigned long long)c) : 0ull);
            cur[tid] = 0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint64_t i = c0 + (uint64_t)k * 256 + tid;
            const bool in = i < a.n;
            const uint32_t pos = hm_lds_claim(cur, HMS_MAX_PARTS + 1, part[k], in);
            if (in) {
                const uint64_t q = base[part[k]] + pos;
                a.lat_out[q] = a.lat[i];
                a.lon_out[q] = a.lon[i];
            }
        }
        __syncthreads();
    }
}

/* hm_count keys of one bucket's cells -> cell-table keys, in place */
__global__ __launch_bounds__(256) void k_stream_rekey(uint64_t* __restrict__ keys, uint64_t m, uint64_t prefix)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride)
        keys[i] = prefix | hms_cell(keys[i]);
}

__global__ __launch_bounds__(256) void k_stream_rekey_dev(uint64_t* __restrict__ keys,
                                                          const unsigned long long* __restrict__ m_dev, uint64_t cap,
                                                          const unsigned long long* __restrict__ state, int cb)
{
    const uint64_t m = min((uint64_t)*m_dev, cap);
    const uint64_t prefix = state[HMS_ST_NLIST] ? (uint64_t)(uint32_t)state[HMS_ST_BMM] << cb : 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride)
        keys[i] = prefix | hms_cell(keys[i]);
}

/* grouped-path records (bucket, zoom, row, col, count) -> cell-table keys;
 * records of tiles outside [0, 2^z)^2 are counted, not converted */
__global__ __launch_bounds__(256) void k_stream_convert(const int64_t* __restrict__ rec, uint64_t m, int cb,
                                                        uint64_t* __restrict__ keys, uint64_t* __restrict__ counts,
                                                        unsigned long long* state)
{
    uint32_t bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const int64_t* r = rec + 5 * i;
        const int z = (int)r[1];
        const int64_t row = r[2], col = r[3];
        const bool in = row >= 0 && col >= 0 && row < (1ll << z) && col < (1ll << z);
        bad += !in;
        keys[i] = in ? ((uint64_t)r[0] << cb) | (hms_pyr_off(z) + ((uint64_t)row << z) + (uint64_t)col) : HMS_EMPTY;
        counts[i] = (uint64_t)r[4];
    }
    uint64_t v[1] = {bad};
    hms_block_sums(v);
    if (threadIdx.x == 0 && v[0]) atomicAdd(&state[HMS_ST_EXOTIC], (unsigned long long)v[0]);
}

__global__ __launch_bounds__(256) void k_stream_init(HmsTable t)
{
    const uint64_t n = t.mask + 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        ((ulonglong2*)t.slots)[i] = make_ulonglong2(HMS_EMPTY, 0ull);
}

__global__ __launch_bounds__(256) void k_stream_fill(uint64_t* p, uint64_t n, uint64_t v)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

/* days since 1970-01-01 -> (year, month 1..12): the proleptic Gregorian
 * civil-from-days conversion (400-year eras of 146097 days, March-based years) */
__device__ __forceinline__ void hms_civil(uint32_t days, uint32_t* y, uint32_t* m)
{
    const uint32_t z = days + 719468u;
    const uint32_t era = z / 146097u;
    const uint32_t doe = z - era * 146097u;
    const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
    const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
    const uint32_t mp = (5u * doy + 2u) / 153u;
    const uint32_t mm = mp < 10u ? mp + 3u : mp - 9u;
    *y = yoe + era * 400u + (mm <= 2u);
    *m = mm;
}

/* label period word of an hour bucket for a span; HMS_SKIP: not in the span */
__device__ __forceinline__ uint32_t hms_label(uint32_t pw, uint32_t base, int span)
{
    if (span == HM_SPAN_ALLTIME) return HMS_TYPE_ALLTIME << 28;
    if (pw == HMS_UNDATED) return HMS_SKIP;
    const uint32_t hour = base + pw;
    if (span == HM_SPAN_HOUR) return pw;
    const uint32_t day = hour / 24u;
    if (span == HM_SPAN_DAY) return (HMS_TYPE_DAY << 28) | day;
    uint32_t y, m;
    hms_civil(day, &y, &m);
    if (span == HM_SPAN_MONTH) return (HMS_TYPE_MONTH << 28) | (y * 12u + m - 1u);
    return (HMS_TYPE_YEAR << 28) | y;
}

/* the period a caller sees: epoch hour, days since 1970, year*12 + month-1, year, 0 */
__device__ __forceinline__ uint32_t hms_period_value(uint32_t pw, uint32_t base)
{
    const uint32_t type = pw >> 28;
    if (type == 0) return base + pw;
    if (type == HMS_TYPE_ALLTIME || type == HMS_TYPE_WINDOW) return 0;
    return pw & 0x0FFFFFFFu;
}

/* log key -> rollup label key (group or HMS_ALLGROUPS, label period word),
 * or ~0: not in the rollup */
__device__ __forceinline__ uint64_t hms_relabel_key(const HmsRelabelArgs& a, uint64_t k)
{
    const uint64_t bk = a.buckets.keys[k >> a.cb];
    const uint32_t pw = (uint32_t)bk;
    if ((pw >> 28) != 0 && pw != HMS_UNDATED) return ~0ull;   /* not a raw bucket (cannot happen) */
    /* a window: the dated hours [lo, hi) under one label per group (the label
     * is the scratch merge's id only, it does not carry the bounds) */
    const uint32_t lp = a.span == HMS_SPAN_WINDOW
                            ? ((pw != HMS_UNDATED && pw >= a.lo && pw < a.hi) ? HMS_TYPE_WINDOW << 28 : HMS_SKIP)
                            : hms_label(pw, a.base, a.span);
    if (lp == HMS_SKIP) return ~0ull;
    if (a.select >= 0 && (int64_t)hms_period_value(lp, a.base) != a.select) return ~0ull;
    const uint32_t g = a.merge ? HMS_ALLGROUPS : (uint32_t)(bk >> 32);
    return ((uint64_t)g << 32) | lp;
}

/* The log's cells of a rollup, re-keyed to their label buckets (interned) and
 * compacted: a block takes 256 * HMS_RL_PPT cells at a time, counts the ones
 * in the rollup, reserves their room with one atomic and writes them.  The
 * lanes sharing lane 0's label intern it once (a merged rollup is one label
 * per period); the rest probe alone. */
#define HMS_RL_PPT 32
__global__ __launch_bounds__(256) void k_stream_relabel(HmsRelabelArgs a)
{
    __shared__ uint32_t scr[256 / 64 + 1];
    __shared__ unsigned long long sbase;
    const int tid = threadIdx.x;
    const uint64_t cmask = (1ull << a.cb) - 1ull;
    uint32_t bclaimed = 0, full = 0;
    constexpr uint64_t CH = 256 * HMS_RL_PPT;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < a.n; c0 += (uint64_t)gridDim.x * CH) {
        uint32_t cnt = 0;
        for (int j = 0; j < HMS_RL_PPT; j++) {
            const uint64_t i = c0 + (uint64_t)j * 256 + tid;
            if (i < a.n) cnt += hms_relabel_key(a, a.keys[i]) != ~0ull;
        }
        uint32_t tot;
        uint32_t pos = hm_block_excl_scan<256>(cnt, scr, &tot);
        if (tid == 0) sbase = tot ? atomicAdd(a.cursor, (unsigned long long)tot) : 0ull;
        __syncthreads();
        const uint64_t base = sbase;
        __syncthreads();
        if (!tot) continue;
        for (int j = 0; j < HMS_RL_PPT; j++) {
            const uint64_t i = c0 + (uint64_t)j * 256 + tid;
            const uint64_t k = i < a.n ? a.keys[i] : 0ull;
            const uint64_t lk = i < a.n ? hms_relabel_key(a, k) : ~0ull;
            const bool in = lk != ~0ull;
            const uint64_t k0 = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(lk >> 32)) << 32) |
                                __builtin_amdgcn_readfirstlane((uint32_t)lk);
            const bool same = in & (lk == k0);
            const uint64_t sm = __ballot(same);
            uint32_t b = 0;
            if (sm && hm_lane() == 0) b = hms_intern(a.buckets, k0, &bclaimed);   /* lane 0 is in the group */
            b = __shfl(b, 0, 64);
            if (in && !same) b = hms_intern(a.buckets, lk, &bclaimed);
            if (in) {
                full |= b == HMS_NO_BUCKET;   /* the caller discards the rollup */
                const uint64_t q = base + pos++;
                a.keys_out[q] = ((uint64_t)(b == HMS_NO_BUCKET ? 0u : b) << a.cb) | (k & cmask);
                a.counts_out[q] = a.counts[i];
            }
        }
    }
    uint64_t v[2] = {bclaimed, full};
    hms_block_sums(v);
    if (tid == 0) {
        if (v[0]) atomicAdd(&a.state[HMS_ST_BUCKETS], (unsigned long long)v[0]);
        if (v[1]) atomicAdd(&a.state[HMS_ST_BFULL], (unsigned long long)v[1]);
    }
}

/* merged label cells -> (hm_count key, count, group, period) */
__global__ __launch_bounds__(256) void k_stream_emit(HmsEmitArgs a)
{
    const uint64_t cmask = (1ull << a.cb) - 1ull;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.n; j += stride) {
        const uint64_t k = a.keys[j];
        const uint64_t bk = a.buckets.keys[k >> a.cb];
        a.keys_out[j] = hms_cell_key(k & cmask, a.zmin, a.zmax);
        a.counts_out[j] = a.counts[j];
        if (a.groups_out) a.groups_out[j] = (uint32_t)(bk >> 32);
        if (a.periods_out) a.periods_out[j] = hms_period_value((uint32_t)bk, a.base);
    }
}

/* pyramid cell index -> hm_count key without the zoom search: the zoom is the
 * largest z with off(z) = (4^z - 1)/3 <= id, that is 4^z <= 3 id + 1 */
__device__ __forceinline__ uint64_t hms_cell_key_log(uint64_t id, int zmin, int zmax)
{
    const int z = min(max((63 - __clzll((long long)(3ull * id + 1ull))) >> 1, zmin), zmax);
    const uint64_t m = id - hms_pyr_off(z);
    return ((uint64_t)z << 58) | ((m >> z) << 29) | (m & ((1ull << z) - 1ull));
}

/* The export's one pass (hm_stream_export), over the log itself: its buckets
 * are raw, so a cell's bucket key is its group and its hour (periods_out: the
 * epoch hour, or HM_STREAM_UNDATED for an undated bucket).  A block takes
 * 256 * HMS_XP_U cells at a time; a thread issues the loads of its HMS_XP_U
 * keys and counts together, then the bucket-key lookups (two dependent loads
 * per cell, as k_stream_expire). */
#define HMS_XP_U 8
__global__ __launch_bounds__(256) void k_stream_export(HmsEmitArgs a)
{
    constexpr int U = HMS_XP_U;
    const int tid = threadIdx.x;
    const uint64_t cmask = (1ull << a.cb) - 1ull;
    constexpr uint64_t CH = 256 * U;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < a.n; c0 += (uint64_t)gridDim.x * CH) {
        uint64_t k[U], cn[U], bk[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            k[u] = i < a.n ? a.keys[i] : 0ull;
            cn[u] = i < a.n ? a.counts[i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < U; u++) bk[u] = a.buckets.keys[(k[u] >> a.cb) & a.buckets.mask];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            if (i >= a.n) continue;
            const uint32_t pw = (uint32_t)bk[u];
            a.keys_out[i] = hms_cell_key_log(k[u] & cmask, a.zmin, a.zmax);
            a.counts_out[i] = cn[u];
            if (a.groups_out) a.groups_out[i] = (uint32_t)(bk[u] >> 32);
            if (a.periods_out) a.periods_out[i] = pw == HMS_UNDATED ? HM_STREAM_UNDATED : a.base + pw;
        }
    }
}

/* A viewport query's filter: ONE pass over the log's keys.  A thread takes
 * HMS_VW_U keys at a time (their loads issued together) and tests each cell id
 * against the rectangles (HmsViewArgs: a few compares per rectangle on
 * wave-uniform bounds).  Most cells of a log fail and cost their 8-byte key
 * and nothing else; a wave none of whose cells lies in the rectangles' common
 * id interval skips even the rectangle loop.  Only the cells inside a
 * rectangle read their bucket's key (hour and group tests), only the
 * survivors their count.  A wave ranks its survivors by ballot and reserves
 * their room with one atomic per HMS_VW_U rows that hold any (the output
 * order is unspecified, so nothing is read twice); labels are interned as
 * k_stream_expire does, once per wave while the label stays the same. */
#ifndef HMS_VW_U
#define HMS_VW_U 8
#endif
__global__ __launch_bounds__(256) void k_stream_view(HmsViewArgs a)
{
    constexpr int U = HMS_VW_U;
    const int tid = threadIdx.x;
    const uint32_t lane = (uint32_t)tid & 63u;
    const uint64_t cmask = (1ull << a.cb) - 1ull;
    uint32_t bclaimed = 0, full = 0;
    uint64_t wk = HMS_EMPTY;          /* the wave's last shared label and its bucket */
    uint32_t wb = HMS_NO_BUCKET;
    constexpr uint64_t CH = 256 * U;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < a.n; c0 += (uint64_t)gridDim.x * CH) {
        uint64_t k[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            k[u] = i < a.n ? a.keys[i] : 0ull;
        }
        uint32_t box = 0;             /* bit u: cell u lies in the rectangles' common interval */
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            box |= (uint32_t)(i < a.n && (k[u] & cmask) - a.box_lo < a.box_span) << u;
        }
        if (!__ballot(box != 0)) continue;
        uint32_t hit = 0;             /* bit u: cell u lies in a rectangle */
        for (int r = 0; r < a.nrects; r++) {
            const HmsViewRect R = a.rects[r];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t d = (k[u] & cmask) - R.id_lo;
                hit |= (uint32_t)(d < R.span && ((uint32_t)d & R.cmask) - R.col_lo < R.col_w) << u;
            }
        }
        hit &= box;
        if (!__ballot(hit != 0)) continue;
        uint64_t lk[U], cn[U], bal[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            lk[u] = (hit >> u) & 1u ? hms_view_key(a, a.buckets.keys[(k[u] >> a.cb) & a.buckets.mask]) : ~0ull;
        uint32_t tot = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            cn[u] = lk[u] != ~0ull ? a.counts[i] : 0ull;
            bal[u] = __ballot(lk[u] != ~0ull);
            tot += (uint32_t)__popcll(bal[u]);
        }
        if (!tot) continue;
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(a.cursor, (unsigned long long)tot);
        uint64_t wq = __shfl(first, 0, 64);
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (!bal[u]) continue;
            const bool in = (bal[u] >> lane) & 1ull;
            const int leader = __ffsll((unsigned long long)bal[u]) - 1;
            const uint64_t k0 = __shfl((unsigned long long)lk[u], leader, 64);
            if (k0 != wk) {
                uint32_t b0 = 0;
                if ((int)lane == leader) b0 = hms_intern(a.buckets, k0, &bclaimed);
                wb = __shfl(b0, leader, 64);
                wk = k0;
            }
            uint32_t b = wb;
            if (in && lk[u] != k0) b = hms_intern(a.buckets, lk[u], &bclaimed);
            if (in) {
                full |= b == HMS_NO_BUCKET;   /* the caller discards the view */
                const uint64_t q = wq + hm_mbcnt(bal[u]);
                a.keys_out[q] = ((uint64_t)(b == HMS_NO_BUCKET ? 0u : b) << a.cb) | (k[u] & cmask);
                a.counts_out[q] = cn[u];
            }
            wq += (uint64_t)__popcll(bal[u]);
        }
    }
    uint64_t v[2] = {bclaimed, full};
    hms_block_sums(v);
    if (tid == 0) {
        if (v[0]) atomicAdd(&a.state[HMS_ST_BUCKETS], (unsigned long long)v[0]);
        if (v[1]) atomicAdd(&a.state[HMS_ST_BFULL], (unsigned long long)v[1]);
    }
}

/* A ranking of groups (hm_stream_top_groups): k_stream_view's filter -- the
 * same interval, rectangle and hour tests -- with every survivor keyed by its
 * group id alone (no label is interned, gmode is not read).  Survivors are many
 * and groups few, and the merge that follows takes a bucket of equal keys in
 * passes over all of it, so equal groups are summed before anything is
 * written: a wave row's survivors of one group across the wave (the first
 * HMS_VG_TURNS groups of a row; the others go on as they are), then those sums
 * in a table of the block's in LDS, written once when the block ends.  A sum
 * that finds no slot within HMS_VG_PROBES is written as a record of its own,
 * with one reservation per wave and chunk as k_stream_view's.  The merge sees
 * at most a record per (block, group) and those few. */
#define HMS_VG_TURNS 4
#define HMS_VG_SLOTS 2048
#define HMS_VG_PROBES 16
__global__ __launch_bounds__(256) void k_stream_view_groups(HmsViewArgs a)
{
    constexpr int U = HMS_VW_U;
    __shared__ uint32_t tg[HMS_VG_SLOTS];             /* group ids, HMS_ALLGROUPS: empty (no cell has that group) */
    __shared__ unsigned long long ts[HMS_VG_SLOTS];
    __shared__ uint32_t scr[256 / 64 + 1];
    __shared__ unsigned long long sbase;
    const int tid = threadIdx.x;
    const uint32_t lane = (uint32_t)tid & 63u;
    const uint64_t cmask = (1ull << a.cb) - 1ull;
    constexpr uint64_t CH = 256 * U;
    for (int j = tid; j < HMS_VG_SLOTS; j += 256) {
        tg[j] = HMS_ALLGROUPS;
        ts[j] = 0;
    }
    __syncthreads();
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < a.n; c0 += (uint64_t)gridDim.x * CH) {
        uint64_t k[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            k[u] = i < a.n ? a.keys[i] : 0ull;
        }
        uint32_t box = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            box |= (uint32_t)(i < a.n && (k[u] & cmask) - a.box_lo < a.box_span) << u;
        }
        if (!__ballot(box != 0)) continue;
        uint32_t hit = 0;
        for (int r = 0; r < a.nrects; r++) {
            const HmsViewRect R = a.rects[r];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t d = (k[u] & cmask) - R.id_lo;
                hit |= (uint32_t)(d < R.span && ((uint32_t)d & R.cmask) - R.col_lo < R.col_w) << u;
            }
        }
        hit &= box;
        if (!__ballot(hit != 0)) continue;
        uint32_t g[U];
        uint64_t sum[U], heads[U];    /* a group's first lane of the row holds its sum; heads: those lanes not in the table */
        uint32_t tot = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            bool in = (hit >> u) & 1u;
            g[u] = 0;
            if (in) {
                const uint64_t bk = a.buckets.keys[(k[u] >> a.cb) & a.buckets.mask];
                const uint32_t pw = (uint32_t)bk;
                const bool dated = (pw >> 28) == 0;
                in = a.alltime ? (dated || pw == HMS_UNDATED) : (dated && pw >= a.lo && pw < a.hi);
                g[u] = (uint32_t)(bk >> 32);
            }
            const uint64_t cn = in ? a.counts[i] : 0ull;
            uint64_t left = __ballot(in);
            sum[u] = 0, heads[u] = 0;
            for (int turn = 0; left; turn++) {   /* one turn per distinct group of the row */
                if (turn == HMS_VG_TURNS) {      /* many groups: the rest go out as they are */
                    if ((left >> lane) & 1ull) sum[u] = cn;
                    heads[u] |= left;
                    break;
                }
                const int leader = __ffsll((unsigned long long)left) - 1;
                const uint32_t g0 = __shfl(g[u], leader, 64);
                const bool mine = in && g[u] == g0;
                uint64_t t = mine ? cn : 0ull;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor((unsigned long long)t, d, 64);
                if ((int)lane == leader) sum[u] = t;
                heads[u] |= 1ull << leader;
                left &= ~__ballot(mine);
            }
            bool placed = false;
            if ((heads[u] >> lane) & 1ull) {
                uint32_t sl = (uint32_t)hms_hash(g[u]) & (HMS_VG_SLOTS - 1);
                for (int probe = 0; probe < HMS_VG_PROBES && !placed; probe++) {
                    const uint32_t o = atomicCAS(&tg[sl], HMS_ALLGROUPS, g[u]);
                    placed = o == HMS_ALLGROUPS || o == g[u];
                    if (placed) atomicAdd(&ts[sl], (unsigned long long)sum[u]);
                    sl = (sl + 1) & (HMS_VG_SLOTS - 1);
                }
            }
            heads[u] &= ~__ballot(placed);
            tot += (uint32_t)__popcll(heads[u]);
        }
        if (!tot) continue;
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(a.cursor, (unsigned long long)tot);
        uint64_t wq = __shfl(first, 0, 64);
#pragma unroll
        for (int u = 0; u < U; u++) {
            if ((heads[u] >> lane) & 1ull) {
                const uint64_t q = wq + hm_mbcnt(heads[u]);
                a.keys_out[q] = g[u];
                a.counts_out[q] = sum[u];
            }
            wq += (uint64_t)__popcll(heads[u]);
        }
    }
    /* the block's table: its sums out, one reservation */
    __syncthreads();
    constexpr int SPT = HMS_VG_SLOTS / 256;
    uint32_t c = 0;
    for (int j = 0; j < SPT; j++) c += tg[tid * SPT + j] != HMS_ALLGROUPS;
    uint32_t total;
    uint32_t off = hm_block_excl_scan<256>(c, scr, &total);
    const unsigned long long base = hm_block_reserve(a.cursor, total, &sbase);
    for (int j = 0; j < SPT; j++) {
        const uint32_t sl = tid * SPT + j;
        if (tg[sl] != HMS_ALLGROUPS) {
            a.keys_out[base + off] = tg[sl];
            a.counts_out[base + off] = ts[sl];
            off++;
        }
    }
}

/* Distinct visitors per cell (hm_stream_visitors), the second fold: the view's
 * merged records are distinct (group label, cell) pairs, so a cell's visitors
 * are the records that name it and its points their counts' sum.  One pass,
 * a record per lane: the bucket bits are stripped, the cell is inserted into
 * the table and its slot (hms_insert_slot) indexes the visitors array beside
 * it.  A low-zoom cell is named by every group -- the whole of zoom 0 is one
 * slot -- so the equal cells of a wave row are summed before the table is
 * touched: the first HMS_VF_TURNS distinct cells of a row each cost one probe
 * and one atomic pair for all their lanes (a turn that finds its cell on one
 * lane only reduces nothing), the others go on as they are. */
#define HMS_VF_TURNS 4
__global__ __launch_bounds__(256) void k_stream_visit_fold(HmsVisitArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t cmask = (1ull << a.cb) - 1ull;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;   /* a multiple of 64: i0 is wave-uniform */
    uint32_t overflow = 0;
    for (uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63ull; i0 < a.n; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool in = i < a.n;
        const uint64_t cell = in ? a.keys[i] & cmask : 0ull;
        uint64_t pts = in ? a.counts[i] : 0ull;
        uint32_t vis = in ? 1u : 0u;
        bool head = in;               /* this lane inserts (pts, vis) */
        uint64_t left = __ballot(in);
        for (int turn = 0; turn < HMS_VF_TURNS && left; turn++) {
            const int leader = __ffsll((unsigned long long)left) - 1;
            const uint64_t c0 = __shfl((unsigned long long)cell, leader, 64);
            const bool mine = ((left >> lane) & 1ull) && cell == c0;
            const uint64_t m = __ballot(mine);
            if (__popcll(m) > 1) {    /* (wave-uniform) */
                uint64_t t = mine ? pts : 0ull;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor((unsigned long long)t, d, 64);
                if ((int)lane == leader) {
                    pts = t;
                    vis = (uint32_t)__popcll(m);
                } else if (mine) {
                    head = false;
                }
            }
            left &= ~m;
        }
        if (head) {
            const uint64_t slot = hms_insert_slot(a.table, cell, pts, &overflow);
            if (slot != ~0ull) atomicAdd(&a.visitors[slot], vis);
        }
    }
    const uint64_t of = hms_wave_sum(overflow);   /* cannot happen: the table has twice the records' slots */
    if (lane == 0 && of) atomicAdd(&a.table.state[HMS_ST_OVERFLOW], (unsigned long long)of);
}

/* The threshold and the emit: the table swept in k_table_extract's manner.  A
 * block takes 256 * HMS_VE_U slots at a time (their loads and their visitors'
 * issued together), judges the occupied ones (hm_visit_judge), counts the
 * emitted (one block scan, one atomic on the cursor per chunk that holds any)
 * and ranks them row by row; those that land below `capacity` are written as
 * (HM_KEY, points, visitors).  The cursor counts every emitted cell, so one
 * launch gives the records and the size a larger call needs.  The withheld
 * cells and points are summed per thread and leave as one atomic pair per
 * block. */
#define HMS_VE_U 8
__global__ __launch_bounds__(256) void k_stream_visit_emit(HmsVisitArgs a)
{
    constexpr int U = HMS_VE_U;
    __shared__ uint32_t scr[256 / 64 + 1];
    __shared__ unsigned long long sbase;
    const int tid = threadIdx.x;
    const ulonglong2* slots = (const ulonglong2*)a.table.slots;
    const uint64_t ns = a.table.mask + 1;
    HmVisitWithheld wh = {0, 0};
    constexpr uint64_t CH = 256 * U;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < ns; c0 += (uint64_t)gridDim.x * CH) {
        ulonglong2 sl[U];
        uint32_t v[U];
        bool sel[U];
        uint32_t cnt = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            sl[u] = i < ns ? slots[i] : make_ulonglong2(HMS_EMPTY, 0ull);
            v[u] = i < ns ? a.visitors[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            sel[u] = sl[u].x != HMS_EMPTY && hm_visit_judge(&wh, v[u], sl[u].y, a.min_visitors);
            cnt += sel[u];
        }
        uint32_t tot;
        const uint32_t pos = hm_block_excl_scan<256>(cnt, scr, &tot);
        if (tid == 0) sbase = tot ? atomicAdd(a.cursor, (unsigned long long)tot) : 0ull;
        __syncthreads();
        uint64_t wq = sbase + __shfl(pos, 0, 64);
        __syncthreads();
        if (!tot || wq >= a.capacity) continue;   /* (wave-uniform; no barrier below) */
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t inb = __ballot(sel[u]);
            const uint64_t q = wq + hm_mbcnt(inb);
            wq += (uint64_t)__popcll(inb);
            if (sel[u] && q < a.capacity) {
                a.keys_out[q] = hms_cell_key_log(sl[u].x, a.zmin, a.zmax);
                a.points_out[q] = sl[u].y;
                if (a.visitors_out) a.visitors_out[q] = v[u];
            }
        }
    }
    uint64_t w[2] = {wh.cells, wh.points};
    hms_block_sums(w);
    if (tid == 0 && w[0]) {
        atomicAdd(&a.table.state[HMS_ST_WCELLS], (unsigned long long)w[0]);
        atomicAdd(&a.table.state[HMS_ST_WPOINTS], (unsigned long long)w[1]);
    }
}

/* is a raw bucket key inside a raster's hours and group */
__device__ __forceinline__ bool hms_raster_in(const HmsRasterArgs& a, uint64_t bk)
{
    const uint32_t pw = (uint32_t)bk, g = (uint32_t)(bk >> 32);
    const bool dated = (pw >> 28) == 0;
    const bool in = a.alltime ? (dated || pw == HMS_UNDATED) : (dated && pw >= a.lo && pw < a.hi);
    return in && (a.gmode != HMS_VIEW_GROUP || g == a.group);
}

/* A raster query: k_stream_view's filter (HMS_VW_U keys in flight, the common
 * interval test, a bucket read for the cells inside a rectangle only, a count
 * read for the survivors only) with nothing after it but the adds: equal cells
 * of different hours and groups land in the same bin, so there is no label,
 * no intern, no ranking and no cursor.  A cell is added to the grid of every
 * tile whose haloed square holds it (the rectangles of neighbour tiles
 * overlap by their halos; a repeated tile is its own grid), one non-returning
 * 64-bit atomic each; the survivors follow the viewport, not the log.
 *
 * FRAMES (hm_stream_raster_frames): the same pass with a time axis.  A
 * survivor's bucket key holds its hour, so its adds go to the grids of its own
 * frame, fstride elements apart: one more multiply-add on the address and,
 * for the survivors only, the division by the wave-uniform frame length (none
 * when that is 1 hour).  A frame is not a label, so still nothing is interned,
 * ranked or merged, and the adds of a screen spread over nframes times the
 * addresses. */
template <bool FRAMES>
__device__ __forceinline__ void hms_raster_pass(const HmsRasterArgs& a)
{
    constexpr int U = HMS_VW_U;
    const int tid = threadIdx.x;
    const uint64_t cmask = (1ull << a.cb) - 1ull;
    const uint32_t WW = a.W * a.W;
    constexpr uint64_t CH = 256 * U;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < a.n; c0 += (uint64_t)gridDim.x * CH) {
        uint64_t k[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            k[u] = i < a.n ? a.keys[i] : 0ull;
        }
        uint32_t box = 0;             /* bit u: cell u lies in the rectangles' common interval */
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            box |= (uint32_t)(i < a.n && (k[u] & cmask) - a.box_lo < a.box_span) << u;
        }
        if (!__ballot(box != 0)) continue;
        uint32_t hit = 0;             /* bit u: cell u lies in a rectangle */
        for (int r = 0; r < a.ntiles; r++) {
            const HmsRasterRect R = a.rects[r];
            const uint32_t zmask = (1u << R.z) - 1u;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t d = (k[u] & cmask) - R.id_lo;
                hit |= (uint32_t)(d < R.span && ((uint32_t)d & zmask) - R.col_lo < R.col_w) << u;
            }
        }
        hit &= box;
        if (!__ballot(hit != 0)) continue;
        uint32_t sel = 0;             /* bit u: ... of the wanted hours and group */
        uint32_t fr[U];               /* FRAMES: a survivor's frame, counted from the first clamped hour's */
#pragma unroll
        for (int u = 0; u < U; u++)
            if ((hit >> u) & 1u) {
                const uint64_t bk = a.buckets.keys[(k[u] >> a.cb) & a.buckets.mask];
                const bool in = hms_raster_in(a, bk);
                sel |= (uint32_t)in << u;
                if (FRAMES && in) {
                    const uint32_t x = (uint32_t)bk - a.lo + a.phase;
                    fr[u] = a.fh == 1 ? x : x / a.fh;
                }
            }
        if (!__ballot(sel != 0)) continue;
        uint64_t cn[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            cn[u] = (sel >> u) & 1u ? a.counts[i] : 0ull;
        }
        for (int r = 0; r < a.ntiles; r++) {
            const HmsRasterRect R = a.rects[r];
            const uint32_t zmask = (1u << R.z) - 1u;
            unsigned long long* g = a.grid + (uint64_t)r * WW;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t d = (k[u] & cmask) - R.id_lo;
                const uint32_t c = ((uint32_t)d & zmask) - R.col_lo;
                if (((sel >> u) & 1u) && d < R.span && c < R.col_w)
                    atomicAdd(&g[(FRAMES ? (uint64_t)fr[u] * a.fstride : 0ull) +
                                 ((uint32_t)(d >> R.z) + R.y0) * a.W + c + R.x0],
                              (unsigned long long)cn[u]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_stream_raster(HmsRasterArgs a) { hms_raster_pass<false>(a); }
__global__ __launch_bounds__(256) void k_stream_raster_frames(HmsRasterArgs a) { hms_raster_pass<true>(a); }

/* old-table bucket key of a log cell when it outlives the cut (undated cells
 * have no time and always do), or ~0 */
__device__ __forceinline__ uint64_t hms_survivor_key(const HmsExpireArgs& a, uint64_t k)
{
    const uint64_t bk = a.old_buckets.keys[k >> a.cb];
    const uint32_t pw = (uint32_t)bk;
    return (pw == HMS_UNDATED || pw >= a.cut) ? bk : ~0ull;
}

/* Retention: one pass over the log that filters and re-keys at once.  The
 * cells that outlive the cut are compacted into the alternate arrays (the
 * block shape of k_stream_relabel: count per chunk, scan, one reservation
 * atomic, write) under the bucket their (group, period) key gets in a FRESH
 * table, so the slots of expired hours, and of every rollup label, are free
 * again afterwards.  Distinct keys stay distinct (the key -> new bucket map is
 * one to one), in any order.  A thread takes its HMS_RL_PPT cells HMS_EX_U at a time: the
 * keys' loads are issued together, then their bucket-key lookups (the pass is
 * two dependent loads per cell, so one cell at a time it runs at their
 * latency). */
#define HMS_EX_U 8
__global__ __launch_bounds__(256) void k_stream_expire(HmsExpireArgs a)
{
    __shared__ uint32_t scr[256 / 64 + 1];
    __shared__ unsigned long long sbase;
    const int tid = threadIdx.x;
    const uint64_t cmask = (1ull << a.cb) - 1ull;
    uint32_t bclaimed = 0, full = 0;
    uint64_t wk = HMS_EMPTY;          /* the wave's last shared key and its new bucket */
    uint32_t wb = HMS_NO_BUCKET;
    constexpr uint64_t CH = 256 * HMS_RL_PPT;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < a.n; c0 += (uint64_t)gridDim.x * CH) {
        uint32_t cnt = 0;
        for (int j0 = 0; j0 < HMS_RL_PPT; j0 += HMS_EX_U) {
            uint64_t k[HMS_EX_U];
#pragma unroll
            for (int u = 0; u < HMS_EX_U; u++) {
                const uint64_t i = c0 + (uint64_t)(j0 + u) * 256 + tid;
                k[u] = i < a.n ? a.keys[i] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < HMS_EX_U; u++) {
                const uint64_t i = c0 + (uint64_t)(j0 + u) * 256 + tid;
                if (i < a.n) cnt += hms_survivor_key(a, k[u]) != ~0ull;
            }
        }
        uint32_t tot;
        const uint32_t pos = hm_block_excl_scan<256>(cnt, scr, &tot);
        if (tid == 0) sbase = tot ? atomicAdd(a.cursor, (unsigned long long)tot) : 0ull;
        __syncthreads();
        /* a wave's survivors go out cell row by cell row (the lanes of one
         * load, ranked by ballot), so its stores are contiguous */
        uint64_t wq = sbase + __shfl(pos, 0, 64);
        __syncthreads();
        if (!tot) continue;
        for (int j0 = 0; j0 < HMS_RL_PPT; j0 += HMS_EX_U) {
            uint64_t k[HMS_EX_U], bk[HMS_EX_U], cn[HMS_EX_U];
#pragma unroll
            for (int u = 0; u < HMS_EX_U; u++) {
                const uint64_t i = c0 + (uint64_t)(j0 + u) * 256 + tid;
                k[u] = i < a.n ? a.keys[i] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < HMS_EX_U; u++) {
                const uint64_t i = c0 + (uint64_t)(j0 + u) * 256 + tid;
                bk[u] = i < a.n ? hms_survivor_key(a, k[u]) : ~0ull;
            }
#pragma unroll
            for (int u = 0; u < HMS_EX_U; u++) {
                const uint64_t i = c0 + (uint64_t)(j0 + u) * 256 + tid;
                cn[u] = bk[u] != ~0ull ? a.counts[i] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < HMS_EX_U; u++) {
                const bool in = bk[u] != ~0ull;
                const uint64_t inb = __ballot(in);
                const uint64_t k0 = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(bk[u] >> 32)) << 32) |
                                    __builtin_amdgcn_readfirstlane((uint32_t)bk[u]);
                const bool same = in & (bk[u] == k0);
                const uint64_t sm = __ballot(same);
                /* lane 0's key, interned once for the lanes that share it and
                 * remembered (wave-uniform): the log is in batch order, so runs
                 * of cells share a bucket and cost no probe at all */
                if (sm && k0 != wk) {
                    uint32_t b0 = 0;
                    if (hm_lane() == 0) b0 = hms_intern(a.new_buckets, k0, &bclaimed);   /* lane 0 is in the group */
                    wb = __shfl(b0, 0, 64);
                    wk = k0;
                }
                uint32_t b = wb;
                if (in && !same) b = hms_intern(a.new_buckets, bk[u], &bclaimed);
                if (in) {
                    full |= b == HMS_NO_BUCKET;   /* cannot happen: no more keys than the old table held */
                    const uint64_t q = wq + hm_mbcnt(inb);
                    a.keys_out[q] = ((uint64_t)(b == HMS_NO_BUCKET ? 0u : b) << a.cb) | (k[u] & cmask);
                    a.counts_out[q] = cn[u];
                }
                wq += (uint64_t)__popcll(inb);
            }
        }
    }
    uint64_t v[2] = {bclaimed, full};
    hms_block_sums(v);
    if (tid == 0) {
        if (v[0]) atomicAdd(&a.state[HMS_ST_BUCKETS], (unsigned long long)v[0]);
        if (v[1]) atomicAdd(&a.state[HMS_ST_BFULL], (unsigned long long)v[1]);
    }
}

/* A selection judged per bucket, not per cell (hm_stream_forget,
 * hm_stream_export_select): whether a cell is selected depends on its bucket's
 * (group, period) alone, so one thread per slot of the bucket table decodes the
 * key, tests the hours and finds the group among the sorted ids by binary
 * search (about 20 L2-resident steps at 2^20 ids), and the passes over the log
 * only gather the word written here.  Rollup labels hold no log cells and are
 * never selected.  For a forget the thread also moves its bucket, when that
 * stays, to the fresh table (distinct keys: one CAS each on its own word) and
 * leaves the new slot as the verdict, so the log pass needs no probe: every
 * unselected raw bucket is carried over, with or without cells in the log. */
__global__ __launch_bounds__(256) void k_stream_select(HmsSelectArgs a)
{
    const uint64_t nb = a.old_buckets.mask + 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t bclaimed = 0, full = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += stride) {
        const uint64_t bk = a.old_buckets.keys[i];
        const uint32_t pw = (uint32_t)bk, g = (uint32_t)(bk >> 32);
        const bool dated = (pw >> 28) == 0;
        const bool raw = bk != HMS_EMPTY && (dated || pw == HMS_UNDATED);
        const bool hours = a.alltime ? raw : (dated && pw >= a.lo && pw < a.hi);
        const bool sel = raw && hours && (!a.ids || hms_select_has(a.ids, a.nids, g));
        uint32_t r = HMS_DROP;
        if (!sel && !a.new_buckets.keys) r = 0;
        if (!sel && raw && a.new_buckets.keys) {
            r = hms_intern(a.new_buckets, bk, &bclaimed);
            full |= r == HMS_NO_BUCKET;   /* cannot happen: no more keys than the old table held */
        }
        a.remap[i] = r;
    }
    uint64_t v[2] = {bclaimed, full};
    hms_block_sums(v);
    if (threadIdx.x == 0) {
        if (v[0]) atomicAdd(&a.state[HMS_ST_BUCKETS], (unsigned long long)v[0]);
        if (v[1]) atomicAdd(&a.state[HMS_ST_BFULL], (unsigned long long)v[1]);
    }
}

/* Forgetting: k_stream_expire's pass (8192-cell chunks, HMS_FG_U keys in
 * flight per thread, count, one block scan, one reservation atomic, survivors
 * ranked by ballot row by row, the alternate arrays as target) with
 * k_stream_select's slot map as predicate and new bucket at once: one 4-byte
 * gather per cell, no probe, no remembered key.  The count pass leaves each
 * thread a bit per surviving cell, so the write pass loads only survivors. */
#define HMS_FG_U 8
__global__ __launch_bounds__(256) void k_stream_forget(HmsForgetArgs a)
{
    static_assert(HMS_RL_PPT <= 32, "a thread's survivors are one 32-bit mask");
    __shared__ uint32_t scr[256 / 64 + 1];
    __shared__ unsigned long long sbase;
    const int tid = threadIdx.x;
    const uint64_t cmask = (1ull << a.cb) - 1ull;
    constexpr uint64_t CH = 256 * HMS_RL_PPT;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < a.n; c0 += (uint64_t)gridDim.x * CH) {
        uint32_t live = 0;
        for (int j0 = 0; j0 < HMS_RL_PPT; j0 += HMS_FG_U) {
            uint64_t k[HMS_FG_U];
            uint32_t r[HMS_FG_U];
#pragma unroll
            for (int u = 0; u < HMS_FG_U; u++) {
                const uint64_t i = c0 + (uint64_t)(j0 + u) * 256 + tid;
                k[u] = i < a.n ? a.keys[i] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < HMS_FG_U; u++) {
                const uint64_t i = c0 + (uint64_t)(j0 + u) * 256 + tid;
                r[u] = i < a.n ? a.remap[(k[u] >> a.cb) & a.mask] : HMS_DROP;
            }
#pragma unroll
            for (int u = 0; u < HMS_FG_U; u++) live |= (uint32_t)(r[u] != HMS_DROP) << (j0 + u);
        }
        uint32_t tot;
        const uint32_t pos = hm_block_excl_scan<256>((uint32_t)__popc(live), scr, &tot);
        if (tid == 0) sbase = tot ? atomicAdd(a.cursor, (unsigned long long)tot) : 0ull;
        __syncthreads();
        uint64_t wq = sbase + __shfl(pos, 0, 64);
        __syncthreads();
        if (!tot) continue;
        for (int j0 = 0; j0 < HMS_RL_PPT; j0 += HMS_FG_U) {
            uint64_t k[HMS_FG_U], cn[HMS_FG_U];
            uint32_t r[HMS_FG_U];
#pragma unroll
            for (int u = 0; u < HMS_FG_U; u++) {
                const uint64_t i = c0 + (uint64_t)(j0 + u) * 256 + tid;
                const bool in = (live >> (j0 + u)) & 1u;   /* only cells below a.n are */
                k[u] = in ? a.keys[i] : 0ull;
                cn[u] = in ? a.counts[i] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < HMS_FG_U; u++) {
                const bool in = (live >> (j0 + u)) & 1u;
                r[u] = in ? a.remap[(k[u] >> a.cb) & a.mask] : HMS_DROP;
            }
#pragma unroll
            for (int u = 0; u < HMS_FG_U; u++) {
                const bool in = (live >> (j0 + u)) & 1u;
                const uint64_t inb = __ballot(in);
                if (in) {
                    const uint64_t q = wq + hm_mbcnt(inb);
                    a.keys_out[q] = ((uint64_t)r[u] << a.cb) | (k[u] & cmask);
                    a.counts_out[q] = cn[u];
                }
                wq += (uint64_t)__popcll(inb);
            }
        }
    }
}

/* The selective export's one pass (hm_stream_export_select): k_stream_export's
 * decoding behind a ballot-ranked compaction.  A block takes 256 * HMS_XS_U
 * cells at a time; a thread issues its keys' loads together, then the verdict
 * gathers; the selected cells are counted (one block scan, one atomic on the
 * cursor per chunk that holds any) and ranked row by row, and only those that
 * land below `capacity` read their count and bucket key and are written.  The
 * cursor counts every selected cell, so one launch gives the records and the
 * size a larger call needs. */
#define HMS_XS_U 8
__global__ __launch_bounds__(256) void k_stream_export_select(HmsExportSelArgs a)
{
    constexpr int U = HMS_XS_U;
    __shared__ uint32_t scr[256 / 64 + 1];
    __shared__ unsigned long long sbase;
    const HmsEmitArgs& e = a.e;
    const int tid = threadIdx.x;
    const uint64_t cmask = (1ull << e.cb) - 1ull;
    constexpr uint64_t CH = 256 * U;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < e.n; c0 += (uint64_t)gridDim.x * CH) {
        uint64_t k[U], q[U], cn[U], bk[U];
        bool sel[U];
        uint32_t cnt = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            k[u] = i < e.n ? e.keys[i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            sel[u] = i < e.n && a.verdict[(k[u] >> e.cb) & e.buckets.mask] == HMS_DROP;
            cnt += sel[u];
        }
        uint32_t tot;
        const uint32_t pos = hm_block_excl_scan<256>(cnt, scr, &tot);
        if (tid == 0) sbase = tot ? atomicAdd(a.cursor, (unsigned long long)tot) : 0ull;
        __syncthreads();
        uint64_t wq = sbase + __shfl(pos, 0, 64);
        __syncthreads();
        if (!tot || wq >= a.capacity) continue;   /* (wave-uniform; no barrier below) */
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t inb = __ballot(sel[u]);
            q[u] = wq + hm_mbcnt(inb);
            wq += (uint64_t)__popcll(inb);
            sel[u] = sel[u] && q[u] < a.capacity;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            cn[u] = sel[u] ? e.counts[i] : 0ull;
            bk[u] = sel[u] ? e.buckets.keys[(k[u] >> e.cb) & e.buckets.mask] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (!sel[u]) continue;
            const uint32_t pw = (uint32_t)bk[u];
            e.keys_out[q[u]] = hms_cell_key_log(k[u] & cmask, e.zmin, e.zmax);
            e.counts_out[q[u]] = cn[u];
            if (e.groups_out) e.groups_out[q[u]] = (uint32_t)(bk[u] >> 32);
            if (e.periods_out) e.periods_out[q[u]] = pw == HMS_UNDATED ? HM_STREAM_UNDATED : e.base + pw;
        }
    }
}

/* Import of pre-aggregated cells (hm_stream_import): cell i of the input goes
 * to the log's tail at position i under the bucket of its (group, hour), so
 * the stores are as coalesced as the loads and nothing is reserved.  A block
 * takes 256 * HMS_IM_U cells at a time (k_stream_expire's shape); a thread
 * issues the loads of its HMS_IM_U keys, groups and hours together, then the
 * counts.  Interning as k_stream_expire: the lanes sharing lane 0's (group,
 * hour) intern it once and the wave remembers it (an export of a time-ordered
 * stream is long runs of one bucket: no probe at all), the others probe alone.
 * Every bucket met is flagged with the import's epoch (k_stream_collect lists
 * them afterwards).  An invalid cell (zoom outside the stream's, row or col
 * outside the square, count 0, group 0xFFFFFFFF, hour outside the stream's) is
 * not written; the first one's index goes to HMS_ST_ERR and the caller drops
 * the tail. */
#define HMS_IM_U 8
__global__ __launch_bounds__(256) void k_stream_import(HmsImportArgs a)
{
    constexpr int U = HMS_IM_U;
    __shared__ unsigned long long sbad[256 / 64];
    const int tid = threadIdx.x;
    uint32_t bclaimed = 0, full = 0;
    uint64_t bad = ~0ull;             /* the first invalid cell this thread met */
    uint64_t wk = HMS_EMPTY;          /* the wave's last shared key and its bucket */
    uint32_t wb = HMS_NO_BUCKET;
    constexpr uint64_t CH = 256 * U;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < a.n; c0 += (uint64_t)gridDim.x * CH) {
        uint64_t k[U], cn[U];
        uint32_t g[U], h[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            k[u] = i < a.n ? a.keys[i] : 0ull;
            g[u] = (a.groups && i < a.n) ? a.groups[i] : HMS_NOGROUP;
            h[u] = (a.hours && i < a.n) ? a.hours[i] : HM_STREAM_UNDATED;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            cn[u] = i < a.n ? a.counts[i] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            const int z = (int)(k[u] >> 58);
            const uint64_t r = (k[u] >> 29) & 0x1FFFFFFFull, c = k[u] & 0x1FFFFFFFull;
            const bool dated = h[u] != HM_STREAM_UNDATED;
            const bool ok = i < a.n && z >= a.zmin && z <= a.zmax && (r >> z) == 0 && (c >> z) == 0 && cn[u] != 0 &&
                            g[u] != HMS_ALLGROUPS &&
                            (!dated || (h[u] >= a.base && h[u] - a.base < HMS_MAX_HOUR_OFFSET));
            if (i < a.n && !ok) bad = min(bad, i);
            const uint64_t bk = ok ? ((uint64_t)g[u] << 32) | (dated ? h[u] - a.base : HMS_UNDATED) : ~0ull;
            const uint64_t k0 = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(bk >> 32)) << 32) |
                                __builtin_amdgcn_readfirstlane((uint32_t)bk);
            const bool same = ok & (bk == k0);
            const uint64_t sm = __ballot(same);
            if (sm && k0 != wk) {
                uint32_t b0 = 0;
                if (hm_lane() == 0) {   /* lane 0 is in the group */
                    b0 = hms_intern(a.buckets, k0, &bclaimed);
                    if (b0 != HMS_NO_BUCKET && a.bflag[b0] != a.epoch) a.bflag[b0] = a.epoch;
                }
                wb = __shfl(b0, 0, 64);
                wk = k0;
            }
            uint32_t b = wb;
            if (ok && !same) {
                b = hms_intern(a.buckets, bk, &bclaimed);
                if (b != HMS_NO_BUCKET && a.bflag[b] != a.epoch) a.bflag[b] = a.epoch;
            }
            if (ok) {
                full |= b == HMS_NO_BUCKET;   /* the caller drops the tail */
                a.keys_out[i] = ((uint64_t)(b == HMS_NO_BUCKET ? 0u : b) << a.cb) | hms_cell(k[u]);
                a.counts_out[i] = cn[u];
            }
        }
    }
    uint64_t v[2] = {bclaimed, full};
    hms_block_sums(v);
    for (int o = 32; o > 0; o >>= 1) bad = min(bad, (uint64_t)__shfl_xor((unsigned long long)bad, o, 64));
    if ((tid & 63) == 0) sbad[tid >> 6] = bad;
    __syncthreads();
    if (tid == 0) {
        if (v[0]) atomicAdd(&a.state[HMS_ST_BUCKETS], (unsigned long long)v[0]);
        if (v[1]) atomicAdd(&a.state[HMS_ST_BFULL], (unsigned long long)v[1]);
        const unsigned long long m = min(min(sbad[0], sbad[1]), min(sbad[2], sbad[3]));
        if (m != ~0ull) atomicMin(&a.state[HMS_ST_ERR], (m << 8) | (unsigned long long)HM_E_ARG);
    }
}

/* the occupied slots of a bucket table, listed (one atomic per wave that
 * finds any) */
__global__ __launch_bounds__(256) void k_stream_occupied(HmsBuckets b, uint32_t* __restrict__ list,
                                                         unsigned long long* n)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nb = b.mask + 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63ull; i0 < nb; i0 += stride) {
        const uint64_t i = i0 + lane;
        const bool m = i < nb && b.keys[i] != HMS_EMPTY;
        const uint64_t bal = __ballot(m);
        if (!bal) continue;
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(n, (unsigned long long)__popcll(bal));
        first = __shfl(first, 0, 64);
        if (m) list[first + hm_mbcnt(bal)] = (uint32_t)i;
    }
}

static dim3 hms_grid(uint64_t n)
{
    uint64_t b = (n + 255) / 256;
    if (b > 2048) b = 2048;   /* 8 blocks per CU; one state atomic per block */
    return dim3((unsigned)(b ? b : 1));
}

/* The keys of the batch's first and last kept-looking points, interned by one
 * thread ahead of k_stream_buckets: a time-ordered batch brings a NEW hour, and
 * every wave of the main kernel would otherwise find it missing at once and
 * CAS the same key word (~5000 same-address atomics per 10M points, 55 us) */
__global__ void k_stream_prime(HmsBucketArgs a)
{
    if (threadIdx.x != 0 || !a.hour) return;
    uint32_t claimed = 0;
    for (int e = 0; e < 2; e++) {
        const uint64_t i = e ? a.n - 1 : 0;
        if (a.keep && !a.keep[i]) continue;
        const uint32_t h = a.hour[i];
        if (h < a.base || h - a.base >= HMS_MAX_HOUR_OFFSET) continue;   /* k_stream_buckets reports it */
        const uint32_t g = a.group ? a.group[i] : HMS_NOGROUP;
        hms_intern(a.buckets, ((uint64_t)g << 32) | (h - a.base), &claimed);
    }
    if (claimed) atomicAdd(&a.state[HMS_ST_BUCKETS], (unsigned long long)claimed);
}

void hm_launch_stream_buckets(hipStream_t s, const HmsBucketArgs& a)
{
    /* ~8+ steps of 256 points per wave: runs of one key stay in registers */
    uint64_t b = (a.n + 8192 - 1) / 8192;
    if (b > 2048) b = 2048;
    if (a.n && a.hour) hipLaunchKernelGGL(k_stream_prime, dim3(1), dim3(64), 0, s, a);
    if (a.n) hipLaunchKernelGGL(k_stream_buckets, dim3((unsigned)(b ? b : 1)), dim3(256), 0, s, a);
}

void hm_launch_stream_collect(hipStream_t s, const uint32_t* bflag, uint64_t nb, uint32_t epoch, uint32_t* list,
                              unsigned long long* state)
{
    uint64_t b = (nb + 4095) / 4096;
    if (b > 1024) b = 1024;
    hipLaunchKernelGGL(k_stream_collect, dim3((unsigned)(b ? b : 1)), dim3(256), 0, s, bflag, nb, epoch, list, state);
}

void hm_launch_stream_batch_list(hipStream_t s, const uint32_t* list, uint32_t nlist, uint32_t* loc)
{
    if (nlist) hipLaunchKernelGGL(k_stream_batch_list, dim3((nlist + 255) / 256), dim3(256), 0, s, list, nlist, loc);
}

void hm_launch_stream_part_count(hipStream_t s, const HmsScatterArgs& a)
{
    uint64_t b = (a.n + 4095) / 4096;
    if (b > 2048) b = 2048;
    if (a.n) hipLaunchKernelGGL(k_stream_part_count, dim3((unsigned)(b ? b : 1)), dim3(256), 0, s, a);
}

void hm_launch_stream_scatter(hipStream_t s, const HmsScatterArgs& a)
{
    uint64_t b = (a.n + 4095) / 4096;
    if (b > 2048) b = 2048;
    if (a.n) hipLaunchKernelGGL(k_stream_scatter, dim3((unsigned)(b ? b : 1)), dim3(256), 0, s, a);
}

void hm_launch_stream_rekey(hipStream_t s, uint64_t* keys, uint64_t m, uint64_t prefix)
{
    if (m) hipLaunchKernelGGL(k_stream_rekey, hms_grid(m), dim3(256), 0, s, keys, m, prefix);
}

void hm_launch_stream_rekey_dev(hipStream_t s, uint64_t* keys, const unsigned long long* m_dev, uint64_t cap,
                                const unsigned long long* state, int cb)
{
    if (cap) hipLaunchKernelGGL(k_stream_rekey_dev, dim3(1024), dim3(256), 0, s, keys, m_dev, cap, state, cb);
}

void hm_launch_stream_convert(hipStream_t s, const int64_t* rec, uint64_t m, int cb, uint64_t* keys, uint64_t* counts,
                              unsigned long long* state)
{
    if (m) hipLaunchKernelGGL(k_stream_convert, hms_grid(m), dim3(256), 0, s, rec, m, cb, keys, counts, state);
}

void hm_launch_stream_init(hipStream_t s, const HmsTable& t)
{
    hipLaunchKernelGGL(k_stream_init, hms_grid(t.mask + 1), dim3(256), 0, s, t);
}

void hm_launch_stream_fill(hipStream_t s, uint64_t* p, uint64_t n, uint64_t v)
{
    if (n) hipLaunchKernelGGL(k_stream_fill, hms_grid(n), dim3(256), 0, s, p, n, v);
}

void hm_launch_stream_relabel(hipStream_t s, const HmsRelabelArgs& a)
{
    const uint64_t chunks = (a.n + 256 * HMS_RL_PPT - 1) / (256 * HMS_RL_PPT);
    if (a.n) hipLaunchKernelGGL(k_stream_relabel, dim3((unsigned)(chunks < 1024 ? chunks : 1024)), dim3(256), 0, s, a);
}

void hm_launch_stream_emit(hipStream_t s, const HmsEmitArgs& a)
{
    if (a.n) hipLaunchKernelGGL(k_stream_emit, hms_grid(a.n), dim3(256), 0, s, a);
}

void hm_launch_stream_export(hipStream_t s, const HmsEmitArgs& a)
{
    const uint64_t chunks = (a.n + 256 * HMS_XP_U - 1) / (256 * HMS_XP_U);
    if (a.n) hipLaunchKernelGGL(k_stream_export, dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(256), 0, s, a);
}

void hm_launch_stream_view(hipStream_t s, const HmsViewArgs& a)
{
    const uint64_t chunks = (a.n + 256 * HMS_VW_U - 1) / (256 * HMS_VW_U);
    if (a.n) hipLaunchKernelGGL(k_stream_view, dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(256), 0, s, a);
}

void hm_launch_stream_view_groups(hipStream_t s, const HmsViewArgs& a)
{
    const uint64_t chunks = (a.n + 256 * HMS_VW_U - 1) / (256 * HMS_VW_U);
    if (a.n)
        hipLaunchKernelGGL(k_stream_view_groups, dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(256), 0, s, a);
}

void hm_launch_stream_visit_fold(hipStream_t s, const HmsVisitArgs& a)
{
    if (a.n) hipLaunchKernelGGL(k_stream_visit_fold, hms_grid(a.n), dim3(256), 0, s, a);
}

void hm_launch_stream_visit_emit(hipStream_t s, const HmsVisitArgs& a)
{
    const uint64_t chunks = (a.table.mask + 1 + 256 * HMS_VE_U - 1) / (256 * HMS_VE_U);
    hipLaunchKernelGGL(k_stream_visit_emit, dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(256), 0, s, a);
}

void hm_launch_stream_raster(hipStream_t s, const HmsRasterArgs& a)
{
    const uint64_t chunks = (a.n + 256 * HMS_VW_U - 1) / (256 * HMS_VW_U);
    if (a.n) hipLaunchKernelGGL(k_stream_raster, dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(256), 0, s, a);
}

void hm_launch_stream_raster_frames(hipStream_t s, const HmsRasterArgs& a)
{
    const uint64_t chunks = (a.n + 256 * HMS_VW_U - 1) / (256 * HMS_VW_U);
    if (a.n)
        hipLaunchKernelGGL(k_stream_raster_frames, dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(256), 0, s, a);
}

void hm_launch_stream_expire(hipStream_t s, const HmsExpireArgs& a)
{
    const uint64_t chunks = (a.n + 256 * HMS_RL_PPT - 1) / (256 * HMS_RL_PPT);
    if (a.n) hipLaunchKernelGGL(k_stream_expire, dim3((unsigned)(chunks < 1024 ? chunks : 1024)), dim3(256), 0, s, a);
}

void hm_launch_stream_select(hipStream_t s, const HmsSelectArgs& a)
{
    hipLaunchKernelGGL(k_stream_select, hms_grid(a.old_buckets.mask + 1), dim3(256), 0, s, a);
}

void hm_launch_stream_forget(hipStream_t s, const HmsForgetArgs& a)
{
    const uint64_t chunks = (a.n + 256 * HMS_RL_PPT - 1) / (256 * HMS_RL_PPT);
    if (a.n) hipLaunchKernelGGL(k_stream_forget, dim3((unsigned)(chunks < 1024 ? chunks : 1024)), dim3(256), 0, s, a);
}

void hm_launch_stream_export_select(hipStream_t s, const HmsExportSelArgs& a)
{
    const uint64_t chunks = (a.e.n + 256 * HMS_XS_U - 1) / (256 * HMS_XS_U);
    if (a.e.n)
        hipLaunchKernelGGL(k_stream_export_select, dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(256), 0, s, a);
}

void hm_launch_stream_import(hipStream_t s, const HmsImportArgs& a)
{
    const uint64_t chunks = (a.n + 256 * HMS_IM_U - 1) / (256 * HMS_IM_U);
    if (a.n) hipLaunchKernelGGL(k_stream_import, dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(256), 0, s, a);
}

void hm_launch_stream_occupied(hipStream_t s, const HmsBuckets& b, uint32_t* list, unsigned long long* n)
{
    uint64_t g = (b.mask + 1 + 4095) / 4096;
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(k_stream_occupied, dim3((unsigned)(g ? g : 1)), dim3(256), 0, s, b, list, n);
}
