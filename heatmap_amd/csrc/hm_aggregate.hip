/* The final level of the count pipeline (see hm_pipeline.h for the path):
 * cell emission and the in-LDS pyramids, k_aggregate for dense buckets, the
 * small-bucket kernels (one wave per bucket) and the pooling of bucket
 * totals. */
#include <hip/hip_runtime.h>
#include <type_traits>
#include "hm_device.h"
#include "hm_pipeline.h"
#define HM_STAMP_MODES(m) ((m) == 5 || (m) == 7)
#include "hm_stamps.h"
#include "hm_runs.h"

/* ------------------------------------------------------------------------ */
/* emission helpers                                                          */
/* ------------------------------------------------------------------------ */

/* Emit the non-zero cells v[0..n) of zoom z: the row-major (2^lg)^2 block
 * whose corner tile at zoom z - lg is `prefix` (a coord).  All threads of the
 * block must call. */
template <typename T, int THREADS>
__device__ void hm_emit_level(const T* v, uint32_t n, int z, uint64_t prefix, int lg, const HmOut& o,
                              uint32_t* scr, unsigned long long* sbase)
{
    const uint32_t per = (n + THREADS - 1) / THREADS;
    const uint32_t i0 = threadIdx.x * per;
    const uint32_t i1 = min(i0 + per, n);
    uint32_t c = 0;
    for (uint32_t i = i0; i < i1; i++) c += v[i] != 0;
    uint32_t tot;
    uint32_t off = hm_block_excl_scan<THREADS>(c, scr, &tot);
    if (tot == 0) return;
    if (threadIdx.x == 0) *sbase = atomicAdd(o.cursor, (unsigned long long)tot);
    __syncthreads();
    const uint64_t base = *sbase;
    __syncthreads();
    for (uint32_t i = i0; i < i1; i++) {
        const T x = v[i];
        if (x != 0) {
            const uint64_t pos = base + off;
            if (pos < o.capacity) {
                o.keys[pos] = hm_cell_key(z, prefix, lg, i);
                o.counts[pos] = (uint64_t)x;
            }
            off++;
        }
    }
}

/* In-LDS 4:1 pyramid over the row-major v[0..4^lg): emits zooms z_top ..
 * z_top-lg+1 (those in [zmin, zmax]) and leaves the total in v[0]. */
template <typename T, int THREADS>
__device__ void hm_pyramid(T* v, int lg, int z_top, uint64_t prefix, const HmOut& o, uint32_t* scr,
                           unsigned long long* sbase)
{
    uint32_t n = 1u << (2 * lg);
    for (int k = 0; k < lg; k++) {
        const int z = z_top - k;
        if (z >= o.zmin && z <= o.zmax) hm_emit_level<T, THREADS>(v, n, z, prefix, lg - k, o, scr, sbase);
        __syncthreads();
        n >>= 2;
        constexpr int MAXPER = (HM_AG_CELLS / 4 + THREADS - 1) / THREADS;
        T acc[MAXPER];
#pragma unroll
        for (int m = 0; m < MAXPER; m++) {
            const uint32_t i = threadIdx.x + m * THREADS;
            acc[m] = i < n ? hm_sum4<T>(v, i, lg - k - 1) : (T)0;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MAXPER; m++) {
            const uint32_t i = threadIdx.x + m * THREADS;
            if (i < n) v[i] = acc[m];
        }
        __syncthreads();
    }
}

/* Emit the non-empty cells i in [0, n) of v (cells with zoom outside [zmin,
 * zmax] skipped) with ONE output reservation per block, coalesced: wave w
 * takes the 64-cell chunks w, w + NW, ...; a chunk's non-empty cells go to
 * consecutive output positions (ballot + mbcnt), so one store instruction
 * writes one contiguous run of keys and one of counts.  cell(i) -> (zoom,
 * key) of cell i; the cells may be written in any order.  Every thread of
 * the block must call. */
template <int THREADS, typename CellF>
__device__ void hm_emit_cells(const uint32_t* v, uint32_t n, CellF cell, const HmOut& o, uint32_t* scr,
                              unsigned long long* sbase)
{
    constexpr int NW = THREADS / 64;
    const int lane = hm_lane(), w = threadIdx.x >> 6;
    uint32_t c = 0;
    for (uint32_t i0 = (uint32_t)w * 64; i0 < n; i0 += NW * 64) {
        const uint32_t i = i0 + lane;
        int z = 0;
        uint64_t k = 0;
        if (i < n) cell(i, z, k);
        const bool nz = i < n && v[i] != 0 && z >= o.zmin && z <= o.zmax;
        c += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(nz));
    }
    if (lane == 0) scr[w] = c;
    __syncthreads();
    if (w == 0) {
        const uint32_t x = lane < NW ? scr[lane] : 0u;
        const uint32_t incl = hm_wave_incl_scan(x);
        if (lane < NW) scr[lane] = incl - x;
        if (lane == NW - 1) *sbase = incl ? atomicAdd(o.cursor, (unsigned long long)incl) : 0ull;
    }
    __syncthreads();
    uint64_t base = *sbase + scr[w];
    __syncthreads();
    for (uint32_t i0 = (uint32_t)w * 64; i0 < n; i0 += NW * 64) {
        const uint32_t i = i0 + lane;
        int z = 0;
        uint64_t k = 0;
        uint32_t x = 0;
        if (i < n) {
            cell(i, z, k);
            x = v[i];
        }
        const bool nz = x != 0 && z >= o.zmin && z <= o.zmax;
        const uint64_t m = __builtin_amdgcn_ballot_w64(nz);
        const uint64_t pos = base + hm_mbcnt(m);
        if (nz && pos < o.capacity) {
            o.keys[pos] = k;
            o.counts[pos] = x;
        }
        base += (uint32_t)__builtin_popcountll(m);
    }
}

/* Bucket pyramid with two output reservations per block: level z_top (4^lg
 * cells in v) is emitted first; then levels z_top-1 .. z_top-lg+1 are built as
 * consecutive regions of v (the first in place), counted together, reserved
 * with one atomic and emitted.  v[0] ends up holding nothing useful; the
 * bucket total is returned (block-uniform). */
template <int THREADS>
__device__ uint64_t hm_bucket_pyramid(uint32_t* v, int lg, int z_top, uint64_t prefix, const HmOut& o,
                                      uint32_t* scr, unsigned long long* sbase)
{
    const uint32_t n0 = 1u << (2 * lg);
    if (lg == 0) return v[0];   /* the bucket is the zoom-z_top cell; k_pool emits it */
    hm_emit_cells<THREADS>(v, n0, [&](uint32_t i, int& z, uint64_t& k) {
        z = z_top;
        k = hm_cell_key(z_top, prefix, lg, i);
    }, o, scr, sbase);
    __syncthreads();
    /* level z_top-1 in place into v[0 .. n0/4) */
    uint32_t n = n0 >> 2;
    {
        constexpr int MAXPER = (HM_AG_CELLS / 4 + THREADS - 1) / THREADS;
        uint32_t acc[MAXPER];
#pragma unroll
        for (int m = 0; m < MAXPER; m++) {
            const uint32_t i = threadIdx.x + m * THREADS;
            acc[m] = i < n ? hm_sum4<uint32_t>(v, i, lg - 1) : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MAXPER; m++) {
            const uint32_t i = threadIdx.x + m * THREADS;
            if (i < n) v[i] = acc[m];
        }
        __syncthreads();
    }
    /* remaining levels appended: level k (k = 1 .. lg-1) at off[k], 4^(lg-k) cells */
    uint32_t off[HM_AG_LG + 1];
    off[1] = 0;
    uint32_t end = n;
    for (int k = 2; k <= lg; k++) {
        const uint32_t src = off[k - 1];
        const uint32_t m = n >> 2;
        off[k] = end;
        for (uint32_t i = threadIdx.x; i < m; i += THREADS)
            v[end + i] = hm_sum4<uint32_t>(v + src, i, lg - k);
        __syncthreads();
        end += m;
        n = m;
    }
    /* v[off[lg]] is the bucket total (zoom z_top - lg); emit levels 1..lg-1 */
    const uint64_t total = v[off[lg]];
    hm_emit_cells<THREADS>(v, off[lg], [&](uint32_t i, int& z, uint64_t& key) {
        int k = 1;
        while (k < lg - 1 && i >= off[k + 1]) k++;
        z = z_top - k;
        key = hm_cell_key(z, prefix, lg - k, i - off[k]);
    }, o, scr, sbase);
    __syncthreads();
    return total;
}

/* Final level, dense buckets: one block per <= HM_TA-key work item counts the
 * item's u16 keys in an LDS 2^lg x 2^lg histogram.  The rows are padded to
 * 2^lg + 8 words (cell (r, c) at r (2^lg + 8) + c: a cluster's cells in one
 * column fall in different banks, the row stride no longer being a multiple
 * of the 64 banks).  A single-item bucket emits its pyramid, at lg = 7 from
 * registers straight off the padded rows (hm_reg_pyramid7), below that from
 * the squeezed histogram; an item of a multi-item bucket adds its squeezed
 * histogram into the bucket's slot and k_aggregate_merged emits it. */
#ifndef HM_AG_PADW
#define HM_AG_PADW 8u   /* pad words per histogram row (a multiple of 4: hm_reg_pyramid7 reads 16-B vectors) */
#endif
#define HM_AG_ROW(lg) ((1u << (lg)) + HM_AG_PADW)
#define HM_AG_PADDED (128u * (128u + HM_AG_PADW))
static_assert(HM_AG_LG == 7 && HM_AG_CELLS == 128 * 128, "padded histogram");

/* The lg = 7 bucket pyramid from registers (k_aggregate's single-item
 * buckets): thread t holds the 4 x 4 block (t >> 5, t & 31) of the padded
 * 128 x 128 histogram, so zooms z_top-1 and z_top-2 are in-register sums; wave
 * 0 takes the 32 x 32 level (through s19) on to the bucket total, its lanes'
 * 4 x 4 blocks giving z_top-3 and z_top-4 and lane shuffles z_top-5, z_top-6
 * and the total.  Two barriers and one output reservation (hm_bucket_pyramid:
 * a barrier per level and LDS passes over every level twice); each level's
 * non-empty cells are ballot-compacted per wave, so the stores stay
 * coalesced.  Emits zooms z_top .. z_top-6 within [zmin, zmax] and returns the
 * bucket total (zoom z_top-7) in wave 0.  Every thread calls; the histogram's
 * rows are ROW words apart; s19 is 1024 words of 16-B-aligned scratch LDS. */
template <uint32_t ROW>
__device__ __forceinline__ uint64_t hm_reg_pyramid7(uint32_t* grid, int z_top, uint64_t prefix, const HmOut& o,
                                                    uint32_t* s19, uint32_t* scr, unsigned long long* sbase)
{
    constexpr int NW = HM_AG_THREADS / 64;
    static_assert(HM_AG_THREADS == 1024, "one 4 x 4 block per thread");
    const int tid = threadIdx.x, lane = hm_lane(), w = tid >> 6;
    const uint32_t br = (uint32_t)tid >> 5, bc = (uint32_t)tid & 31u;
    auto in = [&](int z) { return z >= o.zmin && z <= o.zmax; };
    auto nnz = [](bool nz) { return (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(nz)); };
    uint32_t c[16], d[4];
#pragma unroll
    for (int y = 0; y < 4; y++) {
        const uint4 q = *(const uint4*)&grid[(4u * br + y) * ROW + 4u * bc];
        c[4 * y] = q.x;
        c[4 * y + 1] = q.y;
        c[4 * y + 2] = q.z;
        c[4 * y + 3] = q.w;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = 8 * (j >> 1) + 2 * (j & 1);
        d[j] = c[r] + c[r + 1] + c[r + 4] + c[r + 5];
    }
    const uint32_t e = d[0] + d[1] + d[2] + d[3];
    s19[tid] = e;
    const bool i0 = in(z_top), i1 = in(z_top - 1), i2 = in(z_top - 2);
    uint32_t n = 0;
    if (i0)
#pragma unroll
        for (int j = 0; j < 16; j++) n += nnz(c[j] != 0);
    if (i1)
#pragma unroll
        for (int j = 0; j < 4; j++) n += nnz(d[j] != 0);
    if (i2) n += nnz(e != 0);
    if (lane == 0) scr[w] = n;
    __syncthreads();
    /* wave 0: lane l the 4 x 4 block (l >> 3, l & 7) of the 32 x 32 level */
    const uint32_t R = (uint32_t)lane >> 3, C = (uint32_t)lane & 7u;
    const bool l5 = (lane & 9) == 0, l6 = (lane & 27) == 0;
    const bool i3 = in(z_top - 3), i4 = in(z_top - 4), i5 = in(z_top - 5), i6 = in(z_top - 6);
    uint32_t g[4] = {0u, 0u, 0u, 0u}, h = 0, h5 = 0, h6 = 0, tot = 0;
    if (w == 0) {
        uint32_t f[16];
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const uint4 q = *(const uint4*)&s19[(4u * R + y) * 32u + 4u * C];
            f[4 * y] = q.x;
            f[4 * y + 1] = q.y;
            f[4 * y + 2] = q.z;
            f[4 * y + 3] = q.w;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = 8 * (j >> 1) + 2 * (j & 1);
            g[j] = f[r] + f[r + 1] + f[r + 4] + f[r + 5];
        }
        h = g[0] + g[1] + g[2] + g[3];                 /* z_top-4: (R, C) of 8 x 8 */
        uint32_t s = h + __shfl_xor(h, 1, 64);
        h5 = s + __shfl_xor(s, 8, 64);                 /* z_top-5: (R/2, C/2), lanes & 9 == 0 */
        s = h5 + __shfl_xor(h5, 2, 64);
        h6 = s + __shfl_xor(s, 16, 64);                /* z_top-6: (R/4, C/4), lanes & 27 == 0 */
        s = h6 + __shfl_xor(h6, 4, 64);
        tot = s + __shfl_xor(s, 32, 64);
        uint32_t ns = 0;
        if (i3)
#pragma unroll
            for (int j = 0; j < 4; j++) ns += nnz(g[j] != 0);
        if (i4) ns += nnz(h != 0);
        if (i5) ns += nnz(l5 && h5 != 0);
        if (i6) ns += nnz(l6 && h6 != 0);
        /* the waves' counts, then the small levels (slot NW) */
        const uint32_t x = lane < NW ? scr[lane] : lane == NW ? ns : 0u;
        const uint32_t incl = hm_wave_incl_scan(x);
        if (lane <= NW) scr[lane] = incl - x;
        if (lane == NW) *sbase = incl ? atomicAdd(o.cursor, (unsigned long long)incl) : 0ull;
    }
    __syncthreads();
    uint64_t base = *sbase + scr[w];
    /* the wave's cells staged in its share of the (now dead) histogram as
     * (level << 14 | cell, count) pairs and written out a whole line per
     * store (as k_small_pairs' hm_sp_flush) */
    constexpr uint32_t SC = HM_AG_PADDED / NW / 2 / 64 * 64;   /* cells per wave */
    uint2* stg = (uint2*)grid + (uint32_t)w * SC;
    uint32_t fill = 0;
    const auto flush = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (uint32_t q0 = 0; q0 < fill; q0 += 64) {
            const uint32_t q = q0 + (uint32_t)lane;
            const uint2 x = stg[q < fill ? q : 0u];
            const int l = (int)(x.x >> 14);
            const uint64_t pos = base + q;
            if (q < fill && pos < o.capacity) {
                o.keys[pos] = hm_cell_key(z_top - l, prefix, 7 - l, x.x & 0x3FFFu);
                o.counts[pos] = x.y;
            }
        }
        base += fill;
        fill = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    auto put = [&](bool nz, int z, int lg, uint32_t i, uint32_t v) {
        if (fill + 64u > SC) flush();   /* wave-uniform */
        const uint64_t m = __builtin_amdgcn_ballot_w64(nz);
        if (nz) stg[fill + hm_mbcnt(m)] = make_uint2(((uint32_t)(z_top - z) << 14) | i, v);
        fill += (uint32_t)__builtin_popcountll(m);
    };
    if (i0)
#pragma unroll
        for (int j = 0; j < 16; j++)
            put(c[j] != 0, z_top, 7, (4u * br + (j >> 2)) * 128u + 4u * bc + (j & 3), c[j]);
    if (i1)
#pragma unroll
        for (int j = 0; j < 4; j++) put(d[j] != 0, z_top - 1, 6, (2u * br + (j >> 1)) * 64u + 2u * bc + (j & 1), d[j]);
    if (i2) put(e != 0, z_top - 2, 5, br * 32u + bc, e);
    flush();
    if (w == 0) {
        base = *sbase + scr[NW];
        if (i3)
#pragma unroll
            for (int j = 0; j < 4; j++) put(g[j] != 0, z_top - 3, 4, (2u * R + (j >> 1)) * 16u + 2u * C + (j & 1), g[j]);
        if (i4) put(h != 0, z_top - 4, 3, R * 8u + C, h);
        if (i5) put(l5 && h5 != 0, z_top - 5, 2, (R >> 1) * 4u + (C >> 1), h5);
        if (i6) put(l6 && h6 != 0, z_top - 6, 1, (R >> 2) * 2u + (C >> 2), h6);
        flush();
    }
    return tot;
}
__global__ __launch_bounds__(HM_AG_THREADS, 8) void k_aggregate(HmAggArgs a)
{
    __shared__ alignas(16) uint32_t grid[HM_AG_PADDED + 64];   /* + 64 dummy words (hm_lds_count) */
    __shared__ uint32_t scr[HM_AG_THREADS / 64 + 1];
    __shared__ unsigned long long sbase;
    __shared__ alignas(16) HmRunLds<256> L;                     /* after the count: hm_reg_pyramid7's s19 */
    static_assert(sizeof(HmRunLds<256>) >= 1024 * sizeof(uint32_t), "s19 in the run chunk");
    const int tid = threadIdx.x;
    const uint32_t side = 1u << a.lg, ncell = side * side, npad = side * HM_AG_ROW(a.lg);
    HM_STAMP_M(5, 0);
    for (uint32_t i = tid; i < npad; i += HM_AG_THREADS) grid[i] = 0;
    __syncthreads();
    if (hm_block_id() >= a.items) return;   /* block-uniform */
    const HmItem it = hm_item(a.B, hm_block_id());
    HM_STAMP_M(5, 1);
    struct {
        uint32_t* grid;
        uint32_t dummy;
        int lg;
        __device__ __forceinline__ uint32_t sl(uint32_t k) { return k + (k >> lg) * HM_AG_PADW; }   /* padded row */
        __device__ __forceinline__ void cnt(uint32_t k, bool v)
        {
            hm_lds_count_fast(grid, dummy + (uint32_t)hm_lane(), sl(k), v);
        }
        __device__ __forceinline__ void key(uint32_t k, bool v, uint32_t) { cnt(k, v); }
        __device__ __forceinline__ void add(uint32_t k, bool v) { atomicAdd(&grid[v ? sl(k) : dummy + (uint32_t)hm_lane()], 1u); }
        /* 8 keys: the wave tests its first key only -- more than HM_MERGE_MIN
         * lanes on lane 0's key (a skewed cloud's hot cell) sends all 8 through
         * the merging count, otherwise they are 8 plain atomics (1e9 hotspots:
         * aggregation 762-770 -> 710-723 us at zooms 0-18, 3.58 -> 3.48 ms at
         * 6-21; skew unchanged; plain atomics on every vector took the skewed
         * cloud's aggregation 6.1 -> 8.6 ms) */
        __device__ __forceinline__ void vec(const uint4& x, bool v, uint32_t)
        {
            const uint32_t k0 = x.x & 0xFFFFu;
            const uint64_t m = __builtin_amdgcn_ballot_w64(v && k0 == __builtin_amdgcn_readfirstlane(k0));
            if ((uint32_t)__builtin_popcount((uint32_t)m) + (uint32_t)__builtin_popcount((uint32_t)(m >> 32)) > HM_MERGE_MIN) {
                cnt(x.x & 0xFFFFu, v);
                cnt(x.x >> 16, v);
                cnt(x.y & 0xFFFFu, v);
                cnt(x.y >> 16, v);
                cnt(x.z & 0xFFFFu, v);
                cnt(x.z >> 16, v);
                cnt(x.w & 0xFFFFu, v);
                cnt(x.w >> 16, v);
            } else {
                add(x.x & 0xFFFFu, v);
                add(x.x >> 16, v);
                add(x.y & 0xFFFFu, v);
                add(x.y >> 16, v);
                add(x.z & 0xFFFFu, v);
                add(x.z >> 16, v);
                add(x.w & 0xFFFFu, v);
                add(x.w >> 16, v);
            }
        }
    } f{grid, HM_AG_PADDED, a.lg};
    hm_stream_runs<uint16_t, HM_AG_THREADS, 256, false>(it, a.keys, a.in, L, scr, f);
    HM_STAMP_M(5, 2);
    HM_STAMP_V(5, 5, (unsigned long long)(it.b - it.a));
    HM_STAMP_V(5, 6, (unsigned long long)(it.r1 - it.r0));
    HM_STAMP_V(5, 7, (unsigned long long)it.nitems);
    if (it.nitems == 1 && a.lg == HM_AG_LG) {   /* block-uniform */
        const uint64_t t = hm_reg_pyramid7<HM_AG_ROW(7)>(grid, a.Z, a.B.coord[it.bucket], a.out, (uint32_t*)&L, scr,
                                                         &sbase);
        if (tid == 0) a.totals[it.bucket] = t;
        HM_STAMP_M(5, 3);
        HM_STAMP_M(5, 4);
        return;
    }
    /* squeeze the padding out: cell i back at i */
    constexpr int CPT = HM_AG_CELLS / HM_AG_THREADS;
    uint32_t x[CPT];
#pragma unroll
    for (int k = 0; k < CPT; k++) {
        const uint32_t i = k * HM_AG_THREADS + tid;
        x[k] = i < ncell ? grid[i + (i >> a.lg) * HM_AG_PADW] : 0u;
    }
    if (it.nitems > 1) {
        /* added into the bucket's slot (coalesced: consecutive threads,
         * consecutive words).  Measured against a slot per item summed by
         * k_aggregate_merged: the same on hotspots, and the skew cloud's one
         * 3400-item bucket made that sum a 3.7 ms single-block tail */
        uint32_t* g = a.gslots + (uint64_t)a.B.slots[it.bucket] * HM_AG_CELLS;
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < CPT; k++) {
            const uint32_t i = k * HM_AG_THREADS + tid;
            if (i < ncell && x[k]) atomicAdd(&g[i], x[k]);
            s += x[k];
        }
        s = hm_wave_sum(s);
        if (hm_lane() == 0 && s) atomicAdd(&a.totals[it.bucket], (unsigned long long)s);
        HM_STAMP_M(5, 3);
        HM_STAMP_M(5, 4);
        return;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CPT; k++) {
        const uint32_t i = k * HM_AG_THREADS + tid;
        if (i < ncell) grid[i] = x[k];
    }
    __syncthreads();
    HM_STAMP_M(5, 3);
    const uint64_t t = hm_bucket_pyramid<HM_AG_THREADS>(grid, a.lg, a.Z, a.B.coord[it.bucket], a.out, scr, &sbase);
    if (tid == 0) a.totals[it.bucket] = t;
    HM_STAMP_M(5, 4);
}
/* one block per multi-item bucket: its summed histogram, then its pyramid */
__global__ __launch_bounds__(HM_AG_THREADS) void k_aggregate_merged(HmAggArgs a)
{
    __shared__ alignas(16) uint32_t grid[HM_AG_CELLS];
    __shared__ alignas(16) uint32_t s19[1024];
    __shared__ uint32_t scr[HM_AG_THREADS / 64 + 1];
    __shared__ unsigned long long sbase;
    const uint32_t ncell = 1u << (2 * a.lg);
    if (hm_block_id() >= a.nslots) return;
    const uint32_t b = a.slot_bucket[hm_block_id()];
    const uint4* g = (const uint4*)(a.gslots + (uint64_t)hm_block_id() * HM_AG_CELLS);
    for (uint32_t v = threadIdx.x; v < ncell / 4; v += HM_AG_THREADS) ((uint4*)grid)[v] = g[v];
    __syncthreads();
    if (a.lg == HM_AG_LG)
        hm_reg_pyramid7<1u << HM_AG_LG>(grid, a.Z, a.B.coord[b], a.out, s19, scr, &sbase);
    else
        hm_bucket_pyramid<HM_AG_THREADS>(grid, a.lg, a.Z, a.B.coord[b], a.out, scr, &sbase);
}

/* ------------------------------------------------------------------------ */
/* final level, small buckets (<= HM_SPW_MAX keys): one wavefront per bucket  */
/* ------------------------------------------------------------------------ */

__device__ __forceinline__ uint32_t hm_spread7(uint32_t x)
{
    x = (x | (x << 4)) & 0x0F0Fu;
    x = (x | (x << 2)) & 0x3333u;
    return (x | (x << 1)) & 0x5555u;
}
__device__ __forceinline__ uint32_t hm_compact7(uint32_t x)
{
    x &= 0x5555u;
    x = (x | (x >> 1)) & 0x3333u;
    x = (x | (x >> 2)) & 0x0F0Fu;
    return (x | (x >> 4)) & 0x00FFu;
}

/* the value of lane (lane ^ M): DPP quad permutes for M = 1, 2 (no LDS
 * instruction), ds_swizzle's xor mode below 32 (no address), a bpermute for
 * 32 (HIP's __shfl_xor is a bpermute with a computed address for every M) */
template <int M>
__device__ __forceinline__ uint32_t hm_xor_lane(uint32_t v)
{
    if constexpr (M == 1)
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   /* quad_perm [1,0,3,2] */
    else if constexpr (M == 2)
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   /* quad_perm [2,3,0,1] */
    else if constexpr (M < 32)
        return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (M << 10) | 0x1F);           /* xor within 32 lanes */
    else
        return __shfl_xor(v, M, 64);
}

/* Ascending bitonic sort of the wave's 64*K values, element e = lane*K + u in
 * v[u]: distances < K swap registers, larger ones exchange across lanes.
 * Compile-time recursion over (size, stride), so every lane exchange has a
 * constant distance (hm_xor_lane). */
template <int K, int SIZE, int STRIDE>
__device__ __forceinline__ void hm_bitonic_step(uint32_t (&v)[K], uint32_t lane)
{
    if constexpr (STRIDE >= K) {
#pragma unroll
        for (int u = 0; u < K; u++) {
            const uint32_t e = lane * K + u;
            const uint32_t o = hm_xor_lane<STRIDE / K>(v[u]);
            const bool take_min = ((e & STRIDE) == 0) == ((e & SIZE) == 0);
            v[u] = take_min ? min(v[u], o) : max(v[u], o);
        }
    } else {
#pragma unroll
        for (int u = 0; u < K; u++) {
            if ((u & STRIDE) == 0) {
                const int w = u | STRIDE;
                const bool up = ((lane * K + u) & SIZE) == 0;
                const uint32_t lo = min(v[u], v[w]), hi = max(v[u], v[w]);
                v[u] = up ? lo : hi;
                v[w] = up ? hi : lo;
            }
        }
    }
    if constexpr (STRIDE > 1) hm_bitonic_step<K, SIZE, STRIDE / 2>(v, lane);
}
template <int K, int SIZE>
__device__ __forceinline__ void hm_bitonic_size(uint32_t (&v)[K], uint32_t lane)
{
    hm_bitonic_step<K, SIZE, SIZE / 2>(v, lane);
    if constexpr (SIZE < 64 * K) hm_bitonic_size<K, SIZE * 2>(v, lane);
}
template <int K>
__device__ __forceinline__ void hm_wave_bitonic(uint32_t (&v)[K])
{
    hm_bitonic_size<K, 2>(v, hm_lane());
}

/* Two 32-lane ascending bitonic sorts side by side (lanes 0-31 and 32-63,
 * one value per lane): the 64-lane network's stages up to size 32, with the
 * direction of size 32 taken inside each half */
template <int SIZE, int STRIDE>
__device__ __forceinline__ void hm_seg32_step(uint32_t& v, uint32_t lane)
{
    const uint32_t o = hm_xor_lane<STRIDE>(v);
    const bool take_min = ((lane & STRIDE) == 0) == ((lane & SIZE & 31u) == 0);
    v = take_min ? min(v, o) : max(v, o);
    if constexpr (STRIDE > 1) hm_seg32_step<SIZE, STRIDE / 2>(v, lane);
}
template <int SIZE>
__device__ __forceinline__ void hm_seg32_size(uint32_t& v, uint32_t lane)
{
    hm_seg32_step<SIZE, SIZE / 2>(v, lane);
    if constexpr (SIZE < 32) hm_seg32_size<SIZE * 2>(v, lane);
}

/* Buckets of <= 32 keys (a sparse cloud's common case: the skew background
 * averages ~24 per zoom-11 bucket) two per wave, one 32-lane segment each:
 * the bucket of segment g is the g-th of a pair picked from the wave's
 * ballot.  hm_pair_lane: the wave lane holding this lane's bucket (-1: the
 * segment has none). */
__device__ __forceinline__ int hm_pair_lane(uint64_t& mt)
{
    const int i0 = __builtin_ctzll(mt);
    mt &= mt - 1;
    const int i1 = mt ? __builtin_ctzll(mt) : -1;
    if (mt) mt &= mt - 1;
    return (hm_lane() >> 5) ? i1 : i0;
}

/* Small buckets run in two passes so that the output needs no per-bucket
 * cursor atomic (4M buckets would serialise on it at ~12 ns each):
 *   pass 1 (k_small_sort): a wave gathers a bucket's keys, re-codes them in
 *     Morton order inside the bucket, sorts them (Morton parents preserve the
 *     order, so the cells of level l are the runs of equal code >> 2l), stores
 *     the sorted codes at the bucket's own key range and counts its cells;
 *   an exclusive scan of the counts places every bucket's cells;
 *   pass 2 (k_small_emit): re-reads the sorted codes (coalesced) and writes
 *     each cell at its place; a cell is written by its last element, its count
 *     is that position minus the segment start (a wave max-scan). */

template <int K>
__device__ __forceinline__ void hm_small_load(const uint16_t* src, uint32_t nk, uint32_t (&v)[K])
{
    const uint32_t lane = hm_lane();
#pragma unroll
    for (int u = 0; u < K; u++) {
        const uint32_t e = lane * K + u;
        v[u] = e < nk ? (uint32_t)src[e] : 0xFFFFFFFFu;
    }
}

/* last element of its level-l cell (valid elements only); nx = the next
 * lane's v[0] */
template <int K>
__device__ __forceinline__ void hm_small_ends(const uint32_t (&v)[K], uint32_t nk, int l, bool (&end)[K], uint32_t nx)
{
    const uint32_t lane = hm_lane();
#pragma unroll
    for (int u = 0; u < K; u++) {
        const uint32_t e = lane * K + u;
        const uint32_t next = (u + 1 < K) ? v[u + 1] : nx;
        end[u] = (e < nk) & ((e + 1 == nk) | ((next >> (2 * l)) != (v[u] >> (2 * l))));
    }
}

template <int K>
__device__ __forceinline__ void hm_small_sort(const HmAggArgs& a, const uint16_t* ks, uint32_t nk, uint32_t kb,
                                              uint32_t zmask, uint32_t b)
{
    const uint32_t lane = hm_lane();
    const int lg = a.lg;
    const uint32_t cm = (1u << lg) - 1;
    uint32_t v[K];
    hm_small_load<K>(ks, nk, v);
#pragma unroll
    for (int u = 0; u < K; u++)
        if (v[u] != 0xFFFFFFFFu) v[u] = hm_spread7(v[u] & cm) | (hm_spread7(v[u] >> lg) << 1);
    hm_wave_bitonic<K>(v);
#pragma unroll
    for (int u = 0; u < K; u++) {
        const uint32_t e = lane * K + u;
        if (e < nk) a.codes[kb + e] = (uint16_t)v[u];
    }
    /* cells: element e ends a level-l cell iff its code and the next one's
     * differ above bit 2l, i.e. for the levels below half the bit length of
     * their xor (the last element ends every level): one count per element,
     * not a ballot per (level, element) */
    const uint32_t nx = __shfl_down(v[0], 1, 64);
    const uint32_t zall = (uint32_t)__popc(zmask);
    uint32_t cnt = 0;
#pragma unroll
    for (int u = 0; u < K; u++) {
        const uint32_t e = lane * K + u;
        const uint32_t next = (u + 1 < K) ? v[u + 1] : nx;
        const uint32_t x = v[u] ^ next;
        const uint32_t hl = (33u - (uint32_t)__clz((int)x)) >> 1;   /* x = 0: 0 */
        const uint32_t c = e + 1 == nk ? zall : (uint32_t)__popc(zmask & ((1u << hl) - 1u));
        cnt += e < nk ? c : 0u;
    }
    const uint32_t total = hm_wave_sum(cnt);
    if (lane == 0) a.spcnt[b] = total;
}

template <int K>
__device__ __forceinline__ void hm_small_emit(const HmAggArgs& a, uint32_t nk, uint32_t kb, uint64_t coord,
                                              uint32_t zmask, uint64_t base, uint32_t* hw)
{
    const uint32_t lane = hm_lane();
    const int lg = a.lg;
    uint32_t v[K];
    hm_small_load<K>(a.codes + kb, nk, v);
    /* the four coarsest levels (<= 256 cells each) from a 256-slot LDS
     * histogram of the codes' top 8 bits: one LDS atomic per key; the
     * coarsest-but-three level has 4 slots per lane, the next ones are sums
     * of 4 (in the lane, then across quads of lanes): one store per level and
     * slot group instead of a pass over every key per level */
    /* (buckets of <= 128 keys: the three coarsest levels, 64 slots -- the
     * fourth costs them more as 256 slots than as a pass over their keys) */
    constexpr int NC = K >= 4 ? 4 : 3;
    const int lc = lg >= NC ? lg - NC : 0;
    if (zmask >> lc) {
        uint4* hw4 = (uint4*)hw;
        if (NC == 4) hw4[lane] = make_uint4(0u, 0u, 0u, 0u);
        else hw[lane] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int u = 0; u < K; u++)
            if (lane * K + u < nk) atomicAdd(&hw[v[u] >> (2 * lc)], 1u);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint64_t q = base;
        auto put = [&](bool mine, uint64_t bal, uint32_t code, int l, uint32_t c) {
            if (mine) {
                const int sl = lg - l;
                const uint32_t idx = (hm_compact7(code >> 1) << sl) | hm_compact7(code);
                const uint64_t p = q + hm_mbcnt(bal);
                if (p < a.out.capacity) {
                    a.out.keys[p] = hm_cell_key(a.Z - l, coord, sl, idx);
                    a.out.counts[p] = (uint64_t)c;
                }
            }
            q += (uint64_t)__popcll(bal);
        };
        uint32_t c;   /* the count of prefix = lane at level l1 */
        int l1 = lc;
        if constexpr (NC == 4) {
            const uint4 c4 = hw4[lane];   /* prefixes 4 lane + j (slots past 4^(lg - lc) stay 0) */
            if ((zmask >> lc) & 1u) {
                const uint32_t cj[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const bool mine = cj[j] != 0u;
                    put(mine, __ballot(mine), lane * 4u + (uint32_t)j, lc, cj[j]);
                }
            }
            c = c4.x + c4.y + c4.z + c4.w;
            l1 = lc + 1;
        } else {
            c = hw[lane];
        }
        for (int l = l1; l < lg; l++) {
            const int g = 2 * (l - l1);   /* this level's prefix: lane >> g on lanes with those bits clear */
            if (g) {
                /* sum the 4 finer cells: lanes lane + {0, 1, 2, 3} 2^(g-2) */
                const int st = 1 << (g - 2);
                c += __shfl_down(c, st, 64);
                c += __shfl_down(c, 2 * st, 64);
            }
            const bool mine = (lane & ((1u << g) - 1u)) == 0u && c != 0u && ((zmask >> l) & 1u);
            put(mine, __ballot(mine), lane >> g, l, c);
        }
        base = q;
        __builtin_amdgcn_wave_barrier();   /* hw is free for the next bucket */
    }
    /* the neighbours' codes are level-independent: read once per bucket */
    const uint32_t nx = __shfl_down(v[0], 1, 64);
    const uint32_t pv = __shfl_up(v[K - 1], 1, 64);
    for (int l = 0; l < lc; l++) {
        if (!((zmask >> l) & 1u)) continue;
        bool end[K];
        hm_small_ends<K>(v, nk, l, end, nx);
        /* segment start of every element: running max of head positions */
        uint32_t hs[K];
        uint32_t run = 0;
#pragma unroll
        for (int u = 0; u < K; u++) {
            const uint32_t e = lane * K + u;
            const uint32_t prev = u > 0 ? v[u - 1] : pv;
            run = ((e == 0) | ((prev >> (2 * l)) != (v[u] >> (2 * l)))) ? e : run;
            hs[u] = run;
        }
        /* the last head before this lane's elements: heads' positions grow
         * with the lane, so it is the run of the highest lower lane holding a
         * head (lane 0 always does: element 0) -- one ballot and one
         * cross-lane read instead of a 6-step max-scan */
        const uint64_t hmask = __ballot((run != 0u) | (lane == 0u));
        const uint64_t below = hmask & ((1ull << lane) - 1ull);
        uint32_t ex = __shfl(run, below ? 63 - __clzll((long long)below) : 0, 64);
        ex = lane ? ex : 0u;
        const int zl = a.Z - l;
        const int s = lg - l;
#pragma unroll
        for (int u = 0; u < K; u++) {
            const uint64_t bal = __ballot(end[u]);
            if (end[u]) {
                const uint32_t e = lane * K + u;
                const uint32_t code = v[u] >> (2 * l);
                const uint32_t idx = (hm_compact7(code >> 1) << s) | hm_compact7(code);
                const uint64_t q = base + hm_mbcnt(bal);
                if (q < a.out.capacity) {
                    a.out.keys[q] = hm_cell_key(zl, coord, s, idx);
                    a.out.counts[q] = (uint64_t)(e - max(hs[u], ex) + 1);
                }
            }
            base += __popcll(bal);
        }
    }
}

__device__ __forceinline__ uint32_t hm_small_zmask(const HmAggArgs& a)
{
    uint32_t zmask = 0;
    for (int l = 0; l < a.lg; l++) {
        const int z = a.Z - l;
        zmask |= (uint32_t)(z >= a.out.zmin && z <= a.out.zmax) << l;
    }
    return zmask;
}

/* The register sort of bucket size nk runs with K = ceil(nk / 64) rounded up
 * to a power of two, for K in the instantiation's range only: a kernel's VGPR
 * budget is its widest K's (K = 32 needs ~200, two waves per SIMD), so buckets
 * of <= HM_SPW_SPLIT keys get their own narrow, high-occupancy instantiation
 * and LO < nk <= HI selects a kernel's share. */
template <uint32_t LO, uint32_t HI, typename F>
__device__ __forceinline__ void hm_small_dispatch(uint32_t nk, F&& f)
{
    if constexpr (LO < 64) if (nk <= 64) { f(std::integral_constant<int, 1>{}); return; }
    if constexpr (LO < 128 && HI >= 128) if (nk <= 128) { f(std::integral_constant<int, 2>{}); return; }
    if constexpr (LO < 256 && HI >= 256) if (nk <= 256) { f(std::integral_constant<int, 4>{}); return; }
    if constexpr (LO < 512 && HI >= 512) if (nk <= 512) { f(std::integral_constant<int, 8>{}); return; }
    if constexpr (LO < 1024 && HI >= 1024) if (nk <= 1024) { f(std::integral_constant<int, 16>{}); return; }
    if constexpr (LO < 2048 && HI >= 2048) if (nk <= 2048) { f(std::integral_constant<int, 32>{}); return; }
    if constexpr (HI >= 4096) f(std::integral_constant<int, 64>{});
}

/* Which buckets a wave looks at.  LO == 0 (the narrow instantiation, most
 * buckets): wave w takes the batches of spbatch consecutive buckets w, w +
 * waves, ...  LO > 0 (the wide one: buckets of > HM_SPW_SPLIT keys, few and
 * clustered in space, i.e. in bucket order): lane j of wave w at step s looks
 * at bucket (64 s + j) waves + w, so neighbouring big buckets go to different
 * waves (consecutive batches left one wave sorting several of them while the
 * others idled: the tail of a stream batch's 513-2048-key pass). */
template <uint32_t LO>
struct HmSmallMap {
    static __device__ __forceinline__ uint32_t first(uint32_t wid, uint32_t spb) { return LO ? 0u : wid * spb; }
    static __device__ __forceinline__ uint32_t step(uint32_t nw, uint32_t spb) { return LO ? 64u : nw * spb; }
    static __device__ __forceinline__ uint64_t bucket(uint32_t s0, uint32_t lane, uint32_t wid, uint32_t nw)
    {
        return LO ? (uint64_t)(s0 + lane) * nw + wid : (uint64_t)s0 + lane;
    }
    static __device__ __forceinline__ bool lane_in(uint32_t lane, uint32_t spb) { return LO ? true : lane < spb; }
};

/* the small buckets k_small_pairs takes: <= 32 keys in <= 32 runs (two a
 * wave pass) or 33-64 keys in <= 64 runs (one) */
__device__ __forceinline__ bool hm_sp_fused_ok(uint32_t nk, uint32_t nr)
{
    return nk <= 64 && nr <= (nk <= 32 ? 32u : 64u);
}

/* Persistent: a bucket is this instantiation's when LO < nkeys <= HI (larger
 * ones are k_aggregate's). The LO == 0 instantiation runs first and zeroes the
 * cell count of every bucket that is not its own. */
template <uint32_t LO, uint32_t HI>
__global__ __launch_bounds__(HM_SPW_THREADS) void k_small_sort(HmAggArgs a)
{
    __shared__ uint16_t kss[HM_SPW_THREADS / 64][HI];
    const uint32_t lane = hm_lane();
    uint16_t* ks = kss[threadIdx.x >> 6];
    const uint32_t nw = gridDim.x * (HM_SPW_THREADS / 64);
    const uint32_t zmask = hm_small_zmask(a);
    const uint32_t wid = blockIdx.x * (HM_SPW_THREADS / 64) + (threadIdx.x >> 6);
    const uint32_t step = HmSmallMap<LO>::step(nw, a.spbatch);
    for (uint32_t s0 = HmSmallMap<LO>::first(wid, a.spbatch); HmSmallMap<LO>::bucket(s0, 0, wid, nw) < a.B.count;
         s0 += step) {
        const uint64_t bl64 = HmSmallMap<LO>::bucket(s0, lane, wid, nw);
        const bool in = HmSmallMap<LO>::lane_in(lane, a.spbatch) & (bl64 < a.B.count);
        const uint32_t bl = in ? (uint32_t)bl64 : 0u;
        const uint32_t nkl = in ? a.B.nkeys[bl] : 0u;
        const bool small = in & (LO == 0 || nkl > LO) & (nkl <= HI);
        const uint32_t rbl = small ? a.B.rbase[bl] : 0u, nrl = small ? a.B.nruns[bl] : 0u;
        const uint32_t kbl = small ? a.B.keybase[bl] : 0u;
        /* (the buckets hm_sp_fused_ok takes are k_small_pairs') */
        const bool pairb = LO == 0 && small && hm_sp_fused_ok(nkl, nrl);
        if (LO == 0 && in && (!small || pairb)) a.spcnt[bl] = 0;
        if (small && !pairb) a.totals[bl] = nkl;
        uint64_t m = __ballot(small && !pairb);
        while (m) {
            const int i = __builtin_ctzll(m);
            m &= m - 1;
            const uint32_t b = __shfl(bl, i, 64);
            const uint32_t nk = __shfl(nkl, i, 64), r0 = __shfl(rbl, i, 64), nr = __shfl(nrl, i, 64);
            const uint32_t kb = __shfl(kbl, i, 64);
            /* gather: runs 64 at a time, consecutive keys to consecutive lanes */
            uint32_t fill = 0;
            if (nr <= 4) {
                /* few runs (the common case: one per parent item): their
                 * bounds in scalar registers, a key's run by three compares
                 * instead of a 6-step shuffle search */
                const uint2 run = lane < nr ? a.in.run[r0 + lane] : make_uint2(0, 0);
                const uint32_t x0 = __builtin_amdgcn_readlane(run.x, 0), x1 = __builtin_amdgcn_readlane(run.x, 1);
                const uint32_t x2 = __builtin_amdgcn_readlane(run.x, 2), x3 = __builtin_amdgcn_readlane(run.x, 3);
                const uint32_t p1 = __builtin_amdgcn_readlane(run.y, 0);
                const uint32_t p2 = p1 + __builtin_amdgcn_readlane(run.y, 1);
                const uint32_t p3 = p2 + __builtin_amdgcn_readlane(run.y, 2);
                const uint32_t tot = p3 + __builtin_amdgcn_readlane(run.y, 3);
                for (uint32_t j = lane; j < tot; j += 64) {
                    const uint32_t src = j < p1 ? x0 + j : j < p2 ? x1 + (j - p1) : j < p3 ? x2 + (j - p2) : x3 + (j - p3);
                    ks[j] = a.keys[src];
                }
            } else
            for (uint32_t c0 = 0; c0 < nr; c0 += 64) {
                const uint32_t q = c0 + lane;
                const uint2 run = q < nr ? a.in.run[r0 + q] : make_uint2(0, 0);
                const uint32_t incl = hm_wave_incl_scan(run.y);
                const uint32_t tot = __shfl(incl, 63, 64);
                for (uint32_t j0 = 0; j0 < tot; j0 += 64) {
                    const uint32_t j = j0 + lane;
                    uint32_t lo = 0;
#pragma unroll
                    for (int st = 32; st > 0; st >>= 1)
                        if (__shfl(incl, lo + st - 1, 64) <= j) lo += st;
                    lo = min(lo, 63u);
                    const uint32_t cnt = __shfl(run.y, lo, 64);
                    const uint32_t off = j - (__shfl(incl, lo, 64) - cnt);
                    const uint32_t src = __shfl(run.x, lo, 64) + off;
                    if (j < tot) ks[fill + j] = a.keys[src];
                }
                fill += tot;
            }
            __builtin_amdgcn_wave_barrier();
            hm_small_dispatch<LO, HI>(nk, [&](auto kc) { hm_small_sort<decltype(kc)::value>(a, ks, nk, kb, zmask, b); });
            __builtin_amdgcn_wave_barrier();
        }
    }
}

/* k_small_pairs (round 6): the small buckets of <= 64 keys --
 * the skew cloud's background, ~24 keys per zoom-11 bucket, 4M of them --
 * gathered, sorted, counted AND emitted in one pass.  A wave pass ("row")
 * takes two buckets of <= 32 keys in <= 32 runs (one 32-lane segment each) or
 * one of 33-64 keys in <= 64 runs; a wave sorts up to 32 rows of its batch of
 * 64 buckets into 4 KB of LDS, reserves their cells with ONE cursor atomic
 * (~1.5K cells on the skew cloud: ~65K atomics for 4M buckets, not one per
 * bucket) and emits them from LDS as k_small_emit does: no sorted codes
 * through HBM, no per-bucket count array, no scan or reservation launch. */

/* One row's bucket(s) in three steps, so a wave can keep the next rows'
 * loads in flight while it sorts: W = 32 (a pair: each 32-lane half holds its
 * own bucket) or 64 (one bucket); every lane active; the loads are
 * unconditional (inactive lanes read element 0), so the compiler counts them.
 *   hm_sp_run:  the segment's runs, one a lane;
 *   hm_sp_key:  lane j's key: in the first run whose inclusive key count
 *               passes j (segmented scan + binary search), 0xFFFF if none;
 *   hm_sp_sort: Morton code, segmented sort, the segment's cell count. */
__device__ __forceinline__ uint2 hm_sp_run(const HmAggArgs& a, bool seg, uint32_t r0, uint32_t nr, uint32_t j)
{
    const bool v = seg && j < nr;
    const uint2 r = a.in.run[v ? r0 + j : 0u];
    return v ? r : make_uint2(0, 0);
}
template <int W>
__device__ __forceinline__ uint32_t hm_sp_key(const HmAggArgs& a, uint2 run, bool seg, uint32_t nk, uint32_t lane,
                                              uint2* sc)
{
    const uint32_t j = lane & (W - 1);
    /* each non-empty run r marks its first key position excl_r in the wave's
     * 64-slot scratch with x_r - excl_r; lane j's run starts at the last mark
     * at or below j (a ballot), so its key is at that mark's value + j: a DPP
     * scan and three LDS round trips instead of a shuffle search */
    uint32_t incl = run.y;
    HM_DPP_ADD(incl, 0x111, 0xF);   /* row_shr:1 */
    HM_DPP_ADD(incl, 0x112, 0xF);   /* row_shr:2 */
    HM_DPP_ADD(incl, 0x114, 0xF);   /* row_shr:4 */
    HM_DPP_ADD(incl, 0x118, 0xF);   /* row_shr:8 */
    HM_DPP_ADD(incl, 0x142, 0xA);   /* row_bcast:15: rows 0 -> 1, 2 -> 3 (each 32-lane half scanned) */
    if constexpr (W == 64) HM_DPP_ADD(incl, 0x143, 0xC);   /* row_bcast:31: the whole wave */
    const uint32_t excl = incl - run.y;
    sc[lane] = make_uint2(0u, 0u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (run.y) sc[(lane & ~(uint32_t)(W - 1)) + excl] = make_uint2(run.x - excl, 1u);   /* (run.y = 0 past nr) */
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint64_t marks = __ballot(sc[lane].y != 0u);
    const uint64_t below = marks & ((2ull << lane) - 1ull);
    const uint32_t h = below ? 63u - (uint32_t)__clzll((long long)below) : lane;
    const uint32_t d = sc[h].x;
    const bool v_ok = seg && j < nk;
    const uint32_t k = (uint32_t)a.keys[v_ok ? d + j : 0u];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   /* sc is free for the next row */
    return v_ok ? k : 0xFFFFFFFFu;
}
template <int W>
__device__ __forceinline__ uint32_t hm_sp_sort(const HmAggArgs& a, uint32_t key, uint32_t nk, uint32_t lane,
                                               uint32_t zmask, uint32_t& v)
{
    const uint32_t j = lane & (W - 1);
    const uint32_t cm = (1u << a.lg) - 1;
    const bool v_ok = key != 0xFFFFFFFFu;
    v = v_ok ? hm_spread7(key & cm) | (hm_spread7(key >> a.lg) << 1) : 0xFFFFFFFFu;
    if constexpr (W == 32) {
        hm_seg32_size<2>(v, lane);
    } else {
        uint32_t vv[1] = {v};
        hm_wave_bitonic<1>(vv);
        v = vv[0];
    }
    /* cells ended by this element (hm_small_sort), summed over the segment */
    const uint32_t nx = __shfl_down(v, 1, 64);
    const uint32_t hl = (33u - (uint32_t)__clz((int)(v ^ nx))) >> 1;
    uint32_t total = !v_ok ? 0u
                           : (j + 1 == nk) ? (uint32_t)__popc(zmask) : (uint32_t)__popc(zmask & ((1u << hl) - 1u));
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
    return total;
}

/* the cells of one sorted row segment (a cell is written by its last element,
 * its count = that position - the segment's last end below it) staged in the
 * wave's LDS buffer as one u32 each -- bucket lane (6 bits) | level (3) |
 * row (7) | column (7) | count (7) -- at q (per lane, relative to the buffer),
 * for hm_sp_flush to write out */
template <int W>
__device__ __forceinline__ void hm_sp_stage(const HmAggArgs& a, uint32_t v, bool v_ok, uint32_t nk, uint32_t b,
                                            uint32_t q, uint32_t zmask, uint32_t lane, uint32_t* sb)
{
    const uint32_t j = lane & (W - 1);
    const uint64_t segm = W == 64 ? ~0ull : (lane >> 5) ? 0xFFFFFFFF00000000ull : 0x00000000FFFFFFFFull;
    const uint32_t nx = __shfl_down(v, 1, 64);
    const uint32_t cr = hm_compact7(v >> 1), cc = hm_compact7(v);
    const uint32_t bl = b << 24;
    /* the element ends its level-l cell for the levels below half the bit
     * length of (its code ^ the next one's), every level if it is the last;
     * a cell starts after the previous end in the segment: one ballot a level */
    const uint32_t hl = !v_ok ? 0u : (j + 1 == nk) ? 32u : (33u - (uint32_t)__clz((int)(v ^ nx))) >> 1;
    const uint64_t below = segm & ((1ull << lane) - 1ull);
    const uint32_t s0 = lane & ~(uint32_t)(W - 1);   /* the segment's first lane */
    for (int l = 0; l < a.lg; l++) {
        if (!((zmask >> l) & 1u)) continue;
        const bool end = (uint32_t)l < hl;
        const uint64_t bal = __ballot(end) & segm;
        if (end) {
            const uint64_t pe = bal & below;
            const uint32_t start = pe ? 64u - (uint32_t)__clzll((long long)pe) : s0;
            sb[q + (uint32_t)__popcll(pe)] = bl | ((uint32_t)l << 21) | ((cr >> l) << 14) | ((cc >> l) << 7) | (lane - start + 1);
        }
        q += (uint32_t)__popcll(bal);
    }
}

/* n staged cells to keys / counts [g, g + n): every lane two 8-B stores of
 * consecutive cells, so each 64-B line is written whole by one instruction
 * (a store per cell and level as it ends leaves lines written in pieces by
 * several instructions; skew aggregation 3.88-3.92 -> 3.53-3.77 ms,
 * profiles/r6/small_pairs_block_res_ab.jsonl) */
__device__ __forceinline__ void hm_sp_flush(const HmAggArgs& a, const uint32_t* sb, uint32_t n, uint64_t g,
                                            uint64_t cl, uint32_t lane)
{
    const uint32_t clo = (uint32_t)cl, chi = (uint32_t)(cl >> 32);
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        const uint32_t c = sb[i < n ? i : 0u];
        const int b = (int)((c >> 24) & 63u), l = (int)((c >> 21) & 7u);
        const uint32_t crow = (uint32_t)__shfl((int)chi, b, 64), ccol = (uint32_t)__shfl((int)clo, b, 64);
        const int s = a.lg - l;
        const uint32_t row = (crow << s) | ((c >> 14) & 127u), col = (ccol << s) | ((c >> 7) & 127u);
        const uint64_t p = g + i;
        if (i < n && p < a.out.capacity) {
            a.out.keys[p] = ((uint64_t)(a.Z - l) << 58) | ((uint64_t)row << 29) | col;
            a.out.counts[p] = (uint64_t)(c & 127u);
        }
    }
}

/* The waves of a block reserve their cells together: one cursor atomic per
 * block and round (HM_SPP_WAVES waves' sub-batches of <= 32 rows) instead of
 * one per wave sub-batch (~65K on the skew cloud, on ONE word; skew
 * aggregation -0.3 ms.  The "no atomic" timing builds of
 * profiles/r6/small_pairs_atomics_ab.jsonl overstate the atomics' cost: their
 * made-up positions overlapped, and WRITE_SIZE showed them writing 0.57 of
 * the 6.1 GB of cells, profiles/r6/small_pairs_pmc_bytes.txt).  Block
 * batches (HM_SPP_WAVES x spbatch consecutive buckets) come from a counter,
 * one atomic per block batch.  Rounds are block-synchronous: pass 1 of every
 * wave, a barrier, the reservation (wave 0), a barrier, pass 2.  (An extra
 * wave for the atomics, so that they do not queue behind wave 0's cell
 * stores, measured slower: 9-wave blocks fit 2 to a CU, not 3.) */
template <int NWB>
__global__ __launch_bounds__(64 * NWB) void k_small_pairs(HmAggArgs a)
{
    __shared__ uint16_t cds[NWB][HM_SPP_ROWS][64];   /* a round's rows of sorted codes per wave */
    __shared__ uint2 gsc[NWB][64];          /* hm_sp_key's run marks */
    __shared__ uint32_t sbuf[NWB][HM_SPP_STAGE_CELLS];   /* staged cells (hm_sp_stage) */
    __shared__ uint32_t s_wtot[NWB];        /* the round's cells per wave */
    __shared__ unsigned long long s_base;   /* the round's reservation */
    __shared__ uint32_t s_batch;            /* the block's next batch */
    __shared__ uint32_t s_more[2];          /* a wave has rows for the next round (by round parity) */
    const uint32_t lane = hm_lane();
    const uint32_t wl = threadIdx.x >> 6;
    const bool alloc = wl == 0;   /* the wave of the atomics (wave-uniform) */
    const uint32_t wc = wl;
    const uint32_t zmask = hm_small_zmask(a);
    const uint32_t per_block = NWB * a.spbatch;
    /* (block barriers are LDS-only: a __syncthreads would also wait for the
     * waves' cell stores) */
    if (alloc && lane == 0) {
        s_batch = atomicAdd(a.spq, 1u);
        s_more[0] = s_more[1] = 0u;
    }
    hm_lds_barrier();
    uint32_t rr = 0;   /* round parity */
#if defined(HM_STAMPS) && HM_STAMPS == 7
    /* cycles summed per block: worker 0's pass 1, first-barrier wait, second-
     * barrier wait, pass 2; the atomics (wave 0); rounds; block batches */
    unsigned long long st7[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long t7 = __builtin_amdgcn_s_memtime();
#define HM_ST7(k) do { const unsigned long long n7 = __builtin_amdgcn_s_memtime(); st7[k] += n7 - t7; t7 = n7; } while (0)
#else
#define HM_ST7(k) do { } while (0)
#endif
    for (;;) {
        const uint32_t kb = s_batch;   /* block-uniform */
        if ((uint64_t)kb * per_block >= a.B.count) break;
        uint32_t kn = 0;   /* (thread 0) the block's batch after this one */
        const uint64_t bl64 = (uint64_t)kb * per_block + wc * a.spbatch + lane;
        const bool in = lane < a.spbatch && bl64 < a.B.count;
        const uint32_t bl = in ? (uint32_t)bl64 : 0u;
        const uint32_t nkl = in ? a.B.nkeys[bl] : 0u;
        const bool small = in & (nkl <= HM_SPW_SPLIT);
        const uint32_t nrl = small ? a.B.nruns[bl] : 0u;
        const bool mine = small && hm_sp_fused_ok(nkl, nrl);
        uint64_t mp = __ballot(mine && nkl <= 32), ms = __ballot(mine && nkl > 32);
        const uint32_t rbl = mine ? a.B.rbase[bl] : 0u;
        const uint64_t cl = mine ? a.B.coord[bl] : 0ull;
        if (mine) a.totals[bl] = nkl;
        for (bool first = true;; first = false) {
            /* pass 1: up to 32 rows (pairs first) sorted into LDS; lane 2p + g
             * keeps row p's segment-g cell count.  Software-pipelined: while
             * row p sorts, row p+1's key and row p+2's runs are loading */
            uint32_t segcnt = 0;
            uint64_t mp1 = mp, ms1 = ms;
            const uint32_t nrows = min((uint32_t)HM_SPP_ROWS, (uint32_t)(__popcll(mp) + 1) / 2 + (uint32_t)__popcll(ms));
            if (mp | ms) {   /* wave-uniform */
                struct Row {
                    bool paired, seg;
                    uint32_t nk, r0, nr;
                };
                auto take = [&](bool any) -> Row {
                    Row r;
                    r.paired = !any || mp1 != 0;
                    int src = 0;
                    r.seg = false;
                    if (any && mp1) {
                        const int sl = hm_pair_lane(mp1);
                        r.seg = sl >= 0;
                        src = r.seg ? sl : 0;
                    } else if (any && ms1) {
                        src = __builtin_ctzll(ms1);
                        ms1 &= ms1 - 1;
                        r.seg = true;
                    }
                    const uint32_t nk0 = __shfl(nkl, src, 64), r00 = __shfl(rbl, src, 64), nr0 = __shfl(nrl, src, 64);
                    r.nk = r.seg ? nk0 : 0u;
                    r.r0 = r00;
                    r.nr = r.seg ? nr0 : 0u;
                    return r;
                };
                auto key_of = [&](const Row& r, uint2 run) {
                    return r.paired ? hm_sp_key<32>(a, run, r.seg, r.nk, lane, gsc[wc])
                                    : hm_sp_key<64>(a, run, r.seg, r.nk, lane, gsc[wc]);
                };
                const uint32_t jl = lane & 31u;
                Row A = take(true);
                uint2 runA = hm_sp_run(a, A.seg, A.r0, A.nr, A.paired ? jl : lane);
                Row B = take(nrows > 1);
                uint2 runB = hm_sp_run(a, B.seg, B.r0, B.nr, B.paired ? jl : lane);
                uint32_t keyA = key_of(A, runA);
                for (uint32_t p = 0; p < nrows; p++) {
                    const Row C = take(p + 2 < nrows);
                    const uint2 runC = hm_sp_run(a, C.seg, C.r0, C.nr, C.paired ? jl : lane);
                    const uint32_t keyB = key_of(B, runB);
                    uint32_t v, tot;
                    if (A.paired) tot = hm_sp_sort<32>(a, keyA, A.nk, lane, zmask, v);
                    else tot = hm_sp_sort<64>(a, keyA, A.nk, lane, zmask, v);
                    cds[wc][p][lane] = (uint16_t)v;
                    /* (a single's segment is the whole wave: lane 32 repeats its total) */
                    const uint32_t t0 = __builtin_amdgcn_readlane(tot, 0);
                    const uint32_t t1 = A.paired ? __builtin_amdgcn_readlane(tot, 32) : 0u;
                    segcnt = lane == 2 * p ? t0 : lane == 2 * p + 1 ? t1 : segcnt;
                    A = B;
                    keyA = keyB;
                    B = C;
                    runB = runC;
                }
            }
            HM_ST7(0);
            const uint32_t incl = hm_wave_incl_scan(segcnt);
            const uint32_t excl = incl - segcnt;
            if (lane == 0) {
                s_wtot[wl] = __builtin_amdgcn_readlane(incl, 63);
                if (mp1 | ms1) s_more[rr] = 1u;
            }
            hm_lds_barrier();
            HM_ST7(1);
            const bool more = s_more[rr] != 0u;
            /* one reservation for the block's rows (and, in the first round,
             * the block's next batch, both atomics in flight together) */
            uint32_t wpre = 0, btotal = 0;
#pragma unroll
            for (int w = 0; w < NWB; w++) {
                const uint32_t t = s_wtot[w];
                wpre += (uint32_t)w < wl ? t : 0u;
                btotal += t;
            }
            if (alloc && lane == 0) {
                s_more[rr ^ 1u] = 0u;   /* (last read before the previous round's second barrier) */
                if (first) kn = atomicAdd(a.spq, 1u);
                s_base = btotal ? atomicAdd(a.out.cursor, (unsigned long long)btotal) : 0ull;
            }
            HM_ST7(4);
            hm_lds_barrier();
            HM_ST7(2);
            const uint64_t base = s_base + wpre;
            /* pass 2: the same rows in the same order, codes from LDS */
            uint64_t mp2 = mp, ms2 = ms;
            /* the cells go through the wave's LDS buffer (rows in order: the
             * wave's cells are written in order), flushed before a row that
             * does not fit and at the end */
            uint32_t* sb = sbuf[wc];
            uint32_t flushed = 0;   /* this round's cells written so far */
            const auto sync_sb = [&]() {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            };
            for (uint32_t p = 0; p < ((mp | ms) ? nrows : 0u); p++) {
                const uint32_t v = cds[wc][p][lane];
                const uint32_t rlo = __shfl(excl, (int)(2 * p), 64), rhi = __shfl(incl, (int)(2 * p + 1), 64);
                if (rhi - flushed > HM_SPP_STAGE_CELLS) {
                    sync_sb();
                    hm_sp_flush(a, sb, rlo - flushed, base + flushed, cl, lane);
                    sync_sb();
                    flushed = rlo;
                }
                if (mp2) {
                    const int sl = hm_pair_lane(mp2);
                    const bool seg = sl >= 0;
                    const int sr = seg ? sl : 0;
                    const uint32_t nk0 = __shfl(nkl, sr, 64);
                    const uint32_t nk = seg ? nk0 : 0u;
                    const uint32_t q = __shfl(excl, (int)(2 * p + (lane >> 5)), 64) - flushed;
                    hm_sp_stage<32>(a, v == 0xFFFFu ? 0xFFFFFFFFu : v, seg && (lane & 31u) < nk, nk, (uint32_t)sr, q, zmask,
                                    lane, sb);
                } else {
                    const int i = __builtin_ctzll(ms2);
                    ms2 &= ms2 - 1;
                    const uint32_t nk = __shfl(nkl, i, 64);
                    const uint32_t q = __shfl(excl, (int)(2 * p), 64) - flushed;
                    hm_sp_stage<64>(a, v == 0xFFFFu ? 0xFFFFFFFFu : v, lane < nk, nk, (uint32_t)i, q, zmask, lane, sb);
                }
            }
            {
                const uint32_t wt = __builtin_amdgcn_readlane(incl, 63);
                sync_sb();
                hm_sp_flush(a, sb, wt - flushed, base + flushed, cl, lane);
                sync_sb();
            }
            mp = mp1;
            ms = ms1;
            rr ^= 1u;
            HM_ST7(3);
#if defined(HM_STAMPS) && HM_STAMPS == 7
            st7[6]++;
#endif
            /* every wave has read s_base and s_wtot before it reaches the next
             * round's first barrier, and writes them again only after it */
            __builtin_amdgcn_wave_barrier();   /* cds is free for the next round */
            if (!more) break;
        }
        if (alloc && lane == 0) s_batch = kn;   /* (read at this batch's start, before its first round's barriers) */
        hm_lds_barrier();
#if defined(HM_STAMPS) && HM_STAMPS == 7
        st7[7]++;
#endif
    }
#if defined(HM_STAMPS) && HM_STAMPS == 7
    /* wave 0 (which also makes the atomics) in row b, wave 1 in row 4096 + b */
    if (lane == 0 && wl < 2 && blockIdx.x < 4096)
        for (int q = 0; q < 8; q++) g_stamps[(blockIdx.x + wl * 4096u) * 12 + q] = st7[q];
#endif
#undef HM_ST7
}

/* one reservation for every small bucket's cells */
__global__ void k_small_reserve(HmAggArgs a)
{
    if (threadIdx.x == 0) *a.spbase = atomicAdd(a.out.cursor, (unsigned long long)*a.sptotal);
}

template <uint32_t LO, uint32_t HI>
__global__ __launch_bounds__(HM_SPW_THREADS) void k_small_emit(HmAggArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[HM_SPW_THREADS / 64][256];
    uint32_t* hw = hist[threadIdx.x >> 6];
    const uint32_t lane = hm_lane();
    const uint32_t nw = gridDim.x * (HM_SPW_THREADS / 64);
    const uint32_t zmask = hm_small_zmask(a);
    const uint64_t base = *a.spbase;
    const uint32_t wid = blockIdx.x * (HM_SPW_THREADS / 64) + (threadIdx.x >> 6);
    const uint32_t step = HmSmallMap<LO>::step(nw, a.spbatch);
    for (uint32_t s0 = HmSmallMap<LO>::first(wid, a.spbatch); HmSmallMap<LO>::bucket(s0, 0, wid, nw) < a.B.count;
         s0 += step) {
        const uint64_t bl64 = HmSmallMap<LO>::bucket(s0, lane, wid, nw);
        const bool in = HmSmallMap<LO>::lane_in(lane, a.spbatch) & (bl64 < a.B.count);
        const uint32_t bl = in ? (uint32_t)bl64 : 0u;
        const uint32_t nkl = in ? a.B.nkeys[bl] : 0u;
        const bool small = in & (LO == 0 || nkl > LO) & (nkl <= HI);
        const uint32_t kbl = small ? a.B.keybase[bl] : 0u;
        const uint64_t cl = small ? a.B.coord[bl] : 0ull;
        const uint64_t ol = small ? a.spoff[bl] : 0ull;
        uint64_t m = __ballot(small);
        if constexpr (LO == 0) {
            const uint32_t nrl = small ? a.B.nruns[bl] : 0u;
            m &= ~__ballot(small && hm_sp_fused_ok(nkl, nrl));   /* k_small_pairs' */
        }
        while (m) {
            const int i = __builtin_ctzll(m);
            m &= m - 1;
            const uint32_t nk = __shfl(nkl, i, 64), kb = __shfl(kbl, i, 64);
            const uint64_t coord = __shfl(cl, i, 64), q = base + __shfl(ol, i, 64);
            hm_small_dispatch<LO, HI>(nk, [&](auto kc) { hm_small_emit<decltype(kc)::value>(a, nk, kb, coord, zmask, q, hw); });
        }
    }
}
/* ------------------------------------------------------------------------ */
/* pooling of bucket totals: zooms z_l .. z_{l-1}+1 (root: down to 0)        */
/* ------------------------------------------------------------------------ */

__global__ __launch_bounds__(HM_POOL_THREADS) void k_pool(HmPoolArgs a)
{
    __shared__ unsigned long long v[HM_MAX_FN];
    __shared__ uint32_t scr[HM_POOL_THREADS / 64 + 1];
    __shared__ unsigned long long sbase;
    const uint32_t p = hm_block_id();
    if (p >= a.nparents) return;
    const uint32_t F = 1u << a.dbits;
    for (uint32_t i = threadIdx.x; i < F; i += HM_POOL_THREADS) v[i] = 0;
    __syncthreads();
    const uint32_t c0 = a.child_begin[p], c1 = a.child_begin[p + 1];
    for (uint32_t c = c0 + threadIdx.x; c < c1; c += HM_POOL_THREADS) v[a.child_digit[c]] = a.child_totals[c];
    __syncthreads();
    const uint64_t pm = a.parent_coord ? a.parent_coord[p] : 0ull;
    hm_pyramid<unsigned long long, HM_POOL_THREADS>(v, a.dbits / 2, a.z_child, pm, a.out, scr, &sbase);
    if (threadIdx.x == 0) {
        if (a.parent_totals) a.parent_totals[p] = v[0];
        if (a.emit_root && v[0] && a.out.zmin == 0) {
            const uint64_t pos = atomicAdd(a.out.cursor, 1ull);
            if (pos < a.out.capacity) {
                a.out.keys[pos] = hm_key(0, 0, 0);
                a.out.counts[pos] = v[0];
            }
        }
    }
}

/* k_pool for levels of <= 64 children per parent (dbits <= 6): one wavefront
 * per parent, HM_POOLW_WAVES parents per block and ONE output reservation per
 * block.  (A block per parent took one same-address cursor atomic per emitted
 * zoom -- 196K of them on the uniform cloud's z8 -> z11 level, ~2.2 ms at the
 * L2's ~88 same-address atomics per microsecond.) */
#define HM_POOLW_WAVES 16
__global__ __launch_bounds__(64 * HM_POOLW_WAVES) void k_pool_waves(HmPoolArgs a)
{
    __shared__ unsigned long long lv[HM_POOLW_WAVES][64 + 16 + 4 + 1];
    __shared__ uint32_t wtot[HM_POOLW_WAVES];
    __shared__ unsigned long long sbase;
    const uint32_t lane = hm_lane(), w = threadIdx.x >> 6;
    const uint32_t p = hm_block_id() * HM_POOLW_WAVES + w;
    const bool live = p < a.nparents;
    const int lg = a.dbits / 2;
    const uint32_t F = 1u << a.dbits;
    unsigned long long* cur = lv[w];
    if (lane < F) cur[lane] = 0;
    __builtin_amdgcn_wave_barrier();
    const uint32_t c0 = live ? a.child_begin[p] : 0u, c1 = live ? a.child_begin[p + 1] : 0u;
    if (c0 + lane < c1) cur[a.child_digit[c0 + lane]] = a.child_totals[c0 + lane];
    __builtin_amdgcn_wave_barrier();
    const uint64_t pm = (live && a.parent_coord) ? a.parent_coord[p] : 0ull;
    /* levels k = 0 .. lg-1 (zooms z_child - k), each 4^(lg-k) row-major cells,
     * stored one after another in the wave's LDS row */
    unsigned long long val[3];
    uint64_t bal[3];
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        val[k] = 0;
        bal[k] = 0;
        if (k < lg) {
            const uint32_t nk = 1u << (2 * (lg - k));
            const unsigned long long x = lane < nk ? cur[lane] : 0ull;
            const int z = a.z_child - k;
            val[k] = x;
            bal[k] = __ballot(live && z >= a.out.zmin && z <= a.out.zmax && x != 0ull);
            cnt += (uint32_t)__popcll(bal[k]);
            unsigned long long* nxt = cur + nk;
            if (lane < nk / 4) nxt[lane] = hm_sum4<unsigned long long>(cur, lane, lg - k - 1);
            __builtin_amdgcn_wave_barrier();
            cur = nxt;
        }
    }
    if (live && lane == 0 && a.parent_totals) a.parent_totals[p] = cur[0];
    if (lane == 0) wtot[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int i = 0; i < HM_POOLW_WAVES; i++) t += wtot[i];
        sbase = t ? atomicAdd(a.out.cursor, (unsigned long long)t) : 0ull;
    }
    __syncthreads();
    uint64_t base = sbase;
    for (uint32_t i = 0; i < w; i++) base += wtot[i];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (k < lg) {
            if ((bal[k] >> lane) & 1ull) {
                const uint64_t pos = base + hm_mbcnt(bal[k]);
                if (pos < a.out.capacity) {
                    a.out.keys[pos] = hm_cell_key(a.z_child - k, pm, lg - k, lane);
                    a.out.counts[pos] = val[k];
                }
            }
            base += (uint64_t)__popcll(bal[k]);
        }
    }
}

void hm_launch_aggregate(hipStream_t s, const HmAggArgs& a, uint32_t items, uint32_t nslots)
{
    if (items) hipLaunchKernelGGL(k_aggregate, hm_grid2(items), dim3(HM_AG_THREADS), 0, s, a);
    if (nslots) hipLaunchKernelGGL(k_aggregate_merged, hm_grid2(nslots), dim3(HM_AG_THREADS), 0, s, a);
}
/* HM_SPW_GRID blocks is 8 waves per SIMD, more than is resident of the
 * kernels holding > 96 SGPRs or > 64 VGPRs (k_small_pairs 7, k_small_sort 5,
 * k_small_emit 4).  A grid of only the resident blocks measured slower
 * (profiles/r6/small_grid_ab.jsonl: hotspot aggregation +50 us, z6-21 +150 us,
 * skew no better): k_small_sort / k_small_emit map buckets to waves statically,
 * and the blocks of the second round that start as the first ones drain even
 * out their uneven shares. */
static uint32_t hm_spw_grid(uint32_t wb) { return wb < HM_SPW_GRID ? wb : HM_SPW_GRID; }

void hm_launch_small(hipStream_t s, const HmAggArgs& a, uint64_t* partial)
{
    if (!a.B.count) return;
    /* batches of <= 64 consecutive buckets per wave, small enough that every
     * wave of the grid gets one when buckets are few (a wave walks its batch
     * serially) */
    HmAggArgs b = a;
    const uint32_t waves = HM_SPW_GRID * (HM_SPW_THREADS / 64);
    b.spbatch = 1;
    while (b.spbatch < 64 && (uint64_t)b.spbatch * waves < a.B.count) b.spbatch <<= 1;
    const uint32_t per_block = b.spbatch * (HM_SPW_THREADS / 64);
    const uint32_t wb = (a.B.count + per_block - 1) / per_block;
    const dim3 t(HM_SPW_THREADS), g(hm_spw_grid(wb));
    /* k_small_pairs: block batches from a counter: a grid of what fits, plus
     * spare blocks that find the counter spent */
    const uint32_t bb = b.spbatch * HM_SPP_WAVES;
    const uint32_t nbb = (a.B.count + bb - 1) / bb;
    const uint32_t gp = HM_SPW_GRID * (HM_SPW_THREADS / 64) / HM_SPP_WAVES;
    hipLaunchKernelGGL(k_small_pairs<HM_SPP_WAVES>, dim3(nbb < gp ? nbb : gp), dim3(64 * HM_SPP_WAVES), 0, s, b);
    hipLaunchKernelGGL((k_small_sort<0, HM_SPW_SPLIT>), g, t, 0, s, b);
    if (HM_SPW_MAX > HM_SPW_SPLIT) hipLaunchKernelGGL((k_small_sort<HM_SPW_SPLIT, HM_SPW_MAX>), g, t, 0, s, b);
    hm_launch_scan(s, b.spcnt, b.B.count, partial, (uint64_t*)b.spoff, b.sptotal);
    hipLaunchKernelGGL(k_small_reserve, dim3(1), dim3(64), 0, s, b);
    hipLaunchKernelGGL((k_small_emit<0, HM_SPW_SPLIT>), g, t, 0, s, b);
    if (HM_SPW_MAX > HM_SPW_SPLIT) hipLaunchKernelGGL((k_small_emit<HM_SPW_SPLIT, HM_SPW_MAX>), g, t, 0, s, b);
}
void hm_launch_pool(hipStream_t s, const HmPoolArgs& a, uint32_t nparents)
{
    if (!nparents) return;
    if (!a.emit_root && a.dbits <= 6)
        hipLaunchKernelGGL(k_pool_waves, hm_grid2((nparents + HM_POOLW_WAVES - 1) / HM_POOLW_WAVES),
                           dim3(64 * HM_POOLW_WAVES), 0, s, a);
    else
        hipLaunchKernelGGL(k_pool, hm_grid2(nparents), dim3(HM_POOL_THREADS), 0, s, a);
}
