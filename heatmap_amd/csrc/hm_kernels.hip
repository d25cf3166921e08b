/* gfx950 kernels of the heatmap hot path: level 1 and the levels >= 2 here,
 * k_aggregate, the small-bucket kernels and k_pool in hm_aggregate.hip (the
 * path: see hm_pipeline.h). */
#include <hip/hip_runtime.h>
#include "hm_genkey.h"
#include "hm_device.h"
#include "hm_project.h"
#include "hm_pipeline.h"
#define HM_STAMP_MODES(m) ((m) >= 1 && (m) <= 4)
#include "hm_stamps.h"
#include "hm_runs.h"

#define HM_YTAB_N (HM_YTAB_ROWS * HM_YTAB_STRIDE)
__constant__ double c_ytab[HM_YTAB_N] = HM_YTAB_INIT;

__device__ __forceinline__ void hm_load_ytab(double* tab)
{
    for (int i = threadIdx.x; i < HM_YTAB_N; i += blockDim.x) tab[i] = c_ytab[i];
}

/* ------------------------------------------------------------------------ */
/* projection API kernel (hm_project)                                        */
/* ------------------------------------------------------------------------ */

__global__ __launch_bounds__(256) void k_project(const double* __restrict__ lat, const double* __restrict__ lon,
                                                 int64_t n, int zoom, int64_t* __restrict__ row,
                                                 int64_t* __restrict__ col, uint8_t* __restrict__ status,
                                                 unsigned long long* err_word, unsigned long long* slow_count)
{
    __shared__ double tab[HM_YTAB_N];
    hm_load_ytab(tab);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        int64_t r = 0, c = 0;
        int slow = 0;
        int st = hm_project_point(lat[i], lon[i], zoom, &r, &c, &slow, tab);
        if (HM_UNLIKELY(st == HM_E_RANGE)) {
            /* the row projected (its errors come first), the column is beyond
             * int64: return it exactly, as an integer-valued double */
            if (hm_row(lat[i], zoom, &r, &slow, tab) == HM_OK) {
                c = __double_as_longlong(floor((lon[i] + 180.0) / 360.0 * hm_exp2i(zoom)));
                st = HM_BIGCOL;
            }
        }
        const bool good = st == HM_OK || st == HM_BIGCOL;
        row[i] = good ? r : 0;
        col[i] = good ? c : 0;
        status[i] = (uint8_t)st;
        if (HM_UNLIKELY(!good)) atomicMin(err_word, ((unsigned long long)i << 8) | (unsigned long long)st);
        const uint64_t sm = __ballot(slow);
        if (sm && hm_lane() == __ffsll((unsigned long long)sm) - 1) atomicAdd(slow_count, (unsigned long long)__popcll(sm));
    }
}

/* wave-aggregated append to the exotic list (every lane of the wave calls) */
__device__ __forceinline__ void hm_exotic_append(const HmExotic& x, bool p, int64_t r, int64_t c, int64_t i)
{
    const uint64_t m = __ballot(p);
    if (!m) return;
    const int lead = __ffsll((unsigned long long)m) - 1;
    unsigned long long b = 0;
    if (hm_lane() == lead) b = atomicAdd(x.count, (unsigned long long)__popcll(m));
    b = __shfl(b, lead, 64);
    const uint64_t q = b + hm_mbcnt(m);
    if (p && q < x.cap) {
        x.row[q] = r;
        x.col[q] = c;
        x.idx[q] = i;
    }
}


/* a value the compiler must recompute where it is used (keeps per-lane
 * 64-bit addresses from being hoisted out of a loop and spilled) */
__device__ __forceinline__ uint32_t hm_opaque(uint32_t x)
{
    asm volatile("" : "+v"(x));
    return x;
}

/* every x[k] materialised at this point, as ONE opaque statement: LDS reads
 * issued before it are all waited for with a single s_waitcnt, and none can
 * sink below it (k_l1_fast's copy-out) */
#define HM_PIN16(x)                                                                                                   \
    "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), "+v"(x[8]),       \
        "+v"(x[9]), "+v"(x[10]), "+v"(x[11]), "+v"(x[12]), "+v"(x[13]), "+v"(x[14]), "+v"(x[15])
template <int N>
__device__ __forceinline__ void hm_pin_all(uint32_t (&x)[N])
{
    if constexpr (N == 16) {
        asm volatile("" : HM_PIN16(x));
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) asm volatile("" : "+v"(x[k]));
    }
}
/* ... and one more value with them */
template <int N>
__device__ __forceinline__ void hm_pin_all(uint32_t (&x)[N], uint32_t& y)
{
    if constexpr (N == 16) {
        asm volatile("" : HM_PIN16(x), "+v"(y));
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) asm volatile("" : "+v"(x[k]));
        asm volatile("" : "+v"(y));
    }
}

/* the point stream: 16 GB per 1e9 points read once, with the non-temporal
 * hint so it does not push level 1's partly written key lines out of L2
 * (each region line fills over many tiles; evicted early, it is written back
 * several times) */
typedef double hm_d2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 hm_stream_load2(const double2* p)
{
    const hm_d2v v = __builtin_nontemporal_load((const hm_d2v*)p);
    return make_double2(v.x, v.y);
}

/* hot-tile lookup of zoom-zb tile (rs, cs) in the LDS table image: h when the
 * tile is hot, >= 2^16 otherwise (hm_pipeline.h) */
__device__ __forceinline__ uint32_t hm_hot_find(const uint2* tab, uint32_t rs, uint32_t cs)
{
    const uint2 e = tab[hm_hot_bucket(rs, cs)];
    const uint32_t tk = rs << HM_HOT_TAG;
    return min(e.x ^ tk, e.y ^ tk);
}

/* ------------------------------------------------------------------------ */
/* level 1: projection fused with the first partition                        */
/* ------------------------------------------------------------------------ */

template <typename OutT, int MODE, bool FULL>
__global__ __launch_bounds__(HM_P1_THREADS, HM_P1_WAVES) void k_project_partition(HmPart1Args a)
{
    __shared__ uint32_t cur[HM_D1 + 64];   /* + 64 dummy words (hm_lds_count) */
    /* the staged keys; until the projection is done it holds the hot-tile hash */
    __shared__ __attribute__((aligned(16))) OutT stage[HM_T1 + 64];
    /* digit of each staged key; until the count is done it holds each
     * digit's region (base, capacity << 1 | sharded) for this tile */
    __shared__ __attribute__((aligned(8))) uint16_t sdig[HM_T1 + 64];
    __shared__ unsigned long long scr[HM_P1_THREADS / 64 + 1];
    /* the projection's polynomial table; after the projection it holds, per
     * digit, (region position - stage offset) */
    __shared__ double tab[HM_YTAB_N];
    /* the hot-tile table lives in the stage and the region info in sdig when
     * they fit (8192-point tiles), else in arrays of their own */
    constexpr bool HSEP = sizeof(OutT) * HM_T1 < HM_HOT_SLOTS * 4;
    constexpr bool RSEP = sizeof(uint16_t) * HM_T1 < HM_D1 * sizeof(uint2);
    __shared__ __attribute__((aligned(16))) uint32_t hsep[HSEP ? HM_HOT_SLOTS : 4];
    __shared__ __attribute__((aligned(8))) uint2 rsep[RSEP ? HM_D1 : 1];
    static_assert(sizeof(double) * HM_YTAB_N >= HM_D1 * 4, "dbase lives in the polynomial table");
    uint4* const hsh4 = HSEP ? (uint4*)hsep : (uint4*)stage;
    uint32_t* const dbase = (uint32_t*)tab;
    uint2* const rinfo = RSEP ? rsep : (uint2*)sdig;
    constexpr bool FROM_TILES = MODE == 1;
    const int tid = threadIdx.x;
    const int F = 1 << a.dbits;
    /* hot tiles of this call (block-uniform; the count is an L2-hot word) */
    const uint32_t H = a.hot_z >= 0 ? *a.hot_n : 0u;
    const int64_t base = (a.tile0 + (int64_t)blockIdx.x) * HM_T1;   /* first input point */
    /* the resolved-redo launch is sized for the list's capacity; its length
     * is read here (no host round trip) */
    const int64_t n = (FROM_TILES && a.n_dev) ? min((int64_t)*a.n_dev, a.n) : a.n;
    if (base >= n) return;
    if (MODE == 0) HM_STAMP_M(2, 0);
    const uint32_t lim = 1u << a.Z;
    const double scale = hm_exp2i(a.Z);
    const double kz = HM_INV360 * scale;
    uint32_t dig[HM_P1_PPT];
    uint32_t rest[HM_P1_PPT];
    int nslow = 0;
    /* the polynomial table's loads go out FIRST: the barrier before the
     * projection waits for them (vmcnt retires in issue order), and must not
     * wait for the tile's 128 KB of points -- the projection then starts as
     * soon as the first points land */
    constexpr bool FULLT = FULL && !FROM_TILES;   /* a whole tile of lat/lon input */
    double2 la[HM_P1_PPT / 2], lo[HM_P1_PPT / 2];
    uint32_t kp[HM_P1_PPT / 2];   /* keep bytes of 2 points (u32: no packing, no early wait) */
    if (FULLT) {
        /* keep bytes first of all: consumed before the points */
        if (a.keep) {
            const uint16_t* kp2 = (const uint16_t*)(a.keep + base);
#pragma unroll
            for (int k = 0; k < HM_P1_PPT / 2; k++) kp[k] = kp2[k * HM_P1_THREADS + tid];
        } else {
#pragma unroll
            for (int k = 0; k < HM_P1_PPT / 2; k++) kp[k] = 0x0101;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    constexpr int TPT = (HM_YTAB_N + HM_P1_THREADS - 1) / HM_P1_THREADS;
    double tv[TPT];
    if (!FROM_TILES) {
#pragma unroll
        for (int q = 0; q < TPT; q++) {
            const int i = q * HM_P1_THREADS + tid;
            tv[q] = i < HM_YTAB_N ? c_ytab[i] : 0.0;
        }
    }
    /* this thread's digits' region slots, capacities and bases (small, L2-hot
     * tables), also before the points, and without a dependent load: a hot
     * digit's slot is d*8 + (block & 7), a cold one's d*8 (smask 7 or 0), so
     * both candidates are fetched and the mask picks one later.  (Waiting for
     * the mask before the dependent loads would wait for every point load
     * issued before it.) */
    constexpr int PERD = HM_D1 / HM_P1_THREADS;
    static_assert(HM_D1 % HM_P1_THREADS == 0, "digit slots per thread");
    /* digit slot d is live: a cold digit (d < F) or one of the H hot tiles */
    auto live = [&](int d) { return d < F || (d >= HM_MAX_F1 && (uint32_t)(d - HM_MAX_F1) < H); };
    uint32_t smk[PERD], rcap2[PERD][2], rbase2[PERD][2];
#pragma unroll
    for (int q = 0; q < PERD; q++) {
        const int d = q * HM_P1_THREADS + tid;
        const uint32_t s0 = hm_l1i(d, 0), s1 = hm_l1i(d, blockIdx.x & (HM_L1_SHARDS - 1));
        const bool lv = live(d);
        smk[q] = lv ? a.smask[d] : 0u;
        rcap2[q][0] = lv ? a.rcap[s0] : 0u;
        rcap2[q][1] = lv ? a.rcap[s1] : 0u;
        rbase2[q][0] = lv ? a.rbase[s0] : 0u;
        rbase2[q][1] = lv ? a.rbase[s1] : 0u;
    }
    /* the hot-tile table, also ahead of the points (stored to LDS below) */
    constexpr int HV = HM_HOT_SLOTS / 4 / HM_P1_THREADS;
    static_assert(HM_HOT_SLOTS == 4 * HV * HM_P1_THREADS, "the table is HV uint4 per thread");
    uint4 hv[HV];
#pragma unroll
    for (int j = 0; j < HV; j++) hv[j] = H ? ((const uint4*)a.hot_hash)[j * HM_P1_THREADS + tid] : make_uint4(0u, 0u, 0u, 0u);
    __builtin_amdgcn_sched_barrier(0);
    /* issue every load of the tile before any arithmetic: 16 points x 16 B per
     * lane in flight (double2 = two consecutive points of one array).  Full
     * tiles are a launch of their own (FULL): straight-line loads, so the
     * table's wait below counts exactly the loads issued after it; the tail
     * tile's per-lane code would make the compiler drain everything there. */
    if (FULLT) {
        const double2* lat2 = (const double2*)(a.lat + base);
        const double2* lon2 = (const double2*)(a.lon + base);
#pragma unroll
        for (int k = 0; k < HM_P1_PPT / 2; k++) {
            la[k] = lat2[k * HM_P1_THREADS + tid];
            lo[k] = lon2[k * HM_P1_THREADS + tid];
        }
    } else
#pragma unroll
    for (int k = 0; k < HM_P1_PPT / 2; k++) {
        const int64_t i0 = base + 2 * ((int64_t)k * HM_P1_THREADS + tid);
        kp[k] = 0x0101;
        if (i0 + 1 < n) {
            if (FROM_TILES) {
                la[k].x = __longlong_as_double(a.rows_in[i0]);
                la[k].y = __longlong_as_double(a.rows_in[i0 + 1]);
                lo[k].x = __longlong_as_double(a.cols_in[i0]);
                lo[k].y = __longlong_as_double(a.cols_in[i0 + 1]);
            } else {
                la[k] = *(const double2*)(a.lat + i0);
                lo[k] = *(const double2*)(a.lon + i0);
            }
            if (a.keep) kp[k] = (uint16_t)a.keep[i0] | ((uint16_t)a.keep[i0 + 1] << 8);
        } else if (i0 < n) {
            if (FROM_TILES) {
                la[k].x = __longlong_as_double(a.rows_in[i0]);
                lo[k].x = __longlong_as_double(a.cols_in[i0]);
            } else {
                la[k].x = a.lat[i0];
                lo[k].x = a.lon[i0];
            }
            la[k].y = 0.0;
            lo[k].y = 0.0;
            if (a.keep) kp[k] = (uint16_t)a.keep[i0];
        } else {
            la[k] = make_double2(0.0, 0.0);
            lo[k] = make_double2(0.0, 0.0);
        }
    }
    /* LDS set-up after the loads are issued */
    for (int i = tid; i < HM_D1; i += HM_P1_THREADS) cur[i] = 0;
    /* this tile's region of each digit: the registers are free again for
     * the projection, the count reads it back */
#pragma unroll
    for (int q = 0; q < PERD; q++) {
        const int d = q * HM_P1_THREADS + tid;
        const uint32_t sh = smk[q] != 0;
        rinfo[d] = make_uint2(sh ? rbase2[q][1] : rbase2[q][0], ((sh ? rcap2[q][1] : rcap2[q][0]) << 1) | sh);
    }
    if (H) {
#pragma unroll
        for (int j = 0; j < HV; j++) hsh4[j * HM_P1_THREADS + tid] = hv[j];
    }
    if (!FROM_TILES) {
#pragma unroll
        for (int q = 0; q < TPT; q++) {
            const int i = q * HM_P1_THREADS + tid;
            if (i < HM_YTAB_N) tab[i] = tv[q];
        }
    }
    __syncthreads();
    if (MODE == 0) HM_STAMP_M(2, 1);
    /* fast path for every point, branch-free; points the fast path cannot
     * settle (guard band, polar/out-of-range/non-finite input) are marked in
     * `redo` and resolved afterwards in one ballot-guarded pass */
    const int hb = a.restbits >> 1;      /* offset bits per coordinate in rest */
    const int wd = a.dbits >> 1;         /* digit bits per coordinate */
    const uint32_t lowm = (1u << hb) - 1u;
    const int hs = a.Z - a.hot_z;        /* hot keys: offset bits per coordinate */
    const uint32_t hm = (1u << hs) - 1u;
    /* a tile's digit slot (the skewed LDS slot of its digit, hm_cur_slot: one
     * bijection used for every digit table of the block) and key.  A point in
     * a hot tile (one 16-B read of its table bucket: the entry's tile bits
     * cancel in the XOR, so the minimum is h exactly when the tile is there)
     * takes digit HM_MAX_F1 + h and its zoom-Z offset inside the tile. */
    const uint32_t wm = (1u << wd) - 1u;
    auto key_of = [&](uint32_t r, uint32_t c, bool v, uint32_t& dslot, uint32_t& key) {
        const uint32_t rd = r >> hb, cd = c >> hb;
        /* = hm_dslot(rd << wd | cd): the column digit rotated by 8 rows */
        uint32_t dg = (rd << wd) | (HM_SKEW_CUR ? ((cd + (rd << 3)) & wm) : cd);
        key = ((r & lowm) << hb) | (c & lowm);
        if (H) {   /* block-uniform */
            const uint32_t x = hm_hot_find((const uint2*)hsh4, r >> hs, c >> hs);
            const bool hot = x < (uint32_t)HM_HOT_LIMIT;   /* a miss leaves x >= 2^16 */
            dg = hot ? HM_MAX_F1 + x : dg;
            key = hot ? (((r & hm) << hs) | (c & hm)) : key;
        }
        dslot = v ? dg : 0xFFFFFFFFu;
    };
    uint32_t redo = 0;
#pragma unroll
    for (int k = 0; k < HM_P1_PPT; k++) {
        const int64_t i = base + 2 * ((int64_t)(k >> 1) * HM_P1_THREADS + tid) + (k & 1);
        const double pa = (k & 1) ? la[k >> 1].y : la[k >> 1].x;
        const double po = (k & 1) ? lo[k >> 1].y : lo[k >> 1].x;
        int64_t r, c;
        int ok;
        bool dom;
        if (FROM_TILES) {
            r = __double_as_longlong(pa);
            c = __double_as_longlong(po);
            ok = 1;
            dom = ((uint64_t)r < lim) & ((uint64_t)c < lim);
        } else {
            int32_t r32, c32;
            ok = hm_project_fast(pa, po, scale, kz, &r32, &c32, tab);
            r = r32;
            c = c32;
            dom = true;   /* ok implies 0 <= r32, c32 < 2^Z (hm_project_fast) */
        }
        const bool inb = FULLT || i < n;   /* a whole tile is in range */
        const bool kept = ((kp[k >> 1] >> (8 * (k & 1))) & 0xFF) != 0;
        redo |= (uint32_t)(inb & !(ok & dom)) << k;
        const bool v = inb & ok & dom & kept;
        key_of((uint32_t)r, (uint32_t)c, v, dig[k], rest[k]);
        /* pin the key: without it the compiler keeps every point's
         * projection temporaries alive past this point (158 VGPRs, 1 block/CU) */
        asm volatile("" : "+v"(dig[k]), "+v"(rest[k]));
        /* one point at a time: interleaving all eight projections would need
         * ~200 VGPRs and halve occupancy */
        if ((k % HM_P1_ILP) == HM_P1_ILP - 1) __builtin_amdgcn_sched_barrier(0);
    }
    if (MODE == 0) HM_STAMP_M(2, 2);
    if (MODE == 0) {
        /* defer: k_redo resolves these with the exact chain and feeds them
         * back as extra tiles (keeps the exact path out of this kernel's
         * register allocation) */
        if (__ballot(redo != 0))
#pragma unroll
        for (int k = 0; k < HM_P1_PPT; k++) {
            const bool rd = (redo >> k) & 1u;
            const uint64_t m = __ballot(rd);
            if (m) {
                uint64_t b = 0;
                if (hm_lane() == __ffsll((unsigned long long)m) - 1) b = atomicAdd(a.redo_count, (unsigned long long)__popcll(m));
                b = __shfl(b, __ffsll((unsigned long long)m) - 1, 64);
                const uint64_t q = b + hm_mbcnt(m);
                if (rd && q < a.redo_cap)
                    a.redo_idx[q] = (uint32_t)(base + 2 * ((int64_t)(k >> 1) * HM_P1_THREADS + tid) + (k & 1));
            }
        }
        nslow = __popc(redo);
    } else if (__ballot(redo != 0)) {
        /* every lane runs each step (the exotic append is a wave operation) */
#pragma unroll
        for (int k = 0; k < HM_P1_PPT; k++) {
            const bool rd = (redo >> k) & 1u;
            const int64_t i = base + 2 * ((int64_t)(k >> 1) * HM_P1_THREADS + tid) + (k & 1);
            int64_t r = 0, c = 0;
            int st = HM_OK;
            if (rd) {
                const double pa = (k & 1) ? la[k >> 1].y : la[k >> 1].x;
                const double po = (k & 1) ? lo[k >> 1].y : lo[k >> 1].x;
                if (FROM_TILES) {
                    r = __double_as_longlong(pa);
                    c = __double_as_longlong(po);
                } else {
                    /* the literal reference chain (tile.py:17,21), row before column */
                    st = hm_row_exact(pa, a.Z, &r);
                    if (st == HM_OK) st = hm_col_exact(po, a.Z, &c);
                    nslow++;
                }
            }
            const bool kept = ((kp[k >> 1] >> (8 * (k & 1))) & 0xFF) != 0;
            if (rd && st != HM_OK) atomicMin(a.err_word, ((unsigned long long)i << 8) | (unsigned long long)st);
            const bool good = rd & (st == HM_OK) & kept;
            const bool outside = good & (((uint64_t)r >= lim) | ((uint64_t)c >= lim));
            hm_exotic_append(a.x, outside, r, c, i);
            if (good & !outside) key_of((uint32_t)r, (uint32_t)c, true, dig[k], rest[k]);
        }
    }
    if (!FROM_TILES) {
        const uint32_t ws = hm_wave_sum((uint32_t)nslow);
        if (hm_lane() == 0 && ws) atomicAdd(a.slow_count, (unsigned long long)ws);
    }
    /* one returning atomic per point: the digit histogram and the point's
     * rank within its digit (its slot is the digit's offset + rank) */
    const uint32_t dummy = HM_D1 + (uint32_t)hm_lane();
    uint32_t rank[HM_P1_PPT];
#pragma unroll
    for (int k0 = 0; k0 < HM_P1_PPT; k0 += HM_P1_GROUP) {
        HmClaim gm[HM_P1_GROUP];
        uint32_t old[HM_P1_GROUP];
#pragma unroll
        for (int u = 0; u < HM_P1_GROUP; u++) {
            gm[u] = hm_claim_prep(dig[k0 + u], dig[k0 + u] != 0xFFFFFFFFu, dummy);
            old[u] = atomicAdd(&cur[gm[u].idx], gm[u].inc);
        }
#pragma unroll
        for (int u = 0; u < HM_P1_GROUP; u++) rank[k0 + u] = hm_claim_pos(gm[u], old[u]);
    }
    __syncthreads();
    if (MODE == 0) HM_STAMP_M(2, 3);
    /* reserve each digit's keys in its region (one returning atomic per
     * non-empty digit), issued as soon as the histogram is known; the results
     * are consumed only after the scan and the claim below, so the atomic
     * latency hides behind LDS work */
    constexpr int PER = PERD;
    uint32_t cnt[PER];
    uint32_t gpos[PER];
    uint32_t rcap[PER], rbase[PER], dsl[PER];
    /* thread t holds digits q * T + t: a wave's lanes reserve for
     * consecutive digits (coalesced atomics on the shard-major fill words) */
    uint32_t tsum = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * HM_P1_THREADS + tid;
        const uint2 ri = rinfo[d];
        rbase[q] = ri.x;
        rcap[q] = ri.y >> 1;
        dsl[q] = hm_dslot(d, wd);
        const uint32_t slot = hm_l1i(d, (ri.y & 1u) ? (blockIdx.x & (HM_L1_SHARDS - 1)) : 0u);
        cnt[q] = live(d) ? cur[dsl[q]] : 0u;
        gpos[q] = 0;
        if (cnt[q]) gpos[q] = atomicAdd(&a.fill[slot], cnt[q]);
        tsum += cnt[q];
    }
    /* stage ranges in thread order (a thread's digits q = 0.. adjacent): one
     * 32-bit block scan.  Any disjoint ranges do: the copy-out finds each
     * staged key's region through its digit slot */
    uint32_t total;
    uint32_t offq[PER];
    offq[0] = hm_block_excl_scan<HM_P1_THREADS>(tsum, (uint32_t*)scr, &total);
#pragma unroll
    for (int q = 1; q < PER; q++) offq[q] = offq[q - 1] + cnt[q - 1];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * HM_P1_THREADS + tid;
        if (live(d)) cur[dsl[q]] = offq[q];
    }
    __syncthreads();
    if (MODE == 0) HM_STAMP_M(2, 4);
#pragma unroll
    for (int k = 0; k < HM_P1_PPT; k++) {
        const bool v = dig[k] != 0xFFFFFFFFu;
        const uint32_t pos = v ? cur[v ? dig[k] : 0u] + rank[k] : HM_T1 + hm_lane();
        stage[pos] = (OutT)rest[k];
        sdig[pos] = (uint16_t)dig[k];
    }
    /* lane-parallel copy-out: staged key i of digit slot s goes to region
     * position dbase[s] + i (= rbase + gpos + i - offset of its digit), so a
     * wave stores 64 consecutive staged keys (one or a few digits' runs).  A
     * reservation past the region's capacity is dropped and flagged (the host
     * re-runs the level with exact sizes). */
    bool over = false;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * HM_P1_THREADS + tid;
        if (live(d)) {
            const bool fits = cnt[q] && (uint64_t)gpos[q] + cnt[q] <= (uint64_t)rcap[q];
            over |= cnt[q] && !fits;
            dbase[dsl[q]] = fits ? rbase[q] + gpos[q] - offq[q] : 0xFFFFFFFFu;
        }
    }
    if (MODE == 0) HM_STAMP_M(2, 5);
    if (over) atomicOr(a.overflow, 1ull);
    __syncthreads();
    if (MODE == 0) HM_STAMP_M(2, 6);
    {
        /* every LDS read first (a thread copies <= HM_P1_PPT staged keys),
         * then the stores: no load-use round trip per key */
        OutT* out = (OutT*)a.keys_out;
        uint16_t* hout = (uint16_t*)a.keys_hot;
        uint32_t* hout32 = (uint32_t*)a.keys_hot;   /* mid-level hot tiles (a.hot_bytes 4) */
        uint32_t sv[HM_P1_PPT], sl[HM_P1_PPT], sb[HM_P1_PPT];
#pragma unroll
        for (int j = 0; j < HM_P1_PPT; j++) {
            const uint32_t i = j * HM_P1_THREADS + tid;
            const uint32_t ic = i < total ? i : 0u;
            sl[j] = sdig[ic];
            sv[j] = (uint32_t)stage[ic];
        }
#pragma unroll
        for (int j = 0; j < HM_P1_PPT; j++) sb[j] = dbase[sl[j]];
#pragma unroll
        for (int j = 0; j < HM_P1_PPT; j++) {
            const uint32_t i = j * HM_P1_THREADS + tid;
            if (i < total && sb[j] != 0xFFFFFFFFu) {
                if (sl[j] < HM_MAX_F1)
                    out[sb[j] + i] = (OutT)sv[j];
                else if (a.hot_bytes == 4)
                    hout32[sb[j] + i] = sv[j];
                else
                    hout[sb[j] + i] = (uint16_t)sv[j];
            }
        }
    }
    if (MODE == 0) HM_STAMP_M(2, 7);
}

/* ------------------------------------------------------------------------ */
/* level 1, whole lat/lon tiles (the hot launch of every hm_count call)      */
/* ------------------------------------------------------------------------ */
/* k_l1_fast: the same level-1 pass as k_project_partition<OutT, 0, true> --
 * the same regions, reservations, keys and deferred points -- with the
 * per-point instruction budget cut (round 4):
 *
 *  projection  v_fract_f64 gives each coordinate's fraction in one op and the
 *              floor is a truncating convert (both coordinates are positive on
 *              the accepted range); the column is one fma (lon * kz + 180 kz,
 *              inside the same 2^-49 guard); the column range test is
 *              |lon| < 180 on the input (an accepted y lies in [0, 2^z));
 *  hot lookup  row-tagged 2-way buckets (hm_hot_find): the tile's row and
 *              column are shifts of the point's, no tile id is built, and the
 *              digit is ONE min3 over (way 0, way 1, cold slot) because hot
 *              tiles take the LOW slots [0, HM_MAX_HOT) of this kernel's
 *              numbering and cold digits the slots above;
 *  count+rank  one plain returning LDS atomic per point; lanes are grouped on
 *              lane 0's slot only when a wave-uniform test finds >=
 *              HM_L1_MERGE_MIN of them (skewed clouds), so a hotspot wave pays
 *              two VALU ops per point for the test;
 *  staging     each staged entry is (key, destination position): the copy-out
 *              reads one 8-B LDS word per key and needs no per-digit lookup;
 *              the stage holds the cold keys first and the hot keys after them
 *              (one packed 16|16-bit block scan), so the copy-out's two store
 *              kinds are wave-uniform; hot keys are staged in the cold layout
 *              and narrowed to their zb-relative u16 form in the copy-out.
 *
 * Internal slot s: hot tile h -> s = h; cold z1 digit d -> s = HM_MAX_HOT +
 * hm_dslot(d) (the bank-skewed slot).  Thread t owns slots q * T + t. */
#ifndef HM_L1_MERGE_MIN
#define HM_L1_MERGE_MIN 6
#endif
#define HM_L1_SLOTS (HM_MAX_HOT + HM_MAX_F1)
#define HM_L1_CW 1600                       /* slot words (>= HM_L1_SLOTS + 64 dummies), a multiple of 64 */
static_assert(HM_L1_CW >= HM_L1_SLOTS + 64 && HM_L1_CW % 64 == 0, "count and delta words pair as read2st64");
static_assert(HM_L1_SLOTS % HM_P1_THREADS == 0, "slots per thread");

#ifndef HM_L1_WAVES
#define HM_L1_WAVES 4                       /* k_l1_fast: waves per SIMD its registers allow (4: 2 blocks of 8 waves per CU) */
#endif

/* k_l1_fast's slot -> level-1 digit (hot slot h: digit HM_MAX_F1 + h; cold
 * slot: the bank skew undone), wd = dbits / 2 */
__device__ __forceinline__ uint32_t hm_l1_slot_digit(uint32_t sl, int wd)
{
    if (sl < HM_MAX_HOT) return HM_MAX_F1 + sl;
    const uint32_t u = sl - HM_MAX_HOT, m = (1u << wd) - 1u;
    return HM_SKEW_CUR ? ((u & ~m) | ((u - ((u >> wd) << 3)) & m)) : u;
}
__device__ __forceinline__ bool hm_l1_slot_live(uint32_t sl, uint32_t H, uint32_t F)
{
    return sl < HM_MAX_HOT ? sl < H : (sl - HM_MAX_HOT) < F;
}

/* the slot table of one call (hm_pipeline.h): 8 x 1536 entries,
 * what every one of k_l1_fast's blocks used to work out for itself from
 * rbase, rcap and smask with five dependent scattered loads per slot */
__global__ __launch_bounds__(256) void k_l1_slots(HmPart1Args a, uint4* __restrict__ tab)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x, b = blockIdx.y;
    if (sl >= HM_D1) return;
    const uint32_t H = a.hot_z >= 0 ? min(*a.hot_n, (uint32_t)HM_MAX_HOT) : 0u;
    uint4 e = make_uint4(0u, 0u, 0u, 0u);
    if (hm_l1_slot_live(sl, H, 1u << a.dbits)) {
        const uint32_t d = hm_l1_slot_digit(sl, a.dbits >> 1);
        const uint32_t i = hm_l1i(d, a.smask[d] != 0 ? b : 0u);
        e = make_uint4(a.rbase[i], a.rcap[i], i, 0u);
    }
    tab[b * HM_D1 + sl] = e;
}

void hm_launch_l1_slots(hipStream_t s, const HmPart1Args& a)
{
    static_assert(HM_D1 == HM_MAX_HOT + HM_MAX_F1, "the table's rows are k_l1_fast's slots");
    hipLaunchKernelGGL(k_l1_slots, dim3((HM_D1 + 255) / 256, HM_L1_SHARDS), dim3(256), 0, s, a, (uint4*)a.l1slot);
}
template <typename OutT, bool KEEP>
__global__ __launch_bounds__(HM_P1_THREADS) __attribute__((amdgpu_waves_per_eu(HM_L1_WAVES, HM_L1_WAVES))) void
k_l1_fast(HmPart1Args a)
{
    /* staged (key, destination), + one pad entry per lane for points that
     * stage nothing; during the projection its first 32 KB hold the
     * polynomial table and the hot-tile table */
    __shared__ __attribute__((aligned(16))) uint2 ent[HM_T1 + 64];
    /* per slot: count (atomics) then stage offset in [0, CW); destination minus
     * stage position in [CW, 2 CW) -- one ds_read2st64_b32 reads both */
    __shared__ uint32_t cw[2 * HM_L1_CW];
    __shared__ uint32_t scr[HM_P1_THREADS / 64 + 1];
    __shared__ uint32_t s_over;
    /* the polynomial table plus one poison row (HM_YTAB_ROWS, NaN
     * coefficients) that the clamped index of |lat| > 90, NaN and inf lands
     * on.  Points with 85.05 < |lat| <= 90 are rejected by the latitude test
     * (an accepted point has Y in (0, 1), 0 < R < 2^Z).  (Poisoning the table
     * down to |lat| > 85 instead saves that test but sends 0.06% of a uniform
     * cloud to the exact path: 46x the deferred points, on one counter.) */
    constexpr int YROWS = HM_YTAB_ROWS + 1;
    constexpr int YN = YROWS * HM_YTAB_STRIDE;
    static_assert(sizeof(double) * YN <= 16384 && HM_HOT_SLOTS * 4 <= 16384, "tables fit the stage");
    double* const tab = (double*)ent;
    uint2* const hot2 = (uint2*)((char*)ent + 16384);
    const int tid = threadIdx.x;
    const uint32_t H = a.hot_z >= 0 ? *a.hot_n : 0u;
    const int64_t base = (a.tile0 + (int64_t)blockIdx.x) * HM_T1;
    HM_STAMP_M(4, 0);
    const double scale = hm_exp2i(a.Z);
    const double nscale = -scale, hscale = 0.5 * scale;
    const double kz = HM_INV360 * scale;
    const double c180 = 180.0 * kz;
    const double ghalf = 0.5 - HM_Y_EPS * scale;       /* row: |frac - 1/2| < ghalf */
    const double ghalf2 = 0.5 - scale * 0x1p-49;       /* column */
    constexpr int PERD = HM_L1_SLOTS / HM_P1_THREADS;
    const int wd = a.dbits >> 1;
    /* no liveness test anywhere.  A point's slot is a dummy, a hot tile the
     * table holds (h < H) or the cold slot of its own digit (< F: an accepted
     * point has r, c < 2^Z), so a dead slot's count word stays 0: it reserves
     * nothing, its zero capacity fits its zero count, and the stage offset
     * and delta it writes to its own words are never read */
    /* keep bytes, then the tables, then the points (vmcnt retires in order) */
    uint32_t kp[HM_P1_PPT / 2];   /* KEEP: the keep bytes (a keep-less call compiles the test away) */
    if (KEEP) {
        const uint16_t* kp2 = (const uint16_t*)(a.keep + base);
#pragma unroll
        for (int k = 0; k < HM_P1_PPT / 2; k++) kp[k] = kp2[k * HM_P1_THREADS + tid];
    } else {
#pragma unroll
        for (int k = 0; k < HM_P1_PPT / 2; k++) kp[k] = 0x0101;
    }
    __builtin_amdgcn_sched_barrier(0);
    constexpr int TPT = (YN + HM_P1_THREADS - 1) / HM_P1_THREADS;
    double tv[TPT];
#pragma unroll
    for (int q = 0; q < TPT; q++) {
        const int i = q * HM_P1_THREADS + tid;
        tv[q] = i >= HM_YTAB_N ? __builtin_nan("") : c_ytab[i];
    }
    /* the owned slots' (base, capacity, fill index): one coalesced 16-B load
     * each; no address depends on a load, so nothing waits before the point
     * loads are out */
    uint4 st[PERD];
    {
        const uint4* const row = a.l1slot + (blockIdx.x & (HM_L1_SHARDS - 1)) * HM_L1_SLOTS;
#pragma unroll
        for (int q = 0; q < PERD; q++) st[q] = row[q * HM_P1_THREADS + tid];
    }
    constexpr int HV = HM_HOT_SLOTS / 4 / HM_P1_THREADS;
    uint4 hv[HV];
    /* no branch around the loads (the join of "loaded" and "zero" cost an
     * s_waitcnt vmcnt(0) ahead of the point loads): without hot tiles they
     * read the first 16 KB of rbase, HM_D1 * HM_L1_SHARDS words, unused */
    static_assert(HM_HOT_SLOTS <= HM_D1 * HM_L1_SHARDS, "the stand-in array holds a hot table's bytes");
    const uint4* const hsrc = H ? (const uint4*)a.hot_hash : (const uint4*)a.rbase;
#pragma unroll
    for (int j = 0; j < HV; j++) {
        const uint4 v = hsrc[j * HM_P1_THREADS + tid];
        hv[j] = make_uint4(v.x, v.y, v.z, v.w);
    }
    __builtin_amdgcn_sched_barrier(0);
    double2 la[HM_P1_PPT / 2], lo[HM_P1_PPT / 2];
    {
        const double2* lat2 = (const double2*)(a.lat + base);
        const double2* lon2 = (const double2*)(a.lon + base);
#pragma unroll
        for (int k = 0; k < HM_P1_PPT / 2; k++) {
            la[k] = hm_stream_load2(lat2 + k * HM_P1_THREADS + tid);
            lo[k] = hm_stream_load2(lon2 + k * HM_P1_THREADS + tid);
        }
    }
    for (int i = tid; i < HM_L1_CW; i += HM_P1_THREADS) cw[i] = 0;
    if (tid == 0) s_over = 0;
    if (H) {
#pragma unroll
        for (int j = 0; j < HV; j++) ((uint4*)hot2)[j * HM_P1_THREADS + tid] = hv[j];
    }
#pragma unroll
    for (int q = 0; q < TPT; q++) {
        const int i = q * HM_P1_THREADS + tid;
        if (i < YN) tab[i] = tv[q];
    }
    hm_lds_barrier();
    HM_STAMP_M(4, 1);
    const int hb = a.restbits >> 1;
    const uint32_t lowm = (1u << hb) - 1u;
    const uint32_t keym = (uint32_t)((1ull << (2 * hb)) - 1ull);
    const uint32_t wm = (1u << wd) - 1u;
    const int hs = a.hot_z >= 0 ? a.Z - a.hot_z : 0;
    const uint32_t dummy = HM_L1_SLOTS + (uint32_t)hm_lane();
    uint32_t slot[HM_P1_PPT], key[HM_P1_PPT];
    uint32_t redo = 0;
#pragma unroll
    for (int k = 0; k < HM_P1_PPT; k++) {
        const double pa = (k & 1) ? la[k >> 1].y : la[k >> 1].x;
        const double po = (k & 1) ? lo[k >> 1].y : lo[k >> 1].x;
        /* the projection's own statements: hm_project.h, compiled for the
         * CPU tests too */
        uint32_t r, c;
        const bool ok = hm_project_l1(pa, po, nscale, hscale, kz, c180, ghalf, ghalf2, tab, &r, &c);
        const bool kept = ((kp[k >> 1] >> (8 * (k & 1))) & 0xFFu) != 0;
        redo |= (uint32_t)!ok << k;
        /* cold slot: bank-skewed z1 digit above the hot slots */
        const uint32_t rd = r >> hb, cd = c >> hb;
        const uint32_t rdw = (rd << wd) + HM_MAX_HOT;
        uint32_t sl = HM_SKEW_CUR ? (((cd + (rd << 3)) & wm) | rdw) : (cd | rdw);
        if (H) sl = min(hm_hot_find(hot2, r >> hs, c >> hs), sl);   /* block-uniform */
        key[k] = ((r << hb) | (c & lowm)) & keym;
        slot[k] = (ok & kept) ? sl : dummy;
        asm volatile("" : "+v"(slot[k]), "+v"(key[k]));
        __builtin_amdgcn_sched_barrier(0);
    }
    HM_STAMP_M(4, 2);
    /* deferred points: k_redo resolves them exactly */
    if (__builtin_amdgcn_ballot_w64(redo != 0)) {
#pragma unroll
        for (int k = 0; k < HM_P1_PPT; k++) {
            const bool rd = (redo >> k) & 1u;
            const uint64_t m = __builtin_amdgcn_ballot_w64(rd);
            if (m) {
                uint64_t b = 0;
                if (hm_lane() == __ffsll((unsigned long long)m) - 1) b = atomicAdd(a.redo_count, (unsigned long long)__popcll(m));
                b = __shfl(b, __ffsll((unsigned long long)m) - 1, 64);
                const uint64_t q = b + hm_mbcnt(m);
                if (rd && q < a.redo_cap)
                    a.redo_idx[q] = (uint32_t)(base + 2 * ((int64_t)(k >> 1) * HM_P1_THREADS + tid) + (k & 1));
            }
        }
        const uint32_t ws = hm_wave_sum((uint32_t)__popc(redo));
        if (hm_lane() == 0 && ws) atomicAdd(a.slow_count, (unsigned long long)ws);
    }
    /* count + rank: one returning atomic per point; a wave whose lanes mostly
     * share lane 0's slot adds for them once (lane 0 adds the group size, the
     * rest of the group hits private dummy words) */
    uint32_t rank[HM_P1_PPT];
    uint32_t merged = 0;   /* wave-uniform: points whose atomic was grouped */
#pragma unroll
    for (int k = 0; k < HM_P1_PPT; k++) {
        const uint32_t k0 = __builtin_amdgcn_readfirstlane(slot[k]);
        const uint64_t m = __builtin_amdgcn_ballot_w64(slot[k] == k0);
        const uint32_t pm = (uint32_t)__builtin_popcount((uint32_t)m) + (uint32_t)__builtin_popcount((uint32_t)(m >> 32));
        uint32_t idx = slot[k], inc = 1u;
        if (pm >= HM_L1_MERGE_MIN) {
            merged |= 1u << k;
            const bool in = (m >> hm_lane()) & 1ull;
            idx = (in && hm_lane() != 0) ? dummy : idx;
            inc = hm_lane() == 0 ? pm : inc;
        }
        rank[k] = atomicAdd(&cw[idx], inc);
    }
    if (merged) {
#pragma unroll
        for (int k = 0; k < HM_P1_PPT; k++)
            if ((merged >> k) & 1u) {
                const uint32_t k0 = __builtin_amdgcn_readfirstlane(slot[k]);
                const uint64_t m = __builtin_amdgcn_ballot_w64(slot[k] == k0);
                const uint32_t r0 = __builtin_amdgcn_readfirstlane(rank[k]);
                if ((m >> hm_lane()) & 1ull) rank[k] = r0 + hm_mbcnt(m);
            }
    }
    hm_lds_barrier();
    HM_STAMP_M(4, 3);
    /* reservations: one returning global atomic per non-empty (digit, shard) */
    uint32_t cnt[PERD], gpos[PERD];
#pragma unroll
    for (int q = 0; q < PERD; q++) {
        const uint32_t sl = q * HM_P1_THREADS + tid;
        cnt[q] = cw[sl];
        gpos[q] = 0;
        if (cnt[q]) gpos[q] = atomicAdd(&a.fill[st[q].z], cnt[q]);
    }
    /* stage offsets: cold slots (q >= QH) first, hot slots (q < QH) after
     * them, from one scan of (cold count | hot count << 16) */
    constexpr int QH = HM_MAX_HOT / HM_P1_THREADS;
    static_assert(HM_MAX_HOT % HM_P1_THREADS == 0 && QH >= 1 && QH < PERD, "slots q < QH are the hot tiles");
    uint32_t csum = 0, hsum = 0;
#pragma unroll
    for (int q = 0; q < PERD; q++) (q < QH ? hsum : csum) += cnt[q];
    uint32_t tot2;
    const uint32_t pre = hm_block_excl_scan<HM_P1_THREADS, true>(csum | (hsum << 16), scr, &tot2);
    const uint32_t C = tot2 & 0xFFFFu, total = C + (tot2 >> 16);
    uint32_t offq[PERD];
    {
        uint32_t oc = pre & 0xFFFFu, oh = C + (pre >> 16);
#pragma unroll
        for (int q = 0; q < PERD; q++) {
            offq[q] = q < QH ? oh : oc;
            (q < QH ? oh : oc) += cnt[q];
        }
    }
    bool over = false;
    /* a slot's destination delta: its region base + reservation - stage
     * offset; a region that overflowed: destinations >= 0xFFF00000 (no key
     * position reaches it), dropped by the copy-out */
    auto deltas = [&]() {
#pragma unroll
        for (int q = 0; q < PERD; q++) {
            const uint32_t sl = q * HM_P1_THREADS + tid;
            const uint32_t rc = st[q].y, rb = st[q].x;
            const bool fits = (uint64_t)gpos[q] + cnt[q] <= (uint64_t)rc;
            over |= cnt[q] && !fits;
            cw[HM_L1_CW + sl] = (fits ? rb + gpos[q] : 0xFFF00000u) - offq[q];
        }
        if (over) {
            atomicOr(a.overflow, 1ull);
            s_over = 1;
        }
    };
#pragma unroll
    for (int q = 0; q < PERD; q++) {
        const uint32_t sl = q * HM_P1_THREADS + tid;
        cw[sl] = offq[q];
    }
    hm_lds_barrier();
    HM_STAMP_M(4, 4);
    /* staging, branch-free: a point that stages nothing writes its lane's pad
     * entry.  The entry holds its slot, and the destination
     * deltas are written after the staging, so the reservation atomics'
     * round trip overlaps it (the copy-out looks the delta up per key) */
    /* (the compiler reads each offset under its point's select, one LDS
     * round trip per point; all 16 reads ahead of one wait measured no
     * faster: DESIGN.md 3.1, round 7) */
#pragma unroll
    for (int k = 0; k < HM_P1_PPT; k++) {
        const uint32_t o = cw[slot[k]];   /* (dummies: in range, unused) */
        const uint32_t pos = slot[k] < HM_L1_SLOTS ? o + rank[k] : HM_T1 + (uint32_t)hm_lane();
        ent[pos] = make_uint2(key[k], slot[k]);
    }
    deltas();
    hm_lds_barrier();
    HM_STAMP_M(4, 5);
    /* copy-out: a wave stores 64 consecutive staged keys -- cold keys in [0, C)
     * as OutT, hot keys in [C, total) as u16 (zb-relative); the kind tests
     * are wave-uniform except in the one wave straddling C or total */
    char* const outb = (char*)a.keys_out;
    char* const houtb = (char*)a.keys_hot;
    const uint32_t hm = (1u << hs) - 1u;
    auto put_cold = [&](uint2 e) { *(OutT*)(outb + (uint64_t)e.y * sizeof(OutT)) = (OutT)e.x; };
    const bool hot32 = a.hot_bytes == 4;   /* block-uniform */
    auto put_hot = [&](uint2 e) {
        /* (row offset, col offset) in the hot tile, from the cold key: u16 for
         * a last-level bucket tile, u32 for a mid-level one */
        const uint32_t hk = (((e.x >> hb) & hm) << hs) | (e.x & hm);
        if (hot32) *(uint32_t*)(houtb + (uint64_t)e.y * 4u) = hk;
        else *(uint16_t*)(houtb + (uint64_t)e.y * 2u) = (uint16_t)hk;
    };
    uint2 e[HM_P1_PPT];
    uint32_t sov;   /* s_over (the overflow flag rides in the delta batch) */
    /* three batches: the 16 entries, their 16 deltas, then the stores, with
     * one wait between them.  An entry past total is stale stage (table
     * words): its delta index is clamped into cw, not branched around, and
     * what it reads is never stored */
    uint32_t dl[HM_P1_PPT];
#pragma unroll
    for (int j = 0; j < HM_P1_PPT; j++) {
        e[j] = ent[j * HM_P1_THREADS + tid];
        dl[j] = e[j].y;
    }
    hm_pin_all(dl);   /* (the key comes with the slot: one 8-B read) */
#pragma unroll
    for (int j = 0; j < HM_P1_PPT; j++) dl[j] = cw[HM_L1_CW + min(dl[j], (uint32_t)(HM_L1_CW - 1))];
    sov = s_over;
    hm_pin_all(dl, sov);
    sov = __builtin_amdgcn_readfirstlane(sov);   /* block-uniform: a scalar branch, as before */
#pragma unroll
    for (int j = 0; j < HM_P1_PPT; j++) e[j].y = dl[j] + (uint32_t)(j * HM_P1_THREADS + tid);
    const uint32_t wofs = (uint32_t)tid & ~63u;
    if (!sov) {
#pragma unroll
        for (int j = 0; j < HM_P1_PPT; j++) {
            const uint32_t wb = __builtin_amdgcn_readfirstlane(j * HM_P1_THREADS + wofs);
            const uint32_t i = j * HM_P1_THREADS + tid;
            if (wb + 64 <= C) {
                put_cold(e[j]);
            } else if (wb >= C && wb + 64 <= total) {
                put_hot(e[j]);
            } else if (wb < total) {
                if (i < C) put_cold(e[j]);
                else if (i < total) put_hot(e[j]);
            }
        }
    } else {
        /* a region overflowed (the host re-runs the level with exact sizes) */
#pragma unroll
        for (int j = 0; j < HM_P1_PPT; j++) {
            const uint32_t i = j * HM_P1_THREADS + tid;
            if (i < total && e[j].y < 0xFFF00000u) {
                if (i < C) put_cold(e[j]);
                else put_hot(e[j]);
            }
        }
    }
    HM_STAMP_M(4, 6);
}

/* Sampled digit histogram of level 1 (every stride-th point, fast projection
 * only): sizes the per-digit key regions k_project_partition fills. */
#define HM_SAMPLE_HSLOTS 4096   /* per-block hash of sampled hot-zoom tiles */
template <bool FROM_TILES, bool HOT>
__global__ __launch_bounds__(256) void k_sample_digits(HmPart1Args a, uint64_t stride_pts, uint32_t* hist,
                                                       uint32_t* hot_counts)
{
    __shared__ uint32_t h[HM_MAX_F1 + 64];
    __shared__ double tab[HM_YTAB_N];
    /* HOT: the block's samples per zoom-hot_z tile, pre-aggregated in LDS
     * (a hot tile gets one global atomic per block, not one per sample) */
    __shared__ uint32_t hk[HOT ? HM_SAMPLE_HSLOTS : 1], hc[HOT ? HM_SAMPLE_HSLOTS : 1];
    const int F = 1 << a.dbits;
    for (int i = threadIdx.x; i < F; i += 256) h[i] = 0;
    if (HOT)
        for (int i = threadIdx.x; i < HM_SAMPLE_HSLOTS; i += 256) {
            hk[i] = HM_HOT_EMPTY;
            hc[i] = 0;
        }
    if (!FROM_TILES) hm_load_ytab(tab);
    __syncthreads();
    uint32_t hlost = 0;   /* samples the (full) LDS hash could not take: counted directly */
    const double scale = hm_exp2i(a.Z);
    const double kz = HM_INV360 * scale;
    const uint32_t lim = 1u << a.Z;
    const int hb = a.restbits >> 1, wd = a.dbits >> 1;
    const uint64_t m = (uint64_t)(a.n + stride_pts - 1) / stride_pts;
    const uint64_t m_up = (m + 63) & ~63ull;
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < m_up; j += step) {
        const uint64_t i = j * stride_pts;
        bool v = j < m && (!a.keep || a.keep[i]);
        int64_t r = 0, c = 0;
        if (v) {
            if (FROM_TILES) {
                r = a.rows_in[i];
                c = a.cols_in[i];
            } else {
                int32_t r32, c32;
                v = hm_project_fast(a.lat[i], a.lon[i], scale, kz, &r32, &c32, tab);
                r = r32;
                c = c32;
            }
            v = v && (uint64_t)r < lim && (uint64_t)c < lim;
        }
        const uint32_t d = ((((uint32_t)r) >> hb) << wd) | (((uint32_t)c) >> hb);
        hm_lds_count(h, HM_MAX_F1, d, v);
        if (HOT && v) {
            const int hs = a.Z - a.hot_z;
            const uint32_t t = ((((uint32_t)r) >> hs) << a.hot_z) | (((uint32_t)c) >> hs);
            uint32_t sl = (t * 2654435761u) >> (32 - 12);
            static_assert(HM_SAMPLE_HSLOTS == 1 << 12, "sample hash slots");
            /* a few probes, then the global count: a spread-out cloud (4096+
             * distinct tiles per block) fills the table, and a full scan per
             * sample took uniform clouds 1.5 ms */
            int probes = 0;
            for (;;) {
                const uint32_t o = atomicCAS(&hk[sl], HM_HOT_EMPTY, t);
                if (o == HM_HOT_EMPTY || o == t) {
                    atomicAdd(&hc[sl], 1u);
                    break;
                }
                sl = (sl + 1) & (HM_SAMPLE_HSLOTS - 1);
                if (++probes == 16) {
                    atomicAdd(&hot_counts[t], 1u);
                    hlost++;
                    break;
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < F; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
    if (HOT)
        for (int i = threadIdx.x; i < HM_SAMPLE_HSLOTS; i += 256)
            if (hc[i]) atomicAdd(&hot_counts[hk[i]], hc[i]);
    (void)hlost;
}

/* Hot-tile candidates: every zoom-zb tile with >= thresh sampled points (at
 * most HM_HOT_CAND, first come), listed with its sampled count. */
__global__ __launch_bounds__(256) void k_hot_select(HmHotArgs a)
{
    const uint64_t ntiles = 1ull << (2 * a.zb);
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint32_t* const ncand = a.cand + 2 * HM_HOT_CAND;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < ntiles; t += stride) {
        const uint32_t c = a.counts[t];
        if (c >= a.thresh) {
            const uint32_t j = atomicAdd(ncand, 1u);
            if (j < HM_HOT_CAND) {
                a.cand[2 * j] = (uint32_t)t;
                a.cand[2 * j + 1] = c;
            }
        }
    }
}

/* The hot tiles and the table image k_project_partition looks them up in.
 * The biggest candidates go first: a histogram of their sampled counts (8
 * bins per octave) gives the cutoff bin above which fewer than HM_MAX_HOT
 * candidates lie; those are placed, then the cutoff bin's first come.  A
 * candidate becomes hot tile h (< HM_MAX_HOT) when its bucket has a free way;
 * otherwise it stays cold (any set of hot tiles gives the same counts).  Hot
 * tile h: its sampled count as level-1 histogram entry HM_MAX_F1 + h, taken
 * off its z1 digit, which is flagged as a hot parent.  One block. */
__device__ __forceinline__ uint32_t hm_hot_bin(uint32_t c)
{
    const uint32_t e = 31u - __clz(c | 1u);
    return e < 3 ? c : (e << 3) | ((c >> (e - 3)) & 7u);   /* < 256 */
}

__global__ __launch_bounds__(1024) void k_hot_hash(HmHotArgs a)
{
    __shared__ uint32_t tab[HM_HOT_SLOTS];
    __shared__ uint32_t fill[HM_HOT_BUCKETS];
    __shared__ uint32_t bins[256];
    __shared__ uint32_t nh, cut;
    static_assert(HM_HOT_CAND <= 4 * 1024, "4 candidates a thread");
    const int tid = threadIdx.x;
    for (int i = tid; i < HM_HOT_SLOTS; i += 1024) tab[i] = HM_HOT_EMPTY;
    for (int i = tid; i < HM_HOT_BUCKETS; i += 1024) fill[i] = 0;
    for (int i = tid; i < 256; i += 1024) bins[i] = 0;
    if (tid == 0) nh = 0;
    /* the thread's candidates j = tid + 1024 u, read once for the three passes */
    const uint32_t nc = min(a.cand[2 * HM_HOT_CAND], (uint32_t)HM_HOT_CAND);
    uint32_t ct[4], cc[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint32_t j = tid + 1024u * u;
        const uint2 v = j < nc ? ((const uint2*)a.cand)[j] : make_uint2(0u, 0u);
        ct[u] = v.x;
        cc[u] = v.y;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; u++)
        if (tid + 1024u * u < nc) atomicAdd(&bins[hm_hot_bin(cc[u])], 1u);
    __syncthreads();
    if (tid < 64) {
        /* cutoff: the highest bin b whose candidates from the top (bins >= b)
         * reach HM_HOT_LIMIT, 0 if none -- lane l holds bins 4l .. 4l+3, the
         * bins above them a reversed-lane scan */
        const int l = tid;
        uint32_t s = 0;
        uint32_t bv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) s += (bv[k] = bins[4 * l + k]);
        const uint32_t rs = __shfl(s, 63 - l, 64);              /* lane l: the sum of lane 63 - l */
        const uint32_t incl = hm_wave_incl_scan(rs);              /* lanes 63-l .. 63 from the top */
        const uint32_t above = __shfl(incl, 62 - l < 0 ? 0 : 62 - l, 64);   /* bins of lanes > l */
        uint32_t acc = l == 63 ? 0u : above;
        int best = -1;
#pragma unroll
        for (int k = 3; k >= 0; k--) {
            acc += bv[k];
            if (best < 0 && acc >= HM_HOT_LIMIT) best = 4 * l + k;
        }
        for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
        if (l == 0) cut = best < 0 ? 0u : (uint32_t)best;
    }
    __syncthreads();
    /* pass 0: above the cutoff bin; 1: at it; 2: below it (only while hot
     * digits are left: candidates whose bucket was full leave room) */
    for (int pass = 0; pass < 3; pass++) {
        if (pass == 2 && nh >= HM_HOT_LIMIT) break;   /* (block-uniform: read after the barrier) */
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (tid + 1024u * u >= nc) continue;
            const uint32_t t = ct[u], c = cc[u];
            const uint32_t bn = hm_hot_bin(c);
            if (pass == 0 ? bn <= cut : pass == 1 ? bn != cut : bn >= cut) continue;
            const uint32_t tr = t >> a.zb, tc = t & ((1u << a.zb) - 1u);
            const uint32_t b = hm_hot_bucket(tr, tc);
            const uint32_t w = atomicAdd(&fill[b], 1u);
            if (w >= HM_HOT_WAYS) continue;
            const uint32_t h = atomicAdd(&nh, 1u);
            if (h >= HM_HOT_LIMIT) continue;   /* its way stays empty */
            tab[b * HM_HOT_WAYS + w] = (tr << HM_HOT_TAG) | h;
            a.tiles[h] = t;
            a.hist[HM_MAX_F1 + h] = c;
            const int s = a.zb - a.z1;
            const uint32_t d = ((tr >> s) << a.z1) | (tc >> s);
            a.hotparent[d] = 1;
            atomicSub(&a.hist[d], c);   /* those samples' keys leave the cold digit */
        }
        __syncthreads();
    }
    for (int i = tid; i < HM_HOT_SLOTS; i += 1024) a.hash[i] = tab[i];
    if (tid == 0) *a.n = min(nh, (uint32_t)HM_HOT_LIMIT);
}

void hm_launch_hot_select(hipStream_t s, const HmHotArgs& a)
{
    const uint64_t ntiles = 1ull << (2 * a.zb);
    uint64_t blocks = (ntiles + 4095) / 4096;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_hot_select, dim3((unsigned)blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_hot_hash, dim3(1), dim3(1024), 0, s, a);
}

/* Level-1 region sizes from the sampled histogram, on the device (no host
 * round trip): per digit est = hist * stride; a digit above 64 tiles gets
 * HM_L1_SHARDS shards; per shard cap = e + e/16 + 8 sqrt(e * stride) + 2 T1
 * (e = est / shards); bases = exclusive prefix over (digit, shard), the F
 * cold digits first, then the hot tiles' digits HM_MAX_F1 + h (h < *hot_n),
 * one position space.  The same formula as the host's retry path.  One block
 * of 1024 threads: thread t sizes cold digit t and hot digit HM_MAX_F1 + t. */
__device__ __forceinline__ uint32_t hm_l1_cap(uint32_t hist, uint64_t stride, int* ns)
{
    const double est = (double)hist * (double)stride;
    *ns = est > (double)HM_L1_SHARD_TILES * HM_T1 ? HM_L1_SHARDS : 1;
    const double e = est / *ns;
    /* + HM_L1_ZERO_SAMPLES strides per digit: a digit with few or no samples
     * may still hold that many strides of points (P(0 samples | 24) = 4e-11);
     * the region's unused tail is never read */
    return (uint32_t)fmin(1.0e9, e + e / 16 + 8.0 * sqrt(e * (double)stride) +
                                     (double)HM_L1_ZERO_SAMPLES * (double)stride / *ns + 2.0 * HM_T1);
}

__global__ __launch_bounds__(1024) void k_l1_sizes(const uint32_t* __restrict__ hist, int F,
                                                   const uint32_t* __restrict__ hot_n, uint64_t stride,
                                                   uint32_t* __restrict__ rcap, uint32_t* __restrict__ rbase,
                                                   uint8_t* __restrict__ smask, unsigned long long* total)
{
    __shared__ unsigned long long wsum[1024 / 64];
    static_assert(HM_MAX_HOT <= 1024 && HM_MAX_F1 <= 1024, "one digit of each kind per thread");
    const int t = threadIdx.x;
    const int lane = t & 63, w = t >> 6;
    const uint32_t H = hot_n ? min(*hot_n, (uint32_t)HM_MAX_HOT) : 0u;
    unsigned long long base = 0;
    for (int kind = 0; kind < 2; kind++) {
        const int d = kind ? HM_MAX_F1 + t : t;
        const bool live = kind ? (uint32_t)t < H : t < F;
        uint32_t c = 0;
        int ns = 1;
        if (live) {
            c = hm_l1_cap(hist[d], stride, &ns);
            smask[d] = (uint8_t)(ns - 1);
        }
        const unsigned long long mine = live ? (unsigned long long)c * (unsigned long long)ns : 0ull;
        unsigned long long incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        __syncthreads();
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        unsigned long long before = 0, all = 0;
        for (int i = 0; i < 1024 / 64; i++) {
            before += i < w ? wsum[i] : 0ull;
            all += wsum[i];
        }
        unsigned long long pos = base + before + incl - mine;
        if (live)
            for (int sh = 0; sh < HM_L1_SHARDS; sh++) {
                const uint32_t cs = sh < ns ? c : 0u;
                rcap[hm_l1i(d, sh)] = cs;
                rbase[hm_l1i(d, sh)] = (uint32_t)pos;   /* total < 2^32: the host's bound */
                pos += cs;
            }
        base += all;
    }
    if (t == 0 && total) *total = base;
}

void hm_launch_l1_sizes(hipStream_t s, const uint32_t* hist, int F, const uint32_t* hot_n, uint64_t stride,
                        uint32_t* rcap, uint32_t* rbase, uint8_t* smask, unsigned long long* total)
{
    hipLaunchKernelGGL(k_l1_sizes, dim3(1), dim3(1024), 0, s, hist, F, hot_n, stride, rcap, rbase, smask, total);
}

void hm_launch_sample_digits(hipStream_t s, const HmPart1Args& a, uint64_t stride_pts, uint32_t* hist,
                             uint32_t* hot_counts)
{
    const uint64_t m = ((uint64_t)a.n + stride_pts - 1) / stride_pts;
    uint64_t blocks = (m + 1023) / 1024;
    /* with the hot-tile counts: fewer, fuller blocks (one global atomic per
     * block and tile) */
    const uint64_t cap = hot_counts ? 256 : 2048;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
#define HM_SD(T, H) hipLaunchKernelGGL((k_sample_digits<T, H>), dim3((unsigned)blocks), dim3(256), 0, s, a, stride_pts, \
                                       hist, hot_counts)
    if (a.rows_in) {
        if (hot_counts) HM_SD(true, true);
        else HM_SD(true, false);
    } else {
        if (hot_counts) HM_SD(false, true);
        else HM_SD(false, false);
    }
#undef HM_SD
}

/* Level-1 buckets from the filled regions: one flat run per non-empty digit
 * (its whole region), the bucket list, work-item prefix and, when level 1 is
 * the last level, the merge slots of multi-item buckets.  One block. */
__global__ __launch_bounds__(1024) void k_level1_buckets(HmL1Args a)
{
    __shared__ uint32_t scr[1024 / 64 + 1];
    const int d = threadIdx.x;
    uint32_t f[HM_L1_SHARDS];
    uint32_t nk = 0, nr = 0;
    const int ns = d < a.F ? a.smask[d] + 1 : 0;
#pragma unroll
    for (int sh = 0; sh < HM_L1_SHARDS; sh++) {
        f[sh] = sh < ns ? a.fill[hm_l1i(d, sh)] : 0u;
        nk += f[sh];
        nr += f[sh] != 0;
    }
    /* a digit whose points all went to its hot tiles is still a bucket: the
     * parent of those tiles at level 2 (no keys, no items of its own) */
    const uint32_t ne = nk > 0 || (a.hotparent && d < a.F && a.hotparent[d]);
    const uint32_t nit = nk ? (nk <= a.sparse_max ? 0u : (nk + a.item_keys - 1) / a.item_keys) : 0u;
    uint32_t count, items, runs;
    const uint32_t idx = hm_block_excl_scan<1024>(ne, scr, &count);
    const uint32_t ib = hm_block_excl_scan<1024>(nit, scr, &items);
    const uint32_t r0 = hm_block_excl_scan<1024>(nr, scr, &runs);
    if (a.d2b && d < a.F) a.d2b[d] = ne ? idx : 0xFFFFFFFFu;
    if (ne) {
        /* logical key positions of the bucket: [region base, + nk), its
         * non-empty shards' keys one after the other */
        const uint32_t kb = a.rbase[hm_l1i(d, 0)];
        a.out.nkeys[idx] = nk;
        a.out.nruns[idx] = nr;
        a.out.rbase[idx] = r0;
        a.out.keybase[idx] = kb;
        a.out.item_begin[idx] = ib;
        a.out.digit[idx] = (uint32_t)d;
        const int wd = a.dbits >> 1;
        a.out.coord[idx] = ((uint64_t)(d >> wd) << 32) | (uint64_t)(d & ((1 << wd) - 1));
        uint32_t j = r0, at = kb;
#pragma unroll
        for (int sh = 0; sh < HM_L1_SHARDS; sh++) {
            if (f[sh]) {
                a.runs[j] = make_uint2(a.rbase[hm_l1i(d, sh)], f[sh]);
                a.excl[j] = at;
                at += f[sh];
                j++;
            }
        }
        if (a.slots) {
            int32_t sl = -1;
            if (nit > 1) {
                sl = (int32_t)atomicAdd(a.nslots, 1ull);
                a.slot_bucket[sl] = idx;
            }
            a.slots[idx] = sl;
        }
    }
    if (d == 0) {
        a.out.item_begin[count] = items;
        a.child_begin[0] = 0;
        a.child_begin[1] = count;
        *a.total = ((uint64_t)count << 32) | items;
    }
}

void hm_launch_level1_buckets(hipStream_t s, const HmL1Args& a)
{
    hipLaunchKernelGGL(k_level1_buckets, dim3(1), dim3(1024), 0, s, a);
}

/* Descriptor of work item g (T keys per item): its bucket (binary search over
 * item_begin), its logical positions [a, b) and the runs [r0, r1) that
 * overlap them.  One thread per item; the searches of all items overlap. */
__global__ __launch_bounds__(256) void k_items(HmBuckets B, HmRuns in, uint32_t items, uint32_t T, uint4* desc,
                                               uint32_t* seg)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= items) return;
    const uint32_t bk = hm_upper_bound(B.item_begin, B.count + 1, g) - 1;
    const uint32_t j = g - B.item_begin[bk];
    const uint32_t nitems = B.item_begin[bk + 1] - B.item_begin[bk];
    const uint64_t kb = B.keybase[bk], nk = B.nkeys[bk];
    const uint64_t a = kb + (uint64_t)j * T;
    const uint64_t b = kb + min((uint64_t)(j + 1) * T, nk);
    const uint32_t rb = B.rbase[bk], nr = B.nruns[bk];
    const uint32_t r0 = rb + hm_upper_bound(in.excl + rb, nr, a) - 1;   /* last run starting <= a */
    const uint32_t r1 = rb + hm_lower_bound(in.excl + rb, nr, b);       /* first run starting >= b */
    desc[2 * g] = make_uint4(bk, j, nitems, r0);
    desc[2 * g + 1] = make_uint4(r1, 0u, (uint32_t)a, (uint32_t)b);
    if (seg) {
        /* the item's <= HM_L1_SHARDS runs as (logical start, source index)
         * pairs, unused entries repeating the last run (k_partition_fr) */
        uint4* sg = (uint4*)(seg + 16 * (size_t)g);
        uint32_t v[2 * HM_L1_SHARDS];
        const uint32_t last = r1 > r0 ? r1 - 1 : r0;
#pragma unroll
        for (int q = 0; q < HM_L1_SHARDS; q++) {
            const uint32_t r = min(r0 + q, last);
            v[2 * q] = (uint32_t)in.excl[r];
            v[2 * q + 1] = in.run[r].x;
        }
#pragma unroll
        for (int q = 0; q < HM_L1_SHARDS / 2; q++) sg[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
}

void hm_launch_items(hipStream_t s, const HmBuckets& B, HmRuns in, uint32_t items, uint32_t T, uint4* desc,
                     uint32_t* seg)
{
    if (items) hipLaunchKernelGGL(k_items, dim3((items + 255) / 256), dim3(256), 0, s, B, in, items, T, desc, seg);
}

/* ------------------------------------------------------------------------ */
/* levels >= 2: stream a parent item's runs, counting sort by the next digit */
/* ------------------------------------------------------------------------ */

template <typename OutT>
__global__ __launch_bounds__(HM_PN_THREADS, 8) void k_partition(HmPartNArgs a)
{
    /* streamed keys in staged order, then the digit-sorted output (OutT);
     * words [HM_TN, HM_TN + 64) absorb the writes of idle lanes */
    __shared__ __attribute__((aligned(16))) uint32_t stage[HM_TN + 64];
    __shared__ uint32_t cur[HM_MAX_FN + 64];   /* + 64 dummy words (hm_lds_count) */
    __shared__ uint32_t scr[HM_PN_THREADS / 64 + 1];
    __shared__ unsigned long long scr64[HM_PN_THREADS / 64 + 1];
    __shared__ HmRunLds<512> L;
    HM_STAMP(0);
    const int tid = threadIdx.x;
    const int F = 1 << a.dbits;
    for (int i = tid; i < F; i += HM_PN_THREADS) cur[i] = 0;
    __syncthreads();
    HM_STAMP(1);
    if (hm_block_id() >= a.items) return;
    const HmItem it = hm_item(a.parent, hm_block_id());
    /* parent key: (row << sp) | col, sp = s + w bits each; digit = top w bits
     * of both, rest = low s bits of both.  Streaming re-encodes every key as
     * (digit << 2s) | rest (still <= 32 bits), so the scatter only shifts. */
    const int sw = a.restbits >> 1, ww = a.dbits >> 1, sp = sw + ww;
    const uint32_t restmask = (a.restbits >= 32) ? 0xFFFFFFFFu : ((1u << a.restbits) - 1u);
    struct {
        uint32_t* cur;
        uint32_t dummy;
        uint32_t* stage;
        int s, w, sp;
        __device__ __forceinline__ uint32_t pack(uint32_t k) const
        {
            const uint32_t r = k >> sp, c = k & ((1u << sp) - 1u), m = (1u << s) - 1u;
            const uint32_t d = ((r >> s) << w) | (c >> s);
            return (d << (2 * s)) | ((r & m) << s) | (c & m);
        }
        __device__ __forceinline__ void key(uint32_t k, bool v, uint32_t pos)
        {
            const uint32_t x = pack(k);
            hm_lds_count_m(cur, dummy, hm_cur_slot(x >> (2 * s), w), v);
            stage[v ? pos : HM_TN + hm_lane()] = x;
        }
        __device__ __forceinline__ void vec(const uint4& k, bool v, uint32_t pos)
        {
            const uint4 x = make_uint4(pack(k.x), pack(k.y), pack(k.z), pack(k.w));
            hm_lds_count_m(cur, dummy, hm_cur_slot(x.x >> (2 * s), w), v);
            hm_lds_count_m(cur, dummy, hm_cur_slot(x.y >> (2 * s), w), v);
            hm_lds_count_m(cur, dummy, hm_cur_slot(x.z >> (2 * s), w), v);
            hm_lds_count_m(cur, dummy, hm_cur_slot(x.w >> (2 * s), w), v);
            *(uint4*)&stage[v ? pos : HM_TN] = x;
        }
    } f{cur, HM_MAX_FN, stage, sw, ww, sp};
    HM_STAMP(2);
    hm_stream_runs<uint32_t, HM_PN_THREADS, 512, true>(it, a.keys_in, a.in, L, scr, f);
    HM_STAMP(7);
    const uint32_t total = it.b - it.a;
    constexpr int PER = HM_MAX_FN / HM_PN_THREADS;
    static_assert(HM_TN < (1 << (64 / PER)), "packed digit counts");
    uint32_t cnt[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * HM_PN_THREADS + tid;
        cnt[q] = d < F ? cur[hm_cur_slot(d, ww)] : 0u;
    }
    uint32_t offq[PER];
    hm_digit_offsets<HM_PN_THREADS, PER>(cnt, offq, scr64);
    HM_STAMP(8);
    const uint32_t tile0 = a.parent.item_begin[it.bucket];
    const uint32_t sh = it.j & ((1u << a.shard_bits) - 1u);
    const uint64_t cap = ((uint64_t)it.nitems + (1u << a.shard_bits) - 1) >> a.shard_bits;
    /* run-slot atomics are issued here and their results consumed only after
     * the scatter, so their latency hides behind it */
    uint32_t idx[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * HM_PN_THREADS + tid;
        idx[q] = 0;
        if (d < F && cnt[q])
            idx[q] = atomicAdd(&a.nruns_out[((((uint64_t)it.bucket << a.dbits) + d) << a.shard_bits) + sh], 1u);
    }
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * HM_PN_THREADS + tid;
        if (d < F) cur[hm_cur_slot(d, ww)] = offq[q];
    }
    constexpr int KPT = HM_TN / HM_PN_THREADS;
    uint32_t kv[KPT];
#pragma unroll
    for (int k = 0; k < KPT; k++) {
        const uint32_t i = k * HM_PN_THREADS + tid;
        kv[k] = i < total ? stage[i] : 0u;
    }
    __syncthreads();
    HM_STAMP(9);
    OutT* so = (OutT*)stage;
    /* claim: every slot atomic issued before any result is consumed (the
     * helper's logic of hm_lds_claim, unrolled over the KPT keys) */
    {
        uint32_t old[KPT];
        HmMerge g[KPT];
        bool v[KPT];
#pragma unroll
        for (int k = 0; k < KPT; k++) {
            v[k] = k * HM_PN_THREADS + tid < total;
            g[k] = hm_merge_prep(hm_cur_slot(kv[k] >> a.restbits, ww), v[k], HM_MAX_FN);
            old[k] = atomicAdd(&cur[g[k].idx], g[k].inc);
        }
#pragma unroll
        for (int k = 0; k < KPT; k++)
            so[v[k] ? hm_merge_pos(g[k], old[k]) : HM_TN + tid % 64] = (OutT)(kv[k] & restmask);
    }
    __syncthreads();
    HM_STAMP(10);
    OutT* out = (OutT*)a.keys_out + it.a;
    for (uint32_t i = tid; i < total; i += HM_PN_THREADS) out[i] = so[i];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * HM_PN_THREADS + tid;
        if (d < F && cnt[q]) {
            const uint64_t rb = hm_run_base(tile0, it.nitems, it.bucket, d, a.dbits, a.shard_bits);
            a.runs_out[rb + sh * cap + idx[q]] = make_uint2(it.a + offq[q], cnt[q]);
        }
    }
    HM_STAMP(11);
}

/* Level 2 from the level-1 regions: every parent item spans at most
 * HM_L1_SHARDS contiguous runs, so each thread loads its HM_FR_KPT keys
 * straight into registers (key i of the item at thread i % T) -- no LDS
 * staging of the streamed keys.  One returning LDS atomic per key gives both
 * the digit histogram and the key's rank within its digit; after the scan a
 * key's slot is offset[digit] + rank.  Small blocks (512 threads, ~34 KB of
 * LDS) so that 4 blocks share a CU and one block's loads overlap the others'
 * LDS phases.  Output contract identical to k_partition. */
template <typename OutT>
__global__ __launch_bounds__(HM_FR_THREADS, 8) void k_partition_fr(HmPartNArgs a)
{
    constexpr int T = HM_FR_THREADS;
    constexpr int KPT = HM_TN / T;
    constexpr int PER = HM_MAX_FN / T;
    __shared__ uint32_t cur[HM_MAX_FN + 64];   /* + 64 dummy words */
    constexpr uint32_t V = 16 / sizeof(OutT);   /* keys per 16-B vector */
    /* key e of the item at stage[sh + e], sh = it.a mod V: the copy-out then
     * moves 16-B vectors aligned on both sides */
    __shared__ __attribute__((aligned(16))) OutT stage[HM_TN + 64 + V];
    __shared__ unsigned long long scr[T / 64 + 1];
    const int tid = threadIdx.x;
    const int F = 1 << a.dbits;
    const uint32_t g = hm_block_id();
    if (g >= a.items) return;
    HM_STAMP_M(3, 0);
    const HmItem it = hm_item(a.parent, g);
    /* the item's runs (<= HM_L1_SHARDS, block-uniform): logical start and
     * source index of each, from k_items' per-item table -- one 64-B load
     * next to the descriptor's, not a chain of dependent loads */
    const uint4* sg = (const uint4*)(a.seg + 16 * (size_t)g);
    const uint4 s0 = sg[0], s1 = sg[1], s2 = sg[2], s3 = sg[3];
    const uint32_t rpos[HM_L1_SHARDS] = {s0.x, s0.z, s1.x, s1.z, s2.x, s2.z, s3.x, s3.z};
    const uint32_t rsrc[HM_L1_SHARDS] = {s0.y, s0.w, s1.y, s1.w, s2.y, s2.w, s3.y, s3.w};
    const uint32_t nr = min(it.r1 - it.r0, (uint32_t)HM_L1_SHARDS);
    const uint32_t total = it.b - it.a;
    uint32_t kv[KPT];
#pragma unroll
    for (int k = 0; k < KPT; k++) {
        const uint32_t i = (uint32_t)(k * T + tid);
        const uint32_t p = it.a + i;
        uint32_t src = rsrc[0] + (p - rpos[0]);
#pragma unroll
        for (int j = 1; j < HM_L1_SHARDS; j++)
            src = ((uint32_t)j < nr && rpos[j] <= p) ? rsrc[j] + (p - rpos[j]) : src;
        kv[k] = i < total ? a.keys_in[src] : 0u;
    }
    for (int i = tid; i < F; i += T) cur[i] = 0;
    __syncthreads();
    HM_STAMP_M(3, 1);
    const int sw = a.restbits >> 1, ww = a.dbits >> 1, sp = sw + ww;
    const uint32_t m = (1u << sw) - 1u;
    /* re-encode each key as (digit slot << 2s) | rest (the slot: the digit's
     * hm_cur_slot, a bijection), then count and rank */
    uint32_t rank[KPT];
    const uint32_t dummy = HM_MAX_FN + (uint32_t)hm_lane();
    /* HM_FR_GROUP atomics in flight per thread (more costs registers) */
#pragma unroll
    for (int k0 = 0; k0 < KPT; k0 += HM_FR_GROUP) {
        HmClaim gm[HM_FR_GROUP];
        uint32_t old[HM_FR_GROUP];
#pragma unroll
        for (int u = 0; u < HM_FR_GROUP; u++) {
            const int k = k0 + u;
            const uint32_t r = kv[k] >> sp, c = kv[k] & ((1u << sp) - 1u);
            const uint32_t ds = hm_cur_slot(((r >> sw) << ww) | (c >> sw), ww);
            kv[k] = (ds << (2 * sw)) | ((r & m) << sw) | (c & m);
            const bool v = (uint32_t)(k * T + tid) < total;
            gm[u] = hm_claim_prep(ds, v, dummy);
            old[u] = atomicAdd(&cur[gm[u].idx], gm[u].inc);
        }
#pragma unroll
        for (int u = 0; u < HM_FR_GROUP; u++) rank[k0 + u] = hm_claim_pos(gm[u], old[u]);
    }
    HM_STAMP_M(3, 2);
    __syncthreads();
    HM_STAMP_M(3, 3);
    static_assert(HM_TN < (1 << (64 / PER)), "packed digit counts");
    uint32_t cnt[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * T + tid;
        cnt[q] = d < F ? cur[hm_cur_slot(d, ww)] : 0u;
    }
    if (a.mode == HM_PN_HIST) {
        /* the bucket's child totals (a pass before the partition proper) */
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int d = q * T + tid;
            if (d < F && cnt[q])
                atomicAdd(&a.ctot[((uint64_t)it.bucket << a.dbits) + d], (unsigned long long)cnt[q]);
        }
        return;
    }
    const bool contig = a.mode == HM_PN_CONTIG;
    uint32_t offq[PER];
    hm_digit_offsets<T, PER>(cnt, offq, scr);
    const uint32_t tile0 = a.parent.item_begin[it.bucket];
    const uint32_t sh = it.j & ((1u << a.shard_bits) - 1u);
    const uint64_t cap = ((uint64_t)it.nitems + (1u << a.shard_bits) - 1) >> a.shard_bits;
    /* lanes own consecutive digits: with one run counter per child
     * (shard_bits 0) a wave's run-slot atomics coalesce */
    uint32_t idx[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * T + tid;
        idx[q] = 0;
        if (d < F && cnt[q]) {
            const uint64_t child = ((uint64_t)it.bucket << a.dbits) + d;
            if (contig) {
                /* idx: the key position of this item's range of the child */
                idx[q] = a.cbase_off + (uint32_t)a.cbase[child] + atomicAdd(&a.ccur[child], cnt[q]);
                if (atomicCAS(&a.nruns_out[child], 0u, 1u) == 0u) {
                    const uint64_t rb = hm_run_base(tile0, it.nitems, it.bucket, d, a.dbits, 0);
                    a.runs_out[rb] = make_uint2(a.cbase_off + (uint32_t)a.cbase[child], (uint32_t)a.ctot[child]);
                }
            } else {
                idx[q] = atomicAdd(&a.nruns_out[(child << a.shard_bits) + sh], 1u);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * T + tid;
        if (d < F) cur[hm_cur_slot(d, ww)] = offq[q];
    }
    __syncthreads();
    HM_STAMP_M(3, 4);
    const uint32_t restmask = (a.restbits >= 32) ? 0xFFFFFFFFu : ((1u << a.restbits) - 1u);
    const uint32_t sh0 = contig ? 0u : it.a & (V - 1);
#pragma unroll
    for (int k = 0; k < KPT; k++) {
        const bool v = (uint32_t)(k * T + tid) < total;
        const uint32_t ds = kv[k] >> a.restbits;   /* digit slot */
        const uint32_t pos = v ? sh0 + cur[v ? ds : 0u] + rank[k] : (uint32_t)HM_TN + V + (uint32_t)(tid & 63);
        /* (a child-contiguous level stages the digit slot with the key: the
         * copy-out finds each key's destination from it) */
        stage[pos] = (OutT)(contig ? kv[k] : kv[k] & restmask);
    }
    __syncthreads();
    HM_STAMP_M(3, 5);
    if (contig) {
        /* a digit's keys [offq, offq + cnt) of the stage go to idx.. */
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int d = q * T + tid;
            if (d < F) cur[hm_cur_slot(d, ww)] = idx[q] - offq[q];
        }
        __syncthreads();
        OutT* out = (OutT*)a.keys_out;
        for (uint32_t e = tid; e < total; e += T) {
            const uint32_t x = (uint32_t)stage[e];
            out[cur[x >> a.restbits] + e] = (OutT)(x & restmask);
        }
        return;
    }
    {
        /* 16-B vectors [V t, V t + V) of stage map to out[it.a - sh0 + V t ..) */
        OutT* out = (OutT*)a.keys_out + (it.a - sh0);
        const uint32_t end = sh0 + total, nv = (end + V - 1) / V;
        for (uint32_t t = tid; t < nv; t += T) {
            const uint32_t e0 = t * V;
            if (e0 >= sh0 && e0 + V <= end) {
                *(uint4*)(out + e0) = *(const uint4*)(stage + e0);
            } else {
                for (uint32_t e = max(e0, sh0); e < min(e0 + V, end); e++) out[e] = stage[e];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int d = q * T + tid;
        if (d < F && cnt[q]) {
            const uint64_t rb = hm_run_base(tile0, it.nitems, it.bucket, d, a.dbits, a.shard_bits);
            a.runs_out[rb + sh * cap + idx[q]] = make_uint2(it.a + offq[q], cnt[q]);
        }
    }
    HM_STAMP_M(3, 6);
}

/* Child totals of a child-contiguous level (HM_PN_HIST): a block takes
 * HM_HIST_G consecutive items (items are in bucket order, so they mostly
 * share a bucket), counts their keys' children in LDS and adds each bucket's
 * non-zero counts once per block -- HM_HIST_G times fewer global atomics than
 * one flush per item. */
#define HM_HIST_G 8
__global__ __launch_bounds__(HM_FR_THREADS) void k_partition_hist(HmPartNArgs a)
{
    constexpr int T = HM_FR_THREADS;
    constexpr int KPT = HM_TN / T;
    __shared__ uint32_t cur[HM_MAX_FN];
    const int tid = threadIdx.x;
    const int F = 1 << a.dbits;
    const uint32_t g0 = hm_block_id() * HM_HIST_G;
    if (g0 >= a.items) return;
    const uint32_t g1 = min(g0 + HM_HIST_G, a.items);
    const int sw = a.restbits >> 1, ww = a.dbits >> 1, sp = sw + ww;
    for (int i = tid; i < F; i += T) cur[i] = 0;
    __syncthreads();
    uint32_t bucket = hm_item(a.parent, g0).bucket;
    for (uint32_t g = g0; g < g1; g++) {
        const HmItem it = hm_item(a.parent, g);   /* block-uniform */
        if (it.bucket != bucket) {
            /* flush the previous bucket's counts */
            __syncthreads();
            for (int d = tid; d < F; d += T) {
                const uint32_t c = cur[hm_cur_slot(d, ww)];
                if (c) atomicAdd(&a.ctot[((uint64_t)bucket << a.dbits) + d], (unsigned long long)c);
            }
            __syncthreads();
            for (int i = tid; i < F; i += T) cur[i] = 0;
            __syncthreads();
            bucket = it.bucket;
        }
        const uint4* sg = (const uint4*)(a.seg + 16 * (size_t)g);
        const uint4 s0 = sg[0], s1 = sg[1], s2 = sg[2], s3 = sg[3];
        const uint32_t rpos[HM_L1_SHARDS] = {s0.x, s0.z, s1.x, s1.z, s2.x, s2.z, s3.x, s3.z};
        const uint32_t rsrc[HM_L1_SHARDS] = {s0.y, s0.w, s1.y, s1.w, s2.y, s2.w, s3.y, s3.w};
        const uint32_t nr = min(it.r1 - it.r0, (uint32_t)HM_L1_SHARDS);
        const uint32_t total = it.b - it.a;
        uint32_t kv[KPT];
#pragma unroll
        for (int k = 0; k < KPT; k++) {
            const uint32_t i = (uint32_t)(k * T + tid);
            const uint32_t p = it.a + i;
            uint32_t src = rsrc[0] + (p - rpos[0]);
#pragma unroll
            for (int j = 1; j < HM_L1_SHARDS; j++)
                src = ((uint32_t)j < nr && rpos[j] <= p) ? rsrc[j] + (p - rpos[j]) : src;
            kv[k] = i < total ? a.keys_in[src] : 0u;
        }
#pragma unroll
        for (int k = 0; k < KPT; k++) {
            if ((uint32_t)(k * T + tid) < total) {
                const uint32_t r = kv[k] >> sp, c = kv[k] & ((1u << sp) - 1u);
                atomicAdd(&cur[hm_cur_slot(((r >> sw) << ww) | (c >> sw), ww)], 1u);
            }
        }
    }
    __syncthreads();
    for (int d = tid; d < F; d += T) {
        const uint32_t c = cur[hm_cur_slot(d, ww)];
        if (c) atomicAdd(&a.ctot[((uint64_t)bucket << a.dbits) + d], (unsigned long long)c);
    }
}

void hm_launch_partition_hist(hipStream_t s, const HmPartNArgs& a)
{
    const uint32_t blocks = (a.items + HM_HIST_G - 1) / HM_HIST_G;
    if (blocks) hipLaunchKernelGGL(k_partition_hist, hm_grid2(blocks), dim3(HM_FR_THREADS), 0, s, a);
}

/* ------------------------------------------------------------------------ */
/* run scan: sharded run counters -> one flat, child-ordered run list        */
/* ------------------------------------------------------------------------ */

/* per (child, shard) counter: exclusive offset within the child, and per
 * child its run total.  Lanes read consecutive counters (coalesced); a
 * child's S = 2^shard_bits shards are S consecutive lanes, scanned with
 * shuffles.  Every lane of a wave runs every step. */
__global__ __launch_bounds__(256) void k_rs_count(HmRsArgs a)
{
    const uint32_t S = 1u << a.shard_bits;
    const uint64_t npairs = a.nchildren << a.shard_bits;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint32_t sl = (uint32_t)hm_lane() & (S - 1);
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k - (uint64_t)hm_lane() < npairs; k += stride) {
        const bool in = k < npairs;
        const uint32_t n = in ? a.nruns[k] : 0u;
        uint32_t v = n;
        for (uint32_t o = 1; o < S; o <<= 1) {
            const uint32_t t = __shfl_up(v, o, 64);
            if (sl >= o) v += t;
        }
        if (in) {
            a.shoff[k] = v - n;
            if (sl == S - 1) a.nr[k >> a.shard_bits] = v;
        }
    }
}

/* sharded run list of child c -> flat[runbase[c] .. + nr[c]), one wave per
 * child: lanes 0..S-1 hold the child's shards (count, flat offset, source),
 * and the wave copies the child's runs HM_RS_SLICE at a time, 8 loads per lane
 * in flight, each run's shard found by a shuffle search over the S lanes.
 * A child of more than a.big_min runs (HM_RS_BIG by default; one run per
 * parent work item: the hot tile of a skewed cloud has 10^5) is listed instead, and k_rs_copy_big
 * spreads its slices over every wave of the grid. */
#define HM_RS_SLICE 512
#ifndef HM_RS_LANE_MAX
#define HM_RS_LANE_MAX 256  /* children of at most this many runs: copied 64 / S at a time */
#endif

struct HmRsChild {
    uint32_t n, incl;
    uint64_t src;
};

/* lanes 0..S-1: shard counts and sources of child c (loads only) */
__device__ __forceinline__ HmRsChild hm_rs_child_load(const HmRsArgs& a, uint64_t c)
{
    const uint32_t S = 1u << a.shard_bits;
    const uint32_t lane = (uint32_t)hm_lane();
    const uint64_t k = (c << a.shard_bits) + lane;
    HmRsChild h;
    h.n = 0;
    h.src = 0;
    h.incl = 0;
    if (lane < S) {
        h.n = a.nruns[k];
        const uint64_t p = c >> a.dbits;
        const uint64_t d = c & ((1ull << a.dbits) - 1);
        const uint32_t t0 = a.parent_item_begin[p];
        const uint32_t tp = a.parent_item_begin[p + 1] - t0;
        const uint32_t cap = (tp + S - 1) >> a.shard_bits;
        h.src = hm_run_base(t0, tp, p, d, a.dbits, a.shard_bits) + (uint64_t)lane * cap;
    }
    return h;
}

__device__ __forceinline__ HmRsChild hm_rs_child(const HmRsArgs& a, uint64_t c)
{
    HmRsChild h = hm_rs_child_load(a, c);
    h.incl = hm_wave_incl_scan(h.n);   /* shard offsets within the child */
    return h;
}

/* runs j0 .. j0 + 64 U of the child (each lane's shard: a shuffle search) */
template <int U = HM_RS_SLICE / 64>
__device__ __forceinline__ void hm_rs_slice(const HmRsArgs& a, const HmRsChild& h, uint64_t nr, uint64_t rb,
                                            uint64_t j0)
{
    const uint32_t lane = (uint32_t)hm_lane();
    uint2 r[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t x = j0 + (uint64_t)u * 64 + lane;
        const uint32_t xc = (uint32_t)min(x, nr - 1);
        uint32_t l = 0;
#pragma unroll
        for (int st = 32; st > 0; st >>= 1)
            if (__shfl(h.incl, l + st - 1, 64) <= xc) l += st;
        l = min(l, 63u);
        const uint32_t off = xc - (__shfl(h.incl, l, 64) - __shfl(h.n, l, 64));
        const uint64_t sj = __shfl(h.src, l, 64) + off;
        r[u] = x < nr ? a.runs[sj] : make_uint2(0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint64_t x = j0 + (uint64_t)u * 64 + lane;
        if (x < nr) {
            a.flat[rb + x] = r[u];
            a.cnt[rb + x] = r[u].y;
        }
    }
}

/* a wave takes 64 consecutive children at a time: their run counts and
 * bases in one lane-per-child load, then the non-empty ones in turn (most
 * children of a sparse level are empty or hold a few runs: the per-child
 * chain of dependent loads is what this kernel waits on) */
__global__ __launch_bounds__(256) void k_rs_copy(HmRsArgs a)
{
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    const uint32_t lane = (uint32_t)hm_lane();
    for (uint64_t c0 = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; c0 < a.nchildren; c0 += nw * 64) {
        const uint64_t cl = c0 + lane;
        const uint64_t nrl = cl < a.nchildren ? a.nr[cl] : 0ull;
        const uint64_t rbl = nrl ? a.runbase[cl] : 0ull;
        /* the copied children in order; the next one's shard table loads
         * are issued before the current one's run copy */
        uint64_t m = __ballot((nrl != 0) & (nrl <= a.big_min));
        uint64_t mb = __ballot(nrl > a.big_min);
        while (mb) {
            const int i = __builtin_ctzll(mb);
            mb &= mb - 1;
            uint32_t slot = 0;
            if (lane == 0) slot = atomicAdd(a.nbig, 1u);
            slot = __shfl(slot, 0, 64);
            if (slot < HM_RS_BIG_MAX) {
                if (lane == 0) a.big[slot] = (uint32_t)(c0 + (uint64_t)i);
            } else {
                m |= 1ull << i;   /* list full: copied here */
            }
        }
        {
            /* children of <= HM_RS_LANE_MAX runs (not big, not hot) are copied
             * 64 / S at a time, one (child, shard) per lane: a shard's runs
             * are one contiguous source range, a child's one contiguous flat
             * range, so element x of the group's concatenation finds its
             * (child, shard) by a search over the lanes' inclusive run counts;
             * consecutive children have adjacent flat ranges, so the stores
             * coalesce (one child at a time left the wave waiting on each
             * child's chain of dependent loads) */
            const uint32_t S = 1u << a.shard_bits, G = 64u / S;   /* (shard_bits <= 6, as below) */
            const bool mine_l = ((m >> lane) & 1ull) && nrl <= HM_RS_LANE_MAX && G > 0;
            const uint64_t mineb = __ballot(mine_l);
            m &= ~mineb;
            const uint64_t gmask = G >= 64 ? ~0ull : ((1ull << G) - 1ull);
            for (uint32_t g0 = 0; mineb && g0 < 64; g0 += G) {
                if (!((mineb >> g0) & gmask)) continue;   /* wave-uniform */
                const uint32_t ci = g0 + lane / S, sh = lane & (S - 1u);
                const bool cm = (mineb >> ci) & 1ull;
                const uint64_t rbc = __shfl(rbl, (int)ci, 64);
                uint32_t n = 0;
                uint64_t src = 0;
                if (cm) {
                    const uint64_t c = c0 + ci;
                    n = a.nruns[(c << a.shard_bits) + sh];   /* 0 for a hot tile (k_hot_runs lists its runs) */
                    const uint64_t p = c >> a.dbits, d = c & ((1ull << a.dbits) - 1);
                    const uint32_t t0 = a.parent_item_begin[p];
                    const uint32_t tp = a.parent_item_begin[p + 1] - t0;
                    const uint64_t cap = ((uint64_t)tp + S - 1) >> a.shard_bits;
                    src = hm_run_base(t0, tp, p, d, a.dbits, a.shard_bits) + (uint64_t)sh * cap;
                }
                const uint32_t incl = hm_wave_incl_scan(n);
                const int fl = (int)(lane & ~(S - 1u));   /* the child's first lane */
                const uint32_t cfirst = __shfl(incl, fl, 64) - __shfl(n, fl, 64);
                const uint64_t dst = rbc + (incl - n - cfirst);
                const uint32_t tot = __shfl(incl, 63, 64);
                for (uint32_t x0 = 0; x0 < tot; x0 += 64) {
                    const uint32_t x = x0 + lane;
                    const uint32_t xc = min(x, tot - 1u);
                    uint32_t l = 0;
#pragma unroll
                    for (int st = 32; st > 0; st >>= 1)
                        if (__shfl(incl, (int)(l + st - 1), 64) <= xc) l += st;
                    l = min(l, 63u);
                    const uint32_t j = xc - (__shfl(incl, (int)l, 64) - __shfl(n, (int)l, 64));
                    const uint64_t sj = __shfl(src, (int)l, 64) + j, dj = __shfl(dst, (int)l, 64) + j;
                    if (x < tot) {
                        const uint2 r = a.runs[sj];
                        a.flat[dj] = r;
                        a.cnt[dj] = r.y;
                    }
                }
            }
        }
        if (!m) continue;
        int i = __builtin_ctzll(m);
        m &= m - 1;
        HmRsChild h = hm_rs_child_load(a, c0 + (uint64_t)i);
        for (;;) {
            const int inext = m ? __builtin_ctzll(m) : -1;
            HmRsChild hn;
            if (inext >= 0) {
                m &= m - 1;
                hn = hm_rs_child_load(a, c0 + (uint64_t)inext);
            }
            h.incl = hm_wave_incl_scan(h.n);
            const uint64_t nr = __shfl(nrl, i, 64);
            const uint64_t rb = __shfl(rbl, i, 64);
            /* a sparse level's children hold a few runs: one 64-run step;
             * a hot tile has runs but no sharded ones (k_hot_runs lists them) */
            if (__shfl(h.incl, 63, 64) == 0)
                ;
            else if (nr <= 64)
                hm_rs_slice<1>(a, h, nr, rb, 0);
            else if (nr <= 256)
                hm_rs_slice<4>(a, h, nr, rb, 0);
            else
                for (uint64_t j0 = 0; j0 < nr; j0 += HM_RS_SLICE) hm_rs_slice(a, h, nr, rb, j0);
            if (inext < 0) break;
            i = inext;
            h = hn;
        }
    }
}

/* the listed children: wave w copies slices w, w + waves, ... of each */
__global__ __launch_bounds__(256) void k_rs_copy_big(HmRsArgs a)
{
    const uint32_t nb = min(*a.nbig, (uint32_t)HM_RS_BIG_MAX);
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = (uint32_t)hm_lane();
    for (uint32_t e0 = 0; e0 < nb; e0 += 64) {
        /* 64 listed children per lane-parallel load */
        const bool in = e0 + lane < nb;
        const uint32_t cl = in ? a.big[e0 + lane] : 0u;
        const uint64_t nrl = in ? a.nr[cl] : 0ull;
        const uint64_t rbl = in ? a.runbase[cl] : 0ull;
        const uint32_t ne = min(64u, nb - e0);
        for (uint32_t j = 0; j < ne; j++) {
            const uint64_t nr = __shfl(nrl, (int)j, 64);
            /* rotate the starting wave per child so short tails spread out */
            const uint64_t w0 = (w + (uint64_t)(e0 + j) * 97) % nw;
            if (w0 * HM_RS_SLICE >= nr) continue;
            const uint64_t c = __shfl(cl, (int)j, 64);
            const uint64_t rb = __shfl(rbl, (int)j, 64);
            const HmRsChild h = hm_rs_child(a, c);
            for (uint64_t j0 = w0 * HM_RS_SLICE; j0 < nr; j0 += nw * HM_RS_SLICE) hm_rs_slice(a, h, nr, rb, j0);
        }
    }
}

/* per child: global key range of its runs and work items of the next stage */
__global__ __launch_bounds__(256) void k_rs_keys(HmRsArgs a)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < a.nchildren; c += stride) {
        const uint64_t nr = a.nr[c];
        if (nr == 0) {
            a.nkeys[c] = 0;
            a.keybase[c] = 0;
            /* a forced child is a bucket without keys or items (a hot tile's
             * ancestor: the tile joins it as a child one level down) */
            a.vals[c] = (a.force && a.force[c]) ? (1ull << 32) : 0ull;
            continue;
        }
        const uint64_t rb = a.runbase[c];
        const uint64_t kb = a.excl[rb];
        const uint64_t nflat = a.nflat_dev ? *a.nflat_dev : a.nflat;
        const uint64_t ke = (rb + nr < nflat) ? a.excl[rb + nr] : *a.total_keys;
        const uint32_t nk = (uint32_t)(ke - kb);
        a.nkeys[c] = nk;
        a.keybase[c] = (uint32_t)kb;
        /* last level: buckets of <= HM_SP_MAX keys get no dense work items
         * (one wavefront each: k_small_sort / k_small_emit) */
        const uint32_t nit = nk <= a.sparse_max ? 0u : (nk + a.item_keys - 1) / a.item_keys;
        a.vals[c] = (1ull << 32) | (uint64_t)nit;
    }
}

/* Hot tiles as level-2 children: child (bucket of its z1 digit, its digit
 * below it); its runs are its non-empty level-1 region shards, whose keys K1
 * wrote in the final (u16) form into the level-2 key array.  k_hot_nr sets
 * the children's run counts before the run scan, k_hot_runs lists the runs at
 * their flat positions after it (k_rs_copy skips the children). */
__device__ __forceinline__ uint64_t hm_hot_parent(const HmHotRunArgs& a, uint32_t tr, uint32_t tc, int* s)
{
    const int s1 = a.zb - a.z1;
    uint64_t p = a.d2b[((tr >> s1) << a.z1) | (tc >> s1)];   /* the z1 bucket */
    *s = s1;
    if (a.c2b) {
        /* level 3: the zoom-zp ancestor's bucket among the z1 bucket's children */
        const int sp = a.zb - a.zp, w = a.zp - a.z1;
        const uint32_t m = (1u << w) - 1u;
        p = a.c2b[(p << (2 * w)) | (((tr >> sp) & m) << w) | ((tc >> sp) & m)];
        *s = sp;
    }
    return p;
}

/* the last-level child index of hot tile t */
__device__ __forceinline__ uint64_t hm_hot_child(const HmHotRunArgs& a, uint32_t t)
{
    const uint32_t tr = t >> a.zb, tc = t & ((1u << a.zb) - 1u);
    int s;
    const uint64_t p = hm_hot_parent(a, tr, tc, &s);
    const uint32_t m = (1u << s) - 1u;
    return (p << a.dbits) | (((tr & m) << s) | (tc & m));
}

/* 3-level plan: flag each hot tile's zoom-zp ancestor among the level-2
 * children (child = z1 bucket << dbits | ancestor digit), so it stays a bucket */
__global__ __launch_bounds__(256) void k_hot_force(HmHotRunArgs a, uint8_t* force)
{
    const uint32_t H = *a.n;
    for (uint32_t h = blockIdx.x * 256 + threadIdx.x; h < H; h += gridDim.x * 256) {
        const uint32_t t = a.tiles[h];
        const uint32_t tr = t >> a.zb, tc = t & ((1u << a.zb) - 1u);
        const int s1 = a.zb - a.z1, sp = a.zb - a.zp, w = a.zp - a.z1;
        const uint64_t p = a.d2b[((tr >> s1) << a.z1) | (tc >> s1)];
        const uint32_t m = (1u << w) - 1u;
        force[(p << a.dbits) | (((tr >> sp) & m) << w) | ((tc >> sp) & m)] = 1;
    }
}

__global__ __launch_bounds__(256) void k_hot_nr(HmHotRunArgs a)
{
    const uint32_t H = *a.n;
    for (uint32_t h = blockIdx.x * 256 + threadIdx.x; h < H; h += gridDim.x * 256) {
        uint32_t nr = 0;
#pragma unroll
        for (int sh = 0; sh < HM_L1_SHARDS; sh++) nr += a.fill[hm_l1i(HM_MAX_F1 + h, sh)] != 0;
        if (nr) a.nr[hm_hot_child(a, a.tiles[h])] = nr;
    }
}

__global__ __launch_bounds__(256) void k_hot_runs(HmHotRunArgs a)
{
    const uint32_t H = *a.n;
    for (uint32_t h = blockIdx.x * 256 + threadIdx.x; h < H; h += gridDim.x * 256) {
        uint64_t j = 0;
        bool any = false;
#pragma unroll
        for (int sh = 0; sh < HM_L1_SHARDS; sh++) any |= a.fill[hm_l1i(HM_MAX_F1 + h, sh)] != 0;
        if (!any) continue;
        const uint64_t rb = a.runbase[hm_hot_child(a, a.tiles[h])];
#pragma unroll
        for (int sh = 0; sh < HM_L1_SHARDS; sh++) {
            const uint32_t k = hm_l1i(HM_MAX_F1 + h, sh);
            const uint32_t f = a.fill[k];
            if (f) {
                a.flat[rb + j] = make_uint2(a.rbase[k], f);
                a.cnt[rb + j] = f;
                j++;
            }
        }
    }
}

void hm_launch_hot_force(hipStream_t s, const HmHotRunArgs& a, uint8_t* force)
{
    hipLaunchKernelGGL(k_hot_force, dim3(HM_MAX_HOT / 256), dim3(256), 0, s, a, force);
}

void hm_launch_hot_nr(hipStream_t s, const HmHotRunArgs& a)
{
    hipLaunchKernelGGL(k_hot_nr, dim3(HM_MAX_HOT / 256), dim3(256), 0, s, a);
}

void hm_launch_hot_runs(hipStream_t s, const HmHotRunArgs& a)
{
    hipLaunchKernelGGL(k_hot_runs, dim3(HM_MAX_HOT / 256), dim3(256), 0, s, a);
}

/* ------------------------------------------------------------------------ */
/* device-wide exclusive scan of u64 (any length)                            */
/* ------------------------------------------------------------------------ */

#define HM_SCAN_ITEMS 4096
#define HM_SCAN_THREADS 256
#define HM_SCAN_MAXB 4096

__global__ __launch_bounds__(HM_SCAN_THREADS) void k_scan_reduce(const uint64_t* v, uint64_t n, uint64_t chunk,
                                                                 uint64_t* partial, const uint64_t* ndev)
{
    __shared__ uint64_t red[HM_SCAN_THREADS / 64];
    if (ndev) n = min(n, *ndev);   /* the live length, read on the device */
    const uint64_t b0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t b1 = min(b0 + chunk, n);
    uint64_t s = 0;
    for (uint64_t i = b0 + threadIdx.x; i < b1; i += HM_SCAN_THREADS) s += v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (hm_lane() == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (int w = 0; w < HM_SCAN_THREADS / 64; w++) t += red[w];
        partial[blockIdx.x] = t;
    }
}

/* single block: exclusive scan of up to 1024 * PER values v -> out (may be
 * v itself: a thread reads its PER values before writing them); total ->
 * *total.  PER = 4: the partials of a multi-block scan; PER = 16: a whole
 * scan of <= 16384 values in one dispatch (small calls are dispatch-bound). */
template <int PER>
__global__ __launch_bounds__(1024) void k_scan_one(const uint64_t* v, uint32_t n, uint64_t* out, uint64_t* total,
                                                   const uint64_t* ndev)
{
    __shared__ uint64_t ws[17];
    if (ndev) n = (uint32_t)min((uint64_t)n, *ndev);
    const int tid = threadIdx.x;
    uint64_t x[PER];
    uint64_t s = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const uint32_t i = tid * PER + q;
        x[q] = i < n ? v[i] : 0;
        s += x[q];
    }
    const uint64_t inc = hm_wave_incl_scan64(s);
    const int w = tid >> 6;
    if (hm_lane() == 63) ws[w] = inc;
    __syncthreads();
    if (tid == 0) {
        uint64_t acc = 0;
        for (int k = 0; k < 16; k++) {
            const uint64_t t = ws[k];
            ws[k] = acc;
            acc += t;
        }
        ws[16] = acc;
    }
    __syncthreads();
    uint64_t off = ws[w] + inc - s;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const uint32_t i = tid * PER + q;
        if (i < n) out[i] = off;
        off += x[q];
    }
    if (tid == 0) *total = ws[16];
}

/* block b: its chunk in sub-chunks of HM_SCAN_ITEMS, carrying the prefix.
 * The sub-chunk passes through LDS both ways (padded one word per 16), so
 * global loads and stores are lane-consecutive while each thread scans 16
 * consecutive values.  SUM (grids of <= HM_SCAN_THREADS blocks): the block
 * sums the partials before it itself, and the last block writes the total --
 * no k_scan_one dispatch between the two passes */
#define HM_SCAN_PAD(i) ((i) + ((i) >> 4))
template <bool SUM>
__global__ __launch_bounds__(HM_SCAN_THREADS) void k_scan_down(const uint64_t* v, uint64_t n, uint64_t chunk,
                                                               const uint64_t* partial, uint64_t* out,
                                                               const uint64_t* ndev, uint64_t* total)
{
    __shared__ uint64_t ws[HM_SCAN_THREADS / 64 + 1];
    __shared__ uint64_t buf[HM_SCAN_PAD(HM_SCAN_ITEMS)];
    if (ndev) n = min(n, *ndev);
    constexpr int PER = HM_SCAN_ITEMS / HM_SCAN_THREADS;
    const uint32_t tid = threadIdx.x;
    const uint64_t c0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t c1 = min(c0 + chunk, n);
    uint64_t carry;
    if (SUM) {
        uint64_t p = tid < blockIdx.x ? partial[tid] : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
        if (hm_lane() == 0) ws[tid >> 6] = p;
        __syncthreads();
        carry = 0;
#pragma unroll
        for (int k = 0; k < HM_SCAN_THREADS / 64; k++) carry += ws[k];
        __syncthreads();
    } else {
        carry = partial[blockIdx.x];
    }
    for (uint64_t s0 = c0; s0 < c1; s0 += HM_SCAN_ITEMS) {
        const uint64_t m = min<uint64_t>(c1 - s0, HM_SCAN_ITEMS);
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const uint32_t i = (uint32_t)q * HM_SCAN_THREADS + tid;
            buf[HM_SCAN_PAD(i)] = i < m ? v[s0 + i] : 0ull;
        }
        __syncthreads();
        uint64_t x[PER];
        uint64_t s = 0;
#pragma unroll
        for (int q = 0; q < PER; q++) {
            x[q] = buf[HM_SCAN_PAD(tid * PER + q)];
            s += x[q];
        }
        const uint64_t inc = hm_wave_incl_scan64(s);
        const int w = tid >> 6;
        if (hm_lane() == 63) ws[w] = inc;
        __syncthreads();
        if (tid == 0) {
            uint64_t acc = 0;
            for (int k = 0; k < HM_SCAN_THREADS / 64; k++) {
                const uint64_t t = ws[k];
                ws[k] = acc;
                acc += t;
            }
            ws[HM_SCAN_THREADS / 64] = acc;
        }
        __syncthreads();
        uint64_t off = carry + ws[w] + inc - s;
#pragma unroll
        for (int q = 0; q < PER; q++) {
            buf[HM_SCAN_PAD(tid * PER + q)] = off;
            off += x[q];
        }
        carry += ws[HM_SCAN_THREADS / 64];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const uint32_t i = (uint32_t)q * HM_SCAN_THREADS + tid;
            if (i < m) out[s0 + i] = buf[HM_SCAN_PAD(i)];
        }
        __syncthreads();
    }
    if (SUM && blockIdx.x == gridDim.x - 1 && tid == 0) *total = carry;
}

/* compaction of non-empty children into the bucket list B_l (parent-major) */
__global__ __launch_bounds__(256) void k_compact(HmCompactArgs a)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t F = 1ull << a.dbits;
    const uint32_t count = (uint32_t)(*a.total >> 32);
    const uint32_t items = (uint32_t)(*a.total & 0xFFFFFFFFull);
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.nchildren; c += stride) {
        const uint64_t pre = a.prefix[c];
        const uint32_t idx = (uint32_t)(pre >> 32);
        const uint32_t ib = (uint32_t)(pre & 0xFFFFFFFFull);
        const uint64_t p = c >> a.dbits;
        const uint64_t d = c & (F - 1);
        if (d == 0) a.child_begin[p] = idx;
        if (a.vals[c] >> 32) {
            if (a.c2b) a.c2b[c] = idx;
            a.out.nkeys[idx] = a.nkeys[c];
            a.out.nruns[idx] = (uint32_t)a.nr[c];
            a.out.rbase[idx] = (uint32_t)a.runbase[c];
            a.out.keybase[idx] = a.keybase[c];
            a.out.item_begin[idx] = ib;
            a.out.digit[idx] = (uint32_t)d;
            const uint64_t pc = a.parent_coord[p];
            const int wd = a.dbits >> 1;
            const uint64_t rr = ((pc >> 32) << wd) | (d >> wd);
            const uint64_t cc = ((pc & 0xFFFFFFFFull) << wd) | (d & ((1ull << wd) - 1));
            a.out.coord[idx] = (rr << 32) | cc;
            if (a.slots) {
                const uint32_t nit = (uint32_t)(a.vals[c] & 0xFFFFFFFFull);
                int32_t sl = -1;
                if (nit > 1) {
                    sl = (int32_t)atomicAdd(a.nslots, 1ull);
                    a.slot_bucket[sl] = idx;
                }
                a.slots[idx] = sl;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.out.item_begin[count] = items;
        a.child_begin[a.nparents] = count;
    }
}
/* ------------------------------------------------------------------------ */
/* host launchers                                                            */
/* ------------------------------------------------------------------------ */

__global__ __launch_bounds__(256) void k_fill(HmFill f)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256, t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    for (int e = 0; e < f.k; e++) {
        const uint32_t w = f.word[e];
        if (f.unit[e] == 16) {
            uint4* p = (uint4*)f.p[e];
            const uint4 v = make_uint4(w, w, w, w);
            for (uint64_t i = t; i < f.bytes[e] / 16; i += stride) p[i] = v;
        } else if (f.unit[e] == 4) {
            uint32_t* p = (uint32_t*)f.p[e];
            for (uint64_t i = t; i < f.bytes[e] / 4; i += stride) p[i] = w;
        } else {
            uint8_t* p = (uint8_t*)f.p[e];
            for (uint64_t i = t; i < f.bytes[e]; i += stride) p[i] = (uint8_t)w;
        }
    }
}

void hm_fill_add(HmFill& f, void* p, int value, uint64_t bytes)
{
    if (!bytes) return;
    const uint32_t b = (uint32_t)value & 0xFFu;
    const uintptr_t a = (uintptr_t)p;
    f.p[f.k] = p;
    f.bytes[f.k] = bytes;
    f.word[f.k] = b * 0x01010101u;
    f.unit[f.k] = (a % 16 == 0 && bytes % 16 == 0) ? 16u : (a % 4 == 0 && bytes % 4 == 0) ? 4u : 1u;
    f.k++;
}

void hm_launch_fill(hipStream_t s, const HmFill& f)
{
    if (!f.k) return;
    uint64_t most = 0;
    for (int e = 0; e < f.k; e++) most = std::max<uint64_t>(most, f.bytes[e] / f.unit[e]);
    hipLaunchKernelGGL(k_fill, dim3(hm_grid(most, 256, 2048)), dim3(256), 0, s, f);
}

void hm_launch_project(hipStream_t s, const double* lat, const double* lon, int64_t n, int zoom, int64_t* row,
                       int64_t* col, uint8_t* status, unsigned long long* err_word, unsigned long long* slow)
{
    const dim3 g(hm_grid(n > 0 ? (uint64_t)n : 0, 256, 256 * 16));
    hipLaunchKernelGGL(k_project, g, dim3(256), 0, s, lat, lon, n, zoom, row, col, status, err_word, slow);
}

void hm_launch_part1(hipStream_t s, const HmPart1Args& a0, uint32_t grid, bool out16, int mode)
{
    if (grid == 0) return;
    dim3 b(HM_P1_THREADS);
    /* lat/lon input: the whole tiles in one launch (FULL), the partial last
     * tile in another; tile input (mode 1) reads its length on the device */
    const uint32_t full = mode == 1 ? 0u : (uint32_t)std::min<int64_t>(grid, a0.n / HM_T1);
    HmPart1Args a = a0;
    a.tile0 = 0;
#define HM_P1_CASE(T, M, FL, G) hipLaunchKernelGGL((k_project_partition<T, M, FL>), dim3(G), b, 0, s, a)
#define HM_P1_MODES(T, G)                             \
    do {                                              \
        if (mode == 0) HM_P1_CASE(T, 0, false, G);    \
        else if (mode == 1) HM_P1_CASE(T, 1, false, G); \
        else HM_P1_CASE(T, 2, false, G);              \
    } while (0)
    /* whole tiles: k_l1_fast, or the fused-exact re-run through
     * k_project_partition (mode 2; mode 1 has no whole tiles) */
    if (full) {
        if (mode == 0) {
            if (out16) {
                if (a.keep) hipLaunchKernelGGL((k_l1_fast<uint16_t, true>), dim3(full), b, 0, s, a);
                else hipLaunchKernelGGL((k_l1_fast<uint16_t, false>), dim3(full), b, 0, s, a);
            } else {
                if (a.keep) hipLaunchKernelGGL((k_l1_fast<uint32_t, true>), dim3(full), b, 0, s, a);
                else hipLaunchKernelGGL((k_l1_fast<uint32_t, false>), dim3(full), b, 0, s, a);
            }
        } else if (out16) HM_P1_CASE(uint16_t, 2, true, full);
        else HM_P1_CASE(uint32_t, 2, true, full);
    }
    if (grid > full) {
        a.tile0 = full;
        if (out16) HM_P1_MODES(uint16_t, grid - full);
        else HM_P1_MODES(uint32_t, grid - full);
    }
#undef HM_P1_MODES
#undef HM_P1_CASE
}

/* exact resolution of the points k_project_partition (mode 0) deferred */
__global__ __launch_bounds__(256) void k_redo(HmRedoArgs a)
{
    const uint64_t n = min((uint64_t)*a.redo_count, a.cap);   /* the list holds at most cap */
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) {
        const uint32_t i = a.redo_idx[q];
        int64_t r = 0, c = 0;
        int st = hm_row_exact(a.lat[i], a.Z, &r);
        if (st == HM_OK) st = hm_col_exact(a.lon[i], a.Z, &c);
        const bool kept = !a.keep || a.keep[i];
        const uint64_t lim = 1ull << a.Z;
        if (st != HM_OK) atomicMin(a.err_word, ((unsigned long long)i << 8) | (unsigned long long)st);
        const bool good = (st == HM_OK) & kept;
        const bool outside = good & (((uint64_t)r >= lim) | ((uint64_t)c >= lim));
        hm_exotic_append(a.x, outside, r, c, (int64_t)i);
        if (good & !outside) {
            const unsigned long long o = atomicAdd(a.out_count, 1ull);
            a.rows_out[o] = r;
            a.cols_out[o] = c;
        }
    }
}

void hm_launch_redo(hipStream_t s, const HmRedoArgs& a, uint64_t n)
{
    /* grid-stride: most calls have a handful of points */
    hipLaunchKernelGGL(k_redo, dim3(hm_grid(n, 256, 1024)), dim3(256), 0, s, a);
}

/* the exotic list overflowed its first capacity: rebuild it over every point */
template <bool FROM_TILES>
__global__ __launch_bounds__(256) void k_collect_exotic(const double* lat, const double* lon, const int64_t* rows,
                                                        const int64_t* cols, const uint8_t* keep, int64_t n, int Z,
                                                        HmExotic x)
{
    __shared__ double tab[HM_YTAB_N];
    if (!FROM_TILES) hm_load_ytab(tab);
    __syncthreads();
    const uint64_t lim = 1ull << Z;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n_up = (n + 63) & ~63ll;   /* whole waves stay in the loop */
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += stride) {
        int64_t r = 0, c = 0;
        int st = HM_E_ARG;
        if (i < n) {
            if (FROM_TILES) {
                r = rows[i];
                c = cols[i];
                st = HM_OK;
            } else {
                int slow = 0;
                st = hm_project_point(lat[i], lon[i], Z, &r, &c, &slow, tab);
            }
        }
        const bool kept = i < n && (!keep || keep[i]);
        hm_exotic_append(x, kept & (st == HM_OK) & (((uint64_t)r >= lim) | ((uint64_t)c >= lim)), r, c, i);
    }
}

void hm_launch_collect_exotic(hipStream_t s, const double* lat, const double* lon, const int64_t* rows,
                              const int64_t* cols, const uint8_t* keep, int64_t n, int Z, HmExotic x)
{
    const dim3 g(hm_grid(n > 0 ? (uint64_t)n : 0, 256, 4096));
    if (rows)
        hipLaunchKernelGGL(k_collect_exotic<true>, g, dim3(256), 0, s, lat, lon, rows, cols, keep, n, Z, x);
    else
        hipLaunchKernelGGL(k_collect_exotic<false>, g, dim3(256), 0, s, lat, lon, rows, cols, keep, n, Z, x);
}

/* Grouped counts from lat/lon: the kept points' 128-bit (group, super tile,
 * Morton) general-path keys (hm_genkey.h), built while projecting and
 * compacted, and the OR / AND of all keys (the radix sort skips digits they
 * agree on).  Errors (projection, or a tile beyond the key's fields) by input
 * index.
 *
 * The fast form: hm_project_fast (no transcendental, no call) for every
 * point; the points it cannot settle (guard band, |lat| > 85.05, a tile
 * outside the square, non-finite input: a few per million) are listed for
 * k_project_keys_slow, which takes them through the exact chain
 * (hm_project_point) -- the keys are a multiset (sorted next), so where a key
 * lands in the compacted list is free, and errors go by input index
 * (atomicMin) either way.  (One kernel with the exact chain inline ran at 2
 * waves a SIMD: 2.1 ms for 1e8 points.)
 *
 * Dense (no keep mask): every point's key goes to its own index -- no
 * compaction, no per-tile cursor atomic (one address: 49K of them took ~0.5 ms
 * for 1e8 points).  write_hi = 0: the high halves are not stored (the caller
 * runs the pass again with them when the keys turn out wide; narrow keys
 * share one high half, which the sort and the cascade take as a constant). */
#define HM_PK_PPT 8
__global__ __launch_bounds__(256) void k_project_keys_fast(HmPkArgs a)
{
    __shared__ double tab[HM_YTAB_N];
    __shared__ uint32_t scr[256 / 64 + 1];
    __shared__ unsigned long long base_s;
    hm_load_ytab(tab);
    __syncthreads();
    const double scale = hm_exp2i(a.Z), kz = HM_INV360 * scale;
    unsigned long long o_lo = 0, o_hi = 0, n_lo = ~0ull, n_hi = ~0ull;
    constexpr int64_t TILE = 256 * HM_PK_PPT;
    for (int64_t t0 = (int64_t)blockIdx.x * TILE; t0 < a.n; t0 += (int64_t)gridDim.x * TILE) {
        hm_u128 k[HM_PK_PPT];
        uint32_t pm = 0, sm = 0;
#pragma unroll
        for (int j = 0; j < HM_PK_PPT; j++) {
            const int64_t i = t0 + (int64_t)j * 256 + threadIdx.x;
            k[j] = 0;
            if (i < a.n) {
                int32_t r, c;
                const int fast = hm_project_fast(a.lat[i], a.lon[i], scale, kz, &r, &c, tab);
                sm |= (uint32_t)(!fast) << j;
                if (fast && (!a.keep || a.keep[i])) {
                    bool ok = false;
                    k[j] = hm_gen_key(r, c, a.group ? a.group[i] : 0u, a.Z, &ok);
                    if (!ok) atomicMin(a.err_word, ((unsigned long long)i << 8) | (unsigned long long)HM_E_RANGE);
                    pm |= (uint32_t)ok << j;
                    if (ok) {
                        o_lo |= (unsigned long long)k[j];
                        o_hi |= (unsigned long long)(k[j] >> 64);
                        n_lo &= (unsigned long long)k[j];
                        n_hi &= (unsigned long long)(k[j] >> 64);
                    }
                }
            }
        }
        /* the unsettled points, one list reservation a wave */
#pragma unroll
        for (int j = 0; j < HM_PK_PPT; j++) {
            const bool sl = (sm >> j) & 1u;
            const uint64_t m = __ballot(sl);
            if (!m) continue;
            unsigned long long at = 0;
            if (hm_lane() == 0) at = atomicAdd(a.redo_count, (unsigned long long)__popcll(m));
            at = __shfl(at, 0, 64) + hm_mbcnt(m);
            if (sl && at < a.redo_cap) a.redo_idx[at] = (uint32_t)(t0 + (int64_t)j * 256 + threadIdx.x);
        }
        if (a.dense) {
            /* no keep mask: every point has a key (or the call fails), at its index */
#pragma unroll
            for (int j = 0; j < HM_PK_PPT; j++)
                if ((pm >> j) & 1u) {
                    const int64_t i = t0 + (int64_t)j * 256 + threadIdx.x;
                    a.klo[i] = (uint64_t)k[j];
                    if (a.write_hi) a.khi[i] = (uint64_t)(k[j] >> 64);
                }
            continue;
        }
        uint32_t tot;
        uint32_t pos = hm_block_excl_scan<256>((uint32_t)__popc(pm), scr, &tot);
        const unsigned long long b = hm_block_reserve(a.count, tot, &base_s);
#pragma unroll
        for (int j = 0; j < HM_PK_PPT; j++)
            if ((pm >> j) & 1u) {
                a.klo[b + pos] = (uint64_t)k[j];
                if (a.write_hi) a.khi[b + pos] = (uint64_t)(k[j] >> 64);
                pos++;
            }
    }
    /* one OR / AND per block: these four words take every block's atomics */
    hm_orand_flush_block(a.orand, o_lo, o_hi, n_lo, n_hi);
}

/* the listed points through the exact chain (hm_project_point, then the key);
 * a list that overflowed its capacity: every point the fast form cannot
 * settle, found again by a sweep of the whole input */
__global__ __launch_bounds__(256) void k_project_keys_slow(HmPkArgs a)
{
    __shared__ double tab[HM_YTAB_N];
    hm_load_ytab(tab);
    __syncthreads();
    const uint64_t listed = *a.redo_count;
    const bool sweep = listed > a.redo_cap;
    const uint64_t m = sweep ? (uint64_t)a.n : listed;
    const double scale = hm_exp2i(a.Z), kz = HM_INV360 * scale;
    unsigned long long o_lo = 0, o_hi = 0, n_lo = ~0ull, n_hi = ~0ull;
    for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < m; v += (uint64_t)gridDim.x * 256) {
        const int64_t i = sweep ? (int64_t)v : (int64_t)a.redo_idx[v];
        if (sweep) {
            int32_t r, c;
            if (hm_project_fast(a.lat[i], a.lon[i], scale, kz, &r, &c, tab)) continue;
        }
        int64_t r = 0, c = 0;
        int slow = 0;
        int st = hm_project_point(a.lat[i], a.lon[i], a.Z, &r, &c, &slow, tab);
        bool ok = false;
        hm_u128 k = 0;
        if (st == HM_OK && (!a.keep || a.keep[i])) {
            k = hm_gen_key(r, c, a.group ? a.group[i] : 0u, a.Z, &ok);
            if (!ok) st = HM_E_RANGE;
        }
        if (st != HM_OK) atomicMin(a.err_word, ((unsigned long long)i << 8) | (unsigned long long)st);
        if (ok) {
            const unsigned long long q = a.dense ? (unsigned long long)i : atomicAdd(a.count, 1ull);
            a.klo[q] = (uint64_t)k;
            if (a.write_hi) a.khi[q] = (uint64_t)(k >> 64);
            o_lo |= (unsigned long long)k;
            o_hi |= (unsigned long long)(k >> 64);
            n_lo &= (unsigned long long)k;
            n_hi &= (unsigned long long)(k >> 64);
        }
    }
    /* One set of atomics per wave, and none from a wave with nothing to flush:
     * most of the 1024 blocks are idle, and their 16K same-address atomics
     * would cost ~88 per us.  "Nothing" is read off the OR, so a wave whose
     * only keys are all-zero (super tile -16, -2^47, group 0, tile 0) is
     * skipped too: this kernel's test, not a general form of the flush. */
    hm_orand_wave(o_lo, o_hi, n_lo, n_hi);
    if (hm_lane() == 0 && (o_lo | o_hi)) {
        atomicOr(&a.orand[0], o_lo);
        atomicOr(&a.orand[1], o_hi);
        atomicAnd(&a.orand[2], n_lo);
        atomicAnd(&a.orand[3], n_hi);
    }
}

void hm_launch_project_keys(hipStream_t s, const HmPkArgs& a)
{
    const dim3 g(hm_grid(a.n > 0 ? (uint64_t)a.n : 0, 256 * HM_PK_PPT, 2048));
    hipLaunchKernelGGL(k_project_keys_fast, g, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_project_keys_slow, dim3(1024), dim3(256), 0, s, a);
}

void hm_launch_partN(hipStream_t s, const HmPartNArgs& a, uint32_t items, bool out16, bool few_runs)
{
    if (items == 0) return;
    if (few_runs) {
        if (out16)
            hipLaunchKernelGGL(k_partition_fr<uint16_t>, hm_grid2(items), dim3(HM_FR_THREADS), 0, s, a);
        else
            hipLaunchKernelGGL(k_partition_fr<uint32_t>, hm_grid2(items), dim3(HM_FR_THREADS), 0, s, a);
        return;
    }
    if (out16)
        hipLaunchKernelGGL(k_partition<uint16_t>, hm_grid2(items), dim3(HM_PN_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(k_partition<uint32_t>, hm_grid2(items), dim3(HM_PN_THREADS), 0, s, a);
}

void hm_launch_rs_count(hipStream_t s, const HmRsArgs& a)
{
    hipLaunchKernelGGL(k_rs_count, dim3(hm_grid(a.nchildren << a.shard_bits, 256, 16384)), dim3(256), 0, s, a);
}

void hm_launch_rs_copy(hipStream_t s, const HmRsArgs& a)
{
    const uint64_t pairs = a.nchildren << a.shard_bits;
    if (pairs == 0) return;   /* a level with no parent buckets (nothing kept) */
    hipLaunchKernelGGL(k_rs_copy, dim3(hm_grid((a.nchildren + 63) / 64, 4, 16384)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_rs_copy_big, dim3(1024), dim3(256), 0, s, a);
}

void hm_launch_rs_keys(hipStream_t s, const HmRsArgs& a)
{
    hipLaunchKernelGGL(k_rs_keys, dim3(hm_grid(a.nchildren, 256, 16384)), dim3(256), 0, s, a);
}

/* exclusive scan of v[0, n) -> out, total -> *total.  ndev: the length is
 * min(n, *ndev), read on the device (n: the host's bound, which sizes the
 * grid) -- no read-back before the scan */
void hm_launch_scan(hipStream_t s, const uint64_t* v, uint64_t n, uint64_t* partial, uint64_t* out, uint64_t* total,
                    const uint64_t* ndev)
{
    uint64_t chunk = HM_SCAN_ITEMS;
    while ((n + chunk - 1) / chunk > HM_SCAN_MAXB) chunk += HM_SCAN_ITEMS;
    if (n <= 16 * 1024) {
        hipLaunchKernelGGL(k_scan_one<16>, dim3(1), dim3(1024), 0, s, v, (uint32_t)n, out, total, ndev);
        return;
    }
    const uint32_t nb = (uint32_t)((n + chunk - 1) / chunk);
    const uint32_t g = nb ? nb : 1;
    hipLaunchKernelGGL(k_scan_reduce, dim3(g), dim3(HM_SCAN_THREADS), 0, s, v, n, chunk, partial, ndev);
    if (g <= HM_SCAN_THREADS) {
        hipLaunchKernelGGL(k_scan_down<true>, dim3(g), dim3(HM_SCAN_THREADS), 0, s, v, n, chunk, partial, out, ndev,
                           total);
        return;
    }
    hipLaunchKernelGGL(k_scan_one<4>, dim3(1), dim3(1024), 0, s, partial, g, partial, total, nullptr);
    hipLaunchKernelGGL(k_scan_down<false>, dim3(g), dim3(HM_SCAN_THREADS), 0, s, v, n, chunk, partial, out, ndev,
                       total);
}

void hm_launch_compact(hipStream_t s, const HmCompactArgs& a)
{
    hipLaunchKernelGGL(k_compact, dim3(hm_grid(a.nchildren, 256, 8192)), dim3(256), 0, s, a);
}

/* ------------------------------------------------------------------------ */
/* synthetic point clouds (bit-identical to heatmap_amd/synth.py)            */
/* ------------------------------------------------------------------------ */

__device__ __forceinline__ uint64_t hm_splitmix(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ double hm_u01(uint64_t seed, uint64_t idx, uint32_t lane, uint32_t lanes)
{
    const uint64_t ctr = seed * 0x100000001B3ull + idx * lanes + lane;
    return (double)(hm_splitmix(ctr) >> 11) * 0x1p-53;
}

__global__ __launch_bounds__(256) void k_synth(int kind, uint64_t seed, int64_t start, int64_t n, double* lat,
                                               double* lon, const double* tab, int k)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t idx = (uint64_t)(start + i);
        double la, lo;
        if (kind == 0) {
            const double u1 = hm_u01(seed, idx, 0, 2), u2 = hm_u01(seed, idx, 1, 2);
            la = (u1 * 2.0 - 1.0) * 85.0511287798066;
            lo = u2 * 360.0 - 180.0;
        } else if (kind == 1) {
            const double u0 = hm_u01(seed, idx, 0, 9);
            int c = 0;
            while (c < k - 1 && !(tab[3 * k + c] > u0)) c++;
            double sy = hm_u01(seed, idx, 1, 9) + hm_u01(seed, idx, 2, 9);
            sy = sy + hm_u01(seed, idx, 3, 9);
            sy = sy + hm_u01(seed, idx, 4, 9);
            double sx = hm_u01(seed, idx, 5, 9) + hm_u01(seed, idx, 6, 9);
            sx = sx + hm_u01(seed, idx, 7, 9);
            sx = sx + hm_u01(seed, idx, 8, 9);
            const double gy = (sy - 2.0) * 1.7320508075688772;
            const double gx = (sx - 2.0) * 1.7320508075688772;
            la = tab[c] + tab[2 * k + c] * gy;
            lo = tab[k + c] + tab[2 * k + c] * gx;
        } else {
            const double u0 = hm_u01(seed, idx, 0, 3), u1 = hm_u01(seed, idx, 1, 3), u2 = hm_u01(seed, idx, 2, 3);
            const double w = 360.0 / 262144.0;
            if (u0 < 0.9) {
                la = 47.60014 + (u1 - 0.5) * 0.0008;
                lo = (42015.0 + 0.0625 + u2 * 0.875) * w - 180.0;
            } else {
                la = (u1 * 2.0 - 1.0) * 85.0511287798066;
                lo = u2 * 360.0 - 180.0;
            }
        }
        lat[i] = la;
        lon[i] = lo;
    }
}

void hm_launch_synth(hipStream_t s, int kind, uint64_t seed, int64_t start, int64_t n, double* lat, double* lon,
                     const double* tab, int k)
{
    const dim3 g(hm_grid(n > 0 ? (uint64_t)n : 0, 256, 256 * 32));
    hipLaunchKernelGGL(k_synth, g, dim3(256), 0, s, kind, seed, start, n, lat, lon, tab, k);
}

/* ------------------------------------------------------------------------ */
/* HBM read-stream peak (bench.py's measured_peak): K1's access shape without  */
/* its arithmetic -- two fp64 arrays read once, 16 B per lane per load (the   */
/* double2 loads of k_project_partition), HM_RS_INFLIGHT loads in flight per */
/* lane, one XOR per block written so nothing is dead.                       */
/* ------------------------------------------------------------------------ */
#define HM_RS_THREADS 512
#define HM_RS_V 4   /* 16-B loads in flight per lane and array (8 in all, K1 has 16) */
__global__ __launch_bounds__(HM_RS_THREADS) void k_read_stream(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                                            uint64_t n16, uint64_t* __restrict__ sink)
{
    constexpr uint64_t TILE = (uint64_t)HM_RS_THREADS * HM_RS_V;   /* vectors of each array per tile */
    uint32_t acc = 0;
    for (uint64_t t0 = (uint64_t)blockIdx.x * TILE; t0 < n16; t0 += (uint64_t)gridDim.x * TILE) {
        uint4 va[HM_RS_V], vb[HM_RS_V];
        if (t0 + TILE <= n16) {
#pragma unroll
            for (int k = 0; k < HM_RS_V; k++) {
                va[k] = a[t0 + (uint64_t)k * HM_RS_THREADS + threadIdx.x];
                vb[k] = b[t0 + (uint64_t)k * HM_RS_THREADS + threadIdx.x];
            }
        } else {
#pragma unroll
            for (int k = 0; k < HM_RS_V; k++) {
                const uint64_t i = t0 + (uint64_t)k * HM_RS_THREADS + threadIdx.x;
                va[k] = i < n16 ? a[i] : make_uint4(0u, 0u, 0u, 0u);
                vb[k] = i < n16 ? b[i] : make_uint4(0u, 0u, 0u, 0u);
            }
        }
#pragma unroll
        for (int k = 0; k < HM_RS_V; k++)
            acc ^= va[k].x ^ va[k].y ^ va[k].z ^ va[k].w ^ vb[k].x ^ vb[k].y ^ vb[k].z ^ vb[k].w;
    }
    acc = hm_wave_sum(acc);
    if (hm_lane() == 0 && acc == 0x9E3779B9u) sink[blockIdx.x] = acc;   /* data-dependent: the loads stay live */
}

void hm_launch_read_stream(hipStream_t s, const void* a, const void* b, uint64_t bytes_each, uint64_t* sink)
{
    const uint64_t n16 = bytes_each / 16;
    hipLaunchKernelGGL(k_read_stream, dim3(hm_grid(n16, HM_RS_THREADS * HM_RS_V, 256 * 16)), dim3(HM_RS_THREADS), 0, s,
                       (const uint4*)a, (const uint4*)b, n16, sink);
}
