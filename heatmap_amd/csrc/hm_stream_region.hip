/* Region queries on the resident streaming heatmap (hm_stream_region_series,
 * hm_stream_region_view, hm_stream_region_visitors; the table is hm_region.h,
 * the arguments HmsRegionArgs in hm_pipeline.h).
 *
 * A rectangle selects space with four compares; a district, a geofence or a
 * choropleth does not fit a few rectangles.  A region set gives every covered
 * row of one zoom its column spans, and the filter pass of k_stream_view keeps
 * its shape: HMS_VW_U keys per thread loaded together, one ballot on the id
 * interval of the covered rows -- a wave with no cell of the regions' zoom and
 * rows costs its keys and nothing else -- then, for the cells inside it, the
 * row's spans (hms_region_next).  Only a cell that a span covers reads its
 * bucket key (hours, group), only a survivor its count.  What happens to a
 * survivor is the sink's: per-(frame, region) totals reduced on the device,
 * the cells themselves for the view's merge and emit, or (region, group)
 * records for the distinct visitors per region. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/heatmap_amd.h"
#include "hm_device.h"
#include "hm_pipeline.h"
#include "hm_table.h"
#include "hm_stream_dev.h"
#define HMS_REGION_FN __host__ __device__ __forceinline__   /* hms_region_next on the device */
#include "hm_region.h"
#define HM_VISIT_FN __device__ __forceinline__   /* hm_visit_judge on the device */
#include "hm_visit.h"

#ifndef HMS_VW_U
#define HMS_VW_U 8
#endif

#define HMS_RG_NOKEY 0xFFFFFFFFFFFFFFFFull   /* empty slot of the records table (a region is below 2^12) */

/* out[idx] += c for the lanes with ok, equal idx summed across the wave first:
 * one turn per distinct idx (the first HMS_RG_TURNS of the row; the others add
 * alone).  Every lane of the wave calls. */
__device__ __forceinline__ void hms_rg_wave_add(unsigned long long* out, uint32_t idx, uint64_t c, bool ok)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t left = __ballot(ok);
    for (int turn = 0; left; turn++) {
        if (turn == HMS_RG_TURNS) {
            if ((left >> lane) & 1ull) atomicAdd(&out[idx], (unsigned long long)c);
            break;
        }
        const int leader = __ffsll((unsigned long long)left) - 1;
        const uint32_t i0 = __shfl(idx, leader, 64);
        const bool mine = ok && idx == i0;
        uint64_t t = mine ? c : 0ull;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor((unsigned long long)t, d, 64);
        if ((int)lane == leader) atomicAdd(&out[i0], (unsigned long long)t);
        left &= ~__ballot(mine);
    }
}

template <int SINK>
__device__ __forceinline__ void hms_region_pass(const HmsRegionArgs& a)
{
    constexpr int U = HMS_VW_U;
    extern __shared__ unsigned long long hms_rg_lds[];
    __shared__ uint32_t scr[256 / 64 + 1];
    __shared__ unsigned long long sbase;
    const HmsViewArgs& v = a.v;
    const int tid = threadIdx.x;
    const uint32_t lane = (uint32_t)tid & 63u;
    const uint64_t cmask = (1ull << v.cb) - 1ull;
    const uint32_t zmask = (1u << a.z) - 1u;
    /* the block's LDS: the sink's 64-bit words, then the staged table */
    const bool tot_lds = SINK == HMS_RG_SINK_TOTALS && a.ntot <= HMS_RG_TOT_LDS;
    const uint32_t n64 = SINK == HMS_RG_SINK_TOTALS ? (tot_lds ? a.ntot : 0u)
                                                    : (SINK == HMS_RG_SINK_RECORDS ? 2u * HMS_RG_REC_SLOTS : 0u);
    unsigned long long* acc = hms_rg_lds;                       /* totals */
    unsigned long long* tk = hms_rg_lds;                        /* records: keys, then sums */
    unsigned long long* ts = hms_rg_lds + HMS_RG_REC_SLOTS;
    uint32_t* tab = (uint32_t*)(hms_rg_lds + n64);
    if (SINK == HMS_RG_SINK_TOTALS)
        for (uint32_t j = tid; j < n64; j += 256) acc[j] = 0ull;
    if (SINK == HMS_RG_SINK_RECORDS)
        for (uint32_t j = tid; j < HMS_RG_REC_SLOTS; j += 256) {
            tk[j] = HMS_RG_NOKEY;
            ts[j] = 0ull;
        }
    const uint32_t* rp = a.row_ptr;
    const uint32_t* cl = a.col_lo;
    const uint32_t* ch = a.col_hi;
    const uint32_t* rg = a.region;
    if (a.stage) {
        uint32_t* t_rp = tab;
        uint32_t* t_cl = tab + a.nrows + 1;
        uint32_t* t_ch = t_cl + a.nspans;
        uint32_t* t_rg = t_ch + a.nspans;
        for (uint32_t j = tid; j <= a.nrows; j += 256) t_rp[j] = a.row_ptr[j];
        for (uint32_t j = tid; j < a.nspans; j += 256) {
            t_cl[j] = a.col_lo[j];
            t_ch[j] = a.col_hi[j];
            t_rg[j] = a.region[j];
        }
        rp = t_rp, cl = t_cl, ch = t_ch, rg = t_rg;
    }
    __syncthreads();

    uint32_t bclaimed = 0, full = 0, npairs = 0;
    uint64_t wk = HMS_EMPTY;          /* cells: the wave's last shared label and its bucket */
    uint32_t wb = HMS_NO_BUCKET;
    constexpr uint64_t CH = 256 * U;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < v.n; c0 += (uint64_t)gridDim.x * CH) {
        uint64_t k[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            k[u] = i < v.n ? v.keys[i] : 0ull;
        }
        uint32_t box = 0;             /* bit u: cell u lies in the covered rows' id interval */
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            box |= (uint32_t)(i < v.n && (k[u] & cmask) - a.id_lo < a.id_span) << u;
        }
        if (!__ballot(box != 0)) continue;
        int32_t sp[U];                /* the first span that covers cell u, or -1 */
        uint32_t hit = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t d = (k[u] & cmask) - a.id_lo;
            sp[u] = (box >> u) & 1u ? (int32_t)hms_region_next(rp, cl, ch, (uint32_t)(d >> a.z), (uint32_t)d & zmask, 0)
                                    : -1;
            hit |= (uint32_t)(sp[u] >= 0) << u;
        }
        if (!__ballot(hit != 0)) continue;
        uint64_t bk[U], lk[U], cn[U];
        uint32_t sel = 0;             /* bit u: ... of the wanted hours and group */
#pragma unroll
        for (int u = 0; u < U; u++) {
            bk[u] = (hit >> u) & 1u ? v.buckets.keys[(k[u] >> v.cb) & v.buckets.mask] : 0ull;
            lk[u] = (hit >> u) & 1u ? hms_view_key(v, bk[u]) : ~0ull;
            sel |= (uint32_t)(lk[u] != ~0ull) << u;
        }
        if (!__ballot(sel != 0)) continue;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            cn[u] = (sel >> u) & 1u ? v.counts[i] : 0ull;
        }

        if (SINK == HMS_RG_SINK_TOTALS) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const bool act = (sel >> u) & 1u;
                const uint64_t d = (k[u] & cmask) - a.id_lo;
                const uint32_t rr = (uint32_t)(d >> a.z), cc = (uint32_t)d & zmask;
                uint32_t fr = 0;      /* the survivor's frame, counted from the first clamped hour's */
                if (act && !v.alltime) {
                    const uint32_t x = (uint32_t)bk[u] - v.lo + a.phase;
                    fr = a.fh == 1 ? x : x / a.fh;
                }
                int32_t j = act ? sp[u] : -1;
                while (__ballot(j >= 0)) {          /* one step per covering span of the row's deepest cell */
                    const bool on = j >= 0;
                    const uint32_t idx = on ? fr * a.nregions + rg[j] : 0u;
                    const bool ok = on && idx < a.ntot;
                    if (tot_lds) {
                        if (ok) atomicAdd(&acc[idx], (unsigned long long)cn[u]);
                    } else {
                        hms_rg_wave_add(a.totals, idx, cn[u], ok);
                    }
                    if (on) j = (int32_t)hms_region_next(rp, cl, ch, rr, cc, (int64_t)j + 1);
                }
            }
        }

        if (SINK == HMS_RG_SINK_CELLS) {   /* k_stream_view's writes */
            uint64_t bal[U];
            uint32_t tot = 0;
#pragma unroll
            for (int u = 0; u < U; u++) {
                bal[u] = __ballot(lk[u] != ~0ull);
                tot += (uint32_t)__popcll(bal[u]);
            }
            unsigned long long first = 0;
            if (lane == 0) first = atomicAdd(v.cursor, (unsigned long long)tot);
            uint64_t wq = __shfl(first, 0, 64);
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (!bal[u]) continue;
                const bool in = (bal[u] >> lane) & 1ull;
                const int leader = __ffsll((unsigned long long)bal[u]) - 1;
                const uint64_t k0 = __shfl((unsigned long long)lk[u], leader, 64);
                if (k0 != wk) {
                    uint32_t b0 = 0;
                    if ((int)lane == leader) b0 = hms_intern(v.buckets, k0, &bclaimed);
                    wb = __shfl(b0, leader, 64);
                    wk = k0;
                }
                uint32_t b = wb;
                if (in && lk[u] != k0) b = hms_intern(v.buckets, lk[u], &bclaimed);
                if (in) {
                    full |= b == HMS_NO_BUCKET;   /* the caller discards the view */
                    const uint64_t q = wq + hm_mbcnt(bal[u]);
                    v.keys_out[q] = ((uint64_t)(b == HMS_NO_BUCKET ? 0u : b) << v.cb) | (k[u] & cmask);
                    v.counts_out[q] = cn[u];
                }
                wq += (uint64_t)__popcll(bal[u]);
            }
        }

        if (SINK == HMS_RG_SINK_RECORDS) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const bool act = (sel >> u) & 1u;
                const uint64_t d = (k[u] & cmask) - a.id_lo;
                const uint32_t rr = (uint32_t)(d >> a.z), cc = (uint32_t)d & zmask;
                const uint32_t g = (uint32_t)(bk[u] >> 32);
                int32_t j = act ? sp[u] : -1;
                while (__ballot(j >= 0)) {
                    const bool on = j >= 0;
                    const uint64_t key = on ? ((uint64_t)rg[j] << 32) | g : 0ull;
                    npairs += on;
                    bool placed = false;
                    if (on) {
                        uint32_t sl = (uint32_t)hms_hash(key) & (HMS_RG_REC_SLOTS - 1);
                        for (int probe = 0; probe < HMS_RG_REC_PROBES && !placed; probe++) {
                            const unsigned long long o = atomicCAS(&tk[sl], HMS_RG_NOKEY, (unsigned long long)key);
                            placed = o == HMS_RG_NOKEY || o == key;
                            if (placed) atomicAdd(&ts[sl], (unsigned long long)cn[u]);
                            sl = (sl + 1) & (HMS_RG_REC_SLOTS - 1);
                        }
                    }
                    const uint64_t spill = __ballot(on && !placed);   /* no slot: written as it is */
                    if (spill) {
                        unsigned long long first = 0;
                        if ((int)lane == __ffsll((unsigned long long)spill) - 1)
                            first = atomicAdd(v.cursor, (unsigned long long)__popcll(spill));
                        first = __shfl(first, __ffsll((unsigned long long)spill) - 1, 64);
                        const uint64_t q = first + hm_mbcnt(spill);
                        if (on && !placed && q < a.capacity) {
                            v.keys_out[q] = key;
                            v.counts_out[q] = cn[u];
                        }
                    }
                    if (on) j = (int32_t)hms_region_next(rp, cl, ch, rr, cc, (int64_t)j + 1);
                }
            }
        }
    }

    if (SINK == HMS_RG_SINK_TOTALS && tot_lds) {   /* the block's table: its sums out, once */
        __syncthreads();
        for (uint32_t j = tid; j < a.ntot; j += 256)
            if (acc[j]) atomicAdd(&a.totals[j], acc[j]);
    }
    if (SINK == HMS_RG_SINK_CELLS) {
        uint64_t w[2] = {bclaimed, full};
        hms_block_sums(w);
        if (tid == 0) {
            if (w[0]) atomicAdd(&v.state[HMS_ST_BUCKETS], (unsigned long long)w[0]);
            if (w[1]) atomicAdd(&v.state[HMS_ST_BFULL], (unsigned long long)w[1]);
        }
    }
    if (SINK == HMS_RG_SINK_RECORDS) {             /* the block's table: its sums out, one reservation */
        __syncthreads();
        constexpr int SPT = HMS_RG_REC_SLOTS / 256;
        uint32_t c = 0;
        for (int j = 0; j < SPT; j++) c += tk[tid * SPT + j] != HMS_RG_NOKEY;
        uint32_t total;
        uint32_t off = hm_block_excl_scan<256>(c, scr, &total);
        const unsigned long long base = hm_block_reserve(v.cursor, total, &sbase);
        for (int j = 0; j < SPT; j++) {
            const uint32_t sl = tid * SPT + j;
            if (tk[sl] != HMS_RG_NOKEY) {
                if (base + off < a.capacity) {
                    v.keys_out[base + off] = tk[sl];
                    v.counts_out[base + off] = ts[sl];
                }
                off++;
            }
        }
        uint64_t w[1] = {npairs};
        hms_block_sums(w);
        if (tid == 0 && w[0]) atomicAdd(&v.state[HMS_ST_PAIRS], (unsigned long long)w[0]);
    }
}

__global__ __launch_bounds__(256) void k_stream_region_totals(HmsRegionArgs a)
{
    hms_region_pass<HMS_RG_SINK_TOTALS>(a);
}
__global__ __launch_bounds__(256) void k_stream_region_cells(HmsRegionArgs a)
{
    hms_region_pass<HMS_RG_SINK_CELLS>(a);
}
__global__ __launch_bounds__(256) void k_stream_region_records(HmsRegionArgs a)
{
    hms_region_pass<HMS_RG_SINK_RECORDS>(a);
}

/* Distinct visitors per region, the fold: the merged records are distinct
 * (region, group) pairs, so a region's visitors are the records that name it
 * and its points their counts' sum.  Regions are few and records many: a
 * block adds into arrays of its own in LDS (nregions <= HM_REGION_MAX_REGIONS:
 * 48 KB at most) and to the global ones once, when it ends. */
__global__ __launch_bounds__(256) void k_region_visit_fold(const uint64_t* __restrict__ keys,
                                                           const uint64_t* __restrict__ counts, uint64_t n,
                                                           uint32_t nregions, unsigned long long* __restrict__ points,
                                                           uint32_t* __restrict__ visitors)
{
    extern __shared__ unsigned long long hms_rg_lds[];
    unsigned long long* pts = hms_rg_lds;
    uint32_t* vis = (uint32_t*)(hms_rg_lds + nregions);
    for (uint32_t j = threadIdx.x; j < nregions; j += 256) {
        pts[j] = 0ull;
        vis[j] = 0u;
    }
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t r = (uint32_t)(keys[i] >> 32);
        if (r < nregions) {
            atomicAdd(&pts[r], (unsigned long long)counts[i]);
            atomicAdd(&vis[r], 1u);
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nregions; j += 256)
        if (vis[j]) {
            atomicAdd(&points[j], pts[j]);
            atomicAdd(&visitors[j], vis[j]);
        }
}

/* the threshold (hm_visit_judge), one block: the regions below it are zeroed
 * and counted */
__global__ __launch_bounds__(256) void k_region_visit_sweep(uint32_t nregions, uint64_t min_visitors,
                                                            uint64_t* __restrict__ points,
                                                            uint32_t* __restrict__ visitors, unsigned long long* state)
{
    HmVisitWithheld wh = {0, 0};
    for (uint32_t j = threadIdx.x; j < nregions; j += 256) {
        const uint32_t vj = visitors[j];
        if (vj && !hm_visit_judge(&wh, vj, points[j], min_visitors)) {
            points[j] = 0ull;
            visitors[j] = 0u;
        }
    }
    uint64_t w[2] = {wh.cells, wh.points};
    hms_block_sums(w);
    if (threadIdx.x == 0 && w[0]) {
        atomicAdd(&state[HMS_ST_WCELLS], (unsigned long long)w[0]);
        atomicAdd(&state[HMS_ST_WPOINTS], (unsigned long long)w[1]);
    }
}

uint32_t hm_stream_region_blocks(uint64_t n)
{
    const uint64_t chunks = (n + 256 * HMS_VW_U - 1) / (256 * HMS_VW_U);
    return (uint32_t)(chunks < 2048 ? chunks : 2048);
}

void hm_launch_stream_region(hipStream_t s, const HmsRegionArgs& a, int sink)
{
    if (!a.v.n) return;
    const dim3 grid(hm_stream_region_blocks(a.v.n));
    size_t lds = a.stage ? ((size_t)a.nrows + 1 + 3 * (size_t)a.nspans) * 4 : 0;
    if (sink == HMS_RG_SINK_TOTALS) {
        lds += a.ntot <= HMS_RG_TOT_LDS ? (size_t)a.ntot * 8 : 0;
        hipLaunchKernelGGL(k_stream_region_totals, grid, dim3(256), lds, s, a);
    } else if (sink == HMS_RG_SINK_CELLS) {
        hipLaunchKernelGGL(k_stream_region_cells, grid, dim3(256), lds, s, a);
    } else {
        lds += 2 * (size_t)HMS_RG_REC_SLOTS * 8;
        hipLaunchKernelGGL(k_stream_region_records, grid, dim3(256), lds, s, a);
    }
}

void hm_launch_region_visit_fold(hipStream_t s, const uint64_t* keys, const uint64_t* counts, uint64_t n,
                                 uint32_t nregions, uint64_t* points, uint32_t* visitors)
{
    if (!n) return;
    uint64_t b = (n + 2047) / 2048;   /* 8 records per thread and more: a block's arrays are flushed once */
    if (b > 256) b = 256;
    hipLaunchKernelGGL(k_region_visit_fold, dim3((unsigned)b), dim3(256), (size_t)nregions * 12, s, keys, counts, n,
                       nregions, (unsigned long long*)points, visitors);
}

void hm_launch_region_visit_sweep(hipStream_t s, uint32_t nregions, uint64_t min_visitors, uint64_t* points,
                                  uint32_t* visitors, unsigned long long* state)
{
    hipLaunchKernelGGL(k_region_visit_sweep, dim3(1), dim3(256), 0, s, nregions, min_visitors, points, visitors, state);
}
