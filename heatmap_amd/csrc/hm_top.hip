/* Top-k selection over (key, count) records (hm_cells_top, hm_stream_top,
 * hm_stream_top_groups): the first k records in rank order -- the larger count
 * first, equal counts by the smaller key, both unsigned 64-bit -- picked and
 * ordered on the device, with no host read-back between the passes.
 *
 *   k_top_reduce   OR and AND of every count and of every key (one pass): a
 *                  digit in which no two records differ needs no pass, so
 *                  counts below 2^16 walk two digits, equal counts none.
 *   k_top_pass     one digit pass of the MSD radix walk (hm_top_select.h),
 *                  launched HM_TOP_PASSES times.  Launch j first decides the
 *                  digit of pass j - 1 from that pass's global histogram --
 *                  every block does, they all reach the same state, block 0
 *                  stores it for launch j + 1 -- then counts the records that
 *                  agree with the decided bits by their next digit: per-block
 *                  LDS histograms (a wave whose records share a digit adds
 *                  once) added into the pass's global histogram.  The walk runs
 *                  over the counts, descending, to the k-th largest count T and
 *                  the records above it; when more records tie at T than are
 *                  still wanted it goes on over the keys of those ties,
 *                  ascending, to the last key taken.  A launch after the walk
 *                  has ended copies the state and leaves.
 *   k_top_collect  the records with count > T, or count == T and key <= that
 *                  key (of records that repeat that very key, as many as are
 *                  still wanted): exactly k; ranks by ballot, one reservation
 *                  per wave.
 *   k_top_sort     one block: the <= HM_TOP_MAX_K collected records (or, when
 *                  n <= k, the input itself) through a bitonic network in LDS
 *                  into rank order.
 *   k_top_narrow   ranked u64 group ids -> the u32 array of hm_stream_top_groups.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#define HM_TOP_FN __host__ __device__ __forceinline__   /* the digit walk on the device (before hm_pipeline.h) */
#include "../../include/heatmap_amd.h"
#include "hm_device.h"
#include "hm_pipeline.h"

static_assert(HM_TOP_BINS == 256 && HM_TOP_THREADS == 256, "one histogram bin per thread");
static_assert(HM_TOP_PASSES == 2 * (64 / HM_TOP_DIGIT_BITS), "a count walk and a key walk");
static_assert(sizeof(HmTopState) % 8 == 0, "states are copied as words");

__global__ __launch_bounds__(HM_TOP_THREADS) void k_top_reduce(HmTopArgs a)
{
    __shared__ unsigned long long r[4];
    const int tid = threadIdx.x;
    if (tid < 4) r[tid] = 0;
    __syncthreads();
    uint64_t oc = 0, nc = 0, ok = 0, nk = 0;
    const uint64_t stride = (uint64_t)gridDim.x * HM_TOP_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * HM_TOP_THREADS + tid; i < a.n; i += stride) {
        const uint64_t c = a.counts[i], k = a.keys[i];
        oc |= c, nc |= ~c, ok |= k, nk |= ~k;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        oc |= __shfl_xor((unsigned long long)oc, d, 64);
        nc |= __shfl_xor((unsigned long long)nc, d, 64);
        ok |= __shfl_xor((unsigned long long)ok, d, 64);
        nk |= __shfl_xor((unsigned long long)nk, d, 64);
    }
    if ((tid & 63) == 0) {
        atomicOr(&r[0], (unsigned long long)oc);
        atomicOr(&r[1], (unsigned long long)nc);
        atomicOr(&r[2], (unsigned long long)ok);
        atomicOr(&r[3], (unsigned long long)nk);
    }
    __syncthreads();
    if (tid < 4 && r[tid]) atomicOr(&a.words[HM_TOP_W_ORC + tid], r[tid]);
}

/* the ties at the count walk's value: all of them wanted (no key walk: every
 * key passes), or a walk over their keys to the last one taken */
__device__ __forceinline__ void top_enter_keys(HmTopState& S, uint64_t ties, const unsigned long long* words)
{
    if (ties <= S.c.want) {
        S.k.prefix = ~0ull;
        S.k.want = ~0ull;
        S.k.shift = -1;
        S.phase = HM_TOP_DONE;
        return;
    }
    S.k = hm_top_walk_begin(words[HM_TOP_W_ORK], ~words[HM_TOP_W_NANDK], S.c.want);
    S.phase = S.k.shift < 0 ? HM_TOP_DONE : HM_TOP_KEYS;
}

/* a pass's pick in two levels, so one thread walks 16 + 16 bins and not 256:
 * first over the sums of 16 neighbouring digits, then inside the chosen 16 */
__device__ __forceinline__ uint64_t top_step(HmTopWalk& w, const uint64_t* hist, const uint64_t* sums, int descending)
{
    const HmTopPick g = hm_top_pick(sums, 16, w.want, descending);
    const HmTopPick p = hm_top_pick(hist + 16 * g.digit, 16, g.want, descending);
    hm_top_walk_decided(&w, 16 * g.digit + p.digit, g.beyond + p.beyond, p.want);
    return p.size;
}

/* The state launch `step` works from: step 0 starts the count walk from the
 * reduction's words, step j > 0 decides pass j - 1.  Every block computes it;
 * block 0 stores it.  The whole block calls this. */
__device__ __forceinline__ HmTopState top_advance(const HmTopArgs& a, int step)
{
    __shared__ uint64_t gh[HM_TOP_BINS];
    __shared__ uint64_t gs[16];
    __shared__ HmTopState sh;
    const int tid = threadIdx.x;
    const bool first = step == 0;
    if (!first) gh[tid] = a.hist[(size_t)(step - 1) * HM_TOP_BINS + tid];
    __syncthreads();
    if (!first && tid < 16) {
        uint64_t t = 0;
        for (int j = 0; j < 16; j++) t += gh[16 * tid + j];
        gs[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        HmTopState S;
        if (first) {
            S.c = hm_top_walk_begin(a.words[HM_TOP_W_ORC], ~a.words[HM_TOP_W_NANDC], a.k);
            S.k = HmTopWalk{~0ull, 0, 0, 0, 0, -1, 0};
            S.phase = HM_TOP_COUNTS;
            S.pad = 0;
            if (S.c.shift < 0) top_enter_keys(S, a.n, a.words);   /* every count the same */
        } else {
            S = a.states[step - 1];
            if (S.phase == HM_TOP_COUNTS) {
                const uint64_t size = top_step(S.c, gh, gs, 1);
                if (S.c.shift < 0) top_enter_keys(S, size, a.words);
            } else if (S.phase == HM_TOP_KEYS) {
                top_step(S.k, gh, gs, 0);
                if (S.k.shift < 0) S.phase = HM_TOP_DONE;
            }
        }
        sh = S;
        if (blockIdx.x == 0) a.states[step] = S;
    }
    __syncthreads();
    return sh;
}

__global__ __launch_bounds__(HM_TOP_THREADS) void k_top_pass(HmTopArgs a, int step)
{
    __shared__ uint32_t lh[HM_TOP_BINS];
    const int tid = threadIdx.x;
    const uint32_t lane = (uint32_t)tid & 63u;
    const HmTopState S = top_advance(a, step);
    if (S.phase == HM_TOP_DONE) return;
    const bool on_keys = S.phase == HM_TOP_KEYS;
    const HmTopWalk w = on_keys ? S.k : S.c;
    const uint64_t mask = hm_top_mask(w.shift), T = S.c.prefix;
    lh[tid] = 0;
    __syncthreads();
    for (uint64_t b = (uint64_t)blockIdx.x * HM_TOP_THREADS; b < a.n; b += (uint64_t)gridDim.x * HM_TOP_THREADS) {
        const uint64_t i = b + tid;
        const uint64_t c = i < a.n ? a.counts[i] : 0ull;
        bool in = i < a.n && (on_keys ? c == T : (c & mask) == w.prefix);
        uint64_t v = c;
        if (on_keys) {
            v = in ? a.keys[i] : 0ull;
            in = in && (v & mask) == w.prefix;
        }
        const uint32_t d = (uint32_t)(v >> w.shift) & (HM_TOP_BINS - 1u);
        const uint64_t act = __ballot(in);
        if (!act) continue;
        /* the records of a wave mostly share the digit (a prefix pass over
         * small counts): they add once */
        const int leader = __ffsll((unsigned long long)act) - 1;
        const uint32_t d0 = __shfl(d, leader, 64);
        const uint64_t same = __ballot(in && d == d0);
        if ((int)lane == leader) atomicAdd(&lh[d0], (uint32_t)__popcll(same));
        if (in && d != d0) atomicAdd(&lh[d], 1u);
    }
    __syncthreads();
    if (lh[tid]) atomicAdd(&a.hist[(size_t)step * HM_TOP_BINS + tid], (unsigned long long)lh[tid]);
}

__global__ __launch_bounds__(HM_TOP_THREADS) void k_top_collect(HmTopArgs a)
{
    const int tid = threadIdx.x;
    const uint32_t lane = (uint32_t)tid & 63u;
    const HmTopState S = top_advance(a, HM_TOP_PASSES);
    /* of the records at (T, tkey) -- one, unless keys repeat -- the first S.k.want that come */
    const uint64_t T = S.c.prefix, tkey = S.k.prefix, last_want = S.k.want;
    for (uint64_t b = (uint64_t)blockIdx.x * HM_TOP_THREADS; b < a.n; b += (uint64_t)gridDim.x * HM_TOP_THREADS) {
        const uint64_t i = b + tid;
        const uint64_t c = i < a.n ? a.counts[i] : 0ull;
        const uint64_t k = i < a.n ? a.keys[i] : 0ull;
        bool take = i < a.n && (c > T || (c == T && k <= tkey));
        const uint64_t eq = __ballot(take && c == T && k == tkey && last_want != ~0ull);
        if (eq) {
            unsigned long long e0 = 0;
            if ((int)lane == __ffsll((unsigned long long)eq) - 1)
                e0 = atomicAdd(&a.words[HM_TOP_W_LAST], (unsigned long long)__popcll(eq));
            e0 = __shfl(e0, __ffsll((unsigned long long)eq) - 1, 64);
            if (((eq >> lane) & 1ull) && e0 + hm_mbcnt(eq) >= last_want) take = false;
        }
        const uint64_t bal = __ballot(take);
        if (!bal) continue;
        unsigned long long first = 0;
        if (lane == 0) first = atomicAdd(&a.words[HM_TOP_W_CURSOR], (unsigned long long)__popcll(bal));
        const uint64_t q = __shfl(first, 0, 64) + hm_mbcnt(bal);
        if (take && q < a.k) {   /* (exactly k records pass; the room holds k) */
            a.sel_keys[q] = k;
            a.sel_counts[q] = c;
        }
    }
}

/* a ranks before b */
__device__ __forceinline__ bool top_before(uint64_t ka, uint64_t ca, uint64_t kb, uint64_t cb)
{
    return ca > cb || (ca == cb && ka < kb);
}

__global__ __launch_bounds__(HM_TOP_SORT_THREADS) void k_top_sort(const uint64_t* __restrict__ keys,
                                                                  const uint64_t* __restrict__ counts, uint64_t m,
                                                                  const unsigned long long* __restrict__ m_dev,
                                                                  uint64_t* __restrict__ keys_out,
                                                                  uint64_t* __restrict__ counts_out)
{
    __shared__ uint64_t sk[HM_TOP_MAX_K];
    __shared__ uint64_t sc[HM_TOP_MAX_K];
    const uint32_t tid = threadIdx.x;
    if (m_dev && *m_dev < m) m = *m_dev;
    if (m > HM_TOP_MAX_K) m = HM_TOP_MAX_K;
    uint32_t P = 2;
    while (P < m) P <<= 1;
    /* padded with records that rank last (an equal real record is the same record) */
    for (uint32_t i = tid; i < P; i += HM_TOP_SORT_THREADS) {
        sk[i] = i < m ? keys[i] : ~0ull;
        sc[i] = i < m ? counts[i] : 0ull;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < P / 2; t += HM_TOP_SORT_THREADS) {
                const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;   /* this run ends in rank order */
                const uint64_t ka = sk[lo], ca = sc[lo], kb = sk[hi], cb = sc[hi];
                if (top_before(kb, cb, ka, ca) == up) {
                    sk[lo] = kb, sc[lo] = cb;
                    sk[hi] = ka, sc[hi] = ca;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < m; i += HM_TOP_SORT_THREADS) {
        keys_out[i] = sk[i];
        counts_out[i] = sc[i];
    }
}

__global__ __launch_bounds__(256) void k_top_narrow(const uint64_t* __restrict__ keys,
                                                    const uint64_t* __restrict__ counts, uint64_t m,
                                                    uint32_t* __restrict__ ids_out, uint64_t* __restrict__ counts_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        ids_out[i] = (uint32_t)keys[i];
        counts_out[i] = counts[i];
    }
}

void hm_launch_top_select(hipStream_t s, const HmTopArgs& a)
{
    const dim3 grid(hm_grid(a.n, HM_TOP_THREADS * 16, 1024)), block(HM_TOP_THREADS);
    hipLaunchKernelGGL(k_top_reduce, grid, block, 0, s, a);
    for (int step = 0; step < HM_TOP_PASSES; step++) hipLaunchKernelGGL(k_top_pass, grid, block, 0, s, a, step);
    hipLaunchKernelGGL(k_top_collect, grid, block, 0, s, a);
}

void hm_launch_top_sort(hipStream_t s, const uint64_t* keys, const uint64_t* counts, uint64_t m,
                        const unsigned long long* m_dev, uint64_t* keys_out, uint64_t* counts_out)
{
    if (m)
        hipLaunchKernelGGL(k_top_sort, dim3(1), dim3(HM_TOP_SORT_THREADS), 0, s, keys, counts, m, m_dev, keys_out,
                           counts_out);
}

void hm_launch_top_narrow(hipStream_t s, const uint64_t* keys, const uint64_t* counts, uint64_t m, uint32_t* ids_out,
                          uint64_t* counts_out)
{
    if (m)
        hipLaunchKernelGGL(k_top_narrow, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, keys, counts, m, ids_out,
                           counts_out);
}
