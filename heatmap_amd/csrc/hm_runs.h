/* What the level >= 2 partitions (hm_kernels.hip) and the final aggregation
 * (hm_aggregate.hip) share: a work item's descriptor and the streaming of its
 * runs.  Include after hm_stamps.h: hm_stream_runs carries the stamp sites of
 * both (modes 1 and 5). */
#pragma once
#include "hm_device.h"
#include "hm_pipeline.h"

/* ------------------------------------------------------------------------ */
/* work items and run streaming                                              */
/* ------------------------------------------------------------------------ */

template <typename T>
__device__ __forceinline__ uint32_t hm_upper_bound(const T* a, uint32_t n, T v)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

template <typename T>
__device__ __forceinline__ uint32_t hm_lower_bound(const T* a, uint32_t n, T v)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

/* one 32-B descriptor load (written by k_items) per block */
__device__ __forceinline__ HmItem hm_item(const HmBuckets& B, uint32_t g)
{
    const uint4 d0 = B.desc[2 * g], d1 = B.desc[2 * g + 1];
    HmItem it;
    it.bucket = d0.x;
    it.j = d0.y;
    it.nitems = d0.z;
    it.r0 = d0.w;
    it.r1 = d1.x;
    it.a = d1.z;
    it.b = d1.w;
    return it;
}

/* Run chunk staged in LDS, dense per run i of the chunk: its 16-B-aligned
 * body (first vector, vectors; zero unless long) and two pieces (head and
 * tail of a long run, or the whole short run), each with an exclusive prefix. */
template <int RCH>
struct HmRunLds {
    uint32_t bv[RCH], bn[RCH], pre[RCH + 1];
    uint32_t ps[2 * RCH], pn[2 * RCH], ppre[2 * RCH + 1];
};

/* one wave: pre[0..n] = exclusive prefix of in[0..n), pre[n] = total */
__device__ __forceinline__ void hm_wave_prefix(const uint32_t* in, uint32_t n, uint32_t* pre)
{
    const uint32_t lane = hm_lane();
    const uint32_t per = (n + 63) / 64;
    const uint32_t i0 = min(n, lane * per), i1 = min(n, i0 + per);
    uint32_t sum = 0;
    for (uint32_t i = i0; i < i1; i++) sum += in[i];
    const uint32_t incl = hm_wave_incl_scan(sum);
    uint32_t acc = incl - sum;
    for (uint32_t i = i0; i < i1; i++) {
        const uint32_t x = in[i];
        pre[i] = acc;
        acc += x;
    }
    if (lane == 63) pre[n] = incl;
}

#ifndef HM_SU
#define HM_SU 4
#endif

/* Calls f.vec(uint4 x, valid, pos) / f.key(key, valid, pos) for every key at
 * the item's logical positions [a, b): the keys of vector x are staged order
 * positions pos..pos+V-1, single keys pos; together the positions are a
 * permutation of [0, b - a) (deterministic: no append atomics).  The item's
 * runs are staged RCH at a time and clipped to [a, b).  The 16-B-aligned
 * bodies of runs with >= HM_LONG_RUN keys form one flat vector space, split
 * into contiguous per-wave spans; a lane keeps HM_SU 16-B loads in flight and
 * finds each vector's run by walking a monotone cursor over the body prefix.
 * Short runs and the bodies' unaligned heads and tails ("pieces") go either
 * one lane each (8 loads in flight) or, COOP, 64 pieces per wave expanded
 * into consecutive keys per lane.  Block-uniform: every thread calls. */
template <typename InT, int THREADS, int RCH, bool COOP, typename F>
__device__ __forceinline__ void hm_stream_runs(const HmItem& it, const InT* __restrict__ keys, const HmRuns& in,
                                               HmRunLds<RCH>& L, uint32_t* scr, F& f)
{
    constexpr int NW = THREADS / 64;
    constexpr uint32_t V = 16 / sizeof(InT);   /* keys per 16-B vector */
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = tid >> 6;
    const uint4* kv = (const uint4*)keys;
    if (it.r1 - it.r0 <= HM_L1_SHARDS) {
        /* a few long runs (level-1 regions): each a contiguous key range,
         * streamed directly -- head keys, 16-B body vectors HM_SU per lane in
         * flight, tail keys; positions in that order, run after run */
        uint32_t pos0 = 0;
        for (uint32_t r = it.r0; r < it.r1; r++) {
        const uint2 run = in.run[r];
        const uint64_t s0 = in.excl[r];
        const uint64_t s2 = max(s0, (uint64_t)it.a), e2 = min(s0 + run.y, (uint64_t)it.b);
        const uint32_t cnt = e2 > s2 ? (uint32_t)(e2 - s2) : 0u;
        const uint32_t src = run.x + (uint32_t)(s2 - s0);
        const uint32_t head = min(cnt, (V - (src & (V - 1))) & (V - 1));
        const uint32_t nv = (cnt - head) / V;
        const uint32_t tail = cnt - head - nv * V;
        const uint32_t vb = (src + head) / V;
        for (uint32_t v0 = 0; v0 < nv; v0 += THREADS * HM_SU) {
            uint4 x[HM_SU];
            bool ok[HM_SU];
#pragma unroll
            for (int u = 0; u < HM_SU; u++) {
                const uint32_t v = v0 + u * THREADS + tid;
                ok[u] = v < nv;
                x[u] = ok[u] ? kv[vb + v] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < HM_SU; u++) f.vec(x[u], ok[u], pos0 + head + V * (v0 + u * THREADS + tid));
        }
        const uint32_t t = (uint32_t)tid;
        const uint32_t kh = t < head ? (uint32_t)keys[src + t] : 0u;
        const uint32_t kt = t < tail ? (uint32_t)keys[src + head + nv * V + t] : 0u;
        f.key(kh, t < head, pos0 + t);
        f.key(kt, t < tail, pos0 + head + nv * V + t);
        pos0 += cnt;
        }
        __syncthreads();
        return;
    }
    uint32_t carry = 0;                        /* keys staged by earlier chunks */
    for (uint32_t rc = it.r0; rc < it.r1; rc += RCH) {
        const uint32_t m = min((uint32_t)RCH, it.r1 - rc);
        for (uint32_t i = tid; i < m; i += THREADS) {
            const uint2 run = in.run[rc + i];
            const uint64_t s = in.excl[rc + i];
            const uint64_t e = s + run.y;
            const uint64_t s2 = max(s, (uint64_t)it.a), e2 = min(e, (uint64_t)it.b);
            const uint32_t cnt = e2 > s2 ? (uint32_t)(e2 - s2) : 0u;
            const uint32_t src = run.x + (uint32_t)(s2 - s);
            const uint32_t head = min(cnt, (V - (src & (V - 1))) & (V - 1));
            const uint32_t nv = (cnt - head) / V;
            const bool lg = cnt >= HM_LONG_RUN && nv > 0;
            L.bv[i] = (src + head) / V;
            L.bn[i] = lg ? nv : 0u;
            L.ps[2 * i] = src;
            L.pn[2 * i] = lg ? head : cnt;
            L.ps[2 * i + 1] = src + head + nv * V;
            L.pn[2 * i + 1] = lg ? cnt - head - nv * V : 0u;
        }
        __syncthreads();
        if (sizeof(InT) == 2 && rc == it.r0) HM_STAMP_M(5, 8);
        if (w == 0) hm_wave_prefix(L.bn, m, L.pre);
        if (w == 1 || NW == 1) hm_wave_prefix(L.pn, 2 * m, L.ppre);
        __syncthreads();
        if (sizeof(InT) == 2 && rc == it.r0) HM_STAMP_M(5, 9);
        const uint32_t nb = m, np = 2 * m;
        const uint32_t total = L.pre[nb];
        const uint32_t pbase = carry + V * total;
        /* bodies: contiguous wave spans of the flat vector space */
        const uint32_t span = ((total + NW - 1) / NW + 63) & ~63u;
        const uint32_t vb = min(total, span * w), ve = min(total, vb + span);
        if (vb < ve) {
            uint32_t r = hm_upper_bound(L.pre, nb + 1, vb) - 1;
            for (uint32_t v0 = vb; v0 < ve; v0 += 64 * HM_SU) {
                uint4 x[HM_SU];
                bool ok[HM_SU];
#pragma unroll
                for (int u = 0; u < HM_SU; u++) {
                    const uint32_t v = v0 + u * 64 + lane;
                    ok[u] = v < ve;
                    x[u] = make_uint4(0, 0, 0, 0);
                    if (ok[u]) {
                        while (L.pre[r + 1] <= v) r++;
                        x[u] = kv[L.bv[r] + (v - L.pre[r])];
                    }
                }
#pragma unroll
                for (int u = 0; u < HM_SU; u++) f.vec(x[u], ok[u], carry + V * (v0 + u * 64 + lane));
            }
        }
        if (sizeof(InT) == 4 && rc == it.r0) HM_STAMP(5);
        if (sizeof(InT) == 2 && rc == it.r0) HM_STAMP_M(5, 10);
        /* pieces: a wave takes 64 at a time, scans their lengths and hands
         * consecutive keys to consecutive lanes (piece found by a 6-step
         * shuffle search), 4 loads per lane in flight */
        if (COOP) {
        for (uint32_t q0 = (uint32_t)w * 64; q0 < np; q0 += NW * 64) {
            const uint32_t q = q0 + lane;
            const uint2 pc = q < np ? make_uint2(L.ps[q], L.pn[q]) : make_uint2(0, 0);
            const uint32_t pp = q < np ? pbase + L.ppre[q] : 0u;
            const uint32_t incl = hm_wave_incl_scan(pc.y);
            const uint32_t tot = __shfl(incl, 63, 64);
            for (uint32_t j0 = 0; j0 < tot; j0 += 256) {
                uint32_t kk[4], at[4];
                bool ok[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t j = j0 + u * 64 + lane;
                    uint32_t lo = 0;
#pragma unroll
                    for (int st = 32; st > 0; st >>= 1)
                        if (__shfl(incl, lo + st - 1, 64) <= j) lo += st;
                    lo = min(lo, 63u);
                    const uint32_t cnt = __shfl(pc.y, lo, 64);
                    const uint32_t off = j - (__shfl(incl, lo, 64) - cnt);
                    ok[u] = j < tot;
                    at[u] = __shfl(pp, lo, 64) + off;
                    /* every shuffle outside the ok-branch: a shuffle under a
                     * partial exec mask reads garbage from inactive lanes */
                    const uint32_t src = __shfl(pc.x, lo, 64) + off;
                    kk[u] = ok[u] ? (uint32_t)keys[src] : 0u;
                }
#pragma unroll
                for (int u = 0; u < 4; u++) f.key(kk[u], ok[u], at[u]);
            }
        }
        } else {
            for (uint32_t q = tid; q < np; q += THREADS) {
                const uint32_t cnt = L.pn[q], src = L.ps[q], pq = pbase + L.ppre[q];
                for (uint32_t k0 = 0; k0 < cnt; k0 += 8) {
                    uint32_t kk[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) kk[u] = (k0 + u < cnt) ? (uint32_t)keys[src + k0 + u] : 0u;
#pragma unroll
                    for (int u = 0; u < 8; u++) f.key(kk[u], k0 + u < cnt, pq + k0 + u);
                }
            }
        }
        if (sizeof(InT) == 4 && rc == it.r0) HM_STAMP(6);
        if (sizeof(InT) == 2 && rc == it.r0) HM_STAMP_M(5, 11);
        carry = pbase + L.ppre[np];
        __syncthreads();
    }
}
