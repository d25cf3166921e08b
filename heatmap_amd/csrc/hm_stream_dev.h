/* Device helpers the stream's kernel files share (hm_stream.hip,
 * hm_stream_region.hip): interning a bucket key, and a view's label key of a
 * raw bucket key. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hm_pipeline.h"
#include "hm_table.h"

/* bucket id of key k (interning it), or HMS_NO_BUCKET when the table is full */
__device__ __forceinline__ uint32_t hms_intern(const HmsBuckets& b, uint64_t k, uint32_t* claimed)
{
    uint64_t h = hms_hash(k) & b.mask;
    for (uint64_t probe = 0; probe <= b.mask; probe++) {
        /* a plain (L1-cacheable) read: a key word changes once, EMPTY -> key,
         * so a stale EMPTY only sends us to the CAS, which returns the truth */
        uint64_t cur = b.keys[h];
        if (cur == HMS_EMPTY) {
            const unsigned long long prev =
                atomicCAS((unsigned long long*)&b.keys[h], (unsigned long long)HMS_EMPTY, (unsigned long long)k);
            if (prev == HMS_EMPTY) {
                *claimed += 1;
                return (uint32_t)h;
            }
            cur = prev;
        }
        if (cur == k) return (uint32_t)h;
        h = (h + 1) & b.mask;
    }
    return HMS_NO_BUCKET;
}

/* label key of a raw bucket key in a view (the window's or alltime's label,
 * under the group, HMS_ALLGROUPS or the selected group), or ~0: not in it */
__device__ __forceinline__ uint64_t hms_view_key(const HmsViewArgs& a, uint64_t bk)
{
    const uint32_t pw = (uint32_t)bk, g = (uint32_t)(bk >> 32);
    const bool dated = (pw >> 28) == 0;
    const bool in = a.alltime ? (dated || pw == HMS_UNDATED) : (dated && pw >= a.lo && pw < a.hi);
    if (!in || (a.gmode == HMS_VIEW_GROUP && g != a.group)) return ~0ull;
    const uint32_t lp = (a.alltime ? HMS_TYPE_ALLTIME : HMS_TYPE_WINDOW) << 28;
    return ((uint64_t)(a.gmode == HMS_VIEW_MERGED ? HMS_ALLGROUPS : g) << 32) | lp;
}
