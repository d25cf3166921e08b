/* The group ids of a selection (hm_stream_forget, hm_stream_export_select) as
 * its verdict kernel searches them.  Plain integers, C or C++, no HIP: the
 * host normalises the caller's ids with this, and a CPU test checks it against
 * sets.
 *
 * The caller's ids come in any order and may repeat; the kernel wants them
 * sorted and distinct, so that one bucket's group is found in about log2(n)
 * steps (hms_select_has, the search k_stream_select runs: the .hip file
 * compiles it for the device through HMS_SELECT_FN).  0xFFFFFFFE (the cells
 * without a group) is an id like any other; 0xFFFFFFFF (the merged rollups'
 * marker) names no group and is refused. */
#ifndef HM_STREAM_SELECT_H
#define HM_STREAM_SELECT_H

#include <stdint.h>
#include <stdlib.h>

#define HMS_SELECT_MAX_GROUPS (1 << 20)   /* HM_SELECT_MAX_GROUPS */
#define HMS_SELECT_NO_ID 0xFFFFFFFFu

#ifndef HMS_SELECT_FN
#define HMS_SELECT_FN static inline
#endif

static int hms_select_cmp(const void* a, const void* b)
{
    const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
    return (x > y) - (x < y);
}

/* The selection's ids, sorted and distinct, in out[0 .. result) (room for
 * ngroups).  0: every group (groups == NULL with ngroups == 0).  -1: refused
 * (NULL with a count, a count outside 1 .. HMS_SELECT_MAX_GROUPS, the id
 * 0xFFFFFFFF); out may then hold anything. */
static inline int64_t hms_select_ids(const uint32_t* groups, int64_t ngroups, uint32_t* out)
{
    if (!groups) return ngroups == 0 ? 0 : -1;
    if (ngroups < 1 || ngroups > HMS_SELECT_MAX_GROUPS) return -1;
    for (int64_t i = 0; i < ngroups; i++) {
        if (groups[i] == HMS_SELECT_NO_ID) return -1;
        out[i] = groups[i];
    }
    qsort(out, (size_t)ngroups, sizeof(uint32_t), hms_select_cmp);
    int64_t m = 1;
    for (int64_t i = 1; i < ngroups; i++)
        if (out[i] != out[m - 1]) out[m++] = out[i];
    return m;
}

/* g is one of the n sorted distinct ids (n >= 1) */
HMS_SELECT_FN int hms_select_has(const uint32_t* ids, uint32_t n, uint32_t g)
{
    uint32_t lo = 0, hi = n;   /* the first id >= g lies in [lo, hi] */
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < g) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && ids[lo] == g;
}

#endif
