/* Distinct visitors per cell (hm_stream_visitors): the arithmetic the two
 * kernels and the host share.  Plain integers, C or C++, no HIP: the .hip file
 * compiles it for the device through HM_VISIT_FN, and a CPU test builds it
 * with the host compiler.
 *
 * A cell is emitted when at least min_visitors distinct groups own a selected
 * record of it; the others are withheld, and the call reports how many cells
 * and how many points it withheld.  Nothing here is packed: points are 64
 * bits (a single cell may hold 2^40 of them and more), visitors 32 (there are
 * fewer than 2^32 group ids). */
#ifndef HM_VISIT_H
#define HM_VISIT_H

#include <stdint.h>

#ifndef HM_VISIT_FN
#define HM_VISIT_FN static inline
#endif

#define HM_VISIT_MIN_SLOTS 1024u

typedef struct {
    uint64_t cells, points;
} HmVisitWithheld;

/* is a cell of `visitors` distinct groups emitted at the threshold (>= 1) */
HM_VISIT_FN int hm_visit_keeps(uint32_t visitors, uint64_t min_visitors) { return (uint64_t)visitors >= min_visitors; }

/* one folded cell (visitors >= 1) judged: 1 when it is emitted, else it joins
 * the withheld cells and points */
HM_VISIT_FN int hm_visit_judge(HmVisitWithheld* w, uint32_t visitors, uint64_t points, uint64_t min_visitors)
{
    if (hm_visit_keeps(visitors, min_visitors)) return 1;
    w->cells += 1;
    w->points += points;
    return 0;
}

/* slots of the fold's table for nd (group, cell) records: a power of two, at
 * least twice the records (there are no more cells than records, so the table
 * is at most half full and a probe sequence stays short) */
HM_VISIT_FN uint64_t hm_visit_slots(uint64_t nd)
{
    uint64_t s = HM_VISIT_MIN_SLOTS;
    while (s < 2 * nd) s <<= 1;
    return s;
}

#endif
