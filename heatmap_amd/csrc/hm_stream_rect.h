/* A rectangle of one zoom as the stream's filter kernels test it (HmsViewRect,
 * HmsRasterRect in hm_pipeline.h).  Plain integers, C or C++, no HIP: the
 * host fills the kernels' structs from this, and a CPU test checks it against
 * an enumeration of the cells.
 *
 * A log key's cell bits are the pyramid id of (zoom z, row, col):
 *   (4^z - 1)/3 + (row << z) + col
 * so rows [row_lo, row_hi) of zoom z are the one id range [id_lo, id_lo +
 * span), and inside it a cell's column is (id - id_lo) & (2^z - 1). */
#ifndef HM_STREAM_RECT_H
#define HM_STREAM_RECT_H

#include <stdint.h>

typedef struct HmsRectIds {
    uint64_t id_lo;          /* id of (z, row_lo, 0) */
    uint64_t span;           /* (row_hi - row_lo) << z */
    uint32_t col_lo, col_w;  /* col_lo <= column < col_lo + col_w */
} HmsRectIds;

/* Rows [row_lo, row_hi) x columns [col_lo, col_hi) of zoom z, not empty and
 * already clipped to [0, 2^z)^2.  [*box_lo, *box_hi) grows to hold the
 * rectangle's id range (start it at ~0, 0). */
static inline HmsRectIds hms_rect_ids(int z, int64_t row_lo, int64_t row_hi, int64_t col_lo, int64_t col_hi,
                                      uint64_t* box_lo, uint64_t* box_hi)
{
    HmsRectIds r;
    r.id_lo = ((1ull << (2 * z)) - 1ull) / 3ull + ((uint64_t)row_lo << z);
    r.span = (uint64_t)(row_hi - row_lo) << z;
    r.col_lo = (uint32_t)col_lo;
    r.col_w = (uint32_t)(col_hi - col_lo);
    if (r.id_lo < *box_lo) *box_lo = r.id_lo;
    if (r.id_lo + r.span > *box_hi) *box_hi = r.id_lo + r.span;
    return r;
}

#endif
