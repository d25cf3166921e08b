/* A region set as the stream's region queries test it (hm_stream_region_*,
 * hm_regions in include/heatmap_amd.h).  Plain integers, C or C++, no HIP: the
 * host validates a table with this before it is uploaded, the .hip file
 * compiles the lookup for the device through HMS_REGION_FN, and a CPU test
 * builds both with the host compiler.
 *
 * A region set is up to HM_REGION_MAX_REGIONS sets of cells of ONE zoom z,
 * given as row spans in CSR form: rows [row_lo, row_lo + nrows), row i's spans
 * at [row_ptr[i], row_ptr[i + 1]), span j the columns [col_lo[j], col_hi[j])
 * of region[j].  Within a row the spans are sorted by (col_lo, region); the
 * spans of one region in one row are disjoint; spans of different regions may
 * overlap, and a cell then belongs to each of them.  A row may have no span.
 *
 * A log key's cell bits are the pyramid id (4^z - 1)/3 + (row << z) + col
 * (hm_stream_rect.h), so the covered rows are one id interval, and inside it
 * a cell's row is (id - id_lo) >> z above row_lo and its column the low z
 * bits. */
#ifndef HM_REGION_H
#define HM_REGION_H

#include <stdint.h>

#ifndef HMS_REGION_FN
#define HMS_REGION_FN static inline
#endif

/* the limits of include/heatmap_amd.h (HM_REGION_MAX_*), for the builds that
 * see only this file */
#define HMS_REGION_MAX_REGIONS 4096
#define HMS_REGION_MAX_SPANS (1 << 20)
#define HMS_REGION_MAX_ROWS (1 << 20)

/* which rule a table breaks (hms_region_check) */
enum {
    HMS_RG_OK = 0,
    HMS_RG_ZOOM = 1,      /* zoom outside the stream's, or a null table (index 0) */
    HMS_RG_LIMITS = 2,    /* nregions, nspans or nrows outside the limits (index 0) */
    HMS_RG_ROWS = 3,      /* row_lo < 0 or row_lo + nrows > 2^zoom (index 0) */
    HMS_RG_ROW_PTR = 4,   /* row_ptr does not start at 0, falls, or does not end at nspans (index: the row;
                           * nrows for the end) */
    HMS_RG_COLS = 5,      /* not col_lo < col_hi <= 2^zoom (index: the span) */
    HMS_RG_REGION = 6,    /* region >= nregions (index: the span) */
    HMS_RG_ORDER = 7,     /* not sorted by (col_lo, region) inside its row (index: the later span) */
    HMS_RG_OVERLAP = 8    /* overlaps an earlier span of its region in its row (index: the later span) */
};

typedef struct HmsRegionIds {
    uint64_t id_lo;          /* id of (z, row_lo, 0) */
    uint64_t span;           /* nrows << z */
} HmsRegionIds;

/* the id interval of the rows [row_lo, row_lo + nrows) of zoom z, already
 * inside [0, 2^z) (hms_rect_ids' arithmetic) */
HMS_REGION_FN HmsRegionIds hms_region_ids(int z, int64_t row_lo, int64_t nrows)
{
    HmsRegionIds r;
    r.id_lo = ((1ull << (2 * z)) - 1ull) / 3ull + ((uint64_t)row_lo << z);
    r.span = (uint64_t)nrows << z;
    return r;
}

/* The next span index >= from of row row_rel (counted from row_lo) that
 * covers column col, or -1.  The first call passes from = 0, the next ones
 * the last answer + 1.  Stops at the first span with col_lo > col: the row is
 * sorted by col_lo.  row_rel < nrows is the caller's to guarantee. */
HMS_REGION_FN int64_t hms_region_next(const uint32_t* row_ptr, const uint32_t* col_lo, const uint32_t* col_hi,
                                      uint32_t row_rel, uint32_t col, int64_t from)
{
    const int64_t first = (int64_t)row_ptr[row_rel], end = (int64_t)row_ptr[row_rel + 1];
    for (int64_t j = from > first ? from : first; j < end && col_lo[j] <= col; j++)
        if (col < col_hi[j]) return j;
    return -1;
}

/* HMS_RG_OK, or the first rule the table breaks with *index the offending
 * span or row.  zmin, zmax: the stream's zooms.  scratch: 2 * nregions words
 * (any contents) for the same-region test, which is one pass: a row's spans
 * come by ascending col_lo, so a span overlaps an earlier one of its region
 * iff it starts below the largest col_hi that region has reached in this row
 * (scratch[2 r] = the row + 1 that scratch[2 r + 1] belongs to). */
HMS_REGION_FN int hms_region_check(int zoom, int64_t row_lo, int64_t nrows, int64_t nspans, int64_t nregions,
                                   const uint32_t* row_ptr, const uint32_t* col_lo, const uint32_t* col_hi,
                                   const uint32_t* region, int zmin, int zmax, uint32_t* scratch, int64_t* index)
{
    *index = 0;
    if (zoom < zmin || zoom > zmax || zoom < 0 || zoom > 31 || !row_ptr || !scratch ||
        (nspans > 0 && (!col_lo || !col_hi || !region)))
        return HMS_RG_ZOOM;
    if (nregions < 1 || nregions > HMS_REGION_MAX_REGIONS || nspans < 0 || nspans > HMS_REGION_MAX_SPANS || nrows < 0 ||
        nrows > HMS_REGION_MAX_ROWS)
        return HMS_RG_LIMITS;
    const int64_t side = 1ll << zoom;
    if (row_lo < 0 || row_lo > side || nrows > side - row_lo) return HMS_RG_ROWS;
    if (row_ptr[0] != 0) return HMS_RG_ROW_PTR;
    for (int64_t i = 0; i < nrows; i++)
        if (row_ptr[i + 1] < row_ptr[i] || (int64_t)row_ptr[i + 1] > nspans) {
            *index = i;
            return HMS_RG_ROW_PTR;
        }
    if ((int64_t)row_ptr[nrows] != nspans) {
        *index = nrows;
        return HMS_RG_ROW_PTR;
    }
    for (int64_t r = 0; r < 2 * nregions; r++) scratch[r] = 0;
    for (int64_t i = 0; i < nrows; i++)
        for (int64_t j = row_ptr[i]; j < (int64_t)row_ptr[i + 1]; j++) {
            *index = j;
            if (col_lo[j] >= col_hi[j] || (int64_t)col_hi[j] > side) return HMS_RG_COLS;
            if ((int64_t)region[j] >= nregions) return HMS_RG_REGION;
            if (j > (int64_t)row_ptr[i] &&
                (col_lo[j] < col_lo[j - 1] || (col_lo[j] == col_lo[j - 1] && region[j] < region[j - 1])))
                return HMS_RG_ORDER;
            uint32_t* m = scratch + 2 * region[j];
            if (m[0] == (uint32_t)(i + 1) && col_lo[j] < m[1]) return HMS_RG_OVERLAP;
            if (m[0] != (uint32_t)(i + 1) || col_hi[j] > m[1]) m[1] = col_hi[j];
            m[0] = (uint32_t)(i + 1);
        }
    *index = 0;
    return HMS_RG_OK;
}

#endif
