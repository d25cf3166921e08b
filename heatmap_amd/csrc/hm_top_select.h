/* The digit walk of the top-k selection (hm_top.hip; hm_cells_top,
 * hm_stream_top, hm_stream_top_groups in include/heatmap_amd.h).  Plain
 * integers, C or C++, no HIP: the kernels run it on the device and a CPU test
 * drives the same functions over numpy histograms.
 *
 * The selection looks for the record of rank `want` (1 = first) among the
 * records that agree with the bits decided so far, most significant digit
 * first.  A pass counts those records by their next digit; hm_top_pick then
 * names the digit the wanted record has, how many records rank before every
 * record of that digit (`beyond`: the larger digits of a descending walk, the
 * smaller ones of an ascending walk) and the rank left among the records of
 * the digit.  HmTopWalk strings the passes of one 64-bit walk together: which
 * bits are decided, which digit comes next, and when the value is complete. */
#ifndef HM_TOP_SELECT_H
#define HM_TOP_SELECT_H

#include <stdint.h>

#ifndef HM_TOP_FN
#define HM_TOP_FN static inline
#endif

#define HM_TOP_DIGIT_BITS 8
#define HM_TOP_BINS (1 << HM_TOP_DIGIT_BITS)

typedef struct HmTopPick {
    uint32_t digit;   /* the digit of the wanted record */
    uint64_t beyond;  /* records that rank before every record of that digit */
    uint64_t want;    /* rank of the wanted record among the records of the digit (>= 1) */
    uint64_t size;    /* records of the digit */
} HmTopPick;

/* hist[0 .. nbins): records per digit, 1 <= want <= their sum.  descending:
 * the larger digit ranks first.  A want beyond the sum answers the last
 * non-empty digit walked with want clamped to its size. */
HM_TOP_FN HmTopPick hm_top_pick(const uint64_t* hist, int nbins, uint64_t want, int descending)
{
    HmTopPick p;
    uint64_t before = 0;
    int last = descending ? nbins - 1 : 0;
    p.digit = (uint32_t)last;
    p.beyond = 0;
    p.want = 1;
    p.size = 0;
    for (int j = 0; j < nbins; j++) {
        const int d = descending ? nbins - 1 - j : j;
        const uint64_t h = hist[d];
        if (!h) continue;
        p.digit = (uint32_t)d;
        p.beyond = before;
        p.size = h;
        if (want - before <= h) {
            p.want = want - before;
            return p;
        }
        before += h;
    }
    p.want = p.size ? p.size : 1;
    return p;
}

/* one 64-bit walk: the bits at and above `shift + HM_TOP_DIGIT_BITS` of
 * `prefix` are decided; the next pass counts the digit at `shift` of the
 * records with (value & hm_top_mask(shift)) == prefix */
typedef struct HmTopWalk {
    uint64_t prefix;
    uint64_t want;    /* rank wanted among the records that match the prefix */
    uint64_t beyond;  /* records that rank before every record matching the prefix */
    uint64_t diff;    /* the bits in which the values differ at all (OR ^ AND) */
    uint64_t base;    /* the bits every value has (AND): a digit without a differing bit is read from here */
    int32_t shift;    /* < 0: the value is complete */
    uint32_t pad;
} HmTopWalk;

/* the decided bits of a pass at `shift` */
HM_TOP_FN uint64_t hm_top_mask(int shift)
{
    const int top = shift + HM_TOP_DIGIT_BITS;
    return top >= 64 ? 0ull : ~0ull << top;
}

/* from w->shift down: the digits in which no two values differ are decided
 * without a pass (every record has the bits of `base` there); stops at the
 * next digit that needs one, or below zero */
HM_TOP_FN void hm_top_walk_skip(HmTopWalk* w)
{
    while (w->shift >= 0 && ((w->diff >> w->shift) & (HM_TOP_BINS - 1)) == 0) {
        w->prefix |= w->base & ((uint64_t)(HM_TOP_BINS - 1) << w->shift);
        w->shift -= HM_TOP_DIGIT_BITS;
    }
}

/* A walk over values whose OR is `vor` and whose AND is `vand`: a digit all
 * values share (vor ^ vand has it zero) costs no pass, so counts below 2^16
 * walk two digits, values that differ only in one byte walk one, and values
 * that are all equal none (shift < 0 at once, prefix the value). */
HM_TOP_FN HmTopWalk hm_top_walk_begin(uint64_t vor, uint64_t vand, uint64_t want)
{
    HmTopWalk w;
    w.prefix = 0;
    w.want = want;
    w.beyond = 0;
    w.diff = vor ^ vand;
    w.base = vand;
    w.shift = 64 - HM_TOP_DIGIT_BITS;
    w.pad = 0;
    hm_top_walk_skip(&w);
    return w;
}

/* the digit of a pass is decided: on to the next one that needs a pass */
HM_TOP_FN void hm_top_walk_decided(HmTopWalk* w, uint32_t digit, uint64_t beyond, uint64_t want)
{
    w->prefix |= (uint64_t)digit << w->shift;
    w->beyond += beyond;
    w->want = want;
    w->shift -= HM_TOP_DIGIT_BITS;
    hm_top_walk_skip(w);
}

/* the pass at w->shift counted hist[HM_TOP_BINS]: decide its digit.  Returns
 * the records that share the whole prefix decided so far (when the walk is
 * complete: the records equal to the value). */
HM_TOP_FN uint64_t hm_top_walk_step(HmTopWalk* w, const uint64_t* hist, int descending)
{
    const HmTopPick p = hm_top_pick(hist, HM_TOP_BINS, w->want, descending);
    hm_top_walk_decided(w, p.digit, p.beyond, p.want);
    return p.size;
}

#endif
