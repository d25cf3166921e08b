/* The hours of a frames query (hm_stream_raster_frames) as its kernel tests
 * them.  Plain integers, C or C++, no HIP: the host fills the kernel's struct
 * from this, and a CPU test checks it against an enumeration of the hours.
 *
 * The caller's window [hour_lo, hour_hi) is cut into frames of frame_hours
 * anchored at hour_lo: hour h is in frame (h - hour_lo) / frame_hours.  The
 * log knows an hour as its offset x = h - base from the stream's base hour,
 * 0 <= x < 2^28, so the kernel gets the window clamped to those offsets,
 * [lo, hi), and for a cell of offset x in it computes
 *   frame = frame0 + (x - lo + phase) / fh
 * frame0 = the frame of the first clamped hour, phase = where that hour lies
 * inside its frame.  frame_hours may be any positive int64; fh and phase are
 * 32-bit: a frame longer than 2^28 hours has at most one edge inside the
 * offsets, which fh = 2^28 and a phase that puts the edge at the same offset
 * reproduce. */
#ifndef HM_STREAM_FRAMES_H
#define HM_STREAM_FRAMES_H

#include <stdint.h>

#define HMS_FRAMES_MAX_OFFSET (1ll << 28)   /* hour offsets are below this (HMS_MAX_HOUR_OFFSET) */

typedef struct HmsFramePlan {
    int64_t nframes;         /* ceil((hour_hi - hour_lo) / frame_hours) */
    int64_t frame0;          /* frame of the hour base + lo */
    uint32_t lo, hi;         /* clamped hour offsets; lo == hi: no hour of the stream is inside */
    uint32_t fh, phase;      /* 1 <= fh <= 2^28, phase < fh */
} HmsFramePlan;

/* 0 and *p filled, or -1: hour_hi <= hour_lo, frame_hours < 1 or more than
 * max_frames frames */
static inline int hms_frame_plan(int64_t base, int64_t hour_lo, int64_t hour_hi, int64_t frame_hours,
                                 int64_t max_frames, HmsFramePlan* p)
{
    if (hour_hi <= hour_lo || frame_hours < 1) return -1;
    /* differences of int64 hours in u64: exact, the true values are below 2^64 */
    const uint64_t span = (uint64_t)hour_hi - (uint64_t)hour_lo, fhl = (uint64_t)frame_hours;
    const uint64_t nf = (span - 1) / fhl + 1;
    if (nf > (uint64_t)max_frames) return -1;
    p->nframes = (int64_t)nf;
    const int64_t cap = HMS_FRAMES_MAX_OFFSET;
    const int64_t lo = hour_lo <= base ? 0 : (hour_lo - base < cap ? hour_lo - base : cap);
    const int64_t hi = hour_hi <= base ? 0 : (hour_hi - base < cap ? hour_hi - base : cap);
    p->lo = (uint32_t)lo;
    p->hi = (uint32_t)(hi > lo ? hi : lo);
    p->frame0 = 0;
    p->fh = 1;
    p->phase = 0;
    if (hi <= lo) return 0;              /* all of it outside the stream's hours */
    const uint64_t d0 = (uint64_t)(base + lo) - (uint64_t)hour_lo;   /* base + lo >= hour_lo */
    p->frame0 = (int64_t)(d0 / fhl);
    const uint64_t ph = d0 % fhl;
    if (fhl <= (uint64_t)cap) {
        p->fh = (uint32_t)fhl;
        p->phase = (uint32_t)ph;
    } else {                             /* the one edge, fhl - ph hours after lo, if it is in reach */
        p->fh = (uint32_t)cap;
        p->phase = fhl - ph < (uint64_t)cap ? (uint32_t)((uint64_t)cap - (fhl - ph)) : 0u;
    }
    return 0;
}

#endif
