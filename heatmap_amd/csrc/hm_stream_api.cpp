/* The streaming heatmap of the C-ABI (hm_stream_* in include/heatmap_amd.h):
 * a multi-zoom heatmap resident in device memory, kernels in hm_stream.hip.
 *
 * The state is a log of (bucket | cell, count) pairs, one bucket per (group,
 * hour).  hm_stream_add counts a batch with hm_count (one bucket, the usual
 * case, speculatively and straight into the log's tail; a few buckets one run
 * each; many through one grouped pass) and appends its cells; equal keys are
 * summed when the log fills up or a caller asks (stream_compact).  Every query
 * is a filter pass over the log, then for cells a merge and an emit.
 * Context, arena and the count and merge drivers are hm_api.cpp (hm_ctx.h).
 */
#include <stdlib.h>

#include <algorithm>
#include <thread>
#include <unordered_set>
#include <utility>
#include <vector>

#include "hm_ctx.h"
#include "hm_region.h"
#include "hm_stream_frames.h"
#include "hm_stream_rect.h"
#include "hm_stream_select.h"
#include "hm_visit.h"

namespace {

/* one array of the log: a virtual-address reservation whose first `mapped`
 * bytes are backed, so a full log maps more pages behind its cells instead of
 * being copied into a buffer twice the size; reserved == 0: a plain hipMalloc */
struct LogArr {
    uint64_t* p = nullptr;
    size_t reserved = 0, mapped = 0;
    std::vector<std::pair<hipMemGenericAllocationHandle_t, size_t>> chunks;
};
struct LogPair {
    LogArr keys, counts;
};

/* a few-bucket batch gathered into one run per bucket, the points not kept
 * last: run j is [start[j], start[j + 1]) of plat / plon, bucket hb[j] */
struct Parts {
    uint32_t nparts;
    std::vector<uint32_t> hb;
    std::vector<uint64_t> start;   /* nparts + 2 starts (the last: n), then the run sizes read back */
    uint64_t size(uint32_t j) const { return start[j + 1] - start[j]; }
};

/* the hours of a query: every cell, the undated ones included (HW_ALLTIME),
 * the dated hours at the offsets [lo, hi) from the stream's base, none of
 * the stream's hours, or not a window */
enum { HW_INVALID, HW_EMPTY, HW_RANGE, HW_ALLTIME };
struct HourWindow {
    int kind;
    uint32_t lo, hi;
};

}  // namespace

#define HMS_PAR 4
struct hm_stream {
    hm_ctx* ctx = nullptr;
    int zmin = 0, zmax = 0;
    int cb = 0;                           /* cell bits of a log key */
    uint32_t base = 0;
    unsigned long long* state = nullptr;  /* device HMS_ST_* words */
    HmsBuckets bk{};                      /* (group, period) buckets */
    uint64_t* bk_alt = nullptr;           /* hm_stream_expire: the fresh table the survivors' buckets move to */
    uint32_t *bflag = nullptr, *blist = nullptr, *bloc = nullptr; /* per bucket: last batch, list, run */
    uint32_t epoch = 0;
    uint32_t last_nparts = 1;             /* buckets of the previous batch (1: count the next one speculatively) */
    /* the cell log: llen cells of lcap; alt: the compaction or expiry target
     * (allocated on first use, swapped with the log) */
    LogPair log, alt;
    uint64_t lcap = 0, llen = 0;
    bool compact = true;                  /* the log holds distinct keys */
    bool par = true;                      /* several-bucket batches counted concurrently (HM_STREAM_PAR=0: not) */
    /* while compact: the buckets with cells in the log.  A one-bucket batch
     * of a bucket not in it keeps the log compact (one count's cells are
     * distinct), so a stream of new hours never needs a compaction pass */
    std::unordered_set<uint32_t> log_buckets;
    uint64_t nbuckets = 0;
    unsigned long long* hstate = nullptr; /* pinned mirror of state */
    Buf bids, rec;                        /* per-batch scratch */
    Buf plat, plon, pkeep, pstart;        /* partition path: bucket-contiguous batch */
    int64_t rcap = 0;                     /* records rec holds */
    Buf rk, rc, mk, mc;                   /* rollup scratch: relabeled and merged cells */
    Buf tk, tc;                           /* a ranking's HM_TOP_MAX_K records (hm_stream_top*) */
    Buf vt, vv;                           /* hm_stream_visitors: the per-cell table and its visitors */
    /* hm_stream_region_*: the call's span table on the device, and the pinned
     * words it is packed into for the upload (gev: that upload is done, the
     * words may be overwritten) */
    Buf gt;
    uint32_t* ghost = nullptr;
    size_t ghost_words = 0;
    hipEvent_t gev = nullptr;
    /* several-bucket batches: up to HMS_PAR buckets counted at once, each by
     * its own context, stream and host thread, into its own scratch */
    hm_ctx* pctx[HMS_PAR] = {};
    Buf pk[HMS_PAR], pc[HMS_PAR];
    hipEvent_t pev = nullptr;
    bool vmm = true;                      /* HM_STREAM_VMM=0: plain allocations, grown by copying */
    /* maps the log's next extent ahead of need, on a host thread, while the
     * batches run (whatever changes a reservation or swaps the pairs joins it first) */
    std::thread premap;
};

static void premap_join(hm_stream* s)
{
    if (s->premap.joinable()) s->premap.join();
}

/* ---- the log's growable arrays ---- */
static hipMemAllocationProp log_prop(int device)
{
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    return prop;
}

/* map [mapped, bytes) of the reservation a (bytes: a granularity multiple) */
static bool arr_map(int device, LogArr& a, size_t bytes)
{
    if (bytes <= a.mapped) return true;
    if (bytes > a.reserved) return false;
    const hipMemAllocationProp prop = log_prop(device);
    const size_t add = bytes - a.mapped;
    hipMemGenericAllocationHandle_t h;
    char* at = (char*)a.p + a.mapped;
    hipMemAccessDesc d = {};
    d.location = prop.location;
    d.flags = hipMemAccessFlagsProtReadWrite;
    const bool created = hipMemCreate(&h, add, &prop, 0) == hipSuccess;
    const bool placed = created && hipMemMap(at, add, 0, h, 0) == hipSuccess;
    if (!placed || hipMemSetAccess(at, add, &d, 1) != hipSuccess) {
        (void)hipGetLastError();
        if (placed) (void)hipMemUnmap(at, add);
        if (created) (void)hipMemRelease(h);
        return false;
    }
    a.chunks.push_back({h, add});
    a.mapped = bytes;
    return true;
}

static size_t log_round(int device, size_t bytes)
{
    const hipMemAllocationProp prop = log_prop(device);
    size_t g = 0;
    if (hipMemGetAllocationGranularity(&g, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || !g) {
        (void)hipGetLastError();
        g = 2u << 20;
    }
    return (bytes + g - 1) / g * g;
}

static void arr_free(LogArr& a)
{
    if (a.p && !a.reserved) (void)hipFree(a.p);
    size_t off = 0;
    for (auto& c : a.chunks) {
        (void)hipMemUnmap((char*)a.p + off, c.second);
        (void)hipMemRelease(c.first);
        off += c.second;
    }
    if (a.reserved) (void)hipMemAddressFree(a.p, a.reserved);
    a = LogArr();
}

/* n cells: a reservation of 64x that (at most the device's memory) with the
 * first n mapped, or a plain allocation when reservations are off or fail */
static bool arr_alloc(hm_stream* s, LogArr& a, uint64_t n)
{
    const int dev = s->ctx->device;
    if (s->vmm) {
        size_t total = 0, freeb = 0;
        if (hipMemGetInfo(&freeb, &total) != hipSuccess) {
            (void)hipGetLastError();
            total = 0;
        }
        const size_t want = log_round(dev, (size_t)n * 8);
        a.reserved = log_round(dev, std::max<size_t>(want, std::min<size_t>((size_t)n * 8 * 64, total ? total : want)));
        if (hipMemAddressReserve((void**)&a.p, a.reserved, 0, nullptr, 0) == hipSuccess) {
            if (arr_map(dev, a, want)) return true;
            (void)hipMemAddressFree(a.p, a.reserved);
        }
        (void)hipGetLastError();
        a = LogArr();
    }
    if (hipMalloc((void**)&a.p, n * 8) != hipSuccess) {
        (void)hipGetLastError();
        a.p = nullptr;
        return false;
    }
    return true;
}

static void log_free(hm_stream* s, LogPair& l)
{
    premap_join(s);
    arr_free(l.keys);
    arr_free(l.counts);
}

/* both arrays at n cells, or neither */
static int log_alloc(hm_stream* s, LogPair& l, uint64_t n)
{
    premap_join(s);
    if (arr_alloc(s, l.keys, n) && arr_alloc(s, l.counts, n)) return HM_OK;
    arr_free(l.keys);
    return HM_E_NOMEM;
}

/* grow both arrays to n cells in place; false: not reservations, or too small */
static bool log_grow(hm_stream* s, LogPair& l, uint64_t n)
{
    premap_join(s);
    const int dev = s->ctx->device;
    for (LogArr* a : {&l.keys, &l.counts})
        if (!a->reserved || !arr_map(dev, *a, log_round(dev, (size_t)n * 8))) return false;
    return true;
}

static int stream_sync_state(hm_stream* s)
{
    HIPCHK(hipMemcpyAsync(s->hstate, s->state, HMS_ST_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          s->ctx->stream));
    HIPCHK(hm_sync(s->ctx->stream));
    s->nbuckets = s->hstate[HMS_ST_BUCKETS];
    return HM_OK;
}

static int stream_buf(Buf& b, size_t bytes)
{
    if (b.cap >= bytes) return HM_OK;
    if (b.p) HIPCHK(hipFree(b.p));
    b = Buf();
    if (hipMalloc(&b.p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return HM_E_NOMEM;
    }
    b.cap = bytes;
    return HM_OK;
}

/* sum the log's equal keys (the bucketed LDS merge) into the alternate
 * arrays, then swap them in */
static int stream_compact(hm_stream* s)
{
    if (s->compact || s->llen == 0) {
        s->compact = true;
        return HM_OK;
    }
    int st;
    premap_join(s);
    if (!s->alt.keys.p && (st = log_alloc(s, s->alt, s->lcap))) return st;
    int64_t m = 0;
    if ((st = cells_merge(s->ctx, s->log.keys.p, s->log.counts.p, HM_CELLS_U64, (int64_t)s->llen, nullptr, 0,
                          s->alt.keys.p, s->alt.counts.p, (int64_t)s->lcap, &m)))
        return st;
    std::swap(s->log, s->alt);
    s->llen = (uint64_t)m;
    s->compact = true;   /* (compaction adds no bucket: log_buckets stays exact) */
    return HM_OK;
}

/* the log will be over 3/4 full: map the next doubling's pages now, on a
 * host thread (hipMemCreate of a few hundred MB costs about a batch) */
static void premap_ahead(hm_stream* s, uint64_t need)
{
    if (!s->vmm || s->premap.joinable() || s->lcap - s->llen - need >= s->lcap / 4) return;
    const int dev = s->ctx->device;
    LogPair* l = &s->log;
    const size_t bytes = log_round(dev, (size_t)s->lcap * 16);
    if (bytes > l->keys.reserved || bytes > l->counts.reserved) return;
    if (l->keys.mapped >= bytes && l->counts.mapped >= bytes) return;
    s->premap = std::thread([l, bytes, dev]() {
        (void)hipSetDevice(dev);
        if (arr_map(dev, l->keys, bytes)) (void)arr_map(dev, l->counts, bytes);
    });
}

/* room for `need` more cells at the log's tail: compact first, then grow */
static int stream_room(hm_stream* s, uint64_t need)
{
    if (s->lcap - s->llen >= need) {
        premap_ahead(s, need);
        return HM_OK;
    }
    premap_join(s);
    int st;
    if ((st = stream_compact(s))) return st;
    if (s->lcap - s->llen >= need) return HM_OK;
    uint64_t cap = s->lcap ? s->lcap : 1024;
    while (cap - s->llen < need) cap <<= 1;
    /* reservations: more pages behind the cells, no copy and no sync (the
     * compaction target, when there is one, grows with them or is dropped) */
    if (log_grow(s, s->log, cap)) {
        if (s->alt.keys.p && !log_grow(s, s->alt, cap)) {
            HIPCHK(hm_sync(s->ctx->stream));
            log_free(s, s->alt);
        }
        s->lcap = cap;
        return HM_OK;
    }
    LogPair grown;
    if ((st = log_alloc(s, grown, cap))) return st;
    hipStream_t q = s->ctx->stream;
    if (s->llen) {
        HIPCHK(hipMemcpyAsync(grown.keys.p, s->log.keys.p, s->llen * 8, hipMemcpyDeviceToDevice, q));
        HIPCHK(hipMemcpyAsync(grown.counts.p, s->log.counts.p, s->llen * 8, hipMemcpyDeviceToDevice, q));
    }
    HIPCHK(hm_sync(q));
    log_free(s, s->log);
    log_free(s, s->alt);   /* the compaction target, at the new size when needed */
    s->log = std::move(grown);
    s->lcap = cap;
    return HM_OK;
}

#define HMS_ANY_BUCKET 0xFFFFFFFFu
/* m cells appended at the tail, of the nb buckets listed (HMS_ANY_BUCKET:
 * cells of several buckets not told apart; from then on the log's buckets are
 * not all known, and every append clears the compact flag) */
static void stream_appended(hm_stream* s, uint64_t m, const uint32_t* buckets, uint32_t nb)
{
    if (m) {
        /* each bucket's cells come from one count, so they are distinct: the
         * log stays compact when it was empty, or when none of the buckets
         * has cells in it yet (the log's buckets all known) */
        if (s->llen == 0) s->log_buckets.clear();
        /* (cells not told apart may be of any bucket, one with cells in the
         * log included: they are fresh only for an empty log) */
        bool fresh = !s->log_buckets.count(HMS_ANY_BUCKET);
        for (uint32_t j = 0; j < nb && fresh; j++)
            fresh = buckets[j] != HMS_ANY_BUCKET && !s->log_buckets.count(buckets[j]);
        s->compact = s->compact && (s->llen == 0 || fresh);
        for (uint32_t j = 0; j < nb; j++) s->log_buckets.insert(buckets[j]);
    }
    s->llen += m;
}

/* the room a count that needs m cells is given next */
static uint64_t grown_room(uint64_t m) { return m + m / 4 + 1024; }

/* One run of points counted by context c into the room (keys, counts, cap).
 * HM_E_EXOTIC: a kept point's tile lies outside [0, 2^z)^2, which the log's
 * keys cannot hold (with no record buffer hm_count reports those as capacity).
 * HM_E_CAPACITY: the run needs *m cells; the run of the points not kept (kept
 * = false: counted for its errors only) has none, so for it that is success. */
static int stream_count_run(hm_stream* s, hm_ctx* c, const double* lat, const double* lon, const uint8_t* keep,
                            int64_t n, bool kept, uint64_t* keys, uint64_t* counts, uint64_t cap, int64_t* m)
{
    int64_t nx = 0;
    const int st = hm_count(c, lat, lon, keep, n, s->zmin, s->zmax, keys, counts, (int64_t)cap, m, nullptr, 0, &nx);
    if (nx > 0) return HM_E_EXOTIC;
    return st == HM_E_CAPACITY && !kept ? HM_OK : st;
}

/* The batch's first failing point in input order, as hm_count reports it: the
 * whole batch counted once more with no room for cells (error paths only).
 * A point's error, a failure of that call itself, or HM_OK: every point projects. */
static int stream_first_failure(hm_stream* s, const double* lat, const double* lon, const uint8_t* keep, int64_t n)
{
    int64_t m = 0, nx = 0;
    const int st = hm_count(s->ctx, lat, lon, keep, n, s->zmin, s->zmax, nullptr, nullptr, 0, &m, nullptr, 0, &nx);
    return st == HM_E_CAPACITY ? HM_OK : st;
}

/* a batch of one bucket, part 1: hm_count's cells written at the log's tail
 * (not yet part of the log) */
static int stream_count_tail(hm_stream* s, const double* lat, const double* lon, const uint8_t* keep, int64_t n,
                             int64_t* m)
{
    int st;
    *m = 0;
    if ((st = stream_room(s, 2 * (uint64_t)n + 1024))) return st; /* typical batches: fewer cells than 2 per point */
    for (;;) {
        s->ctx->tail_keys = s->log.keys.p + s->llen;
        s->ctx->tail_state = s->state;
        s->ctx->tail_cb = s->cb;
        s->ctx->tail_done = 0;
        st = stream_count_run(s, s->ctx, lat, lon, keep, n, true, s->log.keys.p + s->llen, s->log.counts.p + s->llen,
                              s->lcap - s->llen, m);
        s->ctx->tail_keys = nullptr;
        if (st != HM_E_CAPACITY) return st;
        if ((st = stream_room(s, grown_room((uint64_t)*m)))) return st;
    }
}

/* part 2: the tail's m cells keyed under the bucket and appended */
static int stream_take_tail(hm_stream* s, int64_t m, uint32_t bucket)
{
    /* re-keyed inside the count already unless it took the fallback path */
    if (!s->ctx->tail_done)
        hm_launch_stream_rekey(s->ctx->stream, s->log.keys.p + s->llen, (uint64_t)m, (uint64_t)bucket << s->cb);
    HIPCHK(hipGetLastError());
    stream_appended(s, (uint64_t)m, &bucket, 1);
    return HM_OK;
}

/* a batch of several buckets: one grouped pass with the bucket as group */
static int stream_fold_grouped(hm_stream* s, const double* lat, const double* lon, const uint8_t* keep, int64_t n)
{
    int64_t m = 0;
    int st = HM_E_CAPACITY;
    for (int64_t want = 2 * n + 1024; st == HM_E_CAPACITY; want = (int64_t)grown_room((uint64_t)m)) {
        if (s->rcap < want) {
            if ((st = stream_buf(s->rec, (size_t)want * 40))) return st;
            s->rcap = want;
        }
        st = grouped_impl(s->ctx, lat, lon, nullptr, nullptr, keep, (const uint32_t*)s->bids.p, n, s->zmin, s->zmax,
                          (int64_t*)s->rec.p, s->rcap, &m);
    }
    if (st) return st;
    if ((st = stream_room(s, (uint64_t)m + 1))) return st;
    hipStream_t q = s->ctx->stream;
    HIPCHK(hipMemsetAsync(s->state + HMS_ST_EXOTIC, 0, 8, q));
    hm_launch_stream_convert(q, (const int64_t*)s->rec.p, (uint64_t)m, s->cb, s->log.keys.p + s->llen,
                             s->log.counts.p + s->llen, s->state);
    HIPCHK(hipGetLastError());
    if ((st = stream_sync_state(s))) return st;
    if (s->hstate[HMS_ST_EXOTIC]) return HM_E_EXOTIC;   /* checked before the cells join the log */
    const uint32_t any = HMS_ANY_BUCKET;
    stream_appended(s, (uint64_t)m, &any, 1);
    return HM_OK;
}

static int stream_gather_parts(hm_stream* s, const double* lat, const double* lon, const uint8_t* keep, int64_t n,
                               Parts& P)
{
    hipStream_t q = s->ctx->stream;
    const uint32_t nparts = P.nparts;
    int st;
    if ((st = stream_buf(s->pstart, (size_t)(nparts + 2) * 16))) return st;
    uint64_t* dstart = (uint64_t*)s->pstart.p;
    HmsScatterArgs a;
    a.lat = lat;
    a.lon = lon;
    a.keep = keep;
    a.bids = (const uint32_t*)s->bids.p;
    a.loc = s->bloc;
    a.n = (uint64_t)n;
    a.nparts = nparts;
    a.start = dstart;
    a.cursor = (unsigned long long*)(dstart + nparts + 2);
    hm_launch_stream_batch_list(q, s->blist, nparts, s->bloc);
    HIPCHK(hipMemsetAsync(a.cursor, 0, (size_t)(nparts + 2) * 8, q));
    hm_launch_stream_part_count(q, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(P.hb.data(), s->blist, nparts * 4, hipMemcpyDeviceToHost, q));
    HIPCHK(hipMemcpyAsync(P.start.data() + nparts + 2, a.cursor, (size_t)(nparts + 1) * 8, hipMemcpyDeviceToHost, q));
    HIPCHK(hm_sync(q));
    uint64_t kept = 0;
    for (uint32_t j = 0; j < nparts; j++) {
        P.start[j] = kept;
        kept += P.start[nparts + 2 + j];
    }
    P.start[nparts] = kept;
    P.start[nparts + 1] = (uint64_t)n;
    if (kept + P.start[2 * nparts + 2] != (uint64_t)n) return HM_E_HIP;   /* cannot happen */
    if ((st = stream_buf(s->plat, (size_t)n * 8)) || (st = stream_buf(s->plon, (size_t)n * 8))) return st;
    HIPCHK(hipMemcpyAsync(dstart, P.start.data(), (size_t)(nparts + 2) * 8, hipMemcpyHostToDevice, q));
    HIPCHK(hipMemsetAsync(a.cursor, 0, (size_t)(nparts + 2) * 8, q));
    a.lat_out = (double*)s->plat.p;
    a.lon_out = (double*)s->plon.p;
    hm_launch_stream_scatter(q, a);
    HIPCHK(hipGetLastError());
    const uint64_t nun = (uint64_t)n - kept;
    if (nun) {
        if ((st = stream_buf(s->pkeep, (size_t)nun))) return st;
        HIPCHK(hipMemsetAsync(s->pkeep.p, 0, nun, q));
    }
    return HM_OK;
}

/* The gathered runs (at most HMS_PAR in all) counted at once, each by its own
 * context, HIP stream and host thread into its own scratch, then copied to
 * the log's tail in bucket order and keyed -- nothing joins the log unless
 * every run counted.  HM_FALLBACK: a run failed (the caller's sequential path
 * re-counts and reports the batch's first failing point). */
static int stream_fold_parts_par(hm_stream* s, const Parts& P)
{
    hm_ctx* ctx = s->ctx;
    hipStream_t q = ctx->stream;
    const uint32_t nparts = P.nparts;
    const uint32_t nall = nparts + 1;    /* + the points not kept (errors only) */
    if (nall > HMS_PAR) return HM_FALLBACK;
    int st;
    for (int t = 0; t < HMS_PAR; t++) {
        if (s->pctx[t]) continue;
        hipStream_t pq = nullptr;
        HIPCHK(hipStreamCreateWithFlags(&pq, hipStreamNonBlocking));
        if ((st = hm_ctx_create(&s->pctx[t], ctx->device, pq))) {
            (void)hipStreamDestroy(pq);
            return st;
        }
    }
    for (int t = 0; t < HMS_PAR; t++) ctx_copy_tuning(s->pctx[t], ctx);   /* hm_ctx_tune of the stream's context */
    if (!s->pev) HIPCHK(hipEventCreateWithFlags(&s->pev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(s->pev, q));   /* the gathered runs are written */
    std::vector<int64_t> m(nall, 0);
    std::vector<int> rc(nall, HM_OK);
    std::vector<std::thread> th;
    for (uint32_t j = 0; j < nall; j++) {
        th.emplace_back([&, j]() {
            hm_ctx* c = s->pctx[j];
            (void)hipSetDevice(c->device);
            const uint64_t nj = P.size(j);
            if (!nj) return;
            if (hipStreamWaitEvent(c->stream, s->pev, 0) != hipSuccess) {
                rc[j] = HM_E_HIP;
                return;
            }
            const bool kept = j < nparts;
            rc[j] = HM_E_CAPACITY;
            for (uint64_t cap = kept ? 2 * nj + 1024 : 0; rc[j] == HM_E_CAPACITY; cap = grown_room((uint64_t)m[j])) {
                if (cap && (stream_buf(s->pk[j], cap * 8) != HM_OK || stream_buf(s->pc[j], cap * 8) != HM_OK)) {
                    rc[j] = HM_E_NOMEM;
                    return;
                }
                rc[j] = stream_count_run(s, c, (const double*)s->plat.p + P.start[j],
                                         (const double*)s->plon.p + P.start[j],
                                         kept ? nullptr : (const uint8_t*)s->pkeep.p, (int64_t)nj, kept,
                                         cap ? (uint64_t*)s->pk[j].p : nullptr, cap ? (uint64_t*)s->pc[j].p : nullptr,
                                         cap, &m[j]);
            }
        });
    }
    for (auto& x : th) x.join();
    for (uint32_t j = 0; j < nall; j++)
        if (rc[j] == HM_E_EXOTIC) return HM_E_EXOTIC;
    for (uint32_t j = 0; j < nall; j++)
        if (rc[j] != HM_OK) return HM_FALLBACK;
    /* the cells to the tail, in bucket order */
    uint64_t need = 0;
    for (uint32_t j = 0; j < nparts; j++) need += (uint64_t)m[j];
    if ((st = stream_room(s, need + 1024))) return st;
    for (uint32_t j = 0; j < nparts; j++) {
        if (!m[j]) continue;
        uint64_t* tk = s->log.keys.p + s->llen;
        HIPCHK(hipMemcpyAsync(tk, s->pk[j].p, (size_t)m[j] * 8, hipMemcpyDeviceToDevice, q));
        HIPCHK(hipMemcpyAsync(s->log.counts.p + s->llen, s->pc[j].p, (size_t)m[j] * 8, hipMemcpyDeviceToDevice, q));
        hm_launch_stream_rekey(q, tk, (uint64_t)m[j], (uint64_t)P.hb[j] << s->cb);
        HIPCHK(hipGetLastError());
        stream_appended(s, (uint64_t)m[j], &P.hb[j], 1);
    }
    return HM_OK;
}

/* a batch of a few buckets: gathered into one run per bucket (+ one run of
 * the points not kept), one hm_count per run written at the log's tail, all
 * counted before the tail joins the log.  Errors: the batch is re-counted as
 * a whole so the reported point is the first failing one in input order, as
 * hm_count's. */
static int stream_fold_parts(hm_stream* s, const double* lat, const double* lon, const uint8_t* keep, int64_t n,
                             uint32_t nparts)
{
    hipStream_t q = s->ctx->stream;
    int st;
    Parts P{nparts, std::vector<uint32_t>(nparts), std::vector<uint64_t>(2 * (nparts + 2), 0)};
    if ((st = stream_gather_parts(s, lat, lon, keep, n, P))) return st;
    if (nparts >= 2 && nparts + 1 <= HMS_PAR && s->par) {   /* one group of threads: the batch stays atomic */
        st = stream_fold_parts_par(s, P);
        if (st != HM_FALLBACK) return st;
    }
    if ((st = stream_room(s, 2 * P.start[nparts] + 1024))) return st;
    for (;;) {
        uint64_t off = 0;
        st = HM_OK;
        for (uint32_t j = 0; j <= nparts && st == HM_OK; j++) {
            const uint64_t nj = P.size(j);
            if (!nj) continue;
            const bool kept = j < nparts;
            int64_t m = 0;
            uint64_t* tk = s->log.keys.p + s->llen + off;
            st = stream_count_run(s, s->ctx, (const double*)s->plat.p + P.start[j],
                                  (const double*)s->plon.p + P.start[j], kept ? nullptr : (const uint8_t*)s->pkeep.p,
                                  (int64_t)nj, kept, tk, s->log.counts.p + s->llen + off, s->lcap - s->llen - off, &m);
            if (st == HM_E_CAPACITY) {   /* more room, and every run again */
                if ((st = stream_room(s, grown_room(off + (uint64_t)m)))) return st;
                st = HM_E_CAPACITY;
            } else if (st == HM_OK && kept) {
                hm_launch_stream_rekey(q, tk, (uint64_t)m, (uint64_t)P.hb[j] << s->cb);
                HIPCHK(hipGetLastError());
                off += (uint64_t)m;
            }
        }
        if (st == HM_E_CAPACITY) continue;
        if (st == HM_E_EXOTIC) return st;
        if (st != HM_OK) {
            const int first = stream_first_failure(s, lat, lon, keep, n);
            return first != HM_OK ? first : st;
        }
        /* several buckets' cells, each bucket's from one count */
        stream_appended(s, off, P.hb.data(), nparts);
        return HM_OK;
    }
}

extern "C" int hm_stream_create(hm_ctx* ctx, int zmin, int zmax, uint32_t base_hour, int64_t initial_cells,
                                int64_t max_buckets, hm_stream** out)
{
    if (!ctx || !out || zmin < 0 || zmax < zmin || zmax > HM_MAX_ZOOM || initial_cells < 0 || max_buckets < 0)
        return HM_E_ARG;
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    hm_stream* s = new hm_stream();
    s->ctx = ctx;
    s->zmin = zmin;
    s->zmax = zmax;
    s->base = base_hour;
    /* cell bits: the pyramid index of zooms 0..zmax, (4^(zmax+1) - 1)/3 values */
    const uint64_t ncell = ((1ull << (2 * (zmax + 1))) - 1) / 3;
    while ((1ull << s->cb) < ncell) s->cb++;
    const int bb = 64 - s->cb;   /* bucket bits: 21 at zmax 21 */
    uint64_t nb = 1024;
    const uint64_t want = max_buckets ? (uint64_t)max_buckets : (1ull << 20);
    while (nb < want + want / 4 && nb < (1ull << bb)) nb <<= 1;
    s->bk.mask = nb - 1;
    s->lcap = std::max<uint64_t>(1024, (uint64_t)initial_cells);
    if (const char* e = getenv("HM_STREAM_PAR")) s->par = atoi(e) != 0;
    if (const char* e = getenv("HM_STREAM_VMM")) s->vmm = atoi(e) != 0;
    int st = HM_OK;
    if (hipMalloc((void**)&s->state, HMS_ST_COUNT * sizeof(unsigned long long)) != hipSuccess ||
        hipHostMalloc((void**)&s->hstate, 2 * HMS_ST_COUNT * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void**)&s->bk.keys, nb * 8) != hipSuccess || hipMalloc((void**)&s->bflag, nb * 4) != hipSuccess ||
        hipMalloc((void**)&s->blist, nb * 4) != hipSuccess || hipMalloc((void**)&s->bloc, nb * 4) != hipSuccess ||
        log_alloc(s, s->log, s->lcap) != HM_OK) {
        (void)hipGetLastError();
        hm_stream_destroy(s);
        return HM_E_NOMEM;
    }
    st = hip_fail(hipMemsetAsync(s->state, 0, HMS_ST_COUNT * sizeof(unsigned long long), ctx->stream), "memset");
    if (st == HM_OK) {
        hm_launch_stream_fill(ctx->stream, s->bk.keys, nb, HMS_EMPTY);
        st = hip_fail(hipGetLastError(), "fill");
        if (st == HM_OK) st = hip_fail(hipMemsetAsync(s->bflag, 0, nb * 4, ctx->stream), "memset");
    }
    if (st == HM_OK) st = stream_sync_state(s);
    if (st) {
        hm_stream_destroy(s);
        return st;
    }
    *out = s;
    return HM_OK;
}

/* The start of a batch (hm_stream_add, hm_stream_import).  hm_last_error
 * becomes this call's: a batch of a few buckets is counted on helper contexts
 * and would leave an earlier call's error standing.  Then, for a batch that
 * is not empty: room for `room` cells at the log's tail, BFULL, EXOTIC, BMM,
 * NLIST, ERR reset in one copy, and the next epoch for the buckets' flags. */
static int stream_batch_begin(hm_stream* s, int64_t n, uint64_t room)
{
    hm_ctx* ctx = s->ctx;
    ctx->last_err_index = -1;
    ctx->last_err_kind = HM_OK;
    if (n == 0) return HM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    int st;
    if (room && (st = stream_room(s, room))) return st;
    unsigned long long* init = s->hstate + HMS_ST_COUNT;
    init[0] = init[1] = init[2] = init[3] = 0;   /* BFULL, EXOTIC, BMM, NLIST */
    init[4] = ~0ull;                             /* ERR */
    HIPCHK(hipMemcpyAsync(s->state + HMS_ST_BFULL, init, 5 * 8, hipMemcpyHostToDevice, ctx->stream));
    if (++s->epoch == 0) s->epoch = 1;   /* wrapped: stale flags only cost an exchange */
    return HM_OK;
}

extern "C" int hm_stream_add(hm_stream* s, const double* lat, const double* lon, const uint8_t* keep,
                             const uint32_t* hour, const uint32_t* group, int64_t n)
{
    if (!s || n < 0 || (n > 0 && (!lat || !lon)) || n >= (int64_t)0xFFFFFFF0ll) return HM_E_ARG;
    hm_ctx* ctx = s->ctx;
    int st;
    if ((st = stream_batch_begin(s, n, 0)) || n == 0) return st;
    hipStream_t q = ctx->stream;
    /* buckets of the kept points (interned; a failing batch may leave unused
     * buckets behind, never cells) */
    const bool per_point = group || hour;
    if (per_point && (st = stream_buf(s->bids, (size_t)n * 4))) return st;
    HmsBucketArgs a;
    a.group = group;
    a.hour = hour;
    a.keep = per_point ? keep : nullptr;
    a.n = per_point ? (uint64_t)n : 1;   /* neither: the one (no group, undated) bucket */
    a.base = s->base;
    a.buckets = s->bk;
    /* per-point bucket ids feed only the several-bucket paths: a batch
     * counted speculatively as one bucket skips writing them (and a batch
     * that turns out to hold several runs the pass again, below) */
    const bool spec = s->last_nparts <= 1;   /* the previous batch was one bucket */
    a.out = per_point && !spec ? (uint32_t*)s->bids.p : nullptr;
    a.bflag = s->bflag;
    a.epoch = s->epoch;
    a.list = s->blist;
    a.state = s->state;
    a.err_word = s->state + HMS_ST_ERR;
    hm_launch_stream_buckets(q, a);
    hm_launch_stream_collect(q, s->bflag, s->bk.mask + 1, s->epoch, s->blist, s->state);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->hstate, s->state, HMS_ST_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
    /* the usual batch is one bucket: count it right away (into the log's
     * tail); the bucket pass's state arrives with the count's first
     * read-back.  Any other outcome drops the tail and takes the paths below
     * (which count again, so errors and their order are the same). */
    int64_t m1 = 0;
    const int st1 = spec ? stream_count_tail(s, lat, lon, keep, n, &m1) : HM_OK;
    HIPCHK(hm_sync(q));
    s->nbuckets = s->hstate[HMS_ST_BUCKETS];
    const uint32_t nparts = (uint32_t)s->hstate[HMS_ST_NLIST];
    s->last_nparts = nparts;
    const unsigned long long e = s->hstate[HMS_ST_ERR];
    if (e != ~0ull) {
        /* a kept point with a bad hour (index << 8 | kind).  A point before it
         * that does not project is the batch's first failing point (input
         * order, as hm_count's); when every point projects, the hour is */
        const int64_t hi = (int64_t)(e >> 8);
        const int first = stream_first_failure(s, lat, lon, keep, n);
        const bool point = first == HM_E_NAN || first == HM_E_DOMAIN || first == HM_E_INF || first == HM_E_RANGE;
        if (point && ctx->last_err_index >= 0 && ctx->last_err_index < hi) return first;
        if (!point && first != HM_OK) return first;
        ctx->last_err_index = hi;
        ctx->last_err_kind = (int)(e & 0xFF);
        return ctx->last_err_kind;
    }
    if (s->hstate[HMS_ST_BFULL]) return HM_E_CAPACITY;   /* max_buckets (group, hour) pairs */
    if (nparts <= 1) { /* one bucket (the usual time-ordered batch), or nothing kept */
        if (!spec && (st = stream_count_tail(s, lat, lon, keep, n, &m1))) return st;
        if (spec && st1) return st1;
        return stream_take_tail(s, m1, nparts ? (uint32_t)s->hstate[HMS_ST_BMM] : 0u);
    }
    if (spec && per_point) {
        /* the ids the speculative pass skipped (the buckets are interned and
         * listed already: the same epoch, nothing new to flag) */
        a.out = (uint32_t*)s->bids.p;
        hm_launch_stream_buckets(q, a);
        HIPCHK(hipGetLastError());
    }
    if (nparts <= HMS_MAX_PARTS) return stream_fold_parts(s, lat, lon, keep, n, nparts);
    return stream_fold_grouped(s, lat, lon, keep, n);
}

extern "C" int hm_stream_cells(hm_stream* s, int64_t* cells, int64_t* capacity, int64_t* buckets)
{
    if (!s) return HM_E_ARG;
    HIPCHK(hipSetDevice(s->ctx->device));
    int st;
    if (cells) {
        /* distinct (bucket, cell) pairs: the log compacted */
        if ((st = stream_compact(s))) return st;
        *cells = (int64_t)s->llen;
    }
    if (capacity) *capacity = (int64_t)s->lcap;
    if (buckets) {
        if ((st = stream_sync_state(s))) return st;
        *buckets = (int64_t)s->nbuckets;
    }
    return HM_OK;
}

/* k_stream_emit's and k_stream_export's arguments: n cells (bucket | cell,
 * count) decoded into the caller's arrays */
static HmsEmitArgs stream_emit_args(const hm_stream* s, const uint64_t* keys, const uint64_t* counts, uint64_t n,
                                    uint64_t* keys_out, uint64_t* counts_out, uint32_t* groups_out,
                                    uint32_t* periods_out)
{
    return HmsEmitArgs{keys, counts, n, s->bk, s->cb, s->zmin, s->zmax, s->base, keys_out, counts_out, groups_out,
                       periods_out};
}

/* The start of a filter pass over the log into the scratch arrays (relabel,
 * view).  *empty: the log holds nothing, no pass to run.  Else the scratch is
 * sized to the log, the cursor and BFULL are reset, and the arguments every
 * such kernel shares are filled in. */
template <class Args>
static int stream_filter_begin(hm_stream* s, Args& a, bool* empty)
{
    hipStream_t q = s->ctx->stream;
    int st;
    *empty = s->llen == 0;
    if (*empty) return HM_OK;
    if ((st = stream_buf(s->rk, s->llen * 8)) || (st = stream_buf(s->rc, s->llen * 8))) return st;
    a.cursor = s->state + HMS_ST_CURSOR;
    HIPCHK(hipMemsetAsync(a.cursor, 0, 8, q));
    HIPCHK(hipMemsetAsync(s->state + HMS_ST_BFULL, 0, 8, q));
    a.keys = s->log.keys.p;
    a.counts = s->log.counts.p;
    a.n = s->llen;
    a.buckets = s->bk;
    a.cb = s->cb;
    a.keys_out = (uint64_t*)s->rk.p;
    a.counts_out = (uint64_t*)s->rc.p;
    a.state = s->state;
    return HM_OK;
}

/* the filter pass's read-back, then the cells it left in the scratch arrays
 * (HMS_ST_CURSOR of them) with equal keys summed: *nd distinct cells in mk / mc */
static int stream_merge(hm_stream* s, int64_t* nd)
{
    int st;
    *nd = 0;
    if ((st = stream_sync_state(s))) return st;
    if (s->hstate[HMS_ST_BFULL]) return HM_E_CAPACITY;   /* no bucket left for a rollup label */
    const uint64_t m = s->hstate[HMS_ST_CURSOR];
    if (m == 0) return HM_OK;
    if ((st = stream_buf(s->mk, m * 8)) || (st = stream_buf(s->mc, m * 8))) return st;
    return cells_merge(s->ctx, (const uint64_t*)s->rk.p, (const uint64_t*)s->rc.p, HM_CELLS_U64, (int64_t)m, nullptr, 0,
                       (uint64_t*)s->mk.p, (uint64_t*)s->mc.p, (int64_t)m, nd);
}

/* the tail of every such query: the label cells merged and emitted */
static int stream_merge_emit(hm_stream* s, uint64_t* keys_out, uint64_t* counts_out, uint32_t* groups_out,
                             uint32_t* periods_out, int64_t capacity, int64_t* n_out)
{
    hm_ctx* ctx = s->ctx;
    int st;
    int64_t nd = 0;
    if ((st = stream_merge(s, &nd)) || nd == 0) return st;
    *n_out = nd;
    if (nd > capacity) return HM_E_CAPACITY;
    hm_launch_stream_emit(ctx->stream, stream_emit_args(s, (const uint64_t*)s->mk.p, (const uint64_t*)s->mc.p,
                                                        (uint64_t)nd, keys_out, counts_out, groups_out, periods_out));
    HIPCHK(hipGetLastError());
    return HM_OK;
}

/* a rollup's three passes: relabel, merge, emit (span: HM_SPAN_*, or
 * HMS_SPAN_WINDOW with the hour offsets [lo, hi)) */
static int stream_rollup(hm_stream* s, int span, int merge_groups, int64_t select, uint32_t lo, uint32_t hi,
                         uint64_t* keys_out, uint64_t* counts_out, uint32_t* groups_out, uint32_t* periods_out,
                         int64_t capacity, int64_t* n_out)
{
    *n_out = 0;
    HIPCHK(hipSetDevice(s->ctx->device));
    /* the log's cells of the rollup, re-keyed to label buckets */
    HmsRelabelArgs a;
    bool empty;
    const int st = stream_filter_begin(s, a, &empty);
    if (st || empty) return st;
    a.span = span;
    a.merge = merge_groups ? 1 : 0;
    a.base = s->base;
    a.select = select;
    a.lo = lo;
    a.hi = hi;
    hm_launch_stream_relabel(s->ctx->stream, a);
    HIPCHK(hipGetLastError());
    return stream_merge_emit(s, keys_out, counts_out, groups_out, periods_out, capacity, n_out);
}

extern "C" int hm_stream_rollup(hm_stream* s, int span, int merge_groups, int64_t select, uint64_t* keys_out,
                                uint64_t* counts_out, uint32_t* groups_out, uint32_t* periods_out, int64_t capacity,
                                int64_t* n_out)
{
    if (!s || !n_out || span < HM_SPAN_HOUR || span > HM_SPAN_ALLTIME || select < -1 || capacity < 0 ||
        (capacity > 0 && (!keys_out || !counts_out)))
        return HM_E_ARG;
    return stream_rollup(s, span, merge_groups, select, 0, 0, keys_out, counts_out, groups_out, periods_out, capacity,
                         n_out);
}

/* hour -> offset from the stream's base, clamped to [0, 2^28] */
static uint32_t stream_hour_offset(const hm_stream* s, int64_t hour)
{
    const int64_t off = hour - (int64_t)s->base;
    return (uint32_t)std::min<int64_t>(std::max<int64_t>(off, 0), (int64_t)HMS_MAX_HOUR_OFFSET);
}

/* [hour_lo, hour_hi) as a query's hours (both HM_STREAM_ALLTIME: all time) */
static HourWindow stream_hours(const hm_stream* s, int64_t hour_lo, int64_t hour_hi)
{
    if (hour_lo == HM_STREAM_ALLTIME && hour_hi == HM_STREAM_ALLTIME) return {HW_ALLTIME, 0, 0};
    if (!s || hour_hi <= hour_lo) return {HW_INVALID, 0, 0};
    const uint32_t lo = stream_hour_offset(s, hour_lo), hi = stream_hour_offset(s, hour_hi);
    return {lo < hi ? HW_RANGE : HW_EMPTY, lo, hi};
}

extern "C" int hm_stream_window(hm_stream* s, int64_t hour_lo, int64_t hour_hi, int merge_groups, uint64_t* keys_out,
                                uint64_t* counts_out, uint32_t* groups_out, int64_t capacity, int64_t* n_out)
{
    const HourWindow w = stream_hours(s, hour_lo, hour_hi);
    if (!s || !n_out || w.kind == HW_INVALID || w.kind == HW_ALLTIME || capacity < 0 ||
        (capacity > 0 && (!keys_out || !counts_out)))
        return HM_E_ARG;
    *n_out = 0;
    if (w.kind == HW_EMPTY) return HM_OK;   /* all of it outside the stream's hours */
    return stream_rollup(s, HMS_SPAN_WINDOW, merge_groups, -1, w.lo, w.hi, keys_out, counts_out, groups_out, nullptr,
                         capacity, n_out);
}

/* A view's filter pass (hm_stream_view, hm_stream_top, hm_stream_top_groups):
 * the rectangles, hours and group checked and the log's cells of the selection
 * written to the scratch arrays, re-keyed to the view's label -- or, by_group,
 * keyed by their group id alone.  *empty: nothing can be selected, no pass ran.
 * one_zoom: rectangles of different zooms are refused.  n_out: hm_stream_view's,
 * zeroed once the arguments checked before the rectangles have passed. */
static int stream_view_filter(hm_stream* s, int64_t hour_lo, int64_t hour_hi, int64_t group, const int64_t* rects,
                              int nrects, bool by_group, bool one_zoom, bool* empty, int64_t* n_out = nullptr)
{
    const HourWindow w = stream_hours(s, hour_lo, hour_hi);
    *empty = true;
    if (!s || !rects || nrects < 1 || nrects > HM_VIEW_MAX_RECTS || w.kind == HW_INVALID || group < HM_VIEW_EACH ||
        group > (int64_t)HMS_NOGROUP)
        return HM_E_ARG;
    if (n_out) *n_out = 0;   /* hm_stream_view: zero from here on, also when a rectangle is refused below */
    HmsViewArgs a;
    a.nrects = 0;
    uint64_t box_hi = 0;
    a.box_lo = ~0ull;
    for (int r = 0; r < nrects; r++) {
        const int64_t z = rects[5 * r], side = 1ll << (z < 0 || z > HM_MAX_ZOOM ? 0 : z);
        int64_t rlo = rects[5 * r + 1], rhi = rects[5 * r + 2], clo = rects[5 * r + 3], chi = rects[5 * r + 4];
        if (z < s->zmin || z > s->zmax || rhi <= rlo || chi <= clo || (one_zoom && z != rects[0])) return HM_E_ARG;
        /* clipped to the square; what is left may be nothing */
        rlo = std::max<int64_t>(rlo, 0), clo = std::max<int64_t>(clo, 0);
        rhi = std::min<int64_t>(rhi, side), chi = std::min<int64_t>(chi, side);
        if (rhi <= rlo || chi <= clo) continue;
        const HmsRectIds ids = hms_rect_ids((int)z, rlo, rhi, clo, chi, &a.box_lo, &box_hi);
        a.rects[a.nrects++] = HmsViewRect{ids.id_lo, ids.span, (uint32_t)(side - 1), ids.col_lo, ids.col_w, 0};
    }
    if (a.nrects == 0) return HM_OK;        /* every rectangle outside the square */
    if (w.kind == HW_EMPTY) return HM_OK;   /* all of it outside the stream's hours */
    a.box_span = box_hi - a.box_lo;
    a.alltime = w.kind == HW_ALLTIME;
    a.lo = w.lo, a.hi = w.hi;
    a.gmode = group == HM_VIEW_MERGED ? HMS_VIEW_MERGED : (group == HM_VIEW_EACH ? HMS_VIEW_EACH : HMS_VIEW_GROUP);
    a.group = group >= 0 ? (uint32_t)group : 0u;
    HIPCHK(hipSetDevice(s->ctx->device));
    const int st = stream_filter_begin(s, a, empty);
    if (st || *empty) return st;
    if (by_group)
        hm_launch_stream_view_groups(s->ctx->stream, a);
    else
        hm_launch_stream_view(s->ctx->stream, a);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_stream_view(hm_stream* s, int64_t hour_lo, int64_t hour_hi, int64_t group, const int64_t* rects,
                              int nrects, uint64_t* keys_out, uint64_t* counts_out, uint32_t* groups_out,
                              int64_t capacity, int64_t* n_out)
{
    if (!n_out || capacity < 0 || (capacity > 0 && (!keys_out || !counts_out))) return HM_E_ARG;
    /* a view's three passes: filter (k_stream_view, in place of the relabel),
     * then the rollup's merge and emit over the survivors only */
    bool empty;
    const int st = stream_view_filter(s, hour_lo, hour_hi, group, rects, nrects, false, false, &empty, n_out);
    if (st || empty) return st;
    return stream_merge_emit(s, keys_out, counts_out, groups_out, nullptr, capacity, n_out);
}

/* the selection over a query's merged cells (mk / mc, nd of them) into the
 * stream's ranked scratch: min(nd, k) records in rank order in tk / tc */
static int stream_rank(hm_stream* s, int64_t nd, int64_t k)
{
    int st;
    if ((st = stream_buf(s->tk, HM_TOP_MAX_K * 8)) || (st = stream_buf(s->tc, HM_TOP_MAX_K * 8))) return st;
    return cells_top(s->ctx, (const uint64_t*)s->mk.p, (const uint64_t*)s->mc.p, nd, k, (uint64_t*)s->tk.p,
                     (uint64_t*)s->tc.p);
}

extern "C" int hm_stream_top(hm_stream* s, int64_t hour_lo, int64_t hour_hi, int64_t group, const int64_t* rects,
                             int nrects, int64_t k, uint64_t* keys_out, uint64_t* counts_out, int64_t* n_out,
                             int64_t* cells_out)
{
    if (!n_out || !keys_out || !counts_out || k < 1 || k > HM_TOP_MAX_K || group == HM_VIEW_EACH) return HM_E_ARG;
    /* the view's filter and merge, then the selection, then the view's emit
     * of the chosen records only */
    bool empty;
    int st = stream_view_filter(s, hour_lo, hour_hi, group, rects, nrects, false, false, &empty);
    if (st == HM_E_ARG) return st;
    *n_out = 0;
    if (cells_out) *cells_out = 0;
    if (st || empty) return st;
    int64_t nd = 0;
    if ((st = stream_merge(s, &nd)) || nd == 0) return st;
    /* One label is in play (merged, or one group), so every merged key has
     * the same bucket bits, and the cell bits -- the pyramid id, ordered by
     * zoom, then row, then column -- order as HM_KEY does: ranking the
     * internal keys is ranking the emitted ones. */
    if ((st = stream_rank(s, nd, k))) return st;
    const int64_t m = std::min(nd, k);
    hm_launch_stream_emit(s->ctx->stream, stream_emit_args(s, (const uint64_t*)s->tk.p, (const uint64_t*)s->tc.p,
                                                           (uint64_t)m, keys_out, counts_out, nullptr, nullptr));
    HIPCHK(hipGetLastError());
    *n_out = m;
    if (cells_out) *cells_out = nd;
    return HM_OK;
}

extern "C" int hm_stream_top_groups(hm_stream* s, int64_t hour_lo, int64_t hour_hi, const int64_t* rects, int nrects,
                                    int64_t k, uint32_t* groups_out, uint64_t* counts_out, int64_t* n_out,
                                    int64_t* groups_total_out)
{
    if (!n_out || !groups_out || !counts_out || k < 1 || k > HM_TOP_MAX_K) return HM_E_ARG;
    /* the survivors keyed by group alone (k_stream_view_groups), then the same
     * merge and selection; the keys are the group ids themselves */
    bool empty;
    int st = stream_view_filter(s, hour_lo, hour_hi, HM_VIEW_MERGED, rects, nrects, true, true, &empty);
    if (st == HM_E_ARG) return st;
    *n_out = 0;
    if (groups_total_out) *groups_total_out = 0;
    if (st || empty) return st;
    int64_t nd = 0;
    if ((st = stream_merge(s, &nd)) || nd == 0) return st;
    if ((st = stream_rank(s, nd, k))) return st;
    const int64_t m = std::min(nd, k);
    hm_launch_top_narrow(s->ctx->stream, (const uint64_t*)s->tk.p, (const uint64_t*)s->tc.p, (uint64_t)m, groups_out,
                         counts_out);
    HIPCHK(hipGetLastError());
    *n_out = m;
    if (groups_total_out) *groups_total_out = nd;
    return HM_OK;
}

extern "C" int hm_stream_visitors(hm_stream* s, int64_t hour_lo, int64_t hour_hi, const int64_t* rects, int nrects,
                                  int64_t min_visitors, uint64_t* keys_out, uint64_t* points_out,
                                  uint32_t* visitors_out, int64_t capacity, int64_t* n_out, int64_t* withheld_out)
{
    if (!n_out || min_visitors < 1 || capacity < 0 || (capacity > 0 && (!keys_out || !points_out))) return HM_E_ARG;
    /* a per-group view's filter and merge (one label per group, interned once
     * and reused), then the fold of its (group, cell) records per cell and the
     * sweep with the threshold */
    bool empty;
    int st = stream_view_filter(s, hour_lo, hour_hi, HM_VIEW_EACH, rects, nrects, false, false, &empty);
    if (st == HM_E_ARG) return st;
    *n_out = 0;
    if (withheld_out) withheld_out[0] = withheld_out[1] = 0;
    if (st || empty) return st;
    int64_t nd = 0;
    if ((st = stream_merge(s, &nd)) || nd == 0) return st;
    hipStream_t q = s->ctx->stream;
    HmsVisitArgs a;
    a.keys = (const uint64_t*)s->mk.p;
    a.counts = (const uint64_t*)s->mc.p;
    a.n = (uint64_t)nd;
    a.cb = s->cb;
    a.zmin = s->zmin;
    a.zmax = s->zmax;
    const uint64_t slots = hm_visit_slots((uint64_t)nd);
    if ((st = stream_buf(s->vt, slots * 16)) || (st = stream_buf(s->vv, slots * 4))) return st;
    a.table = HmsTable{(uint64_t*)s->vt.p, slots - 1, s->state};
    a.visitors = (uint32_t*)s->vv.p;
    a.min_visitors = (uint64_t)min_visitors;
    a.keys_out = keys_out;
    a.points_out = points_out;
    a.visitors_out = visitors_out;
    a.capacity = (uint64_t)capacity;
    a.cursor = s->state + HMS_ST_CURSOR;
    HIPCHK(hipMemsetAsync(s->state + HMS_ST_OVERFLOW, 0, 2 * 8, q));   /* OVERFLOW, CURSOR */
    HIPCHK(hipMemsetAsync(s->state + HMS_ST_WCELLS, 0, 2 * 8, q));     /* WCELLS, WPOINTS */
    HIPCHK(hipMemsetAsync(a.visitors, 0, slots * 4, q));
    hm_launch_stream_init(q, a.table);
    hm_launch_stream_visit_fold(q, a);
    hm_launch_stream_visit_emit(q, a);
    HIPCHK(hipGetLastError());
    /* the emitted count and the withheld totals, one read-back */
    if ((st = stream_sync_state(s))) return st;
    if (s->hstate[HMS_ST_OVERFLOW]) return HM_E_HIP;   /* cannot happen */
    *n_out = (int64_t)s->hstate[HMS_ST_CURSOR];
    if (withheld_out) {
        withheld_out[0] = (int64_t)s->hstate[HMS_ST_WCELLS];
        withheld_out[1] = (int64_t)s->hstate[HMS_ST_WPOINTS];
    }
    return *n_out > capacity ? HM_E_CAPACITY : HM_OK;
}

/* ---- region queries: the view's selection with a span table in place of
 * the rectangles (hm_region.h; kernels in hm_stream_region.hip) ---- */

/* A region query's table: checked on the host (hms_region_check), so that the
 * kernel never indexes outside it, then packed into the stream's pinned words
 * and uploaded into the stream's scratch; a's table fields filled in.  A
 * refused table is HM_E_ARG with the offending span or row as hm_last_error's
 * index.  A table without spans is not uploaded: it selects nothing. */
static int stream_region_table(hm_stream* s, const hm_regions* rg, HmsRegionArgs& a)
{
    hm_ctx* ctx = s->ctx;
    const int64_t nr = std::min<int64_t>(std::max<int64_t>(rg->nregions, 1), HM_REGION_MAX_REGIONS);
    std::vector<uint32_t> scratch(2 * (size_t)nr);
    int64_t bad = 0;
    if (hms_region_check(rg->zoom, rg->row_lo, rg->nrows, rg->nspans, rg->nregions, rg->row_ptr, rg->col_lo,
                         rg->col_hi, rg->region, s->zmin, s->zmax, scratch.data(), &bad) != HMS_RG_OK) {
        ctx->last_err_index = bad;
        ctx->last_err_kind = HM_E_ARG;
        return HM_E_ARG;
    }
    const HmsRegionIds ids = hms_region_ids(rg->zoom, rg->row_lo, rg->nrows);
    a.z = rg->zoom;
    a.id_lo = ids.id_lo;
    a.id_span = ids.span;
    a.nrows = (uint32_t)rg->nrows;
    a.nspans = (uint32_t)rg->nspans;
    a.nregions = (uint32_t)rg->nregions;
    a.row_ptr = a.col_lo = a.col_hi = a.region = nullptr;
    a.stage = 0;
    a.totals = nullptr;
    a.ntot = 0;
    a.fh = 1, a.phase = 0;
    a.capacity = 0;
    a.v.nrects = 0;
    a.v.box_lo = a.v.box_span = 0;
    if (rg->nspans == 0) return HM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nrp = (size_t)rg->nrows + 1, ns = (size_t)rg->nspans, words = nrp + 3 * ns;
    if (!s->gev) HIPCHK(hipEventCreateWithFlags(&s->gev, hipEventDisableTiming));
    HIPCHK(hipEventSynchronize(s->gev));   /* the last call's upload has left the pinned words */
    if (s->ghost_words < words) {
        if (s->ghost) HIPCHK(hipHostFree(s->ghost));
        s->ghost = nullptr;
        s->ghost_words = 0;
        if (hipHostMalloc((void**)&s->ghost, words * 4) != hipSuccess) {
            (void)hipGetLastError();
            return HM_E_NOMEM;
        }
        s->ghost_words = words;
    }
    std::copy(rg->row_ptr, rg->row_ptr + nrp, s->ghost);
    std::copy(rg->col_lo, rg->col_lo + ns, s->ghost + nrp);
    std::copy(rg->col_hi, rg->col_hi + ns, s->ghost + nrp + ns);
    std::copy(rg->region, rg->region + ns, s->ghost + nrp + 2 * ns);
    int st;
    if ((st = stream_buf(s->gt, words * 4))) return st;
    HIPCHK(hipMemcpyAsync(s->gt.p, s->ghost, words * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipEventRecord(s->gev, ctx->stream));
    a.row_ptr = (const uint32_t*)s->gt.p;
    a.col_lo = a.row_ptr + nrp;
    a.col_hi = a.col_lo + ns;
    a.region = a.col_hi + ns;
    a.stage = words <= HMS_RG_STAGE_WORDS;
    return HM_OK;
}

/* the hours and the group of a region query, as a view's */
static void stream_region_select(HmsRegionArgs& a, const HourWindow& w, int64_t group)
{
    a.v.alltime = w.kind == HW_ALLTIME;
    a.v.lo = w.lo, a.v.hi = w.hi;
    a.v.gmode = group == HM_VIEW_MERGED ? HMS_VIEW_MERGED : (group == HM_VIEW_EACH ? HMS_VIEW_EACH : HMS_VIEW_GROUP);
    a.v.group = group >= 0 ? (uint32_t)group : 0u;
}

extern "C" int hm_stream_region_series(hm_stream* s, int64_t hour_lo, int64_t hour_hi, int64_t frame_hours,
                                       int64_t group, const hm_regions* regions, uint64_t* totals_out)
{
    if (!s || !regions || !totals_out || group < HM_VIEW_MERGED || group > (int64_t)HMS_NOGROUP) return HM_E_ARG;
    const bool alltime = hour_lo == HM_STREAM_ALLTIME && hour_hi == HM_STREAM_ALLTIME;
    HmsRegionArgs a;
    int st;
    if ((st = stream_region_table(s, regions, a))) return st;
    HmsFramePlan p;
    p.nframes = 1, p.frame0 = 0, p.lo = 0, p.hi = 1, p.fh = 1, p.phase = 0;
    if (!alltime && hms_frame_plan((int64_t)s->base, hour_lo, hour_hi, frame_hours,
                                   HM_REGION_MAX_TOTALS / (int64_t)a.nregions, &p))
        return HM_E_ARG;
    hm_ctx* ctx = s->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t q = ctx->stream;
    HIPCHK(hipMemsetAsync(totals_out, 0, (size_t)p.nframes * a.nregions * 8, q));
    if (a.nspans == 0 || s->llen == 0 || p.lo == p.hi) return HM_OK;   /* nothing selected: zeros */
    a.v.keys = s->log.keys.p;
    a.v.counts = s->log.counts.p;
    a.v.n = s->llen;
    a.v.buckets = s->bk;
    a.v.cb = s->cb;
    a.v.keys_out = a.v.counts_out = nullptr;
    a.v.cursor = nullptr;
    a.v.state = s->state;
    stream_region_select(a, HourWindow{alltime ? HW_ALLTIME : HW_RANGE, p.lo, p.hi}, group);
    /* the frames the clamped hours reach, counted from the first one's */
    int64_t nfl = alltime ? 1 : (int64_t)((p.hi - 1 - p.lo + p.phase) / p.fh) + 1;
    nfl = std::min<int64_t>(nfl, p.nframes - p.frame0);
    a.totals = (unsigned long long*)totals_out + (uint64_t)p.frame0 * a.nregions;
    a.ntot = (uint32_t)(nfl * a.nregions);
    a.fh = p.fh, a.phase = p.phase;
    hm_launch_stream_region(q, a, HMS_RG_SINK_TOTALS);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_stream_region_view(hm_stream* s, int64_t hour_lo, int64_t hour_hi, int64_t group,
                                     const hm_regions* regions, uint64_t* keys_out, uint64_t* counts_out,
                                     uint32_t* groups_out, int64_t capacity, int64_t* n_out)
{
    const HourWindow w = stream_hours(s, hour_lo, hour_hi);
    if (!s || !regions || !n_out || capacity < 0 || (capacity > 0 && (!keys_out || !counts_out)) ||
        w.kind == HW_INVALID || group < HM_VIEW_EACH || group > (int64_t)HMS_NOGROUP)
        return HM_E_ARG;
    HmsRegionArgs a;
    int st;
    if ((st = stream_region_table(s, regions, a))) return st;
    *n_out = 0;
    if (a.nspans == 0 || w.kind == HW_EMPTY) return HM_OK;
    HIPCHK(hipSetDevice(s->ctx->device));
    /* the view's three passes with the region filter in place of k_stream_view */
    bool empty;
    if ((st = stream_filter_begin(s, a.v, &empty)) || empty) return st;
    stream_region_select(a, w, group);
    hm_launch_stream_region(s->ctx->stream, a, HMS_RG_SINK_CELLS);
    HIPCHK(hipGetLastError());
    return stream_merge_emit(s, keys_out, counts_out, groups_out, nullptr, capacity, n_out);
}

extern "C" int hm_stream_region_visitors(hm_stream* s, int64_t hour_lo, int64_t hour_hi, const hm_regions* regions,
                                         int64_t min_visitors, uint64_t* points_out, uint32_t* visitors_out,
                                         int64_t* withheld_out)
{
    const HourWindow w = stream_hours(s, hour_lo, hour_hi);
    if (!s || !regions || !points_out || !visitors_out || min_visitors < 1 || w.kind == HW_INVALID) return HM_E_ARG;
    HmsRegionArgs a;
    int st;
    if ((st = stream_region_table(s, regions, a))) return st;
    hm_ctx* ctx = s->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t q = ctx->stream;
    HIPCHK(hipMemsetAsync(points_out, 0, (size_t)a.nregions * 8, q));
    HIPCHK(hipMemsetAsync(visitors_out, 0, (size_t)a.nregions * 4, q));
    if (withheld_out) withheld_out[0] = withheld_out[1] = 0;
    if (a.nspans == 0 || w.kind == HW_EMPTY || s->llen == 0) return HM_OK;
    /* The filter's records: what finds no slot in a block's table goes out as
     * it is, at most one record per (survivor, covering span) pair, and every
     * block writes its table, at most HMS_RG_REC_SLOTS records.  The pass
     * counts the pairs, so a scratch that turns out short is sized exactly for
     * the second run. */
    const uint64_t tables = (uint64_t)hm_stream_region_blocks(s->llen) * HMS_RG_REC_SLOTS;
    uint64_t cap = s->llen + tables, m = 0;
    for (int run = 0;; run++) {
        if ((st = stream_buf(s->rk, cap * 8)) || (st = stream_buf(s->rc, cap * 8))) return st;
        bool empty;
        if ((st = stream_filter_begin(s, a.v, &empty))) return st;
        HIPCHK(hipMemsetAsync(s->state + HMS_ST_PAIRS, 0, 8, q));
        stream_region_select(a, w, HM_VIEW_EACH);
        a.capacity = cap;
        hm_launch_stream_region(q, a, HMS_RG_SINK_RECORDS);
        HIPCHK(hipGetLastError());
        if ((st = stream_sync_state(s))) return st;
        m = s->hstate[HMS_ST_CURSOR];
        if (m <= cap) break;
        if (run) return HM_E_HIP;   /* cannot happen: pairs + tables bounds the records */
        cap = s->hstate[HMS_ST_PAIRS] + tables;
    }
    if (m == 0) return HM_OK;
    /* the distinct (region, group) pairs, then per region their number and their counts' sum */
    if ((st = stream_buf(s->mk, m * 8)) || (st = stream_buf(s->mc, m * 8))) return st;
    int64_t nd = 0;
    if ((st = cells_merge(ctx, (const uint64_t*)s->rk.p, (const uint64_t*)s->rc.p, HM_CELLS_U64, (int64_t)m, nullptr, 0,
                          (uint64_t*)s->mk.p, (uint64_t*)s->mc.p, (int64_t)m, &nd)))
        return st;
    HIPCHK(hipMemsetAsync(s->state + HMS_ST_WCELLS, 0, 2 * 8, q));   /* WCELLS, WPOINTS */
    hm_launch_region_visit_fold(q, (const uint64_t*)s->mk.p, (const uint64_t*)s->mc.p, (uint64_t)nd, a.nregions,
                                points_out, visitors_out);
    hm_launch_region_visit_sweep(q, a.nregions, (uint64_t)min_visitors, points_out, visitors_out, s->state);
    HIPCHK(hipGetLastError());
    if ((st = stream_sync_state(s))) return st;
    if (withheld_out) {
        withheld_out[0] = (int64_t)s->hstate[HMS_ST_WCELLS];
        withheld_out[1] = (int64_t)s->hstate[HMS_ST_WPOINTS];
    }
    return HM_OK;
}

/* a raster's tiles, group and log into the kernel's struct: everything but
 * its hours and its grid */
static void stream_raster_fill(const hm_stream* s, int64_t group, const int64_t* tiles, int ntiles, int bins_log2,
                               int halo, HmsRasterArgs& a)
{
    const int64_t W = (1ll << bins_log2) + 2 * halo;
    uint64_t box_hi = 0;
    a.box_lo = ~0ull;
    for (int t = 0; t < ntiles; t++) {
        const int64_t z = tiles[3 * t] + bins_log2, side = 1ll << z;
        const int64_t oy = (tiles[3 * t + 1] << bins_log2) - halo, ox = (tiles[3 * t + 2] << bins_log2) - halo;
        /* the haloed square clipped to [0, 2^z)^2: never empty, the tile itself is inside */
        const int64_t rlo = std::max<int64_t>(oy, 0), rhi = std::min<int64_t>(oy + W, side);
        const int64_t clo = std::max<int64_t>(ox, 0), chi = std::min<int64_t>(ox + W, side);
        const HmsRectIds ids = hms_rect_ids((int)z, rlo, rhi, clo, chi, &a.box_lo, &box_hi);
        a.rects[t] = HmsRasterRect{ids.id_lo, ids.span, ids.col_lo, ids.col_w, (uint8_t)z, (uint8_t)(rlo - oy),
                                   (uint8_t)(clo - ox), 0, 0};
    }
    a.box_span = box_hi - a.box_lo;
    a.keys = s->log.keys.p;
    a.counts = s->log.counts.p;
    a.n = s->llen;
    a.buckets = s->bk;
    a.cb = s->cb;
    a.ntiles = ntiles;
    a.gmode = group == HM_VIEW_MERGED ? HMS_VIEW_MERGED : HMS_VIEW_GROUP;
    a.group = group >= 0 ? (uint32_t)group : 0u;
    a.W = (uint32_t)W;
    a.fh = 1, a.phase = 0, a.fstride = 0;
}

extern "C" int hm_stream_raster(hm_stream* s, int64_t hour_lo, int64_t hour_hi, int64_t group, const int64_t* tiles,
                                int ntiles, int bins_log2, int halo, uint64_t* grid_out)
{
    const HourWindow w = stream_hours(s, hour_lo, hour_hi);
    if (!s || !grid_out || w.kind == HW_INVALID || group < HM_VIEW_MERGED || group > (int64_t)HMS_NOGROUP ||
        !raster_args_ok(tiles, ntiles, bins_log2, halo, s->zmin, s->zmax))
        return HM_E_ARG;
    hm_ctx* ctx = s->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t q = ctx->stream;
    const int64_t S = 1ll << bins_log2, W = S + 2 * halo;
    HIPCHK(hipMemsetAsync(grid_out, 0, (size_t)ntiles * W * W * 8, q));
    if (w.kind == HW_EMPTY) return HM_OK;   /* all of it outside the stream's hours */
    if (s->llen == 0) return HM_OK;
    HmsRasterArgs a;
    stream_raster_fill(s, group, tiles, ntiles, bins_log2, halo, a);
    a.alltime = w.kind == HW_ALLTIME;
    a.lo = w.lo, a.hi = w.hi;
    a.grid = (unsigned long long*)grid_out;
    hm_launch_stream_raster(q, a);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_stream_raster_frames(hm_stream* s, int64_t hour_lo, int64_t hour_hi, int64_t frame_hours,
                                       int64_t group, const int64_t* tiles, int ntiles, int bins_log2, int halo,
                                       uint64_t* grid_out)
{
    HmsFramePlan p;
    if (!s || !grid_out || (hour_lo == HM_STREAM_ALLTIME && hour_hi == HM_STREAM_ALLTIME) ||
        hms_frame_plan((int64_t)s->base, hour_lo, hour_hi, frame_hours, HM_RASTER_MAX_FRAMES, &p) ||
        group < HM_VIEW_MERGED || group > (int64_t)HMS_NOGROUP ||
        !raster_args_ok(tiles, ntiles, bins_log2, halo, s->zmin, s->zmax))
        return HM_E_ARG;
    hm_ctx* ctx = s->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t q = ctx->stream;
    const int64_t W = (1ll << bins_log2) + 2 * halo;
    const uint64_t fstride = (uint64_t)ntiles * W * W;
    HIPCHK(hipMemsetAsync(grid_out, 0, (size_t)p.nframes * fstride * 8, q));
    if (p.lo == p.hi) return HM_OK;         /* all of it outside the stream's hours */
    if (s->llen == 0) return HM_OK;
    HmsRasterArgs a;
    stream_raster_fill(s, group, tiles, ntiles, bins_log2, halo, a);
    a.alltime = 0;
    a.lo = p.lo, a.hi = p.hi;
    a.fh = p.fh, a.phase = p.phase, a.fstride = fstride;
    a.grid = (unsigned long long*)grid_out + (uint64_t)p.frame0 * fstride;   /* the first clamped hour's frame */
    hm_launch_stream_raster_frames(q, a);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

/* ---- retention and forgetting: the log filtered into the alternate arrays,
 * the buckets that stay moved to a fresh table (hm_stream_expire,
 * hm_stream_forget) ---- */

/* Ahead of the pass: the alternate arrays and the fresh table are there (made
 * on first use), the table is empty, and the words the pass counts into are
 * zero: the cells kept (CURSOR), the buckets moved (BUCKETS) and, afterwards,
 * listed (NLIST).  The stream's own bucket count comes back if nothing turns
 * out to be dropped (stream_refile_end). */
static int stream_refile_begin(hm_stream* s)
{
    hipStream_t q = s->ctx->stream;
    int st;
    premap_join(s);
    const uint64_t nb = s->bk.mask + 1;
    if (!s->alt.keys.p && (st = log_alloc(s, s->alt, s->lcap))) return st;
    if (!s->bk_alt && hipMalloc((void**)&s->bk_alt, nb * 8) != hipSuccess) {
        (void)hipGetLastError();
        s->bk_alt = nullptr;
        return HM_E_NOMEM;
    }
    unsigned long long* init = s->hstate + HMS_ST_COUNT;
    for (int j = 0; j < HMS_ST_COUNT; j++) init[j] = 0;
    /* CURSOR, BUCKETS, BFULL, EXOTIC, BMM, NLIST in one copy */
    HIPCHK(hipMemcpyAsync(s->state + HMS_ST_CURSOR, init, (HMS_ST_NLIST - HMS_ST_CURSOR + 1) * 8,
                          hipMemcpyHostToDevice, q));
    hm_launch_stream_fill(q, s->bk_alt, nb, HMS_EMPTY);
    return HM_OK;
}

/* Behind the pass: the one wait, then either nothing was dropped and the
 * stream stays as it is (old_buckets: its bucket count before the pass), or
 * the alternate arrays and the fresh table become the stream's. */
static int stream_refile_end(hm_stream* s, uint64_t old_buckets, int64_t* cells_dropped, int64_t* buckets_freed)
{
    hipStream_t q = s->ctx->stream;
    const uint64_t nb = s->bk.mask + 1;
    unsigned long long* init = s->hstate + HMS_ST_COUNT;
    hm_launch_stream_occupied(q, HmsBuckets{s->bk_alt, s->bk.mask}, s->blist, s->state + HMS_ST_NLIST);
    HIPCHK(hipGetLastError());
    /* log_buckets holds old slot ids: it is rebuilt from the new table's
     * occupied slots, read back as a list (a superset of the buckets with
     * cells in the log -- a forget also carries buckets over that have none,
     * which costs at most an early compaction; there are no more of them than
     * the old table's buckets) */
    std::vector<uint32_t> slots((size_t)std::min<uint64_t>(old_buckets, nb));
    if (!slots.empty())
        HIPCHK(hipMemcpyAsync(slots.data(), s->blist, slots.size() * 4, hipMemcpyDeviceToHost, q));
    const int st = stream_sync_state(s);
    const uint64_t kept = s->hstate[HMS_ST_CURSOR], nslots = s->hstate[HMS_ST_NLIST];
    const bool bad = st || s->hstate[HMS_ST_BFULL] || kept > s->llen || nslots != s->nbuckets || nslots > slots.size();
    if (bad || kept == s->llen) {
        /* nothing dropped (or, cannot happen, the pass failed): the stream stays as it is */
        s->nbuckets = old_buckets;
        init[0] = old_buckets;
        HIPCHK(hipMemcpyAsync(s->state + HMS_ST_BUCKETS, init, 8, hipMemcpyHostToDevice, q));
        HIPCHK(hm_sync(q));
        return st ? st : (bad ? HM_E_HIP : HM_OK);
    }
    std::swap(s->log, s->alt);
    std::swap(s->bk.keys, s->bk_alt);
    if (cells_dropped) *cells_dropped = (int64_t)(s->llen - kept);
    if (buckets_freed) *buckets_freed = (int64_t)(old_buckets - s->nbuckets);
    s->llen = kept;
    /* a filter of distinct keys stays distinct: a compact log stays compact */
    if (kept == 0) s->compact = true;
    s->log_buckets.clear();
    s->log_buckets.insert(slots.begin(), slots.begin() + (size_t)nslots);
    /* slot ids changed: no bucket is flagged by an earlier batch */
    HIPCHK(hipMemsetAsync(s->bflag, 0, nb * 4, q));
    s->last_nparts = 1;
    return HM_OK;
}

extern "C" int hm_stream_expire(hm_stream* s, int64_t before_hour, int64_t* cells_dropped, int64_t* buckets_freed)
{
    if (!s) return HM_E_ARG;
    if (cells_dropped) *cells_dropped = 0;
    if (buckets_freed) *buckets_freed = 0;
    const uint32_t cut = stream_hour_offset(s, before_hour);
    if (cut == 0 || s->llen == 0) return HM_OK;   /* nothing is dated before the base hour */
    HIPCHK(hipSetDevice(s->ctx->device));
    const uint64_t old_buckets = s->nbuckets;
    int st;
    if ((st = stream_refile_begin(s))) return st;
    HmsExpireArgs a;
    a.keys = s->log.keys.p;
    a.counts = s->log.counts.p;
    a.n = s->llen;
    a.old_buckets = s->bk;
    a.new_buckets.keys = s->bk_alt;
    a.new_buckets.mask = s->bk.mask;
    a.cb = s->cb;
    a.cut = cut;
    a.keys_out = s->alt.keys.p;
    a.counts_out = s->alt.counts.p;
    a.cursor = s->state + HMS_ST_CURSOR;
    a.state = s->state;
    hm_launch_stream_expire(s->ctx->stream, a);
    return stream_refile_end(s, old_buckets, cells_dropped, buckets_freed);
}

/* ---- selections of (group, hour) buckets (hm_stream_forget,
 * hm_stream_export_select) ---- */
namespace {
struct Selection {
    std::vector<uint32_t> ids;   /* sorted and distinct; empty: every group */
    HourWindow w;
};
}  // namespace

/* the caller's groups and hours checked and normalised; false: HM_E_ARG */
static bool stream_selection(const hm_stream* s, const uint32_t* groups, int64_t ngroups, int64_t hour_lo,
                             int64_t hour_hi, Selection& sel)
{
    sel.w = stream_hours(s, hour_lo, hour_hi);
    if (!s || sel.w.kind == HW_INVALID) return false;
    if (groups ? (ngroups < 1 || ngroups > HM_SELECT_MAX_GROUPS) : ngroups != 0) return false;
    sel.ids.resize((size_t)ngroups);
    const int64_t m = hms_select_ids(groups, ngroups, sel.ids.data());
    if (m < 0) return false;
    sel.ids.resize((size_t)m);
    return true;
}

/* The selection's verdict per bucket slot enqueued (k_stream_select), in
 * context scratch (*map_out).  fresh: the empty table the buckets that stay
 * are moved to (a forget), or NULL (verdicts only).  The ids' upload reads
 * sel.ids: the caller keeps it until the stream has been waited for. */
static int stream_select_run(hm_stream* s, const Selection& sel, uint64_t* fresh, uint32_t** map_out)
{
    hm_ctx* ctx = s->ctx;
    hipStream_t q = ctx->stream;
    uint32_t *ids = nullptr, *map = nullptr;
    ENSURE(B_SEL_MAP, (s->bk.mask + 1) * 4, map);
    if (!sel.ids.empty()) {
        ENSURE(B_SEL_IDS, sel.ids.size() * 4, ids);
        HIPCHK(hipMemcpyAsync(ids, sel.ids.data(), sel.ids.size() * 4, hipMemcpyHostToDevice, q));
    }
    HmsSelectArgs a;
    a.old_buckets = s->bk;
    a.new_buckets.keys = fresh;
    a.new_buckets.mask = s->bk.mask;
    a.ids = ids;
    a.nids = (uint32_t)sel.ids.size();
    a.alltime = sel.w.kind == HW_ALLTIME;
    a.lo = sel.w.lo;
    a.hi = sel.w.hi;
    a.remap = map;
    a.state = s->state;
    hm_launch_stream_select(q, a);
    HIPCHK(hipGetLastError());
    *map_out = map;
    return HM_OK;
}

static int stream_forget_run(hm_stream* s, const Selection& sel, int64_t* cells_dropped, int64_t* buckets_freed)
{
    const uint64_t old_buckets = s->nbuckets;
    uint32_t* map = nullptr;
    int st;
    if ((st = stream_refile_begin(s)) || (st = stream_select_run(s, sel, s->bk_alt, &map))) return st;
    HmsForgetArgs a;
    a.keys = s->log.keys.p;
    a.counts = s->log.counts.p;
    a.n = s->llen;
    a.remap = map;
    a.mask = s->bk.mask;
    a.cb = s->cb;
    a.keys_out = s->alt.keys.p;
    a.counts_out = s->alt.counts.p;
    a.cursor = s->state + HMS_ST_CURSOR;
    hm_launch_stream_forget(s->ctx->stream, a);
    return stream_refile_end(s, old_buckets, cells_dropped, buckets_freed);
}

/* hm_stream_expire for a selection of buckets: the selected cells leave the
 * log in one pass (k_stream_select, k_stream_forget), the buckets that stay
 * move to a fresh table */
extern "C" int hm_stream_forget(hm_stream* s, const uint32_t* groups, int64_t ngroups, int64_t hour_lo, int64_t hour_hi,
                                int64_t* cells_dropped, int64_t* buckets_freed)
{
    Selection sel;
    if (!stream_selection(s, groups, ngroups, hour_lo, hour_hi, sel)) return HM_E_ARG;
    if (cells_dropped) *cells_dropped = 0;
    if (buckets_freed) *buckets_freed = 0;
    if (sel.w.kind == HW_EMPTY || s->llen == 0) return HM_OK;   /* no hour of the stream's, or no cell at all */
    HIPCHK(hipSetDevice(s->ctx->device));
    const int st = stream_forget_run(s, sel, cells_dropped, buckets_freed);
    if (st) (void)hipStreamSynchronize(s->ctx->stream);   /* (sel.ids may still be read) */
    return st;
}

static int stream_export_select_run(hm_stream* s, const Selection& sel, uint64_t* keys_out, uint64_t* counts_out,
                                    uint32_t* groups_out, uint32_t* hours_out, int64_t capacity, int64_t* n_out)
{
    hipStream_t q = s->ctx->stream;
    uint32_t* map = nullptr;
    int st;
    HIPCHK(hipMemsetAsync(s->state + HMS_ST_CURSOR, 0, 8, q));
    if ((st = stream_select_run(s, sel, nullptr, &map))) return st;
    HmsExportSelArgs a;
    a.e = stream_emit_args(s, s->log.keys.p, s->log.counts.p, s->llen, keys_out, counts_out, groups_out, hours_out);
    a.verdict = map;
    a.capacity = (uint64_t)capacity;
    a.cursor = s->state + HMS_ST_CURSOR;
    hm_launch_stream_export_select(q, a);
    HIPCHK(hipGetLastError());
    if ((st = stream_sync_state(s))) return st;
    *n_out = (int64_t)s->hstate[HMS_ST_CURSOR];
    return *n_out > capacity ? HM_E_CAPACITY : HM_OK;
}

/* hm_stream_export for a selection of buckets: the compacted log's selected
 * cells, listed and counted in one pass (k_stream_select,
 * k_stream_export_select) */
extern "C" int hm_stream_export_select(hm_stream* s, const uint32_t* groups, int64_t ngroups, int64_t hour_lo,
                                       int64_t hour_hi, uint64_t* keys_out, uint64_t* counts_out, uint32_t* groups_out,
                                       uint32_t* hours_out, int64_t capacity, int64_t* n_out)
{
    Selection sel;
    if (!n_out || capacity < 0 || (capacity > 0 && (!keys_out || !counts_out)) ||
        !stream_selection(s, groups, ngroups, hour_lo, hour_hi, sel))
        return HM_E_ARG;
    *n_out = 0;
    HIPCHK(hipSetDevice(s->ctx->device));
    int st;
    if ((st = stream_compact(s))) return st;
    if (sel.w.kind == HW_EMPTY || s->llen == 0) return HM_OK;
    st = stream_export_select_run(s, sel, keys_out, counts_out, groups_out, hours_out, capacity, n_out);
    if (st && st != HM_E_CAPACITY) (void)hipStreamSynchronize(s->ctx->stream);   /* (sel.ids may still be read) */
    return st;
}

/* the whole log, compacted, in one pass (k_stream_export): the log's buckets
 * are raw, so a cell's bucket key is its group and hour (no relabel, no merge) */
extern "C" int hm_stream_export(hm_stream* s, uint64_t* keys_out, uint64_t* counts_out, uint32_t* groups_out,
                                uint32_t* hours_out, int64_t capacity, int64_t* n_out)
{
    if (!s || !n_out || capacity < 0 || (capacity > 0 && (!keys_out || !counts_out))) return HM_E_ARG;
    *n_out = 0;
    HIPCHK(hipSetDevice(s->ctx->device));
    int st;
    if ((st = stream_compact(s))) return st;
    *n_out = (int64_t)s->llen;
    if (s->llen == 0) return HM_OK;
    if ((int64_t)s->llen > capacity) return HM_E_CAPACITY;
    hm_launch_stream_export(s->ctx->stream, stream_emit_args(s, s->log.keys.p, s->log.counts.p, s->llen, keys_out,
                                                             counts_out, groups_out, hours_out));
    HIPCHK(hipGetLastError());
    return HM_OK;
}

/* pre-aggregated cells appended at the log's tail (k_stream_import), their
 * buckets listed as a batch's are; one state read-back, and the tail becomes
 * part of the log only when every cell was valid and found a bucket */
extern "C" int hm_stream_import(hm_stream* s, const uint64_t* keys, const uint64_t* counts, const uint32_t* groups,
                                const uint32_t* hours, int64_t n, int flags)
{
    if (!s || n < 0 || (n > 0 && (!keys || !counts)) || (flags & ~HM_IMPORT_DISTINCT)) return HM_E_ARG;
    hm_ctx* ctx = s->ctx;
    int st;
    if ((st = stream_batch_begin(s, n, (uint64_t)n)) || n == 0) return st;
    hipStream_t q = ctx->stream;
    HmsImportArgs a;
    a.keys = keys;
    a.counts = counts;
    a.groups = groups;
    a.hours = hours;
    a.n = (uint64_t)n;
    a.buckets = s->bk;
    a.cb = s->cb;
    a.zmin = s->zmin;
    a.zmax = s->zmax;
    a.base = s->base;
    a.keys_out = s->log.keys.p + s->llen;
    a.counts_out = s->log.counts.p + s->llen;
    a.bflag = s->bflag;
    a.epoch = s->epoch;
    a.state = s->state;
    hm_launch_stream_import(q, a);
    const uint64_t nb = s->bk.mask + 1;
    hm_launch_stream_collect(q, s->bflag, nb, s->epoch, s->blist, s->state);
    HIPCHK(hipGetLastError());
    /* the import's bucket list comes back with the state: a first part is
     * copied unasked (an export of a time-ordered stream has few buckets), the
     * rest only when there is more */
    std::vector<uint32_t> list((size_t)std::min<uint64_t>({(uint64_t)n, nb, 1024}));
    HIPCHK(hipMemcpyAsync(list.data(), s->blist, list.size() * 4, hipMemcpyDeviceToHost, q));
    if ((st = stream_sync_state(s))) return st;
    const unsigned long long e = s->hstate[HMS_ST_ERR];
    if (e != ~0ull) {
        ctx->last_err_index = (int64_t)(e >> 8);
        ctx->last_err_kind = HM_E_ARG;
        return HM_E_ARG;
    }
    if (s->hstate[HMS_ST_BFULL]) return HM_E_CAPACITY;   /* max_buckets (group, hour) pairs */
    const uint64_t nlist = s->hstate[HMS_ST_NLIST];
    if (nlist > nb) return HM_E_HIP;   /* cannot happen */
    if (nlist > list.size()) {
        list.resize((size_t)nlist);
        HIPCHK(hipMemcpyAsync(list.data(), s->blist, (size_t)nlist * 4, hipMemcpyDeviceToHost, q));
        HIPCHK(hm_sync(q));
    }
    /* compactness: the log's buckets stay exactly known (the import's list
     * joins them); its keys stay distinct only when the caller promises the
     * input's are and none of its buckets has cells in the log yet */
    if (s->llen == 0) s->compact = true;
    stream_appended(s, (uint64_t)n, list.data(), (uint32_t)nlist);
    if (!(flags & HM_IMPORT_DISTINCT)) s->compact = false;
    s->last_nparts = 1;   /* the next batch is counted speculatively as one bucket again */
    return HM_OK;
}

extern "C" int hm_stream_extract(hm_stream* s, int64_t hour, uint64_t* keys_out, uint64_t* counts_out,
                                 uint32_t* hours_out, int64_t capacity, int64_t* n_out)
{
    if (!s) return HM_E_ARG;
    if (hour == HM_STREAM_ALLTIME)
        return hm_stream_rollup(s, HM_SPAN_ALLTIME, 1, -1, keys_out, counts_out, nullptr, nullptr, capacity, n_out);
    if (hour == HM_STREAM_EACH_HOUR)
        return hm_stream_rollup(s, HM_SPAN_HOUR, 1, -1, keys_out, counts_out, nullptr, hours_out, capacity, n_out);
    if (hour < (int64_t)s->base || hour - (int64_t)s->base >= HM_STREAM_MAX_HOURS) return HM_E_ARG;
    return hm_stream_rollup(s, HM_SPAN_HOUR, 1, hour, keys_out, counts_out, nullptr, hours_out, capacity, n_out);
}

extern "C" int hm_stream_destroy(hm_stream* s)
{
    if (!s) return HM_OK;
    premap_join(s);
    if (s->ctx) (void)hipSetDevice(s->ctx->device);
    if (s->ctx && s->ctx->stream) (void)hipStreamSynchronize(s->ctx->stream);
    for (void* p : {(void*)s->state, (void*)s->bk.keys, (void*)s->bk_alt, (void*)s->bflag, (void*)s->blist,
                    (void*)s->bloc, s->bids.p, s->rec.p, s->plat.p, s->plon.p, s->pkeep.p, s->pstart.p, s->rk.p,
                    s->rc.p, s->mk.p, s->mc.p, s->tk.p, s->tc.p, s->vt.p, s->vv.p, s->gt.p})
        if (p) (void)hipFree(p);
    if (s->ghost) (void)hipHostFree(s->ghost);
    if (s->gev) (void)hipEventDestroy(s->gev);
    log_free(s, s->log);
    log_free(s, s->alt);
    if (s->hstate) (void)hipHostFree(s->hstate);
    for (int t = 0; t < HMS_PAR; t++) {
        for (void* p : {s->pk[t].p, s->pc[t].p})
            if (p) (void)hipFree(p);
        if (s->pctx[t]) {
            hipStream_t q = s->pctx[t]->stream;
            hm_ctx_destroy(s->pctx[t]);
            if (q) (void)hipStreamDestroy(q);
        }
    }
    if (s->pev) (void)hipEventDestroy(s->pev);
    delete s;
    return HM_OK;
}
