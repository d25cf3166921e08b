/* C-ABI of heatmap_amd (include/heatmap_amd.h): context, device memory arena
 * and the host-side orchestration of the count pipeline.
 *
 * Per hm_count call (Z = zmax, zb = max(0, Z-7)):
 *   levels z_1 = min(6, zb), z_{l+1} = min(z_l + 5, zb) ... z_L = zb
 *   k_project_partition (level 1) -> [k_runscan, scan, k_compact, k_partition]*
 *   -> k_aggregate (zooms Z..zb+1) -> k_pool for l = L..1 (zooms zb..0).
 * The host reads back two or three scalars per level (bucket and work-item
 * counts) to size the next grid; everything else stays on the device.
 * The driver is CountCall: run() calls its phases in that order, and LevelOut
 * is what one level hands to the next.
 *
 * Also here: the general path's driver, the cell merges and routes, the
 * formatters and the context-level rasters.  The streaming heatmap
 * (hm_stream_*) is hm_stream_api.cpp; hm_ctx.h holds what the two share.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <math.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "hm_genkey.h"
#include "hm_ctx.h"

namespace {

struct Level {
    int zc;              /* child zoom z_l */
    int dbits;           /* 2*(z_l - z_{l-1}) */
    uint32_t nparents;   /* |B_{l-1}| */
    uint64_t nchildren;  /* nparents << dbits */
    uint32_t count = 0;  /* |B_l| */
    uint32_t items = 0;  /* work items of the next stage */
    bool out16 = false;
};

}  // namespace

#define HM_SPREAD_MIN_KEYS (1u << 19)
/* with hot tiles: the cold keys' mean level-1 bucket above which they take
 * 3-zoom levels.  Off by default: measured slower (hotspots 6.6 -> 7.0 ms,
 * skew 15.4 -> 24.7 ms: the middle level's run-streaming partition and a
 * pool over 64K zoom-8 buckets cost more than the short runs they save) */
#define HM_SPREAD_MIN_COLD 1e30
#define HM_SPREAD_ZOOMS 3

int hip_fail(hipError_t e, const char* what)
{
    if (e == hipSuccess) return HM_OK;
    fprintf(stderr, "heatmap_amd: HIP error in %s: %s\n", what, hipGetErrorString(e));
    return HM_E_HIP;
}

/* Wait for the stream.  HM_SYNC_SPIN_US > 0 (environment, read once per
 * process): poll it for up to that long first, then block.  (Measured with a
 * HIP API trace: after a polled wait the next few launches took ~60 us each
 * instead of ~6, so the default is a plain blocking wait.) */
static int hm_spin_us()
{
    static const int us = [] {
        const char* e = getenv("HM_SYNC_SPIN_US");
        return e ? atoi(e) : 0;
    }();
    return us;
}
hipError_t hm_sync(hipStream_t s)
{
    const int spin = hm_spin_us();
    if (spin > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t e = hipStreamQuery(s);
            if (e != hipErrorNotReady) return e;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin)) break;
        }
    }
    return hipStreamSynchronize(s);
}

int ensure(hm_ctx* c, int slot, size_t bytes, void** out)
{
    if (bytes == 0) bytes = 16;
    Buf& b = c->bufs[slot];
    if (b.cap < bytes) {
        if (b.p) HIPCHK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
        size_t want = bytes + bytes / 8;
        if (hipMalloc(&b.p, want) != hipSuccess) {
            (void)hipGetLastError();
            b.p = nullptr;
            return HM_E_NOMEM;
        }
        b.cap = want;
    }
    *out = b.p;
    return HM_OK;
}

/* the arena is a cache: after an allocation failure every buffer is
 * released at the API boundary (nothing of the failed call is in flight
 * past the synchronisation) so the next call starts from an empty arena */
void arena_release(hm_ctx* c)
{
    (void)hipStreamSynchronize(c->stream);
    for (auto& b : c->bufs) {
        if (b.p) (void)hipFree(b.p);
        b.p = nullptr;
        b.cap = 0;
    }
    (void)hipGetLastError();
}

extern "C" {

int hm_abi_version(void) { return HM_ABI_VERSION; }

const char* hm_status_string(int s)
{
    switch (s) {
    case HM_OK: return "ok";
    case HM_E_NAN: return "cannot convert float NaN to integer";
    case HM_E_DOMAIN: return "math domain error";
    case HM_E_INF: return "cannot convert float infinity to integer";
    case HM_E_RANGE: return "value outside the range supported by the device path";
    case HM_E_EXOTIC: return "the streaming heatmap holds tiles inside [0, 2^zmax)^2 only";
    case HM_E_ARG: return "invalid argument";
    case HM_E_CAPACITY: return "output capacity too small";
    case HM_E_WIDE: return "a routed count needs 64 bits (route again with count_bytes = 8)";
    case HM_E_HIP: return "HIP runtime error";
    case HM_E_NOMEM: return "device allocation failed";
    default: return "unknown status";
    }
}

int hm_ctx_create(hm_ctx** out, int device, void* stream)
{
    if (!out) return HM_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device || device < 0) {
        (void)hipGetLastError();
        fprintf(stderr, "heatmap_amd: no HIP device %d (found %d); there is no CPU fallback\n", device, n);
        return HM_E_HIP;
    }
    HIPCHK(hipSetDevice(device));
    hm_ctx* c = new hm_ctx();
    c->device = device;
    c->stream = (hipStream_t)stream;
    c->bufs.resize(B_COUNT);
    for (int i = 0; i < HM_NEV; i++) c->ev[i] = nullptr;
    c->spread_min_keys = HM_SPREAD_MIN_KEYS;
    if (const char* e = getenv("HM_SPREAD_MIN_KEYS")) c->spread_min_keys = atof(e);
    c->spread_min_cold = HM_SPREAD_MIN_COLD;
    if (const char* e = getenv("HM_SPREAD_MIN_COLD")) c->spread_min_cold = atof(e);
    c->rs_big_min = HM_RS_BIG;
    if (const char* e = getenv("HM_RS_BIG_MIN")) c->rs_big_min = (uint64_t)atoll(e);
    if (const char* e = getenv("HM_HOT")) c->hot = atoi(e);
    if (const char* e = getenv("HM_HOT_MID")) c->hot_mid = atoi(e);
    if (const char* e = getenv("HM_HOT_INV_SHARE")) c->hot_inv_share = atof(e);
    if (const char* e = getenv("HM_HOT_MIN_KEYS")) c->hot_min_keys = atof(e);
    if (const char* e = getenv("HM_RUN_SHARD_BITS")) c->run_shard_bits = atoi(e);
    if (const char* e = getenv("HM_SAMPLE_LOG2")) c->sample_log2 = std::min(30, std::max(8, atoi(e)));
    if (const char* e = getenv("HM_DEBUG_L1")) c->debug_l1 = atoi(e);
    if (const char* e = getenv("HM_STAGE_TIMING")) c->stage_timing = atoi(e);
    if (const char* e = getenv("HM_CONTIG")) c->contig = atoi(e);
    if (const char* e = getenv("HM_TA_MIN")) c->ta_min = (uint32_t)std::max(1024, std::min((int)HM_TA, atoi(e)));
    if (const char* e = getenv("HM_TA_ITEMS")) c->ta_items = (uint32_t)std::max(1, atoi(e));
    int st = HM_OK;
    if (hipMalloc(&c->state, ST_COUNT * sizeof(unsigned long long)) != hipSuccess) {
        c->state = nullptr;
        st = HM_E_NOMEM;
    } else if (hipHostMalloc(&c->host_state, 4 * ST_COUNT * sizeof(unsigned long long)) != hipSuccess) {
        c->host_state = nullptr;
        st = HM_E_NOMEM;
    } else if (hipHostMalloc(&c->host_aux, (2 + 2 * HM_L1_SHARDS) * HM_D1 * sizeof(uint32_t)) != hipSuccess) {
        c->host_aux = nullptr;
        st = HM_E_NOMEM;
    }
    for (int i = 0; i < HM_NEV && st == HM_OK; i++)
        if (hipEventCreate(&c->ev[i]) != hipSuccess) {
            c->ev[i] = nullptr;
            st = HM_E_HIP;
        }
    if (st != HM_OK) {
        (void)hipGetLastError();
        hm_ctx_destroy(c);
        return st;
    }
    *out = c;
    return HM_OK;
}

int hm_ctx_set_stream(hm_ctx* c, void* stream)
{
    if (!c) return HM_E_ARG;
    c->stream = (hipStream_t)stream;
    return HM_OK;
}

int hm_ctx_tune(hm_ctx* c, const char* name, double value, double* old)
{
    if (!c || !name) return HM_E_ARG;
    double prev;
    if (!strcmp(name, "HM_SPREAD_MIN_KEYS")) {
        prev = c->spread_min_keys;
        c->spread_min_keys = value;
    } else if (!strcmp(name, "HM_SPREAD_MIN_COLD")) {
        prev = c->spread_min_cold;
        c->spread_min_cold = value;
    } else if (!strcmp(name, "HM_CONTIG")) {
        prev = c->contig;
        c->contig = value != 0;
    } else if (!strcmp(name, "HM_STAGE_TIMING")) {
        prev = c->stage_timing;
        c->stage_timing = value != 0;
    } else if (!strcmp(name, "HM_SAMPLE_LOG2")) {
        if (!(value >= 8 && value <= 30)) return HM_E_ARG;
        prev = c->sample_log2;
        c->sample_log2 = (int)value;
    } else if (!strcmp(name, "HM_RS_BIG_MIN")) {
        prev = (double)c->rs_big_min;
        c->rs_big_min = (uint64_t)(value < 0 ? 0 : value);
    } else if (!strcmp(name, "HM_HOT")) {
        prev = c->hot;
        c->hot = value != 0;
    } else if (!strcmp(name, "HM_HOT_MID")) {
        prev = c->hot_mid;
        c->hot_mid = value != 0;
    } else if (!strcmp(name, "HM_HOT_INV_SHARE")) {
        if (!(value >= 1)) return HM_E_ARG;
        prev = c->hot_inv_share;
        c->hot_inv_share = value;
    } else if (!strcmp(name, "HM_HOT_MIN_KEYS")) {
        prev = c->hot_min_keys;
        c->hot_min_keys = value;
    } else if (!strcmp(name, "HM_RUN_SHARD_BITS")) {
        if (value > 5) return HM_E_ARG;
        prev = c->run_shard_bits;
        c->run_shard_bits = value < 0 ? -1 : (int)value;
    } else if (!strcmp(name, "HM_TA_MIN")) {
        const uint32_t v = (value >= 1024 && value <= (double)HM_TA) ? (uint32_t)value : 0u;
        if (!v || (double)v != value || (v & (v - 1))) return HM_E_ARG;
        prev = c->ta_min;
        c->ta_min = v;
    } else if (!strcmp(name, "HM_TA_ITEMS")) {
        if (!(value >= 1 && value <= 4294967295.0)) return HM_E_ARG;
        prev = c->ta_items;
        c->ta_items = (uint32_t)value;
    } else {
        return HM_E_ARG;
    }
    if (old) *old = prev;
    return HM_OK;
}

int hm_ctx_destroy(hm_ctx* c)
{
    if (!c) return HM_OK;
    (void)hipSetDevice(c->device);
    for (auto& b : c->bufs)
        if (b.p) (void)hipFree(b.p);
    if (c->state) (void)hipFree(c->state);
    if (c->host_state) (void)hipHostFree(c->host_state);
    if (c->host_aux) (void)hipHostFree(c->host_aux);
    for (int i = 0; i < HM_NEV; i++)
        if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    delete c;
    return HM_OK;
}

int hm_last_error(hm_ctx* c, int64_t* index, int* kind)
{
    if (!c) return HM_E_ARG;
    if (index) *index = c->last_err_index;
    if (kind) *kind = c->last_err_kind;
    return HM_OK;
}

int hm_last_stats(hm_ctx* c, int64_t* slow_points, double* stage_us, int n_stages)
{
    if (!c) return HM_E_ARG;
    if (slow_points) *slow_points = c->last_slow;
    for (int i = 0; i < n_stages && i < 9; i++) stage_us[i] = c->stage_us[i];
    if (n_stages > 7) stage_us[7] = (double)c->last_levels;
    return HM_OK;
}

}  // extern "C"

/* the plan-tuning fields of one context copied to another (a stream's helper
 * contexts count with the settings of the stream's own) */
void ctx_copy_tuning(hm_ctx* d, const hm_ctx* c)
{
    d->spread_min_keys = c->spread_min_keys;
    d->spread_min_cold = c->spread_min_cold;
    d->sample_log2 = c->sample_log2;
    d->debug_l1 = c->debug_l1;
    d->stage_timing = c->stage_timing;
    d->contig = c->contig;
    d->ta_min = c->ta_min;
    d->ta_items = c->ta_items;
    d->rs_big_min = c->rs_big_min;
    d->hot = c->hot;
    d->hot_mid = c->hot_mid;
    d->hot_inv_share = c->hot_inv_share;
    d->hot_min_keys = c->hot_min_keys;
    d->run_shard_bits = c->run_shard_bits;
}

static int reset_state(hm_ctx* ctx)
{
    HIPCHK(hipMemsetAsync(ctx->state, 0, ST_COUNT * sizeof(unsigned long long), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->state + ST_ERR, 0xFF, sizeof(unsigned long long), ctx->stream));
    return HM_OK;
}

static int read_state(hm_ctx* ctx)
{
    HIPCHK(hipMemcpyAsync(ctx->host_state, ctx->state, ST_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(hm_sync(ctx->stream));
    return HM_OK;
}

static int take_error(hm_ctx* ctx)
{
    const unsigned long long e = ctx->host_state[ST_ERR];
    ctx->last_slow = (int64_t)ctx->host_state[ST_SLOW];
    /* the first failing point in input order (atomicMin of index << 8 | kind) */
    if (e == ~0ull) {
        ctx->last_err_index = -1;
        ctx->last_err_kind = HM_OK;
        return HM_OK;
    }
    ctx->last_err_index = (int64_t)(e >> 8);
    ctx->last_err_kind = (int)(e & 0xFF);
    return ctx->last_err_kind;
}

extern "C" int hm_project(hm_ctx* ctx, const double* lat, const double* lon, int64_t n, int zoom, int64_t* row,
                          int64_t* col, uint8_t* status)
{
    /* zoom may be negative: Tile.parent_id of a zoom-0 tile projects at zoom
     * -1, i.e. times 2**-1 = 0.5 (tile.py:60-61) */
    if (!ctx || n < 0 || zoom < -30 || zoom > 30 || (n > 0 && (!lat || !lon || !row || !col || !status)))
        return HM_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    int st = reset_state(ctx);
    if (st) return st;
    if (n > 0)
        hm_launch_project(ctx->stream, lat, lon, n, zoom, row, col, status, ctx->state + ST_ERR, ctx->state + ST_SLOW);
    HIPCHK(hipGetLastError());
    if ((st = read_state(ctx))) return st;
    return take_error(ctx);
}

/* ------------------------------------------------------------------------ */

/* ------------------------------------------------------------------------ */
/* general path: n exact zoom-Z tiles (device lists) -> records of zooms       */
/* [zmin, Z] (hm_general.hip).  *total = records (all of them, even past the   */
/* capacity).  Errors (tiles beyond the key's range) go to the error word.      */
/* ------------------------------------------------------------------------ */
static int gen_count(hm_ctx* ctx, const int64_t* row, const int64_t* col, const uint32_t* group, const int64_t* index,
                     uint64_t n, int Z, int zmin, const HmGenEmit& e, uint64_t* total, const double* lat = nullptr,
                     const double* lon = nullptr, const uint8_t* keep = nullptr)
{
    *total = 0;
    if (n == 0) return HM_OK;
    if (n >= (1ull << 32)) return HM_E_ARG;   /* radix ranks are u32 */
    hipStream_t s = ctx->stream;
    uint64_t *klo[2], *khi[2];
    unsigned long long* orand;
    ENSURE(B_GEN_KA, n * 8, klo[0]);
    ENSURE(B_GEN_KB, n * 8, klo[1]);
    ENSURE(B_GEN_KHA, n * 8, khi[0]);
    ENSURE(B_GEN_KHB, n * 8, khi[1]);
    ENSURE(B_GEN_ORAND, 4 * 8, orand);
    unsigned long long* up = ctx->host_state + ST_COUNT;
    HIPCHK(hm_sync(s));
    up[0] = 0;
    up[1] = 0;
    up[2] = ~0ull;
    up[3] = ~0ull;
    HIPCHK(hipMemcpyAsync(orand, up, 4 * 8, hipMemcpyHostToDevice, s));
    if (lat) {
        /* points: projected straight into keys (the kept ones, compacted) */
        HmPkArgs pk;
        pk.lat = lat;
        pk.lon = lon;
        pk.keep = keep;
        pk.group = group;
        pk.n = (int64_t)n;
        pk.Z = Z;
        pk.klo = klo[0];
        pk.khi = khi[0];
        pk.count = ctx->state + ST_XCOUNT;
        pk.err_word = ctx->state + ST_ERR;
        pk.orand = orand;
        pk.redo_cap = std::min<uint64_t>(n, std::max<uint64_t>(1u << 16, n / 256));
        ENSURE(B_REDO_IDX, pk.redo_cap * sizeof(uint32_t) + 4, pk.redo_idx);
        pk.redo_count = ctx->state + ST_REDO;
        pk.dense = keep == nullptr;
        pk.write_hi = 0;
        HIPCHK(hipMemsetAsync(ctx->state + ST_XCOUNT, 0, sizeof(unsigned long long), s));
        HIPCHK(hipMemsetAsync(ctx->state + ST_REDO, 0, sizeof(unsigned long long), s));
        hm_launch_project_keys(s, pk);
        HIPCHK(hipGetLastError());
        unsigned long long* dn = ctx->host_state + 2 * ST_COUNT;
        HIPCHK(hipMemcpyAsync(dn, orand, 4 * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hm_sync(s));
        if (dn[1] != dn[3]) {
            /* wide keys (groups past 2^22 at zoom 21, tiles outside the
             * square): again, with the high halves */
            HIPCHK(hipMemcpyAsync(orand, up, 4 * 8, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(ctx->state + ST_XCOUNT, 0, sizeof(unsigned long long), s));
            HIPCHK(hipMemsetAsync(ctx->state + ST_REDO, 0, sizeof(unsigned long long), s));
            pk.write_hi = 1;
            hm_launch_project_keys(s, pk);
        }
    } else {
        HmGenArgs ga;
        ga.row = row;
        ga.col = col;
        ga.group = group;
        ga.index = index;
        ga.n = n;
        ga.Z = Z;
        ga.klo = klo[0];
        ga.khi = khi[0];
        ga.orand = orand;
        ga.err_word = ctx->state + ST_ERR;
        hm_launch_gen_keys(s, ga);
    }
    HIPCHK(hipGetLastError());
    unsigned long long* down = ctx->host_state + 2 * ST_COUNT;
    HIPCHK(hipMemcpyAsync(down, orand, 4 * 8, hipMemcpyDeviceToHost, s));
    int st;
    if ((st = read_state(ctx))) return st;
    if ((st = take_error(ctx))) return st;
    if (lat && keep) {
        n = ctx->host_state[ST_XCOUNT];
        if (n == 0) return HM_OK;
    }
    /* LSD passes over the digits that differ between keys; the high halves
     * move only when they differ */
    const bool wide = down[1] != down[3];
    const unsigned __int128 var = ((((unsigned __int128)down[1]) << 64) | down[0]) ^
                                  ((((unsigned __int128)down[3]) << 64) | down[2]);
    if (e.width == 2) {
        /* packed records hold HM_KEYs: every key's super tile (its zoom-0
         * tile) must be (0, 0), i.e. the same super-tile field in all keys
         * (OR == AND there) and that field the encoding of (0, 0) */
        const int f0 = 2 * Z + 32;
        const unsigned __int128 fm = (((unsigned __int128)1 << (5 + HM_GEN_SC_BITS)) - 1) << f0;
        const unsigned __int128 orv = (((unsigned __int128)down[1]) << 64) | down[0];
        const unsigned __int128 zero = ((unsigned __int128)((uint64_t)HM_GEN_SR_BIAS << HM_GEN_SC_BITS |
                                                           (uint64_t)HM_GEN_SC_BIAS)) << f0;
        if ((var & fm) != 0 || (orv & fm) != zero) return HM_E_EXOTIC;
    }
    int shs[16], np = 0;
    for (int sh = 0; sh < 128; sh += 8)
        if ((uint64_t)((var >> sh) & 0xFF)) shs[np++] = sh;
    uint8_t* rxs;
    ENSURE(B_GEN_HIST, 256 + 16 * 2048 + hm_rx_os_tiles(n) * 2048, rxs);
    const int cur = hm_launch_rx_sort(s, wide, klo, khi, n, shs, np, rxs);
    HIPCHK(hipGetLastError());
    /* zoom cascade (k_cascade): step k makes the zoom-(Z-k) cells and writes
     * the records of zoom Z-k+1; a last launch writes the zmin records.  Item
     * counts and record offsets stay on the device (one read-back at the end) */
    const int K = Z - zmin + 1;
    const uint64_t ntc = hm_cascade_tiles(n);
    uint8_t* cs;
    uint32_t *e0, *e1;
    ENSURE(B_GEN_FLAG, 512 + 2 * ntc * 8, cs);
    ENSURE(B_GEN_IDX, n * 4, e0);
    ENSURE(B_GEN_C, n * 4, e1);
    unsigned* tick = (unsigned*)cs;
    uint32_t* mdev = (uint32_t*)(cs + 128);
    unsigned long long* rbase = (unsigned long long*)(cs + 256);
    static_assert(HM_MAX_ZOOM + 3 <= 32, "cascade state slots");
    HIPCHK(hipMemsetAsync(cs, 0, 512 + 2 * ntc * 8, s));
    HmCascArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.tstat = (uint64_t*)(cs + 512);
    ca.tstat2 = ca.tstat + ntc;
    ca.e = e;
    ca.hic = down[1];
    /* packed records: two zoom steps per launch where two levels of records
     * are left before the last (k_cascade2) */
    const bool fuse = e.width == 2 && !e.split;
    int in = cur;                       /* key buffer of the launch's input */
    uint32_t* ecur = nullptr;           /* ENDs of the input cells (none: raw keys) */
    uint32_t* eb[2] = {e0, e1};
    int eo = 0;
    int slot = 0;                       /* launch index: its count, record base, ticket and epoch */
    for (int kz = 0;;) {                /* the input level is zoom Z - kz + 1 (kz >= 1), raw keys at kz = 0 */
        const bool last = kz == K;
        const bool two = fuse && kz >= 1 && kz + 2 <= K;
        ca.kin_lo = klo[in];
        ca.kin_hi = khi[in];
        ca.ein = ecur;
        ca.m_in = slot ? mdev + (slot - 1) : nullptr;
        ca.m_host = n;
        ca.clr = 2 * (two ? kz + 1 : kz);
        ca.Z = Z;
        ca.zin = Z - kz + 1;
        ca.emit = kz > 0;
        ca.kout_lo = klo[1 - in];
        ca.kout_hi = khi[1 - in];
        ca.eout = eb[eo];
        ca.m_out = mdev + slot;
        ca.epoch = (uint64_t)slot + 1;
        ca.ticket = tick + slot;
        ca.rbase_in = slot ? rbase + slot : nullptr;
        ca.rbase_out = slot ? rbase + slot + 1 : nullptr;
        hm_launch_cascade(s, ca, n, last ? 1 : (two ? 2 : 0), wide);
        HIPCHK(hipGetLastError());
        slot++;
        if (last) break;
        in = 1 - in;
        ecur = eb[eo];
        eo ^= 1;
        kz += two ? 2 : 1;
    }
    HIPCHK(hipMemcpyAsync(down, rbase + slot, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hm_sync(s));
    *total = down[0];
    return HM_OK;
}

/* hm_count for data too sparse for the pipeline's dense per-level child
 * arrays (e.g. uniform clouds at zoom 21): every kept point through the
 * general path, cells inside the square emitted as HM_KEYs */
static int count_fallback(hm_ctx* ctx, const double* lat, const double* lon, const int64_t* rows,
                          const int64_t* cols, const uint8_t* keep, int64_t n, int zmin, int zmax, uint64_t* keys_out,
                          uint64_t* counts_out, int64_t capacity, int64_t* n_out, int64_t* xcells_out,
                          int64_t xcapacity, int64_t* nx_out)
{
    int st = reset_state(ctx);
    if (st) return st;
    int64_t *row = nullptr, *col = nullptr, *idx = nullptr;
    if (rows) {
        uint32_t* grp;
        ENSURE(B_X_ROW, (uint64_t)n * 8 + 8, row);
        ENSURE(B_X_COL, (uint64_t)n * 8 + 8, col);
        ENSURE(B_X_IDX, (uint64_t)n * 8 + 8, idx);
        ENSURE(B_GL_GRP, (uint64_t)n * 4 + 4, grp);
        hm_launch_tiles_list(ctx->stream, rows, cols, keep, nullptr, n, row, col, grp, idx, ctx->state + ST_XCOUNT);
        HIPCHK(hipGetLastError());
        if ((st = read_state(ctx))) return st;
        if ((st = take_error(ctx))) return st;
    }
    HmGenEmit e;
    memset(&e, 0, sizeof(e));
    e.cells = xcells_out;
    e.capacity = (uint64_t)xcapacity;
    e.width = 4;
    e.split = 1;
    e.keys = keys_out;
    e.counts = counts_out;
    e.kcapacity = (uint64_t)capacity;
    e.kcursor = ctx->state + ST_CURSOR;
    e.xcursor = ctx->state + ST_XCURSOR;
    uint64_t total = 0;
    if (rows)
        st = gen_count(ctx, row, col, nullptr, idx, ctx->host_state[ST_XCOUNT], zmax, zmin, e, &total);
    else   /* points projected straight into keys */
        st = gen_count(ctx, nullptr, nullptr, nullptr, nullptr, (uint64_t)n, zmax, zmin, e, &total, lat, lon, keep);
    if (st) return st;
    if ((st = read_state(ctx))) return st;
    *n_out = (int64_t)ctx->host_state[ST_CURSOR];
    *nx_out = (int64_t)ctx->host_state[ST_XCURSOR];
    ctx->last_slow = 0;
    ctx->last_levels = 0;
    for (int i = 0; i < 9; i++) ctx->stage_us[i] = 0;
    return (*n_out > capacity || *nx_out > xcapacity) ? HM_E_CAPACITY : HM_OK;
}

/* Level plan for dense, evenly spread clouds (uniform-like). With 6 zooms
 * per level, each level-2 work item (HM_TN keys) of such a cloud scatters
 * over ~3400 of its 4^6 digits: runs of one or two keys, each a run-slot
 * atomic, a run record and a scan entry (1e9 uniform points: 24 ms of
 * level-2 partitioning). Levels of 3 zooms (64 digits) keep the runs long
 * at the price of one more pass over the keys (1e9 uniform points: 68 -> 48
 * ms per count; the same plan costs hotspot clouds 60%, so it is chosen only
 * when level 1's sampled histogram is flat -- no digit above 4x the mean --
 * and the mean level-1 bucket holds >= HM_SPREAD_MIN_KEYS keys; the
 * environment variable of that name overrides the threshold). */
static void spread_replan(const uint32_t* h, int F, double npts, int zb, int* zs, int* L, double min_keys,
                          bool flat)
{
    uint64_t tot = 0, mx = 0;
    int ne = 0;
    for (int i = 0; i < F; i++) {
        tot += h[i];
        mx = std::max<uint64_t>(mx, h[i]);
        ne += h[i] != 0;
    }
    if (ne == 0 || npts < min_keys * ne || (flat && (double)mx * ne > 4.0 * (double)tot)) return;
    int step = HM_SPREAD_ZOOMS;
    while (zs[0] + step * (HM_MAX_LEVELS - 1) < zb) step++;
    if (step >= HM_LEVEL_ZOOMS) return;
    int l = 1, z = zs[0];
    while (z < zb) {
        z = std::min(z + step, zb);
        zs[l++] = z;
    }
    *L = l;
}

/* ------------------------------------------------------------------------ */
/* the count pipeline's host driver.  One CountCall per attempt of hm_count / */
/* hm_count_tiles; run() is the driver: plan, level 1, levels 2..L,           */
/* aggregate, pool, finish.  The phases return the status code.               */
/* ------------------------------------------------------------------------ */
namespace {

/* What level l hands to level l + 1 (the last level: to the aggregation).
 * Beside it the next level reads only B[l] and lv[l].items, and the hot-tile
 * state below. */
struct LevelOut {
    void* keys = nullptr;                          /* the level's output keys: u32, u16 from the last level */
    int slot_k = 0;                                /* ping-pong A/B: which of B_KEYS_*, B_FLAT_*, B_EXCL_* the
                                                    * next level writes (the other holds keys and runs) */
    HmRuns runs = {nullptr, nullptr};              /* flat child-ordered runs and their key prefix */
    const uint32_t* parent_item_begin = nullptr;   /* B_l's work-item prefix */
    const uint64_t* parent_coord = nullptr;        /* B_l's tiles */
    uint32_t nparents = 1;                         /* |B_l| (the root below level 1) */
    uint64_t level_keys = 0;                       /* keys entering level l + 1 (global positions) */
    uint32_t* seg = nullptr;                       /* B_l's items' run tables (k_partition_fr): level 1's when
                                                    * L > 1, a child-contiguous level's, else null */
};

/* level 1's kernel arguments and sizes, shared by its pieces */
struct Level1Work {
    HmPart1Args a;                   /* holds fill, l1slot and redo_idx */
    uint32_t *rbase, *rcap;          /* the regions' bases and sizes */
    uint8_t* smask;
    HmL1Args ba;                     /* k_level1_buckets */
    int F;                           /* digits of the level */
    uint32_t* hist;                  /* sampled digit histogram */
    int64_t *redo_rows, *redo_cols;  /* the deferred points, resolved (lat/lon input) */
    uint64_t stride;                 /* points per sample */
    uint64_t total_cap;              /* key positions of the regions */
    void* kout;
};

/* one level >= 2: what level_begin chooses and the buffers its pieces share */
struct LevelWork {
    int restbits;
    bool contig;          /* child-contiguous level (HM_PN_CONTIG) */
    bool hot3;            /* hot tiles in a 3-level plan, joining at the last level */
    int sb;               /* run-counter shard bits */
    uint64_t l1_total;    /* where level 1's key positions end */
    void* kout;
    uint2* runs_sh;
    uint32_t* nruns;
    uint32_t* rs_big;
    HmRsArgs ra;          /* the run scan's arrays (compact reads nr, runbase, nkeys, keybase, vals) */
    uint64_t* prefix;
};

struct CountCall {
    /* ---- arguments ---- */
    hm_ctx* ctx;
    const double* lat;
    const double* lon;
    const int64_t* rows;
    const int64_t* cols;
    const uint8_t* keep;
    int64_t n;
    int zmin, Z;
    uint64_t* keys_out;
    uint64_t* counts_out;
    int64_t capacity;
    int64_t* n_out;
    int64_t* xcells_out;
    int64_t xcapacity;
    int64_t* nx_out;

    /* ---- the plan (plan(); L and zs[1..] revised once, at the end of level 1) ---- */
    hipStream_t s = nullptr;
    int zb = 0;                 /* bucket zoom of the last level */
    int zs[HM_MAX_LEVELS];      /* child zoom of each level */
    int L = 0;
    uint32_t ta = HM_TA;        /* keys per aggregation work item */
    bool timing = false;        /* stage events recorded */
    uint32_t tiles_in = 0;      /* HM_T1-point input tiles */
    bool from_tiles = false;    /* hm_count_tiles */
    uint64_t redo_cap = 0;      /* capacity of k_redo's list */
    bool spread = false;        /* levels 2.. take fewer zooms (spread_replan) */

    /* ---- level l -> level l + 1 ---- */
    LevelOut hand;

    /* ---- hot tiles ---- */
    bool hot_on = false;        /* hot tiles sampled and looked up by level 1 */
    bool hot_mid = false;       /* ... at zs[1] of a 3-level plan (they skip level 2 only) */
    int hz = 0;                 /* zoom of the hot tiles: the bucket zoom of level 2 */
    uint32_t nhot = 0;          /* hot tiles found */
    uint64_t l2_elems = 0;      /* mid-level hot tiles: level 2's key array (elements) */
    HmHotRunArgs hr = {};       /* hot tiles as level-2 children */

    /* ---- what aggregate(), pool() and finish() read ---- */
    Level lv[HM_MAX_LEVELS];
    HmBuckets B[HM_MAX_LEVELS] = {};
    unsigned long long* totals[HM_MAX_LEVELS + 1];
    uint32_t nslots = 0;        /* the last level's multi-item buckets (merge slots) */
    int32_t* slots = nullptr;
    uint32_t* slot_bucket = nullptr;
    HmExotic xl = {};           /* kept points outside [0, 2^Z)^2 */
    uint64_t nx = 0;            /* ... their number */
    HmOut o;

    /* ---- hm_last_stats ---- */
    int l1_reruns = 0;          /* level-1 re-runs after a region overflow */
    int npart = 0;              /* level >= 2 partition launches timed (ev[5..]) */
    int nev = 0;                /* stage-boundary events recorded (ev[0..4]) */

    /* digit slots: F cold digits, hot tile h at HM_MAX_F1 + h */
    static constexpr int FS = HM_D1 * HM_L1_SHARDS;
    /* a level's totals (runs, keys, count << 32 | items): they come back with the state */
    uint64_t* ltot() const { return (uint64_t*)(ctx->state + ST_LTOT); }

    int run();
    int plan();
    int begin_level(int l);
    int bucket_arrays(int l, uint64_t cap, HmCompactOut& out);
    int publish(int l, const HmCompactOut& out, HmRuns runs, void* keys, uint64_t level_keys, int seg_slot);
    int level1();
    int level1_setup(Level1Work& w);
    int level1_size(Level1Work& w);
    int level1_bucket_args(Level1Work& w);
    int level1_resize(Level1Work& w);
    int level1_redo(Level1Work& w);
    int level1_buckets(Level1Work& w);
    int level1_run(Level1Work& w);
    int level1_finish(Level1Work& w);
    int level(int l);
    int level_begin(int l, LevelWork& w);
    int level_partition(int l, LevelWork& w);
    int level_runscan(int l, LevelWork& w);
    int level_compact(int l, LevelWork& w);
    int aggregate();
    int pool();
    int finish();
};

int CountCall::run()
{
    int st;
    if ((st = plan())) return st;
    if ((st = level1())) return st;
    for (int l = 1; l < L; l++)
        if ((st = level(l))) return st;
    if (timing) HIPCHK(hipEventRecord(ctx->ev[nev], s));
    nev++;
    if ((st = aggregate())) return st;
    if (timing) HIPCHK(hipEventRecord(ctx->ev[nev], s));
    nev++;
    if ((st = pool())) return st;
    if (timing) HIPCHK(hipEventRecord(ctx->ev[nev], s));
    nev++;
    return finish();
}

int CountCall::plan()
{
    if (!ctx || !n_out || !nx_out || n < 0 || n >= (int64_t)0xFFFFFFF0ll || zmin < 0 || Z < zmin ||
        Z > HM_COUNT_MAX_ZOOM || capacity < 0 || (capacity > 0 && (!keys_out || !counts_out)) || xcapacity < 0 ||
        (xcapacity > 0 && !xcells_out))
        return HM_E_ARG;
    *n_out = 0;
    *nx_out = 0;
    /* set again only when THIS attempt re-keys a stream's tail (an attempt
     * that fails after it, then count_fallback, leaves the keys un-keyed) */
    ctx->tail_done = 0;
    HIPCHK(hipSetDevice(ctx->device));
    s = ctx->stream;
    zb = Z > HM_AG_LG ? Z - HM_AG_LG : 0;
    hz = zb;
    {
        int z = zb < HM_Z1 ? zb : HM_Z1;
        zs[L++] = z;
        while (z < zb) {
            z = std::min(z + HM_LEVEL_ZOOMS, zb);
            if (L >= HM_MAX_LEVELS) return HM_E_ARG;
            zs[L++] = z;
        }
    }
    /* key bits after level l: 2*(Z - zs[l]); must fit u32 (level 1 output) */
    if (2 * (Z - zs[0]) > 32) return HM_E_ARG;
    /* stage timings (hm_last_stats) for calls of >= 2^24 points: each event
     * record is an API call, and small calls (stream batches) are bound by
     * the host's issue rate */
    timing = n >= (1ll << 24) && ctx->stage_timing;
    /* keys per aggregation work item: HM_TA, halved (down to HM_TA_MIN, 16K)
     * until the call has >= HM_TA_ITEMS (128) items' worth of points -- a
     * 1e7-point call otherwise runs ~40 items on 256 CUs */
    while (ta > ctx->ta_min && (uint64_t)n < (uint64_t)ta * ctx->ta_items) ta >>= 1;
    for (int i = 0; i < 9; i++) ctx->stage_us[i] = 0;
    ctx->stage_us[8] = (double)ta;          /* hm_last_stats: keys per aggregation work item */
    ctx->last_levels = L;

    /* level 1 reads the input in HM_T1-point tiles; points the fast path
     * defers (lat/lon input only) go to k_redo, at most redo_cap of them */
    tiles_in = (uint32_t)((n + HM_T1 - 1) / HM_T1);
    from_tiles = rows != nullptr;
    redo_cap = from_tiles ? 0 : std::max<uint64_t>(1u << 20, (uint64_t)n / 256);
    if (redo_cap > (uint64_t)n) redo_cap = (uint64_t)n;
    /* exotic list: first capacity like the redo list's; rebuilt if it overflows */
    xl.cap = std::min<uint64_t>((uint64_t)n, std::max<uint64_t>(1u << 20, (uint64_t)n / 256));
    ENSURE(B_X_ROW, xl.cap * 8 + 8, xl.row);
    ENSURE(B_X_COL, xl.cap * 8 + 8, xl.col);
    ENSURE(B_X_IDX, xl.cap * 8 + 8, xl.idx);
    xl.count = ctx->state + ST_XCOUNT;
    return HM_OK;
}

/* level l's descriptor, from the plan as it stands (level 1: before the
 * replan; levels >= 2: after it) and the buckets the level below published */
int CountCall::begin_level(int l)
{
    Level& V = lv[l];
    V.zc = zs[l];
    V.dbits = 2 * (zs[l] - (l ? zs[l - 1] : 0));
    V.nparents = hand.nparents;
    V.nchildren = (uint64_t)hand.nparents << V.dbits;
    V.out16 = (l == L - 1);
    if (V.nchildren > (uint64_t)HM_SCAN_LIMIT) return HM_FALLBACK;
    return HM_OK;
}

/* level l's seven bucket arrays (B_l), cap entries each */
int CountCall::bucket_arrays(int l, uint64_t cap, HmCompactOut& out)
{
    ENSURE(B_BK0 + l * 8 + 0, cap * 4, out.nkeys);
    ENSURE(B_BK0 + l * 8 + 1, cap * 4, out.nruns);
    ENSURE(B_BK0 + l * 8 + 2, cap * 4, out.rbase);
    ENSURE(B_BK0 + l * 8 + 3, cap * 4, out.item_begin);
    ENSURE(B_BK0 + l * 8 + 4, cap * 4, out.digit);
    ENSURE(B_BK0 + l * 8 + 5, cap * 8, out.coord);
    ENSURE(B_BK0 + l * 8 + 6, cap * 4, out.keybase);
    return HM_OK;
}

/* B_l from the level's bucket arrays and its read-back count, the work items
 * of the next stage (k_items), and the hand-off to it.  seg_slot: the arena
 * slot of the items' run tables (B_SEG, B_SEG2), or -1 for none */
int CountCall::publish(int l, const HmCompactOut& out, HmRuns runs, void* keys, uint64_t level_keys, int seg_slot)
{
    const Level& V = lv[l];
    const bool last = l == L - 1;
    HmBuckets& b = B[l];
    b.count = V.count;
    b.nkeys = out.nkeys;
    b.nruns = out.nruns;
    b.rbase = out.rbase;
    b.keybase = out.keybase;
    b.item_begin = out.item_begin;
    b.digit = out.digit;
    b.coord = out.coord;
    b.slots = last ? slots : nullptr;
    uint4* desc;
    ENSURE(B_DESC0 + l, ((uint64_t)V.items + 1) * 2 * sizeof(uint4), desc);
    b.desc = desc;
    hand.seg = nullptr;
    if (seg_slot >= 0) ENSURE(seg_slot, ((uint64_t)V.items + 1) * 16 * sizeof(uint32_t), hand.seg);
    hm_launch_items(s, b, runs, V.items, last ? ta : HM_TN, desc, hand.seg);
    HIPCHK(hipGetLastError());
    hand.keys = keys;
    hand.runs = runs;
    hand.parent_item_begin = out.item_begin;
    hand.parent_coord = out.coord;
    hand.nparents = V.count;
    hand.level_keys = level_keys;
    hand.slot_k ^= 1;
    return HM_OK;
}

/* ---- level 1: projection + partition into per-digit regions ---- */
int CountCall::level1()
{
    int st;
    if ((st = begin_level(0))) return st;
    Level1Work w;
    if ((st = level1_setup(w))) return st;
    if ((st = level1_size(w))) return st;
    if ((st = level1_bucket_args(w))) return st;
    if ((st = level1_run(w))) return st;
    return level1_finish(w);
}

/* level 1's buffers, the call's one fill dispatch, the sample pass and the
 * hot-tile selection */
int CountCall::level1_setup(Level1Work& w)
{
    const Level& V = lv[0];
    /* the call's state words and level 1's zeroed buffers: one fill dispatch,
     * launched before level 1's sampling */
    HmFill f1;
    memset(&f1, 0, sizeof(f1));
    hm_fill_add(f1, ctx->state + 1, 0, (ST_COUNT - 1) * sizeof(unsigned long long));
    hm_fill_add(f1, ctx->state + ST_ERR, 0xFF, sizeof(unsigned long long));
    static_assert(ST_ERR == 0, "error word first");
    w.F = 1 << V.dbits;
    uint32_t* fill;
    ENSURE(B_L1_FILL, FS * 4, fill);
    ENSURE(B_L1_RBASE, FS * 4, w.rbase);
    ENSURE(B_L1_RCAP, FS * 4, w.rcap);
    ENSURE(B_L1_HIST, HM_D1 * 4, w.hist);
    ENSURE(B_L1_SMASK, HM_D1, w.smask);
    uint32_t* const hist = w.hist;
    uint4* l1slot = nullptr;   /* k_l1_fast's slot table (lat/lon input) */
    if (!from_tiles) ENSURE(B_L1_SLOT, (size_t)FS * sizeof(uint4), l1slot);
    /* hot tiles are level-2 buckets: zoom zs[1], a dense sample
     * histogram of <= 4^11 tiles.  In the two-level plan (level 1 at
     * z1, the last at zb) they skip every partition after level 1; in
     * a three-level plan (zmax 19-21: z5 -> z11 -> zb) they skip level 2
     * and join level 3 with the level-2 buckets (HM_HOT_MID) */
    hot_mid = ctx->hot && ctx->hot_mid && L == 3 && zs[1] <= 11 && zs[0] == HM_Z1 && n > 0 && V.dbits == 2 * HM_Z1;
    hot_on = hot_mid || (ctx->hot && L == 2 && zb <= 11 && zs[0] == HM_Z1 && n > 0 && V.dbits == 2 * HM_Z1);
    hz = hot_mid ? zs[1] : zb;
    uint32_t* redo_idx = nullptr;
    w.redo_rows = w.redo_cols = nullptr;
    if (!from_tiles) {
        ENSURE(B_REDO_IDX, redo_cap * sizeof(uint32_t), redo_idx);
        ENSURE(B_REDO_ROWS, redo_cap * sizeof(int64_t), w.redo_rows);
        ENSURE(B_REDO_COLS, redo_cap * sizeof(int64_t), w.redo_cols);
    }
    HmPart1Args& a = w.a;
    memset(&a, 0, sizeof(a));
    a.lat = lat;
    a.lon = lon;
    a.rows_in = rows;
    a.cols_in = cols;
    a.keep = keep;
    a.n = n;
    a.Z = Z;
    a.dbits = V.dbits;
    a.restbits = 2 * (Z - zs[0]);
    a.fill = fill;
    a.rbase = w.rbase;
    a.rcap = w.rcap;
    a.smask = w.smask;
    a.l1slot = l1slot;
    a.overflow = ctx->state + ST_OVERFLOW;
    a.err_word = ctx->state + ST_ERR;
    a.x = xl;
    a.slow_count = ctx->state + ST_SLOW;
    a.redo_idx = redo_idx;
    a.redo_count = ctx->state + ST_REDO;
    a.redo_cap = redo_cap;
    /* region sizes: a sampled digit histogram with a generous margin */
    /* ~256K samples (1M samples above 2^28 points took 90 us per 1e9-point
     * count; the regions' 8-sigma margins scale with sqrt(stride)) */
    /* (2^16 samples below 2^24 points, where the sample pass's ~30 us
     * is a batch's cost; the regions' slack scales with the stride) */
    const int slog = n < (1ll << 24) ? std::min(ctx->sample_log2, 16) : ctx->sample_log2;
    const uint64_t stride = w.stride = std::max<uint64_t>(1, (uint64_t)n >> slog);
    hm_fill_add(f1, hist, 0, HM_D1 * 4);
    hm_fill_add(f1, fill, 0, FS * 4);
    uint32_t* hot_counts = nullptr;
    uint32_t* hot_tiles = nullptr;
    uint32_t* hot_hash = nullptr;
    uint8_t* hot_parent = nullptr;
    uint32_t* hot_n = (uint32_t*)(ctx->state + ST_NHOT);
    if (hot_on) {
        ENSURE(B_HOT_COUNTS, (4ull << (2 * hz)), hot_counts);
        ENSURE(B_HOT, (HM_MAX_HOT + HM_HOT_SLOTS + 2 * HM_HOT_CAND + 1) * 4, hot_tiles);
        ENSURE(B_HOT_PARENT, HM_MAX_F1, hot_parent);
        hot_hash = hot_tiles + HM_MAX_HOT;
        hm_fill_add(f1, hot_counts, 0, 4ull << (2 * hz));
        hm_fill_add(f1, hot_hash + HM_HOT_SLOTS + 2 * HM_HOT_CAND, 0, 4);   /* candidates */
        hm_fill_add(f1, hot_parent, 0, HM_MAX_F1);
        a.hot_z = hz;
        a.hot_bytes = hot_mid ? 4 : 2;
        a.hot_hash = hot_hash;
        a.hot_n = hot_n;
    } else {
        a.hot_z = -1;
    }
    hm_launch_fill(s, f1);
    if (n > 0) hm_launch_sample_digits(s, a, stride, hist, hot_counts);
    HIPCHK(hipGetLastError());
    if (hot_on) {
        hr.tiles = hot_tiles;
        hr.n = hot_n;
        hr.zb = hz;
        hr.z1 = zs[0];
        hr.fill = fill;
        hr.rbase = w.rbase;
        HmHotArgs ha;
        ha.counts = hot_counts;
        ha.zb = hz;
        ha.z1 = zs[0];
        const uint64_t m = ((uint64_t)n + stride - 1) / stride;
        ha.thresh = (uint32_t)std::max<double>(
            {1.0, ceil((double)m / ctx->hot_inv_share), ceil(ctx->hot_min_keys / (double)stride)});
        ha.tiles = hot_tiles;
        ha.hist = hist;
        ha.hotparent = hot_parent;
        ha.n = hot_n;
        ha.hash = hot_hash;
        ha.cand = hot_hash + HM_HOT_SLOTS;
        hm_launch_hot_select(s, ha);
        HIPCHK(hipGetLastError());
    }
    return HM_OK;
}

/* the regions' sizes (on the device) and the host's bound of their total,
 * which sizes the key buffer: w.total_cap */
int CountCall::level1_size(Level1Work& w)
{
    const HmPart1Args& a = w.a;
    const int F = w.F;
    const uint64_t stride = w.stride;
    int st;
    /* the region sizes are computed on the device (k_l1_sizes); the key
     * buffer takes the host's bound of their total: est sums to at
     * most nn (a hot tile's samples leave its cold digit), at most M
     * (digit, shard) entries are non-empty, and sum sqrt(e stride) <=
     * sqrt(M nn stride) (Cauchy-Schwarz) */
    const double nn = (double)n + (double)(F + (hot_on ? HM_MAX_HOT : 0)) * (double)stride;
    const double M = F + std::min((double)F, nn / ((double)HM_L1_SHARD_TILES * HM_T1)) * (HM_L1_SHARDS - 1) +
                     (hot_on ? (double)HM_MAX_HOT * HM_L1_SHARDS : 0.0);
    double bound = nn * 17.0 / 16.0 + 8.0 * sqrt(M * nn * (double)stride) + M * 2.0 * HM_T1 +
                   (double)(F + (hot_on ? HM_MAX_HOT : 0)) * HM_L1_ZERO_SAMPLES * (double)stride + 1024.0;
    hm_launch_l1_sizes(s, w.hist, F, hot_on ? (uint32_t*)(ctx->state + ST_NHOT) : nullptr, stride, w.rcap, w.rbase,
                       w.smask, ctx->state + ST_L1TOTAL);
    if (a.l1slot) hm_launch_l1_slots(s, a);
    HIPCHK(hipGetLastError());
    if (bound >= (double)0xFFF00000ull) {
        /* the bound passes the u32 key positions (n above ~1.5e9):
         * read the exact total of the sized regions instead */
        if ((st = read_state(ctx))) return st;
        bound = (double)ctx->host_state[ST_L1TOTAL] + 1024.0;
        if (bound >= (double)0xFFF00000ull) return HM_FALLBACK;   /* key positions are u32 */
    }
    w.total_cap = (uint64_t)bound;
    return HM_OK;
}

/* the non-empty digits are the level's buckets, one run each */
int CountCall::level1_bucket_args(Level1Work& w)
{
    const Level& V = lv[0];
    HmL1Args& ba = w.ba;
    int st;
    memset(&ba, 0, sizeof(ba));
    const uint64_t cap = (uint64_t)w.F + 1;
    if ((st = bucket_arrays(0, cap, ba.out))) return st;
    ENSURE(B_FLAT_A, (uint64_t)FS * sizeof(uint2) + 8, ba.runs);
    ENSURE(B_EXCL_A, (uint64_t)FS * sizeof(uint64_t) + 8, ba.excl);
    ENSURE(B_CHILD0, 2 * 4, ba.child_begin);
    ba.F = w.F;
    ba.dbits = V.dbits;
    ba.fill = w.a.fill;
    ba.rbase = w.rbase;
    ba.smask = w.smask;
    ba.item_keys = (L == 1) ? ta : HM_TN;
    ba.sparse_max = (L == 1) ? HM_SP_MAX : 0u;
    ba.total = ltot();
    if (hot_on) {   /* hot parents all zero when no tile turned out hot */
        uint32_t* d2b;
        ENSURE(B_D2B, HM_MAX_F1 * 4, d2b);
        ba.hotparent = hr.tiles ? (const uint8_t*)ctx->bufs[B_HOT_PARENT].p : nullptr;
        ba.d2b = d2b;
        hr.d2b = d2b;
    }
    if (L == 1) {
        ENSURE(B_SLOTS, cap * 4, slots);
        ENSURE(B_SLOTBKT, cap * 4, slot_bucket);
        ba.slots = slots;
        ba.nslots = ctx->state + ST_NSLOTS;
        ba.slot_bucket = slot_bucket;
    }
    return HM_OK;
}

/* a region overflowed: fill[] now holds the exact sizes (the shard of every
 * tile is fixed by its block id); read them back (one host wait) and lay the
 * regions out again */
int CountCall::level1_resize(Level1Work& w)
{
    const HmPart1Args& a = w.a;
    /* pinned host scratch: caps [FS] | bases [FS] */
    uint32_t* hc = ctx->host_aux + HM_D1;
    uint32_t* hb = hc + HM_D1 * HM_L1_SHARDS;
    l1_reruns++;
    HIPCHK(hipMemcpyAsync(hc, a.fill, FS * 4, hipMemcpyDeviceToHost, s));
    if (ctx->debug_l1) HIPCHK(hipMemcpyAsync(hb, w.rcap, FS * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hm_sync(s));
    if (ctx->debug_l1) {
        /* HM_DEBUG_L1=1: the overflowing regions, and the sample behind them */
        for (int i = 0; i < FS; i++)
            if (hc[i] > hb[i])
                fprintf(stderr, "hm l1 overflow: digit %d shard %d fill %u cap %u hist %u stride %llu\n", i % HM_D1,
                        i / HM_D1, hc[i], hb[i], ctx->host_aux[i % HM_D1], (unsigned long long)w.stride);
    }
    for (int i = 0; i < FS; i++) hc[i] += 64;
    /* a digit's shards stay consecutive: its keys' logical
     * positions are one range (k_level1_buckets) */
    w.total_cap = 0;
    for (int d = 0; d < HM_D1; d++)
        for (int sh = 0; sh < HM_L1_SHARDS; sh++) {
            hb[hm_l1i(d, sh)] = (uint32_t)w.total_cap;
            w.total_cap += hc[hm_l1i(d, sh)];
        }
    if (w.total_cap >= 0xFFF00000ull) return HM_FALLBACK;
    HIPCHK(hipMemcpyAsync(w.rcap, hc, FS * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w.rbase, hb, FS * 4, hipMemcpyHostToDevice, s));
    if (a.l1slot) hm_launch_l1_slots(s, a);   /* the table holds the regions' bases and sizes */
    return HM_OK;
}

/* lat/lon input: the points the fast path deferred, resolved exactly (k_redo)
 * and partitioned as tile input */
int CountCall::level1_redo(Level1Work& w)
{
    HmRedoArgs ra;
    ra.lat = lat;
    ra.lon = lon;
    ra.keep = keep;
    ra.Z = Z;
    ra.redo_idx = w.a.redo_idx;
    ra.redo_count = ctx->state + ST_REDO;
    ra.rows_out = w.redo_rows;
    ra.cols_out = w.redo_cols;
    ra.out_count = ctx->state + ST_REDO_OUT;
    ra.err_word = ctx->state + ST_ERR;
    ra.x = xl;
    ra.cap = redo_cap;
    hm_launch_redo(s, ra, redo_cap);
    HIPCHK(hipGetLastError());
    /* the deferred points, resolved exactly, as tile input; the
     * launch covers the list's capacity and reads its length
     * on the device (no host round trip) */
    HmPart1Args b = w.a;
    b.lat = nullptr;
    b.lon = nullptr;
    b.rows_in = w.redo_rows;
    b.cols_in = w.redo_cols;
    b.keep = nullptr;
    b.n = (int64_t)redo_cap;
    b.n_dev = ctx->state + ST_REDO_OUT;
    hm_launch_part1(s, b, (uint32_t)((redo_cap + HM_T1 - 1) / HM_T1), lv[0].out16, 1);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

/* the level's buckets from the filled regions, launched before the one host
 * sync of level 1 (its results are used only if the level turns out clean:
 * no error, no redo or region overflow) */
int CountCall::level1_buckets(Level1Work& w)
{
    hm_launch_level1_buckets(s, w.ba);
    HIPCHK(hipGetLastError());
    if (L > 1) HIPCHK(hipMemcpyAsync(ctx->host_aux, w.hist, w.F * 4, hipMemcpyDeviceToHost, s));
    return read_state(ctx);
}

/* the attempts: the partition, its buckets and the level's one host sync;
 * again with the exact chain fused in if the redo list overflowed, and once
 * more from the top, with exact region sizes, if a region did */
int CountCall::level1_run(Level1Work& w)
{
    const Level& V = lv[0];
    HmPart1Args& a = w.a;
    int st;
    for (int attempt = 0;; attempt++) {
        ENSURE(hand.slot_k ? B_KEYS_B : B_KEYS_A, (w.total_cap + 8) * (V.out16 ? 2 : 4), w.kout);
        a.keys_out = w.kout;
        if (hot_on) {
            /* hot keys: straight into level 2's output key array (level 2
             * writes the cold keys' positions of it): u16 when that is the
             * last level's, u32 for mid-level hot tiles -- whose array
             * also holds the child-contiguous cold keys above every
             * level-1 position (l2_elems) */
            void* kh = nullptr;
            if (hot_mid) l2_elems = w.total_cap + (uint64_t)n + 16;
            ENSURE(hand.slot_k ? B_KEYS_A : B_KEYS_B, hot_mid ? l2_elems * 4 : (w.total_cap + 8) * 2, kh);
            a.keys_hot = kh;
        }
        if (attempt > 0) {
            /* (the first attempt's are zero from the call's fill) */
            HIPCHK(hipMemsetAsync(a.fill, 0, FS * 4, s));
            /* ST_XCOUNT .. ST_OVERFLOW (XCOUNT, SLOW, REDO, REDO_OUT, OVERFLOW;
             * CURSOR, NSLOTS, XCURSOR are still 0 here) in one memset */
            static_assert(ST_XCOUNT == 1 && ST_OVERFLOW == 8 && ST_NHOT > ST_OVERFLOW, "level-1 words");
            HIPCHK(hipMemsetAsync(ctx->state + ST_XCOUNT, 0, 8 * 8, s));
        }
        if (timing) HIPCHK(hipEventRecord(ctx->ev[0], s));
        hm_launch_part1(s, a, tiles_in, V.out16, from_tiles ? 1 : 0);
        HIPCHK(hipGetLastError());
        if (timing) HIPCHK(hipEventRecord(ctx->ev[1], s));
        nev = 2;
        if (!from_tiles && (st = level1_redo(w))) return st;
        if ((st = level1_buckets(w))) return st;
        if ((st = take_error(ctx))) return st;
        const uint64_t nredo = ctx->host_state[ST_REDO];
        ctx->last_slow = (int64_t)nredo;
        if (!from_tiles && nredo > redo_cap) {
            /* adversarial input (mostly polar / guard band): redo the
             * level with the exact chain fused into the kernel */
            HIPCHK(hipMemsetAsync(a.fill, 0, FS * 4, s));
            HIPCHK(hipMemsetAsync(ctx->state + ST_OVERFLOW, 0, 8, s));
            HIPCHK(hipMemsetAsync(xl.count, 0, 8, s));
            HIPCHK(hipMemsetAsync(ctx->state + ST_NSLOTS, 0, 8, s));   /* level1_buckets again */
            /* hm_last_stats: the points this run resolves, not those
             * plus the first run's deferred ones (every point twice) */
            HIPCHK(hipMemsetAsync(ctx->state + ST_SLOW, 0, 8, s));
            hm_launch_part1(s, a, tiles_in, V.out16, 2);
            HIPCHK(hipGetLastError());
            if ((st = level1_buckets(w))) return st;
            if ((st = take_error(ctx))) return st;
        }
        if (!ctx->host_state[ST_OVERFLOW]) break;
        if (attempt > 0) return HM_E_HIP;   /* cannot happen: the same points */
        if ((st = level1_resize(w))) return st;
    }
    return HM_OK;
}

/* after the level's sync: the exotic list rebuilt if it overflowed, the hot
 * tiles found, the plan of levels 2.. revised, B_1 and its items published */
int CountCall::level1_finish(Level1Work& w)
{
    Level& V = lv[0];
    const int F = w.F;
    int st;
    nx = ctx->host_state[ST_XCOUNT];
    if (nx > xl.cap) {
        /* more kept out-of-square points than the list held: rebuild it */
        xl.cap = nx;
        ENSURE(B_X_ROW, xl.cap * 8, xl.row);
        ENSURE(B_X_COL, xl.cap * 8, xl.col);
        ENSURE(B_X_IDX, xl.cap * 8, xl.idx);
        HIPCHK(hipMemsetAsync(xl.count, 0, sizeof(unsigned long long), s));
        hm_launch_collect_exotic(s, lat, lon, rows, cols, keep, n, Z, xl);
        HIPCHK(hipGetLastError());
        if ((st = read_state(ctx))) return st;
        nx = ctx->host_state[ST_XCOUNT];
        if (nx > xl.cap) return HM_E_HIP;   /* cannot happen: the same points */
    }
    nhot = hot_on ? (uint32_t)(ctx->host_state[ST_NHOT] & 0xFFFFFFFFull) : 0u;
    if (!nhot) hot_mid = false;
    /* levels 2.. may take the spread plan (the level-1 pass is the
     * same under both: its output is u32 keys whenever L > 1) */
    if (hot_mid) {
        /* the plan stays z5 -> z11 -> zb: the hot tiles are zoom-11 buckets */
    } else if (L > 1 && !nhot) {
        spread_replan(ctx->host_aux, F, (double)n, zb, zs, &L, ctx->spread_min_keys, true);
    } else if (L > 1) {
        /* with hot tiles the rest is the cloud's sparse background: 3
         * zooms per level unless it is tiny (a 6-zoom level scatters
         * each 8192-key item over 4096 children, runs of ~1 key); the
         * hot tiles then join at the last level.  (host_aux holds the
         * cold digits' sampled counts: the hot samples were taken off) */
        double cold = 0;
        for (int i = 0; i < F; i++) cold += ctx->host_aux[i];
        spread_replan(ctx->host_aux, F, cold * (double)w.stride, zb, zs, &L, ctx->spread_min_cold, false);
    }
    spread = L > 2 && zs[1] - zs[0] < HM_LEVEL_ZOOMS;
    ctx->last_levels = L;
    V.count = (uint32_t)(ctx->host_state[ST_LTOT] >> 32);
    V.items = (uint32_t)(ctx->host_state[ST_LTOT] & 0xFFFFFFFFull);
    if (L == 1) nslots = (uint32_t)(ctx->host_state[ST_NSLOTS] & 0xFFFFFFFFull);
    return publish(0, w.ba.out, HmRuns{w.ba.runs, w.ba.excl}, w.kout, w.total_cap, L > 1 ? B_SEG : -1);
}

/* ---- levels >= 2 (l: the level's index, level 2 is l = 1) ---- */
int CountCall::level(int l)
{
    int st;
    if ((st = begin_level(l))) return st;
    LevelWork w;
    if ((st = level_begin(l, w))) return st;
    if ((st = level_partition(l, w))) return st;
    if ((st = level_runscan(l, w))) return st;
    return level_compact(l, w);
}

/* the level's choices (shard bits, child-contiguous or not, key slot), the
 * partition's output buffers and the level's zeroed counters */
int CountCall::level_begin(int l, LevelWork& w)
{
    const Level& V = lv[l];
    w.restbits = 2 * (Z - zs[l]);
    const uint64_t ntiles = lv[l - 1].items;
    /* run-counter shards: up to 32 (a hot child takes one returning atomic
     * per parent work item; one counter per child made k_partition 16%
     * slower), fewer when the dense child space is large; <= 2^25 */
    /* with hot tiles (their children skip this level) or the spread plan,
     * no child is hot: one counter per child, and the partition kernels'
     * run-slot atomics coalesce (lanes own consecutive digits) */
    /* a child-contiguous level (HM_PN_CONTIG): the middle level of a
     * 3-level plan without hot tiles (Z >= 19) writes each child's keys
     * as ONE run, so the last level reads every item from <= 8 runs
     * (k_partition_fr) instead of streaming runs of a few keys each */
    /* (with mid-level hot tiles the cold keys go above every level-1
     * position, where the hot tiles' keys are: cbase_off) */
    /* level 1's positions end at its regions' total capacity (k_l1_sizes),
     * or, after an overflow re-run, at the exact sizes' total (level_keys) */
    w.l1_total = l1_reruns ? hand.level_keys : ctx->host_state[ST_L1TOTAL];
    w.contig = ctx->contig && l == 1 && L == 3 && (!nhot || hot_mid) && !V.out16 && hand.seg != nullptr &&
               (!hot_mid || w.l1_total + (uint64_t)n < 0xFFF00000ull);
    int sb = ctx->run_shard_bits >= 0 ? ctx->run_shard_bits : ((nhot || spread) ? 0 : HM_RUN_SHARD_BITS);
    if (w.contig) sb = 0;
    while (sb > 0 && (V.nchildren << sb) > (1ull << 25)) sb--;
    w.sb = sb;
    const uint64_t run_cap = (ntiles + ((uint64_t)hand.nparents << sb)) << V.dbits;
    if (run_cap >= (1ull << 32)) return HM_E_NOMEM;

    /* outputs of the level's partition kernel: keys at the item's global
     * positions, and sharded runs */
    const uint64_t nkeys_out = hand.level_keys;
    /* with hot tiles the last level's keys go where level 1 put the hot
     * tiles' (B); a 3-level plan's middle level then takes a third array */
    w.hot3 = nhot && L == 3 && !hot_mid;
    const int kslot = w.hot3 ? (l == 1 ? B_KEYS_C : B_KEYS_B) : (hand.slot_k ? B_KEYS_B : B_KEYS_A);
    ENSURE(kslot, std::max<uint64_t>(nkeys_out + 8, (hot_mid && l == 1) ? l2_elems : 0) * (V.out16 ? 2 : 4), w.kout);
    ENSURE(B_RUNS_SH, run_cap * sizeof(uint2), w.runs_sh);
    ENSURE(B_NRUNS, (V.nchildren << sb) * sizeof(uint32_t), w.nruns);
    ENSURE(B_RS_BIG, (HM_RS_BIG_MAX + 1) * sizeof(uint32_t), w.rs_big);
    /* the level's zeroed counters in one launch */
    HmFill zf;
    zf.k = 0;
    hm_fill_add(zf, w.nruns, 0, (V.nchildren << sb) * sizeof(uint32_t));
    hm_fill_add(zf, w.rs_big + HM_RS_BIG_MAX, 0, sizeof(uint32_t));   /* the run scan's big-child count */
    hm_launch_fill(s, zf);
    return HM_OK;
}

/* the partition of B_{l-1}'s keys by the level's digit; a child-contiguous
 * level first takes the child totals and their scan */
int CountCall::level_partition(int l, LevelWork& w)
{
    const Level& V = lv[l];
    HmPartNArgs a;
    memset(&a, 0, sizeof(a));
    a.parent = B[l - 1];
    a.keys_in = (const uint32_t*)hand.keys;
    a.in = hand.runs;
    a.dbits = V.dbits;
    a.restbits = w.restbits;
    a.shard_bits = w.sb;
    a.keys_out = w.kout;
    a.nruns_out = w.nruns;
    a.runs_out = w.runs_sh;
    a.items = lv[l - 1].items;
    a.seg = hand.seg;
    if (timing) HIPCHK(hipEventRecord(ctx->ev[5 + 2 * (l - 1)], s));
    if (w.contig) {
        /* child totals, their scan, then the partition proper */
        uint64_t *ptl, *ttl;
        ENSURE(B_PARTIAL, 4096 * sizeof(uint64_t), ptl);
        ENSURE(B_TOTAL, 4 * sizeof(uint64_t), ttl);
        ENSURE(B_CTOT, V.nchildren * 8, a.ctot);
        ENSURE(B_CBASE, V.nchildren * 8, a.cbase);
        ENSURE(B_CCUR, V.nchildren * 4, a.ccur);
        HIPCHK(hipMemsetAsync(a.ctot, 0, V.nchildren * 8, s));
        HIPCHK(hipMemsetAsync(a.ccur, 0, V.nchildren * 4, s));
        a.mode = HM_PN_HIST;
        a.cbase_off = hot_mid ? (uint32_t)w.l1_total : 0u;
        hm_launch_partition_hist(s, a);
        hm_launch_scan(s, (const uint64_t*)a.ctot, V.nchildren, ptl, (uint64_t*)a.cbase, ttl + 3);
        a.mode = HM_PN_CONTIG;
    }
    hm_launch_partN(s, a, lv[l - 1].items, V.out16, hand.seg != nullptr);
    HIPCHK(hipGetLastError());
    if (timing) HIPCHK(hipEventRecord(ctx->ev[6 + 2 * (l - 1)], s));
    npart = l;
    return HM_OK;
}

/* run scan: sharded counters -> flat child-ordered runs + key prefix, with
 * the hot tiles hooked in as children of their level */
int CountCall::level_runscan(int l, LevelWork& w)
{
    const Level& V = lv[l];
    HmRsArgs& ra = w.ra;
    memset(&ra, 0, sizeof(ra));
    ra.nchildren = V.nchildren;
    ra.dbits = V.dbits;
    ra.shard_bits = w.sb;
    ra.nruns = w.nruns;
    ra.runs = w.runs_sh;
    ra.parent_item_begin = hand.parent_item_begin;
    ra.item_keys = (l == L - 1) ? ta : HM_TN;
    ra.sparse_max = (l == L - 1) ? HM_SP_MAX : 0u;
    uint64_t *partial, *tot;
    ENSURE(B_SHOFF, (V.nchildren << w.sb) * sizeof(uint32_t), ra.shoff);
    ENSURE(B_NR, V.nchildren * sizeof(uint64_t), ra.nr);
    uint64_t* runbase;
    ENSURE(B_RUNBASE0 + l, V.nchildren * sizeof(uint64_t), runbase);
    ra.runbase = runbase;
    ENSURE(B_PARTIAL, 4096 * sizeof(uint64_t), partial);
    tot = ltot();
    hm_launch_rs_count(s, ra);
    /* hot tiles are children of the last level: of their z5 bucket at
     * level 2, of their zs[1] ancestor (kept as a bucket, below) at level 3 */
    const bool hot_level = nhot && l == (hot_mid ? 1 : L - 1);
    if (hot_level) {
        hr.dbits = V.dbits;
        hr.nr = ra.nr;
        hr.zp = zs[l - 1];
        hr.c2b = (l == 2 && w.hot3) ? (const uint32_t*)ctx->bufs[B_C2B].p : nullptr;
        hm_launch_hot_nr(s, hr);
    }
    /* a 3-level plan with hot tiles: each hot tile's zs[1] ancestor must be
     * a level-2 bucket (its parent at level 3) even without cold keys */
    uint8_t* force = nullptr;
    if (w.hot3 && l == 1) {
        ENSURE(B_HOT_FORCE, V.nchildren, force);
        HIPCHK(hipMemsetAsync(force, 0, V.nchildren, s));
        hr.dbits = V.dbits;
        hr.zp = zs[1];
        hm_launch_hot_force(s, hr, force);
    }
    ra.force = force;
    hm_launch_scan(s, ra.nr, V.nchildren, partial, runbase, tot + 0);
    HIPCHK(hipGetLastError());
    unsigned long long* down = ctx->host_state + 2 * ST_COUNT;
    /* the flat run list is sized by a bound, its length stays on the
     * device (tot[0]): at most one run per (parent item, child) and per
     * key, plus the hot tiles' region shards */
    uint64_t nflat = std::min<uint64_t>(hand.level_keys, (uint64_t)lv[l - 1].items << V.dbits) +
                     (uint64_t)HM_MAX_HOT * HM_L1_SHARDS + 1;
    ra.nflat_dev = tot + 0;
    if (nflat * 24 > (8ull << 30)) {
        /* a bound of more than 8 GiB of run buffers: read the count back */
        HIPCHK(hipMemcpyAsync(down, tot, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hm_sync(s));
        nflat = down[0];
        ra.nflat_dev = nullptr;
    }
    ra.nflat = nflat;
    uint2* flat;
    uint64_t* excl;
    ENSURE(hand.slot_k ? B_FLAT_B : B_FLAT_A, (nflat + 1) * sizeof(uint2), flat);
    ENSURE(hand.slot_k ? B_EXCL_B : B_EXCL_A, (nflat + 1) * sizeof(uint64_t), excl);
    ENSURE(B_CNT, (nflat + 1) * sizeof(uint64_t), ra.cnt);
    ra.flat = flat;
    ra.excl = excl;
    ra.big = w.rs_big;
    ra.nbig = ra.big + HM_RS_BIG_MAX;   /* zeroed with nruns */
    ra.big_min = ctx->rs_big_min;
    hm_launch_rs_copy(s, ra);
    if (hot_level) {
        hr.runbase = runbase;
        hr.flat = flat;
        hr.cnt = ra.cnt;
        hm_launch_hot_runs(s, hr);
    }
    hm_launch_scan(s, ra.cnt, nflat, partial, excl, tot + 1, ra.nflat_dev);
    ra.total_keys = tot + 1;
    ENSURE(B_NKEYS, V.nchildren * sizeof(uint32_t), ra.nkeys);
    ENSURE(B_KEYBASE, V.nchildren * sizeof(uint32_t), ra.keybase);
    ENSURE(B_VALS, V.nchildren * sizeof(uint64_t), ra.vals);
    ENSURE(B_PREFIX, V.nchildren * sizeof(uint64_t), w.prefix);
    hm_launch_rs_keys(s, ra);
    hm_launch_scan(s, ra.vals, V.nchildren, partial, w.prefix, tot + 2);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

/* the non-empty children become B_l (k_compact); the level's one read-back
 * brings its totals, then B_l and its items are published */
int CountCall::level_compact(int l, LevelWork& w)
{
    Level& V = lv[l];
    const HmRsArgs& ra = w.ra;
    int st;
    /* B_l arrays: sized by nchildren (upper bound of |B_l|) */
    const uint64_t cap = V.nchildren + 1;
    HmCompactArgs ca;
    memset(&ca, 0, sizeof(ca));
    if ((st = bucket_arrays(l, cap, ca.out))) return st;
    uint32_t* child_begin;
    ENSURE(B_CHILD0 + l, ((uint64_t)hand.nparents + 1) * 4, child_begin);
    ca.nchildren = V.nchildren;
    ca.nparents = hand.nparents;
    ca.dbits = V.dbits;
    ca.vals = ra.vals;
    ca.prefix = w.prefix;
    ca.total = ltot() + 2;
    ca.nkeys = ra.nkeys;
    ca.nr = ra.nr;
    ca.runbase = ra.runbase;
    ca.keybase = ra.keybase;
    ca.parent_coord = hand.parent_coord;
    ca.child_begin = child_begin;
    if (w.hot3 && l == 1) ENSURE(B_C2B, V.nchildren * 4, ca.c2b);   /* child -> bucket, for level 3 */
    if (l == L - 1) {
        ENSURE(B_SLOTS, cap * 4, slots);
        ENSURE(B_SLOTBKT, cap * 4, slot_bucket);
        ca.slots = slots;
        ca.nslots = ctx->state + ST_NSLOTS;
        ca.slot_bucket = slot_bucket;
    }
    hm_launch_compact(s, ca);
    HIPCHK(hipGetLastError());
    if ((st = read_state(ctx))) return st;   /* the level's totals come with it (ST_LTOT) */
    const uint64_t tot_h = ctx->host_state[ST_LTOT + 2];
    V.count = (uint32_t)(tot_h >> 32);
    V.items = (uint32_t)(tot_h & 0xFFFFFFFFull);
    if (l == L - 1) nslots = (uint32_t)(ctx->host_state[ST_NSLOTS] & 0xFFFFFFFFull);
    /* after a child-contiguous level every item of the next spans one run */
    return publish(l, ca.out, HmRuns{ra.flat, ra.excl}, w.kout, ctx->host_state[ST_LTOT + 1],
                   w.contig ? B_SEG2 : -1);
}

/* final aggregation over B_L */
int CountCall::aggregate()
{
    o.keys = keys_out;
    o.counts = counts_out;
    o.capacity = (uint64_t)capacity;
    o.cursor = ctx->state + ST_CURSOR;
    o.zmin = zmin;
    o.zmax = Z;
    for (int l = 0; l < L; l++) ENSURE(B_TOT0 + l, ((uint64_t)lv[l].count + 1) * 8, totals[l]);
    const int l = L - 1;
    uint32_t* gslots = nullptr;
    ENSURE(B_GSLOTS, (uint64_t)(nslots ? nslots : 1) * HM_AG_CELLS * 4, gslots);
    uint64_t* sptot;
    ENSURE(B_TOTAL, 4 * sizeof(uint64_t), sptot);   /* total, base, k_small_pairs' batch counter */
    {
        HmFill zf;
        zf.k = 0;
        if (nslots) hm_fill_add(zf, gslots, 0, (size_t)nslots * HM_AG_CELLS * 4);
        hm_fill_add(zf, totals[l], 0, ((size_t)lv[l].count + 1) * 8);
        hm_fill_add(zf, sptot + 2, 0, 8);
        hm_launch_fill(s, zf);
    }
    HmAggArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B[l];
    a.keys = (const uint16_t*)hand.keys;
    a.in = hand.runs;
    a.Z = Z;
    a.lg = Z - zb;
    a.totals = totals[l];
    a.gslots = gslots;
    a.slot_bucket = slot_bucket;
    a.out = o;
    a.items = lv[l].items;
    a.nslots = nslots;
    const uint64_t cnt = (uint64_t)lv[l].count + 1;
    uint64_t *spcnt, *spoff, *partial;
    ENSURE(B_VALS, cnt * 8, spcnt);
    ENSURE(B_PREFIX, cnt * 8, spoff);
    ENSURE(B_PARTIAL, 4096 * sizeof(uint64_t), partial);
    ENSURE(B_SPCODES, (hand.level_keys + 8) * 2, a.codes);
    a.spcnt = spcnt;
    a.spoff = spoff;
    a.sptotal = sptot;
    a.spbase = (unsigned long long*)(sptot + 1);
    a.spq = (uint32_t*)(sptot + 2);
    hm_launch_aggregate(s, a, lv[l].items, nslots);
    hm_launch_small(s, a, partial);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

/* pooling: level l children -> parents in B_{l-1} (root for l = 0) */
int CountCall::pool()
{
    for (int l = L - 1; l >= 0; l--) {
        HmPoolArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.dbits = lv[l].dbits;
        pa.z_child = lv[l].zc;
        pa.emit_root = (l == 0);
        void* cb = ctx->bufs[B_CHILD0 + l].p;
        pa.child_begin = (const uint32_t*)cb;
        pa.child_digit = B[l].digit;
        pa.child_totals = totals[l];
        pa.parent_coord = l ? B[l - 1].coord : nullptr;
        pa.parent_totals = l ? totals[l - 1] : nullptr;
        pa.out = o;
        pa.nparents = lv[l].nparents;
        hm_launch_pool(s, pa, lv[l].nparents);
        HIPCHK(hipGetLastError());
    }
    return HM_OK;
}

/* a stream's tail re-keyed, the call's last read-back, hm_last_stats, the
 * cells outside the square and the capacity verdict */
int CountCall::finish()
{
    int st;
    if (ctx->tail_keys) {
        hm_launch_stream_rekey_dev(s, ctx->tail_keys, ctx->state + ST_CURSOR, (uint64_t)capacity, ctx->tail_state,
                                   ctx->tail_cb);
        HIPCHK(hipGetLastError());
        ctx->tail_done = 1;
    }
    if ((st = read_state(ctx))) return st;
    hipEvent_t* ev = ctx->ev;
    for (int i = 0; timing && i + 1 < nev; i++) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
        ctx->stage_us[i] = ms * 1000.0;
    }
    for (int l = 1; timing && l <= npart; l++) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev[5 + 2 * (l - 1)], ev[6 + 2 * (l - 1)]);
        ctx->stage_us[4] += ms * 1000.0;
    }
    ctx->stage_us[5] = (double)l1_reruns;   /* hm_last_stats: level-1 re-runs (a region overflowed) */
    ctx->stage_us[6] = (double)nhot;        /* hm_last_stats: hot tiles of the call */
    const unsigned long long nc = ctx->host_state[ST_CURSOR];
    *n_out = (int64_t)nc;
    /* cells outside the square: the general path over the exotic list */
    uint64_t xt = 0;
    if (nx) {
        HmGenEmit e;
        memset(&e, 0, sizeof(e));
        e.cells = xcells_out;
        e.capacity = (uint64_t)xcapacity;
        e.width = 4;
        if ((st = gen_count(ctx, xl.row, xl.col, nullptr, xl.idx, nx, Z, zmin, e, &xt))) return st;
        if ((st = read_state(ctx))) return st;
    }
    *nx_out = (int64_t)xt;
    if (nc > (unsigned long long)capacity || xt > (uint64_t)xcapacity) return HM_E_CAPACITY;
    return HM_OK;
}
}  // namespace

/* one attempt of hm_count / hm_count_tiles: the pipeline, or the general path
 * when the pipeline's dense child space is too large */
static int count_impl(hm_ctx* ctx, const double* lat, const double* lon, const int64_t* rows, const int64_t* cols,
                      const uint8_t* keep, int64_t n, int zmin, int zmax, uint64_t* keys_out, uint64_t* counts_out,
                      int64_t capacity, int64_t* n_out, int64_t* xcells_out, int64_t xcapacity, int64_t* nx_out)
{
    CountCall c{ctx, lat, lon, rows, cols, keep, n, zmin, zmax, keys_out, counts_out, capacity, n_out, xcells_out,
                xcapacity, nx_out};
    int st = c.run();
    if (st == HM_FALLBACK)
        st = count_fallback(ctx, lat, lon, rows, cols, keep, n, zmin, zmax, keys_out, counts_out, capacity, n_out,
                            xcells_out, xcapacity, nx_out);
    return st;
}

/* an entry point's attempts: a second one after an allocation failure, with
 * the arena released (cached buffers of earlier calls may be what is missing) */
template <class Attempt>
static int retry_nomem(hm_ctx* ctx, Attempt attempt)
{
    int st = attempt();
    if (st == HM_E_NOMEM) {
        arena_release(ctx);
        st = attempt();
    }
    return st;
}

extern "C" int hm_count(hm_ctx* ctx, const double* lat, const double* lon, const uint8_t* keep, int64_t n, int zmin,
                        int zmax, uint64_t* keys_out, uint64_t* counts_out, int64_t capacity, int64_t* n_out,
                        int64_t* xcells_out, int64_t xcapacity, int64_t* nx_out)
{
    if (n > 0 && (!lat || !lon)) return HM_E_ARG;
    return retry_nomem(ctx, [=] {
        return count_impl(ctx, lat, lon, nullptr, nullptr, keep, n, zmin, zmax, keys_out, counts_out, capacity, n_out,
                          xcells_out, xcapacity, nx_out);
    });
}

extern "C" int hm_count_tiles(hm_ctx* ctx, const int64_t* row, const int64_t* col, const uint8_t* keep, int64_t n,
                              int zmin, int zmax, uint64_t* keys_out, uint64_t* counts_out, int64_t capacity,
                              int64_t* n_out, int64_t* xcells_out, int64_t xcapacity, int64_t* nx_out)
{
    if (n > 0 && (!row || !col)) return HM_E_ARG;
    return retry_nomem(ctx, [=] {
        return count_impl(ctx, nullptr, nullptr, row, col, keep, n, zmin, zmax, keys_out, counts_out, capacity, n_out,
                          xcells_out, xcapacity, nx_out);
    });
}

int grouped_impl(hm_ctx* ctx, const double* lat, const double* lon, const int64_t* rows, const int64_t* cols,
                 const uint8_t* keep, const uint32_t* group, int64_t n, int zmin, int zmax, int64_t* cells_out,
                 int64_t capacity, int64_t* n_out, uint64_t* pkeys, uint64_t* pcounts)
{
    const bool packed = pkeys || pcounts;
    if (!ctx || !n_out || n < 0 || n >= (int64_t)0xFFFFFFF0ll || zmin < 0 || zmax < zmin ||
        zmax > HM_COUNT_MAX_ZOOM || capacity < 0 ||
        (capacity > 0 && (packed ? (!pkeys || !pcounts) : !cells_out)))
        return HM_E_ARG;
    *n_out = 0;
    HIPCHK(hipSetDevice(ctx->device));
    int st = reset_state(ctx);
    if (st) return st;
    if (n == 0) return HM_OK;
    uint64_t total = 0;
    HmGenEmit e;
    memset(&e, 0, sizeof(e));
    e.cells = cells_out;
    e.capacity = (uint64_t)capacity;
    e.width = 5;
    if (packed) {
        e.cells = nullptr;
        e.keys = pkeys;
        e.counts = pcounts;
        e.width = 2;
    }
    if (rows) {
        int64_t *row, *col, *idx;
        uint32_t* grp;
        ENSURE(B_X_ROW, (uint64_t)n * 8, row);
        ENSURE(B_X_COL, (uint64_t)n * 8, col);
        ENSURE(B_X_IDX, (uint64_t)n * 8, idx);
        ENSURE(B_GL_GRP, (uint64_t)n * 4, grp);
        hm_launch_tiles_list(ctx->stream, rows, cols, keep, group, n, row, col, grp, idx, ctx->state + ST_XCOUNT);
        HIPCHK(hipGetLastError());
        if ((st = read_state(ctx))) return st;
        if ((st = take_error(ctx))) return st;
        st = gen_count(ctx, row, col, grp, idx, ctx->host_state[ST_XCOUNT], zmax, zmin, e, &total);
    } else {   /* points projected straight into keys */
        st = gen_count(ctx, nullptr, nullptr, group, nullptr, (uint64_t)n, zmax, zmin, e, &total, lat, lon, keep);
    }
    if (st) return st;
    *n_out = (int64_t)total;
    return total > (uint64_t)capacity ? HM_E_CAPACITY : HM_OK;
}

extern "C" int hm_count_grouped(hm_ctx* ctx, const double* lat, const double* lon, const uint8_t* keep,
                                const uint32_t* group, int64_t n, int zmin, int zmax, int64_t* cells_out,
                                int64_t capacity, int64_t* n_out)
{
    if (n > 0 && (!lat || !lon)) return HM_E_ARG;
    return retry_nomem(ctx, [=] {
        return grouped_impl(ctx, lat, lon, nullptr, nullptr, keep, group, n, zmin, zmax, cells_out, capacity, n_out);
    });
}

extern "C" int hm_count_grouped_packed(hm_ctx* ctx, const double* lat, const double* lon, const uint8_t* keep,
                                       const uint32_t* group, int64_t n, int zmin, int zmax, uint64_t* keys_out,
                                       uint64_t* gcounts_out, int64_t capacity, int64_t* n_out)
{
    if (n > 0 && (!lat || !lon)) return HM_E_ARG;
    return retry_nomem(ctx, [=] {
        return grouped_impl(ctx, lat, lon, nullptr, nullptr, keep, group, n, zmin, zmax, nullptr, capacity, n_out,
                            keys_out, gcounts_out);
    });
}

extern "C" int hm_count_grouped_packed_tiles(hm_ctx* ctx, const int64_t* row, const int64_t* col,
                                             const uint8_t* keep, const uint32_t* group, int64_t n, int zmin, int zmax,
                                             uint64_t* keys_out, uint64_t* gcounts_out, int64_t capacity,
                                             int64_t* n_out)
{
    if (n > 0 && (!row || !col)) return HM_E_ARG;
    return retry_nomem(ctx, [=] {
        return grouped_impl(ctx, nullptr, nullptr, row, col, keep, group, n, zmin, zmax, nullptr, capacity, n_out,
                            keys_out, gcounts_out);
    });
}

extern "C" int hm_count_grouped_tiles(hm_ctx* ctx, const int64_t* row, const int64_t* col, const uint8_t* keep,
                                      const uint32_t* group, int64_t n, int zmin, int zmax, int64_t* cells_out,
                                      int64_t capacity, int64_t* n_out)
{
    if (n > 0 && (!row || !col)) return HM_E_ARG;
    return retry_nomem(ctx, [=] {
        return grouped_impl(ctx, nullptr, nullptr, row, col, keep, group, n, zmin, zmax, cells_out, capacity, n_out);
    });
}

/* ------------------------------------------------------------------------ */
/* multi-GPU cell exchange (kernels in hm_merge.hip)                          */
/* ------------------------------------------------------------------------ */

extern "C" int64_t hm_dense_grid_size(int dense_zmax)
{
    if (dense_zmax < 0) return 0;
    if (dense_zmax > 14) return -1;
    return (int64_t)(((1ull << (2 * (dense_zmax + 1))) - 1) / 3);
}

extern "C" int hm_cells_route(hm_ctx* ctx, const uint64_t* keys, const uint64_t* counts, int64_t n, int nranks,
                              int delta, int dense_zmax, uint64_t* grid, void* keys_out, void* counts_out,
                              int layout, int64_t* send_counts)
{
    const bool rec = layout == HM_CELLS_REC10, grp = layout == HM_CELLS_G12;
    if (!ctx || n < 0 || nranks < 1 || nranks > 64 || delta < 0 || delta > 28 || dense_zmax > 14 ||
        (layout != HM_CELLS_U32 && layout != HM_CELLS_U64 && !rec && !grp) || (dense_zmax >= 0 && !grid) ||
        (grp && dense_zmax >= 0) || !send_counts ||
        (n > 0 && (!keys || !counts || !keys_out || (!rec && !counts_out))))
        return HM_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t gsz = hm_dense_grid_size(dense_zmax);
    if (gsz > 0) HIPCHK(hipMemsetAsync(grid, 0, (size_t)gsz * 8, s));
    for (int r = 0; r < nranks; r++) send_counts[r] = 0;
    if (n == 0) return HM_OK;
    const unsigned blocks = hm_route_blocks((uint64_t)n);
    const uint64_t m = (uint64_t)blocks * nranks;
    HmRouteArgs a;
    memset(&a, 0, sizeof(a));
    ENSURE(B_RT_CNT, m * 8, a.block_cnt);
    uint64_t* off;
    ENSURE(B_RT_OFF, (m + 2) * 8, off);    /* + the total, + the wide flag */
    uint64_t *partial, *tot;
    ENSURE(B_PARTIAL, 4096 * sizeof(uint64_t), partial);
    ENSURE(B_TOTAL, 4 * sizeof(uint64_t), tot);
    a.keys = keys;
    a.counts = counts;
    a.n = (uint64_t)n;
    a.nranks = nranks;
    a.delta = delta;
    a.dense_zmax = dense_zmax;
    a.grid = grid;
    a.block_off = off;
    if (layout == HM_CELLS_U64) {
        a.keys_out = (uint64_t*)keys_out;
        a.counts_out = (uint64_t*)counts_out;
    } else {
        if (rec) {
            a.rec_out = (uint16_t*)keys_out;
        } else {
            a.keys_out = (uint64_t*)keys_out;
            a.counts_out32 = (uint32_t*)counts_out;
            a.grouped = grp;
        }
        a.wide = (unsigned long long*)(off + m + 1);
        HIPCHK(hipMemsetAsync(a.wide, 0, 8, s));
    }
    hm_launch_cells_route(s, a, false);
    hm_launch_scan(s, a.block_cnt, m, partial, off, off + m);
    hm_launch_cells_route(s, a, true);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> h(m + 2);
    HIPCHK(hipMemcpyAsync(h.data(), off, (m + 2) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hm_sync(s));
    for (int r = 0; r < nranks; r++)
        send_counts[r] = (int64_t)(h[(uint64_t)(r + 1) * blocks] - h[(uint64_t)r * blocks]);
    return (layout != HM_CELLS_U64 && h[m + 1]) ? HM_E_WIDE : HM_OK;
}

int cells_merge(hm_ctx* ctx, const void* keys_in, const void* counts_in, int layout, int64_t n, const int64_t* runs,
                int nruns, uint64_t* keys_out, uint64_t* counts_out, int64_t capacity, int64_t* n_out)
{
    const uint16_t* recs = layout == HM_CELLS_REC10 ? (const uint16_t*)keys_in : nullptr;
    const uint64_t* keys = recs ? nullptr : (const uint64_t*)keys_in;
    const uint64_t* counts = layout == HM_CELLS_U64 ? (const uint64_t*)counts_in : nullptr;
    const uint32_t* counts32 = layout == HM_CELLS_U32 ? (const uint32_t*)counts_in : nullptr;
    if (((uintptr_t)recs & 1) != 0) return HM_E_ARG;   /* records: u16 words */
    if (!ctx || !n_out || n < 0 || capacity < 0 || (n > 0 && !keys_in) || (n > 0 && !recs && !counts && !counts32) ||
        (capacity > 0 && (!keys_out || !counts_out)) || nruns < 0 || (nruns > 0 && !runs))
        return HM_E_ARG;
    int64_t sum = 0;
    for (int i = 0; i < nruns; i++) {
        if (runs[i] < 0) return HM_E_ARG;
        sum += runs[i];
    }
    if (runs && sum != n) return HM_E_ARG;
    *n_out = 0;
    if (n == 0) return HM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    unsigned long long* down = ctx->host_state + 2 * ST_COUNT;
    const uint64_t *pk_all = nullptr, *pc_all = nullptr;   /* the first partition pass's copy (u64 counts) */
    {
        /* bucketed LDS merge (hm_merge.hip): 2^lb hash buckets of <= ~1800
         * cells (one LDS table pass each), one block per bucket; the cells are
         * hash-partitioned by the top lb bits in one or two coalesced passes
         * of <= 7 bits */
        HmMergeArgs a;
        memset(&a, 0, sizeof(a));
        int lb = 0;
        while (lb < 14 && ((uint64_t)n >> lb) > 1800) lb++;
        const int b1 = lb <= 7 ? lb : (lb + 1) / 2, b2 = lb - b1;
        auto chunks = [](uint64_t cells, uint64_t per, uint32_t cap) {
            return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cap, (cells + per - 1) / per));
        };
        HmMbPass p1;
        memset(&p1, 0, sizeof(p1));
        p1.kin = keys;
        p1.cin = counts;
        p1.cin32 = counts32;
        p1.rin = recs;
        p1.n = (uint64_t)n;
        p1.nseg = 1;
        p1.C = chunks((uint64_t)n, 65536, 512);
        p1.shift = b1 ? 64 - b1 : 63;   /* b1 = 0: one bucket (digit mask 0; no shift by 64) */
        p1.bits = b1;
        const uint64_t m1 = ((uint64_t)1 << b1) * p1.C;
        uint64_t *cnt1, *off1, *pk, *pc;
        ENSURE(B_MB_CNT, m1 * 8, cnt1);
        ENSURE(B_MB_OFF, (m1 + 1) * 8, off1);
        ENSURE(B_MB_KEYS, (uint64_t)n * 8, pk);
        ENSURE(B_MB_COUNTS, (uint64_t)n * 8, pc);
        uint64_t* partial;
        ENSURE(B_PARTIAL, 4096 * sizeof(uint64_t), partial);
        p1.cnt = cnt1;
        p1.off = off1;
        p1.kout = pk;
        p1.cout = pc;
        hm_launch_mb_pass(s, p1, false);
        hm_launch_scan(s, cnt1, m1, partial, off1, off1 + m1);
        hm_launch_mb_pass(s, p1, true);
        a.pkeys = pk;
        a.pcounts = pc;
        a.boff = off1;
        a.nblocks = p1.C;
        if (b2 > 0) {
            /* second pass: each first-pass bucket (a segment) by the next b2 bits */
            HmMbPass p2 = p1;
            p2.kin = pk;
            p2.cin = pc;
            p2.cin32 = nullptr;
            p2.rin = nullptr;
            p2.segoff = off1;
            p2.segstride = p1.C;
            p2.nseg = 1u << b1;
            p2.C = chunks((uint64_t)n >> b1, 32768, 64);
            p2.shift = 64 - lb;
            p2.bits = b2;
            const uint64_t m2 = ((uint64_t)1 << lb) * p2.C;
            uint64_t *cnt2, *off2, *qk, *qc;
            ENSURE(B_MB_CNT2, m2 * 8, cnt2);
            ENSURE(B_MB_OFF2, (m2 + 1) * 8, off2);
            ENSURE(B_MB_KEYS2, (uint64_t)n * 8, qk);
            ENSURE(B_MB_COUNTS2, (uint64_t)n * 8, qc);
            p2.cnt = cnt2;
            p2.off = off2;
            p2.kout = qk;
            p2.cout = qc;
            hm_launch_mb_pass(s, p2, false);
            hm_launch_scan(s, cnt2, m2, partial, off2, off2 + m2);
            hm_launch_mb_pass(s, p2, true);
            a.pkeys = qk;
            a.pcounts = qc;
            a.boff = off2;
            a.nblocks = p2.C;
        }
        a.keys = keys;
        a.counts = counts;
        a.n = (uint64_t)n;
        a.lb = lb;
        pk_all = pk;
        pc_all = pc;
        unsigned long long* st;
        ENSURE(B_MG_STATE, 8 * sizeof(unsigned long long), st);
        HIPCHK(hipMemsetAsync(st, 0, 8 * sizeof(unsigned long long), s));
        a.keys_out = keys_out;
        a.counts_out = counts_out;
        a.cap = (uint64_t)capacity;
        a.cursor = st;
        a.overflow = st + 1;
        hm_launch_mb_merge(s, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(down, st, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hm_sync(s));
        if (!down[1]) {
            *n_out = (int64_t)down[0];
            return *n_out > capacity ? HM_E_CAPACITY : HM_OK;
        }
        /* a bucket's table filled up (adversarial hash collisions): the
         * global hash table below takes the whole merge again */
    }
    uint64_t cap = 1024;
    while (cap < 2 * (uint64_t)n) cap <<= 1;
    HmsTable t;
    ENSURE(B_MG_TABLE, cap * 16, t.slots);
    ENSURE(B_MG_STATE, 8 * sizeof(unsigned long long), t.state);
    t.mask = cap - 1;
    HIPCHK(hipMemsetAsync(t.state, 0, 8 * sizeof(unsigned long long), s));
    hm_launch_stream_init(s, t);
    if (!counts) {
        /* u32 counts or records: the partition pass's u64 copy, in partition order */
        hm_launch_cells_merge(s, pk_all, pc_all, (uint64_t)n, t);
    } else if (runs) {
        /* runs of distinct keys: no two threads of a launch insert one key */
        int64_t off = 0;
        for (int i = 0; i < nruns; i++) {
            hm_launch_cells_merge_unique(s, keys + off, counts + off, (uint64_t)runs[i], t);
            off += runs[i];
        }
    } else {
        hm_launch_cells_merge(s, keys, counts, (uint64_t)n, t);
    }
    hm_launch_table_extract(s, t, keys_out, counts_out, (uint64_t)capacity, t.state + HMS_ST_CURSOR);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(down, t.state, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hm_sync(s));
    if (down[HMS_ST_OVERFLOW]) return HM_E_HIP;   /* cannot happen: load factor <= 1/2 */
    *n_out = (int64_t)down[HMS_ST_CURSOR];
    return *n_out > capacity ? HM_E_CAPACITY : HM_OK;
}

static bool cells_layout_ok(int layout)
{
    return layout == HM_CELLS_U64 || layout == HM_CELLS_U32 || layout == HM_CELLS_REC10;
}

extern "C" int hm_cells_merge(hm_ctx* ctx, const void* keys, const void* counts, int layout, int64_t n,
                              uint64_t* keys_out, uint64_t* counts_out, int64_t capacity, int64_t* n_out)
{
    if (!cells_layout_ok(layout)) return HM_E_ARG;
    return cells_merge(ctx, keys, counts, layout, n, nullptr, 0, keys_out, counts_out, capacity, n_out);
}

extern "C" int hm_cells_merge_runs(hm_ctx* ctx, const void* keys, const void* counts, int layout, int64_t n,
                                   const int64_t* runs, int nruns, uint64_t* keys_out, uint64_t* counts_out,
                                   int64_t capacity, int64_t* n_out)
{
    if (!cells_layout_ok(layout)) return HM_E_ARG;
    return cells_merge(ctx, keys, counts, layout, n, runs, nruns, keys_out, counts_out, capacity, n_out);
}

/* the pieces exchange (hm_merge.hip, "the pieces exchange"): the route orders
 * each owner's group by the first merge digit, so the owner gathers digit
 * s's pieces, partitions them by the next bits and merges */
extern "C" int hm_cells_route_pieces(hm_ctx* ctx, const uint64_t* keys, const uint64_t* counts, int64_t n,
                                     int nranks, int delta, int dense_zmax, int bits, int self_rank, uint64_t* grid,
                                     void* keys_out, void* counts_out, int layout, int64_t* sizes, int stride)
{
    const bool rec = layout == HM_CELLS_REC10, grp = layout == HM_CELLS_G12;
    if (!ctx || n < 0 || nranks < 1 || nranks > 64 || delta < 0 || delta > 28 || dense_zmax > 14 || bits < 0 ||
        self_rank < -1 || self_rank >= nranks ||
        bits > 7 || ((int64_t)nranks << bits) > HM_XR_MAXD || stride < 2 + (1 << bits) || !sizes ||
        (layout != HM_CELLS_U32 && layout != HM_CELLS_U64 && !rec && !grp) || (dense_zmax >= 0 && !grid) ||
        (grp && dense_zmax >= 0) || (n > 0 && (!keys || !counts || !keys_out || (!rec && !counts_out))) ||
        (rec && ((uintptr_t)keys_out & 1)))
        return HM_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t gsz = hm_dense_grid_size(dense_zmax);
    if (gsz > 0) HIPCHK(hipMemsetAsync(grid, 0, (size_t)gsz * 8, s));
    HmRouteArgs a;
    memset(&a, 0, sizeof(a));
    a.C = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(1024, ((uint64_t)n + 16383) / 16384));
    const uint64_t m = ((uint64_t)nranks << bits) * a.C;
    ENSURE(B_RT_CNT, m * 8, a.block_cnt);
    uint64_t* off;
    ENSURE(B_RT_OFF, (m + 2) * 8, off);    /* + the total, + the wide flag */
    uint64_t* partial;
    ENSURE(B_PARTIAL, 4096 * sizeof(uint64_t), partial);
    a.keys = keys;
    a.counts = counts;
    a.n = (uint64_t)n;
    a.nranks = nranks;
    a.delta = delta;
    a.dense_zmax = dense_zmax;
    a.grid = grid;
    a.block_off = off;
    a.bits = bits;
    a.sizes = (long long*)sizes;
    a.stride = stride;
    a.self = self_rank;
    if (layout == HM_CELLS_U64) {
        a.keys_out = (uint64_t*)keys_out;
        a.counts_out = (uint64_t*)counts_out;
    } else if (rec) {
        a.rec_out = (uint16_t*)keys_out;
    } else {
        a.keys_out = (uint64_t*)keys_out;
        a.counts_out32 = (uint32_t*)counts_out;
        a.grouped = grp;
    }
    if (layout != HM_CELLS_U64) {
        a.wide = (unsigned long long*)(off + m + 1);
        HIPCHK(hipMemsetAsync(a.wide, 0, 8, s));
    }
    hm_launch_xroute(s, a, false, layout);
    hm_launch_scan(s, a.block_cnt, m, partial, off, off + m);
    if (n > 0) hm_launch_xroute(s, a, true, layout);
    hm_launch_xroute_sizes(s, a);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_cells_merge_pieces(hm_ctx* ctx, int layout, int nruns, const void* const* key_src,
                                     const void* const* count_src, const int64_t* pieces, int bits,
                                     uint64_t* keys_out, uint64_t* counts_out, int64_t capacity, int64_t* n_out)
{
    const bool rec = layout == HM_CELLS_REC10, c64 = layout == HM_CELLS_U64;
    if (!ctx || !n_out || nruns < 1 || nruns > 64 || bits < 0 || bits > 7 || !pieces || !key_src ||
        (layout != HM_CELLS_U32 && !c64 && layout != HM_CELLS_G12 && !rec) || (!rec && !count_src) ||
        capacity < 0 || (capacity > 0 && (!keys_out || !counts_out)))
        return HM_E_ARG;
    const uint32_t S = 1u << bits, R = (uint32_t)nruns;
    uint64_t n = 0;
    for (uint32_t r = 0; r < R; r++) {
        uint64_t len = 0;
        for (uint32_t d = 0; d < S; d++) {
            if (pieces[r * S + d] < 0) return HM_E_ARG;
            len += (uint64_t)pieces[r * S + d];
        }
        if (len && (!key_src[r] || (!rec && !count_src[r]) || (rec && ((uintptr_t)key_src[r] & 1))))
            return HM_E_ARG;
        n += len;
    }
    *n_out = 0;
    if (n == 0) return HM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    unsigned long long* down = ctx->host_state + 2 * ST_COUNT;
    /* buckets of <= HM_MB2_TARGET cells (one LDS table pass each) */
    int lb = bits;
    while (lb < bits + 8 && (n >> lb) > HM_MB2_TARGET) lb++;
    const int b2 = lb - bits;
    /* piece table: vpre [S][R + 1], key address [S][R], count address [S][R] */
    const size_t ksz = rec ? 10 : 8, csz = c64 ? 8 : 4;
    std::vector<unsigned long long> tab((size_t)S * (R + 1) + 2 * (size_t)S * R, 0ull);
    unsigned long long *vpre = tab.data(), *kp = vpre + (size_t)S * (R + 1), *cp = kp + (size_t)S * R;
    for (uint32_t r = 0; r < R; r++) {
        uint64_t e = 0;   /* cells of run r before piece d */
        for (uint32_t d = 0; d < S; d++) {
            kp[d * R + r] = (unsigned long long)((uintptr_t)key_src[r] + e * ksz);
            cp[d * R + r] = rec ? 0ull : (unsigned long long)((uintptr_t)count_src[r] + e * csz);
            e += (uint64_t)pieces[r * S + d];
        }
    }
    for (uint32_t d = 0; d < S; d++) {
        uint64_t v = 0;
        for (uint32_t r = 0; r < R; r++) {
            vpre[d * (R + 1) + r] = v;
            v += (uint64_t)pieces[r * S + d];
        }
        vpre[d * (R + 1) + R] = v;
    }
    unsigned long long* dtab;
    ENSURE(B_MG_PIECES, tab.size() * 8, dtab);
    HIPCHK(hipMemcpyAsync(dtab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    HmMbGather g;
    memset(&g, 0, sizeof(g));
    g.vpre = dtab;
    g.kp = dtab + (size_t)S * (R + 1);
    g.cp = rec ? nullptr : g.kp + (size_t)S * R;
    g.R = R;
    g.S = S;
#ifndef HM_MG_CHUNK
#define HM_MG_CHUNK 16384
#endif
    g.C = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(64, ((n >> bits) + HM_MG_CHUNK - 1) / HM_MG_CHUNK));
    g.shift = lb ? 64 - lb : 63;
    g.bits = b2;
    g.in_layout = rec ? HM_CELLS_REC10 : (c64 ? HM_CELLS_U64 : HM_CELLS_U32);
    uint64_t *partial, *qk;
    void* qc;
    unsigned long long* st;
    ENSURE(B_PARTIAL, 4096 * sizeof(uint64_t), partial);
    ENSURE(B_MG_STATE, 8 * sizeof(unsigned long long), st);
    HmMergeArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.lb = lb;
    a.keys_out = keys_out;
    a.counts_out = counts_out;
    a.cap = (uint64_t)capacity;
    a.cursor = st;
    a.overflow = st + 1;
    /* fill mode: no count pass -- buckets of a fixed capacity (the mean
     * + 1/4 + 64; hash buckets are near the mean), claimed per tile; a bucket
     * past it (st[2]) or a full LDS table sends the call to the counted form */
    const char* fe = getenv("HM_GATHER_FILL");   /* 0: always the counted form (A/B) */
    const char* be = getenv("HM_GATHER_BCAP");   /* test hook: a bucket capacity (forces the fallback) */
    const uint64_t nbk = 1ull << lb;
    const bool fill = (!fe || atoi(fe) != 0) && n >= 4096;
    auto counted = [&]() -> int {
        const uint64_t m2 = ((uint64_t)S << b2) * g.C;
        uint64_t *cnt2, *off2;
        ENSURE(B_MB_CNT2, m2 * 8, cnt2);
        ENSURE(B_MB_OFF2, (m2 + 1) * 8, off2);
        ENSURE(B_MB_KEYS2, n * 8, qk);
        ENSURE(B_MB_COUNTS2, n * csz, qc);
        g.cnt = cnt2;
        g.off = off2;
        g.kout = qk;
        g.cout = qc;
        g.fill = nullptr;
        hm_launch_mb_gather(s, g, false);
        hm_launch_scan(s, cnt2, m2, partial, off2, off2 + m2);
        hm_launch_mb_gather(s, g, true);
        a.boff = off2;
        a.nblocks = g.C;
        a.bfill = nullptr;
        return HM_OK;
    };
    HIPCHK(hipMemsetAsync(st, 0, 8 * sizeof(unsigned long long), s));
    if (fill) {
        const uint64_t mean = (n + nbk - 1) / nbk;
        const uint64_t bcap = be && atoll(be) > 0 ? (uint64_t)atoll(be) : mean + mean / 4 + 64;
        unsigned long long* fc;
        ENSURE(B_MB_CNT2, nbk * 8, fc);
        ENSURE(B_MB_KEYS2, nbk * bcap * 8, qk);
        ENSURE(B_MB_COUNTS2, nbk * bcap * csz, qc);
        HIPCHK(hipMemsetAsync(fc, 0, nbk * 8, s));
        g.kout = qk;
        g.cout = qc;
        g.fill = fc;
        g.bcap = bcap;
        g.over = st + 2;
        hm_launch_mb_gather(s, g, true);
        a.bfill = fc;
        a.bcap = bcap;
    } else {
        int st2 = counted();
        if (st2 != HM_OK) return st2;
    }
    if (c64) a.pcounts = (uint64_t*)qc;
    else a.pcounts32 = (const uint32_t*)qc;
    a.pkeys = qk;
    hm_launch_mb_merge2(s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(down, st, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hm_sync(s));
    if (fill && (down[1] || down[2])) {
        /* a bucket past its capacity, or a full table: partition again with the
         * count pass (contiguous buckets, which the global table below can take) */
        HIPCHK(hipMemsetAsync(st, 0, 8 * sizeof(unsigned long long), s));
        int st2 = counted();
        if (st2 != HM_OK) return st2;
        a.pkeys = qk;
        if (c64) a.pcounts = (uint64_t*)qc;
        else a.pcounts32 = (const uint32_t*)qc;
        hm_launch_mb_merge2(s, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(down, st, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hm_sync(s));
    }
    if (!down[1]) {
        *n_out = (int64_t)down[0];
        return *n_out > capacity ? HM_E_CAPACITY : HM_OK;
    }
    /* a bucket's table filled up (adversarial hash collisions): a global hash
     * table takes the partitioned cells */
    uint64_t cap = 1024;
    while (cap < 2 * n) cap <<= 1;
    HmsTable t;
    ENSURE(B_MG_TABLE, cap * 16, t.slots);
    ENSURE(B_MG_STATE, 8 * sizeof(unsigned long long), t.state);
    t.mask = cap - 1;
    HIPCHK(hipMemsetAsync(t.state, 0, 8 * sizeof(unsigned long long), s));
    hm_launch_stream_init(s, t);
    if (c64) hm_launch_cells_merge(s, qk, (const uint64_t*)qc, n, t);
    else hm_launch_cells_merge32(s, qk, (const uint32_t*)qc, n, t);
    hm_launch_table_extract(s, t, keys_out, counts_out, (uint64_t)capacity, t.state + HMS_ST_CURSOR);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(down, t.state, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hm_sync(s));
    if (down[HMS_ST_OVERFLOW]) return HM_E_HIP;
    *n_out = (int64_t)down[HMS_ST_CURSOR];
    return *n_out > capacity ? HM_E_CAPACITY : HM_OK;
}

extern "C" int hm_dense_cells(hm_ctx* ctx, const uint64_t* grid, int dense_zmax, uint64_t* keys_out,
                              uint64_t* counts_out, int64_t capacity, int64_t* n_out)
{
    if (!ctx || !n_out || !grid || dense_zmax < 0 || dense_zmax > 14 || capacity < 0 ||
        (capacity > 0 && (!keys_out || !counts_out)))
        return HM_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    unsigned long long* cur = ctx->state + ST_CURSOR;
    HIPCHK(hipMemsetAsync(cur, 0, 8, s));
    hm_launch_dense_extract(s, grid, (uint64_t)hm_dense_grid_size(dense_zmax), dense_zmax, keys_out, counts_out,
                            (uint64_t)capacity, cur);
    HIPCHK(hipGetLastError());
    int st = read_state(ctx);
    if (st) return st;
    *n_out = (int64_t)ctx->host_state[ST_CURSOR];
    return *n_out > capacity ? HM_E_CAPACITY : HM_OK;
}

extern "C" int hm_format_bins(hm_ctx* ctx, const int64_t* zoom, const int64_t* row, const int64_t* col,
                              const int64_t* value, const uint8_t* head, const uint8_t* last, const int64_t* offset,
                              int64_t n, uint8_t* text)
{
    if (!ctx || n < 0 || (n > 0 && (!zoom || !row || !col || !value || !head || !last || !offset || !text)))
        return HM_E_ARG;
    if (n == 0) return HM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HmFormatArgs a{zoom, row, col, value, head, last, offset, n, text};
    hm_launch_format_bins(ctx->stream, a);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_format_ids(hm_ctx* ctx, const uint8_t* names, const int64_t* name_off, const int64_t* label,
                             const uint8_t* spans, const int64_t* span_off, const int64_t* span, const int64_t* tz,
                             const int64_t* tr, const int64_t* tc, const int64_t* offset, int64_t n, uint8_t* text)
{
    if (!ctx || n < 0 ||
        (n > 0 && (!names || !name_off || !label || !spans || !span_off || !span || !tz || !tr || !tc || !offset ||
                   !text)))
        return HM_E_ARG;
    if (n == 0) return HM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HmIdArgs a{names, name_off, label, spans, span_off, span, tz, tr, tc, offset, n, text};
    hm_launch_format_ids(ctx->stream, a);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_synth(hm_ctx* ctx, int kind, uint64_t seed, int64_t start, int64_t n, double* lat, double* lon,
                        const double* table, int k)
{
    if (!ctx || n < 0 || kind < 0 || kind > 2 || (n > 0 && (!lat || !lon)) || (kind == 1 && (!table || k <= 0)))
        return HM_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    if (n > 0) hm_launch_synth(ctx->stream, kind, seed, start, n, lat, lon, table, k);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_bench_read(hm_ctx* ctx, const void* a, const void* b, int64_t bytes_each, uint64_t* sink)
{
    if (!ctx || bytes_each < 0 || (bytes_each & 15) || (bytes_each > 0 && (!a || !b || !sink))) return HM_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    if (bytes_each > 0) hm_launch_read_stream(ctx->stream, a, b, (uint64_t)bytes_each, sink);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

/* ---- top-k selection (hm_top.hip) ---- */

int cells_top(hm_ctx* ctx, const uint64_t* keys, const uint64_t* counts, int64_t n, int64_t k, uint64_t* keys_out,
              uint64_t* counts_out)
{
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t q = ctx->stream;
    if (n <= k) {   /* every record: only the order is missing */
        hm_launch_top_sort(q, keys, counts, (uint64_t)n, nullptr, keys_out, counts_out);
        HIPCHK(hipGetLastError());
        return HM_OK;
    }
    unsigned char* scratch;
    HmTopArgs a;
    ENSURE(B_TOP_SCRATCH, HM_TOP_SCRATCH_BYTES, scratch);
    ENSURE(B_TOP_KEYS, HM_TOP_MAX_K * 8, a.sel_keys);
    ENSURE(B_TOP_COUNTS, HM_TOP_MAX_K * 8, a.sel_counts);
    HIPCHK(hipMemsetAsync(scratch, 0, HM_TOP_SCRATCH_BYTES, q));
    a.keys = keys;
    a.counts = counts;
    a.n = (uint64_t)n;
    a.k = (uint64_t)k;
    a.words = (unsigned long long*)scratch;
    a.states = (HmTopState*)(scratch + HM_TOP_W_COUNT * 8);
    a.hist = (unsigned long long*)(scratch + HM_TOP_W_COUNT * 8 + (HM_TOP_PASSES + 1) * sizeof(HmTopState));
    hm_launch_top_select(q, a);
    hm_launch_top_sort(q, a.sel_keys, a.sel_counts, (uint64_t)k, a.words + HM_TOP_W_CURSOR, keys_out, counts_out);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

/* do the byte ranges [a, a + na) and [b, b + nb) share a byte */
static bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

extern "C" int hm_cells_top(hm_ctx* ctx, const uint64_t* keys, const uint64_t* counts, int64_t n, int64_t k,
                            uint64_t* keys_out, uint64_t* counts_out, int64_t* n_out)
{
    if (!ctx || !n_out || n < 0 || k < 1 || k > HM_TOP_MAX_K || (n > 0 && (!keys || !counts || !keys_out || !counts_out)))
        return HM_E_ARG;
    if (n > 0) {
        const uint64_t in = (uint64_t)n * 8, out = (uint64_t)k * 8;
        for (const void* o : {(const void*)keys_out, (const void*)counts_out})
            if (ranges_overlap(o, out, keys, in) || ranges_overlap(o, out, counts, in)) return HM_E_ARG;
        if (ranges_overlap(keys_out, out, counts_out, out)) return HM_E_ARG;
    }
    /* written once the work is enqueued (no wait), so that a failure leaves it as it was */
    const int st = n ? cells_top(ctx, keys, counts, n, k, keys_out, counts_out) : HM_OK;
    if (st == HM_OK) *n_out = n < k ? n : k;
    return st;
}

/* ---- rasters: dense tile grids and rendered tiles (hm_raster.hip) ---- */

/* the shared argument check of the two scatters: tiles inside their squares,
 * bin zooms inside [zlo, zhi] */
bool raster_args_ok(const int64_t* tiles, int ntiles, int bins_log2, int halo, int zlo, int zhi)
{
    if (!tiles || ntiles < 1 || ntiles > HM_RASTER_MAX_TILES || bins_log2 < 0 || bins_log2 > HM_RASTER_MAX_BINS_LOG2 ||
        halo < 0 || halo > HM_RASTER_MAX_HALO)
        return false;
    for (int t = 0; t < ntiles; t++) {
        const int64_t tz = tiles[3 * t], tr = tiles[3 * t + 1], tc = tiles[3 * t + 2];
        if (tz < 0 || tz > HM_MAX_ZOOM || tz + bins_log2 < zlo || tz + bins_log2 > zhi) return false;
        if (tr < 0 || tc < 0 || tr >= (1ll << tz) || tc >= (1ll << tz)) return false;
    }
    return true;
}

extern "C" int hm_cells_raster(hm_ctx* ctx, const uint64_t* keys, const uint64_t* counts, int64_t n,
                               const int64_t* tiles, int ntiles, int bins_log2, int halo, uint64_t* grid_out)
{
    if (!ctx || !grid_out || n < 0 || (n > 0 && (!keys || !counts)) ||
        !raster_args_ok(tiles, ntiles, bins_log2, halo, 0, HM_MAX_ZOOM))
        return HM_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t q = ctx->stream;
    const int64_t S = 1ll << bins_log2, W = S + 2 * halo;
    HIPCHK(hipMemsetAsync(grid_out, 0, (size_t)ntiles * W * W * 8, q));
    if (n == 0) return HM_OK;
    HmCellsRasterArgs a;
    a.keys = keys;
    a.counts = counts;
    a.n = (uint64_t)n;
    a.ntiles = ntiles;
    a.W = (uint32_t)W;
    a.grid = (unsigned long long*)grid_out;
    for (int t = 0; t < ntiles; t++) {
        a.tiles[t].z = (int32_t)(tiles[3 * t] + bins_log2);
        a.tiles[t].oy = (int32_t)((tiles[3 * t + 1] << bins_log2) - halo);
        a.tiles[t].ox = (int32_t)((tiles[3 * t + 2] << bins_log2) - halo);
    }
    hm_launch_cells_raster(q, a);
    HIPCHK(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_raster_render(hm_ctx* ctx, const uint64_t* grid, int ntiles, int bins_log2, int halo, int radius,
                                int scale, uint64_t vmax, const uint32_t* lut, uint8_t* rgba_out, uint8_t* levels_out,
                                uint64_t* vmax_used)
{
    if (!ctx || !grid || !lut || !rgba_out || ((uintptr_t)rgba_out & 3) || ntiles < 1 || ntiles > HM_RASTER_MAX_TILES ||
        bins_log2 < 0 || bins_log2 > HM_RASTER_MAX_BINS_LOG2 || halo < 0 || halo > HM_RASTER_MAX_HALO || radius < 0 ||
        radius > halo || (scale != HM_SCALE_LINEAR && scale != HM_SCALE_LOG))
        return HM_E_ARG;
    const uint64_t wide = 1ull << (56 - 4 * radius);
    if (vmax >= wide) return HM_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t q = ctx->stream;
    HmRenderArgs a;
    a.grid = grid;
    a.ntiles = ntiles;
    a.bins_log2 = bins_log2;
    a.halo = halo;
    a.radius = radius;
    a.scale = scale;
    a.vs = vmax << (4 * radius);
    a.wide = wide;
    ENSURE(B_RS_B, ((size_t)ntiles << (2 * bins_log2)) * 8, a.B);
    ENSURE(B_RS_MX, 16, a.mx);
    a.lut = lut;
    a.rgba = (uint32_t*)rgba_out;
    a.levels = levels_out;
    HIPCHK(hipMemsetAsync(a.mx, 0, 16, q));
    hm_launch_raster_blur(q, a);
    hm_launch_raster_colour(q, a);
    HIPCHK(hipGetLastError());
    unsigned long long* down = ctx->host_state + 2 * ST_COUNT;
    HIPCHK(hipMemcpyAsync(down, a.mx, 16, hipMemcpyDeviceToHost, q));
    HIPCHK(hm_sync(q));
    if (down[0] >= wide) return HM_E_WIDE;
    if (vmax_used) *vmax_used = a.vs ? a.vs : (uint64_t)down[1];
    return HM_OK;
}

extern "C" int hm_raster_accumulate(hm_ctx* ctx, const uint64_t* grid_in, int64_t nframes, int64_t frame_elems,
                                    int64_t window, uint64_t* grid_out)
{
    if (!ctx || !grid_in || !grid_out || nframes < 1 || frame_elems < 1 || window < 0 ||
        nframes > (INT64_MAX / 8) / frame_elems)
        return HM_E_ARG;
    const uintptr_t in = (uintptr_t)grid_in, out = (uintptr_t)grid_out, bytes = (uintptr_t)(nframes * frame_elems * 8);
    if (in < out + bytes && out < in + bytes) return HM_E_ARG;   /* the leaving frame is read after its slot is written */
    HIPCHK(hipSetDevice(ctx->device));
    hm_launch_raster_accumulate(ctx->stream, grid_in, grid_out, (uint64_t)nframes, (uint64_t)frame_elems,
                                (uint64_t)((window == 0 || window > nframes) ? nframes : window));
    HIPCHK(hipGetLastError());
    return HM_OK;
}
