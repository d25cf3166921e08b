/* Dense tile rasters and rendered RGBA tiles (hm_cells_raster, hm_raster_render;
 * the stream's own scatter, k_stream_raster, lives in hm_stream.hip).
 *
 * A raster is ntiles grids of W x W u64 bins, W = S + 2 halo, S = 2^bins_log2:
 * tile (tz, tr, tc) holds the bins of zoom tz + bins_log2 from (tr << b) - halo
 * by row and (tc << b) - halo by column.  Cells are ADDED into their bins, so
 * equal cells need no merge first.
 *
 * Rendering is integer throughout and so defined bit for bit:
 *   k_raster_blur    one workgroup per HM_BLUR_BLOCK^2 outputs: the block's
 *                    inputs with a radius-wide apron go to LDS, a horizontal
 *                    then a vertical pass with the binomial weights C(2R, k)
 *                    give B (the blurred count in units of 2^-4R, never divided).
 *                    The same pass takes the two maxima the levels need: raw g
 *                    over every haloed grid (the width test: B * 255 must fit
 *                    u64) and B over the interiors (the automatic scale), each
 *                    reduced per block and added to the call's words with one
 *                    atomic max per block.
 *   k_raster_colour  B -> level 0..255 (linear, or a piecewise-linear fixed
 *                    point log2) -> the LUT's RGBA word.
 *
 * Grids of several frames (hm_stream_raster_frames) are frame-major, so one
 * frame is a raster as above; k_raster_accumulate sums them along the frames.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/heatmap_amd.h"
#include "hm_device.h"
#include "hm_pipeline.h"

#define HM_CR_U 8   /* keys in flight per thread */

__global__ __launch_bounds__(256) void k_cells_raster(HmCellsRasterArgs a, uint32_t zooms)
{
    constexpr int U = HM_CR_U;
    const int tid = threadIdx.x;
    const uint32_t WW = a.W * a.W;
    constexpr uint64_t CH = 256 * U;
    for (uint64_t c0 = (uint64_t)blockIdx.x * CH; c0 < a.n; c0 += (uint64_t)gridDim.x * CH) {
        uint64_t k[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = c0 + (uint64_t)u * 256 + tid;
            k[u] = i < a.n ? a.keys[i] : ~0ull;   /* zoom 63: no tile's */
        }
        uint32_t any = 0;             /* bit u: a cell of a listed zoom, inside the square */
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int z = HM_KEY_ZOOM(k[u]);
            const bool ok = z <= HM_MAX_ZOOM && ((zooms >> z) & 1u) && (HM_KEY_ROW(k[u]) >> z) == 0 &&
                            (HM_KEY_COL(k[u]) >> z) == 0;
            any |= (uint32_t)ok << u;
        }
        if (!__ballot(any != 0)) continue;
        for (int t = 0; t < a.ntiles; t++) {
            const HmRasterTile T = a.tiles[t];
            unsigned long long* g = a.grid + (uint64_t)t * WW;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t y = (uint32_t)((int32_t)HM_KEY_ROW(k[u]) - T.oy);
                const uint32_t x = (uint32_t)((int32_t)HM_KEY_COL(k[u]) - T.ox);
                if (((any >> u) & 1u) && HM_KEY_ZOOM(k[u]) == T.z && y < a.W && x < a.W)
                    atomicAdd(&g[y * a.W + x], (unsigned long long)a.counts[c0 + (uint64_t)u * 256 + tid]);
            }
        }
    }
}

void hm_launch_cells_raster(hipStream_t s, const HmCellsRasterArgs& a)
{
    uint32_t zooms = 0;
    for (int t = 0; t < a.ntiles; t++) zooms |= 1u << a.tiles[t].z;
    const uint64_t chunks = (a.n + 256 * HM_CR_U - 1) / (256 * HM_CR_U);
    if (a.n)
        hipLaunchKernelGGL(k_cells_raster, dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(256), 0, s, a, zooms);
}

/* the block's two maxima -> the call's words, one atomic each */
__device__ __forceinline__ void hm_block_max2(uint64_t gmax, uint64_t bmax, unsigned long long* mx)
{
    __shared__ unsigned long long red[2][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        gmax = max(gmax, (uint64_t)__shfl_xor((unsigned long long)gmax, o, 64));
        bmax = max(bmax, (uint64_t)__shfl_xor((unsigned long long)bmax, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = gmax;
        red[1][threadIdx.x >> 6] = bmax;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long* r = red[threadIdx.x];
        const unsigned long long m = max(max(r[0], r[1]), max(r[2], r[3]));
        if (m) atomicMax(&mx[threadIdx.x], m);
    }
}

/* Block shape: HM_BLUR_BLOCK x HM_BLUR_BLOCK outputs (32 x 32), an apron of
 * R <= 8 bins on every side: (32 + 2R)^2 u64 inputs (18 KB at R = 8) and
 * (32 + 2R) x 32 u64 after the horizontal pass (12 KB), 30 KB of LDS, so two
 * workgroups share a CU; a 256 x 256 tile is 8 x 8 blocks, a tile of S <= 32
 * one partly used block. */
__global__ __launch_bounds__(256) void k_raster_blur(HmRenderArgs a)
{
    constexpr int BS = HM_BLUR_BLOCK, EMAX = BS + 2 * HM_RASTER_MAX_HALO;
    __shared__ uint64_t in[EMAX * EMAX];
    __shared__ uint64_t tmp[EMAX * BS];
    __shared__ uint32_t w[2 * HM_RASTER_MAX_HALO + 1];
    const int tid = threadIdx.x;
    const int S = 1 << a.bins_log2, H = a.halo, R = a.radius, W = S + 2 * H, E = BS + 2 * R;
    const int nb = (S + BS - 1) / BS;
    const int t = blockIdx.y, by = blockIdx.x / nb, bx = blockIdx.x % nb;
    const uint64_t* g = a.grid + (uint64_t)t * W * W;
    if (tid == 0) {
        uint32_t c = 1;
        for (int k = 0; k <= 2 * R; k++) {
            w[k] = c;
            c = c * (uint32_t)(2 * R - k) / (uint32_t)(k + 1);
        }
    }
    /* the raw maximum: this block's share of every haloed grid */
    uint64_t gmax = 0, bmax = 0;
    {
        const uint64_t total = (uint64_t)a.ntiles * W * W;
        const uint64_t nblocks = (uint64_t)gridDim.x * gridDim.y;
        const uint64_t bid = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
        for (uint64_t i = bid * 256 + tid; i < total; i += nblocks * 256) gmax = max(gmax, a.grid[i]);
    }
    /* inputs: grid rows H + by*BS - R .. + E (those past the grid feed no kept output) */
    const int y0 = H + by * BS - R, x0 = H + bx * BS - R;
    for (int i = tid; i < E * E; i += 256) {
        const int yy = i / E, xx = i - yy * E;
        const int sy = y0 + yy, sx = x0 + xx;
        in[yy * E + xx] = (sy < W && sx < W) ? g[(uint64_t)sy * W + sx] : 0ull;
    }
    __syncthreads();
    for (int i = tid; i < E * BS; i += 256) {
        const int yy = i / BS, x = i % BS;
        uint64_t acc = 0;
        for (int j = 0; j <= 2 * R; j++) acc += (uint64_t)w[j] * in[yy * E + x + j];
        tmp[yy * BS + x] = acc;
    }
    __syncthreads();
    for (int i = tid; i < BS * BS; i += 256) {
        const int y = i / BS, x = i % BS;
        const int oy = by * BS + y, ox = bx * BS + x;
        if (oy >= S || ox >= S) continue;
        uint64_t acc = 0;
        for (int j = 0; j <= 2 * R; j++) acc += (uint64_t)w[j] * tmp[(y + j) * BS + x];
        a.B[((uint64_t)t * S + oy) * S + ox] = acc;
        bmax = max(bmax, acc);
    }
    hm_block_max2(gmax, bmax, a.mx);
}

/* q(u) = 256 floor(log2 u) + the next 8 bits of u: a piecewise-linear log2 with 8 fractional bits, u >= 1 */
__device__ __forceinline__ uint32_t hm_q(uint64_t u)
{
    const int e = 63 - __clzll((long long)u);
    return 256u * (uint32_t)e + (uint32_t)(((u << (63 - e)) >> 55) & 255ull);
}

__global__ __launch_bounds__(256) void k_raster_colour(HmRenderArgs a)
{
    const uint64_t n = (uint64_t)a.ntiles << (2 * a.bins_log2);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    /* the maxima were written by the kernel before this one */
    if (a.mx[0] >= a.wide) return;   /* HM_E_WIDE: the outputs stay untouched */
    const uint64_t vs = a.vs ? a.vs : a.mx[1];
    const uint64_t B = a.B[i];
    uint32_t level = 0;
    if (B != 0 && vs != 0) {
        uint64_t l;
        if (a.scale == HM_SCALE_LINEAR) {
            l = B * 255ull / vs;
        } else {
            const uint64_t one = 1ull << (4 * a.radius);
            const uint32_t off = 256u * 4u * (uint32_t)a.radius;
            const uint32_t qb = hm_q(B + one) - off, qv = hm_q(vs + one) - off;
            l = (uint64_t)qb * 255u / (qv ? qv : 1u);
        }
        level = (uint32_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
    }
    a.rgba[i] = a.lut[level];
    if (a.levels) a.levels[i] = (uint8_t)level;
}

void hm_launch_raster_blur(hipStream_t s, const HmRenderArgs& a)
{
    const int S = 1 << a.bins_log2, nb = (S + HM_BLUR_BLOCK - 1) / HM_BLUR_BLOCK;
    hipLaunchKernelGGL(k_raster_blur, dim3((unsigned)(nb * nb), (unsigned)a.ntiles), dim3(256), 0, s, a);
}

void hm_launch_raster_colour(hipStream_t s, const HmRenderArgs& a)
{
    const uint64_t n = (uint64_t)a.ntiles << (2 * a.bins_log2);
    hipLaunchKernelGGL(k_raster_colour, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}

/* Trailing or cumulative sums along the frames of a frame-major grid
 * (hm_raster_accumulate): out[f][e] = in[f - window + 1 .. f][e] summed.  The
 * threads of a wave own consecutive elements e, so every frame's load and
 * store is one coalesced row; a thread walks the frames with a running sum,
 * adding the entering frame and subtracting the leaving one (read again from
 * the input: 16 B read and 8 B written per element, 8 B read while the window
 * is still filling and throughout a cumulative sum).  HM_ACC_U frames' loads
 * are issued together.  window: 1 .. nframes (nframes: nothing ever leaves). */
#define HM_ACC_U 4
__global__ __launch_bounds__(256) void k_raster_accumulate(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                           uint64_t nframes, uint64_t elems, uint64_t window)
{
    constexpr int U = HM_ACC_U;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < elems; e += (uint64_t)gridDim.x * 256) {
        uint64_t sum = 0;
        for (uint64_t f0 = 0; f0 < nframes; f0 += U) {
            uint64_t add[U], sub[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t f = f0 + u;
                add[u] = f < nframes ? in[f * elems + e] : 0ull;
                sub[u] = (f < nframes && f >= window) ? in[(f - window) * elems + e] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t f = f0 + u;
                sum += add[u] - sub[u];
                if (f < nframes) out[f * elems + e] = sum;
            }
        }
    }
}

void hm_launch_raster_accumulate(hipStream_t s, const uint64_t* in, uint64_t* out, uint64_t nframes, uint64_t elems,
                                 uint64_t window)
{
    const uint64_t blocks = (elems + 255) / 256;
    hipLaunchKernelGGL(k_raster_accumulate, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, in, out,
                       nframes, elems, window);
}
