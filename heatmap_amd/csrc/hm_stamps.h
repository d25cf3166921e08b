/* Phase stamps of the count kernels (profiling builds only).
 *
 * A kernel source states which stamp modes its kernels carry, then includes
 * this header:
 *     #define HM_STAMP_MODES(m) ((m) == 5 || (m) == 7)
 *     #include "hm_stamps.h"
 * Modes: 1 k_partition, 2 k_project_partition, 3 k_partition_fr, 4 k_l1_fast,
 * 5 k_aggregate, 7 k_small_pairs.
 *
 * -DHM_STAMPS=<mode> (tools/stamps.py): thread 0 of the first HM_STAMP_BLOCKS
 * blocks of that kernel records s_memtime at up to 12 points.  The source that
 * carries the mode defines g_stamps and hm_debug_stamps; in every other source
 * the stamp sites expand to nothing, those of shared code (hm_runs.h) too, so
 * a build holds both exactly once.
 * -DHM_ISA_MARKS=<mode> (tools/isa_phases.py): the stamp sites of that kernel
 * as assembly comments; the build is only ever read, not run. */
#pragma once
#include <hip/hip_runtime.h>
#include "hm_device.h"

#ifndef HM_STAMP_MODES
#error "define HM_STAMP_MODES(m), the stamp modes this source carries, before including hm_stamps.h"
#endif

#if defined(HM_STAMPS) && HM_STAMP_MODES(HM_STAMPS)
#define HM_STAMP_BLOCKS 65536
__device__ unsigned long long g_stamps[HM_STAMP_BLOCKS * 12];
#define HM_STAMP_M(m, k)                                                                       \
    do {                                                                                       \
        if (HM_STAMPS == (m) && threadIdx.x == 0 && hm_block_id() < HM_STAMP_BLOCKS)           \
            g_stamps[hm_block_id() * 12 + (k)] = __builtin_amdgcn_s_memtime();                 \
    } while (0)
#define HM_STAMP_V(m, k, v)                                                                    \
    do {                                                                                       \
        if (HM_STAMPS == (m) && threadIdx.x == 0 && hm_block_id() < HM_STAMP_BLOCKS)           \
            g_stamps[hm_block_id() * 12 + (k)] = (v);                                          \
    } while (0)
extern "C" int hm_debug_stamps(void* host, size_t bytes)
{
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), bytes, 0, hipMemcpyDeviceToHost);
}
#elif defined(HM_ISA_MARKS)
#define HM_STAMP_M(m, k)                                                                       \
    do {                                                                                       \
        if (HM_ISA_MARKS == (m)) asm volatile("; hm_phase_mark " #k);                          \
    } while (0)
#define HM_STAMP_V(m, k, v) do { } while (0)
#else
#define HM_STAMP_M(m, k) do { } while (0)
#define HM_STAMP_V(m, k, v) do { } while (0)
#endif
#define HM_STAMP(k) HM_STAMP_M(1, k)
