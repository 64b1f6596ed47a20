// grasp_common.h — what grasp.hip (gg_grasp_contacts) and grasp_clear.hip (gg_grasp_clearance) share: the tiling
// constants of "one lane per grasp, points staged through LDS, the point range split into chunks", the cull's margin
// and conditioning rule, outward fp32 rounding, and the chunk plan.
#ifndef GG_GRASP_COMMON_H
#define GG_GRASP_COMMON_H
#include <math.h>

#include "gg_common.h"

#define GC_TILE 256              // grasps per workgroup (one per lane)
#define GC_STAGE 256             // points per LDS stage
#define GC_TARGET_BLOCKS 2048    // chunks x grasp tiles aimed for: 8 workgroups per CU
#define GC_MIN_CHUNK 512         // fewest points a chunk is given
#define GC_MARGIN 1e-6           // relative widening of the cull box (>> the fp64 test's rounding)
#define GC_MAX_COND 1e3          // max|R| max|R^-T| above this: no cull for that grasp
#define GC_ROW 17

__device__ __forceinline__ float gc_down(double x) {
    float f = (float)x;
    return (double)f > x ? nextafterf(f, -INFINITY) : f;
}
__device__ __forceinline__ float gc_up(double x) {
    float f = (float)x;
    return (double)f < x ? nextafterf(f, INFINITY) : f;
}

// C chunks of len points (len a multiple of GC_STAGE), from (N, M) only, so that a call's summation order never
// depends on the device.
static void gc_chunks(int N, int M, int *C, int *len) {
    *C = 0;
    *len = 0;
    if (N <= 0 || M <= 0) return;
    const int tiles = (M + GC_TILE - 1) / GC_TILE;
    int c = GC_TARGET_BLOCKS / tiles;
    c = max(1, min(c, (N + GC_MIN_CHUNK - 1) / GC_MIN_CHUNK));
    int l = (N + c - 1) / c;
    l = (l + GC_STAGE - 1) / GC_STAGE * GC_STAGE;
    *len = l;
    *C = (N + l - 1) / l;
}

#endif /* GG_GRASP_COMMON_H */
