// field_cell.h — the cell rule that field.hip and place.hip share (include/gg_raster.h "distance field": a division
// may propose the cell, the fp64 comparisons decide).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define FIELD_CELL_CLAMP 1073741824.0   // 2^30: a cell index beyond it is outside every volume and every reach

// The cell along one axis of d = p - lo: floor(d / h), corrected by one so that c h <= d < (c + 1) h holds in fp64.
// d finite.  Clamped to +-2^30 (outside every volume, and further from it than any reach).
__device__ __forceinline__ int field_cell(double d, double h) {
    double c = floor(d / h);
    c = c < -FIELD_CELL_CLAMP ? -FIELD_CELL_CLAMP : (c > FIELD_CELL_CLAMP ? FIELD_CELL_CLAMP : c);
    if (c * h > d)
        c -= 1.0;
    else if ((c + 1.0) * h <= d)
        c += 1.0;
    return (int)c;
}
