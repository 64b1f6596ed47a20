// field_volume.h — what every reader of the distance field's volume shares (field.hip, arm.hip): the grid record and
// its host-side checks, the free-cell rule of the route kernels, and the probe of one sphere centre.  The volume is
// [X][Y][Z], z fastest; include/gg_raster.h "distance field" has the contract.  place.hip needs only the cell rule and
// includes field_cell.h alone.
#pragma once
#include <math.h>

#include "field_cell.h"
#include "gg_common.h"

struct FieldDims {
    int X, Y, Z;
    __device__ __forceinline__ bool inside(int x, int y, int z) const {
        return x >= 0 && x < X && y >= 0 && y < Y && z >= 0 && z < Z;
    }
    // the one place the index expression lives
    __device__ __forceinline__ size_t at(int x, int y, int z) const { return ((size_t)x * Y + y) * Z + z; }
};

struct FieldGrid : FieldDims {
    double lo[3], h;
};

// The free-cell rule: cell (x, y, z) is open iff it is inside the volume and dist2 >= need.
struct FieldFree : FieldDims {
    const int *dist2;
    int need;
    __device__ __forceinline__ bool open(int x, int y, int z) const {
        return inside(x, y, z) && dist2[at(x, y, z)] >= need;
    }
};

// dist2 of the cell that holds the sphere centre (x, y, z) of frame T (R row-major, then t), `outside` when that cell
// is not in the volume.  A world coordinate is ((T[3a] x + T[3a+1] y) + T[3a+2] z) + T[9+a], in this order
// (-ffp-contract=off); a centre that is not finite is outside.
__device__ __forceinline__ int field_probe(const FieldGrid &g, const int *__restrict__ dist2, const double *T, double x,
                                           double y, double z, int outside) {
    const int dim[3] = {g.X, g.Y, g.Z};
    int cell[3];
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c = ((T[3 * a] * x + T[3 * a + 1] * y) + T[3 * a + 2] * z) + T[9 + a];
        const bool ok = isfinite(c);
        cell[a] = ok ? field_cell(c - g.lo[a], g.h) : -1;
        in = in && cell[a] >= 0 && cell[a] < dim[a];
    }
    return in ? dist2[g.at(cell[0], cell[1], cell[2])] : outside;
}

// Host side: the checks every C entry makes of dims, grid and need.
static inline bool field_dims_ok(const int32_t *dims) {
    if (!dims) return false;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 1 || dims[a] > GG_FIELD_MAX_DIM) return false;
        cells *= dims[a];
    }
    return cells <= GG_FIELD_MAX_CELLS;
}

static inline bool field_grid(const int32_t *dims, const double *grid, FieldGrid *g) {
    for (int a = 0; a < 4; ++a)
        if (!isfinite(grid[a])) return false;
    if (!(grid[3] > 0.0)) return false;
    *g = FieldGrid{{dims[0], dims[1], dims[2]}, {grid[0], grid[1], grid[2]}, grid[3]};
    return true;
}

static inline int64_t field_cells(const int32_t *dims) { return (int64_t)dims[0] * dims[1] * dims[2]; }

#define FIELD_DIMS_MSG "need 1 <= dims[a] <= GG_FIELD_MAX_DIM and dims[0] dims[1] dims[2] <= GG_FIELD_MAX_CELLS"
#define FIELD_GRID_MSG "grid: the corner must be finite and the cell edge h finite and > 0"

#define GG_REQUIRE_FIELD_NEED(need) GG_REQUIRE((need) >= 0 && (need) <= GG_FIELD_FAR, "need must be in 0..GG_FIELD_FAR")
