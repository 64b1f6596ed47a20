// tsdf.hip — mesh export: depth frames fused into a truncated signed distance volume, and its zero level set as a
// welded, oriented triangle mesh (marching tetrahedra).  What the reference reaches through nerfstudio's
// `ns-export tsdf` (exporter/tsdf_utils.py + skimage's marching cubes), written for splat and sensor depth.  The
// contract is in include/gg_raster.h (gg_tsdf_*) and PARITY.md "Mesh export"; the design in DESIGN.md §3.16.
//
// gg_tsdf_integrate   one launch: a workgroup owns a 4 x 8 x 8 brick of lattice points, one thread per point, the
//                     point's state in registers across all views (read and written once per call, no atomics).  Per
//                     view the workgroup first decides, from the brick's eight corners in fp64 with a margin far above
//                     fp32 rounding, whether any of its points can pass the projection tests; if none can, the view
//                     is skipped by the whole brick (wave-uniform branch, no depth gathers).
// gg_tsdf_mesh_count  reset (one fill), tm_count_kernel (a thread per cell: the 6 tetrahedra's cases, the used edges
//                     OR-ed into per-point 7-bit masks, the cell's face count), tm_scan_kernel (vertex and face
//                     offsets: two decoupled look-back scans, scan.h, in one launch), tm_totals_kernel.
// gg_tsdf_mesh_emit   tm_vertex_kernel (a thread per point: its vertices), tm_face_kernel (a thread per cell).
#include <math.h>

#include "scan.h"

#define TS_THREADS 256
#define TS_BX 4                    // brick: 4 x 8 x 8 points, z fastest (one wave = one x slice of 8 x 8)
#define TS_BY 8
#define TS_BZ 8
#define TS_TOL 1e-4                // brick test margin, relative (fp32 rounding of the per-point path: ~1e-6)
#define TM_THREADS 256
#define TM_PER 4                   // points per thread of the scan pass
#define TM_POINTS (TM_THREADS * TM_PER)

struct TsGrid {
    int X, Y, Z;
    float o[3], s[3];
};

// ---------------------------------------------------------------------------------------------------------------
// integration
// ---------------------------------------------------------------------------------------------------------------
struct TsParams {
    TsGrid g;
    float trunc;
    int V, H, W;
    int nby, nbz;                  // bricks along y, z
};

// false only if no point of the brick [lo, hi] (lattice indices) can pass c2 > 0, 0 <= u < W, 0 <= v < H in fp32.
// Every lane evaluates corner (lane & 7); the answer is wave-uniform.
__device__ __forceinline__ bool ts_brick_sees(const TsParams &p, const float *__restrict__ E,
                                              const float *__restrict__ K, const int *lo, const int *hi) {
    const int c = threadIdx.x & 7;
    double q[3], pmax[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double l = (double)p.g.o[a] + (double)lo[a] * (double)p.g.s[a];
        const double h = (double)p.g.o[a] + (double)hi[a] * (double)p.g.s[a];
        q[a] = ((c >> (2 - a)) & 1) ? h : l;
        pmax[a] = fmax(fabs(l), fabs(h));
    }
    double cc[3], B[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double e0 = E[4 * r], e1 = E[4 * r + 1], e2 = E[4 * r + 2], e3 = E[4 * r + 3];
        cc[r] = ((e0 * q[0] + e1 * q[1]) + e2 * q[2]) + e3;
        B[r] = ((fabs(e0) * pmax[0] + fabs(e1) * pmax[1]) + fabs(e2) * pmax[2]) + fabs(e3);
    }
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3], W = p.W, H = p.H;
    const double m2 = TS_TOL * B[2];
    if (__all(cc[2] < -m2)) return false;                        // behind the camera
    if (!__all(cc[2] > m2)) return true;                         // straddles the camera plane: no decision
    const double mu = TS_TOL * (fabs(fx) * B[0] + (fabs(cx) + W) * B[2]);
    const double mv = TS_TOL * (fabs(fy) * B[1] + (fabs(cy) + H) * B[2]);
    if (__all(fx * cc[0] + cx * cc[2] < -mu)) return false;                  // u < 0
    if (__all(fx * cc[0] + (cx - W) * cc[2] > mu)) return false;             // u >= W
    if (__all(fy * cc[1] + cy * cc[2] < -mv)) return false;                  // v < 0
    if (__all(fy * cc[1] + (cy - H) * cc[2] > mv)) return false;             // v >= H
    return true;
}

template <bool COLOR>
__global__ __launch_bounds__(TS_THREADS) void tsdf_integrate_kernel(TsParams p, const float *__restrict__ depth,
                                                                    const float *__restrict__ rgb,
                                                                    const float *__restrict__ intr,
                                                                    const float *__restrict__ w2c,
                                                                    float *__restrict__ tsdf, float *__restrict__ weight,
                                                                    float *__restrict__ color,
                                                                    float *__restrict__ cweight) {
    const int b = blockIdx.x;
    const int bz = b % p.nbz, r = b / p.nbz, by = r % p.nby, bx = r / p.nby;
    const int t = threadIdx.x;
    const int i = bx * TS_BX + (t >> 6), j = by * TS_BY + ((t >> 3) & 7), k = bz * TS_BZ + (t & 7);
    const bool live = i < p.g.X && j < p.g.Y && k < p.g.Z;
    const int lo[3] = {bx * TS_BX, by * TS_BY, bz * TS_BZ};
    const int hi[3] = {min(lo[0] + TS_BX, p.g.X) - 1, min(lo[1] + TS_BY, p.g.Y) - 1, min(lo[2] + TS_BZ, p.g.Z) - 1};
    const size_t idx = live ? ((size_t)i * p.g.Y + j) * p.g.Z + k : 0;
    const float x = p.g.o[0] + (float)i * p.g.s[0];
    const float y = p.g.o[1] + (float)j * p.g.s[1];
    const float z = p.g.o[2] + (float)k * p.g.s[2];
    float T = 0.f, Wt = 0.f, C0 = 0.f, C1 = 0.f, C2 = 0.f, Kw = 0.f;
    if (live) {
        T = tsdf[idx];
        Wt = weight[idx];
        if (COLOR) {
            C0 = color[3 * idx];
            C1 = color[3 * idx + 1];
            C2 = color[3 * idx + 2];
            Kw = cweight[idx];
        }
    }
    const float Wf = (float)p.W, Hf = (float)p.H, tr = p.trunc;
    for (int view = 0; view < p.V; ++view) {
        const float *E = w2c + 12 * (size_t)view;
        const float *Kp = intr + 4 * (size_t)view;
        if (!ts_brick_sees(p, E, Kp, lo, hi)) continue;
        if (!live) continue;
        const float c2 = ((E[8] * x + E[9] * y) + E[10] * z) + E[11];
        if (!(c2 > 0.f)) continue;
        const float c0 = ((E[0] * x + E[1] * y) + E[2] * z) + E[3];
        const float c1 = ((E[4] * x + E[5] * y) + E[6] * z) + E[7];
        const float u = (Kp[0] * c0) / c2 + Kp[2];
        const float v = (Kp[1] * c1) / c2 + Kp[3];
        if (!(u >= 0.f && u < Wf && v >= 0.f && v < Hf)) continue;
        const size_t pix = ((size_t)view * p.H + (int)v) * p.W + (int)u;     // u, v >= 0: truncation is floor
        const float d = depth[pix];
        if (!(d > 0.f)) continue;                                            // 0, negative, NaN: no observation
        const float dist = d - c2;
        if (!(dist >= -tr)) continue;
        const float obs = fminf(1.f, dist / tr);
        const float Wn = Wt + 1.f;
        T = (T * Wt + obs) / Wn;
        Wt = Wn;
        if (COLOR && fabsf(dist) < tr) {
            const float Kn = Kw + 1.f;
            C0 = (C0 * Kw + rgb[3 * pix]) / Kn;
            C1 = (C1 * Kw + rgb[3 * pix + 1]) / Kn;
            C2 = (C2 * Kw + rgb[3 * pix + 2]) / Kn;
            Kw = Kn;
        }
    }
    if (live) {
        tsdf[idx] = T;
        weight[idx] = Wt;
        if (COLOR) {
            color[3 * idx] = C0;
            color[3 * idx + 1] = C1;
            color[3 * idx + 2] = C2;
            cweight[idx] = Kw;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the marching-tetrahedra table, derived at compile time from the Kuhn decomposition (header: gg_tsdf_mesh_*)
// ---------------------------------------------------------------------------------------------------------------
// corner id of a cell: (ox << 2) | (oy << 1) | oz; an edge code: corner id of its lower end * 8 + direction
constexpr int kDir[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
constexpr int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

struct MtTable {
    uint8_t corner[6][4];          // corner ids of each tetrahedron
    uint8_t ntri[6][16];
    uint8_t edge[6][16][2][3];
};

struct MtVec {
    int v[3];
};

constexpr MtVec mt_corner(int t, int n) {   // corner n = 0..3 of tetrahedron t
    MtVec c{{0, 0, 0}};
    for (int s = 0; s < n && s < 3; ++s) c.v[kPerm[t][s]] = 1;
    return c;
}
constexpr int mt_id(MtVec c) { return (c.v[0] << 2) | (c.v[1] << 1) | c.v[2]; }
constexpr uint8_t mt_edge(int t, int a, int b) {
    const int l = a < b ? a : b, h = a < b ? b : a;
    const MtVec cl = mt_corner(t, l), ch = mt_corner(t, h);
    int d = 0;
    for (int q = 0; q < 7; ++q)
        if (kDir[q][0] == ch.v[0] - cl.v[0] && kDir[q][1] == ch.v[1] - cl.v[1] && kDir[q][2] == ch.v[2] - cl.v[2]) d = q;
    return (uint8_t)(mt_id(cl) * 8 + d);
}
// sign of det(M_e1 - 2 w, M_e2 - 2 w, M_e3 - 2 w), M_e = the sum of an edge's two corners (twice its midpoint)
constexpr long mt_orient(int t, const int (&e)[3][2], int w) {
    long m[3][3] = {};
    const MtVec cw = mt_corner(t, w);
    for (int r = 0; r < 3; ++r) {
        const MtVec a = mt_corner(t, e[r][0]), b = mt_corner(t, e[r][1]);
        for (int c = 0; c < 3; ++c) m[r][c] = a.v[c] + b.v[c] - 2 * cw.v[c];
    }
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}
// triangle on edges e (corner pairs), wound so that its normal points away from w when sign > 0 (towards w if < 0)
constexpr void mt_put(MtTable &T, int t, int cs, int slot, int (&e)[3][2], int w, int sign) {
    if (sign * mt_orient(t, e, w) < 0) {
        for (int q = 0; q < 2; ++q) {
            const int tmp = e[1][q];
            e[1][q] = e[2][q];
            e[2][q] = tmp;
        }
    }
    for (int r = 0; r < 3; ++r) T.edge[t][cs][slot][r] = mt_edge(t, e[r][0], e[r][1]);
}
constexpr MtTable mt_make_table() {
    MtTable T{};
    for (int t = 0; t < 6; ++t) {
        for (int n = 0; n < 4; ++n) T.corner[t][n] = (uint8_t)mt_id(mt_corner(t, n));
        for (int cs = 0; cs < 16; ++cs) {
            int in[4] = {}, out[4] = {}, ni = 0, no = 0;
            for (int n = 0; n < 4; ++n) {
                if ((cs >> n) & 1) in[ni++] = n;
                else out[no++] = n;
            }
            if (ni == 1 || ni == 3) {
                const int a = ni == 1 ? in[0] : out[0];             // the corner apart
                const int *o = ni == 1 ? out : in;
                int e[3][2] = {{a, o[0]}, {a, o[1]}, {a, o[2]}};
                mt_put(T, t, cs, 0, e, a, ni == 1 ? 1 : -1);
                T.ntri[t][cs] = 1;
            } else if (ni == 2) {
                const int pp = in[0], qq = in[1], rr = out[0], ss = out[1];
                int e0[3][2] = {{pp, rr}, {pp, ss}, {qq, ss}};
                int e1[3][2] = {{pp, rr}, {qq, ss}, {qq, rr}};
                mt_put(T, t, cs, 0, e0, pp, 1);
                mt_put(T, t, cs, 1, e1, qq, 1);
                T.ntri[t][cs] = 2;
            }
        }
    }
    return T;
}
__constant__ MtTable kMt = mt_make_table();

struct TmParams {
    TsGrid g;
    int64_t P;                     // lattice points
    int nblocks;                   // scan workgroups
};

__device__ __forceinline__ int64_t tm_corner_offset(const TsGrid &g, int cid) {
    return ((int64_t)((cid >> 2) & 1) * g.Y + ((cid >> 1) & 1)) * g.Z + (cid & 1);
}
__device__ __forceinline__ unsigned tm_mask(const uint32_t *__restrict__ masks, int64_t q) {
    return (masks[q >> 2] >> (8 * (q & 3))) & 0x7fu;
}
// the cell whose lower corner is point p, or false at the upper borders
__device__ __forceinline__ bool tm_cell(const TsGrid &g, int64_t p) {
    const int k = (int)(p % g.Z);
    const int64_t r = p / g.Z;
    const int j = (int)(r % g.Y), i = (int)(r / g.Y);
    return i < g.X - 1 && j < g.Y - 1 && k < g.Z - 1;
}

// ---------------------------------------------------------------------------------------------------------------
// count: used edges and faces per cell
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_THREADS) void tm_count_kernel(TmParams pr, const float *__restrict__ tsdf,
                                                              const float *__restrict__ weight,
                                                              uint32_t *__restrict__ masks, uint8_t *__restrict__ fc) {
    const int64_t p = (int64_t)blockIdx.x * TM_THREADS + threadIdx.x;
    if (p >= pr.P) return;
    int nf = 0;
    if (tm_cell(pr.g, p)) {
        float Tc[8];
        bool obs = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int64_t q = p + tm_corner_offset(pr.g, c);
            Tc[c] = tsdf[q];
            obs = obs && weight[q] > 0.f;
        }
        if (obs) {
            unsigned cm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int t = 0; t < 6; ++t) {
                int cs = 0;
#pragma unroll
                for (int n = 0; n < 4; ++n) cs |= (Tc[kMt.corner[t][n]] < 0.f ? 1 : 0) << n;
                const int nt = kMt.ntri[t][cs];
                for (int s = 0; s < nt; ++s)
                    for (int e = 0; e < 3; ++e) {
                        const int code = kMt.edge[t][cs][s][e];
                        cm[code >> 3] |= 1u << (code & 7);
                    }
                nf += nt;
            }
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (cm[c]) {
                    const int64_t q = p + tm_corner_offset(pr.g, c);
                    atomicOr(masks + (q >> 2), cm[c] << (8 * (q & 3)));
                }
        }
    }
    fc[p] = (uint8_t)nf;
}

// ---------------------------------------------------------------------------------------------------------------
// offsets: exclusive scans of the vertex and face counts, TM_POINTS points per workgroup
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_THREADS) void tm_scan_kernel(TmParams pr, const uint32_t *__restrict__ masks,
                                                             const uint8_t *__restrict__ fc,
                                                             uint32_t *__restrict__ voff, uint32_t *__restrict__ foff,
                                                             ScanState *stv, ScanState *stf) {
    __shared__ unsigned int s_slot, s_exv, s_exf, wsv[4], wsf[4];
    const int bid = scan_ticket(stv, &s_slot);
    const int64_t base = (int64_t)bid * TM_POINTS + (int64_t)threadIdx.x * TM_PER;
    unsigned nv[TM_PER], nf[TM_PER], sv = 0, sf = 0;
#pragma unroll
    for (int e = 0; e < TM_PER; ++e) {
        const int64_t q = base + e;
        nv[e] = q < pr.P ? (unsigned)__popc(tm_mask(masks, q)) : 0u;
        nf[e] = q < pr.P ? (unsigned)fc[q] : 0u;
        sv += nv[e];
        sf += nf[e];
    }
    unsigned totv, totf;
    unsigned exv = scan_block256(sv, wsv, totv);
    unsigned exf = scan_block256(sf, wsf, totf);
    exv += scan_lookback(stv, bid, pr.nblocks, totv, &s_exv);
    exf += scan_lookback(stf, bid, pr.nblocks, totf, &s_exf);
#pragma unroll
    for (int e = 0; e < TM_PER; ++e) {
        const int64_t q = base + e;
        if (q < pr.P) {
            voff[q] = exv;
            foff[q] = exf;
        }
        exv += nv[e];
        exf += nf[e];
    }
}

__global__ void tm_totals_kernel(const ScanState *stv, const ScanState *stf, int64_t *__restrict__ counts) {
    if (threadIdx.x == 0) {
        counts[0] = (int64_t)stv->total;       // all ones (-1) if a look-back gave up
        counts[1] = (int64_t)stf->total;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// emit
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tm_grad(const float *__restrict__ T, int64_t q, int idx, int n, int64_t stride,
                                         float s) {
    if (n < 2) return 0.f;
    if (idx == 0) return (T[q + stride] - T[q]) / s;
    if (idx == n - 1) return (T[q] - T[q - stride]) / s;
    return (T[q + stride] - T[q - stride]) / (2.f * s);
}

__global__ __launch_bounds__(TM_THREADS) void tm_vertex_kernel(TmParams pr, const float *__restrict__ tsdf,
                                                               const float *__restrict__ color,
                                                               const uint32_t *__restrict__ masks,
                                                               const uint32_t *__restrict__ voff, int64_t cap,
                                                               float *__restrict__ vert, float *__restrict__ nrm,
                                                               float *__restrict__ col) {
    const int64_t p = (int64_t)blockIdx.x * TM_THREADS + threadIdx.x;
    if (p >= pr.P) return;
    const unsigned m = tm_mask(masks, p);
    if (!m) return;
    const TsGrid &g = pr.g;
    const int k = (int)(p % g.Z);
    const int64_t r = p / g.Z;
    const int j = (int)(r % g.Y), i = (int)(r / g.Y);
    const int ia[3] = {i, j, k};
    const int64_t stride[3] = {(int64_t)g.Y * g.Z, g.Z, 1};
    const int dims[3] = {g.X, g.Y, g.Z};
    const float Ta = tsdf[p];
    float ga[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) ga[a] = tm_grad(tsdf, p, ia[a], dims[a], stride[a], g.s[a]);
    const unsigned base = voff[p];
    for (int d = 0; d < 7; ++d) {
        if (!((m >> d) & 1)) continue;
        const int64_t id = (int64_t)base + __popc(m & ((1u << d) - 1));
        if (id >= cap) continue;
        int ib[3];
        int64_t q = p;
        bool in = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            ib[a] = ia[a] + kDir[d][a];
            q += kDir[d][a] * stride[a];
            in = in && ib[a] < dims[a];
        }
        if (!in) continue;                                        // (only a workspace no count call filled)
        const float Tb = tsdf[q];
        const float t = Ta / (Ta - Tb);
        float n[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float gc = kDir[d][a] ? (float)ia[a] + t : (float)ia[a];
            vert[3 * id + a] = g.o[a] + gc * g.s[a];
            const float gb = tm_grad(tsdf, q, ib[a], dims[a], stride[a], g.s[a]);
            n[a] = ga[a] + t * (gb - ga[a]);
        }
        const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) nrm[3 * id + a] = len > 0.f ? n[a] / len : 0.f;
        if (col) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float ca = color[3 * p + a], cb = color[3 * q + a];
                col[3 * id + a] = ca + t * (cb - ca);
            }
        }
    }
}

__global__ __launch_bounds__(TM_THREADS) void tm_face_kernel(TmParams pr, const float *__restrict__ tsdf,
                                                             const uint32_t *__restrict__ masks,
                                                             const uint8_t *__restrict__ fc,
                                                             const uint32_t *__restrict__ voff,
                                                             const uint32_t *__restrict__ foff, int64_t cap,
                                                             int32_t *__restrict__ faces) {
    const int64_t p = (int64_t)blockIdx.x * TM_THREADS + threadIdx.x;
    if (p >= pr.P || fc[p] == 0 || !tm_cell(pr.g, p)) return;   // faces only where the count pass found them
    float Tc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) Tc[c] = tsdf[p + tm_corner_offset(pr.g, c)];
    int64_t f = foff[p];
    for (int t = 0; t < 6; ++t) {
        int cs = 0;
#pragma unroll
        for (int n = 0; n < 4; ++n) cs |= (Tc[kMt.corner[t][n]] < 0.f ? 1 : 0) << n;
        const int nt = kMt.ntri[t][cs];
        for (int s = 0; s < nt; ++s, ++f) {
            if (f >= cap) continue;
            for (int e = 0; e < 3; ++e) {
                const int code = kMt.edge[t][cs][s][e], d = code & 7;
                const int64_t q = p + tm_corner_offset(pr.g, code >> 3);
                faces[3 * f + e] = (int32_t)(voff[q] + __popc(tm_mask(masks, q) & ((1u << d) - 1)));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
static bool ts_dims_ok(const int32_t *dims) {
    if (!dims) return false;
    int64_t P = 1;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 1 || dims[a] > GG_TSDF_MAX_DIM) return false;
        P *= dims[a];
    }
    return P <= GG_TSDF_MAX_POINTS;
}

static bool ts_grid(const int32_t *dims, const float *grid, TsGrid *g) {
    for (int a = 0; a < 6; ++a)
        if (!isfinite(grid[a])) return false;
    for (int a = 3; a < 6; ++a)
        if (!(grid[a] > 0.f)) return false;
    *g = TsGrid{dims[0], dims[1], dims[2], {grid[0], grid[1], grid[2]}, {grid[3], grid[4], grid[5]}};
    return true;
}

struct TmLayout {
    uint32_t *masks;
    uint8_t *fc;
    uint32_t *voff, *foff;
    ScanState *stv, *stf;
    size_t reset_bytes;            // masks + both scan states: one fill
};

static size_t tm_layout(int64_t P, TmLayout *L, char *base) {
    const int nb = (int)((P + TM_POINTS - 1) / TM_POINTS);
    const size_t sb = gg_scan_state_bytes(nb);
    GgCarve cv{base, 0};
    uint32_t *masks = (uint32_t *)cv.take(4 * (size_t)((P + 3) / 4));
    ScanState *stv = (ScanState *)cv.take(sb);
    ScanState *stf = (ScanState *)cv.take(sb);
    const size_t reset = cv.off;
    uint8_t *fc = (uint8_t *)cv.take((size_t)P);
    uint32_t *voff = (uint32_t *)cv.take(4 * (size_t)P);
    uint32_t *foff = (uint32_t *)cv.take(4 * (size_t)P);
    if (L) *L = TmLayout{masks, fc, voff, foff, stv, stf, reset};
    return cv.off;
}

static int64_t ts_points(const int32_t *dims) { return (int64_t)dims[0] * dims[1] * dims[2]; }

extern "C" int gg_tsdf_integrate(const int32_t *dims, const float *grid, float trunc, int num_views, int height,
                                 int width, const float *depth, const float *rgb, const float *intrinsics,
                                 const float *w2c, float *tsdf, float *weight, float *color, float *color_weight,
                                 gg_stream_t stream) {
    GG_REQUIRE(ts_dims_ok(dims), "need 1 <= dims[a] <= GG_TSDF_MAX_DIM and dims[0] dims[1] dims[2] <= GG_TSDF_MAX_POINTS");
    GG_REQUIRE(grid, "null pointer: grid (a host array of 6 floats)");
    TsGrid g;
    GG_REQUIRE(ts_grid(dims, grid, &g), "grid: origin must be finite and voxel sizes finite and > 0");
    GG_REQUIRE(isfinite(trunc) && trunc > 0.f, "trunc must be finite and > 0");
    GG_REQUIRE(num_views >= 0 && num_views <= GG_TSDF_MAX_VIEWS, "need 0 <= num_views <= GG_TSDF_MAX_VIEWS");
    GG_REQUIRE(height >= 1 && width >= 1 && height <= GG_TSDF_MAX_SIDE && width <= GG_TSDF_MAX_SIDE,
               "need 1 <= height, width <= GG_TSDF_MAX_SIDE");
    GG_REQUIRE(tsdf && weight, "null pointer: tsdf / weight");
    GG_REQUIRE(num_views == 0 || (depth && intrinsics && w2c), "null pointer: depth / intrinsics / w2c");
    GG_REQUIRE(rgb ? (color && color_weight) : (!color && !color_weight),
               "color and color_weight are given exactly when rgb is");
    GG_REQUIRE((((uintptr_t)depth | (uintptr_t)rgb | (uintptr_t)intrinsics | (uintptr_t)w2c | (uintptr_t)tsdf |
                 (uintptr_t)weight | (uintptr_t)color | (uintptr_t)color_weight) & 3) == 0,
               "depth / rgb / intrinsics / w2c / tsdf / weight / color / color_weight must be 4-byte aligned");
    if (num_views == 0) return GG_OK;
    TsParams p{g, trunc, num_views, height, width, (g.Y + TS_BY - 1) / TS_BY, (g.Z + TS_BZ - 1) / TS_BZ};
    const int64_t nbx = (g.X + TS_BX - 1) / TS_BX;
    const unsigned blocks = (unsigned)(nbx * p.nby * p.nbz);
    hipStream_t s = (hipStream_t)stream;
    gg_prof_begin(GG_K_TSDF_INTEGRATE, s);
    if (rgb)
        hipLaunchKernelGGL(tsdf_integrate_kernel<true>, dim3(blocks), dim3(TS_THREADS), 0, s, p, depth, rgb, intrinsics,
                           w2c, tsdf, weight, color, color_weight);
    else
        hipLaunchKernelGGL(tsdf_integrate_kernel<false>, dim3(blocks), dim3(TS_THREADS), 0, s, p, depth, rgb,
                           intrinsics, w2c, tsdf, weight, color, color_weight);
    gg_prof_end(GG_K_TSDF_INTEGRATE, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" size_t gg_tsdf_mesh_workspace(const int32_t *dims) {
    if (!ts_dims_ok(dims)) return 0;
    return tm_layout(ts_points(dims), nullptr, nullptr);
}

extern "C" int gg_tsdf_mesh_count(const int32_t *dims, const float *tsdf, const float *weight, int64_t *counts,
                                  void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(ts_dims_ok(dims), "need 1 <= dims[a] <= GG_TSDF_MAX_DIM and dims[0] dims[1] dims[2] <= GG_TSDF_MAX_POINTS");
    GG_REQUIRE(tsdf && weight && counts, "null pointer: tsdf / weight / counts");
    GG_REQUIRE((((uintptr_t)tsdf | (uintptr_t)weight) & 3) == 0 && ((uintptr_t)counts & 7) == 0,
               "tsdf / weight / counts misaligned");
    const int64_t P = ts_points(dims);
    const size_t need = tm_layout(P, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    TmLayout L;
    tm_layout(P, &L, (char *)ws);
    TmParams pr{TsGrid{dims[0], dims[1], dims[2], {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}}, P,
                (int)((P + TM_POINTS - 1) / TM_POINTS)};
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((P + TM_THREADS - 1) / TM_THREADS);
    gg_prof_begin(GG_K_TSDF_MESH, s);
    if (gg_fill_async(ws, 0, L.reset_bytes, s) != hipSuccess) {
        gg_set_error("%s: workspace reset failed", __func__);
        return GG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(tm_count_kernel, dim3(blocks), dim3(TM_THREADS), 0, s, pr, tsdf, weight, L.masks, L.fc);
    hipLaunchKernelGGL(tm_scan_kernel, dim3((unsigned)pr.nblocks), dim3(TM_THREADS), 0, s, pr, L.masks, L.fc, L.voff,
                       L.foff, L.stv, L.stf);
    hipLaunchKernelGGL(tm_totals_kernel, dim3(1), dim3(64), 0, s, L.stv, L.stf, counts);
    gg_prof_end(GG_K_TSDF_MESH, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_tsdf_mesh_emit(const int32_t *dims, const float *grid, const float *tsdf, const float *color,
                                 int64_t num_vertices, int64_t num_faces, float *vertices, float *normals,
                                 float *colors, int32_t *faces, const void *ws, size_t ws_bytes, gg_stream_t stream) {
    GG_REQUIRE(ts_dims_ok(dims), "need 1 <= dims[a] <= GG_TSDF_MAX_DIM and dims[0] dims[1] dims[2] <= GG_TSDF_MAX_POINTS");
    GG_REQUIRE(grid, "null pointer: grid (a host array of 6 floats)");
    TsGrid g;
    GG_REQUIRE(ts_grid(dims, grid, &g), "grid: origin must be finite and voxel sizes finite and > 0");
    GG_REQUIRE(tsdf, "null pointer: tsdf");
    GG_REQUIRE(num_vertices >= 0 && num_faces >= 0, "negative capacity");
    GG_REQUIRE(num_vertices == 0 || (vertices && normals), "null pointer: vertices / normals");
    GG_REQUIRE(num_faces == 0 || faces, "null pointer: faces");
    GG_REQUIRE((((uintptr_t)tsdf | (uintptr_t)color | (uintptr_t)vertices | (uintptr_t)normals | (uintptr_t)colors |
                 (uintptr_t)faces) & 3) == 0,
               "tsdf / color / vertices / normals / colors / faces must be 4-byte aligned");
    const int64_t P = ts_points(dims);
    const size_t need = tm_layout(P, nullptr, nullptr);
    GG_REQUIRE_WS(ws, ws_bytes, need);
    TmLayout L;
    tm_layout(P, &L, (char *)const_cast<void *>(ws));
    TmParams pr{g, P, (int)((P + TM_POINTS - 1) / TM_POINTS)};
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((P + TM_THREADS - 1) / TM_THREADS);
    float *col_out = (color && colors) ? colors : nullptr;
    gg_prof_begin(GG_K_TSDF_MESH, s);
    if (num_vertices > 0)
        hipLaunchKernelGGL(tm_vertex_kernel, dim3(blocks), dim3(TM_THREADS), 0, s, pr, tsdf, color, L.masks, L.voff,
                           num_vertices, vertices, normals, col_out);
    if (num_faces > 0)
        hipLaunchKernelGGL(tm_face_kernel, dim3(blocks), dim3(TM_THREADS), 0, s, pr, tsdf, L.masks, L.fc, L.voff,
                           L.foff, num_faces, faces);
    gg_prof_end(GG_K_TSDF_MESH, s);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
