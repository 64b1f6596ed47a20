// edit.hip — scene update after a grasp (reference nerfstudio/scripts/update.py): select every
// Gaussian whose mean lies inside the convex hull of an object's points (`points_inside_convex_hull`, :293-328) and
// move the selected ones rigidly (`transformed_gs`, :217-240) — in ONE pass over the Gaussians on the device instead
// of the reference's host round trip (means -> numpy -> scipy Delaunay.find_simplex -> mask -> device).
//
// One lane per Gaussian.  The hull arrives as F outward half-spaces n.x + d <= tol (Qhull's `equations`), fp64,
// staged through LDS HE_CHUNK planes at a time; every lane of a wave reads the same plane (LDS broadcast).  Most
// Gaussians are outside a grasped object, so a wave stops walking the planes as soon as none of its lanes is still
// inside (one ballot per plane), and a workgroup stops staging further chunks once none of its lanes is.  A far
// point fails about half of a hull's planes, so most workgroups are done within their first chunk: the chunk is
// small for that reason (staging all 1000 planes of a dense hull per workgroup, 32 KB, made F ~ 1000 ten times
// slower than F ~ 100 at 5 M Gaussians).
// The count is a ballot popcount per wave, summed per workgroup, then one 64-bit atomic per workgroup.
#include "gg_common.h"

#define HE_THREADS 256
#define HE_CHUNK 128          // planes per LDS stage: 128 x 4 doubles = 4 KB, two loads per lane

struct HullRigid {
    float r[12];              // [R | t], row-major 3 x 4
};

// gg_quat_to_rotmat_fwd's per-lane arithmetic (project.hip: quat_normalise + quat_to_rotmat_fwd_kernel), restated
// with the same operation order so that R(q) is bit-identical (tests/test_scene_edit_gpu.py holds the two together)
__device__ __forceinline__ void he_quat_to_rotmat(float4 q, float *R) {
    const float nn = ((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w;
    const float d = fmaxf(sqrtf(nn), GG_QUAT_NORM_EPS);
    const float w = q.x / d, x = q.y / d, y = q.z / d, z = q.w / d;
    R[0] = 1.0f - 2.0f * (y * y + z * z);
    R[1] = 2.0f * (x * y - w * z);
    R[2] = 2.0f * (x * z + w * y);
    R[3] = 2.0f * (x * y + w * z);
    R[4] = 1.0f - 2.0f * (x * x + z * z);
    R[5] = 2.0f * (y * z - w * x);
    R[6] = 2.0f * (x * z - w * y);
    R[7] = 2.0f * (y * z + w * x);
    R[8] = 1.0f - 2.0f * (x * x + y * y);
}

// Shepperd's method: branch on the largest of tr, m00, m11, m22, so the square root's argument is >= 1 for a
// rotation.  The tr branch is the reference's `rotmat_to_quat` (update.py:331-339) operation for operation; that
// formula alone takes sqrt of 1 + tr -> 0 near a half turn (NaN once fp32 rounds it below zero, PARITY.md).
// Sign flipped to w >= 0; not renormalised.
__device__ __forceinline__ float4 he_rotmat_to_quat(const float *m) {
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7],
                m22 = m[8];
    const float tr = (m00 + m11) + m22;
    float w, x, y, z;
    if (tr >= m00 && tr >= m11 && tr >= m22) {
        w = sqrtf(((1.0f + m00) + m11) + m22) / 2.0f;
        const float w4 = 4.0f * w;
        x = (m21 - m12) / w4;
        y = (m02 - m20) / w4;
        z = (m10 - m01) / w4;
    } else if (m00 >= m11 && m00 >= m22) {
        const float s = sqrtf(((1.0f + m00) - m11) - m22) * 2.0f;     // 4x
        w = (m21 - m12) / s;
        x = s / 4.0f;
        y = (m01 + m10) / s;
        z = (m02 + m20) / s;
    } else if (m11 >= m22) {
        const float s = sqrtf(((1.0f + m11) - m00) - m22) * 2.0f;     // 4y
        w = (m02 - m20) / s;
        x = (m01 + m10) / s;
        y = s / 4.0f;
        z = (m12 + m21) / s;
    } else {
        const float s = sqrtf(((1.0f + m22) - m00) - m11) * 2.0f;     // 4z
        w = (m10 - m01) / s;
        x = (m02 + m20) / s;
        y = (m12 + m21) / s;
        z = s / 4.0f;
    }
    if (w < 0.0f) {
        w = -w;
        x = -x;
        y = -y;
        z = -z;
    }
    return make_float4(w, x, y, z);
}

template <bool MOVE>
__global__ __launch_bounds__(HE_THREADS) void hull_edit_kernel(int N, float *__restrict__ means, float4 *__restrict__ quats,
                                                               int F, const double *__restrict__ planes, double tol,
                                                               HullRigid rt, uint8_t *__restrict__ mask,
                                                               unsigned long long *__restrict__ count) {
    extern __shared__ double s_planes[];            // min(F, HE_CHUNK) x 4
    __shared__ unsigned int s_wave[HE_THREADS / GG_WAVE];
    const int i = blockIdx.x * HE_THREADS + threadIdx.x;
    const bool live = i < N;
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f;
    if (live) {
        m0 = means[(size_t)i * 3 + 0];
        m1 = means[(size_t)i * 3 + 1];
        m2 = means[(size_t)i * 3 + 2];
    }
    const double x0 = (double)m0, x1 = (double)m1, x2 = (double)m2;
    bool inside = live;
    for (int c0 = 0; c0 < F; c0 += HE_CHUNK) {
        const int nc = min(HE_CHUNK, F - c0);       // (the __syncthreads_or below ends every read of the last chunk)
        const double *src = planes + (size_t)c0 * 4;
        for (int k = threadIdx.x; k < nc * 4; k += HE_THREADS) s_planes[k] = src[k];
        __syncthreads();
        if (__ballot(inside) != 0ull) {
            for (int k = 0; k < nc; ++k) {
                const double *p = s_planes + 4 * k;
                const double v = ((p[0] * x0 + p[1] * x1) + p[2] * x2) + p[3];
                inside = inside && (v <= tol);      // NaN / inf means: the comparison is false -> outside
                if (__ballot(inside) == 0ull) break;
            }
        }
        if (c0 + nc < F && !__syncthreads_or(inside)) break;     // block-uniform: no lane left inside
    }
    if (live) mask[i] = inside ? 1 : 0;
    const unsigned long long b = __ballot(inside);
    if ((threadIdx.x & (GG_WAVE - 1)) == 0) s_wave[threadIdx.x / GG_WAVE] = (unsigned int)__popcll(b);
    if (MOVE && inside) {
        const float *r = rt.r;
        means[(size_t)i * 3 + 0] = ((r[0] * m0 + r[1] * m1) + r[2] * m2) + r[3];
        means[(size_t)i * 3 + 1] = ((r[4] * m0 + r[5] * m1) + r[6] * m2) + r[7];
        means[(size_t)i * 3 + 2] = ((r[8] * m0 + r[9] * m1) + r[10] * m2) + r[11];
        float Rq[9], M[9];
        he_quat_to_rotmat(quats[i], Rq);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                M[a * 3 + c] = (r[a * 4 + 0] * Rq[c] + r[a * 4 + 1] * Rq[3 + c]) + r[a * 4 + 2] * Rq[6 + c];
        quats[i] = he_rotmat_to_quat(M);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int s = 0;
#pragma unroll
        for (int w = 0; w < HE_THREADS / GG_WAVE; ++w) s += s_wave[w];
        if (s) atomicAdd(count, (unsigned long long)s);
    }
}

extern "C" int gg_hull_edit(int num_points, float *means, float *quats, int num_planes, const double *planes,
                            double tol, const float *rt, uint8_t *mask, int64_t *count_out, gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0, "num_points < 0");
    GG_REQUIRE(num_planes >= 4, "num_planes < 4 (a bounded hull in 3-D has at least 4 facets)");
    GG_REQUIRE(count_out, "null pointer: count_out");
    GG_REQUIRE(((uintptr_t)count_out & 7) == 0, "count_out must be 8-byte aligned");
    GG_REQUIRE(num_points == 0 || (means && planes && mask), "null pointer: means / planes / mask");
    GG_REQUIRE(num_points == 0 || !rt || quats, "null pointer: quats (a transform moves means and quats)");
    GG_REQUIRE(!quats || ((uintptr_t)quats & 15) == 0, "quats must be 16-byte aligned");
    GG_REQUIRE(((uintptr_t)means & 3) == 0 && ((uintptr_t)planes & 7) == 0, "means / planes misaligned");
    HullRigid r{};
    if (rt)
        for (int k = 0; k < 12; ++k) r.r[k] = rt[k];
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = gg_fill_async(count_out, 0, sizeof(int64_t), s);
    if (e != hipSuccess) {
        gg_set_error("%s: zeroing the count failed: %s", __func__, hipGetErrorString(e));
        return GG_ERR_LAUNCH;
    }
    if (num_points == 0) return GG_OK;
    const unsigned blocks = (unsigned)((num_points + HE_THREADS - 1) / HE_THREADS);
    const size_t lds = (size_t)min(num_planes, HE_CHUNK) * 4 * sizeof(double);
    if (rt)
        hipLaunchKernelGGL(hull_edit_kernel<true>, dim3(blocks), dim3(HE_THREADS), lds, s, num_points, means,
                           (float4 *)quats, num_planes, planes, tol, r, mask, (unsigned long long *)count_out);
    else
        hipLaunchKernelGGL(hull_edit_kernel<false>, dim3(blocks), dim3(HE_THREADS), lds, s, num_points, means,
                           (float4 *)quats, num_planes, planes, tol, r, mask, (unsigned long long *)count_out);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
