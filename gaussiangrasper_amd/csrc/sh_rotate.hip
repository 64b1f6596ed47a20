// sh_rotate.hip — the scene update's third array (gaussiangrasper_amd.edit): the spherical-harmonic
// colour coefficients of the moved Gaussians, turned with them.  The lobes are expressed in world axes, so a Gaussian
// moved by R keeps its appearance only if band l of its coefficients is multiplied by that band's (2l+1) x (2l+1)
// rotation matrix D_l (gaussiangrasper_amd/sh_rotation.py builds them for this library's basis).  In place, on the
// mask gg_hull_edit just wrote, on the same stream; nothing waits on the host.
//
// A row is 3 K floats (300 B at K = 25); one lane per row would read and write with that stride.  So a workgroup
// takes SR_ROWS consecutive rows cooperatively: one mask byte per lane, the selected rows compacted into a list
// (ballot + popcount, row order kept), and then the lanes run ACROSS the list's floats — lane e takes float e % RF of
// listed row e / RF, RF = 3 (K - 1), band 0 left out — so a row is read and written as one contiguous piece.  The
// rows are staged whole in LDS (SR_ROWS x RF floats: 36 KB at K = 25) before any output is formed, because every
// output of a band depends on every input of it; the outputs go from registers straight back to global memory, so
// nothing a lane still has to read is overwritten.  D sits in LDS too (164 floats), filled from the kernel arguments.
// A workgroup with no selected row — most of them, for a grasped object — ends after its mask bytes.  No grid cap and
// no loop over tiles: one workgroup per SR_ROWS rows.
#include "gg_common.h"

#pragma clang fp contract(off)

#define SR_THREADS 256
#define SR_ROWS 128           // rows per workgroup: one mask byte each for the first SR_ROWS lanes
#define SR_MAX_BANDS 164      // 9 + 25 + 49 + 81 floats: D_1 .. D_4, row-major, concatenated

struct ShBands {
    float d[SR_MAX_BANDS];
};

template <int K>
__global__ __launch_bounds__(SR_THREADS) void sh_rotate_kernel(int N, float *__restrict__ coeffs,
                                                               const uint8_t *__restrict__ mask, ShBands bands) {
    constexpr int RF = 3 * (K - 1);                 // floats of a row past band 0
    constexpr int ND = K == 4 ? 9 : K == 9 ? 34 : K == 16 ? 83 : 164;
    __shared__ float s_c[SR_ROWS * RF];
    __shared__ float s_d[ND];
    __shared__ int s_rows[SR_ROWS];
    __shared__ int s_cnt[SR_ROWS / GG_WAVE];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * SR_ROWS;
    const long long i = base + tid;
    const bool sel = tid < SR_ROWS && i < N && (mask ? mask[i] != 0 : true);
    const unsigned long long b = __ballot(sel);
    const int lane = tid & (GG_WAVE - 1), wave = tid / GG_WAVE;
    if (wave < SR_ROWS / GG_WAVE && lane == 0) s_cnt[wave] = __popcll(b);
    for (int k = tid; k < ND; k += SR_THREADS) s_d[k] = bands.d[k];
    __syncthreads();
    int total = 0, before = 0;
#pragma unroll
    for (int w = 0; w < SR_ROWS / GG_WAVE; ++w) {
        if (w < wave) before += s_cnt[w];
        total += s_cnt[w];
    }
    if (total == 0) return;                         // block-uniform
    if (sel) s_rows[before + __popcll(b & ((1ull << lane) - 1ull))] = tid;
    __syncthreads();
    const int nf = total * RF;                      // <= SR_ROWS * RF
    for (int e = tid; e < nf; e += SR_THREADS) {
        const int r = e / RF, f = e - r * RF;
        s_c[e] = coeffs[(size_t)(base + s_rows[r]) * (3 * K) + 3 + f];
    }
    __syncthreads();
    for (int e = tid; e < nf; e += SR_THREADS) {
        const int r = e / RF, f = e - r * RF;
        const int a = 1 + f / 3, ch = f - 3 * (a - 1);
        const int l = a < 4 ? 1 : a < 9 ? 2 : a < 16 ? 3 : 4;
        const int lo = l * l, n = 2 * l + 1;
        const int off = l == 1 ? 0 : l == 2 ? 9 : l == 3 ? 34 : 83;
        const float *d = s_d + off + (a - lo) * n;
        const float *c = s_c + r * RF + 3 * (lo - 1) + ch;
        float acc = d[0] * c[0];
        for (int j = 1; j < n; ++j) acc = acc + d[j] * c[3 * j];
        coeffs[(size_t)(base + s_rows[r]) * (3 * K) + 3 + f] = acc;
    }
}

extern "C" int gg_sh_rotate(int num_points, int num_bases, float *coeffs, const uint8_t *mask, const float *bands,
                            gg_stream_t stream) {
    GG_REQUIRE(num_points >= 0, "num_points < 0");
    GG_REQUIRE(num_bases == 1 || num_bases == 4 || num_bases == 9 || num_bases == 16 || num_bases == 25,
               "num_bases must be 1, 4, 9, 16 or 25");
    if (num_points == 0 || num_bases == 1) return GG_OK;      // band 0 does not turn
    GG_REQUIRE(coeffs && bands, "null pointer: coeffs / bands");
    GG_REQUIRE(((uintptr_t)coeffs & 3) == 0, "coeffs misaligned");
    const int nd = num_bases == 4 ? 9 : num_bases == 9 ? 34 : num_bases == 16 ? 83 : SR_MAX_BANDS;
    ShBands d{};
    for (int k = 0; k < nd; ++k) d.d[k] = bands[k];
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(((long long)num_points + SR_ROWS - 1) / SR_ROWS)), block(SR_THREADS);
    switch (num_bases) {
    case 4: hipLaunchKernelGGL(sh_rotate_kernel<4>, grid, block, 0, s, num_points, coeffs, mask, d); break;
    case 9: hipLaunchKernelGGL(sh_rotate_kernel<9>, grid, block, 0, s, num_points, coeffs, mask, d); break;
    case 16: hipLaunchKernelGGL(sh_rotate_kernel<16>, grid, block, 0, s, num_points, coeffs, mask, d); break;
    default: hipLaunchKernelGGL(sh_rotate_kernel<25>, grid, block, 0, s, num_points, coeffs, mask, d); break;
    }
    GG_CHECK_LAUNCH();
    return GG_OK;
}
