// arm.hip — the arm behind the gripper: forward kinematics of a serial chain, inverse kinematics along gripper pose
// paths by damped least squares, and the whole arm's link spheres against the scene's distance field.  The contract is
// in include/gg_raster.h (gg_arm_*) and PARITY.md "Arm reachability"; the design in DESIGN.md §3.31.
//
// gg_arm_fk       a thread per configuration.
// gg_arm_follow   a thread per (path, seed): the waypoints of a path in order, each from the solution of the one
//                 before.  The chain is a kernel argument (scalar loads with constant offsets once the joint loops are
//                 unrolled); per joint the thread keeps the world axis and origin (6 doubles), forms the Jacobian's
//                 columns from them when it needs them, and accumulates J J^T column by column, so that no array is
//                 indexed by a value the compiler does not know.  No thread waits for another, no atomics; the loops
//                 are bounded by num_waypoints and max_iter.
// The three kernels are templates on the joint count J, so every `j < J` is decided when they are compiled, and the
// joint's kind enters by factors of 1 and 0, not by a branch: no condition that is the same for every lane is kept
// across the iteration loop (DESIGN.md §3.31 has the reason).
// gg_arm_clear    a one-wave workgroup per configuration: every lane runs the chain (the same values in all of them),
//                 lane 0 leaves the J + 2 frames in LDS, the lanes stride over the spheres, and a butterfly over
//                 (slack, index) leaves the minimum and the lowest sphere that attains it in every lane.
// gg_arm_self     a one-wave workgroup per configuration: the frames as in clear, then the sphere centres in LDS, the
//                 lanes stride over the pairs s < t in lexicographic order, and a butterfly over (gap, s S + t).
// gg_arm_motion   a one-wave workgroup per edge: the sweep bound B by a butterfly maximum, the sample count n from it
//                 (the same in every lane, read back through readfirstlane so that the sample loop is a scalar loop),
//                 then per sample what clear and self do, and a running (minimum, first sample, index).  Whether
//                 the field and the pairs are tested are template arguments, not conditions kept across the loops.
//
// All arithmetic is fp64 and the file is built with -ffp-contract=off: a composed entry is (a0 b0 + a1 b1) + a2 b2,
// plus t, exactly as the header says.
#include <math.h>

#include <type_traits>

#include "field_volume.h"

#define ARM_THREADS 64
#define ARM_FRAMES (GG_ARM_MAX_JOINTS + 2)

struct ArmChain {
    int J;
    double rev[GG_ARM_MAX_JOINTS], pri[GG_ARM_MAX_JOINTS];       // 1, 0 for a revolute joint; 0, 1 for a prismatic one
    double base[12];
    double fixed[GG_ARM_MAX_JOINTS][12];          // A_j, j < J
    double tip[12];                              // A_J: the last link to the gripper frame
    double axis[GG_ARM_MAX_JOINTS][3];
    double lo[GG_ARM_MAX_JOINTS], hi[GG_ARM_MAX_JOINTS];
};

struct ArmLaw {
    double tol_p, tol_r, L, k, lambda_min, max_step;
    int max_iter;
};

// ---------------------------------------------------------------------------------------------------------------
// the chain
// ---------------------------------------------------------------------------------------------------------------
// T <- T B: R = R_T R_B, t = R_T t_B + t_T; each entry a sum of three products added left to right (plus t).
__device__ __forceinline__ void arm_compose(double *T, const double *B) {
    double o[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * r + c] = (T[3 * r] * B[c] + T[3 * r + 1] * B[3 + c]) + T[3 * r + 2] * B[6 + c];
        o[9 + r] = ((T[3 * r] * B[9] + T[3 * r + 1] * B[10]) + T[3 * r + 2] * B[11]) + T[9 + r];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = o[i];
}

// M_j(q): Rodrigues' rotation about the unit axis a, (I c + (1 - c) a a^T) + s [a]x, or the translation q a.  No
// branch on the joint's kind: with (rev, pri) = (1, 0) or (0, 1) the angle is rev q and the slide pri q, and a factor of
// exactly 1 or 0 changes no bit of a finite value: a prismatic joint gets the rotation of angle 0, which is I, and a
// revolute one the translation 0.  (A kind is the same for every lane; a branch on it, kept across the iteration loop
// while lanes leave it, is the form the compiler was seen to get wrong: DESIGN.md 3.31.)
__device__ __forceinline__ void arm_motion(double rev, double pri, const double *a, double q, double *M) {
    const double ang = rev * q, slide = pri * q;
    const double c = cos(ang), s = sin(ang), v = 1.0 - c;
    M[0] = (c + v * (a[0] * a[0]));
    M[1] = (v * (a[0] * a[1])) + s * (-a[2]);
    M[2] = (v * (a[0] * a[2])) + s * a[1];
    M[3] = (v * (a[1] * a[0])) + s * a[2];
    M[4] = (c + v * (a[1] * a[1]));
    M[5] = (v * (a[1] * a[2])) + s * (-a[0]);
    M[6] = (v * (a[2] * a[0])) + s * (-a[1]);
    M[7] = (v * (a[2] * a[1])) + s * a[0];
    M[8] = (c + v * (a[2] * a[2]));
    M[9] = slide * a[0];
    M[10] = slide * a[1];
    M[11] = slide * a[2];
}

template <int J>
__device__ __forceinline__ bool arm_finite_q(const double *q) {
    bool fin = true;
#pragma unroll
    for (int j = 0; j < J; ++j) fin = fin && isfinite(q[j]);
    return fin;
}

// ---------------------------------------------------------------------------------------------------------------
// fk
// ---------------------------------------------------------------------------------------------------------------
template <int J>
__global__ __launch_bounds__(ARM_THREADS) void arm_fk_kernel(ArmChain arm, int M, const double *__restrict__ q_in,
                                                             double *__restrict__ frames) {
    const int m = blockIdx.x * ARM_THREADS + threadIdx.x;        // M <= 2^26 and the grid covers M: no overflow
    if (m >= M) return;
    double q[GG_ARM_MAX_JOINTS];
#pragma unroll
    for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) q[j] = j < J ? q_in[(size_t)m * J + j] : 0.0;
    double *out = frames + (size_t)m * (J + 2) * 12;
    if (!arm_finite_q<J>(q)) {
        for (int i = 0; i < (J + 2) * 12; ++i) out[i] = __builtin_nan("");
        return;
    }
    double T[12], Mj[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) out[i] = T[i] = arm.base[i];
#pragma unroll
    for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) {
        if (j < J) {
            arm_compose(T, arm.fixed[j]);
            arm_motion(arm.rev[j], arm.pri[j], arm.axis[j], q[j], Mj);
            arm_compose(T, Mj);
#pragma unroll
            for (int i = 0; i < 12; ++i) out[(j + 1) * 12 + i] = T[i];
        }
    }
    arm_compose(T, arm.tip);
#pragma unroll
    for (int i = 0; i < 12; ++i) out[(J + 1) * 12 + i] = T[i];
}

// ---------------------------------------------------------------------------------------------------------------
// follow
// ---------------------------------------------------------------------------------------------------------------
// The rotation vector of a rotation matrix through its quaternion (Shepperd: the largest of trace, R00, R11, R22 is
// the pivot, the first of equals), w >= 0.
__device__ __forceinline__ void arm_rotvec(const double *R, double *e) {
    const double t = (R[0] + R[4]) + R[8];
    double w, x, y, z;
    if (t >= R[0] && t >= R[4] && t >= R[8]) {
        w = 1.0 + t;
        x = R[7] - R[5];
        y = R[2] - R[6];
        z = R[3] - R[1];
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        w = R[7] - R[5];
        x = ((1.0 + R[0]) - R[4]) - R[8];
        y = R[3] + R[1];
        z = R[6] + R[2];
    } else if (R[4] >= R[8]) {
        w = R[2] - R[6];
        x = R[3] + R[1];
        y = ((1.0 + R[4]) - R[8]) - R[0];
        z = R[7] + R[5];
    } else {
        w = R[3] - R[1];
        x = R[6] + R[2];
        y = R[7] + R[5];
        z = ((1.0 + R[8]) - R[0]) - R[4];
    }
    const double n = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / n;
    x = x / n;
    y = y / n;
    z = z / n;
    if (w < 0.0) {
        w = -w;
        x = -x;
        y = -y;
        z = -z;
    }
    const double nv = sqrt((x * x + y * y) + z * z);
    if (nv < 1e-12) {
        e[0] = 2.0 * x;
        e[1] = 2.0 * y;
        e[2] = 2.0 * z;
    } else {
        const double ang = 2.0 * atan2(nv, w);
        e[0] = ang * (x / nv);
        e[1] = ang * (y / nv);
        e[2] = ang * (z / nv);
    }
}

// Column j of the geometric Jacobian with its rotational rows scaled by L, from the joint's world axis z and origin o
// and the gripper's position p: [z x (p - o); L z] for a revolute joint, [z; 0] for a prismatic one, by factors of 1 and 0.
__device__ __forceinline__ void arm_column(double rev, double pri, const double *z, const double *o, const double *p,
                                           double L, double *c) {
    const double d0 = p[0] - o[0], d1 = p[1] - o[1], d2 = p[2] - o[2];
    c[0] = rev * (z[1] * d2 - z[2] * d1) + pri * z[0];
    c[1] = rev * (z[2] * d0 - z[0] * d2) + pri * z[1];
    c[2] = rev * (z[0] * d1 - z[1] * d0) + pri * z[2];
    c[3] = rev * (L * z[0]);
    c[4] = rev * (L * z[1]);
    c[5] = rev * (L * z[2]);
}

template <int J>
__global__ __launch_bounds__(ARM_THREADS) void arm_follow_kernel(ArmChain arm, ArmLaw law, int P, int W, int S,
                                                                 const float *__restrict__ poses,
                                                                 const double *__restrict__ seeds,
                                                                 double *__restrict__ q_out, int *__restrict__ iters,
                                                                 double *__restrict__ resid,
                                                                 int *__restrict__ first_fail) {
    const int i = blockIdx.x * ARM_THREADS + threadIdx.x;        // P S <= 2^26
    if (i >= P * S) return;
    const int path = i / S;
    double q[GG_ARM_MAX_JOINTS];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) {
        q[j] = 0.0;
        if (j < J) {
            const double v = seeds[(size_t)i * J + j];
            ok = ok && isfinite(v);
            q[j] = fmin(fmax(v, arm.lo[j]), arm.hi[j]);
        }
    }
    int w = 0;
    for (; w < W && ok; ++w) {
        double Rt[9], pt[3];                                     // the target
        const float *pose = poses + ((size_t)path * W + w) * 12;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float v = pose[k];
            ok = ok && isfinite(v);
            Rt[k] = (double)v;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = pose[9 + k];
            ok = ok && isfinite(v);
            pt[k] = (double)v;
        }
        if (!ok) break;
        int it = 0;
        double np_ = 0.0, nr_ = 0.0;
        for (;;) {
            // FK, keeping every joint's world axis and origin
            double T[12], Mj[12], zs[GG_ARM_MAX_JOINTS][3], os[GG_ARM_MAX_JOINTS][3];
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = arm.base[k];
#pragma unroll
            for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) {
                if (j < J) {
                    arm_compose(T, arm.fixed[j]);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        zs[j][k] = (T[3 * k] * arm.axis[j][0] + T[3 * k + 1] * arm.axis[j][1]) + T[3 * k + 2] * arm.axis[j][2];
                        os[j][k] = T[9 + k];
                    }
                    arm_motion(arm.rev[j], arm.pri[j], arm.axis[j], q[j], Mj);
                    arm_compose(T, Mj);
                }
            }
            arm_compose(T, arm.tip);
            // the error
            double e[6], Re[9], er[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) e[k] = pt[k] - T[9 + k];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    Re[3 * a + b] = (Rt[3 * a] * T[3 * b] + Rt[3 * a + 1] * T[3 * b + 1]) + Rt[3 * a + 2] * T[3 * b + 2];
            arm_rotvec(Re, er);
            np_ = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
            nr_ = sqrt((er[0] * er[0] + er[1] * er[1]) + er[2] * er[2]);
            if (!(isfinite(np_) && isfinite(nr_))) {
                ok = false;
                break;
            }
            if (np_ <= law.tol_p && nr_ <= law.tol_r) break;     // converged
            if (it == law.max_iter) {
                ok = false;
                break;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) e[3 + k] = law.L * er[k];
            double ee = e[0] * e[0];
#pragma unroll
            for (int k = 1; k < 6; ++k) ee = ee + e[k] * e[k];
            const double lambda2 = law.k * ee + law.lambda_min * law.lambda_min;
            // A = J J^T + lambda2 I (lower triangle), a column at a time
            double A[6][6];
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) A[a][b] = 0.0;
#pragma unroll
            for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) {
                if (j < J) {
                    double c[6];
                    arm_column(arm.rev[j], arm.pri[j], zs[j], os[j], T + 9, law.L, c);
#pragma unroll
                    for (int a = 0; a < 6; ++a)
#pragma unroll
                        for (int b = 0; b <= a; ++b) A[a][b] = A[a][b] + c[a] * c[b];
                }
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) A[a][a] = A[a][a] + lambda2;
            // Cholesky in place, then the two triangular solves
            bool pd = true;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    double s = A[a][b];
#pragma unroll
                    for (int k = 0; k < b; ++k) s = s - A[a][k] * A[b][k];
                    if (a == b) {
                        pd = pd && s > 0.0;
                        A[a][a] = sqrt(s);
                    } else {
                        A[a][b] = s / A[b][b];
                    }
                }
            }
            if (!pd) {
                ok = false;
                break;
            }
            double y[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double s = e[a];
#pragma unroll
                for (int k = 0; k < a; ++k) s = s - A[a][k] * y[k];
                y[a] = s / A[a][a];
            }
#pragma unroll
            for (int a = 5; a >= 0; --a) {
                double s = y[a];
#pragma unroll
                for (int k = a + 1; k < 6; ++k) s = s - A[k][a] * y[k];
                y[a] = s / A[a][a];
            }
            // dq = J^T y, limited to max_step
            double dq[GG_ARM_MAX_JOINTS], big = 0.0;
            bool fin = true;
#pragma unroll
            for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) {
                dq[j] = 0.0;
                if (j < J) {
                    double c[6];
                    arm_column(arm.rev[j], arm.pri[j], zs[j], os[j], T + 9, law.L, c);
                    double s = c[0] * y[0];
#pragma unroll
                    for (int k = 1; k < 6; ++k) s = s + c[k] * y[k];
                    dq[j] = s;
                    fin = fin && isfinite(s);
                    big = fmax(big, fabs(s));
                }
            }
            if (!fin) {
                ok = false;
                break;
            }
            const double scale = big > law.max_step ? law.max_step / big : 1.0;
#pragma unroll
            for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j)
                if (j < J) {
                    const double step = big > law.max_step ? dq[j] * scale : dq[j];
                    q[j] = fmin(fmax(q[j] + step, arm.lo[j]), arm.hi[j]);
                }
            ++it;
        }
        if (!ok) break;
        const size_t at = (size_t)i * W + w;
#pragma unroll
        for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j)
            if (j < J) q_out[at * J + j] = q[j];
        iters[at] = it;
        resid[at * 2] = np_;
        resid[at * 2 + 1] = nr_;
    }
    // w: the failed waypoint, or W
    first_fail[i] = w;
    for (int v = w; v < W; ++v) {
        const size_t at = (size_t)i * W + v;
        for (int j = 0; j < J; ++j) q_out[at * J + j] = __builtin_nan("");
        iters[at] = -1;
        resid[at * 2] = __builtin_nan("");
        resid[at * 2 + 1] = __builtin_nan("");
    }
}

// ---------------------------------------------------------------------------------------------------------------
// clear
// ---------------------------------------------------------------------------------------------------------------
template <int J>
__global__ __launch_bounds__(GG_WAVE) void arm_clear_kernel(ArmChain arm, FieldGrid g, const int *__restrict__ dist2,
                                                            int M, const double *__restrict__ q_in, int S,
                                                            const float *__restrict__ spheres,
                                                            const int *__restrict__ frame,
                                                            const int *__restrict__ need2, int outside,
                                                            int *__restrict__ slack, int *__restrict__ worst) {
    __shared__ double s_frames[ARM_FRAMES * 12];
    const int m = blockIdx.x;                                    // one wave, one configuration; the grid is M
    const int lane = threadIdx.x;
    double q[GG_ARM_MAX_JOINTS];
#pragma unroll
    for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) q[j] = j < J ? q_in[(size_t)m * J + j] : 0.0;
    if (!arm_finite_q<J>(q)) {                                 // the same in every lane of the wave
        if (lane == 0) {
            slack[m] = INT32_MIN;
            worst[m] = -1;
        }
        return;
    }
    {
        double T[12], Mj[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = arm.base[i];
        if (lane == 0)
#pragma unroll
            for (int i = 0; i < 12; ++i) s_frames[i] = T[i];
#pragma unroll
        for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) {
            if (j < J) {
                arm_compose(T, arm.fixed[j]);
                arm_motion(arm.rev[j], arm.pri[j], arm.axis[j], q[j], Mj);
                arm_compose(T, Mj);
                if (lane == 0)
#pragma unroll
                    for (int i = 0; i < 12; ++i) s_frames[(j + 1) * 12 + i] = T[i];
            }
        }
        arm_compose(T, arm.tip);
        if (lane == 0)
#pragma unroll
            for (int i = 0; i < 12; ++i) s_frames[(J + 1) * 12 + i] = T[i];
    }
    __syncthreads();                                             // a one-wave workgroup: the LDS writes are done
    int best = GG_FIELD_FAR, who = INT32_MAX;
    for (int s = lane; s < S; s += GG_WAVE) {
        const int f = min(max(frame[s], 0), J + 1);              // the caller keeps it in 0..J+1; no read leaves LDS
        const int d = field_probe(g, dist2, s_frames + f * 12, (double)spheres[3 * s], (double)spheres[3 * s + 1],
                                  (double)spheres[3 * s + 2], outside);
        const int sl = d - need2[s];
        if (sl < best || (sl == best && s < who)) best = sl, who = s;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int ob = __shfl_xor(best, off, GG_WAVE), ow = __shfl_xor(who, off, GG_WAVE);
        if (ob < best || (ob == best && ow < who)) best = ob, who = ow;
    }
    if (lane == 0) {
        slack[m] = best;
        worst[m] = who == INT32_MAX ? -1 : who;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// self and motion
// ---------------------------------------------------------------------------------------------------------------
// Which frame pairs are tested, as bits: bit f (J_MAX + 2) + g of the 100.  A kernel argument that lanes index with
// their own f and g; two words and a shift need no array.
struct ArmPairs {
    unsigned long long lo, hi;
    __device__ __forceinline__ bool on(int f, int g) const {
        const int b = f * ARM_FRAMES + g;
        return ((b < 64 ? lo >> b : hi >> (b - 64)) & 1ull) != 0;
    }
};

// The dynamic LDS of one workgroup: the J + 2 frames, then per sphere the world centre (3 doubles) and the radius, then
// the spheres' frames as bytes.
struct ArmLds {
    double *frames, *centre, *radius;
    unsigned char *frame_of;
};

__device__ __forceinline__ ArmLds arm_lds(double *base, int S) {
    ArmLds l;
    l.frames = base;
    l.centre = base + ARM_FRAMES * 12;
    l.radius = l.centre + 3 * (size_t)S;
    l.frame_of = (unsigned char *)(l.radius + S);
    return l;
}

static size_t arm_lds_bytes(int S) { return (size_t)(ARM_FRAMES * 12 + 4 * S) * sizeof(double) + (size_t)S; }

// What a workgroup reads of the sphere table once: the frame of every sphere, clamped into 0..J + 1 as clear clamps it,
// and the radii when the pairs are tested.
template <int J, bool SELF>
__device__ __forceinline__ void arm_stage_spheres(const ArmLds &l, int lane, int S, const int *__restrict__ frame,
                                                  const double *__restrict__ radius) {
    for (int s = lane; s < S; s += GG_WAVE) {
        l.frame_of[s] = (unsigned char)min(max(frame[s], 0), J + 1);
        if (SELF) l.radius[s] = radius[s];
    }
}

// Every lane runs the chain of q (the same values in all of them); lane 0 leaves F_0 .. F_{J+1} in LDS.
template <int J>
__device__ __forceinline__ void arm_frames_to_lds(const ArmChain &arm, const double *q, int lane, double *s_frames) {
    double T[12], Mj[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = arm.base[i];
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 12; ++i) s_frames[i] = T[i];
#pragma unroll
    for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) {
        if (j < J) {
            arm_compose(T, arm.fixed[j]);
            arm_motion(arm.rev[j], arm.pri[j], arm.axis[j], q[j], Mj);
            arm_compose(T, Mj);
            if (lane == 0)
#pragma unroll
                for (int i = 0; i < 12; ++i) s_frames[(j + 1) * 12 + i] = T[i];
        }
    }
    arm_compose(T, arm.tip);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 12; ++i) s_frames[(J + 1) * 12 + i] = T[i];
}

// One configuration whose frames are in LDS: the lanes stride over the spheres; with FIELD the probe of clear and the
// butterfly over (slack, sphere); with SELF the world centres go to LDS, in the probe's own operation order.
template <bool FIELD, bool SELF>
__device__ __forceinline__ void arm_sphere_pass(const ArmLds &l, const FieldGrid &g, const int *__restrict__ dist2,
                                                int lane, int S, const float *__restrict__ spheres,
                                                const int *__restrict__ need2, int outside, int *slack, int *worst) {
    int best = GG_FIELD_FAR, who = INT32_MAX;
    for (int s = lane; s < S; s += GG_WAVE) {
        const double *T = l.frames + (int)l.frame_of[s] * 12;
        const double x = (double)spheres[3 * s], y = (double)spheres[3 * s + 1], z = (double)spheres[3 * s + 2];
        if (FIELD) {
            const int sl = field_probe(g, dist2, T, x, y, z, outside) - need2[s];
            if (sl < best || (sl == best && s < who)) best = sl, who = s;
        }
        if (SELF) {
#pragma unroll
            for (int a = 0; a < 3; ++a) l.centre[3 * s + a] = ((T[3 * a] * x + T[3 * a + 1] * y) + T[3 * a + 2] * z) + T[9 + a];
        }
    }
    if (FIELD) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const int ob = __shfl_xor(best, off, GG_WAVE), ow = __shfl_xor(who, off, GG_WAVE);
            if (ob < best || (ob == best && ow < who)) best = ob, who = ow;
        }
    }
    *slack = best;
    *worst = who == INT32_MAX ? -1 : who;
}

// The centres are in LDS: lane l takes the pairs l, l + 64, ... of the lexicographic order of (s, t), s < t, walking
// (s, t) forward row by row; the butterfly over (gap, s S + t) leaves the minimum and the lowest pair that attains it
// in every lane.  key INT32_MAX: no tested pair.
__device__ __forceinline__ void arm_pair_pass(const ArmLds &l, const ArmPairs &pairs, int lane, int S, double *gap,
                                              int *key) {
    double best = __builtin_inf();
    int who = INT32_MAX;
    int s = 0, t = 1 + lane;
    for (;;) {
        while (t >= S && s < S - 1) {                            // past the end of row s: on into row s + 1
            t -= S;
            ++s;
            t += s + 1;
        }
        if (s >= S - 1) break;
        if (pairs.on((int)l.frame_of[s], (int)l.frame_of[t])) {
            const double dx = l.centre[3 * s] - l.centre[3 * t], dy = l.centre[3 * s + 1] - l.centre[3 * t + 1],
                         dz = l.centre[3 * s + 2] - l.centre[3 * t + 2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            const double gp = sqrt(d2) - (l.radius[s] + l.radius[t]);
            const int k = s * S + t;
            if (gp < best || (gp == best && k < who)) best = gp, who = k;
        }
        t += GG_WAVE;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off, GG_WAVE);
        const int ow = __shfl_xor(who, off, GG_WAVE);
        if (ob < best || (ob == best && ow < who)) best = ob, who = ow;
    }
    *gap = best;
    *key = who;
}

template <int J>
__global__ __launch_bounds__(GG_WAVE) void arm_self_kernel(ArmChain arm, ArmPairs pairs, int M,
                                                           const double *__restrict__ q_in, int S,
                                                           const float *__restrict__ spheres,
                                                           const int *__restrict__ frame,
                                                           const double *__restrict__ radius, double *__restrict__ gap,
                                                           int *__restrict__ pair) {
    extern __shared__ double arm_dyn[];
    const ArmLds l = arm_lds(arm_dyn, S);
    const int m = blockIdx.x;                                    // one wave, one configuration; the grid is M
    const int lane = threadIdx.x;
    double q[GG_ARM_MAX_JOINTS];
#pragma unroll
    for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) q[j] = j < J ? q_in[(size_t)m * J + j] : 0.0;
    if (!arm_finite_q<J>(q)) {                                 // the same in every lane of the wave
        if (lane == 0) {
            gap[m] = __builtin_nan("");
            pair[2 * (size_t)m] = -1;
            pair[2 * (size_t)m + 1] = -1;
        }
        return;
    }
    arm_stage_spheres<J, true>(l, lane, S, frame, radius);
    arm_frames_to_lds<J>(arm, q, lane, l.frames);
    __syncthreads();                                             // a one-wave workgroup: the LDS writes are done
    int unused_slack, unused_worst;
    arm_sphere_pass<false, true>(l, FieldGrid{}, nullptr, lane, S, spheres, nullptr, 0, &unused_slack, &unused_worst);
    __syncthreads();
    double gp;
    int key;
    arm_pair_pass(l, pairs, lane, S, &gp, &key);
    if (lane == 0) {
        gap[m] = gp;
        pair[2 * (size_t)m] = key == INT32_MAX ? -1 : key / S;
        pair[2 * (size_t)m + 1] = key == INT32_MAX ? -1 : key % S;
    }
}

struct ArmMotionOut {
    int *samples, *slack, *slack_at, *worst;
    double *gap;
    int *gap_at, *pair;
};

template <int J, bool FIELD, bool SELF>
__global__ __launch_bounds__(GG_WAVE) void arm_motion_kernel(ArmChain arm, ArmPairs pairs, FieldGrid g,
                                                             const int *__restrict__ dist2, int E,
                                                             const double *__restrict__ q_a,
                                                             const double *__restrict__ q_b, int S,
                                                             const float *__restrict__ spheres,
                                                             const int *__restrict__ frame,
                                                             const int *__restrict__ need2, int outside,
                                                             const double *__restrict__ radius,
                                                             const double *__restrict__ reach, double res,
                                                             int max_samples, ArmMotionOut out) {
    extern __shared__ double arm_dyn[];
    const ArmLds l = arm_lds(arm_dyn, S);
    const int e = blockIdx.x;                                    // one wave, one edge; the grid is E
    const int lane = threadIdx.x;
    double qa[GG_ARM_MAX_JOINTS], dq[GG_ARM_MAX_JOINTS], qb[GG_ARM_MAX_JOINTS];
#pragma unroll
    for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) {
        qa[j] = j < J ? q_a[(size_t)e * J + j] : 0.0;
        qb[j] = j < J ? q_b[(size_t)e * J + j] : 0.0;
    }
    // the sweep bound: b_s with j ascending from 0.0, B their maximum (exact, so the butterfly's order does not matter)
    double B = 0.0;
    int n = 0;
#pragma unroll
    for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) dq[j] = qb[j] - qa[j];
    // the same in every lane of the wave, and a scalar: no lane mask of it lives across the loops below
    if (__builtin_amdgcn_readfirstlane((int)(arm_finite_q<J>(qa) && arm_finite_q<J>(qb)))) {
        for (int s = lane; s < S; s += GG_WAVE) {
            double b = 0.0;
#pragma unroll
            for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j)
                if (j < J) b = b + fabs(dq[j]) * reach[(size_t)j * S + s];
            B = fmax(B, b);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) B = fmax(B, __shfl_xor(B, off, GG_WAVE));
        if (!(B > (double)max_samples * res)) {
            // the smallest n >= 1 with n res >= B: the division proposes, the comparisons decide
            const double guess = ceil(B / res);
            n = guess >= 1.0 ? (guess <= (double)max_samples ? (int)guess : max_samples) : 1;
            while (n < max_samples && (double)n * res < B) ++n;
            while (n > 1 && (double)(n - 1) * res >= B) --n;
        }
    }
    n = __builtin_amdgcn_readfirstlane(n);                       // a scalar: the sample loop is the same for the wave
    if (n == 0) {                                                // not finite, or not resolved by max_samples
        if (lane == 0) {
            out.samples[e] = 0;
            out.slack[e] = INT32_MIN;
            out.slack_at[e] = out.worst[e] = out.gap_at[e] = -1;
            out.gap[e] = __builtin_nan("");
            out.pair[2 * (size_t)e] = out.pair[2 * (size_t)e + 1] = -1;
        }
        return;
    }
    arm_stage_spheres<J, SELF>(l, lane, S, frame, radius);
    int slack = INT32_MAX, slack_at = 0, worst = -1, gap_at = 0, gap_key = INT32_MAX;
    double gap = __builtin_inf();
    for (int i = 0; i <= n; ++i) {
        double q[GG_ARM_MAX_JOINTS];
        const double f = (double)i / (double)n;
#pragma unroll
        for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) q[j] = i == n ? qb[j] : qa[j] + f * dq[j];
        arm_frames_to_lds<J>(arm, q, lane, l.frames);
        __syncthreads();                                         // frames (and, at i == 0, the sphere table) are in LDS
        int sl, wo;
        arm_sphere_pass<FIELD, SELF>(l, g, dist2, lane, S, spheres, need2, outside, &sl, &wo);
        if (FIELD && sl < slack) slack = sl, slack_at = i, worst = wo;
        __syncthreads();                                         // the centres are in LDS; the frames may be rewritten
        if (SELF) {
            double gp;
            int key;
            arm_pair_pass(l, pairs, lane, S, &gp, &key);
            if (gp < gap) gap = gp, gap_at = i, gap_key = key;
        }
    }
    if (lane == 0) {
        out.samples[e] = n;
        out.slack[e] = FIELD ? slack : GG_FIELD_FAR;
        out.slack_at[e] = FIELD ? slack_at : -1;
        out.worst[e] = FIELD ? worst : -1;
        out.gap[e] = gap;
        out.gap_at[e] = SELF ? gap_at : -1;
        out.pair[2 * (size_t)e] = gap_key == INT32_MAX ? -1 : gap_key / S;
        out.pair[2 * (size_t)e + 1] = gap_key == INT32_MAX ? -1 : gap_key % S;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------
static bool arm_rotation_ok(const double *T) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double d = (T[a] * T[b] + T[3 + a] * T[3 + b]) + T[6 + a] * T[6 + b];
            if (!(fabs(d - (a == b ? 1.0 : 0.0)) <= 1e-9)) return false;
        }
    return true;
}

#define ARM_REFUSE(...)                   \
    do {                                  \
        gg_set_error(__VA_ARGS__);        \
        return false;                     \
    } while (0)

// The host array `arm` as the kernels' argument; false (and the error set) for an arm the header refuses.
static bool arm_chain(const char *who, int num_joints, const double *arm, ArmChain *c) {
    if (num_joints < 1 || num_joints > GG_ARM_MAX_JOINTS)
        ARM_REFUSE("%s: num_joints must be in 1..GG_ARM_MAX_JOINTS", who);
    if (!arm) ARM_REFUSE("%s: null pointer: arm (a host array of GG_ARM_DOUBLES(num_joints) doubles)", who);
    const int J = num_joints;
    for (int i = 0; i < GG_ARM_DOUBLES(J); ++i)
        if (!isfinite(arm[i])) ARM_REFUSE("%s: arm: entry %d is not finite", who, i);
    *c = ArmChain{};
    c->J = J;
    for (int i = 0; i < 12; ++i) c->base[i] = arm[i];
    if (!arm_rotation_ok(c->base)) ARM_REFUSE("%s: arm: base: |R^T R - I|max > 1e-9", who);
    for (int j = 0; j <= J; ++j) {
        double *A = j < J ? c->fixed[j] : c->tip;
        for (int i = 0; i < 12; ++i) A[i] = arm[12 + 12 * j + i];
        if (!arm_rotation_ok(A)) ARM_REFUSE("%s: arm: fixed[%d]: |R^T R - I|max > 1e-9", who, j);
    }
    const double *joints = arm + 12 * (J + 2);
    for (int j = 0; j < J; ++j) {
        const double *r = joints + 6 * j;
        const double n2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
        if (!(fabs(n2 - 1.0) <= 1e-9)) ARM_REFUSE("%s: arm: axis[%d]: the squared length is off 1 by more than 1e-9", who, j);
        if (r[3] > r[4]) ARM_REFUSE("%s: arm: joint %d: lo > hi", who, j);
        if (r[5] != 0.0 && r[5] != 1.0) ARM_REFUSE("%s: arm: kind[%d] must be 0 (revolute) or 1 (prismatic)", who, j);
        for (int k = 0; k < 3; ++k) c->axis[j][k] = r[k];
        c->lo[j] = r[3];
        c->hi[j] = r[4];
        c->rev[j] = r[5] == 0.0 ? 1.0 : 0.0;
        c->pri[j] = r[5] == 0.0 ? 0.0 : 1.0;
    }
    return true;
}

// The kernels are templates on the joint count: every `j < J` is decided when they are compiled.
template <typename F>
static void arm_dispatch(int J, F &&launch) {
    switch (J) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 3: launch(std::integral_constant<int, 3>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 5: launch(std::integral_constant<int, 5>{}); break;
        case 6: launch(std::integral_constant<int, 6>{}); break;
        case 7: launch(std::integral_constant<int, 7>{}); break;
        default: launch(std::integral_constant<int, 8>{}); break;
    }
}

extern "C" int gg_arm_fk(int num_joints, const double *arm, int num_rows, const double *q, double *frames,
                         gg_stream_t stream) {
    ArmChain c;
    if (!arm_chain(__func__, num_joints, arm, &c)) return GG_ERR_INVALID_ARG;
    GG_REQUIRE(num_rows >= 0 && num_rows <= GG_FIELD_MAX_POSES, "need 0 <= num_rows <= GG_FIELD_MAX_POSES");
    if (num_rows == 0) return GG_OK;
    GG_REQUIRE(q && frames, "null pointer: q / frames");
    GG_REQUIRE((((uintptr_t)q | (uintptr_t)frames) & 7) == 0, "q / frames misaligned");
    arm_dispatch(num_joints, [&](auto joints) {
        hipLaunchKernelGGL((arm_fk_kernel<decltype(joints)::value>),
                           dim3((unsigned)((num_rows + ARM_THREADS - 1) / ARM_THREADS)), dim3(ARM_THREADS), 0,
                           (hipStream_t)stream, c, num_rows, q, frames);
    });
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_arm_follow(int num_joints, const double *arm, int num_paths, int num_waypoints, const float *poses,
                             int num_seeds, const double *seeds, double tol_p, double tol_r, double rot_length,
                             double gain, double lambda_min, double max_step, int max_iter, double *q_out,
                             int32_t *iters, double *resid, int32_t *first_fail, gg_stream_t stream) {
    ArmChain c;
    if (!arm_chain(__func__, num_joints, arm, &c)) return GG_ERR_INVALID_ARG;
    GG_REQUIRE(num_paths >= 0 && num_waypoints >= 0 && num_seeds >= 0, "num_paths / num_waypoints / num_seeds < 0");
    GG_REQUIRE((int64_t)num_paths * num_seeds <= GG_FIELD_MAX_POSES &&
                   (int64_t)num_paths * num_seeds * (int64_t)(num_waypoints > 0 ? num_waypoints : 1) <= GG_FIELD_MAX_POSES,
               "num_paths num_seeds num_waypoints > GG_FIELD_MAX_POSES");
    GG_REQUIRE(isfinite(tol_p) && tol_p >= 0.0, "tol_p must be finite and >= 0");
    GG_REQUIRE(isfinite(tol_r) && tol_r >= 0.0, "tol_r must be finite and >= 0");
    GG_REQUIRE(isfinite(rot_length) && rot_length > 0.0, "rot_length must be finite and > 0");
    GG_REQUIRE(isfinite(gain) && gain >= 0.0, "gain must be finite and >= 0");
    GG_REQUIRE(isfinite(lambda_min) && lambda_min > 0.0, "lambda_min must be finite and > 0");
    GG_REQUIRE(isfinite(max_step) && max_step > 0.0, "max_step must be finite and > 0");
    GG_REQUIRE(max_iter >= 0 && max_iter <= GG_ARM_MAX_ITER, "max_iter must be in 0..GG_ARM_MAX_ITER");
    if (num_paths == 0 || num_seeds == 0) return GG_OK;
    GG_REQUIRE(seeds && first_fail, "null pointer: seeds / first_fail");
    GG_REQUIRE(num_waypoints == 0 || (poses && q_out && iters && resid), "null pointer: poses / q_out / iters / resid");
    GG_REQUIRE((((uintptr_t)seeds | (uintptr_t)q_out | (uintptr_t)resid) & 7) == 0 &&
                   (((uintptr_t)poses | (uintptr_t)iters | (uintptr_t)first_fail) & 3) == 0,
               "poses / seeds / q_out / iters / resid / first_fail misaligned");
    const ArmLaw law{tol_p, tol_r, rot_length, gain, lambda_min, max_step, max_iter};
    const int total = num_paths * num_seeds;
    arm_dispatch(num_joints, [&](auto joints) {
        hipLaunchKernelGGL((arm_follow_kernel<decltype(joints)::value>),
                           dim3((unsigned)((total + ARM_THREADS - 1) / ARM_THREADS)), dim3(ARM_THREADS), 0,
                           (hipStream_t)stream, c, law, num_paths, num_waypoints, num_seeds, poses, seeds, q_out, iters,
                           resid, first_fail);
    });
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_arm_clear(int num_joints, const double *arm, const int32_t *dims, const double *grid,
                            const int32_t *dist2, int num_rows, const double *q, int num_spheres, const float *spheres,
                            const int32_t *frame, const int32_t *need2, int32_t outside, int32_t *slack,
                            int32_t *worst, gg_stream_t stream) {
    ArmChain c;
    if (!arm_chain(__func__, num_joints, arm, &c)) return GG_ERR_INVALID_ARG;
    GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
    GG_REQUIRE(grid, "null pointer: grid (a host array of 4 doubles)");
    FieldGrid g;
    GG_REQUIRE(field_grid(dims, grid, &g), FIELD_GRID_MSG);
    GG_REQUIRE(num_rows >= 0 && num_rows <= GG_FIELD_MAX_POSES, "need 0 <= num_rows <= GG_FIELD_MAX_POSES");
    GG_REQUIRE(num_spheres >= 0 && num_spheres <= GG_FIELD_MAX_SPHERES,
               "num_spheres must be in 0..GG_FIELD_MAX_SPHERES");
    GG_REQUIRE(outside >= 0 && outside <= GG_FIELD_FAR, "outside must be in 0..GG_FIELD_FAR");
    if (num_rows == 0) return GG_OK;
    GG_REQUIRE(dist2 && q && slack && worst, "null pointer: dist2 / q / slack / worst");
    GG_REQUIRE(num_spheres == 0 || (spheres && frame && need2), "null pointer: spheres / frame / need2");
    GG_REQUIRE(((uintptr_t)q & 7) == 0 && (((uintptr_t)dist2 | (uintptr_t)spheres | (uintptr_t)frame |
                                            (uintptr_t)need2 | (uintptr_t)slack | (uintptr_t)worst) & 3) == 0,
               "dist2 / q / spheres / frame / need2 / slack / worst misaligned");
    arm_dispatch(num_joints, [&](auto joints) {
        hipLaunchKernelGGL((arm_clear_kernel<decltype(joints)::value>), dim3((unsigned)num_rows), dim3(GG_WAVE), 0,
                           (hipStream_t)stream, c, g, dist2, num_rows, q, num_spheres, spheres, frame, need2, outside,
                           slack, worst);
    });
    GG_CHECK_LAUNCH();
    return GG_OK;
}

// The host table `pairs` [(J + 2)][(J + 2)] as the kernels' bits; null: nothing is tested.
static ArmPairs arm_pairs(int J, const uint8_t *pairs) {
    ArmPairs p{0ull, 0ull};
    if (!pairs) return p;
    for (int f = 0; f < J + 2; ++f)
        for (int g = 0; g < J + 2; ++g)
            if (pairs[f * (J + 2) + g]) {
                const int b = f * ARM_FRAMES + g;
                (b < 64 ? p.lo : p.hi) |= 1ull << (b & 63);
            }
    return p;
}

extern "C" int gg_arm_self(int num_joints, const double *arm, int num_rows, const double *q, int num_spheres,
                           const float *spheres, const int32_t *frame, const double *radius, const uint8_t *pairs,
                           double *gap, int32_t *pair, gg_stream_t stream) {
    ArmChain c;
    if (!arm_chain(__func__, num_joints, arm, &c)) return GG_ERR_INVALID_ARG;
    GG_REQUIRE(num_rows >= 0 && num_rows <= GG_FIELD_MAX_POSES, "need 0 <= num_rows <= GG_FIELD_MAX_POSES");
    GG_REQUIRE(num_spheres >= 0 && num_spheres <= GG_ARM_MAX_SELF_SPHERES,
               "num_spheres must be in 0..GG_ARM_MAX_SELF_SPHERES");
    GG_REQUIRE(pairs, "null pointer: pairs (a host array of (num_joints + 2)^2 bytes)");
    if (num_rows == 0) return GG_OK;
    GG_REQUIRE(q && gap && pair, "null pointer: q / gap / pair");
    GG_REQUIRE(num_spheres == 0 || (spheres && frame && radius), "null pointer: spheres / frame / radius");
    GG_REQUIRE((((uintptr_t)q | (uintptr_t)radius | (uintptr_t)gap) & 7) == 0 &&
                   (((uintptr_t)spheres | (uintptr_t)frame | (uintptr_t)pair) & 3) == 0,
               "q / radius / gap / spheres / frame / pair misaligned");
    const ArmPairs p = arm_pairs(num_joints, pairs);
    arm_dispatch(num_joints, [&](auto joints) {
        hipLaunchKernelGGL((arm_self_kernel<decltype(joints)::value>), dim3((unsigned)num_rows), dim3(GG_WAVE),
                           arm_lds_bytes(num_spheres), (hipStream_t)stream, c, p, num_rows, q, num_spheres, spheres,
                           frame, radius, gap, pair);
    });
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_arm_motion(int num_joints, const double *arm, const int32_t *dims, const double *grid,
                             const int32_t *dist2, int num_edges, const double *q_a, const double *q_b,
                             int num_spheres, const float *spheres, const int32_t *frame, const int32_t *need2,
                             int32_t outside, const double *radius, const uint8_t *pairs, const double *reach,
                             double res, int max_samples, int32_t *samples, int32_t *slack, int32_t *slack_at,
                             int32_t *worst, double *gap, int32_t *gap_at, int32_t *pair, gg_stream_t stream) {
    ArmChain c;
    if (!arm_chain(__func__, num_joints, arm, &c)) return GG_ERR_INVALID_ARG;
    FieldGrid g{};
    if (dist2) {
        GG_REQUIRE(field_dims_ok(dims), FIELD_DIMS_MSG);
        GG_REQUIRE(grid, "null pointer: grid (a host array of 4 doubles)");
        GG_REQUIRE(field_grid(dims, grid, &g), FIELD_GRID_MSG);
        GG_REQUIRE(outside >= 0 && outside <= GG_FIELD_FAR, "outside must be in 0..GG_FIELD_FAR");
    }
    GG_REQUIRE(num_edges >= 0 && num_edges <= GG_FIELD_MAX_POSES, "need 0 <= num_edges <= GG_FIELD_MAX_POSES");
    GG_REQUIRE(num_spheres >= 0 && num_spheres <= GG_ARM_MAX_SELF_SPHERES,
               "num_spheres must be in 0..GG_ARM_MAX_SELF_SPHERES");
    GG_REQUIRE(isfinite(res) && res > 0.0, "res must be finite and > 0");
    GG_REQUIRE(max_samples >= 1 && max_samples <= GG_ARM_MAX_SAMPLES, "max_samples must be in 1..GG_ARM_MAX_SAMPLES");
    if (num_edges == 0) return GG_OK;
    GG_REQUIRE(q_a && q_b, "null pointer: q_a / q_b");
    GG_REQUIRE(samples && slack && slack_at && worst && gap && gap_at && pair,
               "null pointer: samples / slack / slack_at / worst / gap / gap_at / pair");
    GG_REQUIRE(num_spheres == 0 || (spheres && frame && reach), "null pointer: spheres / frame / reach");
    GG_REQUIRE(num_spheres == 0 || !dist2 || need2, "null pointer: need2");
    GG_REQUIRE(num_spheres == 0 || !pairs || radius, "null pointer: radius");
    GG_REQUIRE((((uintptr_t)q_a | (uintptr_t)q_b | (uintptr_t)radius | (uintptr_t)reach | (uintptr_t)gap) & 7) == 0,
               "q_a / q_b / radius / reach / gap misaligned");
    GG_REQUIRE((((uintptr_t)dist2 | (uintptr_t)spheres | (uintptr_t)frame | (uintptr_t)need2 | (uintptr_t)samples |
                 (uintptr_t)slack | (uintptr_t)slack_at | (uintptr_t)worst | (uintptr_t)gap_at | (uintptr_t)pair) & 3) == 0,
               "dist2 / spheres / frame / need2 / samples / slack / slack_at / worst / gap_at / pair misaligned");
    const ArmPairs p = arm_pairs(num_joints, pairs);
    const ArmMotionOut out{samples, slack, slack_at, worst, gap, gap_at, pair};
    const bool with_field = dist2 != nullptr, with_self = pairs != nullptr;
    arm_dispatch(num_joints, [&](auto joints) {
        constexpr int J = decltype(joints)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)num_edges), dim3(GG_WAVE), arm_lds_bytes(num_spheres),
                               (hipStream_t)stream, c, p, g, dist2, num_edges, q_a, q_b, num_spheres, spheres, frame,
                               need2, outside, radius, reach, res, max_samples, out);
        };
        if (with_field && with_self) launch(arm_motion_kernel<J, true, true>);
        else if (with_field) launch(arm_motion_kernel<J, true, false>);
        else if (with_self) launch(arm_motion_kernel<J, false, true>);
        else launch(arm_motion_kernel<J, false, false>);
    });
    GG_CHECK_LAUNCH();
    return GG_OK;
}
