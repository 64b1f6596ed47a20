// trajectory.hip — arm trajectories: the time law over a blended polyline and its controller-rate samples
// (include/gg_raster.h "Arm trajectories").
//
// gg_traj_time    a wave per path, TR_WAVES paths a workgroup.  The path is a dependent chain of up to m (2W - 3) grid
//                 steps, walked once backwards (xbar) and once forwards (x, u, t).  Within a step the rows of the
//                 interval sit one per lane (lane 2j + e: joint j at the near or the far end; lane 2J: the bounds of
//                 x_{i+1}); the (lower, upper) pairs are strided over the 64 lanes, each with one fp64 division, and a
//                 butterfly takes the minimum.  Every loop is the same for the whole wave and all 64 lanes stay active
//                 in it.  No LDS, no atomics, no workgroup barrier: a wave never waits for another.
// gg_traj_sample  a thread per (path, sample): a binary search in the path's grid times, then the interval's own
//                 piece.
#include <math.h>

#include "gg_common.h"

#define TR_THREADS 256
#define TR_WAVES (TR_THREADS / GG_WAVE)
#define TR_MAX_SAMPLES (1 << 30)

struct TrLimits {
    double v[GG_ARM_MAX_JOINTS], a[GG_ARM_MAX_JOINTS];
};

// One piece of the path, the same in every lane.  kind 0: the line of segment k between the blends of its ends, f0 =
// f_k, f1 = f_{k+1}, L = (1 - f0) - f1.  kind 1: the blend about waypoint k, f0 = f_k.
struct TrPiece {
    int kind, k;
    double f0, L, delta;
};

// the blend fraction of waypoint k as the law takes it: 0 at both ends, else clamped into [0, 1/2] (NaN: 0)
__device__ __forceinline__ double tr_fraction(const double *__restrict__ blend, int k, int n) {
    return k <= 0 || k >= n - 1 ? 0.0 : fmin(fmax(blend[k], 0.0), 0.5);
}

// Slot t of a path of n waypoints: t = 2k the line of segment k, t = 2k - 1 the blend about waypoint k.  False for a
// piece that is skipped: a blend of fraction 0, a line of length 0.
__device__ __forceinline__ bool tr_piece(const double *__restrict__ blend, int n, int m, int slot, TrPiece &pc) {
    if (slot & 1) {
        pc.kind = 1;
        pc.k = (slot + 1) >> 1;
        pc.f0 = tr_fraction(blend, pc.k, n);
        pc.L = 2.0 * pc.f0;
        pc.delta = pc.L / (double)m;
        return pc.f0 > 0.0;
    }
    pc.kind = 0;
    pc.k = slot >> 1;
    pc.f0 = tr_fraction(blend, pc.k, n);
    pc.L = (1.0 - pc.f0) - tr_fraction(blend, pc.k + 1, n);
    pc.delta = pc.L / (double)m;
    return pc.L > 0.0;
}

// the geometry of joint j on interval a of a piece: q at the interval's start, q' at both ends, q''
struct TrGeom {
    double q, qp0, qp1, qpp;
};
__device__ __forceinline__ TrGeom tr_geom(const TrPiece &pc, int a, int m, double wm, double w0, double wp) {
    TrGeom g;
    const double tau = (double)a / (double)m;
    if (pc.kind == 0) {
        const double d = wp - w0;
        const double sigma = pc.f0 + tau * pc.L;
        g.q = w0 + sigma * d;
        g.qp0 = d;
        g.qp1 = d;
        g.qpp = 0.0;
    } else {
        const double dm = w0 - wm, dp = wp - w0;
        const double e = dp - dm;
        g.qp0 = dm + tau * e;
        g.qp1 = a + 1 == m ? dp : dm + ((double)(a + 1) / (double)m) * e;
        g.qpp = e / pc.L;
        const double p0 = w0 - pc.f0 * dm;
        g.q = (p0 + tau * (pc.L * dm)) + (tau * tau) * (pc.f0 * e);
    }
    return g;
}

__device__ __forceinline__ double tr_wave_min(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off, GG_WAVE));
    return v;
}
__device__ __forceinline__ double tr_wave_max(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, GG_WAVE));
    return v;
}

// a value another lane of this wave stored before the fence between the two passes
__device__ __forceinline__ double tr_load(const double *p) {
    return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p),
                                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// The rows of one interval, one per lane: the upper line u <= cu + d x, the lower line u >= cl + d x (the two share
// their slope), and the cap on x of a row without u.  A lane without a row holds the neutral (+inf, -inf, 0, +inf).
struct TrRow {
    double cu, cl, d, cap;
};
__device__ __forceinline__ TrRow tr_row(int lane, int J, const TrGeom &g, double acc, double two, double next) {
    TrRow r{INFINITY, -INFINITY, 0.0, INFINITY};
    if (lane < 2 * J) {
        const double B = (lane & 1) ? two * g.qpp + g.qp1 : g.qp0;
        if (B != 0.0) {
            r.cu = acc / fabs(B);
            r.cl = -r.cu;
            r.d = -(g.qpp / B);
        } else if (g.qpp != 0.0) {
            r.cap = acc / fabs(g.qpp);
        }
    } else if (lane == 2 * J) {
        r.cu = next / two;
        r.cl = 0.0;
        r.d = -(1.0 / two);
    }
    return r;
}

// the velocity cap of joint j on an interval: (v / max(|q'| at its ends))^2, +inf for a joint that does not move
__device__ __forceinline__ double tr_vcap(const TrGeom &g, double vel) {
    const double mx = fmax(fabs(g.qp0), fabs(g.qp1));
    if (!(mx > 0.0)) return INFINITY;
    const double r = vel / mx;
    return r * r;
}

__global__ __launch_bounds__(TR_THREADS) void traj_time_kernel(TrLimits lim, int J, int P, int W, int m, int gmax,
                                                               const double *__restrict__ way,
                                                               const int *__restrict__ length,
                                                               const double *__restrict__ blend_all,
                                                               int *__restrict__ count_out, double *xbar_all,
                                                               double *__restrict__ x_all, double *__restrict__ u_all,
                                                               double *__restrict__ t_all, double *__restrict__ q_grid,
                                                               double *__restrict__ duration,
                                                               double *__restrict__ infeasible,
                                                               int *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * TR_WAVES + (threadIdx.x >> 6);
    if (p >= P) return;                                         // the same for the whole wave
    const int n = min(max(__builtin_amdgcn_readfirstlane(length[p]), 1), W);
    const double *w = way + (size_t)p * W * J;
    const double *blend = blend_all + (size_t)p * W;
    double *xbar = xbar_all + (size_t)p * (gmax + 1);
    double *x = x_all + (size_t)p * (gmax + 1);
    double *t = t_all + (size_t)p * (gmax + 1);
    double *u = u_all + (size_t)p * gmax;
    double *qg = q_grid ? q_grid + (size_t)p * (gmax + 1) * J : nullptr;
    const int j = min(lane >> 1, J - 1);                        // this lane's joint; lanes >= 2 J hold no joint row
    const double vel = lim.v[j], acc = lim.a[j];
    const int R = 2 * J + 1;

    // ---- the status: every waypoint finite, no segment of length zero
    int st = GG_TRAJ_OK;
    {
        bool bad = false;
        for (int e = lane; e < n * J; e += GG_WAVE) bad = bad || !isfinite(w[e]);
        if (__ballot(bad)) st = GG_TRAJ_NOT_FINITE;
        if (st == GG_TRAJ_OK) {
            bool zero = false;
            for (int k = lane; k < n - 1; k += GG_WAVE) {
                bool moves = false;
                for (int jj = 0; jj < J; ++jj) moves = moves || (w[(k + 1) * J + jj] - w[k * J + jj]) != 0.0;
                zero = zero || !moves;
            }
            if (__ballot(zero)) st = GG_TRAJ_ZERO_SEGMENT;
        }
    }
    const int slots = 2 * (n - 1) - 1;                          // -1 for a path of one waypoint: no piece
    int G = 0;
    TrPiece pc;
    if (st == GG_TRAJ_OK)
        for (int s = 0; s < slots; ++s) G += tr_piece(blend, n, m, s, pc) ? m : 0;

    double dur = st == GG_TRAJ_OK ? 0.0 : (double)NAN, worst = dur;
    if (st == GG_TRAJ_OK && G > 0) {
        // ---- backwards: xbar_i, the largest x from which the interval's rows can be met
        if (lane == 0) xbar[G] = 0.0;
        double next = 0.0;
        int i = G;
        for (int s = slots - 1; s >= 0; --s) {
            if (!tr_piece(blend, n, m, s, pc)) continue;
            const int k = pc.k;
            const double wm = w[max(k - 1, 0) * J + j], w0 = w[k * J + j], wp = w[(k + 1) * J + j];
            // the piece starts at a stop: the path's start, or a waypoint without a blend
            const bool stop = pc.kind == 0 && tr_fraction(blend, k, n) == 0.0;
            const double two = 2.0 * pc.delta;
            for (int a = m - 1; a >= 0; --a) {
                --i;
                const TrGeom g = tr_geom(pc, a, m, wm, w0, wp);
                const double vc = tr_wave_min(lane < 2 * J ? tr_vcap(g, vel) : (double)INFINITY);
                const TrRow r = tr_row(lane, J, g, acc, two, fmin(next, vc));
                double best = fmin(r.cap, vc);
                for (int base = 0; base < R * R; base += GG_WAVE) {
                    const int pr = base + lane;
                    const int lo = min(pr / R, R - 1), hi = pr - (pr / R) * R;
                    const double cl = __shfl(r.cl, lo, GG_WAVE), dl = __shfl(r.d, lo, GG_WAVE);
                    const double cu = __shfl(r.cu, hi, GG_WAVE), dh = __shfl(r.d, hi, GG_WAVE);
                    const double dd = dl - dh;
                    if (pr < R * R && dd > 0.0) best = fmin(best, (cu - cl) / dd);
                }
                next = a == 0 && stop ? 0.0 : fmax(tr_wave_min(best), 0.0);
                if (lane == 0) xbar[i] = next;
            }
        }
        __threadfence();                                        // xbar is read back below, by other lanes
        // ---- forwards: the largest u at every step
        double xi = 0.0, ti = 0.0;
        worst = 0.0;
        if (lane == 0) x[0] = 0.0, t[0] = 0.0;
        i = 0;
        for (int s = 0; s < slots; ++s) {
            if (!tr_piece(blend, n, m, s, pc)) continue;
            const int k = pc.k;
            const double wm = w[max(k - 1, 0) * J + j], w0 = w[k * J + j], wp = w[(k + 1) * J + j];
            const double two = 2.0 * pc.delta;
            for (int a = 0; a < m; ++a, ++i) {
                const TrGeom g = tr_geom(pc, a, m, wm, w0, wp);
                if (qg && lane < 2 * J && !(lane & 1)) qg[(size_t)i * J + j] = g.q;
                const double vc = tr_wave_min(lane < 2 * J ? tr_vcap(g, vel) : (double)INFINITY);
                const double bound = fmin(tr_load(xbar + i + 1), vc);
                const TrRow r = tr_row(lane, J, g, acc, two, bound);
                const double ui = tr_wave_min(r.cu + r.d * xi);
                const double low = tr_wave_max(r.cl + r.d * xi);
                worst = fmax(worst, low - ui);
                const double xn = fmin(fmax(xi + two * ui, 0.0), bound);
                const double dt = two / (sqrt(xi) + sqrt(xn));
                ti = ti + dt;
                xi = xn;
                if (lane == 0) u[i] = ui, x[i + 1] = xn, t[i + 1] = ti;
            }
        }
        if (qg && lane < J) qg[(size_t)G * J + lane] = w[(n - 1) * J + lane];
        dur = ti;
        if (!isfinite(dur)) st = GG_TRAJ_NO_DURATION;
    } else if (st == GG_TRAJ_OK) {                              // one waypoint: at rest there
        if (lane == 0) xbar[0] = 0.0, x[0] = 0.0, t[0] = 0.0;
        if (qg && lane < J) qg[lane] = w[lane];
    }
    if (st != GG_TRAJ_OK) {
        G = -1;                                                 // every row NaN from entry 0 on
        dur = worst = (double)NAN;
    }
    for (int e = G + 1 + lane; e <= gmax; e += GG_WAVE) xbar[e] = x[e] = t[e] = (double)NAN;
    for (int e = max(G, 0) + lane; e < gmax; e += GG_WAVE) u[e] = (double)NAN;
    if (qg)
        for (int e = (G + 1) * J + lane; e < (gmax + 1) * J; e += GG_WAVE) qg[e] = (double)NAN;
    if (lane == 0) {
        count_out[p] = max(G, 0);
        duration[p] = dur;
        infeasible[p] = worst;
        status[p] = st;
    }
}

__global__ __launch_bounds__(TR_THREADS) void traj_sample_kernel(int J, int P, int W, int m, int gmax,
                                                                 const double *__restrict__ way,
                                                                 const int *__restrict__ length,
                                                                 const double *__restrict__ blend_all,
                                                                 const int *__restrict__ count,
                                                                 const double *__restrict__ x_all,
                                                                 const double *__restrict__ u_all,
                                                                 const double *__restrict__ t_all,
                                                                 const double *__restrict__ duration,
                                                                 const int *__restrict__ status, double dt, int K,
                                                                 double *__restrict__ q, double *__restrict__ qd,
                                                                 double *__restrict__ qdd, int *__restrict__ num) {
    const long long at = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
    if (at >= (long long)P * K) return;
    const int p = (int)(at / K), k = (int)(at - (long long)p * K);
    const int n = min(max(length[p], 1), W);
    const int G = min(max(count[p], 0), gmax);
    const double dur = duration[p];
    // one more than the smallest k with k dt >= duration: a division proposes it, these comparisons decide it
    int total = 0;
    if (status[p] == GG_TRAJ_OK && isfinite(dur) && dur >= 0.0) {
        const double r = dur / dt;
        if (r >= (double)TR_MAX_SAMPLES) {
            total = TR_MAX_SAMPLES;
        } else {
            int k0 = (int)r;
            if ((double)k0 * dt < dur) ++k0;
            if ((double)k0 * dt < dur) ++k0;
            if (k0 > 0 && (double)(k0 - 1) * dt >= dur) --k0;
            total = k0 + 1;
        }
    }
    if (k == 0) num[p] = total;
    double *oq = q + (size_t)at * J, *od = qd + (size_t)at * J, *oa = qdd + (size_t)at * J;
    if (k >= total) {
        for (int j = 0; j < J; ++j) oq[j] = od[j] = oa[j] = (double)NAN;
        return;
    }
    const double *w = way + (size_t)p * W * J;
    if (G == 0) {                                               // one waypoint: at rest there
        for (int j = 0; j < J; ++j) oq[j] = w[j], od[j] = 0.0, oa[j] = 0.0;
        return;
    }
    const double *blend = blend_all + (size_t)p * W;
    const double *t = t_all + (size_t)p * (gmax + 1);
    const double tt = fmin((double)k * dt, dur);
    int lo = 0, hi = G;                                         // the last interval with t_i <= tt, at most G - 1
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (t[mid] <= tt) lo = mid;
        else hi = mid;
    }
    const int i = lo;
    // the piece of interval i: the (i / m)-th piece that is not skipped
    TrPiece pc;
    int left = i / m;
    const int slots = 2 * (n - 1) - 1;
    bool found = false;
    for (int s = 0; s < slots && !found; ++s)
        if (tr_piece(blend, n, m, s, pc)) {
            found = left == 0;
            --left;
        }
    if (!found) {                                               // count does not belong to this path: the caller's
        for (int j = 0; j < J; ++j) oq[j] = od[j] = oa[j] = (double)NAN;
        return;
    }
    const int a = i - (i / m) * m;
    const double xi = x_all[(size_t)p * (gmax + 1) + i], ui = u_all[(size_t)p * gmax + i];
    const double tau = tt - t[i];
    const double root = sqrt(xi);
    const double sd = root + ui * tau;
    const double ds = fmin(fmax((root + (0.5 * ui) * tau) * tau, 0.0), pc.delta);
    for (int j = 0; j < J; ++j) {
        const TrGeom g = tr_geom(pc, a, m, w[max(pc.k - 1, 0) * J + j], w[pc.k * J + j], w[(pc.k + 1) * J + j]);
        const double qp = g.qp0 + ds * g.qpp;
        oq[j] = (g.q + ds * g.qp0) + ((0.5 * ds) * ds) * g.qpp;
        od[j] = qp * sd;
        oa[j] = g.qpp * (sd * sd) + qp * ui;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the C ABI
// ---------------------------------------------------------------------------------------------------------------
static bool traj_shape_ok(int J, int P, int W, int m) {
    return J >= 1 && J <= GG_ARM_MAX_JOINTS && W >= 1 && W <= GG_TRAJ_MAX_WAYPOINTS && m >= 2 &&
           m <= GG_TRAJ_MAX_STEPS && P >= 0 && (int64_t)P * (GG_TRAJ_GRID(W, m) + 1) <= (int64_t)GG_FIELD_MAX_POSES;
}
#define TR_SHAPE_MSG                                                                                            \
    "need num_joints in 1..GG_ARM_MAX_JOINTS, num_waypoints in 1..GG_TRAJ_MAX_WAYPOINTS, steps (m) in "         \
    "2..GG_TRAJ_MAX_STEPS, num_paths >= 0 and num_paths (GG_TRAJ_GRID + 1) <= GG_FIELD_MAX_POSES"

extern "C" int gg_traj_time(int num_joints, int num_paths, int num_waypoints, const double *way,
                            const int32_t *length, const double *blend, const double *v_max, const double *a_max,
                            int steps, int32_t *count, double *xbar, double *x, double *u, double *t, double *q_grid,
                            double *duration, double *infeasible, int32_t *status, gg_stream_t stream) {
    GG_REQUIRE(traj_shape_ok(num_joints, num_paths, num_waypoints, steps), TR_SHAPE_MSG);
    GG_REQUIRE(v_max && a_max, "null pointer: v_max / a_max (host arrays of num_joints doubles)");
    TrLimits lim{};
    for (int j = 0; j < GG_ARM_MAX_JOINTS; ++j) {
        const int s = j < num_joints ? j : 0;
        GG_REQUIRE(isfinite(v_max[s]) && v_max[s] > 0.0, "v_max: every entry must be finite and > 0");
        GG_REQUIRE(isfinite(a_max[s]) && a_max[s] > 0.0, "a_max: every entry must be finite and > 0");
        lim.v[j] = v_max[s];
        lim.a[j] = a_max[s];
    }
    if (num_paths == 0) return GG_OK;
    GG_REQUIRE(way && length && blend, "null pointer: way / length / blend");
    GG_REQUIRE(count && xbar && x && u && t && duration && infeasible && status,
               "null pointer: count / xbar / x / u / t / duration / infeasible / status");
    GG_REQUIRE((((uintptr_t)way | (uintptr_t)blend | (uintptr_t)xbar | (uintptr_t)x | (uintptr_t)u | (uintptr_t)t |
                 (uintptr_t)q_grid | (uintptr_t)duration | (uintptr_t)infeasible) & 7) == 0,
               "way / blend / xbar / x / u / t / q_grid / duration / infeasible misaligned");
    GG_REQUIRE((((uintptr_t)length | (uintptr_t)count | (uintptr_t)status) & 3) == 0,
               "length / count / status misaligned");
    hipLaunchKernelGGL(traj_time_kernel, dim3((unsigned)((num_paths + TR_WAVES - 1) / TR_WAVES)), dim3(TR_THREADS), 0,
                       (hipStream_t)stream, lim, num_joints, num_paths, num_waypoints, steps,
                       GG_TRAJ_GRID(num_waypoints, steps), way, length, blend, count, xbar, x, u, t, q_grid, duration,
                       infeasible, status);
    GG_CHECK_LAUNCH();
    return GG_OK;
}

extern "C" int gg_traj_sample(int num_joints, int num_paths, int num_waypoints, const double *way,
                              const int32_t *length, const double *blend, int steps, const int32_t *count,
                              const double *x, const double *u, const double *t, const double *duration,
                              const int32_t *status, double dt, int num_samples, double *q, double *qd, double *qdd,
                              int32_t *num, gg_stream_t stream) {
    GG_REQUIRE(traj_shape_ok(num_joints, num_paths, num_waypoints, steps), TR_SHAPE_MSG);
    GG_REQUIRE(isfinite(dt) && dt > 0.0, "dt must be finite and > 0");
    GG_REQUIRE(num_samples >= 1 && (int64_t)num_paths * num_samples <= (int64_t)GG_FIELD_MAX_POSES,
               "need num_samples >= 1 and num_paths num_samples <= GG_FIELD_MAX_POSES");
    if (num_paths == 0) return GG_OK;
    GG_REQUIRE(way && length && blend && count && x && u && t && duration && status,
               "null pointer: way / length / blend / count / x / u / t / duration / status");
    GG_REQUIRE(q && qd && qdd && num, "null pointer: q / qd / qdd / num");
    GG_REQUIRE((((uintptr_t)way | (uintptr_t)blend | (uintptr_t)x | (uintptr_t)u | (uintptr_t)t | (uintptr_t)duration |
                 (uintptr_t)q | (uintptr_t)qd | (uintptr_t)qdd) & 7) == 0,
               "way / blend / x / u / t / duration / q / qd / qdd misaligned");
    GG_REQUIRE((((uintptr_t)length | (uintptr_t)count | (uintptr_t)status | (uintptr_t)num) & 3) == 0,
               "length / count / status / num misaligned");
    const long long cells = (long long)num_paths * num_samples;
    hipLaunchKernelGGL(traj_sample_kernel, dim3((unsigned)((cells + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS),
                       0, (hipStream_t)stream, num_joints, num_paths, num_waypoints, steps,
                       GG_TRAJ_GRID(num_waypoints, steps), way, length, blend, count, x, u, t, duration, status, dt,
                       num_samples, q, qd, qdd, num);
    GG_CHECK_LAUNCH();
    return GG_OK;
}
