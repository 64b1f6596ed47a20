// register_math.h — the per-point arithmetic of csrc/register.hip, fp64, usable on the host too: the symmetric 3x3
// eigen-solver behind the normals, the 3x3 solve behind the colour gradients, and the two Jacobian rows of one
// correspondence.  Nothing here may be contracted to an FMA (the library is built with -ffp-contract=off).
#pragma once
#include <math.h>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

#define RG_SUMS 32
#define RG_MAX_SWEEPS 16

__host__ __device__ inline double rg_dot(const double (&x)[3], const double (&y)[3]) {
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

__host__ __device__ inline void rg_cross(const double (&x)[3], const double (&y)[3], double (&o)[3]) {
    o[0] = x[1] * y[2] - x[2] * y[1];
    o[1] = x[2] * y[0] - x[0] * y[2];
    o[2] = x[0] * y[1] - x[1] * y[0];
}

// One Jacobi rotation in the (P, Q) plane: a <- J^T a J with a[P][Q] = 0 afterwards, v <- v J (Golub & Van Loan,
// Matrix Computations, algorithm 8.4.1).  An off-diagonal entry too small to change either diagonal entry is set
// to zero instead.
template <int P, int Q>
__host__ __device__ inline void rg_rotate(double (&a)[3][3], double (&v)[3][3]) {
    constexpr int R = 3 - P - Q;
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double g = 100.0 * fabs(apq);
    if (fabs(a[P][P]) + g == fabs(a[P][P]) && fabs(a[Q][Q]) + g == fabs(a[Q][Q])) {
        a[P][Q] = a[Q][P] = 0.0;
        return;
    }
    const double tau = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
    const double arp = a[R][P], arq = a[R][Q];
    a[P][P] = a[P][P] - t * apq;
    a[Q][Q] = a[Q][Q] + t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
}

// Unit eigenvector of the smallest eigenvalue of the symmetric matrix with upper triangle c = (xx, xy, xz, yy, yz,
// zz), by cyclic Jacobi sweeps; signed so that its largest-magnitude component is positive (first index on ties).
// The first index wins among equal smallest eigenvalues.
__host__ __device__ inline void rg_smallest_eigvec(const double (&c)[6], double (&n)[3]) {
    double a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < RG_MAX_SWEEPS; ++sweep) {
        if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0) break;
        rg_rotate<0, 1>(a, v);
        rg_rotate<0, 2>(a, v);
        rg_rotate<1, 2>(a, v);
    }
    const bool k1 = a[1][1] < a[0][0] && !(a[2][2] < a[1][1]);
    const bool k2 = a[2][2] < a[0][0] && a[2][2] < a[1][1];
    double e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = k2 ? v[k][2] : (k1 ? v[k][1] : v[k][0]);
    const double len = sqrt(rg_dot(e, e));
    const double a0 = fabs(e[0]), a1 = fabs(e[1]), a2 = fabs(e[2]);
    const double lead = (a0 >= a1 && a0 >= a2) ? e[0] : (a1 >= a2 ? e[1] : e[2]);
    const double sgn = lead < 0.0 ? -len : len;
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = e[k] / sgn;
}

// x = m^-1 r for the symmetric m with upper triangle (xx, xy, xz, yy, yz, zz), by cofactors; det is returned.
__host__ __device__ inline double rg_solve_sym3(const double (&m)[6], const double (&r)[3], double (&x)[3]) {
    const double c00 = m[3] * m[5] - m[4] * m[4], c01 = m[2] * m[4] - m[1] * m[5], c02 = m[1] * m[4] - m[2] * m[3];
    const double c11 = m[0] * m[5] - m[2] * m[2], c12 = m[1] * m[2] - m[0] * m[4], c22 = m[0] * m[3] - m[1] * m[1];
    const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
    x[0] = ((c00 * r[0] + c01 * r[1]) + c02 * r[2]) / det;
    x[1] = ((c01 * r[0] + c11 * r[1]) + c12 * r[2]) / det;
    x[2] = ((c02 * r[0] + c12 * r[1]) + c22 * r[2]) / det;
    return det;
}

// The colour-gradient system is m = T + k^2 n n^T with T the sum of the tangential rows' outer products (T n = 0)
// and k = count - 1, so det m = k^2 det2(T): it is singular exactly when the tangential rows span less than a
// plane.  tr = trace T bounds det2(T) by (tr / 2)^2; the system counts as singular unless det2(T) exceeds 2^-40 of
// that bound.
#define RG_SINGULAR_REL 0x1p-40
__host__ __device__ inline bool rg_gradient_singular(double det, double k, double tr) {
    const double h = 0.5 * tr;
    return !(det > (RG_SINGULAR_REL * (k * k)) * (h * h));
}

// The sums' terms of one correspondence (include/gg_raster.h gg_icp_step): s the moved source point, q, n, d, iq
// the target's point, normal, colour gradient and intensity, is the source's intensity, d2 the squared distance,
// wg = sqrt(lambda), wp = sqrt(1 - lambda).  out: RG_SUMS doubles.  ab (may be null): RG_SUMS doubles, the same terms
// with every product's absolute value.
__host__ __device__ inline void rg_terms(const double (&s)[3], const double (&q)[3], const double (&n)[3],
                                         const double (&d)[3], double is, double iq, double d2, double wg, double wp,
                                         double *out, double *ab) {
    const double e[3] = {s[0] - q[0], s[1] - q[1], s[2] - q[2]};
    const double rg = rg_dot(e, n);
    double jg[6], jp[6], cr[3];
    rg_cross(s, n, cr);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        jg[k] = wg * cr[k];
        jg[3 + k] = wg * n[k];
    }
    const double w[3] = {(s[0] - rg * n[0]) - q[0], (s[1] - rg * n[1]) - q[1], (s[2] - rg * n[2]) - q[2]};
    const double ri = is - (iq + rg_dot(d, w));
    const double dn = rg_dot(d, n);
    const double g[3] = {-(d[0] - dn * n[0]), -(d[1] - dn * n[1]), -(d[2] - dn * n[2])};
    rg_cross(s, g, cr);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        jp[k] = wp * cr[k];
        jp[3 + k] = wp * g[k];
    }
    const double rgw = wg * rg, riw = wp * ri;
    int o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            const double a = jg[i] * jg[j], b = jp[i] * jp[j];
            out[o] = a + b;
            if (ab) ab[o] = fabs(a) + fabs(b);
            ++o;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double a = jg[i] * rgw, b = jp[i] * riw;
        out[21 + i] = a + b;
        if (ab) ab[21 + i] = fabs(a) + fabs(b);
    }
    out[27] = 1.0;
    out[28] = d2;
    out[29] = rg * rg;
    out[30] = ri * ri;
    out[31] = 0.0;
    if (ab) {
        ab[27] = 1.0;
        ab[28] = d2;
        ab[29] = out[29];
        ab[30] = out[30];
        ab[31] = 0.0;
    }
}
