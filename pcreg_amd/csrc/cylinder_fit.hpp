// pcreg_amd/csrc/cylinder_fit.hpp -- the refit of pcreg_model_fit_cylinders_f32 (its contract, include/pcreg.h), its one
// definition: from the rounded sums of a round's inliers to (centre, w, R), or to "not used".  Two steps, each after one exact pass.
//
// 1. THE AXIS (fit_cylinders_basis).  A6 = the six sums of gn_a gn_b of the inliers' quantised normals (xx xy xz yy yz zz), each
//    rounded once to double.  A cylinder's normals are perpendicular to its axis, so the axis minimises sum (n . w)^2: the
//    eigenvector of A's smallest eigenvalue.  fit_cylinders_jacobi is the library's cyclic Jacobi (wave_math.hpp's jacobi_sym3,
//    sweep for sweep and operation for operation) with ONE change: the rotation's cosine is c = 1 / sqrt(t t + 1), two correctly
//    rounded operations, where jacobi_sym3 calls rsqrt -- on the device an approximation refined to about one ulp, whose bits no
//    float64 restatement can give.  Then the column of the smallest diagonal entry (ties to the lowest index), the sign rule, and
//    the basis of the cross-section: e_k the coordinate axis of w's smallest-magnitude component (first of equals),
//    c = w x e_k by the general formula (the products with 0 and 1 are exact), l2 = (cx cx + cy cy) + cz cz, u = c / sqrt(l2),
//    v = w x u, each component fl(fl(a b) - fl(c d)).
// 2. THE CIRCLE (fit_cylinders_circle).  With (xi, yi) the inliers' quantised differences in the (u, v) plane and w2 = xi^2 + yi^2,
//    the circle |(xi, yi) - c|^2 = R^2 is the linear model (xi, yi) . a + beta = w2 with a = 2 c, beta = R^2 - |c|^2.  Eliminating
//    beta leaves N a = h, N = n S2 - S1 S1^T (N3: xx xy yy), h = n (sum (xi, yi) w2) - S1 (sum w2), both formed exactly in
//    integers by the caller and rounded once per entry.  Here: L00 = sqrt(N00); L10 = N01 / L00; L11 = sqrt(N11 - L10 L10);
//    y0 = h0 / L00; y1 = (h1 - L10 y0) / L11; a1 = y1 / L11; a0 = (y0 - L10 a1) / L00; c2 = a / 2;
//    beta = (sw - (a0 S1x + a1 S1y)) / n; R_g^2 = beta + (c2x c2x + c2y c2y);
//    centre = p0 + (c2x u + c2y v) back, component by component; R = sqrt(R_g^2) back      (back = 2^-(17 - e), a power of two)
// Only + - * / sqrt appear, one rounding each, in the order written, so a float64 restatement gives the same bits
// (tests/cylinders_ref.py: finish64).
//
// Plain C++17 on the host (tests/test_cylinder_fit_host.py holds it to finish64 bit for bit) and device code under hipcc; no HIP
// header, no project header.  Compile with -ffp-contract=off, as the library is: nothing below is fused.
#pragma once
#include <cfloat>
#include <cmath>

#if !defined(PCREG_HD)
#if defined(__HIPCC__)
#define PCREG_HD __host__ __device__
#else
#define PCREG_HD
#endif
#endif

namespace pcreg {

PCREG_HD inline bool fit_cylinders_finite(double v) { return v - v == 0.0; }
// a radicand a root may be taken of: a finite number above 0 (a NaN fails)
PCREG_HD inline bool fit_cylinders_radicand_ok(double v) { return v > 0.0 && fit_cylinders_finite(v); }

// a = {a00, a01, a02, a11, a12, a22} (in/out: the diagonal ends up in a[0], a[3], a[5]); V row-major 3 x 3, columns = eigenvectors
PCREG_HD inline void fit_cylinders_jacobi(double (&a)[6], double (&V)[9]) {
    for (int i = 0; i < 9; ++i) V[i] = (i % 4) == 0 ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        const double off = fabs(a[1]) + fabs(a[2]) + fabs(a[4]);
        const double dia = fabs(a[0]) + fabs(a[3]) + fabs(a[5]);
        if (off <= 1e-300 || off <= DBL_EPSILON * 1e-3 * dia) break;
        // rotation in the (P, Q) plane; R is the third index.  APP/AQQ/APQ/ARP/ARQ name the entries of `a`.
#define PCREG_CY_ROT(APP, AQQ, APQ, ARP, ARQ, P, Q)                                                \
        if (a[APQ] != 0.0) {                                                                       \
            const double h = 2.0 * a[APQ], d = a[AQQ] - a[APP];                                    \
            const double t = copysign(fabs(h), h * d >= 0.0 ? 1.0 : -1.0) / (fabs(d) + sqrt(d * d + h * h)); \
            const double c = 1.0 / sqrt(t * t + 1.0), s = c * t;                                   \
            const double tp = t * a[APQ];                                                          \
            a[APP] -= tp; a[AQQ] += tp; a[APQ] = 0.0;                                              \
            const double rp = a[ARP], rq = a[ARQ];                                                 \
            a[ARP] = c * rp - s * rq; a[ARQ] = s * rp + c * rq;                                    \
            for (int k = 0; k < 3; ++k) {                                                          \
                const double vp = V[k * 3 + P], vq = V[k * 3 + Q];                                 \
                V[k * 3 + P] = c * vp - s * vq; V[k * 3 + Q] = s * vp + c * vq;                    \
            }                                                                                      \
        }
        PCREG_CY_ROT(0, 3, 1, 2, 4, 0, 1)       // (0,1): third index 2 -> a02, a12
        PCREG_CY_ROT(0, 5, 2, 1, 4, 0, 2)       // (0,2): third index 1 -> a01, a12
        PCREG_CY_ROT(3, 5, 4, 1, 2, 1, 2)       // (1,2): third index 0 -> a01, a02
#undef PCREG_CY_ROT
    }
}

// the sign rule of an axis: with a reference vector, negated when w . ref < 0; without, the component of largest magnitude is made
// positive, the first of equals in x, y, z order
PCREG_HD inline bool fit_cylinders_negate(const double (&w)[3], bool use_ref, double rx, double ry, double rz) {
    if (use_ref) return (w[0] * rx + w[1] * ry) + w[2] * rz < 0.0;
    double m = w[0];                                              // (no indexing by a variable: the device keeps w in registers)
    if (fabs(w[1]) > fabs(m)) m = w[1];
    if (fabs(w[2]) > fabs(m)) m = w[2];
    return m < 0.0;
}

PCREG_HD inline void fit_cylinders_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// (w, u, v) from A6 and n_n, the number of inliers with a usable normal; (rx, ry, rz) is read with use_ref alone.  false -- and the outputs
// untouched -- when n_n < 2, when Jacobi's diagonal or the chosen column is not finite, or when l2 is not a finite number above 0.
PCREG_HD inline bool fit_cylinders_basis(const double (&A6)[6], long long n_n, bool use_ref, double rx, double ry, double rz,
                                         double (&w)[3], double (&u)[3], double (&v)[3]) {
    if (n_n < 2) return false;
    double a[6], V[9];
    for (int i = 0; i < 6; ++i) a[i] = A6[i];
    fit_cylinders_jacobi(a, V);
    if (!fit_cylinders_finite(a[0]) || !fit_cylinders_finite(a[3]) || !fit_cylinders_finite(a[5])) return false;
    int c = 0;                                                    // the smallest diagonal entry, the first of equal ones
    if (a[3] < a[0]) c = 1;
    if (a[5] < (c == 1 ? a[3] : a[0])) c = 2;
    double ww[3] = {c == 0 ? V[0] : c == 1 ? V[1] : V[2], c == 0 ? V[3] : c == 1 ? V[4] : V[5], c == 0 ? V[6] : c == 1 ? V[7] : V[8]};
    if (!fit_cylinders_finite(ww[0]) || !fit_cylinders_finite(ww[1]) || !fit_cylinders_finite(ww[2])) return false;
    if (fit_cylinders_negate(ww, use_ref, rx, ry, rz)) { ww[0] = -ww[0]; ww[1] = -ww[1]; ww[2] = -ww[2]; }
    int k = 0;                                                    // w's smallest-magnitude component, the first of equal ones
    double wk = fabs(ww[0]);
    if (fabs(ww[1]) < wk) { k = 1; wk = fabs(ww[1]); }
    if (fabs(ww[2]) < wk) k = 2;
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double cr[3];
    fit_cylinders_cross(ww, e, cr);
    const double l2 = (cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2];
    if (!fit_cylinders_radicand_ok(l2)) return false;
    const double l = sqrt(l2);
    const double uu[3] = {cr[0] / l, cr[1] / l, cr[2] / l};
    double vv[3];
    fit_cylinders_cross(ww, uu, vv);
    for (int i = 0; i < 3; ++i) { w[i] = ww[i]; u[i] = uu[i]; v[i] = vv[i]; }
    return true;
}

// (centre, R) from N3, h, S1 = (double)(sum xi, sum yi), sw = (double)sum w2, n = (double)count, the trial's first row p0 widened
// to double, the basis and back = 2^-(17 - e).  false -- and the outputs untouched -- when the contract says the refit is NOT
// USED: a radicand of the factorisation or R_g^2 not a finite number above 0, centre or R not finite, (float)R outside
// [min_radius, max_radius].
PCREG_HD inline bool fit_cylinders_circle(const double (&N3)[3], const double (&h)[2], const double (&S1)[2], double sw, double n,
                                          const double (&p0)[3], const double (&u)[3], const double (&v)[3], double back,
                                          float min_radius, float max_radius, double (&centre)[3], double& R) {
    const double r0 = N3[0];
    if (!fit_cylinders_radicand_ok(r0)) return false;
    const double L00 = sqrt(r0);
    const double L10 = N3[1] / L00;
    const double r1 = N3[2] - L10 * L10;
    if (!fit_cylinders_radicand_ok(r1)) return false;
    const double L11 = sqrt(r1);
    const double y0 = h[0] / L00;
    const double y1 = (h[1] - L10 * y0) / L11;
    const double a1 = y1 / L11;
    const double a0 = (y0 - L10 * a1) / L00;
    const double cx = a0 / 2.0, cy = a1 / 2.0;
    const double beta = (sw - (a0 * S1[0] + a1 * S1[1])) / n;
    const double Rg2 = beta + (cx * cx + cy * cy);
    if (!fit_cylinders_radicand_ok(Rg2)) return false;
    double o[3];
    for (int i = 0; i < 3; ++i) o[i] = p0[i] + (cx * u[i] + cy * v[i]) * back;
    const double Rr = sqrt(Rg2) * back;
    if (!fit_cylinders_finite(o[0]) || !fit_cylinders_finite(o[1]) || !fit_cylinders_finite(o[2]) || !fit_cylinders_finite(Rr)) return false;
    const float Rf = (float)Rr;
    if (!(Rf >= min_radius && Rf <= max_radius)) return false;
    centre[0] = o[0]; centre[1] = o[1]; centre[2] = o[2];
    R = Rr;
    return true;
}

}  // namespace pcreg
