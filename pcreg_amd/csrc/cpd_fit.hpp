// pcreg_amd/csrc/cpd_fit.hpp -- the fit of the coherent-point-drift refit (pcreg_model_refit_cpd_f32's contract, include/pcreg.h;
// DESIGN 4.27), its one definition: from the 19 weighted sums of a transform to (T_step, sigma2_out), or to "empty".
//
//   s[0]      Np  = sum p_i                        u_i = p'_i - o, the moved point about the origin o
//   s[1..3]   Sp  = sum p_i u_i                    y_i = p_i u_i + g_i V_i, the weighted model side about o
//   s[4..6]   Sm  = sum y_i
//   s[7..15]  C   = sum u_i (x) y_i, C_ab at 7 + 3 a + b
//   s[16]     Spp = sum p_i |u_i|^2
//   s[17]     Smm = sum (p_i |u_i|^2 + 2 u_i . g_i V_i + g_i W_i)
//   s[18]     sum_res2 = sum g_i W_i   (reported, not used by the fit)
//   1. Np a finite number above 0, or empty.  mp = Sp / Np, mm = Sm / Np, component by component.
//   2. A_ab = C_ba - mm_a * Sp_b: the cross-covariance (model side a, data side b), centred.
//   3. sc = the largest |A_ab| (a finite number above 0, or empty); An = A / sc.
//   4. G = An^T An, G_ab = (An_0a An_0b + An_1a An_1b) + An_2a An_2b for a <= b; fit_cylinders_jacobi(G): eigenvalues l, columns V.
//   5. i1 the index of the largest l (the first of equal ones), i2 of the larger of the other two (the first of equal ones);
//      v1, v2 those columns of V.
//   6. w1 = An v1, each component (An_a0 v_0 + An_a1 v_1) + An_a2 v_2; s1 = sqrt((w1_0^2 + w1_1^2) + w1_2^2), a finite number above 0,
//      or empty; u1 = w1 / s1.  w2 = An v2; d = (u1_0 w2_0 + u1_1 w2_1) + u1_2 w2_2; w2 = w2 - d u1; s2 = sqrt(|w2|^2).
//      EMPTY unless s2 > 2^-26 s1: s1 and s2 are the two largest singular values of An, and a rotation about a single
//      direction is not determined.  u2 = w2 / s2.
//   7. u3 = u1 x u2, v3 = v1 x v2 (each component fl(fl(a b) - fl(c d))); R_ab = (u1_a v1_b + u2_a v2_b) + u3_a v3_b.
//      Both triples are right-handed, so det R = +1 whatever the sign of det A: this IS coherent point drift's determinant
//      correction U diag(1, 1, det(U V^T)) V^T, and it maximises tr(A^T R) over the rotations.  (estimateTransform.m has none.)
//   8. tr = the sum of A_ab R_ab over a, b row-major, term by term from 0.0.
//   9. sigma2_out = (((Smm - mm . Sm) - 2 tr) + (Spp - mp . Sp)) / (3 Np), dots as (x0 y0 + x1 y1) + x2 y2; a finite number above
//      0, or empty.
//  10. T_step: p -> R (p - (o + mp)) + (o + mm): T[4 j + i] = R_ji, T[4 j + 3] = (o_j + mm_j) - ((R_j0 c_0 + R_j1 c_1) + R_j2 c_2)
//      with c = o + mp; T[15] = 1; every entry finite, or empty.
// Only + - * / sqrt fabs copysign appear, one rounding each, in the order written, so a float64 restatement gives the same bits
// (tests/cpd_ref.py: fit64).
//
// Plain C++17 on the host (tests/test_cpd_ref.py holds it to fit64 bit for bit) and device code under hipcc; no HIP header, no
// project header but cylinder_fit.hpp.  Compile with -ffp-contract=off, as the library is: nothing below is fused.
#pragma once
#include "cylinder_fit.hpp"

namespace pcreg {

constexpr int kCpdSums = 19;
constexpr double kCpdMinRatio = 0x1p-26;          // the second singular value at or below this share of the first: no rotation

PCREG_HD inline double cpd_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// T_step (16 doubles in the library's layout, new_j = x T[4j] + y T[4j+1] + z T[4j+2] + T[4j+3]) and sigma2_out from the sums
// taken about the origin o.  false -- T and sigma2_out untouched -- when the contract says "empty".
PCREG_HD inline bool cpd_fit(const double (&s)[kCpdSums], const double (&o)[3], double (&T)[16], double& sigma2_out) {
    const double Np = s[0];
    if (!(Np > 0.0) || !fit_cylinders_finite(Np)) return false;
    const double Sp[3] = {s[1], s[2], s[3]}, Sm[3] = {s[4], s[5], s[6]};
    const double mp[3] = {Sp[0] / Np, Sp[1] / Np, Sp[2] / Np}, mm[3] = {Sm[0] / Np, Sm[1] / Np, Sm[2] / Np};
    double A[3][3], sc = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            A[a][b] = s[7 + 3 * b + a] - mm[a] * Sp[b];
            if (!fit_cylinders_finite(A[a][b])) return false;
            if (fabs(A[a][b]) > sc) sc = fabs(A[a][b]);
        }
    if (!(sc > 0.0)) return false;
    double An[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) An[a][b] = A[a][b] / sc;
    double g[6], V[9];
    g[0] = (An[0][0] * An[0][0] + An[1][0] * An[1][0]) + An[2][0] * An[2][0];
    g[1] = (An[0][0] * An[0][1] + An[1][0] * An[1][1]) + An[2][0] * An[2][1];
    g[2] = (An[0][0] * An[0][2] + An[1][0] * An[1][2]) + An[2][0] * An[2][2];
    g[3] = (An[0][1] * An[0][1] + An[1][1] * An[1][1]) + An[2][1] * An[2][1];
    g[4] = (An[0][1] * An[0][2] + An[1][1] * An[1][2]) + An[2][1] * An[2][2];
    g[5] = (An[0][2] * An[0][2] + An[1][2] * An[1][2]) + An[2][2] * An[2][2];
    fit_cylinders_jacobi(g, V);
    const double l0 = g[0], l1 = g[3], l2 = g[5];
    if (!fit_cylinders_finite(l0) || !fit_cylinders_finite(l1) || !fit_cylinders_finite(l2)) return false;
    int i1 = 0;                                                   // (no indexing by a variable: the device keeps V in registers)
    if (l1 > l0) i1 = 1;
    if (l2 > (i1 == 1 ? l1 : l0)) i1 = 2;
    const int oa = i1 == 0 ? 1 : 0, ob = i1 == 2 ? 1 : 2;
    const double la = oa == 0 ? l0 : l1, lb = ob == 1 ? l1 : l2;
    const int i2 = lb > la ? ob : oa;
    const double v1[3] = {i1 == 0 ? V[0] : i1 == 1 ? V[1] : V[2], i1 == 0 ? V[3] : i1 == 1 ? V[4] : V[5], i1 == 0 ? V[6] : i1 == 1 ? V[7] : V[8]};
    const double v2[3] = {i2 == 0 ? V[0] : i2 == 1 ? V[1] : V[2], i2 == 0 ? V[3] : i2 == 1 ? V[4] : V[5], i2 == 0 ? V[6] : i2 == 1 ? V[7] : V[8]};
    double w1[3], w2[3];
    for (int a = 0; a < 3; ++a) {
        w1[a] = (An[a][0] * v1[0] + An[a][1] * v1[1]) + An[a][2] * v1[2];
        w2[a] = (An[a][0] * v2[0] + An[a][1] * v2[1]) + An[a][2] * v2[2];
    }
    const double n1 = cpd_dot(w1, w1);
    if (!fit_cylinders_radicand_ok(n1)) return false;
    const double s1 = sqrt(n1);
    const double u1[3] = {w1[0] / s1, w1[1] / s1, w1[2] / s1};
    const double d = cpd_dot(u1, w2);
    for (int a = 0; a < 3; ++a) w2[a] = w2[a] - d * u1[a];
    const double n2 = cpd_dot(w2, w2);
    if (!fit_cylinders_radicand_ok(n2)) return false;
    const double s2 = sqrt(n2);
    if (!(s2 > kCpdMinRatio * s1)) return false;
    const double u2[3] = {w2[0] / s2, w2[1] / s2, w2[2] / s2};
    double u3[3], v3[3];
    fit_cylinders_cross(u1, u2, u3);
    fit_cylinders_cross(v1, v2, v3);
    double R[3][3], tr = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            R[a][b] = (u1[a] * v1[b] + u2[a] * v2[b]) + u3[a] * v3[b];
            tr = tr + A[a][b] * R[a][b];
        }
    const double sig = (((s[17] - cpd_dot(mm, Sm)) - 2.0 * tr) + (s[16] - cpd_dot(mp, Sp))) / (3.0 * Np);
    if (!(sig > 0.0) || !fit_cylinders_finite(sig)) return false;
    const double c[3] = {o[0] + mp[0], o[1] + mp[1], o[2] + mp[2]};
    double out[16];
    for (int j = 0; j < 3; ++j) {
        for (int i = 0; i < 3; ++i) out[4 * j + i] = R[j][i];
        out[4 * j + 3] = (o[j] + mm[j]) - ((R[j][0] * c[0] + R[j][1] * c[1]) + R[j][2] * c[2]);
    }
    out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
    for (int e = 0; e < 12; ++e)
        if (!fit_cylinders_finite(out[e])) return false;
    for (int e = 0; e < 16; ++e) T[e] = out[e];
    sigma2_out = sig;
    return true;
}

}  // namespace pcreg
