// pcreg_amd/csrc/plane_fit.hpp -- the fit of the point-to-plane refit (pcreg_model_refit_plane_f32's contract, include/pcreg.h;
// DESIGN 4.16), its one definition: from the 28 sums of a transform's plane pairs to T_step, or to "empty".
//
//   sums[0..20]  A_ij = sum J_i J_j, i <= j, the upper triangle row-major      J = (u x n, n), u = p - o
//   sums[21..26] g_i  = sum J_i r                                               r = n . (p - m)
//   sums[27]     rr   = sum r r   (reported, not used by the fit)
// The fit minimises sum (r + w . c + t . n)^2, that is A x = -g with x = (w, t), by a Cholesky factorisation of the matrix
// scaled to a unit diagonal; the rotation of the small vector w is the exact Cayley / quaternion form, so that T_step is a
// rigid motion whatever the size of w.  Only + - * / sqrt appear, in the order written, so a float64 restatement gives the
// same bits (tests/plane_ref.py: finish64).
//
// Plain C++17 on the host (tests/test_plane_fit_host.py holds it to finish64 bit for bit) and device code under hipcc; no HIP
// header, no project header.  Compile with -ffp-contract=off, as the library is: nothing below is fused.
#pragma once
#include <cmath>

#if !defined(PCREG_HD)
#if defined(__HIPCC__)
#define PCREG_HD __host__ __device__
#else
#define PCREG_HD
#endif
#endif

namespace pcreg {

constexpr int kPlaneSums = 28;                    // 21 + 6 + 1
constexpr int kPlaneMinPairs = 6;                 // six unknowns
constexpr double kPlaneMinPivot = 0x1p-26;        // a pivot of the scaled matrix at or below this: the planes do not constrain x

// the place of A_ij (i <= j) among the sums
PCREG_HD constexpr int plane_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

PCREG_HD inline bool plane_finite(double v) { return v - v == 0.0; }

// T_step (16 doubles in the library's layout, new_j = x T[4j] + y T[4j+1] + z T[4j+2] + T[4j+3]) from the sums of n_plane plane
// pairs taken about the origin o.  false -- and T untouched -- when the contract says "empty": n_plane < 6, some A_ii not a
// finite number above 0, some pivot not above 2^-26, x or T_step not finite.
PCREG_HD inline bool plane_fit(const double (&sums)[kPlaneSums], int n_plane, const double (&o)[3], double (&T)[16]) {
    if (n_plane < kPlaneMinPairs) return false;
    // 1. s_i = sqrt(A_ii)
    double s[6];
    for (int i = 0; i < 6; ++i) {
        const double a = sums[plane_tri(i, i)];
        if (!(a > 0.0) || !plane_finite(a)) return false;
        s[i] = sqrt(a);
    }
    // 2. C_ij = A_ij / (s_i s_j), C_ii = 1;  3. C = L L^T row by row, every sum subtracted term by term in ascending k
    double L[6][6];
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < i; ++j) {
            double v = sums[plane_tri(j, i)] / (s[j] * s[i]);
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
        double p = 1.0;
        for (int k = 0; k < i; ++k) p = p - L[i][k] * L[i][k];
        if (!(p > kPlaneMinPivot)) return false;                 // (a NaN pivot fails too)
        L[i][i] = sqrt(p);
    }
    // 4. L y = -g / s, ascending;  5. L^T z = y, descending, its sum in ascending k;  6. x = z / s
    double y[6], x[6];
    for (int i = 0; i < 6; ++i) {
        double v = -sums[21 + i] / s[i];
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
        x[i] = v / L[i][i];                                      // (z_i, scaled in place below)
    }
    for (int i = 0; i < 6; ++i) {
        x[i] = x[i] / s[i];
        if (!plane_finite(x[i])) return false;
    }
    // the rotation of the unit quaternion (a, b, c, d) = (1, w / 2) / |(1, w / 2)|
    const double hx = x[0] / 2.0, hy = x[1] / 2.0, hz = x[2] / 2.0;
    const double S = sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz));
    const double a = 1.0 / S, b = hx / S, c = hy / S, d = hz / S;
    double R[3][3];
    R[0][0] = 1.0 - 2.0 * (c * c + d * d); R[0][1] = 2.0 * (b * c - a * d);       R[0][2] = 2.0 * (b * d + a * c);
    R[1][0] = 2.0 * (b * c + a * d);       R[1][1] = 1.0 - 2.0 * (b * b + d * d); R[1][2] = 2.0 * (c * d - a * b);
    R[2][0] = 2.0 * (b * d - a * c);       R[2][1] = 2.0 * (c * d + a * b);       R[2][2] = 1.0 - 2.0 * (b * b + c * c);
    // the step p -> R (p - o) + o + t
    double out[16];
    for (int j = 0; j < 3; ++j) {
        for (int i = 0; i < 3; ++i) out[4 * j + i] = R[j][i];
        out[4 * j + 3] = (o[j] + x[3 + j]) - ((R[j][0] * o[0] + R[j][1] * o[1]) + R[j][2] * o[2]);
    }
    out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
    for (int e = 0; e < 12; ++e)
        if (!plane_finite(out[e])) return false;
    for (int e = 0; e < 16; ++e) T[e] = out[e];
    return true;
}

}  // namespace pcreg
