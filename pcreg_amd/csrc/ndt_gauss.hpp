// pcreg_amd/csrc/ndt_gauss.hpp -- the Gaussian of one voxel of the NDT table (pcreg_ndt's contract, include/pcreg.h),
// its one definition: from the voxel's member rows, in ascending original row order, to (mean, C) or to "void".
//
//   1. THE MEAN      s = 0.0; s = s + (double)x_i over the members in order, per coordinate; mean = s / (double)count.
//   2. THE MOMENTS   m = {0, 0, 0, 0, 0, 0} (xx xy xz yy yz zz); per member in order d = (double)x_i - mean by component and
//                    m_ab = m_ab + d_a * d_b (a product, then an addition: nothing fused); cov_ab = m_ab / (double)(count - 1).
//   3. THE AXES      fit_cylinders_jacobi (cylinder_fit.hpp) on cov: eigenvalues l_0, l_1, l_2 on the diagonal in place, the
//                    eigenvectors the columns of V (V[3 a + k] is component a of v_k).
//   4. THE FLOOR     lmax = l_0; if (l_1 > lmax) lmax = l_1; if (l_2 > lmax) lmax = l_2.  VOID when some l_k is not finite or lmax is
//                    not above 0.  f = 0.01 * lmax; l_k = f where l_k < f (a negative l_k of a flat voxel too).
//   5. C             for a <= b (xx xy xz yy yz zz): C_ab = ((V[3a] * V[3b]) / l_0 + (V[3a+1] * V[3b+1]) / l_1) + (V[3a+2] * V[3b+2]) / l_2.
// Only + - * / sqrt fabs copysign appear, one rounding each, in the order written, so a float64 restatement gives the same bits
// (tests/ndt_ref.py: gauss64).  The floor bounds the condition number of C by 100 (up to Jacobi's residual).
//
// Plain C++17 on the host (tests/test_ndt_gauss_host.py holds it to gauss64 bit for bit) and device code under hipcc; no HIP
// header, no project header but cylinder_fit.hpp.  Compile with -ffp-contract=off, as the library is: nothing below is fused.
#pragma once
#include "cylinder_fit.hpp"

namespace pcreg {

constexpr int kNdtMinPointsLeast = 3;             // the smallest min_points a table takes
constexpr double kNdtFloor = 0.01;                // an eigenvalue below this share of the largest one is raised to it

// (mean, C) of the `count` members row(i) -> (x, y, z), i = 0 .. count - 1 in ascending original row order; `row` is called twice
// per member.  false -- mean written, C untouched -- when the voxel is void.  count >= 2 (the callers ask count >= min_points >= 3).
template <class Row>
PCREG_HD inline bool ndt_gauss(int count, Row row, double (&mean)[3], double (&C)[6]) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < count; ++i) {
        float x, y, z;
        row(i, x, y, z);
        s[0] = s[0] + (double)x; s[1] = s[1] + (double)y; s[2] = s[2] + (double)z;
    }
    const double dn = (double)count;
    mean[0] = s[0] / dn; mean[1] = s[1] / dn; mean[2] = s[2] / dn;
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < count; ++i) {
        float x, y, z;
        row(i, x, y, z);
        const double d0 = (double)x - mean[0], d1 = (double)y - mean[1], d2 = (double)z - mean[2];
        m[0] = m[0] + d0 * d0; m[1] = m[1] + d0 * d1; m[2] = m[2] + d0 * d2;
        m[3] = m[3] + d1 * d1; m[4] = m[4] + d1 * d2; m[5] = m[5] + d2 * d2;
    }
    const double dm = (double)(count - 1);
    double a[6], V[9];
    for (int k = 0; k < 6; ++k) a[k] = m[k] / dm;
    fit_cylinders_jacobi(a, V);
    double l0 = a[0], l1 = a[3], l2 = a[5];
    if (!fit_cylinders_finite(l0) || !fit_cylinders_finite(l1) || !fit_cylinders_finite(l2)) return false;
    double lmax = l0;
    if (l1 > lmax) lmax = l1;
    if (l2 > lmax) lmax = l2;
    if (!(lmax > 0.0)) return false;
    const double f = kNdtFloor * lmax;
    if (l0 < f) l0 = f;
    if (l1 < f) l1 = f;
    if (l2 < f) l2 = f;
    C[0] = ((V[0] * V[0]) / l0 + (V[1] * V[1]) / l1) + (V[2] * V[2]) / l2;
    C[1] = ((V[0] * V[3]) / l0 + (V[1] * V[4]) / l1) + (V[2] * V[5]) / l2;
    C[2] = ((V[0] * V[6]) / l0 + (V[1] * V[7]) / l1) + (V[2] * V[8]) / l2;
    C[3] = ((V[3] * V[3]) / l0 + (V[4] * V[4]) / l1) + (V[5] * V[5]) / l2;
    C[4] = ((V[3] * V[6]) / l0 + (V[4] * V[7]) / l1) + (V[5] * V[8]) / l2;
    C[5] = ((V[6] * V[6]) / l0 + (V[7] * V[7]) / l1) + (V[8] * V[8]) / l2;
    return true;
}

}  // namespace pcreg
