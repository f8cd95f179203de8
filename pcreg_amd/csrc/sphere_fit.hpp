// pcreg_amd/csrc/sphere_fit.hpp -- the algebraic least-squares sphere of the refit of pcreg_model_fit_spheres_f32 (its contract,
// include/pcreg.h), its one definition: from the rounded normal equations of a round's inliers to (centre, R), or to
// "not used".
//
// With g the inliers' quantised differences from the trial's first row and w = |g|^2, the sphere |g - c|^2 = R^2 is the linear
// model g . a + beta = w with a = 2 c and beta = R^2 - |c|^2.  Eliminating beta from its normal equations leaves
//   N a = h,   N = n S2 - S1 S1^T  (N6: xx xy xz yy yz zz),   h = n (sum g w) - S1 (sum w),
// both formed exactly in integers by the caller and rounded once per entry.  Here: N = L L^T, L y = h, L^T a = y, then
//   c_g = a / 2,   beta = (sw - ((a0 S1x + a1 S1y) + a2 S1z)) / n,   R_g^2 = beta + ((cx cx + cy cy) + cz cz),
//   centre = p0 + c_g back,   R = sqrt(R_g^2) back          (back = 2^-(17 - e), a power of two)
// Only + - * / sqrt appear, one rounding each, in the order written, so a float64 restatement gives the same bits
// (tests/spheres_ref.py: finish64).
//
// Plain C++17 on the host (tests/test_sphere_fit_host.py holds it to finish64 bit for bit) and device code under hipcc; no HIP
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

PCREG_HD inline bool fit_spheres_finite(double v) { return v - v == 0.0; }
// a radicand the factorisation may take the root of: a finite number above 0 (a NaN fails)
PCREG_HD inline bool fit_spheres_radicand_ok(double v) { return v > 0.0 && fit_spheres_finite(v); }

// (centre, R) from N6, h, S1 = (double)sum g, sw = (double)sum w, n = (double)count, the trial's first row p0 widened to double
// and back = 2^-(17 - e).  false -- and the outputs untouched -- when the contract says the refit is NOT USED: a radicand of the
// factorisation or R_g^2 not a finite number above 0, centre or R not finite, (float)R outside [min_radius, max_radius].
PCREG_HD inline bool fit_spheres_solve(const double (&N6)[6], const double (&h)[3], const double (&S1)[3], double sw, double n,
                                      const double (&p0)[3], double back, float min_radius, float max_radius,
                                      double (&centre)[3], double& R) {
    // 1. N = L L^T, column by column; every sum subtracted term by term, left to right
    const double r0 = N6[0];
    if (!fit_spheres_radicand_ok(r0)) return false;
    const double L00 = sqrt(r0);
    const double L10 = N6[1] / L00;
    const double L20 = N6[2] / L00;
    const double r1 = N6[3] - L10 * L10;
    if (!fit_spheres_radicand_ok(r1)) return false;
    const double L11 = sqrt(r1);
    const double L21 = (N6[4] - L20 * L10) / L11;
    const double r2 = (N6[5] - L20 * L20) - L21 * L21;
    if (!fit_spheres_radicand_ok(r2)) return false;
    const double L22 = sqrt(r2);
    // 2. L y = h, ascending;  3. L^T a = y, descending, the lower index subtracted first
    const double y0 = h[0] / L00;
    const double y1 = (h[1] - L10 * y0) / L11;
    const double y2 = ((h[2] - L20 * y0) - L21 * y1) / L22;
    const double a2 = y2 / L22;
    const double a1 = (y1 - L21 * a2) / L11;
    const double a0 = ((y0 - L10 * a1) - L20 * a2) / L00;
    // 4. c_g, beta, R_g^2
    const double cx = a0 / 2.0, cy = a1 / 2.0, cz = a2 / 2.0;
    const double beta = (sw - ((a0 * S1[0] + a1 * S1[1]) + a2 * S1[2])) / n;
    const double Rg2 = beta + ((cx * cx + cy * cy) + cz * cz);
    if (!fit_spheres_radicand_ok(Rg2)) return false;
    // 5. back to the cloud's units
    const double ox = p0[0] + cx * back, oy = p0[1] + cy * back, oz = p0[2] + cz * back;
    const double Rr = sqrt(Rg2) * back;
    if (!fit_spheres_finite(ox) || !fit_spheres_finite(oy) || !fit_spheres_finite(oz) || !fit_spheres_finite(Rr)) return false;
    const float Rf = (float)Rr;
    if (!(Rf >= min_radius && Rf <= max_radius)) return false;
    centre[0] = ox; centre[1] = oy; centre[2] = oz;
    R = Rr;
    return true;
}

}  // namespace pcreg
