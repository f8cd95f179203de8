// pcreg_amd/csrc/cull_rule.hpp -- the culling rule of the point search, its one definition.
//
// A box B of queries with a bound D on the distance that still matters, a box T of model rows: T is skipped when
//     G2 > 1e-30  &&  G2 (1 - 32u) > D,      G2 = g_x^2 + g_y^2 + g_z^2,  g_c = max(0, T.lo_c - B.hi_c, B.lo_c - T.hi_c),
// the gaps formed in double from the float boxes, u = 2^-24.  Then every computed fp32 distance fmaf(dz,dz, fmaf(dy,dy, dx*dx))
// from a point of B to a point of T exceeds D: the soundness argument is DESIGN 4.1's.  What a caller owes: culling switched
// on, a finite D, boxes without NaN (an empty box (+inf, -inf) has infinite gaps and is skipped for any finite D).
//
// Plain C++17 on the host (tests/test_cull_rule_host.py holds it to the float64 reference) and device code under hipcc; no
// HIP header, no project header.  Compile with -ffp-contract=off, as the library is: the sums below are not fused.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PCREG_HD __host__ __device__
#else
#define PCREG_HD
#endif

namespace pcreg {

// G2 between the box (tlo, thi) and the box (blo, bhi), three coordinates each.  Either side may be floats or doubles already
// converted (the conversion is exact); a point passes lo = hi.
template <typename T, typename B>
PCREG_HD inline double cull_gap2(const T* tlo, const T* thi, const B* blo, const B* bhi) {
    double g2 = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double gap = fmax(0.0, fmax((double)tlo[c] - (double)bhi[c], (double)blo[c] - (double)thi[c]));
        g2 += gap * gap;
    }
    return g2;
}

// the verdict: a relative margin of 32u, and no bound at all below 1e-30 (subnormal squares)
PCREG_HD inline bool cull_skips(double g2, float D) {
    const double u = 5.9604644775390625e-08;
    return g2 > 1e-30 && g2 * (1.0 - 32.0 * u) > (double)D;
}

}  // namespace pcreg
