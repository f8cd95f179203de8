// pcreg_amd/csrc/direct_rule.hpp -- the direct-answer rule of the two-nearest search ("Direct answers"), its one
// definition.
//
// A seeded query q holds dk: two real model rows lie within the fp32 chain distance d = fmaf(dz,dz, fmaf(dy,dy, dx*dx)),
// dx = q - m, of it.  Every row with d <= dk lies in a small box of ordering-grid cells around q:
//   * d >= fl(d_c * d_c) for each axis c (the chain only adds non-negative terms, and rounding is monotone), so the exact
//     square d_c^2 is at most dk plus half an ulp of dk: d_c^2 <= dk (1 + u) + 2^-150, u = 2^-24 (the second term covers a
//     zero or subnormal dk);
//   * d_c = fl(q_c - m_c), so |q_c - m_c| <= |d_c| / (1 - u) (a difference of floats is exact where it is subnormal).
// rho = sqrt(dk (1 + 4u) + 2^-149) (1 + 4u), formed in double, exceeds both with room for the double roundings.  Per axis,
// lo is the largest float <= q_c - rho and hi the smallest float >= q_c + rho: every float m_c with |q_c - m_c| <= rho lies
// in [lo, hi].  order_cell() -- the per-axis expression of sort_key() -- is monotone non-decreasing for inv_s >= 0 (float
// subtraction, multiplication by a non-negative number, floorf and the clamp all are; a NaN product, 0 * inf or inf * 0,
// falls to cell 0 exactly where its neighbours do), so the row's cell lies in [order_cell(lo), order_cell(hi)] on every axis.
// The two answers, and every row tied with the second, have d <= dk: the top two by (distance, original row) over the
// rows of those cells are the exhaustive search's bits.
//
// Plain C++17 on the host (tests/test_knn_direct_ref.py holds it to the float64 / np.float32 restatement) and device code
// under hipcc; no HIP header, no project header.  Compile with -ffp-contract=off, as the library is.
#pragma once
#include <cmath>

#ifndef PCREG_HD
#if defined(__HIPCC__)
#define PCREG_HD __host__ __device__
#else
#define PCREG_HD
#endif
#endif

namespace pcreg {

// A query is answered directly when dk and its coordinates are finite, its cell range holds at most kDirectCells cells and
// those cells at most kDirectRows rows.  Conditions, not measurements: everything else takes the tile walk.
constexpr int kDirectCells = 27;
constexpr int kDirectRows = 512;

// one axis of the ordering grid: the cell of coordinate v, clamped into [0, top] (NaN -> 0: fmaxf returns the number)
PCREG_HD inline float order_cell(float v, float s0, float inv_s, float top) {
    return fminf(fmaxf(floorf((v - s0) * inv_s), 0.0f), top);
}

// rho: an upper bound of |q_c - m_c| for every row m with chain distance <= dk (dk finite, >= 0)
PCREG_HD inline double direct_radius(float dk) {
    const double u = 5.9604644775390625e-08;                     // 2^-24
    return sqrt((double)dk * (1.0 + 4.0 * u) + 1.4012984643248171e-45 /* 2^-149 */) * (1.0 + 4.0 * u);
}
// the largest float <= t and the smallest float >= t (t a double, not NaN; beyond the float range: -inf / +inf)
PCREG_HD inline float direct_float_below(double t) {
    float f = (float)t;
    if ((double)f > t) f = nextafterf(f, -INFINITY);
    return f;
}
PCREG_HD inline float direct_float_above(double t) {
    float f = (float)t;
    if ((double)f < t) f = nextafterf(f, INFINITY);
    return f;
}

struct DirectRange { int lo[3], hi[3]; };
PCREG_HD inline bool direct_finite(float v) { return fabsf(v) < INFINITY; }          // (false for NaN)

// The cell range of query q with seed distance dk in the ordering grid (origin s0, inv_s >= 0, cells 0 .. top per axis).
// false: dk or a coordinate is not finite (or dk < 0) -- no range, the query takes the tile walk.
PCREG_HD inline bool direct_range(const float q[3], float dk, const float s0[3], float inv_s, int top, DirectRange* r) {
    if (!(direct_finite(dk) && dk >= 0.0f && direct_finite(q[0]) && direct_finite(q[1]) && direct_finite(q[2]))) return false;
    const double rho = direct_radius(dk);
    for (int c = 0; c < 3; ++c) {
        const float lo = direct_float_below((double)q[c] - rho), hi = direct_float_above((double)q[c] + rho);
        r->lo[c] = (int)order_cell(lo, s0[c], inv_s, (float)top);
        r->hi[c] = (int)order_cell(hi, s0[c], inv_s, (float)top);
    }
    return true;
}
PCREG_HD inline int direct_cells(const DirectRange& r) {
    return (r.hi[0] - r.lo[0] + 1) * (r.hi[1] - r.lo[1] + 1) * (r.hi[2] - r.lo[2] + 1);
}

}  // namespace pcreg
