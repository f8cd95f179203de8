// pcreg_amd/csrc/info_pair.hpp -- the 27 accumulated terms of one pair with an information matrix, their one definition: the
// NDT step (pcreg_ndt_refit_f32's contract, include/pcreg.h) adds them weighted by the pair's e, the plane-to-plane
// step (pcreg_model_refit_gicp_f32's) unweighted with C := W of gicp_pair.hpp.
//
//   C[6]   the pair's symmetric information matrix, xx xy xz yy yz zz
//   x[3]   the residual (moved point - mean, or moved point - model row)
//   u[3]   the lever (moved point - origin)
//   y  = C x, each row (C_a0 x_0 + C_a1 x_1) + C_a2 x_2;  qq = (x_0 y_0 + x_1 y_1) + x_2 y_2
//   W_a = u x (row a of C), so (W_a)_j is component a of C c_j with c_j = e_j x u;  M = u x (W_0j, W_1j, W_2j): M_i = c_i . C c_j
//   acc[info_tri(i, j)]       += M_i          i <= j < 3     the rotation block of J^T C J, J = (c_0 c_1 c_2 I)
//   acc[info_tri(i, 3 + j)]   += (W_j)_i      i, j < 3       c_i . (column j of C)
//   acc[info_tri(3+a, 3+b)]   += C_ab         a <= b
//   acc[21 + i] += (u x y)_i;  acc[24 + i] += y_i            J^T y
// in the order j = 0, 1, 2 (its M terms, then its W terms), the C block, then i = 0, 1, 2 (u x y, then y).  kWeighted: each add
// is fma(e, term, sum), one rounding; otherwise sum + term and e is not read -- fma(1.0, term, sum) has the same bits.  The
// 28th sum of the layout (plane_fit.hpp) stays with the caller: NDT's is se + e, the plane-to-plane step's rr + qq.
// info_pair is info_residual (y, qq) followed by info_terms (the 27 adds); NDT calls the two apart, its e being exp(-d2/2 qq).
// A cross product's component is fl(fl(a b) - fl(c d)); only + - * and fma appear, in the order written, so a float64
// restatement gives the same bits (tests/ndt_ref.py: info_pair64).
//
// Plain C++17 on the host (tests/test_info_pair_host.py holds it to info_pair64 bit for bit) and device code under hipcc; no HIP
// header, no project header.  Compile with -ffp-contract=off, as the library is: nothing below is fused but the fma.
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

// plane_fit.hpp's plane_tri: the place of A_ij (i <= j) among the sums
PCREG_HD constexpr int info_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

PCREG_HD inline void info_cross(const double (&a)[3], double b0, double b1, double b2, double (&c)[3]) {
    c[0] = a[1] * b2 - a[2] * b1;
    c[1] = a[2] * b0 - a[0] * b2;
    c[2] = a[0] * b1 - a[1] * b0;
}

template <bool kWeighted>
PCREG_HD inline double info_add(double e, double term, double sum) {
    if constexpr (kWeighted) return fma(e, term, sum);
    else return sum + term;
}

// y = C x; returns qq = x . y (NDT's weight e is a function of it, so it comes before the terms)
PCREG_HD inline double info_residual(const double (&C)[6], const double (&x)[3], double (&y)[3]) {
    y[0] = (C[0] * x[0] + C[1] * x[1]) + C[2] * x[2];
    y[1] = (C[1] * x[0] + C[3] * x[1]) + C[4] * x[2];
    y[2] = (C[2] * x[0] + C[4] * x[1]) + C[5] * x[2];
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

// the 27 terms of a pair whose y = C x is known
template <bool kWeighted>
PCREG_HD inline void info_terms(const double (&C)[6], const double (&y)[3], const double (&u)[3], double e, double (&acc)[27]) {
    double W[3][3], M[3], gy[3];
    info_cross(u, C[0], C[1], C[2], W[0]);
    info_cross(u, C[1], C[3], C[4], W[1]);
    info_cross(u, C[2], C[4], C[5], W[2]);
    for (int j = 0; j < 3; ++j) {
        info_cross(u, W[0][j], W[1][j], W[2][j], M);
        for (int i = 0; i <= j; ++i) acc[info_tri(i, j)] = info_add<kWeighted>(e, M[i], acc[info_tri(i, j)]);
        for (int i = 0; i < 3; ++i) acc[info_tri(i, 3 + j)] = info_add<kWeighted>(e, W[j][i], acc[info_tri(i, 3 + j)]);
    }
    acc[info_tri(3, 3)] = info_add<kWeighted>(e, C[0], acc[info_tri(3, 3)]); acc[info_tri(3, 4)] = info_add<kWeighted>(e, C[1], acc[info_tri(3, 4)]);
    acc[info_tri(3, 5)] = info_add<kWeighted>(e, C[2], acc[info_tri(3, 5)]); acc[info_tri(4, 4)] = info_add<kWeighted>(e, C[3], acc[info_tri(4, 4)]);
    acc[info_tri(4, 5)] = info_add<kWeighted>(e, C[4], acc[info_tri(4, 5)]); acc[info_tri(5, 5)] = info_add<kWeighted>(e, C[5], acc[info_tri(5, 5)]);
    info_cross(u, y[0], y[1], y[2], gy);
    for (int i = 0; i < 3; ++i) {
        acc[21 + i] = info_add<kWeighted>(e, gy[i], acc[21 + i]);
        acc[24 + i] = info_add<kWeighted>(e, y[i], acc[24 + i]);
    }
}

// both: a pair whose weight does not depend on qq
template <bool kWeighted>
PCREG_HD inline void info_pair(const double (&C)[6], const double (&x)[3], const double (&u)[3], double e, double (&acc)[27], double (&y)[3],
                               double& qq) {
    qq = info_residual(C, x, y);
    info_terms<kWeighted>(C, y, u, e, acc);
}

}  // namespace pcreg
