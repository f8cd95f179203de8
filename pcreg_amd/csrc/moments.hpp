// pcreg_amd/csrc/moments.hpp -- the 27 moments of a correspondence set that estimateTransform is fitted from (fit_moments,
// ransac.hip) and the wave-level fp64 sums that reduce them, their one definition: ransac.hip accumulates them per hypothesis,
// knn_score.hip per (candidate transform, chunk of queries).
#pragma once
#include <hip/hip_runtime.h>

namespace pcreg {
namespace {

// ---------------------------------------------------------------- lane utilities
__device__ __forceinline__ double rdlane(double v, int l) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// wave_sum of 27 values at once, the same bits as 27 calls.  wave_sum's butterfly adds lane l and lane l ^ o for o = 32, 16, ..., 1;
// after every step the two partners hold the same bits (fp addition commutes), so only ONE of them needs to go on with a given
// value: at distance 32 the lower half-wave keeps values 0-13 and the upper one 14-26, each sending the other its remaining
// half, and so on down -- 14 + 7 + 4 + 2 + 1 + 1 = 29 exchanged doubles instead of 27 x 6 = 162.  Value k ends in the lanes whose
// bits 5..1 spell its path (k = 14 b5 + 7 b4 + 4 b3 + 2 b2 + b1) and is broadcast from there with v_readlane.
__device__ __forceinline__ void wave_sum27(double (&v)[27]) {
    const int lane = threadIdx.x & 63;
    const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8, b2 = lane & 4, b1 = lane & 2;
    double k1[14], k2[8], k3[4], k4[2];
#pragma unroll
    for (int j = 0; j < 14; ++j) {
        const double hi = 14 + j < 27 ? v[14 + j < 27 ? 14 + j : 26] : 0.0;
        k1[j] = (b5 ? hi : v[j]) + __shfl_xor(b5 ? v[j] : hi, 32);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) k2[j] = (b4 ? k1[7 + j] : k1[j]) + __shfl_xor(b4 ? k1[j] : k1[7 + j], 16);
    k2[7] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) k3[j] = (b3 ? k2[4 + j] : k2[j]) + __shfl_xor(b3 ? k2[j] : k2[4 + j], 8);
#pragma unroll
    for (int j = 0; j < 2; ++j) k4[j] = (b2 ? k3[2 + j] : k3[j]) + __shfl_xor(b2 ? k3[j] : k3[2 + j], 4);
    double k5 = (b1 ? k4[1] : k4[0]) + __shfl_xor(b1 ? k4[0] : k4[1], 2);
    k5 += __shfl_xor(k5, 1);
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const int c5 = k >= 14, r5 = k - 14 * c5, c4 = r5 >= 7, r4 = r5 - 7 * c4, c3 = r4 >= 4, r3 = r4 - 4 * c3, c2 = r3 >= 2, c1 = r3 - 2 * c2;
        v[k] = rdlane(k5, 32 * c5 + 16 * c4 + 8 * c3 + 4 * c2 + 2 * c1);
    }
}

// Moments of a correspondence set, taken about a fixed origin (o1,o2) inside the data (ransac_origin) so that the
// centring of estimateTransform.m:55-58 does not cancel digits:
//   mom[0..2]  = sum(d')      mom[3..5] = sum(m')            (d' = p1-o1, m' = p2-o2)
//   mom[6..14] = sum(m'_i d'_j), row-major i,j
//   mom[15..20]= raw Gram of p1 (xx,xy,xz,yy,yz,zz), mom[21..26] = raw Gram of p2.
__device__ __forceinline__ void mom_core(double (&mom)[27], const double (&p)[6], const double (&o)[6]) {
    double d0 = p[0] - o[0], d1 = p[1] - o[1], d2 = p[2] - o[2];
    double m0 = p[3] - o[3], m1 = p[4] - o[4], m2 = p[5] - o[5];
    mom[0] += d0; mom[1] += d1; mom[2] += d2; mom[3] += m0; mom[4] += m1; mom[5] += m2;
    mom[6]  = fma(m0, d0, mom[6]);  mom[7]  = fma(m0, d1, mom[7]);  mom[8]  = fma(m0, d2, mom[8]);
    mom[9]  = fma(m1, d0, mom[9]);  mom[10] = fma(m1, d1, mom[10]); mom[11] = fma(m1, d2, mom[11]);
    mom[12] = fma(m2, d0, mom[12]); mom[13] = fma(m2, d1, mom[13]); mom[14] = fma(m2, d2, mom[14]);
}
// the raw Grams only feed the rank test of estimateTransform.m:11-14
__device__ __forceinline__ void mom_gram(double (&mom)[27], const double (&p)[6]) {
    mom[15] = fma(p[0], p[0], mom[15]); mom[16] = fma(p[0], p[1], mom[16]); mom[17] = fma(p[0], p[2], mom[17]);
    mom[18] = fma(p[1], p[1], mom[18]); mom[19] = fma(p[1], p[2], mom[19]); mom[20] = fma(p[2], p[2], mom[20]);
    mom[21] = fma(p[3], p[3], mom[21]); mom[22] = fma(p[3], p[4], mom[22]); mom[23] = fma(p[3], p[5], mom[23]);
    mom[24] = fma(p[4], p[4], mom[24]); mom[25] = fma(p[4], p[5], mom[25]); mom[26] = fma(p[5], p[5], mom[26]);
}
__device__ __forceinline__ void mom_accumulate(double (&mom)[27], const double (&p)[6],
                                               const double (&o)[6]) {
    mom_core(mom, p, o);
    mom_gram(mom, p);
}

}  // namespace
}  // namespace pcreg
