// pcreg_amd/csrc/fpfh_pair.hpp -- the pair features and bins of the FPFH contract (pcreg_model_fpfh_f32 in include/pcreg.h; DESIGN
// 4.19), shared by the k-nearest form (knn_fpfh.hip) and the radius form (knn_fpfh_radius.hip): both count the same pairs into the
// same bins, whatever neighbourhood rule chose the pairs.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace pcreg {

constexpr int kFpfhBins = 11;                        // per feature
constexpr int kFpfhDim = 3 * kFpfhBins;              // 33

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// the bin of a feature already mapped onto [0, 1]: floor(11 x) clamped to 0 .. 10
__device__ __forceinline__ int fpfh_bin(double x01) { return (int)fmin(fmax(floor((double)kFpfhBins * x01), 0.0), (double)(kFpfhBins - 1)); }

// The pair (i, j) of the contract: p the coordinates, n the normals, widened fp32.  true: the pair contributes, b1 .. b3 its bins.
__device__ __forceinline__ bool fpfh_pair(double pix, double piy, double piz, double nix, double niy, double niz, double pjx, double pjy,
                                          double pjz, double njx, double njy, double njz, int& b1, int& b2, int& b3) {
    const double kPi = 3.14159265358979323846;
    double dx = pjx - pix, dy = pjy - piy, dz = pjz - piz;
    const double len = __dsqrt_rn(dot3(dx, dy, dz, dx, dy, dz));
    const double ai = dot3(nix, niy, niz, dx, dy, dz) / len;
    const double aj = dot3(njx, njy, njz, dx, dy, dz) / len;
    const bool swap = fabs(ai) < fabs(aj);                        // strictly: a tie keeps i the source
    const double sx = swap ? njx : nix, sy = swap ? njy : niy, sz = swap ? njz : niz;       // ns
    const double tx = swap ? nix : njx, ty = swap ? niy : njy, tz = swap ? niz : njz;       // nt
    dx = swap ? -dx : dx; dy = swap ? -dy : dy; dz = swap ? -dz : dz;
    const double f3 = swap ? -aj : ai;
    double vx = dy * sz - dz * sy, vy = dz * sx - dx * sz, vz = dx * sy - dy * sx;          // v = d x ns
    const double vl = __dsqrt_rn(dot3(vx, vy, vz, vx, vy, vz));
    vx = vx / vl; vy = vy / vl; vz = vz / vl;
    const double wx = sy * vz - sz * vy, wy = sz * vx - sx * vz, wz = sx * vy - sy * vx;    // w = ns x v
    const double f2 = dot3(vx, vy, vz, tx, ty, tz);
    const double f1 = atan2(dot3(wx, wy, wz, tx, ty, tz), dot3(sx, sy, sz, tx, ty, tz));
    const double inf = (double)INFINITY;
    const bool finite_n = fabs(nix) < inf && fabs(niy) < inf && fabs(niz) < inf && fabs(njx) < inf && fabs(njy) < inf && fabs(njz) < inf;
    b1 = fpfh_bin((f1 + kPi) / (2.0 * kPi));
    b2 = fpfh_bin((f2 + 1.0) * 0.5);
    b3 = fpfh_bin((f3 + 1.0) * 0.5);
    return len > 0.0 && vl > 0.0 && f1 == f1 && f2 == f2 && f3 == f3 && finite_n;
}

}  // namespace pcreg
