// pcreg_amd/csrc/knn_selfjoin.hpp -- what the self-joins of a prepared model that keep a k-list per row share (knn_normals.hip,
// knn_denoise.hip): the seed bound of every sorted row, the k-th entry of a register list, the finite test,
// and the bound of a workgroup's tile.
#pragma once
#include "common.hpp"
#include "knn_fast_common.hpp"
#include "knn_walk.hpp"
#include "knn_klist.hpp"
#include <cmath>

namespace pcreg {
namespace {

constexpr int kNKnnMaxK = PCREG_KNN_MAX_K;
constexpr int kNSeedWin = 64;                        // sorted rows the seed bound looks at (one per lane of a wave)
constexpr int kNWgPerTile = kT16 / kWalkQPerWg;      // 8 workgroups per tile a, 64 of its rows each
static_assert(kNKnnMaxK <= kNSeedWin, "the seed window holds at least k rows");

__device__ __forceinline__ bool nfinite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;       // (false for NaN)
}

// The k-th entry of a sorted list, as klist_kth gives it: the smallest entry at or behind place k - 1.  klist_kth's chain of
// selects between list entries is folded by the compiler into ONE load at a computed address, which keeps the whole list in
// memory (LDS up to KB = 8, 80 / 144 bytes of scratch at KB = 16 / 32); a select against a constant cannot be folded that way.
template <int KB>
__device__ __forceinline__ float klist_kth_reg(const float (&ld)[KB], int k) {
    float v = INFINITY;
#pragma unroll
    for (int s = 0; s < KB; ++s) v = fminf(v, s >= k - 1 ? ld[s] : INFINITY);
    return v;
}

// ---- N1. seed bound: one wave per sorted row -------------------------------------------------------------------------
// The window: 64 consecutive sorted rows centred on the row, clamped into [0, M); it holds the row itself.  Its k-th smallest
// distance (bitonic sort across the wave) bounds the true k-th distance from above; a NaN or infinite distance (a non-finite
// row of the window) counts as +inf, so the bound never shrinks below a finite row's distance.
__global__ __launch_bounds__(kBlock) void normals_seed_kernel(const float* __restrict__ ms, int M, int k, float* __restrict__ dk) {
    const int lane = threadIdx.x & 63;
    const long long sr = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (sr >= M) return;                                        // (wave-uniform)
    const float qx = ms[sr], qy = ms[sr + (size_t)M], qz = ms[sr + 2 * (size_t)M];
    int w0 = (int)sr - kNSeedWin / 2;
    w0 = min(w0, M - kNSeedWin); w0 = max(w0, 0);
    const int r = w0 + lane;
    float d = INFINITY;
    if (r < M) {
        d = point_d2(qx, qy, qz, ms[r], ms[r + (size_t)M], ms[r + 2 * (size_t)M]);
        if (!(d == d)) d = INFINITY;
    }
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const float o = __shfl_xor(d, stride);
            const bool up = (lane & size) == 0, lower = (lane & stride) == 0;
            d = (lower == up) ? fminf(d, o) : fmaxf(d, o);
        }
    }
    const float v = __shfl(d, k - 1);
    if (lane == 0) dk[sr] = nfinite3(qx, qy, qz) ? v : 0.0f;
}

// The bound of the workgroups of tile ta: the largest seed over ALL of tile ta's rows (every workgroup forms the same value).
// One barrier inside; s_red is the caller's.
__device__ __forceinline__ float selfjoin_tile_bound(const float* __restrict__ dk, int ta, int M, float (&s_red)[kBlock / 64]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float D = 0.0f;
    for (int r = tid; r < kT16; r += kBlock) {
        const long long s = (long long)ta * kT16 + r;
        if (s < M) {
            const float e = dk[s];
            D = e < INFINITY ? fmaxf(D, e) : INFINITY;            // +inf (or NaN): no bound, culling off for the block
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) D = fmaxf(D, __shfl_xor(D, o));
    if (lane == 0) s_red[wave] = D;
    __syncthreads();
    return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

}  // namespace
}  // namespace pcreg
