// pcreg_amd/csrc/knn_selfjoin.hpp -- what the self-joins of a prepared model that keep a k-list per row share (knn_normals.hip,
// knn_denoise.hip, knn_fpfh.hip), and only that: the seed bound of every sorted row and its launch, the
// k-th entry of a register list, the bound of a workgroup's tile, and the (distance, row) k-list walk of the normals and the
// FPFH.  What every self-join does around walk_tiles is knn_walk.hpp's; the KB dispatch is knn_klist.hpp's.
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
constexpr int kSelfKbMin = 4;                        // the smallest list of a self-join: KB = 4, 8, 16, 32
static_assert(kNKnnMaxK <= kNSeedWin, "the seed window holds at least k rows");

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
    if (lane == 0) dk[sr] = finite3(qx, qy, qz) ? v : 0.0f;
}
// its launch: dk[sorted row] for M > 0 rows
inline void launch_selfjoin_seed(const ModelView& v, int k, float* dk, hipStream_t st) {
    hipLaunchKernelGGL(normals_seed_kernel, dim3((unsigned)((v.M + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st, (const float*)v.ms,
                       v.M, k, dk);
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

// what a k-list self-join starts a row's bound from: its seed; a dead lane admits nothing, a NaN seed is no bound
__device__ __forceinline__ float selfjoin_row_bound(const float* __restrict__ dk, const WalkSelfRow& q) {
    const float thr = q.in_model ? dk[q.sr] : -INFINITY;
    return thr == thr ? thr : INFINITY;
}

// ---- the (distance, row) k-list walk of the normals and the FPFH --------------------------------------------------------
// Workgroup blockIdx.x = (tile a, part) owns 64 sorted rows of tile a, four lanes per row, each with a sorted list of KB >= k
// (distance, row) pairs in registers.  The block's box is tile a's, its bound D the largest seed over tile a's rows; a tile on
// EITHER side of a is visited unless the visit rule skips it.  A row enters a list only when d <= thr, thr = min(seed, the k-th
// entry of any of the row's four lists), each of which bounds the true k-th distance from above.  After the two merges every
// lane of a row holds the row's list in (ld, li), (distance, original row) ascending, the empty entries (+inf, -1) last.
// -> this thread's row.  Counts one search of n_tiles^2 pairs.
// The walk works on a list of its OWN and hands it over at the end: on the caller's arrays, reached through the reference
// parameters, the compiler turned the insertion's selects into branches and moves (normals_walk_kernel<32>: 208 VGPRs for 179, and
// 3 % slower at k = 32).
template <int KB>
__device__ __forceinline__ WalkSelfRow selfjoin_klist_walk(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                           const float* __restrict__ tbox, int n_tiles, int cull, int k,
                                                           const float* __restrict__ dk, unsigned long long* __restrict__ stats,
                                                           float (&ld_out)[KB], int (&li_out)[KB]) {
    float ld[KB]; int li[KB];
    __shared__ WalkLds lds;
    __shared__ float s_red[kBlock / 64];
    const int ta = blockIdx.x / kWalkWgPerTile, part = blockIdx.x % kWalkWgPerTile;
    walk_count_search(stats, (unsigned long long)n_tiles * (unsigned long long)n_tiles);
    float abox[6];
    walk_tile_box(tbox, ta, abox);
    const float D = selfjoin_tile_bound(dk, ta, M, s_red);
    const WalkSelfRow q = walk_self_row(ms, perm, M, ta, part);
    float thr = selfjoin_row_bound(dk, q);
#pragma unroll
    for (int s = 0; s < KB; ++s) { ld[s] = INFINITY; li[s] = -1; }
    walk_tiles(
        lds, 0, n_tiles, q.qx, q.qy, q.qz, part == 0 ? stats : nullptr,
        [&](int ct) { return walk_visits(tbox, ct, abox, D, cull); },
        [&](int r) { return walk_row_finite(ms, perm, M, r); },
        [](int) {},
        [&](int, const float4 (&p)[4], float (&d)[4]) {
            if (fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= thr) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d[u] <= thr) {
                        klist_insert<KB>(ld, li, d[u], __float_as_int(p[u].w));
                        thr = fminf(thr, klist_kth_reg<KB>(ld, k));
                    }
                }
            }
        },
        [&] {
            thr = fminf(thr, __shfl_xor(thr, 1));                 // the row's four lanes share the tightest bound
            thr = fminf(thr, __shfl_xor(thr, 2));
        });
    klist_merge_xor<KB>(ld, li, 1);
    klist_merge_xor<KB>(ld, li, 2);
#pragma unroll
    for (int s = 0; s < KB; ++s) { ld_out[s] = ld[s]; li_out[s] = li[s]; }
    return q;
}

}  // namespace
}  // namespace pcreg
