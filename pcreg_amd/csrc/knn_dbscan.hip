// pcreg_amd/csrc/knn_dbscan.hip -- the two walks of DBSCAN on a PREPARED model that unite nothing: the neighbour
// count of every row, and the cluster of every border row.  Rows i and j (j may be i) are neighbours iff both are finite and
// d = fmaf(dz,dz, fmaf(dy,dy, dx*dx)) <= r2 in fp32 -- the clustering's predicate; a row is a core row iff it has at
// least minpts neighbours, itself included.  The union-find over the core rows, the numbering and the labels are
// knn_cluster.hip's, and so is the launcher; this file holds no atomic and no loop that reads global memory in its condition.
//   D1  dbscan_count_kernel    the FULL self-join: tile a's rows against every tile b that DESIGN 4.1's rule (D = r2, the box of
//                              tile a) does not rule out; four lanes per row count their hits in a register, two shuffles sum
//                              them, one plain store per row: cnt_sorted[sorted row]
//   D2  dbscan_init_kernel     by original row: cnt[i] = the same count, parent[i] = i, the outputs' tails cleared
//   D3  dbscan_border_kernel   after the flatten: the full self-join again, live only the finite rows that are NOT core, staged only
//                              the core rows; a hit loads the staged row's root (a plain load: the flatten is a finished launch)
//                              and the lane keeps the smallest; the smallest over a row's four lanes goes into parent[row].  The
//                              rows written (non-core) and the rows read (core) are disjoint, so no workgroup sees another's store
#include "common.hpp"
#include "knn_fast_common.hpp"
#include "knn_walk.hpp"
#include <climits>
#include <cmath>

namespace pcreg {

namespace {

// ---- D1 ---------------------------------------------------------------------------------------------------------------
// Workgroup (tile a, part p) owns sorted rows a * 512 + p * 64 + (tid >> 2), as the clustering walk does.  A non-finite row is
// staged as NaN and its own lanes admit nothing: it counts nobody and nobody counts it, itself included.
__global__ __launch_bounds__(kBlock) void dbscan_count_kernel(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                              const float* __restrict__ tbox, int n_tiles, int cull, float r2,
                                                              int32_t* __restrict__ cnt_sorted, unsigned long long* __restrict__ stats) {
    __shared__ WalkLds lds;
    const int ta = blockIdx.x / kWalkWgPerTile, part = blockIdx.x % kWalkWgPerTile;
    walk_count_search(stats, (unsigned long long)n_tiles * (unsigned long long)n_tiles);
    float abox[6];
    walk_tile_box(tbox, ta, abox);
    const WalkSelfRow q = walk_self_row(ms, perm, M, ta, part);
    const float rr = q.live ? r2 : -1.0f;                         // (a dead lane admits nothing: d is never negative)
    int n = 0;
    walk_tiles(
        lds, 0, n_tiles, q.qx, q.qy, q.qz, part == 0 ? stats : nullptr,
        [&](int ct) { return walk_visits(tbox, ct, abox, r2, cull); },
        [&](int r) { return walk_row_finite(ms, perm, M, r); },
        [](int) {},
        [&](int, const float4 (&)[4], float (&d)[4]) {
#pragma unroll
            for (int u = 0; u < 4; ++u) n += d[u] <= rr ? 1 : 0;
        },
        [] {});
    n += __shfl_xor(n, 1);
    n += __shfl_xor(n, 2);
    if (q.in_model && (threadIdx.x & (kWalkLanes - 1)) == 0) cnt_sorted[q.sr] = n;
}

// ---- D2 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void dbscan_init_kernel(int M, const int32_t* __restrict__ perm, const int32_t* __restrict__ cnt_sorted,
                                                             int32_t* __restrict__ cnt, int32_t* __restrict__ parent,
                                                             int32_t* __restrict__ first, int32_t* __restrict__ sizes) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= M) return;
    const int i = perm[s];
    cnt[i] = cnt_sorted[s];
    parent[i] = i;
    if (first) first[s] = 0;
    if (sizes) sizes[s] = 0;
}

// ---- D3 ---------------------------------------------------------------------------------------------------------------
// A workgroup without a live row leaves before the walk; the vote is the workgroup's, so nobody misses a barrier.  Clusters are
// numbered in ascending order of their roots, so the smallest root is the smallest cluster number.
__global__ __launch_bounds__(kBlock) void dbscan_border_kernel(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                               const float* __restrict__ tbox, int n_tiles, int cull, float r2,
                                                               const int32_t* __restrict__ cnt_sorted, int minpts, int32_t* parent,
                                                               unsigned long long* __restrict__ stats) {
    __shared__ WalkLds lds;
    const int ta = blockIdx.x / kWalkWgPerTile, part = blockIdx.x % kWalkWgPerTile;
    walk_count_search(stats, (unsigned long long)n_tiles * (unsigned long long)n_tiles);
    float abox[6];
    walk_tile_box(tbox, ta, abox);
    const WalkSelfRow q = walk_self_row(ms, perm, M, ta, part);
    const bool live = q.live && cnt_sorted[q.sr] < minpts;
    if (!__syncthreads_or(live ? 1 : 0)) return;
    const float rr = live ? r2 : -1.0f;
    int best = INT_MAX;
    walk_tiles(
        lds, 0, n_tiles, q.qx, q.qy, q.qz, part == 0 ? stats : nullptr,
        [&](int ct) { return walk_visits(tbox, ct, abox, r2, cull); },
        [&](int r) { return walk_row_core(ms, perm, M, cnt_sorted, minpts, r); },
        [](int) {},
        [&](int, const float4 (&p)[4], float (&d)[4]) {
            if (fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= rr) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d[u] <= rr) best = min(best, parent[__float_as_int(p[u].w)]);
                }
            }
        },
        [] {});
    best = min(best, __shfl_xor(best, 1));
    best = min(best, __shfl_xor(best, 2));
    if (live && best != INT_MAX && (threadIdx.x & (kWalkLanes - 1)) == 0) parent[q.row_i] = best;
}

}  // namespace

void enqueue_dbscan_count(const ModelView& v, float r2, int cull, int32_t* cnt_sorted, int32_t* cnt, int32_t* parent, int32_t* first,
                          int32_t* sizes, hipStream_t st) {
    const int M = v.M, n_tiles = (M + kT16 - 1) / kT16;
    hipLaunchKernelGGL(dbscan_count_kernel, dim3((unsigned)(n_tiles * kWalkWgPerTile)), dim3(kBlock), 0, st, (const float*)v.ms,
                       (const int32_t*)v.perm, M, (const float*)v.tbox, n_tiles, cull, r2, cnt_sorted, knn_stats_dev());
    hipLaunchKernelGGL(dbscan_init_kernel, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, M, (const int32_t*)v.perm,
                       (const int32_t*)cnt_sorted, cnt, parent, first, sizes);
}

void enqueue_dbscan_border(const ModelView& v, float r2, int cull, const int32_t* cnt_sorted, int minpts, int32_t* parent, hipStream_t st) {
    const int M = v.M, n_tiles = (M + kT16 - 1) / kT16;
    hipLaunchKernelGGL(dbscan_border_kernel, dim3((unsigned)(n_tiles * kWalkWgPerTile)), dim3(kBlock), 0, st, (const float*)v.ms,
                       (const int32_t*)v.perm, M, (const float*)v.tbox, n_tiles, cull, r2, cnt_sorted, minpts, parent, knn_stats_dev());
}

}  // namespace pcreg
