// pcreg_amd/csrc/knn_cluster.hip -- clusterPoints against a PREPARED model: the connected components of the graph in which
// rows i != j are adjacent iff d = fmaf(dz,dz, fmaf(dy,dy, dx*dx)) <= r2, dx = m_i - m_j in fp32 (the point search's formula;
// inclusive; a NaN distance never passes; +inf passes r2 = +inf).  A row with a non-finite coordinate has no neighbour.
// Clusters are numbered in ascending order of their smallest row.  Exact and deterministic by construction.
//
// The prepared model (knn_fast.hip) is used as it is: the sorted copy, perm, the tile boxes.
//   C1  cluster_init_kernel     parent[i] = i (original-row space), the outputs' tails cleared
//   C2  cluster_walk_kernel     self-join: tile a's rows against every tile b >= a that DESIGN 4.1's rule (D = r2, the box of
//                               tile a) does not rule out; four lanes per row; on the diagonal only j > i.  A hit unites the
//                               two ORIGINAL rows in a lock-free union-find: the larger root is hooked under the smaller by a
//                               compare-and-swap, find jumps pointers on its way.  No workgroup waits for another
//   C3  cluster_flatten_kernel  parent[i] = root of i (its cluster's smallest row); the roots per chunk of 2048 rows
//   C4  cluster_number_kernel   the chunk scan's second launch (chunk_scan.hpp): the cluster number of every root, first[],
//                               n_clusters
//   C5  cluster_label_kernel    label[i] = number[parent[i]]; sizes[] by integer atomicAdd, one per (wave, cluster)
//
// DBSCAN of the prepared model runs on the same union-find: with the neighbour count of every row (knn_dbscan.hip)
// the walk stages and keeps live the CORE rows only (cluster_walk_kernel<true>), flatten and number take a root for a cluster
// only if it is core, a border row is hooked under its smallest core neighbour's root after the flatten (knn_dbscan.hip), and
// dbscan_label_kernel leaves the rest at -1.
#include "common.hpp"
#include "knn_fast_common.hpp"
#include "knn_walk.hpp"
#include "chunk_scan.hpp"
#include <cmath>

namespace pcreg {

namespace {

#define PCREG_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- the union-find over parent[] (original rows).  Invariant: parent[x] <= x, so the forest is acyclic and a set's root is
// its smallest row.  Inside the walk every access is a relaxed agent-scope atomic; a stale value is still an ancestor.
__device__ __forceinline__ int uf_load(int32_t* parent, int x) { return __hip_atomic_load(parent + x, PCREG_RLX_AGENT); }
// the root of x; every node passed on the way is pointed at its grandparent (only ever an ancestor, only into non-root slots)
__device__ __forceinline__ int uf_find(int32_t* parent, int x) {
    int cur = uf_load(parent, x);
    if (cur != x) {
        int prev = x, next;
        while (cur > (next = uf_load(parent, cur))) {
            __hip_atomic_store(parent + prev, next, PCREG_RLX_AGENT);
            prev = cur;
            cur = next;
        }
    }
    return cur;
}
// Merges the sets of a and b; returns their common root as of the merge.  A compare-and-swap succeeds only on a slot that is a
// root at that instant; a failure means another lane hooked that root first, and the loop goes on from the value it wrote: the
// number of iterations is bounded by the number of merges in the launch.  Nothing spins on anybody's progress.
__device__ __forceinline__ int uf_unite(int32_t* parent, int a, int b, unsigned long long* stats) {
    int ra = uf_find(parent, a), rb = uf_find(parent, b);
    while (ra != rb) {
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int expected = hi;
        const bool ok = __hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT);
        if (stats) { atomicAdd(&stats[2], 1ull); if (!ok) atomicAdd(&stats[3], 1ull); }
        if (ok) return lo;
        ra = uf_find(parent, expected);                            // hi had been hooked under `expected` (< hi)
        rb = lo;
    }
    return ra;
}

// ---- C1 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cluster_init_kernel(int M, int32_t* __restrict__ parent, int32_t* __restrict__ first,
                                                              int32_t* __restrict__ sizes) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    parent[i] = i;
    if (first) first[i] = 0;
    if (sizes) sizes[i] = 0;
}

// ---- C2. the walk -----------------------------------------------------------------------------------------------------
// Workgroup (tile a, part p) owns sorted rows a * 512 + p * 64 + (tid >> 2); lane sub = tid & 3 of a row scores rows sub,
// sub + 4, .. of every visited tile b >= a from LDS (x, y, z, original row).  Pair (a, b) is skipped by DESIGN 4.1's rule with
// D = r2 and B = tile a's box: every row pair of a skipped tile pair has a computed d > r2.  The walk itself is knn_walk.hpp's,
// and so are the row prologue (walk_self_row), the staging rule (walk_row_finite) and the visit rule (walk_visits).
// A non-finite row is staged as NaN and its own lanes admit nothing, so it stays a set of its own whatever r2.
// kCoreOnly (DBSCAN's core walk): the same holds for every row with cnt[sorted row] < minpts, and a workgroup none of whose 64
// rows is core leaves before the walk (the vote is the workgroup's, so nobody misses a barrier).
template <bool kCoreOnly>
__global__ __launch_bounds__(kBlock) void cluster_walk_kernel(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                              const float* __restrict__ tbox, int n_tiles, int cull, int skip_same, float r2,
                                                              const int32_t* __restrict__ cnt, int minpts, int32_t* parent,
                                                              unsigned long long* __restrict__ stats,
                                                              unsigned long long* __restrict__ cstats) {
    __shared__ WalkLds lds;
    const int ta = blockIdx.x / kWalkWgPerTile, part = blockIdx.x % kWalkWgPerTile;
    walk_count_search(stats, (unsigned long long)n_tiles * (unsigned long long)(n_tiles + 1) / 2ull);
    if (cstats && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&cstats[0], 1ull);
    float abox[6];
    walk_tile_box(tbox, ta, abox);
    const WalkSelfRow q = walk_self_row(ms, perm, M, ta, part);
    bool live = q.live;
    if constexpr (kCoreOnly) {
        live = live && cnt[q.sr] >= minpts;
        if (!__syncthreads_or(live ? 1 : 0)) return;
    }
    const float rr = live ? r2 : -1.0f;                           // (a dead lane admits nothing: d is never negative)
    int my_root = q.row_i;                                        // the last root this lane saw for its row
    unsigned long long n_hit = 0;
    int above = -1;                                               // on the diagonal only the rows behind this one
    walk_tiles(
        lds, ta, n_tiles, q.qx, q.qy, q.qz, part == 0 ? stats : nullptr,
        [&](int ct) { return walk_visits(tbox, ct, abox, r2, cull); },
        [&](int r) {
            if constexpr (kCoreOnly) return walk_row_core(ms, perm, M, cnt, minpts, r);
            else return walk_row_finite(ms, perm, M, r);
        },
        [&](int ct) { above = ct == ta ? q.rl : -1; },
        [&](int r, const float4 (&p)[4], float (&d)[4]) {
            const float qnan = __int_as_float(0x7FC00000);
#pragma unroll
            for (int u = 0; u < 4; ++u) d[u] = r + u * kWalkLanes > above ? d[u] : qnan;
            if (fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= rr) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d[u] <= rr) {
                        const int row_j = __float_as_int(p[u].w);
                        ++n_hit;
                        // one load: a row that already points at this lane's root is in its set (sets only merge)
                        if (skip_same && uf_load(parent, row_j) == my_root) continue;
                        my_root = uf_unite(parent, my_root, row_j, cstats);
                    }
                }
            }
        },
        [] {});
    if (cstats && n_hit) atomicAdd(&cstats[1], n_hit);
}

// ---- C3. flatten: parent[i] = the root of i; the number of roots per chunk ----------------------------------------------
// (the walk is a finished launch: its parent[] is visible.  A thread's store only replaces an ancestor of i by the root, so
// the threads that pass through i in the same launch still reach the same root.)
// cnt (by ORIGINAL row) and minpts are DBSCAN's: only a core root stands for a cluster.  clusterPoints passes no cnt: every row is core.
__device__ __forceinline__ bool row_is_core(const int32_t* __restrict__ cnt, int minpts, int i) { return !cnt || cnt[i] >= minpts; }
__global__ __launch_bounds__(kBlock) void cluster_flatten_kernel(int M, int32_t* parent, const int32_t* __restrict__ cnt, int minpts,
                                                                 int32_t* __restrict__ csum) {
    const int base = blockIdx.x * kScanChunk;
    int32_t v = 0;
    for (int k = threadIdx.x; k < kScanChunk; k += kBlock) {
        const int i = base + k;
        if (i < M) {
            int r = uf_load(parent, i);
            while (true) { const int n = uf_load(parent, r); if (n == r) break; r = n; }
            __hip_atomic_store(parent + i, r, PCREG_RLX_AGENT);
            v += r == i && row_is_core(cnt, minpts, i) ? 1 : 0;
        }
    }
    chunk_sum(v, csum);
}

// ---- C4. number the roots in row order --------------------------------------------------------------------------------
// the two-launch chunk scan (chunk_scan.hpp) over the rows' "is a root": num[i] (roots only) = the roots before row i; the last
// chunk writes n_clusters
__global__ __launch_bounds__(kBlock) void cluster_number_kernel(int M, const int32_t* __restrict__ parent, const int32_t* __restrict__ cnt,
                                                                int minpts, const int32_t* __restrict__ csum, int32_t* __restrict__ num,
                                                                int32_t* __restrict__ first, int32_t* __restrict__ n_clusters) {
    const int i0 = blockIdx.x * kScanChunk + threadIdx.x * kScanPer;
    int32_t f[kScanPer], mine = 0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) { f[u] = i0 + u < M && parent[i0 + u] == i0 + u && row_is_core(cnt, minpts, i0 + u) ? 1 : 0; mine += f[u]; }
    int32_t run = chunk_offset(csum, mine);
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        if (f[u]) { num[i0 + u] = run; if (first) first[run] = i0 + u; }
        run += f[u];
        if (i0 + u == M - 1) *n_clusters = run;
    }
}

// ---- C5 ---------------------------------------------------------------------------------------------------------------
// sizes: one atomicAdd per (wave, cluster) -- the lanes of a wave that share a cluster are counted by their leader.  Rows that
// follow each other mostly share a cluster when clusters are large (a million single adds to ONE word took 11 ms), and when
// they do not, the adds go to different words anyway.
__device__ __forceinline__ void wave_count_sizes(bool live, int c, int32_t* __restrict__ sizes) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __builtin_amdgcn_ballot_w64(live);
    while (todo) {                                                // (wave-uniform: every lane sees the same todo)
        const int lead = __ffsll((long long)todo) - 1;
        const int cl = __shfl(c, lead);
        const unsigned long long same = __builtin_amdgcn_ballot_w64(live && c == cl);
        if (lane == lead) atomicAdd(&sizes[cl], (int)__popcll(same));
        todo &= ~same;
    }
}
__global__ __launch_bounds__(kBlock) void cluster_label_kernel(int M, const int32_t* __restrict__ parent, const int32_t* __restrict__ num,
                                                               int32_t* __restrict__ label, int32_t* __restrict__ sizes) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < M;
    int c = -1;
    if (live) { c = num[parent[i]]; label[i] = c; }
    if (sizes) wave_count_sizes(live, c, sizes);
}
// DBSCAN's: a core row carries its root's number; a non-core row that the border walk hooked under a root (parent[i] != i)
// carries that root's; every other row is noise, -1, and counted in no cluster.  core / count (either may be null) are the
// caller's copies of what the count walk found.
__global__ __launch_bounds__(kBlock) void dbscan_label_kernel(int M, const int32_t* __restrict__ parent, const int32_t* __restrict__ num,
                                                              const int32_t* __restrict__ cnt, int minpts, int32_t* __restrict__ label,
                                                              uint8_t* __restrict__ core, int32_t* __restrict__ count,
                                                              int32_t* __restrict__ sizes) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int c = -1;
    if (i < M) {
        const int n = cnt[i], p = parent[i];
        const bool is_core = n >= minpts;
        if (is_core || p != i) c = num[p];
        label[i] = c;
        if (core) core[i] = is_core ? 1 : 0;
        if (count) count[i] = n;
    }
    if (sizes) wave_count_sizes(c >= 0, c, sizes);
}

// Workspace: [parent, M] [cluster number of every root, M] [roots per chunk of 2048 rows]:
// 2 * roundup(4 * max(M, 1), 256) + roundup(4 * max(ceil(M / 2048), 1), 256) bytes, whatever r2 and the result
struct ClusterWs { int32_t* parent; int32_t* num; int32_t* csum; };
ClusterWs cluster_ws_layout(int M, void* base, size_t* bytes) {
    ClusterWs s{};
    const size_t mm = (size_t)(M > 0 ? M : 1);
    WsWalk w(base);
    s.parent = w.take<int32_t>(mm);
    s.num = w.take<int32_t>(mm);
    s.csum = w.take<int32_t>((mm + kScanChunk - 1) / kScanChunk);
    *bytes = w.bytes();
    return s;
}
// DBSCAN's: [parent, M] [cluster number of every core root, M] [neighbour count by sorted row, M] [... by original row, M]
// [core roots per chunk of 2048 rows]:
// 4 * roundup(4 * max(M, 1), 256) + roundup(4 * max(ceil(M / 2048), 1), 256) bytes, whatever r2, minpts and the result
struct DbscanWs { int32_t* parent; int32_t* num; int32_t* cnt_sorted; int32_t* cnt; int32_t* csum; };
DbscanWs dbscan_ws_layout(int M, void* base, size_t* bytes) {
    DbscanWs s{};
    const size_t mm = (size_t)(M > 0 ? M : 1);
    WsWalk w(base);
    s.parent = w.take<int32_t>(mm);
    s.num = w.take<int32_t>(mm);
    s.cnt_sorted = w.take<int32_t>(mm);
    s.cnt = w.take<int32_t>(mm);
    s.csum = w.take<int32_t>((mm + kScanChunk - 1) / kScanChunk);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t cluster_ws_bytes(int M) {
    size_t b; (void)cluster_ws_layout(M, nullptr, &b);
    return b;
}

int launch_model_cluster(const ModelView& v, float r2, int32_t* label, int32_t* n_clusters, int32_t* first, int32_t* sizes, void* ws,
                         size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(r2 >= 0.0f && n_clusters && (label || v.M == 0));
    size_t need;
    const ClusterWs s = cluster_ws_layout(v.M, ws, &need);
    if (ws_bytes < need) { set_error("cluster workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_WORKSPACE; }
    const int M = v.M;
    if (M == 0) {                                                 // no cluster
        PCREG_HIP(hipMemsetAsync(n_clusters, 0, sizeof(int32_t), st));
        return PCREG_OK;
    }
    const int n_tiles = (M + kT16 - 1) / kT16, chunks = (M + kScanChunk - 1) / kScanChunk, blocks = (M + kBlock - 1) / kBlock;
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;          // "knn_nocull": visit every tile pair, same bits
    const int skip_same = debug_flag(kDbgClusterNoSkip) ? 0 : 1; // "cluster_noskip": unite on every hit, same bits
    hipLaunchKernelGGL(cluster_init_kernel, dim3(blocks), dim3(kBlock), 0, st, M, s.parent, first, sizes);
    hipLaunchKernelGGL(cluster_walk_kernel<false>, dim3((unsigned)(n_tiles * kWalkWgPerTile)), dim3(kBlock), 0, st, (const float*)v.ms,
                       (const int32_t*)v.perm, M, (const float*)v.tbox, n_tiles, cull, skip_same, r2, (const int32_t*)nullptr, 1, s.parent,
                       knn_stats_dev(), cluster_stats_dev());
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3(chunks), dim3(kBlock), 0, st, M, s.parent, (const int32_t*)nullptr, 1, s.csum);
    hipLaunchKernelGGL(cluster_number_kernel, dim3(chunks), dim3(kBlock), 0, st, M, (const int32_t*)s.parent, (const int32_t*)nullptr, 1,
                       (const int32_t*)s.csum, s.num, first, n_clusters);
    hipLaunchKernelGGL(cluster_label_kernel, dim3(blocks), dim3(kBlock), 0, st, M, (const int32_t*)s.parent, (const int32_t*)s.num, label,
                       sizes);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

size_t dbscan_ws_bytes(int M) {
    size_t b; (void)dbscan_ws_layout(M, nullptr, &b);
    return b;
}

int launch_model_dbscan(const ModelView& v, float r2, int minpts, int32_t* label, int32_t* n_clusters, uint8_t* core, int32_t* count,
                        int32_t* first, int32_t* sizes, void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(r2 >= 0.0f && minpts >= 1 && n_clusters && (label || v.M == 0));
    size_t need;
    const DbscanWs s = dbscan_ws_layout(v.M, ws, &need);
    if (ws_bytes < need) { set_error("dbscan workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_WORKSPACE; }
    const int M = v.M;
    if (M == 0) {                                                 // no cluster
        PCREG_HIP(hipMemsetAsync(n_clusters, 0, sizeof(int32_t), st));
        return PCREG_OK;
    }
    const int n_tiles = (M + kT16 - 1) / kT16, chunks = (M + kScanChunk - 1) / kScanChunk, blocks = (M + kBlock - 1) / kBlock;
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;          // "knn_nocull": visit every tile pair, same bits
    const int skip_same = debug_flag(kDbgClusterNoSkip) ? 0 : 1; // "cluster_noskip": unite on every hit, same bits
    enqueue_dbscan_count(v, r2, cull, s.cnt_sorted, s.cnt, s.parent, first, sizes, st);
    hipLaunchKernelGGL(cluster_walk_kernel<true>, dim3((unsigned)(n_tiles * kWalkWgPerTile)), dim3(kBlock), 0, st, (const float*)v.ms,
                       (const int32_t*)v.perm, M, (const float*)v.tbox, n_tiles, cull, skip_same, r2, (const int32_t*)s.cnt_sorted, minpts,
                       s.parent, knn_stats_dev(), cluster_stats_dev());
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3(chunks), dim3(kBlock), 0, st, M, s.parent, (const int32_t*)s.cnt, minpts, s.csum);
    hipLaunchKernelGGL(cluster_number_kernel, dim3(chunks), dim3(kBlock), 0, st, M, (const int32_t*)s.parent, (const int32_t*)s.cnt, minpts,
                       (const int32_t*)s.csum, s.num, first, n_clusters);
    enqueue_dbscan_border(v, r2, cull, s.cnt_sorted, minpts, s.parent, st);
    hipLaunchKernelGGL(dbscan_label_kernel, dim3(blocks), dim3(kBlock), 0, st, M, (const int32_t*)s.parent, (const int32_t*)s.num,
                       (const int32_t*)s.cnt, minpts, label, core, count, sizes);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
