// pcreg_amd/csrc/knn_k.hip -- the k nearest model points per query (1 <= k <= PCREG_KNN_MAX_K) against a PREPARED model.
//
// Contract: for every query the k model rows with the smallest d = fmaf(dz,dz, fmaf(dy,dy, dx*dx)), dx = q - m in fp32 (the
// top-2 search's formula), ordered by (distance, original row); slots past M hold (-1, +inf).  Exact by construction: every
// distance is the fp32 chain itself, so there is no certificate and no tail.
//
// The prepared model (knn_fast.hip) is used as it is: the sorted fp32 copy, perm, the tile boxes and the ordering grid's
// cell ends.  A search is a memset and four launches:
//   K1  memset + knn_k_seed_kernel   one wave per query: the k-th smallest distance dk_k over a window of 64 consecutive
//                                    sorted rows around the query's own ordering cell (k distinct real rows lie within it:
//                                    an upper bound of the true k-th distance); counts the queries per parent cell
//   K2  launch_query_order           scan + query_order_kernel (knn_fast.hip): query slots in spatial order
//   K3  knn_k_kernel<KB>             blocks of 512 query slots; each of a block's 8 workgroups forms the block's box and
//                                    largest dk_k, skips the tiles DESIGN 4.1's rule rules out, and walks the others for its
//                                    64 queries: four lanes per query, each with a sorted list of KB >= k (distance, row)
//                                    pairs in registers, merged by two shuffle rounds at the end
// The merge of per-shard lists (pcreg_dev_merge_topk_f32) is knn_k_merge_kernel<KB>.
#include "common.hpp"
#include "knn_fast_common.hpp"
#include "knn_walk.hpp"
#include "knn_klist.hpp"
#include <cmath>

namespace pcreg {

namespace {

constexpr int kKnnMaxK = PCREG_KNN_MAX_K;
constexpr int kKSeedWin = 64;                        // sorted rows the seed bound looks at (one per lane of a wave)
static_assert(kKnnMaxK <= kKSeedWin, "the seed window holds at least k rows");

// ---- K1. seed bound: one wave per query ----------------------------------------------------------------------------
// After model_order_scatter_kernel's atomics sort_cnt[c] is the END row of ordering cell c (and the start of c + 1).  The
// window: 64 consecutive sorted rows centred on the query's own cell, clamped into [0, M).  Its k-th smallest distance
// (bitonic sort across the wave) bounds the true k-th distance from above; fewer than k rows leave +inf (culling off).
// A NaN distance (non-finite input) counts as +inf, so the bound never shrinks below a real row's distance.
__global__ __launch_bounds__(kBlock) void knn_k_seed_kernel(const float* __restrict__ q, int Q, int ldq, const float* __restrict__ ms, int M,
                                                            const int32_t* __restrict__ sort_cnt, const Prep* __restrict__ prep, int k,
                                                            float* __restrict__ dk, int32_t* __restrict__ qcnt) {
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (qi >= Q) return;                                        // (wave-uniform)
    const float qx = q[qi], qy = q[qi + (size_t)ldq], qz = q[qi + 2 * (size_t)ldq];
    const int key = sort_key(qx, qy, qz, prep);
    if (lane == 0) atomicAdd(&qcnt[key >> 3], 1);               // the query order's counts (parent cells)
    const int end = sort_cnt[key], start = key > 0 ? sort_cnt[key - 1] : 0;
    int w0 = start + (end - start) / 2 - kKSeedWin / 2;
    w0 = min(w0, M - kKSeedWin); w0 = max(w0, 0);
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
    if (lane == 0) dk[qi] = v;
}

// ---- K3. the candidate walk ----------------------------------------------------------------------------------------
// Workgroup (block qb, part p) owns slots qb * 512 + p * 64 + (tid >> 2); lane sub = tid & 3 of a query scores rows sub,
// sub + 4, .. of every visited tile from LDS (x, y, z, original row) and keeps the KB best (distance, row) pairs it saw.  A
// row enters a list only when d <= thr, thr = min(dk_k, the k-th entry of any of the query's four lists), each of which bounds
// the true k-th distance from above; a row farther than that is neither among the k nearest nor tied with the k-th.
// Tiles are skipped by DESIGN 4.1's rule with D = max dk_k over the block's queries (any +inf turns it off).  The walk itself
// is knn_walk.hpp's.
template <int KB>
__global__ __launch_bounds__(kBlock) void knn_k_kernel(const float* __restrict__ q, int Q, int ldq, const int32_t* __restrict__ qperm,
                                                       const float* __restrict__ dk, const float* __restrict__ ms,
                                                       const int32_t* __restrict__ perm, int M, const float* __restrict__ tbox, int n_tiles,
                                                       int cull, int k, int idx_base, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                       unsigned long long* __restrict__ stats) {
    __shared__ WalkLds lds;
    __shared__ float s_red[kBlock / 64][7];
    __shared__ float s_box[7];
    const int tid = threadIdx.x;
    const int qb = blockIdx.x / kWalkWgPerBlock, part = blockIdx.x % kWalkWgPerBlock;
    walk_block_box<7>(s_red, s_box, q, Q, ldq, qperm, dk, qb);    // the block's box and largest dk_k
    walk_count_search(stats, (unsigned long long)((Q + kWalkQBlock - 1) / kWalkQBlock) * (unsigned long long)n_tiles);
    // this thread's query
    const int sub = tid & (kWalkLanes - 1);
    const int slot = qb * kWalkQBlock + part * kWalkQPerWg + (tid / kWalkLanes);
    const bool live = slot < Q;
    const int qi = live ? qperm[slot] : 0;
    const float qx = q[qi], qy = q[qi + (size_t)ldq], qz = q[qi + 2 * (size_t)ldq];
    float thr = live ? dk[qi] : -INFINITY;                        // (a dead lane admits nothing)
    if (!(thr == thr)) thr = INFINITY;
    float ld[KB]; int li[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) { ld[s] = INFINITY; li[s] = -1; }
    walk_tiles(
        lds, 0, n_tiles, qx, qy, qz, part == 0 ? stats : nullptr,
        [&](int ct) {
            const float Db = s_box[6];
            return !(cull != 0 && Db < INFINITY && cull_skips(cull_gap2(tbox + (size_t)ct * 6, tbox + (size_t)ct * 6 + 3, s_box, s_box + 3), Db));
        },
        [&](int r) { return walk_row(ms, perm, M, r); },
        [](int) {},
        [&](int, const float4 (&p)[4], float (&d)[4]) {
            if (fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= thr) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d[u] <= thr) {
                        klist_insert<KB>(ld, li, d[u], __float_as_int(p[u].w));
                        thr = fminf(thr, klist_kth<KB>(ld, k));
                    }
                }
            }
        },
        [&] {
            thr = fminf(thr, __shfl_xor(thr, 1));                 // the query's four lanes share the tightest bound
            thr = fminf(thr, __shfl_xor(thr, 2));
        });
    klist_merge_xor<KB>(ld, li, 1);
    klist_merge_xor<KB>(ld, li, 2);
    if (live && sub == 0) {
#pragma unroll
        for (int s = 0; s < KB; ++s) {
            if (s < k) {
                idx[(size_t)qi * k + s] = li[s] >= 0 ? li[s] + idx_base : -1;
                dist[(size_t)qi * k + s] = ld[s];
            }
        }
    }
}

// an empty model: every slot (-1, +inf)
__global__ void knn_k_fill_empty_kernel(size_t n, int32_t* __restrict__ idx, float* __restrict__ dist) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { idx[i] = -1; dist[i] = INFINITY; }
}

// R lists of k per query, list r at r * stride elements: one thread per query inserts every entry by (distance, index);
// -1 entries are empty, a repeated index is kept once (as pcreg_dev_merge_top2_f32 does)
template <int KB>
__global__ __launch_bounds__(256) void knn_k_merge_kernel(const int32_t* __restrict__ idx_in, const float* __restrict__ dist_in, int R, int Q,
                                                          int k, size_t stride, int32_t* __restrict__ idx, float* __restrict__ dist) {
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= Q) return;
    float ld[KB]; int li[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) { ld[s] = INFINITY; li[s] = -1; }
    for (int r = 0; r < R; ++r) {
        const size_t o = (size_t)r * stride + (size_t)qi * k;
        for (int e = 0; e < k; ++e) {
            const int j = idx_in[o + e];
            const float d = dist_in[o + e];
            if (j < 0) continue;
            bool dup = false;
#pragma unroll
            for (int s = 0; s < KB; ++s) dup |= li[s] == j;
            if (!dup) klist_insert<KB>(ld, li, d, j);
        }
    }
#pragma unroll
    for (int s = 0; s < KB; ++s) {
        if (s < k) { idx[(size_t)qi * k + s] = li[s]; dist[(size_t)qi * k + s] = li[s] >= 0 ? ld[s] : INFINITY; }
    }
}

struct KnnKWs { int32_t* qcnt; int32_t* qperm; float* dk; };
KnnKWs knn_k_ws_layout(int Q, void* base, size_t* bytes) {
    KnnKWs s{};
    const size_t qq = (size_t)(Q > 0 ? Q : 1);
    WsWalk w(base);
    s.qcnt = (int32_t*)w.take_bytes((size_t)kQueryKeys * 4);
    s.qperm = w.take<int32_t>(qq);
    s.dk = w.take<float>(qq);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t knn_k_ws_bytes(int Q, int M, int k) {
    (void)M; (void)k;                              // the lists live in registers: O(Q) words, whatever k and M
    size_t b; (void)knn_k_ws_layout(Q, nullptr, &b);
    return b;
}

int launch_model_knn(const ModelView& v, const float* q, int Q, int ldq, int k, int32_t idx_base, int32_t* idx, float* dist,
                     void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(k >= 1 && k <= kKnnMaxK && Q >= 0 && ldq >= Q && Q <= kMaxQTiles * 1024);
    if (Q == 0) return PCREG_OK;
    size_t need;
    const KnnKWs s = knn_k_ws_layout(Q, ws, &need);
    if (ws_bytes < need) { set_error("knn workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_WORKSPACE; }
    if (v.M == 0) {
        hipLaunchKernelGGL(knn_k_fill_empty_kernel, dim3(256), dim3(256), 0, st, (size_t)Q * k, idx, dist);
        PCREG_HIP(hipGetLastError());
        return PCREG_OK;
    }
    PCREG_HIP(hipMemsetAsync(s.qcnt, 0, (size_t)kQueryKeys * 4, st));
    hipLaunchKernelGGL(knn_k_seed_kernel, dim3((Q + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, st, q, Q, ldq, (const float*)v.ms, v.M,
                       (const int32_t*)v.sort_cnt, (const Prep*)v.prep, k, s.dk, s.qcnt);
    int rc = launch_query_order(v, q, Q, ldq, s.qcnt, s.qperm, st);
    if (rc) return rc;
    const int n_tiles = (v.M + kT16 - 1) / kT16;
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;          // "knn_nocull": visit every tile, same bits
    unsigned long long* stats = knn_stats_dev();                  // "knn_stats": searches, visited, nominal (no tail here)
    const dim3 grid((unsigned)(((Q + kWalkQBlock - 1) / kWalkQBlock) * kWalkWgPerBlock));
    klist_dispatch<1>(k, [&](auto kb) {
        hipLaunchKernelGGL(knn_k_kernel<kb.value>, grid, dim3(kBlock), 0, st, q, Q, ldq, (const int32_t*)s.qperm, (const float*)s.dk,
                           (const float*)v.ms, (const int32_t*)v.perm, v.M, (const float*)v.tbox, n_tiles, cull, k, (int)idx_base, idx, dist, stats);
    });
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

int launch_merge_topk_f32(const int32_t* idx_in, const float* dist_in, int R, int Q, int k, size_t rank_stride, int32_t* idx, float* dist,
                          hipStream_t st) {
    PCREG_ARG(k >= 1 && k <= kKnnMaxK && R >= 1 && Q >= 0 && (rank_stride == 0 || rank_stride >= (size_t)Q * k));
    if (Q == 0) return PCREG_OK;
    const size_t stride = rank_stride ? rank_stride : (size_t)Q * k;
    const dim3 grid((unsigned)((Q + 255) / 256));
    klist_dispatch<1>(k, [&](auto kb) {
        hipLaunchKernelGGL(knn_k_merge_kernel<kb.value>, grid, dim3(256), 0, st, idx_in, dist_in, R, Q, k, stride, idx, dist);
    });
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
