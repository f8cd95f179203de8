// pcreg_amd/csrc/knn_range.hip -- radius queries (rangesearch) against a PREPARED model: every model row within a squared
// distance r2 of each query, a ragged result.
//
// Contract: row j belongs to query i iff d = fmaf(dz,dz, fmaf(dy,dy, dx*dx)) <= r2, dx = q - m in fp32 (the point search's
// formula; inclusive; a NaN distance never passes; +inf passes r2 = +inf).  A query's rows are ordered by (distance, original
// row).  Exact by construction: every distance is the fp32 chain itself.
//
// The prepared model (knn_fast.hip) is used as it is.  Two calls of the same shape (count, scan | fill, order), each forming its
// own query order:
//   R1  memset + range_qcell_kernel   the queries per parent cell of the ordering grid
//   R2  launch_query_order            scan + query_order_kernel (knn_fast.hip): query slots in spatial order
//   R3  range_walk_kernel<FILL>       blocks of 512 query slots; each of a block's 8 workgroups forms the block's box, skips the
//                                     tiles DESIGN 4.1's rule rules out with D = r2, and walks the others for its 64 queries: four
//                                     lanes per query.  Count: hits summed over the four lanes.  Fill: a hit takes the next
//                                     place of the query's segment (an LDS cursor), clamped into the segment and the capacity
//   R4  count: range_scan_kernel      counts -> seg_off in int64: the two-launch chunk scan (chunk_scan.hpp)
//       fill:  range_sort_wave_kernel one wave per query: segments of up to 64 rows sorted in registers, longer ones listed
//              range_sort_wg_kernel   one workgroup per listed segment: up to kRangeLdsCap rows in LDS, above that in place in
//                                     global memory (no memory proportional to the result)
#include "common.hpp"
#include "knn_fast_common.hpp"
#include "knn_walk.hpp"
#include "chunk_scan.hpp"
#include <cmath>

namespace pcreg {

namespace {

constexpr int kRangeMaxQ = kMaxQTiles * 1024;        // 4 Mi queries per call
constexpr int kScanMaxChunks = kRangeMaxQ / kScanChunk;
constexpr int kRangeLdsCap = 2048;                   // longest segment sorted in LDS (16 KiB of 64-bit keys)
constexpr int kSortWgGrid = 2048;                    // workgroups of range_sort_wg_kernel (they loop over the list)
static_assert(kScanMaxChunks <= kScanChunk, "one workgroup sums every chunk before its own");

// the part of [seg_off[qi], seg_off[qi + 1]) inside [0, capacity), whatever seg_off holds: 0 <= b <= e <= capacity
__device__ __forceinline__ void range_segment(const int64_t* __restrict__ seg_off, int qi, int64_t capacity, int64_t& b, int64_t& e) {
    const int64_t s0 = seg_off[qi], s1 = seg_off[qi + 1];
    b = s0 < 0 ? 0 : (s0 > capacity ? capacity : s0);
    e = s1 < b ? b : (s1 > capacity ? capacity : s1);
}

// ---- R1. the query order's counts -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void range_qcell_kernel(const float* __restrict__ q, int Q, int ldq, const Prep* __restrict__ prep,
                                                             int32_t* __restrict__ qcnt) {
    const int qi = blockIdx.x * kBlock + threadIdx.x;
    if (qi >= Q) return;
    atomicAdd(&qcnt[sort_key(q[qi], q[qi + (size_t)ldq], q[qi + 2 * (size_t)ldq], prep) >> 3], 1);
}

// ---- R3. the walk -----------------------------------------------------------------------------------------------------
// Workgroup (block qb, part p) owns slots qb * 512 + p * 64 + (tid >> 2); lane sub = tid & 3 of a query scores rows sub,
// sub + 4, .. of every visited tile from LDS (x, y, z, original row).  A tile is skipped by DESIGN 4.1's rule with D = r2 and
// the block's box: every row of a skipped tile has a computed d > r2 for every query of the block.  The walk itself is
// knn_walk.hpp's.
// FILL: found[qi] is the number of rows the query HAS (not the number kept); the rows land at seg begin + 0, 1, .. in the order
// the lanes arrive, and only inside the clamped segment.
template <bool FILL>
__global__ __launch_bounds__(kBlock) void range_walk_kernel(const float* __restrict__ q, int Q, int ldq, const int32_t* __restrict__ qperm,
                                                            const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                            const float* __restrict__ tbox, int n_tiles, int cull, float r2,
                                                            int32_t* __restrict__ counts, const int64_t* __restrict__ seg_off,
                                                            int64_t capacity, int idx_base, int32_t* __restrict__ idx,
                                                            float* __restrict__ dist, int32_t* __restrict__ found,
                                                            unsigned long long* __restrict__ stats) {
    __shared__ WalkLds lds;
    __shared__ float s_red[kBlock / 64][6];
    __shared__ float s_box[6];
    __shared__ int s_cur[kWalkQPerWg];
    const int tid = threadIdx.x;
    const int qb = blockIdx.x / kWalkWgPerBlock, part = blockIdx.x % kWalkWgPerBlock;
    if (tid < kWalkQPerWg) s_cur[tid] = 0;
    walk_block_box<6>(s_red, s_box, q, Q, ldq, qperm, nullptr, qb);
    walk_count_search(stats, (unsigned long long)((Q + kWalkQBlock - 1) / kWalkQBlock) * (unsigned long long)n_tiles);
    // this thread's query
    const int sub = tid & (kWalkLanes - 1), ql = tid / kWalkLanes;
    const int slot = qb * kWalkQBlock + part * kWalkQPerWg + ql;
    const bool live = slot < Q;
    const int qi = live ? qperm[slot] : 0;
    const float qx = q[qi], qy = q[qi + (size_t)ldq], qz = q[qi + 2 * (size_t)ldq];
    const float rr = live ? r2 : -1.0f;                           // (a dead lane admits nothing: d is never negative)
    int64_t seg_b = 0, seg_e = 0;
    if (FILL && live) range_segment(seg_off, qi, capacity, seg_b, seg_e);
    int cnt = 0;
    walk_tiles(
        lds, 0, n_tiles, qx, qy, qz, part == 0 ? stats : nullptr,
        [&](int ct) {
            return !(cull != 0 && r2 < INFINITY && cull_skips(cull_gap2(tbox + (size_t)ct * 6, tbox + (size_t)ct * 6 + 3, s_box, s_box + 3), r2));
        },
        [&](int r) { return walk_row(ms, perm, M, r); },
        [](int) {},
        [&](int, const float4 (&p)[4], float (&d)[4]) {
            if (!FILL) {
#pragma unroll
                for (int u = 0; u < 4; ++u) cnt += d[u] <= rr ? 1 : 0;
            } else if (fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= rr) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d[u] <= rr) {
                        const int64_t at = seg_b + (int64_t)atomicAdd(&s_cur[ql], 1);
                        if (at < seg_e) { idx[at] = __float_as_int(p[u].w) + idx_base; dist[at] = d[u]; }
                    }
                }
            }
        },
        [] {});
    if (!FILL) {
        cnt += __shfl_xor(cnt, 1);
        cnt += __shfl_xor(cnt, 2);
        if (live && sub == 0) counts[qi] = cnt;
    } else {
        __syncthreads();
        if (live && sub == 0) found[qi] = s_cur[ql];
    }
}

// ---- R4 (count). counts -> seg_off, int64 ----------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void range_chunk_sum_kernel(const int32_t* __restrict__ counts, int Q, int64_t* __restrict__ csum) {
    const int base = blockIdx.x * kScanChunk;
    int64_t v = 0;
    for (int i = threadIdx.x; i < kScanChunk; i += kBlock) v += base + i < Q ? (int64_t)counts[base + i] : 0;
    chunk_sum(v, csum);
}
// thread t of chunk c owns 8 consecutive counts; the last chunk also writes seg_off[Q]
__global__ __launch_bounds__(kBlock) void range_scan_kernel(const int32_t* __restrict__ counts, int Q, const int64_t* __restrict__ csum,
                                                            int64_t* __restrict__ seg_off) {
    const int i0 = blockIdx.x * kScanChunk + threadIdx.x * kScanPer;
    int c[kScanPer]; int64_t mine = 0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) { c[u] = i0 + u < Q ? counts[i0 + u] : 0; mine += c[u]; }
    int64_t run = chunk_offset(csum, mine);
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        if (i0 + u < Q) seg_off[i0 + u] = run;
        run += c[u];
        if (i0 + u == Q - 1) seg_off[Q] = run;
    }
}

// ---- R4 (fill). each segment by (distance, row) ------------------------------------------------------------------------
// d is never negative, -0 or NaN inside a result, so (bits(d) << 32) | row orders by (distance, row); rows are distinct, so
// the order is total and the arrival order of the fill does not show.
__device__ __forceinline__ unsigned long long range_key(float d, int row) { return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)row; }
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
    const unsigned lo32 = (unsigned)__shfl_xor((int)(unsigned)v, o), hi32 = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
    return ((unsigned long long)hi32 << 32) | lo32;
}
// what the fill left of query qi: the first n places of its clamped segment
__device__ __forceinline__ int64_t range_filled(const int64_t* __restrict__ seg_off, const int32_t* __restrict__ found, int qi, int64_t capacity,
                                                int64_t& n) {
    int64_t b, e;
    range_segment(seg_off, qi, capacity, b, e);
    const int64_t f = found[qi];
    n = f < e - b ? f : e - b;
    return b;
}
// one wave per query: up to min(cap, 64) rows in registers (a bitonic network over the lanes), longer segments to the list
__global__ __launch_bounds__(kBlock) void range_sort_wave_kernel(int Q, const int64_t* __restrict__ seg_off, const int32_t* __restrict__ found,
                                                                 int64_t capacity, int idx_base, int cap, int32_t* idx, float* dist,
                                                                 int32_t* __restrict__ list, int32_t* __restrict__ n_list) {
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (qi >= Q) return;                                        // (wave-uniform)
    int64_t n;
    const int64_t b = range_filled(seg_off, found, qi, capacity, n);
    if (n <= 1) return;
    if (n > 64 || n > cap) {
        if (lane == 0) list[atomicAdd(n_list, 1)] = qi;
        return;
    }
    unsigned long long key = ~0ull;
    if (lane < n) key = range_key(dist[b + lane], idx[b + lane] - idx_base);
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const unsigned long long o = shfl_xor_u64(key, stride);
            const bool up = (lane & size) == 0, lower = (lane & stride) == 0;
            key = (lower == up) ? (o < key ? o : key) : (o > key ? o : key);
        }
    }
    if (lane < n) { dist[b + lane] = __uint_as_float((unsigned)(key >> 32)); idx[b + lane] = (int)(unsigned)key + idx_base; }
}
// The network of both long paths: a bitonic sorter whose comparators all point the same way (the smaller key to the lower
// place): stage k first compares place a with its mirror image inside the block of k, then half-cleaners of k/4, k/8, ...
// A place at or past n holds +inf by definition, and no comparator moves +inf down, so one that touches such a place is
// skipped: any n is sorted by the network of the next power of two.  Comparator t of a step: places (a, b), a < b.
__device__ __forceinline__ void range_net_pair(int64_t t, int64_t k, int64_t j, bool first, int64_t& a, int64_t& b) {
    if (first) { const int64_t h = k >> 1, r = t % h; a = (t / h) * k + r; b = a + (k - 1 - 2 * r); }
    else { a = (t / j) * 2 * j + (t % j); b = a + j; }
}
__global__ __launch_bounds__(kBlock) void range_sort_wg_kernel(const int64_t* __restrict__ seg_off, const int32_t* __restrict__ found,
                                                               int64_t capacity, int idx_base, int cap, int32_t* idx, float* dist,
                                                               const int32_t* __restrict__ list, const int32_t* __restrict__ n_list) {
    __shared__ unsigned long long s_key[kRangeLdsCap];
    const int tid = threadIdx.x;
    const int n_seg = *n_list;
    for (int e = blockIdx.x; e < n_seg; e += gridDim.x) {
        const int qi = list[e];
        int64_t n;
        const int64_t b = range_filled(seg_off, found, qi, capacity, n);
        int64_t P = 2;
        while (P < n) P <<= 1;
        __syncthreads();                                          // the previous segment's LDS readers are done
        if (n <= cap && n <= kRangeLdsCap) {
            for (int i = tid; i < (int)P; i += kBlock) s_key[i] = i < n ? range_key(dist[b + i], idx[b + i] - idx_base) : ~0ull;
            for (int64_t k = 2; k <= P; k <<= 1) {
                for (int64_t j = k >> 1; j > 0; j >>= 1) {
                    __syncthreads();
                    for (int64_t t = tid; t < P / 2; t += kBlock) {
                        int64_t a, c;
                        range_net_pair(t, k, j, j == k >> 1, a, c);
                        const unsigned long long x = s_key[a], y = s_key[c];
                        if (y < x) { s_key[a] = y; s_key[c] = x; }
                    }
                }
            }
            __syncthreads();
            for (int i = tid; i < (int)n; i += kBlock) { dist[b + i] = __uint_as_float((unsigned)(s_key[i] >> 32)); idx[b + i] = (int)(unsigned)s_key[i] + idx_base; }
        } else {
            // in place: the workgroup's own stores and loads of one segment, ordered by the barriers
            for (int64_t k = 2; k <= P; k <<= 1) {
                for (int64_t j = k >> 1; j > 0; j >>= 1) {
                    __syncthreads();
                    for (int64_t t = tid; t < P / 2; t += kBlock) {
                        int64_t a, c;
                        range_net_pair(t, k, j, j == k >> 1, a, c);
                        if (c >= n) continue;
                        const float da = dist[b + a], dc = dist[b + c];
                        const int ia = idx[b + a], ic = idx[b + c];
                        if (range_key(dc, ic - idx_base) < range_key(da, ia - idx_base)) { dist[b + a] = dc; idx[b + a] = ic; dist[b + c] = da; idx[b + c] = ia; }
                    }
                }
            }
        }
    }
}

// Workspace: [per-parent-cell counters | list length] [slot -> query, Q] [rows found per query, Q] [long segments, Q]
// [chunk sums of the scan]: 131 328 + 16 384 + 3 * roundup(4 * max(Q, 1), 256) bytes, whatever M, r2 and the result size
struct RangeWs { int32_t* qcnt; int32_t* n_list; int32_t* qperm; int32_t* found; int32_t* list; int64_t* csum; };
RangeWs range_ws_layout(int Q, void* base, size_t* bytes) {
    RangeWs s{};
    const size_t qq = (size_t)(Q > 0 ? Q : 1);
    WsWalk w(base);
    s.qcnt = (int32_t*)w.take_bytes((size_t)kQueryKeys * 4 + 256);
    s.n_list = s.qcnt ? s.qcnt + kQueryKeys : nullptr;
    s.qperm = w.take<int32_t>(qq);
    s.found = w.take<int32_t>(qq);
    s.list = w.take<int32_t>(qq);
    s.csum = (int64_t*)w.take_bytes((size_t)kScanMaxChunks * 8);
    *bytes = w.bytes();
    return s;
}

}  // namespace

// R1: qcnt (kQueryKeys counters and the 256 bytes behind them) cleared, then the counts
int launch_query_cells(const ModelView& v, const float* q, int Q, int ldq, int32_t* qcnt, hipStream_t st) {
    PCREG_HIP(hipMemsetAsync(qcnt, 0, (size_t)kQueryKeys * 4 + 256, st));
    hipLaunchKernelGGL(range_qcell_kernel, dim3((Q + kBlock - 1) / kBlock), dim3(kBlock), 0, st, q, Q, ldq, (const Prep*)v.prep, qcnt);
    return PCREG_OK;
}

namespace {

// R1 + R2 of either call
int range_order(const ModelView& v, const float* q, int Q, int ldq, const RangeWs& s, hipStream_t st) {
    const int rc = launch_query_cells(v, q, Q, ldq, s.qcnt, st);
    return rc ? rc : launch_query_order(v, q, Q, ldq, s.qcnt, s.qperm, st);
}

}  // namespace

size_t range_ws_bytes(int Q, int M) {
    (void)M;                                       // O(Q) words, whatever M, r2 and the number of rows returned
    size_t b; (void)range_ws_layout(Q, nullptr, &b);
    return b;
}

int launch_model_range_count(const ModelView& v, const float* q, int Q, int ldq, float r2, int32_t* counts, int64_t* seg_off, void* ws,
                             size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(Q >= 0 && ldq >= Q && Q <= kRangeMaxQ && r2 >= 0.0f);
    size_t need;
    const RangeWs s = range_ws_layout(Q, ws, &need);
    if (ws_bytes < need) { set_error("range workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_WORKSPACE; }
    if (Q == 0 || v.M == 0) {                                     // empty segments
        if (Q > 0) PCREG_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)Q, st));
        PCREG_HIP(hipMemsetAsync(seg_off, 0, sizeof(int64_t) * ((size_t)Q + 1), st));
        return PCREG_OK;
    }
    int rc = range_order(v, q, Q, ldq, s, st);
    if (rc) return rc;
    const int n_tiles = (v.M + kT16 - 1) / kT16;
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;          // "knn_nocull": visit every tile, same bits
    const dim3 grid((unsigned)(((Q + kWalkQBlock - 1) / kWalkQBlock) * kWalkWgPerBlock));
    hipLaunchKernelGGL(range_walk_kernel<false>, grid, dim3(kBlock), 0, st, q, Q, ldq, (const int32_t*)s.qperm, (const float*)v.ms,
                       (const int32_t*)v.perm, v.M, (const float*)v.tbox, n_tiles, cull, r2, counts, (const int64_t*)nullptr, (int64_t)0, 0,
                       (int32_t*)nullptr, (float*)nullptr, (int32_t*)nullptr, knn_stats_dev());
    const int chunks = (Q + kScanChunk - 1) / kScanChunk;
    hipLaunchKernelGGL(range_chunk_sum_kernel, dim3(chunks), dim3(kBlock), 0, st, (const int32_t*)counts, Q, s.csum);
    hipLaunchKernelGGL(range_scan_kernel, dim3(chunks), dim3(kBlock), 0, st, (const int32_t*)counts, Q, (const int64_t*)s.csum, seg_off);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

int launch_model_range_fill(const ModelView& v, const float* q, int Q, int ldq, float r2, int32_t idx_base, const int64_t* seg_off,
                            int64_t capacity, int32_t* idx, float* dist, void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(Q >= 0 && ldq >= Q && Q <= kRangeMaxQ && r2 >= 0.0f && capacity >= 0);
    size_t need;
    const RangeWs s = range_ws_layout(Q, ws, &need);
    if (ws_bytes < need) { set_error("range workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_WORKSPACE; }
    if (Q == 0 || v.M == 0 || capacity == 0) return PCREG_OK;     // nothing to write
    int rc = range_order(v, q, Q, ldq, s, st);
    if (rc) return rc;
    const int n_tiles = (v.M + kT16 - 1) / kT16;
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;
    const int dbg_cap = debug_flag(kDbgRangeSortCap);             // "range_sort_cap": longer segments take the in-place path
    const int cap = dbg_cap > 0 ? std::min(dbg_cap, kRangeLdsCap) : kRangeLdsCap;
    const dim3 grid((unsigned)(((Q + kWalkQBlock - 1) / kWalkQBlock) * kWalkWgPerBlock));
    hipLaunchKernelGGL(range_walk_kernel<true>, grid, dim3(kBlock), 0, st, q, Q, ldq, (const int32_t*)s.qperm, (const float*)v.ms,
                       (const int32_t*)v.perm, v.M, (const float*)v.tbox, n_tiles, cull, r2, (int32_t*)nullptr, seg_off, capacity,
                       (int)idx_base, idx, dist, s.found, knn_stats_dev());
    hipLaunchKernelGGL(range_sort_wave_kernel, dim3((Q + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, st, Q, seg_off,
                       (const int32_t*)s.found, capacity, (int)idx_base, cap, idx, dist, s.list, s.n_list);
    hipLaunchKernelGGL(range_sort_wg_kernel, dim3((unsigned)std::min(Q, kSortWgGrid)), dim3(kBlock), 0, st, seg_off, (const int32_t*)s.found,
                       capacity, (int)idx_base, cap, idx, dist, (const int32_t*)s.list, (const int32_t*)s.n_list);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
