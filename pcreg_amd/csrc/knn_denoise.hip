// pcreg_amd/csrc/knn_denoise.hip -- statistical outlier removal of a PREPARED model (MATLAB's pcdenoise): the mean distance of
// every row to its k nearest other rows, the threshold mean + t * std over the rows, and the rows at or below it, ascending.
// The contract is pcreg_model_denoise_f32's (include/pcreg.h); DESIGN 4.18.
//
// The prepared model (knn_fast.hip) is used as it is, as the normals use it (knn_normals.hip).  A call is six launches:
//   D1  normals_seed_kernel        the seed bound of every sorted row with k + 1 (the list holds the row itself)
//   D2  denoise_walk_kernel<KB>    normals_walk_kernel's walk with a list of KB >= k + 1 DISTANCES per lane and no rows; after the two
//                                  merges every lane of a row holds the row's k + 1 smallest distances ascending; the epilogue adds
//                                  their double square roots in that order and divides; lane 0 stores to the ORIGINAL row
//   D3  denoise_chunk_sum_kernel   per chunk of 2048 original rows: the finite d_i and their sum
//   D4  denoise_chunk_dev_kernel   every workgroup adds the chunk sums (mu), then its chunk's sum of (d_i - mu)^2
//   D5  denoise_thr_count_kernel   every workgroup adds the chunk deviations (sd, thr), then counts its chunk's d_i <= thr
//   D6  denoise_scatter_kernel     chunk_scan.hpp's predicate compaction (D5 counts): the inlier rows ascending, and their number
// THE ORDER of every floating-point sum is block_tree_sum's, a function of the number of terms alone; there is no atomic on a
// floating-point value.  Nothing synchronises; no workgroup waits for another.
#include "knn_selfjoin.hpp"
#include "chunk_scan.hpp"
#include <cmath>

namespace pcreg {

namespace {

// ---- D2. the walk and the mean distance -----------------------------------------------------------------------------------
// selfjoin_klist_walk's prologue, staging rule and visit rule (knn_walk.hpp, knn_selfjoin.hpp) with k1 = k + 1 in k's place; the
// list is this kernel's own: distances only, the k1-th entry in a fixed register.
// A row enters a list only when d <= thr, thr = min(seed, the k1-th entry of any of the row's four lists).
template <int KB>
__global__ __launch_bounds__(kBlock) void denoise_walk_kernel(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                              const float* __restrict__ tbox, int n_tiles, int cull, int k1,
                                                              const float* __restrict__ dk, double* __restrict__ mean_dist,
                                                              unsigned long long* __restrict__ stats) {
    __shared__ WalkLds lds;
    __shared__ float s_red[kBlock / 64];
    const int ta = blockIdx.x / kWalkWgPerTile, part = blockIdx.x % kWalkWgPerTile;
    walk_count_search(stats, (unsigned long long)n_tiles * (unsigned long long)n_tiles);
    float abox[6];
    walk_tile_box(tbox, ta, abox);
    const float D = selfjoin_tile_bound(dk, ta, M, s_red);
    const WalkSelfRow q = walk_self_row(ms, perm, M, ta, part);
    float thr = selfjoin_row_bound(dk, q);
    // The list holds k1 live places at its END: the KB - k1 places in front are filled with -inf, which no distance (>= 0) moves, so
    // the k1-th smallest distance seen is always the LAST entry -- a fixed register, where klist_kth_reg's select per entry against
    // the uniform k keeps 2 KB scalar registers of masks alive through the walk (KB = 32 spilled 8 of them).
    float ld[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) ld[s] = s < KB - k1 ? -INFINITY : INFINITY;
    walk_tiles(
        lds, 0, n_tiles, q.qx, q.qy, q.qz, part == 0 ? stats : nullptr,
        [&](int ct) { return walk_visits(tbox, ct, abox, D, cull); },
        [&](int r) { return walk_row_finite(ms, perm, M, r); },
        [](int) {},
        [&](int, const float4 (&)[4], float (&d)[4]) {
            if (fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= thr) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d[u] <= thr) {
                        klist_insert<KB>(ld, d[u]);
                        thr = fminf(thr, ld[KB - 1]);
                    }
                }
            }
        },
        [&] {
            thr = fminf(thr, __shfl_xor(thr, 1));                 // the row's four lanes share the tightest bound
            thr = fminf(thr, __shfl_xor(thr, 2));
        });
    // the filler becomes +inf: (+inf ..., the ascending distances) is bitonic, and one half-cleaner cascade leaves the list ascending
    // with the empty places last, as the merges and the epilogue want it
#pragma unroll
    for (int s = 0; s < KB; ++s) ld[s] = ld[s] == -INFINITY ? INFINITY : ld[s];
    klist_sort_bitonic<KB>(ld);
    klist_merge_xor<KB>(ld, 1);
    klist_merge_xor<KB>(ld, 2);

    // ---- the epilogue: every lane of the row holds the row's distances ascending; the found ones form a prefix ----
    int n = 0;
#pragma unroll
    for (int s = 0; s < KB; ++s) n += (s < k1 && ld[s] < INFINITY) ? 1 : 0;
    double sum = 0.0;                                             // (the leading 0 of the row itself adds nothing)
#pragma unroll
    for (int s = 0; s < KB; ++s) {
        const double r = __dsqrt_rn((double)ld[s]);
        sum = s < n ? sum + r : sum;
    }
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const double d = n >= 2 ? sum / (double)(n - 1) : qnan;
    if (q.in_model && (threadIdx.x & (kWalkLanes - 1)) == 0) mean_dist[q.row_i] = d;
}

// ---- D3 .. D6. the statistic, the mask and the compaction -------------------------------------------------------------------
// The sum of one value per thread of a workgroup of kScanBlock threads, in a FIXED order: a butterfly over each group of 64
// threads (partners at distance 32, 16, 8, 4, 2, 1; IEEE addition commutes, so both partners form the same bits), then the four
// group sums as (g0 + g1) + (g2 + g3).  Every thread returns the same value.  s4 is the caller's, one array per call site.
template <typename T>
__device__ __forceinline__ T block_tree_sum(T v, T (&s4)[kScanBlock / 64]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}
// ... of an array of n values: thread t adds values t, t + 256, ... in ascending order from zero, then block_tree_sum
template <typename T>
__device__ __forceinline__ T array_tree_sum(const T* __restrict__ a, int n, T (&s4)[kScanBlock / 64]) {
    T v = 0;
    for (int c = threadIdx.x; c < n; c += kScanBlock) v = v + a[c];
    return block_tree_sum(v, s4);
}
__device__ __forceinline__ bool dfinite(double d) { return fabs(d) < (double)INFINITY; }     // (false for NaN)

// thread t of chunk c owns original rows 2048 c + 8 t .. + 7 (chunk_scan.hpp's assignment) and adds them in ascending order
__global__ __launch_bounds__(kScanBlock) void denoise_chunk_sum_kernel(const double* __restrict__ md, int M, double* __restrict__ psum,
                                                                       int32_t* __restrict__ pcnt) {
    __shared__ double s_sum[kScanBlock / 64];
    __shared__ int32_t s_cnt[kScanBlock / 64];
    const long long i0 = (long long)blockIdx.x * kScanChunk + (long long)threadIdx.x * kScanPer;
    double v = 0.0; int32_t c = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        const double d = i0 + j < M ? md[i0 + j] : (double)INFINITY;
        const bool on = dfinite(d);
        v = on ? v + d : v; c += on ? 1 : 0;
    }
    v = block_tree_sum(v, s_sum);
    c = block_tree_sum(c, s_cnt);
    if (threadIdx.x == 0) { psum[blockIdx.x] = v; pcnt[blockIdx.x] = c; }
}

// scal: [0] mu  [1] nf  [2] thr
__global__ __launch_bounds__(kScanBlock) void denoise_chunk_dev_kernel(const double* __restrict__ md, int M, int n_chunks,
                                                                       const double* __restrict__ psum, const int32_t* __restrict__ pcnt,
                                                                       double* __restrict__ pdev, double* __restrict__ scal) {
    __shared__ double s_sum[kScanBlock / 64], s_dev[kScanBlock / 64];
    __shared__ int32_t s_cnt[kScanBlock / 64];
    const double S = array_tree_sum(psum, n_chunks, s_sum);
    const int32_t nf = array_tree_sum(pcnt, n_chunks, s_cnt);
    const double mu = S / (double)nf;                             // (nf = 0: 0 / 0 = NaN)
    const long long i0 = (long long)blockIdx.x * kScanChunk + (long long)threadIdx.x * kScanPer;
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        const double d = i0 + j < M ? md[i0 + j] : (double)INFINITY;
        const double e = d - mu;
        v = dfinite(d) ? v + e * e : v;
    }
    v = block_tree_sum(v, s_dev);
    if (threadIdx.x == 0) {
        pdev[blockIdx.x] = v;
        if (blockIdx.x == 0) { scal[0] = mu; scal[1] = (double)nf; }
    }
}

__global__ __launch_bounds__(kScanBlock) void denoise_thr_count_kernel(const double* __restrict__ md, int M, int n_chunks, double t,
                                                                       const double* __restrict__ pdev, double* __restrict__ scal,
                                                                       int32_t* __restrict__ pin, double* __restrict__ stats_out) {
    __shared__ double s_dev[kScanBlock / 64];
    const double ssd = array_tree_sum(pdev, n_chunks, s_dev);
    const double mu = scal[0], nf = scal[1];
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    const double sd = nf >= 2.0 ? __dsqrt_rn(ssd / (nf - 1.0)) : nf == 1.0 ? 0.0 : qnan;
    const double thr = mu + t * sd;
    chunk_pred_count(M, pin, [&](long long i) { return md[i] <= thr; });          // (NaN on either side: no inlier)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scal[2] = thr;
        if (stats_out) { stats_out[0] = thr; stats_out[1] = mu; stats_out[2] = sd; stats_out[3] = nf; }
    }
}

__global__ __launch_bounds__(kScanBlock) void denoise_scatter_kernel(const double* __restrict__ md, int M, const double* __restrict__ scal,
                                                                     const int32_t* __restrict__ pin, int32_t* __restrict__ inliers,
                                                                     int32_t* __restrict__ n_inliers) {
    const double thr = scal[2];
    const int32_t at = chunk_pred_emit(M, pin, [&](long long i) { return md[i] <= thr; },
                                       [&](int32_t at, long long i) { if (inliers) inliers[at] = (int32_t)i; });      // (no list: count only)
    if (n_inliers && chunk_is_last_thread()) *n_inliers = at;
}

// M = 0: no row, no statistic
__global__ void denoise_empty_kernel(int32_t* __restrict__ n_inliers, double* __restrict__ stats_out) {
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    if (n_inliers) *n_inliers = 0;
    if (stats_out) { stats_out[0] = qnan; stats_out[1] = qnan; stats_out[2] = qnan; stats_out[3] = 0.0; }
}

// Workspace, with R = max(M, 1) and C = max(ceil(M / 2048), 1): [seed bound of every sorted row, R floats][mean distance by original
// row, R doubles (used when the caller wants none)][chunk sums, C doubles][chunk deviations, C doubles][chunk finite counts, C
// int32][chunk inlier counts, C int32][mu, nf, thr: 256 bytes]:
// roundup(4 R, 256) + roundup(8 R, 256) + 2 roundup(8 C, 256) + 2 roundup(4 C, 256) + 256 bytes, whatever k
struct DenoiseWs { float* dk; double* md; double* psum; double* pdev; int32_t* pcnt; int32_t* pin; double* scal; int n_chunks; };
DenoiseWs denoise_ws_layout(int M, void* base, size_t* bytes) {
    DenoiseWs s{};
    WsWalk w(base);
    const size_t R = (size_t)(M > 0 ? M : 1);
    s.n_chunks = (int)((R + kScanChunk - 1) / kScanChunk);
    s.dk = w.take<float>(R);
    s.md = w.take<double>(R);
    s.psum = w.take<double>((size_t)s.n_chunks);
    s.pdev = w.take<double>((size_t)s.n_chunks);
    s.pcnt = w.take<int32_t>((size_t)s.n_chunks);
    s.pin = w.take<int32_t>((size_t)s.n_chunks);
    s.scal = (double*)w.take_bytes(256);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t denoise_ws_bytes(int M, int k) {
    (void)k;                                                      // the lists live in registers
    size_t b; (void)denoise_ws_layout(M, nullptr, &b);
    return b;
}

int launch_model_denoise(const ModelView& v, int k, double threshold, double* mean_dist, int32_t* inliers, int32_t* n_inliers, double* stats,
                         void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(k >= 1 && k <= kNKnnMaxK - 1 && threshold >= 0.0 && threshold < (double)INFINITY && (n_inliers || !inliers));
    size_t need;
    const DenoiseWs s = denoise_ws_layout(v.M, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: denoise workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M;
    if (M == 0) {
        hipLaunchKernelGGL(denoise_empty_kernel, dim3(1), dim3(1), 0, st, n_inliers, stats);
        PCREG_HIP(hipGetLastError());
        return PCREG_OK;
    }
    const int k1 = k + 1;
    const int n_tiles = (M + kT16 - 1) / kT16;
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;          // "knn_nocull": visit every tile, same bits
    unsigned long long* kstats = knn_stats_dev();                 // "knn_stats": searches, visited, nominal (n_tiles^2)
    double* md = mean_dist ? mean_dist : s.md;
    launch_selfjoin_seed(v, k1, s.dk, st);
    klist_dispatch<kSelfKbMin>(k1, [&](auto kb) {
        hipLaunchKernelGGL(denoise_walk_kernel<kb.value>, dim3((unsigned)n_tiles * kWalkWgPerTile), dim3(kBlock), 0, st, (const float*)v.ms,
                           (const int32_t*)v.perm, M, (const float*)v.tbox, n_tiles, cull, k1, (const float*)s.dk, md, kstats);
    });
    const dim3 cgrid((unsigned)s.n_chunks), cblock(kScanBlock);
    hipLaunchKernelGGL(denoise_chunk_sum_kernel, cgrid, cblock, 0, st, (const double*)md, M, s.psum, s.pcnt);
    hipLaunchKernelGGL(denoise_chunk_dev_kernel, cgrid, cblock, 0, st, (const double*)md, M, s.n_chunks, (const double*)s.psum,
                       (const int32_t*)s.pcnt, s.pdev, s.scal);
    hipLaunchKernelGGL(denoise_thr_count_kernel, cgrid, cblock, 0, st, (const double*)md, M, s.n_chunks, threshold, (const double*)s.pdev, s.scal,
                       s.pin, stats);
    if (n_inliers)
        hipLaunchKernelGGL(denoise_scatter_kernel, cgrid, cblock, 0, st, (const double*)md, M, (const double*)s.scal, (const int32_t*)s.pin, inliers,
                           n_inliers);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
