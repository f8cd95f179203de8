// pcreg_amd/csrc/knn_fpfh_radius.hip -- the FPFH descriptor (33 numbers) of every row of a PREPARED model from the rows within a
// squared radius and a normal per row: the neighbourhood rule of Rusu's paper, with an optional cap on the number of neighbours
// (the n nearest within the radius).  The contract is pcreg_model_fpfh_radius_f32's (include/pcreg.h); DESIGN 4.24.  The pair
// features, the bins and the weighting are the k-nearest form's (knn_fpfh.hip, fpfh_pair.hpp); only the neighbourhood differs, and
// with it the size of a count: up to M - 1, so the SPFH counts are uint32.
//
// The size of the lists is data, so the call is two: the count (the radius search's own, with the model's rows as the queries),
// and, once the caller has read the total and sized the workspace, the fill and the two kernels of this file:
//   launch_model_range_fill      (knn_range.hip) every row's segment of (original row, fp32 squared distance) in (distance, row) order
//   R1  fpfh_radius_spfh_kernel<L>   L = 64 lanes (a wave) per ORIGINAL row: the counted window of the row's segment (its leading zeros skipped, at
//                                    most max_neighbors entries, nothing at +inf), the pairs group-strided over the lanes, counted
//                                    into the row's 33 LDS words by integer atomics; the group stores the counts, m_i and the window's
//                                    length
//   R2  fpfh_radius_weight_kernel    one thread per (original row, bin): the same window in list order, (c_j[b] / m_j) / d2 added
//                                    sequentially; the 33 sums of a row meet in LDS and every thread re-adds its feature's eleven in
//                                    bin order, so the eleven threads of a feature hold the same S_f
// No floating-point value is added across threads in any order but that one: the result is a function of (model rows, normals, r2,
// max_neighbors) alone.  Nothing synchronises; no workgroup waits for another.  Every row index read from a list is checked against
// M before it is used: a capacity below the total (truncated segments) or a seg_off of another radius reads nothing out of bounds.
#include "common.hpp"
#include "knn_fast_common.hpp"
#include "knn_walk.hpp"                              // finite3
#include "fpfh_pair.hpp"
#include <cmath>

namespace pcreg {

namespace {

constexpr int kFpfhRadiusMaxM = kMaxQTiles * 1024;  // the radius search's queries per call: the model's rows are one batch
constexpr int kSpfhLanes = 64;                       // lanes per row of R1: a wave a row (4 and 16 measured: DESIGN 4.24)
constexpr int kWeightRows = kBlock / kFpfhDim;       // rows per workgroup of R2: 7 (231 of 256 threads carry a bin)

// the part of [seg_off[i], seg_off[i + 1]) inside [0, capacity), whatever seg_off holds (the radius search's rule): begin and length
__device__ __forceinline__ void radius_segment(const int64_t* __restrict__ seg_off, size_t i, int64_t capacity, int M, int64_t& b, int& len) {
    const int64_t s0 = seg_off[i], s1 = seg_off[i + 1];
    b = s0 < 0 ? 0 : (s0 > capacity ? capacity : s0);
    const int64_t e = s1 < b ? b : (s1 > capacity ? capacity : s1);
    len = (int)(e - b > (int64_t)M ? (int64_t)M : e - b);        // (a segment of the model's own rows holds at most M)
}

// ---- R1. the SPFH counts over ragged segments ------------------------------------------------------------------------------
// Group g of the workgroup serves original row blockIdx * (kBlock / L) + g.  The segment is sorted by (distance, row): its zeros
// lead and its +inf entries trail, so the counted window is [z, min(z + n, f)) with z the entries that are not > 0 and f the
// entries < +inf, both counted group-strided and added over the group (integers).
template <int L>
__global__ __launch_bounds__(kBlock) void fpfh_radius_spfh_kernel(const float* __restrict__ m, int ldm, int M, const float* __restrict__ normals,
                                                                  int ldn, const int64_t* __restrict__ seg_off, int64_t capacity, int max_nb,
                                                                  const int32_t* __restrict__ lrow, const float* __restrict__ ldist,
                                                                  uint32_t* __restrict__ spfh, int32_t* __restrict__ mcount,
                                                                  int32_t* __restrict__ n_nb) {
    constexpr int kRows = kBlock / L;
    __shared__ uint32_t s_hist[kRows * kFpfhDim];
    const int g = threadIdx.x / L, sub = threadIdx.x % L;
    const long long row = (long long)blockIdx.x * kRows + g;
    const bool in_model = row < (long long)M;
    const size_t ri = in_model ? (size_t)row : 0;
    for (int t = threadIdx.x; t < kRows * kFpfhDim; t += kBlock) s_hist[t] = 0u;
    __syncthreads();
    int64_t b = 0; int len = 0;
    if (in_model) radius_segment(seg_off, ri, capacity, M, b, len);
    int z = 0, f = 0;
    for (int s = sub; s < len; s += L) {
        const float d2 = ldist[b + s];
        z += d2 > 0.0f ? 0 : 1;
        f += d2 < INFINITY ? 1 : 0;
    }
#pragma unroll
    for (int o = 1; o < L; o <<= 1) { z += __shfl_xor(z, o); f += __shfl_xor(f, o); }
    const int wb = z < len ? z : len;
    int we = f < wb ? wb : f;
    if (max_nb > 0 && we - wb > max_nb) we = wb + max_nb;
    const double pix = (double)m[ri], piy = (double)m[ri + (size_t)ldm], piz = (double)m[ri + 2 * (size_t)ldm];
    const double nix = (double)normals[ri], niy = (double)normals[ri + (size_t)ldn], niz = (double)normals[ri + 2 * (size_t)ldn];
    uint32_t* hist = s_hist + g * kFpfhDim;
    for (int s = wb + sub; s < we; s += L) {
        const int j = lrow[b + s];
        const bool ok = (unsigned)j < (unsigned)M;
        const size_t rj = ok ? (size_t)j : ri;
        const double pjx = (double)m[rj], pjy = (double)m[rj + (size_t)ldm], pjz = (double)m[rj + 2 * (size_t)ldm];
        const double njx = (double)normals[rj], njy = (double)normals[rj + (size_t)ldn], njz = (double)normals[rj + 2 * (size_t)ldn];
        int b1, b2, b3;
        const bool on = fpfh_pair(pix, piy, piz, nix, niy, niz, pjx, pjy, pjz, njx, njy, njz, b1, b2, b3) && ok;
        if (on) {
            atomicAdd(&hist[b1], 1u);
            atomicAdd(&hist[kFpfhBins + b2], 1u);
            atomicAdd(&hist[2 * kFpfhBins + b3], 1u);
        }
    }
    __syncthreads();
    if (in_model) {
        uint32_t* o = spfh + ri * (size_t)kFpfhDim;
        for (int c = sub; c < kFpfhDim; c += L) o[c] = hist[c];
        if (sub == 0) {
            uint32_t mi = 0u;
#pragma unroll
            for (int c = 0; c < kFpfhBins; ++c) mi += hist[c];
            mcount[ri] = (int32_t)mi;
            if (n_nb) n_nb[ri] = we - wb;
        }
    }
}

// ---- R2. the weighted sum of the neighbours' histograms --------------------------------------------------------------------
// Thread t of the workgroup serves bin t % 33 of original row blockIdx * 7 + t / 33: the 33 threads of a row read the 132
// contiguous bytes of neighbour j's counts and store 33 consecutive doubles.  The window is R1's, found again from the list: the
// leading entries that are not > 0 are skipped, then at most max_nb entries are taken, and an entry at +inf (they trail) adds nothing.
// Four list entries are fetched ahead of the four dependent gathers; the additions keep the list's order.
__global__ __launch_bounds__(kBlock) void fpfh_radius_weight_kernel(const float* __restrict__ m, int ldm, int M, const int64_t* __restrict__ seg_off,
                                                                    int64_t capacity, int max_nb, const int32_t* __restrict__ lrow,
                                                                    const float* __restrict__ ldist, const uint32_t* __restrict__ spfh,
                                                                    const int32_t* __restrict__ mcount, double* __restrict__ out) {
    __shared__ double s_acc[kWeightRows * kFpfhDim];
    const int t = threadIdx.x, g = t / kFpfhDim, bin = t - g * kFpfhDim;
    const long long row = (long long)blockIdx.x * kWeightRows + g;
    const bool in_model = g < kWeightRows && row < (long long)M;
    const size_t r = in_model ? (size_t)row : 0;
    double acc = 0.0;
    if (in_model) {
        int64_t b; int len;
        radius_segment(seg_off, r, capacity, M, b, len);
        int s = 0;
        while (s < len && !(ldist[b + s] > 0.0f)) ++s;
        const int end = (max_nb > 0 && len - s > max_nb) ? s + max_nb : len;
        for (; s < end; s += 4) {
            int j[4]; float d2[4]; bool use[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool live = s + u < end;
                j[u] = live ? lrow[b + s + u] : -1;
                d2[u] = live ? ldist[b + s + u] : INFINITY;
            }
            uint32_t c[4]; int mj[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                use[u] = (unsigned)j[u] < (unsigned)M && d2[u] < INFINITY && d2[u] > 0.0f;
                const size_t rj = use[u] ? (size_t)j[u] : r;
                mj[u] = mcount[rj];
                c[u] = spfh[rj * (size_t)kFpfhDim + (size_t)bin];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double term = ((double)c[u] / (double)mj[u]) / (double)d2[u];
                acc = (use[u] && mj[u] > 0) ? acc + term : acc;
            }
        }
    }
    if (t < kWeightRows * kFpfhDim) s_acc[t] = acc;
    __syncthreads();
    if (in_model) {
        const double* a = s_acc + g * kFpfhDim + (bin / kFpfhBins) * kFpfhBins;
        double S = a[0];
#pragma unroll
        for (int k = 1; k < kFpfhBins; ++k) S = S + a[k];
        const bool finite = finite3(m[r], m[r + (size_t)ldm], m[r + 2 * (size_t)ldm]);
        const double qnan = __longlong_as_double(0x7FF8000000000000ll);
        out[r * (size_t)kFpfhDim + (size_t)bin] = !finite ? qnan : S > 0.0 ? (acc / S) * 100.0 : 0.0;
    }
}

// Workspace, with R = max(M, 1) and C = the capacity: [the radius search's own workspace for M queries][the lists' rows, C int32]
// [their fp32 squared distances, C floats][m_j, R int32][the SPFH counts, 33 R uint32 (used when the caller wants none)]:
// range_ws_bytes(M) + 2 roundup(4 C, 256) + roundup(4 R, 256) + roundup(132 R, 256) bytes
struct FpfhRadiusWs { void* range; size_t range_bytes; int32_t* lrow; float* ldist; int32_t* mcount; uint32_t* spfh; };
FpfhRadiusWs fpfh_radius_ws_layout(int M, int64_t capacity, void* base, size_t* bytes) {
    FpfhRadiusWs s{};
    WsWalk w(base);
    const size_t R = (size_t)(M > 0 ? M : 1), Cp = (size_t)(capacity > 0 ? capacity : 0);
    s.range_bytes = align_up(range_ws_bytes(M > 0 ? M : 0, M), 256);
    s.range = w.take_bytes(s.range_bytes);
    s.lrow = w.take<int32_t>(Cp);
    s.ldist = w.take<float>(Cp);
    s.mcount = w.take<int32_t>(R);
    s.spfh = w.take<uint32_t>(R * (size_t)kFpfhDim);
    *bytes = w.bytes();
    return s;
}

template <int L>
void launch_spfh(const ModelView& v, int max_nb, const float* normals, int ldn, const int64_t* seg_off, int64_t capacity, const FpfhRadiusWs& s,
                 uint32_t* counts, int32_t* n_nb, hipStream_t st) {
    constexpr int kRows = kBlock / L;
    hipLaunchKernelGGL(fpfh_radius_spfh_kernel<L>, dim3((unsigned)((v.M + kRows - 1) / kRows)), dim3(kBlock), 0, st, v.m, v.ldm, v.M, normals, ldn,
                       seg_off, capacity, max_nb, (const int32_t*)s.lrow, (const float*)s.ldist, counts, s.mcount, n_nb);
}

}  // namespace

size_t fpfh_radius_ws_bytes(int M, int64_t capacity) {
    size_t b; (void)fpfh_radius_ws_layout(M, capacity, nullptr, &b);
    return b;
}

int fpfh_radius_max_rows() { return kFpfhRadiusMaxM; }

int launch_model_fpfh_radius_count(const ModelView& v, float r2, int32_t* counts, int64_t* seg_off, void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(r2 >= 0.0f && v.M <= kFpfhRadiusMaxM && (counts || v.M == 0) && seg_off);
    size_t need;
    const FpfhRadiusWs s = fpfh_radius_ws_layout(v.M, 0, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: fpfh radius workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    return launch_model_range_count(v, v.m, v.M, v.ldm, r2, counts, seg_off, s.range, s.range_bytes, st);
}

int launch_model_fpfh_radius(const ModelView& v, float r2, int max_neighbors, const float* normals, int ldn, const int64_t* seg_off,
                             int64_t capacity, double* fpfh, uint32_t* spfh, int32_t* n_neighbors, void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(r2 >= 0.0f && max_neighbors >= 0 && capacity >= 0 && v.M <= kFpfhRadiusMaxM && ldn >= v.M && seg_off &&
              ((normals && fpfh) || v.M == 0));
    size_t need;
    const FpfhRadiusWs s = fpfh_radius_ws_layout(v.M, capacity, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: fpfh radius workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M;
    if (M == 0) return PCREG_OK;
    const int rc = launch_model_range_fill(v, v.m, M, v.ldm, r2, 0, seg_off, capacity, s.lrow, s.ldist, s.range, s.range_bytes, st);
    if (rc) return rc;
    uint32_t* counts = spfh ? spfh : s.spfh;
    const int lanes = debug_flag(kDbgFpfhRadiusLanes);           // "fpfh_radius_lanes": 4 or 16 lanes a row, same bits
    if (lanes == 4) launch_spfh<4>(v, max_neighbors, normals, ldn, seg_off, capacity, s, counts, n_neighbors, st);
    else if (lanes == 16) launch_spfh<16>(v, max_neighbors, normals, ldn, seg_off, capacity, s, counts, n_neighbors, st);
    else launch_spfh<kSpfhLanes>(v, max_neighbors, normals, ldn, seg_off, capacity, s, counts, n_neighbors, st);
    hipLaunchKernelGGL(fpfh_radius_weight_kernel, dim3((unsigned)((M + kWeightRows - 1) / kWeightRows)), dim3(kBlock), 0, st, v.m, v.ldm, M, seg_off,
                       capacity, max_neighbors, (const int32_t*)s.lrow, (const float*)s.ldist, (const uint32_t*)counts, (const int32_t*)s.mcount,
                       fpfh);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
