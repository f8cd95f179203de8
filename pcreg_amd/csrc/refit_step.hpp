// pcreg_amd/csrc/refit_step.hpp -- the skeleton of "refit B candidate transforms by one step of method X" (DESIGN 4.28), its one
// definition.  The rigid (4.14), point-to-plane (4.16), NDT (4.25), plane-to-plane (4.26) and coherent-point-drift (4.27) steps
// differ in the middle of their sums kernel and in their fit; everything around that middle is here:
//   moved_point        the transformed query every step and the scoring agree on
//   chunk_tail         a workgroup's up to 28 sums of a chunk of 2048 queries -> that chunk's partials, one fixed tree
//   hit_rows           the winning model row of a thread's eight queries (the plane and plane-to-plane sums)
//   finish_step        one wave per transform: the chunks in ascending order, the method's fit, then
//   step_compose       T_step, T_out = T_in * T_step and the empty rule (a failed fit: empty = 1 and 32 zeros)
//   scan_chunks        the chunks of Q queries
// (launch_refit_empty, a call without pairs, is common.hpp's: one kernel in knn_score.hip serves every method.)
// fp64 sums in one fixed order only: nothing here depends on the order in which workgroups run.
#pragma once
#include "chunk_scan.hpp"
#include "moments.hpp"
#include "compose.hpp"
#include <algorithm>

namespace pcreg {
namespace {

inline int scan_chunks(int Q) { return std::max(1, (Q + kScanChunk - 1) / kScanChunk); }

// ---- the moved point ----------------------------------------------------------------------------------------------------
// t = transform bl of T; true when all sixteen are zero (what a failed ransac leaves: it moves nothing)
__device__ __forceinline__ bool load_transform(const double* __restrict__ T, int bl, double (&t)[16]) {
    bool zero = true;
#pragma unroll
    for (int e = 0; e < 16; ++e) { t[e] = T[(size_t)bl * 16 + e]; zero = zero && t[e] == 0.0; }
    return zero;
}
__device__ __forceinline__ bool transform_is_zero(const double* __restrict__ T, int bl) {
    bool zero = true;
    for (int e = 0; e < 16; ++e) zero = zero && T[(size_t)bl * 16 + e] == 0.0;
    return zero;
}
// [x y z 1] * t as quick_tf_kernel forms it (sweep.hip; the build's -ffp-contract=off): the chain in double on the widened fp32
// query, rounded once to fp32.  An all-zero transform's point is NaN.  The scoring contract rests on every kernel
// that moves a query calling this.
__device__ __forceinline__ void moved_point(const double (&t)[16], double x, double y, double z, bool t_zero, float (&p)[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double v = ((x * t[4 * j] + y * t[4 * j + 1]) + z * t[4 * j + 2]) + t[4 * j + 3];
        p[j] = t_zero ? __int_as_float(0x7FC00000) : (float)v;
    }
}

// ---- the chunk tail -----------------------------------------------------------------------------------------------------
// v = N values every lane of a wave holds alike (a wave's sums): lane 0 of each wave through LDS, the four waves added in
// ascending order; thread k < N of the workgroup of kScanBlock threads returns sum k, the others 0.  (A caller that comes here
// again in the same kernel puts a __syncthreads in between: the LDS array is read until every thread has returned.)
template <int N>
__device__ __forceinline__ double waves_sum(const double (&v)[N]) {
    __shared__ double s_m[kScanBlock / 64][N];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s_m[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    const int k = threadIdx.x < N ? threadIdx.x : 0;
    const double sum = ((s_m[0][k] + s_m[1][k]) + s_m[2][k]) + s_m[3][k];
    return threadIdx.x < N ? sum : 0.0;
}
// ... out[blockIdx.x * N + k] = sum k of this workgroup
template <int N>
__device__ __forceinline__ void waves_sum_store(const double (&v)[N], double* __restrict__ out) {
    const double sum = waves_sum(v);
    if (threadIdx.x < N) out[(size_t)blockIdx.x * N + threadIdx.x] = sum;
}
// the N <= 28 sums of a moments kernel: the thread's acc[0 .. min(N, 27)) and, where N is 28, `last`; wave_sum27 and wave_sum, then
// waves_sum.  chunk_sums returns sum k in thread k < N; chunk_tail stores it as waves_sum_store does
template <int N>
__device__ __forceinline__ double chunk_sums(double (&acc)[27], double last) {
    static_assert(N >= 1 && N <= 28, "27 sums through wave_sum27 and one more");
    wave_sum27(acc);
    double v[N];
#pragma unroll
    for (int k = 0; k < (N < 27 ? N : 27); ++k) v[k] = acc[k];
    if constexpr (N == 28) v[27] = wave_sum(last);
    return waves_sum(v);
}
template <int N>
__device__ __forceinline__ void chunk_tail(double (&acc)[27], double last, double* __restrict__ out) {
    const double sum = chunk_sums<N>(acc, last);
    if (threadIdx.x < N) out[(size_t)blockIdx.x * N + threadIdx.x] = sum;
}
// a few sums, each through wave_sum
template <int N>
__device__ __forceinline__ void chunk_tail_few(double (&a)[N], double* __restrict__ out) {
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = wave_sum(a[k]);
    waves_sum_store(a, out);
}

// ---- the hit prologue ---------------------------------------------------------------------------------------------------
// row[u] = the winning ORIGINAL row of query i0 + u of transform bl where that query has a hit (best == best), -1 otherwise: the
// eight (best, row) loads of a thread, issued together.  (A hit's row is a model row: the walk wrote it.)
__device__ __forceinline__ void hit_rows(const float* __restrict__ best, const int32_t* __restrict__ prow, int bl, int i0, int Q, int M,
                                         int (&row)[kScanPer]) {
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        row[u] = -1;
        if (i0 + u < Q) {
            const size_t s = (size_t)bl * Q + i0 + u;
            const float d = best[s];
            const int r = prow[s];
            if (d == d && (unsigned)r < (unsigned)M) row[u] = r;
        }
    }
}

// ---- the finish step ----------------------------------------------------------------------------------------------------
// Lanes 0 .. 15 of the one wave of transform bl hold v = entry `lane` of T_step (zero where !ok): T_step (may be null) and
// T_out = T_in * T_step, every entry compose.hpp's compose_entry.
// !ok: empty = 1 and T_out zeros.
__device__ __forceinline__ void step_compose(int bl, int lane, double v, bool ok, const double* __restrict__ T_in, double* __restrict__ T_out,
                                             double* __restrict__ T_step, int32_t* __restrict__ empty) {
    __shared__ double s_S[16];
    if (lane < 16) {
        s_S[lane] = v;
        if (T_step) T_step[(size_t)bl * 16 + lane] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    if (lane < 16) {
        const int r = lane & 3, c = lane >> 2;
        const double w = compose_entry(T_in + (size_t)bl * 16, s_S, r, c);
        T_out[(size_t)bl * 16 + r + 4 * c] = ok ? w : 0.0;
    }
    if (lane == 0) empty[bl] = ok ? 0 : 1;
}
// One wave per transform bl = blockIdx.x: lane k < N adds sum k over the chunks in ascending order, lane N the chunks' counts
// (kCount); every lane then holds the same N sums and the count and runs fit(sums, cnt, T) -> T_step or false; step_compose
// follows.  Returns the fit's answer; sums and cnt are left for the caller's own outputs.
template <int N, bool kCount, class Fit>
__device__ __forceinline__ bool finish_step(const double* __restrict__ psums, const int32_t* __restrict__ pcnt, int chunks, const double* __restrict__ T_in,
                                            double* __restrict__ T_out, double* __restrict__ T_step, int32_t* __restrict__ empty, Fit fit,
                                            double (&sums)[N], int& cnt) {
    __shared__ double s_sum[N];
    __shared__ int32_t s_cnt;
    const int bl = blockIdx.x, lane = threadIdx.x;
    if (lane < N) {
        double v = 0.0;
        for (int c = 0; c < chunks; ++c) v += psums[((size_t)bl * chunks + c) * N + lane];
        s_sum[lane] = v;
    } else if (kCount && lane == N) {
        int32_t n = 0;
        for (int c = 0; c < chunks; ++c) n += pcnt[(size_t)bl * chunks + c];
        s_cnt = n;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < N; ++k) sums[k] = s_sum[k];
    cnt = kCount ? s_cnt : 0;
    double T[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) T[e] = 0.0;
    const bool ok = fit(sums, cnt, T);
    double v = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) if (e == lane) v = T[e];
    step_compose(bl, lane, ok ? v : 0.0, ok, T_in, T_out, T_step, empty);
    return ok;
}

}  // namespace
}  // namespace pcreg
