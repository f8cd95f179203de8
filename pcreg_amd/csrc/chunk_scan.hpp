// pcreg_amd/csrc/chunk_scan.hpp -- the two-launch chunk scan, its one definition: an exclusive scan of one value
// per element over any number of chunks of kScanChunk elements, a workgroup of kScanBlock threads per chunk, no workgroup
// waiting for another.  Launch 1: every chunk's sum (chunk_sum).  Launch 2: thread t of chunk c owns the chunk's elements
// kScanPer t .. kScanPer t + kScanPer - 1 and learns what lies before them (chunk_offset).  T is int32_t or int64_t.
// On top of the two: the compaction of a per-row predicate into an ascending row list (chunk_pred_count, chunk_pred_emit).
#pragma once
#include "common.hpp"

namespace pcreg {
namespace {

constexpr int kScanBlock = 256;
constexpr int kScanChunk = 2048;                     // elements per workgroup
constexpr int kScanPer = kScanChunk / kScanBlock;    // consecutive elements per thread of launch 2

// csum[this chunk] = the sum of the workgroup's v (each thread's sum over its elements, in any assignment)
template <typename T>
__device__ __forceinline__ void chunk_sum(T v, T* __restrict__ csum) {
    __shared__ T s[kScanBlock / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) csum[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

// the sum of everything before this thread's elements: the chunks before chunk `chunk` of csum, plus `mine` of the threads before
// this one (a grid of several scans side by side names its own chunk; chunk_offset is the one scan whose chunk is the workgroup)
template <typename T>
__device__ __forceinline__ T chunk_offset_at(const T* __restrict__ csum, int chunk, T mine) {
    __shared__ T s[kScanBlock / 64], s_thr[kScanBlock];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T before = 0;
    for (int c = tid; c < chunk; c += kScanBlock) before += csum[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
    if (lane == 0) s[wave] = before;
    s_thr[tid] = mine;
    __syncthreads();
    const T run = s[0] + s[1] + s[2] + s[3];
    // inclusive scan of the 256 thread sums (Hillis-Steele in LDS)
    for (int o = 1; o < kScanBlock; o <<= 1) {
        const T add = tid >= o ? s_thr[tid - o] : 0;
        __syncthreads();
        s_thr[tid] += add;
        __syncthreads();
    }
    return run + (s_thr[tid] - mine);
}
template <typename T>
__device__ __forceinline__ T chunk_offset(const T* __restrict__ csum, T mine) {
    return chunk_offset_at<T>(csum, (int)blockIdx.x, mine);
}

// ---- the compaction of a predicate pred(i) on rows 0 .. n - 1 into an ascending row list, on the scan's two launches ----------
// this thread's rows with pred
template <class Pred>
__device__ __forceinline__ int32_t chunk_pred_mine(int n, Pred pred) {
    const long long i0 = (long long)blockIdx.x * kScanChunk + (long long)threadIdx.x * kScanPer;
    int32_t c = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) c += (i0 + j < n && pred(i0 + j)) ? 1 : 0;
    return c;
}
// launch 1: csum[this chunk] = the chunk's rows with pred
template <class Pred>
__device__ __forceinline__ void chunk_pred_count(int n, int32_t* __restrict__ csum, Pred pred) {
    chunk_sum<int32_t>(chunk_pred_mine(n, pred), csum);
}
// launch 2: emit(at, i) for each of this thread's rows i with pred, ascending, at = the number of such rows before i.  Returns at
// behind the thread's last row: what the last thread of the last chunk holds is the list's length.
template <class Pred, class Emit>
__device__ __forceinline__ int32_t chunk_pred_emit(int n, const int32_t* __restrict__ csum, Pred pred, Emit emit) {
    const long long i0 = (long long)blockIdx.x * kScanChunk + (long long)threadIdx.x * kScanPer;
    int32_t at = chunk_offset<int32_t>(csum, chunk_pred_mine(n, pred));
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        if (i0 + j < n && pred(i0 + j)) { emit(at, i0 + j); ++at; }
    }
    return at;
}
__device__ __forceinline__ bool chunk_is_last_thread() { return blockIdx.x == gridDim.x - 1 && threadIdx.x == kScanBlock - 1; }

}  // namespace
}  // namespace pcreg
