// pcreg_amd/csrc/knn_trim.hip -- the trim pass of the scoring chain: between the walk and everything that reads
// `best` (knn_score.hip), keep each transform's `keep` closest candidate pairs and turn the others into misses.
//
// Contract (include/pcreg.h): the candidate pairs of transform b are the non-NaN entries of best[b][0 .. Q); n_within[b] is their
// number and keep = n_within == 0 ? 0 : min(n_within, max(1, (int)floor(keep_ratio * (double)n_within + 0.5))), in double, the
// product rounded before the sum.  THE KEPT PAIRS are the `keep` first in the order (d ascending, query ascending); d is never
// negative and never NaN, so its bit pattern orders as an unsigned integer (+inf last).  d2_cut = the largest kept d, +inf
// when keep is 0.  A trimmed slot gets NaN in best and -1 / +inf in the caller's idx / dist, as a miss has.
//
// Per batch of nb transforms, grid (transform, chunk of 2048 queries) as score_reduce_kernel unless said otherwise:
//   T0  hipMemsetAsync                the [nb][256] digit counters (each T2 leaves them zero for the next pass)
//   T1  trim_hist_kernel  x 4         pass p = 0 .. 3, most significant byte first: the chunk's entries whose upper 8 p bits are
//                                     the transform's prefix, counted by their next byte in LDS (integer atomics; a wave whose
//                                     entries all fall in one bin adds once), then one global integer atomic per non-zero bin
//   T2  trim_pick_kernel  x 4         one wave per transform after each T1: the bin that holds the wanted rank; prefix <- prefix : bin,
//                                     rank <- rank - (the entries in lower bins).  Pass 0 also gives n_within and keep.
//                                     After pass 3: prefix = the bits of d2_cut, rank + 1 = the ties to keep
//   T3  trim_count_kernel             per chunk: its entries equal to the cut (chunk_sum)
//   T4  trim_mask_kernel              thread t owns eight consecutive queries: the ties before them (chunk_offset_at over the
//                                     transform's chunks, ascending), then NaN for every entry above the cut and for the ties
//                                     beyond the budget; one thread per transform writes n_within and d2_cut
// Every dependency is a launch boundary.  The counters are integer sums, so the order in which workgroups arrive changes
// nothing: the kept set is a function of `best` and keep_ratio alone.
#include "common.hpp"
#include "chunk_scan.hpp"
#include <cmath>
#include <cstdint>

namespace pcreg {

namespace {

// the select state of one transform
struct TrimSel { uint32_t prefix; int32_t rank; int32_t keep; int32_t n_within; };
static_assert(sizeof(TrimSel) == kTrimSelBytes, "score_ws_layout sizes the state by kTrimSelBytes");

__device__ __forceinline__ int32_t trim_keep(double ratio, int32_t n) {
    if (n == 0) return 0;
    const double x = floor(__dadd_rn(__dmul_rn(ratio, (double)n), 0.5));
    const int32_t k = (int32_t)x;                                // (x <= n + 1 <= 4 Mi + 1)
    return k < 1 ? 1 : k > n ? n : k;
}

// ---- T1. one byte's histogram ---------------------------------------------------------------------------------------------
// the threads take the chunk's entries strided (the sums do not depend on who counts what)
__global__ __launch_bounds__(kScanBlock) void trim_hist_kernel(const float* __restrict__ best, int Q, int chunks, int pass,
                                                               const TrimSel* __restrict__ sel, int32_t* __restrict__ hist) {
    __shared__ int32_t s_h[256];
    const int bl = blockIdx.x / chunks, c = blockIdx.x - bl * chunks, tid = threadIdx.x, lane = tid & 63;
    uint32_t prefix = 0;
    if (pass > 0) {
        const TrimSel s = sel[bl];
        if (s.keep == 0) return;                                 // (the whole workgroup: a transform without pairs)
        prefix = s.prefix;
    }
    s_h[tid] = 0;
    __syncthreads();
    const int lo = 24 - 8 * pass;                                // the digit's lowest bit
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const int i = c * kScanChunk + u * kScanBlock + tid;
        bool in = false;
        uint32_t digit = 0;
        if (i < Q) {
            const float d = best[(size_t)bl * Q + i];
            const uint32_t key = __float_as_uint(d);
            in = d == d && (pass == 0 || (key >> (lo + 8)) == prefix);
            digit = (key >> lo) & 255u;
        }
        const unsigned long long m = __ballot(in);
        if (m != 0) {                                            // (wave-uniform)
            const int lead = __ffsll((long long)m) - 1;
            const uint32_t d0 = (uint32_t)__shfl((int)digit, lead);
            if (__ballot(in && digit == d0) == m) {              // one bin for the whole wave: one add
                if (lane == lead) atomicAdd(&s_h[d0], (int32_t)__popcll(m));
            } else if (in) {
                atomicAdd(&s_h[digit], 1);
            }
        }
    }
    __syncthreads();
    const int32_t v = s_h[tid];
    if (v != 0) atomicAdd(&hist[(size_t)bl * 256 + tid], v);
}

// ---- T2. the bin of the wanted rank -----------------------------------------------------------------------------------------
// one wave per transform; lane l owns bins 4 l .. 4 l + 3, reads them and clears them
__global__ __launch_bounds__(64) void trim_pick_kernel(int32_t* __restrict__ hist, int pass, double keep_ratio, TrimSel* __restrict__ sel) {
    const int bl = blockIdx.x, lane = threadIdx.x;
    int32_t* __restrict__ h = hist + (size_t)bl * 256 + 4 * lane;
    const int32_t c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
    h[0] = 0; h[1] = 0; h[2] = 0; h[3] = 0;                      // the next pass counts from zero
    const int32_t mine = (c0 + c1) + (c2 + c3);
    int32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    TrimSel s;
    if (pass == 0) {
        s.n_within = __shfl(incl, 63);
        s.keep = trim_keep(keep_ratio, s.n_within);
        s.prefix = 0;
        s.rank = s.keep - 1;
        if (s.keep == 0) {
            s.rank = 0;
            if (lane == 0) sel[bl] = s;
            return;
        }
    } else {
        s = sel[bl];
        if (s.keep == 0) return;
    }
    const int32_t excl = incl - mine;
    if (excl <= s.rank && s.rank < incl) {                       // exactly one lane: 0 <= rank < the entries under the prefix
        int32_t r = s.rank - excl;
        int b = 0;
        if (r >= c0) { r -= c0; b = 1; if (r >= c1) { r -= c1; b = 2; if (r >= c2) { r -= c2; b = 3; } } }
        s.prefix = (s.prefix << 8) | (uint32_t)(4 * lane + b);
        s.rank = r;
        sel[bl] = s;
    }
}

// ---- T3. the ties of every chunk ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanBlock) void trim_count_kernel(const float* __restrict__ best, int Q, int chunks, const TrimSel* __restrict__ sel,
                                                                int32_t* __restrict__ tie) {
    const int bl = blockIdx.x / chunks, c = blockIdx.x - bl * chunks;
    const TrimSel s = sel[bl];
    int32_t cnt = 0;
    if (s.keep != 0) {
#pragma unroll
        for (int u = 0; u < kScanPer; ++u) {
            const int i = c * kScanChunk + u * kScanBlock + (int)threadIdx.x;
            if (i < Q) {
                const float d = best[(size_t)bl * Q + i];
                if (d == d && __float_as_uint(d) == s.prefix) ++cnt;
            }
        }
    }
    chunk_sum(cnt, tie);
}

// ---- T4. the mask -------------------------------------------------------------------------------------------------------------
// idx / dist: the caller's tables at this batch's first transform, or null
__global__ __launch_bounds__(kScanBlock) void trim_mask_kernel(float* __restrict__ best, int Q, int chunks, const TrimSel* __restrict__ sel,
                                                               const int32_t* __restrict__ tie, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                               int32_t* __restrict__ n_within, float* __restrict__ d2_cut) {
    const int bl = blockIdx.x / chunks, c = blockIdx.x - bl * chunks;
    const int i0 = c * kScanChunk + (int)threadIdx.x * kScanPer;
    const TrimSel s = sel[bl];
    if (c == 0 && threadIdx.x == 0) {
        if (n_within) n_within[bl] = s.n_within;
        if (d2_cut) d2_cut[bl] = s.keep != 0 ? __uint_as_float(s.prefix) : INFINITY;
    }
    if (s.keep == 0 || s.keep == s.n_within) return;             // (the whole workgroup) nothing to trim
    float d[kScanPer];
    int32_t mine = 0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        d[u] = __int_as_float(0x7FC00000);
        if (i0 + u < Q) d[u] = best[(size_t)bl * Q + i0 + u];
        mine += (d[u] == d[u] && __float_as_uint(d[u]) == s.prefix) ? 1 : 0;
    }
    int32_t at = chunk_offset_at<int32_t>(tie + (size_t)bl * chunks, c, mine);
    const int32_t budget = s.rank + 1;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        if (d[u] == d[u]) {                                      // (a pair: its query is below Q)
            const uint32_t key = __float_as_uint(d[u]);
            const bool trim = key > s.prefix || (key == s.prefix && at++ >= budget);
            if (trim) {
                const size_t slot = (size_t)bl * Q + i0 + u;
                best[slot] = __int_as_float(0x7FC00000);
                if (idx) idx[slot] = -1;
                if (dist) dist[slot] = INFINITY;
            }
        }
    }
}

// a call without pairs (Q = 0 or a model without rows)
__global__ __launch_bounds__(kScanBlock) void trim_empty_kernel(int B, int32_t* __restrict__ n_within, float* __restrict__ d2_cut) {
    const int b = blockIdx.x * kScanBlock + threadIdx.x;
    if (b >= B) return;
    if (n_within) n_within[b] = 0;
    if (d2_cut) d2_cut[b] = INFINITY;
}

}  // namespace

int launch_score_trim(float* best, int Q, int chunks, int nb, double keep_ratio, int32_t* hist, void* sel, int32_t* tie, int32_t* idx, float* dist,
                      int32_t* n_within, float* d2_cut, hipStream_t st) {
    PCREG_ARG(keep_ratio > 0.0 && keep_ratio <= 1.0 && Q > 0 && nb > 0 && chunks == (Q + kScanChunk - 1) / kScanChunk);
    PCREG_HIP(hipMemsetAsync(hist, 0, sizeof(int32_t) * 256 * (size_t)nb, st));
    const dim3 grid((unsigned)((size_t)nb * chunks)), block(kScanBlock);
    TrimSel* s = (TrimSel*)sel;
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(trim_hist_kernel, grid, block, 0, st, (const float*)best, Q, chunks, pass, (const TrimSel*)s, hist);
        hipLaunchKernelGGL(trim_pick_kernel, dim3(nb), dim3(64), 0, st, hist, pass, keep_ratio, s);
    }
    hipLaunchKernelGGL(trim_count_kernel, grid, block, 0, st, (const float*)best, Q, chunks, (const TrimSel*)s, tie);
    hipLaunchKernelGGL(trim_mask_kernel, grid, block, 0, st, best, Q, chunks, (const TrimSel*)s, (const int32_t*)tie, idx, dist, n_within, d2_cut);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

int launch_trim_empty(int B, int32_t* n_within, float* d2_cut, hipStream_t st) {
    if (B <= 0 || (!n_within && !d2_cut)) return PCREG_OK;
    hipLaunchKernelGGL(trim_empty_kernel, dim3((B + kScanBlock - 1) / kScanBlock), dim3(kScanBlock), 0, st, B, n_within, d2_cut);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
