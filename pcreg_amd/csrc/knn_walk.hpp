// pcreg_amd/csrc/knn_walk.hpp -- the exact tile walk of the point search, its one definition: knn_k_kernel,
// range_walk_kernel and cluster_walk_kernel are a prologue, walk_tiles with their four lambdas, and an epilogue.
//
// A workgroup of kBlock threads serves kWalkQPerWg queries, kWalkLanes lanes each; kWalkWgPerBlock workgroups share a culling
// block of kWalkQBlock query slots (a model tile, for the self-join) and every one of them forms the block's box for itself.
// The walk goes in rounds of kBlock candidate tiles: each thread judges one, a ballot and the per-wave counts place the visited
// ones in an ascending LDS list; then tile t + 1 of the list is fetched into registers while tile t is scored from LDS, lane
// sub of a query taking rows sub, sub + 4, ..., four rows a trip.
#pragma once
#include "knn_fast_common.hpp"

namespace pcreg {
namespace {

constexpr int kWalkLanes = 4;                              // lanes per query
constexpr int kWalkQPerWg = kBlock / kWalkLanes;           // 64 queries per workgroup
constexpr int kWalkQBlock = 512;                           // query slots per culling block (the top-2 search's unit)
constexpr int kWalkWgPerBlock = kWalkQBlock / kWalkQPerWg; // 8 workgroups per block
static_assert(kT16 % kBlock == 0 && kT16 % (4 * kWalkLanes) == 0, "tile staging and the unrolled walk");

struct WalkLds {
    float4 tile[kT16];                                     // (x, y, z, original row) of the tile being scored
    int list[kBlock];                                      // the round's visited tiles, ascending
    int wcnt[kBlock / 64];                                 // ... and how many each wave listed
};

// a row no query meets: d = NaN never passes d <= bound (padding past M; the self-join's non-finite rows)
__device__ __forceinline__ float4 walk_no_row() {
    const float qnan = __int_as_float(0x7FC00000);
    return make_float4(qnan, qnan, qnan, __int_as_float(-1));
}
// sorted row r as the walk stages it
__device__ __forceinline__ float4 walk_row(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M, int r) {
    return r < M ? make_float4(ms[r], ms[r + (size_t)M], ms[r + 2 * (size_t)M], __int_as_float(perm[r])) : walk_no_row();
}

// The box of culling block qb over ALL its queries, and with N == 7 the largest dk over them (+inf or NaN: no bound), into
// box[0 .. N): lo xyz, hi xyz, D.  Every workgroup of the block forms the same values.  One barrier inside (what the caller
// wrote to LDS before the call is visible after it); box[] itself is visible after the caller's next barrier.
template <int N>
__device__ __forceinline__ void walk_block_box(float (&red)[kBlock / 64][N], float (&box)[N], const float* __restrict__ q, int Q, int ldq,
                                               const int32_t* __restrict__ qperm, const float* __restrict__ dk, int qb) {
    static_assert(N == 6 || N == 7, "a box, or a box and a distance");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, D = 0.0f;
    for (int r = tid; r < kWalkQBlock; r += kBlock) {
        const int slot = qb * kWalkQBlock + r;
        if (slot < Q) {
            const int qi = qperm[slot];
            const float p[3] = {q[qi], q[qi + (size_t)ldq], q[qi + 2 * (size_t)ldq]};
#pragma unroll
            for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], p[c]); hi[c] = fmaxf(hi[c], p[c]); }
            if constexpr (N == 7) {
                const float e = dk[qi];
                D = e < INFINITY ? fmaxf(D, e) : INFINITY;        // +inf (or NaN): no bound, culling off for the block
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
        if constexpr (N == 7) D = fmaxf(D, __shfl_xor(D, o));
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { red[wave][c] = lo[c]; red[wave][3 + c] = hi[c]; }
        if constexpr (N == 7) red[wave][N - 1] = D;
    }
    __syncthreads();
    if (tid < N) {
        float v = red[0][tid];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) v = tid < 3 ? fminf(v, red[w][tid]) : fmaxf(v, red[w][tid]);
        box[tid] = v;
    }
}

// The walk over tiles first_tile .. n_tiles - 1 for the query (qx, qy, qz) of this thread's four lanes.
//   visit(ct)          -> bool   is tile ct < n_tiles scored?  (called once per thread and round, after a barrier)
//   row(r)             -> float4 sorted row r as it is staged, r possibly past the model's end
//   begin_tile(ct)               before tile ct of the list is scored
//   score(r, p, d)               one trip: p[u] = staged row r + 4 u of the tile, d[u] = point_d2(query, p[u]); d may be edited
//   end_tile()                   after the tile's last trip
// stats (or null): stats[1] += the tiles listed, by thread 0.
template <class Visit, class Row, class BeginTile, class Score, class EndTile>
__device__ __forceinline__ void walk_tiles(WalkLds& lds, int first_tile, int n_tiles, float qx, float qy, float qz,
                                           unsigned long long* __restrict__ stats, Visit visit, Row row, BeginTile begin_tile,
                                           Score score, EndTile end_tile) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = tid & (kWalkLanes - 1);
    for (int c0 = first_tile; c0 < n_tiles; c0 += kBlock) {
        __syncthreads();                                          // the caller's LDS written / the previous round's list consumed
        {
            const int ct = c0 + tid;
            const bool v = ct < n_tiles && visit(ct);
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(v);
            if (lane == 0) lds.wcnt[wave] = (int)__popcll(bal);
            __syncthreads();
            int base = 0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) base += w < wave ? lds.wcnt[w] : 0;
            if (v) lds.list[base + (int)__popcll(bal & ((1ull << lane) - 1ull))] = ct;
        }
        __syncthreads();
        const int ntile = lds.wcnt[0] + lds.wcnt[1] + lds.wcnt[2] + lds.wcnt[3];
        if (stats && tid == 0 && ntile > 0) atomicAdd(&stats[1], (unsigned long long)ntile);
        constexpr int kRowsPerThread = kT16 / kBlock;
        float4 pre[kRowsPerThread];
        auto fetch = [&](int t) {
            const int r0 = lds.list[t] * kT16;
#pragma unroll
            for (int u = 0; u < kRowsPerThread; ++u) pre[u] = row(r0 + u * kBlock + tid);
        };
        if (ntile > 0) fetch(0);
        for (int t = 0; t < ntile; ++t) {
            __syncthreads();                                      // the previous tile's readers are done
#pragma unroll
            for (int u = 0; u < kRowsPerThread; ++u) lds.tile[u * kBlock + tid] = pre[u];
            begin_tile(lds.list[t]);
            __syncthreads();
            if (t + 1 < ntile) fetch(t + 1);
            for (int r = sub; r < kT16; r += 4 * kWalkLanes) {
                float4 p[4]; float d[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { p[u] = lds.tile[r + u * kWalkLanes]; d[u] = point_d2(qx, qy, qz, p[u].x, p[u].y, p[u].z); }
                score(r, p, d);
            }
            end_tile();
        }
    }
}

}  // namespace
}  // namespace pcreg
