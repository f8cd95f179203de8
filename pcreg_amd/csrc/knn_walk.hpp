// pcreg_amd/csrc/knn_walk.hpp -- the exact tile walk of the point search, its one definition: every walk kernel is
// a prologue, walk_tiles with its lambdas, and an epilogue.  What the self-joins' prologues and lambdas have in common is here
// as well, once: the finite test, what a row is staged as (walk_row, walk_row_finite, walk_row_core), the visit rule (walk_visits), the
// "knn_stats" header (walk_count_search), tile a's box (walk_tile_box) and this thread's row (walk_self_row).  The three
// query-side kernels (knn_k.hip, knn_range.hip, knn_score.hip) share the header and still write their query prologue and visit
// rule out: docs/BENCH_NOTES.md, 2026-10-20, has why.
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
__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;       // (false for NaN)
}
// ... and as the self-joins stage it: a non-finite row is no row at all, so it is nobody's neighbour
__device__ __forceinline__ float4 walk_row_finite(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M, int r) {
    if (r < M) {
        const float x = ms[r], y = ms[r + (size_t)M], z = ms[r + 2 * (size_t)M];
        if (finite3(x, y, z)) return make_float4(x, y, z, __int_as_float(perm[r]));
    }
    return walk_no_row();
}
// ... and as DBSCAN's core walks stage it: a row with fewer than minpts neighbours is no row either.  cnt is by
// SORTED row; a non-finite row's count is 0
__device__ __forceinline__ float4 walk_row_core(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                const int32_t* __restrict__ cnt, int minpts, int r) {
    return r < M && cnt[r] >= minpts ? walk_row_finite(ms, perm, M, r) : walk_no_row();
}

// The visit rule: tile ct is scored unless DESIGN 4.1's rule (cull_rule.hpp) skips it for the box (lo xyz, hi xyz) and the
// bound D; culling switched off, or no finite D, visits every tile.
__device__ __forceinline__ bool walk_visits(const float* __restrict__ tbox, int ct, const float* box, float D, int cull) {
    return !(cull != 0 && D < INFINITY && cull_skips(cull_gap2(tbox + (size_t)ct * 6, tbox + (size_t)ct * 6 + 3, box, box + 3), D));
}

// The search header of "knn_stats" (stats or null): one search more, and the (block, tile) pairs it would visit without the rule.
// walk_tiles adds the pairs visited.
__device__ __forceinline__ void walk_count_search(unsigned long long* __restrict__ stats, unsigned long long nominal) {
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(&stats[0], 1ull);
        atomicAdd(&stats[2], nominal);
    }
}

// ---- this thread's row in a self-join ---------------------------------------------------------------------------------
// The queries are the model's own sorted rows, a culling block is tile ta and its box the tile's.  Workgroup
// (ta, part) of the kWalkWgPerTile of a tile owns sorted rows ta * kT16 + part * 64 + (tid >> 2).  A thread past the model's end
// reads row 0 and stores nothing; how its lanes are kept from admitting a row is the caller's (live, or a bound below zero).
constexpr int kWalkWgPerTile = kT16 / kWalkQPerWg;         // 8 workgroups per tile a, 64 of its rows each
struct WalkSelfRow {
    float qx, qy, qz;
    int row_i;                                             // the ORIGINAL row
    size_t sr;                                             // the sorted row (0 past the model's end)
    int rl;                                                // its place inside tile a
    bool in_model, live;                                   // live: in the model and finite
};
// tile ta's box (lo xyz, hi xyz), the self-join's culling box.  A call of its own, not a part of walk_self_row: a kernel with a
// tile bound loads the box in front of the bound's barrier and its row behind it (both in one call cost the normals 0.8 %)
__device__ __forceinline__ void walk_tile_box(const float* __restrict__ tbox, int ta, float (&box)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) box[c] = tbox[(size_t)ta * 6 + c];
}
__device__ __forceinline__ WalkSelfRow walk_self_row(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M, int ta,
                                                     int part) {
    WalkSelfRow q;
    q.rl = part * kWalkQPerWg + (int)threadIdx.x / kWalkLanes;
    const long long srow = (long long)ta * kT16 + q.rl;
    q.in_model = srow < M;
    q.sr = q.in_model ? (size_t)srow : 0;
    q.qx = ms[q.sr]; q.qy = ms[q.sr + (size_t)M]; q.qz = ms[q.sr + 2 * (size_t)M];
    q.row_i = perm[q.sr];
    q.live = q.in_model && finite3(q.qx, q.qy, q.qz);
    return q;
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
