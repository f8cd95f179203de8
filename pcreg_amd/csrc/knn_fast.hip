// pcreg_amd/csrc/knn_fast.hip -- certified fast path of the fp32 3-D point search against a PREPARED model.
//
// Same contract as knn2_points_kernel (knn_points.hip): for every query the two nearest model points under
// d = fmaf(dz,dz, fmaf(dy,dy, dx*dx)), dx = q - m, ties to the lowest index -- the bits the oracle produces.
//
// The reference matches MANY surfaces against ONE model (completeExperimentFast.m:131-149,201-216), so everything that
// depends on the model alone is done once (model_prepare):
//   P1  model_bbox_partial/final_kernel   box of the model -> centre c, power-of-two scale sigma, seeding- and ordering-grid geometry
//   P2  model_order_*                     counting sort of the rows by the Morton code of their ordering-grid cell: perm, the
//                                         sorted fp32 copy the rest is built from
//   P3  prep_model_f16_kernel             sorted rows -> tiles of f16 matrix-core operands, R_m^2, and the seeding grid's cells
//   P4  tile_box_kernel                   the exact fp32 box of every tile of kT16 sorted rows
// and a search is SEVEN launches (a 128-KB memset of the query order's counters among them):
//   S1 + S1d  seed_direct_kernel   for a seeded model, both phases in one launch and one 8-lane group per query:
//     S1  (seed_body)        a first threshold per query from the model-wide seeding grid and its seed distance dk; clears
//                            the call's counters and the candidate lists; per-workgroup boxes of the queries (query grid,
//                            below); counts the queries per parent cell of the ordering grid (after the memset) and keeps
//                            each query's place inside its cell
//     S1d (direct_body)      a seeded query whose dk-box covers few ordering-grid cells with few rows is answered exactly from
//                            those cells of the sorted copy and marked (direct_rule.hpp; DESIGN 4.1, "Direct answers"); S1c
//                            and S2 do not score a marked query, S3 only enters it into the query grid.  Every workgroup
//                            leaves its (answered, rows) pair in a slot of its own; S1b sums them
//             seed_query_kernel alone runs S1 where there is no direct phase (no seeding grid, "knn_direct" = 1, "knn_stats"),
//             and seed_query_kernel + knn_direct_kernel are the same two bodies in two launches ("knn_seed_fused" = 1)
//   S1b query_order_ranked_kernel   publishes the direct phase's sums (ctr->n_direct, direct_rows) and leaves when every query
//                            has been answered; else the query SLOTS in spatial order (qperm); every workgroup derives the cell
//                            offsets it needs from the counters itself, so no scan launch sits between S1 and the slots
//   S1c knn_plan_kernel (knn_mfma16.hip)   the visit plan: per block of 512 query slots, ONCE, the box and largest dk of its
//                            scored queries and the ascending list of the model tiles they cannot rule out
//   S2  knn_candidates_f16_pipe_kernel (knn_mfma16.hip)   the scores of a block against the tiles of its plan, on the matrix
//                            cores + selection; the grid keeps W workgroups per block, W_eff = ceil(n_vis / kPlanC) (at most
//                            W) of them share the plan's positions and the others leave after one word
//   S3  knn_finalize_kernel  one 8-lane group per query: exact fmaf-chain distances of the listed candidates over the sorted
//                            copy, (distance, original index) top-2, and the CERTIFICATE: every point outside the lists has
//                            s >= G (the final threshold word), hence exact d >= G + |q~|^2 - E; proven answers are
//                            written, the others are listed; fills the query grid (a point of a skipped tile is farther
//                            than two real model points: DESIGN 4.1, culling)
//   S4  knn_tail_kernel      the listed queries again, exactly.  Few: one workgroup per query culls the tiles with the same
//                            rule against the query's own dk (the block box shrunk to a point), lists the survivors and scans
//                            them in the sorted copy, dealt over its waves, (distance, original row) order.  Many: the tiled all-pairs form over the unsorted
//                            model; a per-tile arrival counter lets the last workgroup merge, so there is no second launch.
//                            Idle (one read) when the list is empty.
// By-product: a uniform grid over the QUERIES (boxes in S1, geometry by a surplus workgroup of S2, cells in S3), which
// the Unique back-check of the match stage walks (knn_points.hip: match_finish_kernel) -- no launches of its own.
//
// S1, S1c, S3 and S4 are latency-bound (a few MB each): they issue every load of a step before they use the first -- an address
// that a condition would have guarded is clamped into the array and its value masked ("The small kernels").
//
// Rounding bound (u = 2^-24, R_m = max|m~|, r = |q~|), derived in DESIGN.md section 4.1:
//   E = u*(3 R_m^2 + 16 r R_m + 32.1 (R_m^2 + 2 r R_m) + 4.04 (r + R_m)^2) + 16 u (d2 + |G + r^2|)
#include "common.hpp"
#include "select.hpp"
#include "knn_fast_common.hpp"
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <algorithm>

namespace pcreg {

size_t knn_f16_prep_bytes(int M);
void knn_f16_shape(int Q, int M, int target_blocks, int* q_blocks, int* W);
int launch_prep_model_f16(const float* m, int M, int ldm, const void* prep, unsigned* rm2, void* mtiles, int32_t* seed_cnt,
                          void* seed_slots, hipStream_t st);
int launch_knn_candidates_f16(const float* q, int Q, int ldq, const int32_t* qperm, const float* dk, int M, const void* prep,
                              const void* mtiles, const float* tbox, const float* ubox, int cull, int32_t* n_vis, int32_t* vis_list, uint32_t* vis_mask, unsigned* gthr,
                              void* cand_ent, int32_t* cand_cnt, void* ctr, int target_blocks, bool dry, bool timed, const float* ug_part,
                              int ug_nparts, int ug_cells, void* ug_prep, int* W_out, hipStream_t st);

namespace {

// ---- P1. bounding box of the model (two-stage, deterministic) ----------------------------------------------------
__global__ __launch_bounds__(kBlock) void model_bbox_partial_kernel(const float* __restrict__ m, int M, int ldm,
                                                                    float* __restrict__ part /*[grid][6]: lo, hi*/,
                                                                    int32_t* __restrict__ zero_me, int n_zero) {
    // the seeding grid's cell counters are cleared here (saves a memset; nothing reads them before the fill)
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n_zero; i += gridDim.x * kBlock) zero_me[i] = 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < M; i += gridDim.x * kBlock) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float v = m[i + (size_t)c * ldm]; lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v); }
    }
    __shared__ float s[kBlock / 64][6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s[threadIdx.x >> 6][c] = lo[c]; s[threadIdx.x >> 6][3 + c] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = s[0][threadIdx.x];
        for (int w = 1; w < kBlock / 64; ++w) v = threadIdx.x < 3 ? fminf(v, s[w][threadIdx.x]) : fmaxf(v, s[w][threadIdx.x]);
        part[blockIdx.x * 6 + threadIdx.x] = v;
    }
}
__global__ void model_bbox_final_kernel(const float* __restrict__ part, int nparts, int M, int cell_cap, Prep* __restrict__ prep,
                                        unsigned* __restrict__ rm2_bits) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < nparts; b += 64)              // launched with one wave
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], part[b * 6 + c]); hi[c] = fmaxf(hi[c], part[b * 6 + 3 + c]); }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
    }
    if (threadIdx.x == 0) {
        prep->cx = 0.5f * lo[0] + 0.5f * hi[0]; prep->cy = 0.5f * lo[1] + 0.5f * hi[1]; prep->cz = 0.5f * lo[2] + 0.5f * hi[2];
        {   // an upper bound of max |m~|^2 from the box itself: the seeding margin uses it
            float ax = 0.5f * (hi[0] - lo[0]), ay = 0.5f * (hi[1] - lo[1]), az = 0.5f * (hi[2] - lo[2]);
            prep->rm2 = (ax * ax + ay * ay + az * az) * 1.0001f;
        }
        float H = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]) * 0.5f;
        float sg = 1.0f;
        if (H > 0.0f && H < INFINITY) sg = ldexpf(1.0f, 5 - ilogbf(H));        // sigma * H in [32, 64)
        prep->sigma = sg; prep->inv_sigma2 = 1.0f / (sg * sg);                 // powers of two: exact
        prep->pad0 = prep->pad1 = 0.0f;
        // seeding grid: cells of about two model points over the model's box plus one cell of margin on every side (a
        // query outside looks at the border cells); at most cell_cap cells
        float ext[3], emax = 0.0f;
        for (int c = 0; c < 3; ++c) { ext[c] = hi[c] - lo[c]; emax = fmaxf(emax, ext[c]); }
        int n[3] = {1, 1, 1};
        float h = 1.0f, g0[3] = {lo[0], lo[1], lo[2]};
        if (emax > 0.0f && emax < INFINITY) {
            float e2[3];
            for (int c = 0; c < 3; ++c) e2[c] = fmaxf(ext[c], emax * 1e-3f);
            h = cbrtf(e2[0] * e2[1] * e2[2] / fmaxf((float)M * 0.5f, 1.0f));
            for (int it = 0; it < 64; ++it) {
                long tot = 1;
                for (int c = 0; c < 3; ++c) {
                    g0[c] = lo[c] - h;
                    n[c] = (int)fminf(ceilf(ext[c] / h) + 2.0f, 2048.0f); if (n[c] < 1) n[c] = 1; tot *= n[c];
                }
                if (tot <= cell_cap) break;
                h *= 1.2f;
            }
            if ((long)n[0] * n[1] * n[2] > cell_cap) { n[0] = n[1] = n[2] = 1; g0[0] = lo[0]; g0[1] = lo[1]; g0[2] = lo[2]; h = emax * 2.0f; }
        }
        prep->gx0 = g0[0]; prep->gy0 = g0[1]; prep->gz0 = g0[2]; prep->inv_h = 1.0f / h;
        prep->nx = n[0]; prep->ny = n[1]; prep->nz = n[2]; prep->ncell = n[0] * n[1] * n[2];
        // ordering grid: cubic cells, 2^kSortBits along the longest side (a flat axis gets fewer)
        prep->sx0 = lo[0]; prep->sy0 = lo[1]; prep->sz0 = lo[2];
        prep->inv_s = (emax > 0.0f && emax < INFINITY) ? (float)(1 << kSortBits) / emax : 0.0f;
        *rm2_bits = 0u;
    }
}

// ---- P2 / S1b. counting sort by ordering-grid cell (as descriptors.hip builds its grid: count, scan, scatter) -------
// The scatter takes places inside a cell by atomics, so the order inside a cell varies from run to run; nothing but the
// set of tiles a query block visits depends on it (ties are ordered by ORIGINAL row: knn_finalize_kernel).
__global__ __launch_bounds__(kBlock) void model_order_count_kernel(const float* __restrict__ m, int M, int ldm, const Prep* __restrict__ prep,
                                                                   int32_t* __restrict__ cnt) {
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < M; i += gridDim.x * kBlock)
        atomicAdd(&cnt[sort_key(m[i], m[i + (size_t)ldm], m[i + 2 * (size_t)ldm], prep)], 1);
}
// in place, ONE workgroup of 1024: thread t owns n / 1024 consecutive counters (n a multiple of 4096)
__global__ __launch_bounds__(1024) void exclusive_scan_1wg_kernel(int32_t* __restrict__ a, int n) {
    __shared__ int s_w[16];
    const int per4 = n / 4096, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int4* p = (int4*)a + (size_t)threadIdx.x * per4;
    int sum = 0;
#pragma unroll 8
    for (int k = 0; k < per4; ++k) { const int4 v = p[k]; sum += v.x + v.y + v.z + v.w; }      // eight loads in flight
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o); if (lane >= o) inc += y; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int run = inc - sum;
    for (int k = 0; k < wave; ++k) run += s_w[k];
#pragma unroll 8
    for (int k = 0; k < per4; ++k) {
        const int4 v = p[k];
        int4 o;
        o.x = run; run += v.x; o.y = run; run += v.y; o.z = run; run += v.z; o.w = run; run += v.w;
        p[k] = o;
    }
}
__global__ __launch_bounds__(kBlock) void model_order_scatter_kernel(const float* __restrict__ m, int M, int ldm, const Prep* __restrict__ prep,
                                                                     int32_t* __restrict__ off, int32_t* __restrict__ perm, float* __restrict__ ms) {
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < M; i += gridDim.x * kBlock) {
        const float x = m[i], y = m[i + (size_t)ldm], z = m[i + 2 * (size_t)ldm];
        const int d = atomicAdd(&off[sort_key(x, y, z, prep)], 1);
        perm[d] = i; ms[d] = x; ms[d + (size_t)M] = y; ms[d + 2 * (size_t)M] = z;
    }
}
// P4: the exact box of each tile of kT16 sorted rows (padding rows excluded), and of each of its UNITS of 64 consecutive rows
// (ubox [n_tiles * kT16 / 64][6]; a partly filled unit's box covers its existing rows, an empty one holds (+inf, -inf): the
// unit rule of knn_plan_kernel never keeps it); one workgroup per tile, a wave's pass over 64 rows is one unit
__global__ __launch_bounds__(kBlock) void tile_box_kernel(const float* __restrict__ ms, int M, float* __restrict__ tbox, float* __restrict__ ubox) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int r = threadIdx.x; r < kT16; r += kBlock) {
        const int i = blockIdx.x * kT16 + r;
        float ulo[3] = {INFINITY, INFINITY, INFINITY}, uhi[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (i < M) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { ulo[c] = uhi[c] = ms[i + (size_t)c * M]; lo[c] = fminf(lo[c], ulo[c]); hi[c] = fmaxf(hi[c], uhi[c]); }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { ulo[c] = fminf(ulo[c], __shfl_xor(ulo[c], o)); uhi[c] = fmaxf(uhi[c], __shfl_xor(uhi[c], o)); }
        }
        if ((threadIdx.x & 63) == 0) {
            float* ub = ubox + ((size_t)blockIdx.x * (kT16 / 64) + (size_t)(r >> 6)) * 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) { ub[c] = ulo[c]; ub[3 + c] = uhi[c]; }
        }
    }
    __shared__ float s[kBlock / 64][6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s[threadIdx.x >> 6][c] = lo[c]; s[threadIdx.x >> 6][3 + c] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = s[0][threadIdx.x];
        for (int w = 1; w < kBlock / 64; ++w) v = threadIdx.x < 3 ? fminf(v, s[w][threadIdx.x]) : fmaxf(v, s[w][threadIdx.x]);
        tbox[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
}
// S1b: query slot of every query (the counts come from seed_query_kernel, scanned in place)
__global__ __launch_bounds__(kBlock) void query_order_kernel(const float* __restrict__ q, int Q, int ldq, const Prep* __restrict__ prep,
                                                             int32_t* __restrict__ off, int32_t* __restrict__ qperm) {
    const int qi = blockIdx.x * kBlock + threadIdx.x;
    if (qi >= Q) return;
    const int key = sort_key(q[qi], q[qi + (size_t)ldq], q[qi + 2 * (size_t)ldq], prep) >> 3;
    qperm[atomicAdd(&off[key], 1)] = qi;
}

// S1b of the two-nearest search in ONE launch, without a scan on the critical path: cnt holds the per-parent-cell counts and
// rank each query's place inside its cell (both from seed_query_kernel).  Every workgroup sums all kQueryKeys counters
// itself (L2-resident, 128 per thread) and keeps the exclusive offsets of every 16th in LDS; a query adds the at most 15
// counters in front of its own cell's.  No atomics: cnt is only read.
//
// The direct answers' count is summed here as well.  The workgroups of the direct phase (direct_body, below) leave their
// (answered, rows) pairs in dparts [nparts] with plain stores -- null when no direct phase ran: nothing was answered -- and
// this launch is the first one after them: workgroup 0 publishes the two sums in ctr->n_direct / ctr->direct_rows, where
// knn_plan_kernel, knn_direct_stats_kernel and the tests read them as before.  When every query has been answered nobody
// reads qperm in this call and the kernel leaves before it sums a counter.  The readers of qperm, all in
// launch_model_search: knn_plan_kernel (leaves on n_direct == Q before its first qperm read), knn_candidates_f16_pipe_kernel
// (reads n_vis[qb] = 0 first and leaves; its surplus workgroup reads ug_part only), and nobody else -- knn_finalize_kernel
// and knn_tail_kernel take no qperm.  search_export (a test hook) then copies the slots of an earlier call.
// Every workgroup forms the sum itself while the pairs are few (kDirectPartsAll: 16 KB, an eighth of the counters it would
// sum otherwise); beyond that only workgroup 0 does, and the others write their slots as if somebody read them.
constexpr int kDirectPartsAll = 2048;
__global__ __launch_bounds__(kBlock) void query_order_ranked_kernel(const float* __restrict__ q, int Q, int ldq, const Prep* __restrict__ prep,
                                                                    const int32_t* __restrict__ cnt, const int32_t* __restrict__ rank,
                                                                    int32_t* __restrict__ qperm, const int2* __restrict__ dparts, int nparts,
                                                                    SearchCounters* __restrict__ ctr) {
    constexpr int kPer = kQueryKeys / kBlock, kSub = kPer / 16;
    static_assert(kQueryKeys % (kBlock * 16) == 0, "every thread owns whole groups of 16 counters");
    __shared__ int s_sub[kQueryKeys / 16], s_w[kBlock / 64];
    __shared__ int s_dir[kBlock / 64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (dparts != nullptr && (nparts <= kDirectPartsAll || blockIdx.x == 0)) {
        int nd = 0, nr = 0;
        for (int i = threadIdx.x; i < nparts; i += kBlock) { const int2 v = dparts[i]; nd += v.x; nr += v.y; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { nd += __shfl_xor(nd, o); nr += __shfl_xor(nr, o); }
        if (lane == 0) { s_dir[wave][0] = nd; s_dir[wave][1] = nr; }
        __syncthreads();
        nd = 0; nr = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) { nd += s_dir[w][0]; nr += s_dir[w][1]; }
        if (blockIdx.x == 0 && threadIdx.x == 0) { ctr->n_direct = nd; ctr->direct_rows = nr; }
        if (nparts <= kDirectPartsAll && nd == Q) return;
    }
    const int4* p = (const int4*)cnt + (size_t)threadIdx.x * (kPer / 4);
    int sub[kSub], sum = 0;
#pragma unroll
    for (int j = 0; j < kSub; ++j) {
        const int4 a = p[4 * j], b = p[4 * j + 1], c = p[4 * j + 2], d = p[4 * j + 3];
        sub[j] = sum;
        sum += (a.x + a.y + a.z + a.w) + (b.x + b.y + b.z + b.w) + (c.x + c.y + c.z + c.w) + (d.x + d.y + d.z + d.w);
    }
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o); if (lane >= o) inc += y; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int run = inc - sum;
    for (int k = 0; k < wave; ++k) run += s_w[k];
#pragma unroll
    for (int j = 0; j < kSub; ++j) s_sub[threadIdx.x * kSub + j] = run + sub[j];
    __syncthreads();
    const int qi = blockIdx.x * kBlock + threadIdx.x;
    if (qi >= Q) return;
    const int key = sort_key(q[qi], q[qi + (size_t)ldq], q[qi + 2 * (size_t)ldq], prep) >> 3;
    const int4* f = (const int4*)cnt + (size_t)(key >> 4) * 4;
    const int r = key & 15;
    int off = s_sub[key >> 4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int4 v = f[i];
        off += (4 * i < r ? v.x : 0) + (4 * i + 1 < r ? v.y : 0) + (4 * i + 2 < r ? v.z : 0) + (4 * i + 3 < r ? v.w : 0);
    }
    qperm[off + rank[qi]] = qi;
}

// ---- S1. seeding: a first threshold per query from the model-wide grid ------------------------------------------
// The candidate kernel only touches its sorted lists when a score beats the query's threshold, and a wave pays that
// slow path whenever ANY of its lanes does.  Starting from +inf every lane does so O(log n) times; starting from "the
// k-th nearest of a few model points around the query" (k = kSeedRank = 2) almost never.  The grid remembers up to kSeedSlots points per
// cell (whoever arrived first: the threshold is a hint, results never depend on it); a query looks at the 27 cells
// around its own (clamped into the grid: any model point's exact distance is a valid upper bound), takes the
// k-th smallest EXACT distance dk and publishes the s-space threshold dk - |q~|^2 plus twice the score error bound, so
// that its true k nearest are still below it.  Every point that is later skipped was compared with a word >= the
// final word G, which is all the certificate needs.
__device__ __forceinline__ int seed_cell(float v, float lo, float inv_h, int n) {
    int c = (int)floorf((v - lo) * inv_h);
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
}
// eight lanes per query, two quads: in round r the quads look at cells 2r and 2r + 1 of the 27, and lane k of a quad at slot
// k of its quad's cell, so the four slots of a cell (one 64-byte line) arrive through ONE load instruction of four adjacent
// lanes and a wave's load touches 16 lines, not 64.  14 rounds (the last with one live cell), one distance per lane and
// round, every (cell, slot) pair exactly once; a lane keeps its own sorted four smallest distances, and three xor-shuffle
// rounds merge the eight lists.
constexpr int kSeedRounds = (27 + 1) / 2;
__host__ __device__ constexpr int seed_offsets(int c27) { return (c27 % 3) | (((c27 / 3) % 3) << 2) | ((c27 / 9) << 4); }
constexpr int kSeedBatch = 7;     // rounds whose counters and slots are loaded before the first is used (64 VGPRs: the kernel is
                                  // pinned to eight waves per SIMD, one residency round)
static_assert(kSeedSlots == 4 && kSeedRounds % kSeedBatch == 0, "a quad per cell, the rounds in whole batches");
__device__ __forceinline__ void sort4(float (&d)[4]) {
#define PCREG_CS(a, b) { const float lo_ = fminf(d[a], d[b]), hi_ = fmaxf(d[a], d[b]); d[a] = lo_; d[b] = hi_; }
    PCREG_CS(0, 1) PCREG_CS(2, 3) PCREG_CS(0, 2) PCREG_CS(1, 3) PCREG_CS(1, 2)
#undef PCREG_CS
}
// The body of S1, for its two callers: seed_query_kernel (kFused = false) and seed_direct_kernel (kFused = true), which goes
// on to the direct phase in the same group.  After the xor-shuffle merge every lane of a group holds the same d[], so the
// group's eight lanes all return the query, its seed distance dk and (lane 0) its place in its cell; nothing is read
// again.  Lane 0 stores gthr and dk_out here; with kFused the caller stores the two words that wait for the direct phase:
// cand_cnt (once: the mark or 0) and the place, whose atomic is issued first and consumed last.
struct SeedOut { float qx, qy, qz, dk; int qi, rank; bool live; };
template <bool kFused>
__device__ __forceinline__ SeedOut seed_body(const float* __restrict__ q, int Q, int ldq,
                                             const Prep* __restrict__ prep, const int32_t* __restrict__ cnt,
                                             const float4* __restrict__ slots, int seeded, unsigned* __restrict__ gthr,
                                             int32_t* __restrict__ cand_cnt, SearchCounters* __restrict__ ctr,
                                             float* __restrict__ ug_part, int32_t* __restrict__ ug_cnt, int ug_cells,
                                             float* __restrict__ dk_out, int32_t* __restrict__ qcnt, int32_t* __restrict__ qrank) {
    // housekeeping for the launches that follow
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < (int)(sizeof(SearchCounters) / 4); i += gridDim.x * kBlock) ((int32_t*)ctr)[i] = 0;
    if (ug_cnt) for (int i = blockIdx.x * kBlock + threadIdx.x; i < ug_cells; i += gridDim.x * kBlock) ug_cnt[i] = 0;
    const int qi = (blockIdx.x * kBlock + threadIdx.x) >> 3, sub = threadIdx.x & 7;
    const bool live = qi < Q;
    const int qq = live ? qi : 0;
    const float qx = q[qq], qy = q[qq + (size_t)ldq], qz = q[qq + 2 * (size_t)ldq];
    SeedOut out{qx, qy, qz, INFINITY, qi, 0, live};
    if (ug_part) {                  // box of this workgroup's queries (the query grid's geometry follows from all of them)
        __shared__ float s_box[kBlock / 64][6];
        float v[6] = {live ? qx : INFINITY, live ? qy : INFINITY, live ? qz : INFINITY, live ? qx : -INFINITY, live ? qy : -INFINITY, live ? qz : -INFINITY};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { v[c] = fminf(v[c], __shfl_xor(v[c], o)); v[3 + c] = fmaxf(v[3 + c], __shfl_xor(v[3 + c], o)); }
        }
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int c = 0; c < 6; ++c) s_box[threadIdx.x >> 6][c] = v[c];
        }
        __syncthreads();
        if (threadIdx.x < 6) {
            float r = s_box[0][threadIdx.x];
            for (int w = 1; w < kBlock / 64; ++w) r = threadIdx.x < 3 ? fminf(r, s_box[w][threadIdx.x]) : fmaxf(r, s_box[w][threadIdx.x]);
            ug_part[(size_t)blockIdx.x * 6 + threadIdx.x] = r;
        }
    }
    if (!seeded) {                                            // +inf: no hint
        if (live && sub == 0) {
            cand_cnt[qi] = 0; gthr[qi] = 0xFFFFFFFFu; dk_out[qi] = INFINITY;
            if (qcnt) qrank[qi] = atomicAdd(&qcnt[sort_key(qx, qy, qz, prep) >> 3], 1);
        }
        return out;
    }
    const int nx = prep->nx, ny = prep->ny, nz = prep->nz;
    const int cx = seed_cell(qx, prep->gx0, prep->inv_h, nx), cy = seed_cell(qy, prep->gy0, prep->inv_h, ny), cz = seed_cell(qz, prep->gz0, prep->inv_h, nz);
    // The quad's cell of every round first, in straight-line code (an excluded one -- past the 27, or outside the grid --
    // reads the query's own cell and counts as empty), then the counting atomic, then kSeedBatch rounds at a time: the
    // cells' counters (one address for the quad) and the lane's slots with nothing consumed in between.
    const int quad = sub >> 2, slot = sub & 3, own = (cz * ny + cy) * nx + cx;
    int cell[kSeedRounds]; unsigned on = 0;
#pragma unroll
    for (int r = 0; r < kSeedRounds; ++r) {
        const int a = 2 * r, b = a + 1;                       // the two quads' cells of this round: compile-time numbers, their
        const int o = quad ? seed_offsets(b) : seed_offsets(a);     // offsets in the 3 x 3 x 3 block as one literal each
        const int x = cx + (o & 3) - 1, y = cy + ((o >> 2) & 3) - 1, z = cz + (o >> 4) - 1;
        const bool ok = (b < 27 || !quad) & ((unsigned)x < (unsigned)nx) & ((unsigned)y < (unsigned)ny) & ((unsigned)z < (unsigned)nz);
        cell[r] = ok ? (z * ny + y) * nx + x : own;
        on |= (unsigned)ok << r;
    }
    // The query order's counts and this query's place in its cell.  The place is stored at the very end: nothing before
    // needs it, so the atomic's round trip runs alongside the grid loads.  (The query's coordinates are consumed above:
    // no wait for them can fall behind the atomic and wait for it too.)
    const int key = sort_key(qx, qy, qz, prep) >> 3;
    int rank = 0;
    if (live && sub == 0) {
        if (!kFused) cand_cnt[qi] = 0;                        // the query's candidate list starts empty
        if (qcnt) rank = atomicAdd(&qcnt[key], 1);
    }
    float d[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
#pragma unroll
    for (int r0 = 0; r0 < kSeedRounds; r0 += kSeedBatch) {
        int n[kSeedBatch]; float4 pp[kSeedBatch];
#pragma unroll
        for (int t = 0; t < kSeedBatch; ++t) n[t] = cnt[cell[r0 + t]];
#pragma unroll
        for (int t = 0; t < kSeedBatch; ++t) pp[t] = slots[(size_t)cell[r0 + t] * kSeedSlots + slot];
#pragma unroll
        for (int t = 0; t < kSeedBatch; ++t) {
            const float ex = qx - pp[t].x, ey = qy - pp[t].y, ez = qz - pp[t].z;
            const float dd = __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
            // sorted insertion in straight-line code; a distance that does not count (a NaN among them) enters as +inf
            const bool counts = ((on >> (r0 + t)) & 1) & (slot < min(n[t], kSeedSlots)) & (dd < d[3]);      // (&: no branch to sink a load into)
            float c = counts ? dd : INFINITY;
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float lo = fminf(d[k], c); c = fmaxf(d[k], c); d[k] = lo; }
        }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {               // the four smallest of two sorted fours: min(a_i, b_{3-i}), then sort
        float e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = __shfl_xor(d[k], o);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = fminf(d[k], e[3 - k]);
        sort4(d);
    }
    // The k-th smallest exact distance of the sample bounds the true k-th nearest distance from above; any rank >= 2 keeps
    // both true neighbours under the threshold (kSeedRank = 2 since round 3).
    const float dk = d[kSeedRank - 1];
    out.dk = dk; out.rank = rank;
    if (!live || sub != 0) return out;
    unsigned word = 0xFFFFFFFFu;                           // +inf: no hint
    if (dk < INFINITY) {
        const float tx = qx - prep->cx, ty = qy - prep->cy, tz = qz - prep->cz;
        const double r2 = (double)tx * tx + (double)ty * ty + (double)tz * tz;
        const double E = score_error_bound(1, (double)prep->rm2, sqrt(r2));
        const double u = 5.9604644775390625e-08;
        const double t = (double)dk - r2 + 2.0 * E + 16.0 * u * ((double)dk + fabs((double)dk - r2));
        word = f2ord(nextafterf((float)t, INFINITY));
    }
    gthr[qi] = word;
    dk_out[qi] = dk;                   // the distance itself: two real model points lie within dk of the query (culling)
    if (!kFused && qcnt) qrank[qi] = rank;
    return out;
}
__global__ __launch_bounds__(kBlock, 8) void seed_query_kernel(const float* __restrict__ q, int Q, int ldq,
                                                            const Prep* __restrict__ prep, const int32_t* __restrict__ cnt,
                                                            const float4* __restrict__ slots, int seeded, unsigned* __restrict__ gthr,
                                                            int32_t* __restrict__ cand_cnt, SearchCounters* __restrict__ ctr,
                                                            float* __restrict__ ug_part, int32_t* __restrict__ ug_cnt, int ug_cells,
                                                            float* __restrict__ dk_out, int32_t* __restrict__ qcnt, int32_t* __restrict__ qrank) {
    (void)seed_body<false>(q, Q, ldq, prep, cnt, slots, seeded, gthr, cand_cnt, ctr, ug_part, ug_cnt, ug_cells, dk_out, qcnt, qrank);
}

// ---- S3. exact re-rank + certificate: one 8-lane group per query --------------------------------------------------
__device__ __forceinline__ bool lex_lt_f(float da, int ia, float db, int ib) {
    return da < db || (da == db && (unsigned)ia < (unsigned)ib);
}
// A list entry is (first sorted row jb, minimum score) of the 16 model points jb + 8 (r / 4) + r % 4, r = 0..15, that one
// lane of knn_candidates_f16_pipe_kernel scored together; pass 2 expands every entry that can still matter over the
// sorted copy ms (ld = M) and ranks by (distance, ORIGINAL row perm[jj]), so the lowest-row tie rule holds whatever tile
// a point was sorted into.  Points past M (tile padding) are skipped.  A query's list: cand_cnt[qi] entries at
// ent[(size_t)qi * cap + e].
constexpr int LPQ = 8;
// A lane keeps its first kOwnEnt entries (e = lane, lane + LPQ, ..: the first LPQ * kOwnEnt of the list) in registers for both
// passes, all loaded before the first is used; a longer list (cap = W * KC reaches 320) goes on in a loop that reads one entry
// per lane and trip.  Pass 2 is the GROUP's work: every lane flags which of its entries survive the cut, and the group walks
// the flagged entries of a trip (an 8-bit slice of a ballot) kEntBatch at a time, the wave as long as its longest group.  The
// owner's first row j is broadcast and lane r ranks rows rr = r and rr = r + 8 of the sixteen, so lanes 0-3 and 4-7 read
// the four-row runs j .., j + 8 .. (and j + 16 .., j + 24 ..) as 16 contiguous bytes each: eight loads per lane and entry,
// all issued before the first compare.  A row past M reads row M - 1 instead and is left out of the ranking, so no load
// leaves ms[0 .. 3M) or perm[0 .. M); the plain loads need no alignment of M.  Every lane keeps its own top two; (distance,
// original row) is a total order over distinct rows, so the group reduction's result does not depend on who saw which row.
constexpr int kOwnEnt = 8;                       // (tests/test_gpu_knn_chains.py builds lists beyond 128 entries: keep LPQ * kOwnEnt below)
constexpr int kEntBatch = 1;                      // flagged entries of a group whose rows are loaded before the first is ranked (2: 71 VGPRs,
                                                  // 13.6 us against 13.0, docs/BENCH_NOTES.md 2026-10-20)
__device__ __forceinline__ void expand_flagged(unsigned flagged, int j_own, int lane, float qx, float qy, float qz,
                                               const float* __restrict__ ms, int M, const int32_t* __restrict__ perm,
                                               float& d1, float& d2, int& i1, int& i2) {
    // `flagged`: the group's lanes whose entry of this trip (first row j_own) is to be expanded; the same word in all eight
    const int r0 = 8 * (lane >> 2) + (lane & 3);                // row rr = lane of an entry; rr = lane + 8 is 16 rows on
    while (flagged) {
        int j[kEntBatch]; bool have[kEntBatch];
        float x[kEntBatch][2], y[kEntBatch][2], z[kEntBatch][2]; int oj[kEntBatch][2];
#pragma unroll
        for (int t = 0; t < kEntBatch; ++t) {                 // (past the last flagged entry: the first one again, masked)
            have[t] = flagged != 0;
            const int owner = have[t] ? __builtin_ctz(flagged) : 0;
            flagged &= flagged - 1;
            j[t] = __shfl(j_own, owner, LPQ);
            if (t > 0 && !have[t]) j[t] = j[0];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int jj = min(j[t] + r0 + 16 * h, M - 1);
                x[t][h] = ms[jj]; y[t][h] = ms[jj + (size_t)M]; z[t][h] = ms[jj + 2 * (size_t)M]; oj[t][h] = perm[jj];
            }
        }
#pragma unroll
        for (int t = 0; t < kEntBatch; ++t) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float d = point_d2(qx, qy, qz, x[t][h], y[t][h], z[t][h]);
                const bool in2 = have[t] && j[t] + r0 + 16 * h < M && lex_lt_f(d, oj[t][h], d2, i2), in1 = in2 && lex_lt_f(d, oj[t][h], d1, i1);
                d2 = in1 ? d1 : (in2 ? d : d2); i2 = in1 ? i1 : (in2 ? oj[t][h] : i2);      // (selects: straight-line code)
                d1 = in1 ? d : d1; i1 = in1 ? oj[t][h] : i1;
            }
        }
    }
}
// the group's 8-bit slice of a wave's ballot
__device__ __forceinline__ unsigned group_flags(bool f) {
    return (unsigned)(__ballot(f) >> (threadIdx.x & 63 & ~(LPQ - 1))) & ((1u << LPQ) - 1);
}
// group-shuffle top-2 reduction of the LPQ lanes' sorted pairs, ordered by (dist, idx); empty slots are (+inf, -1 -> max uint)
__device__ __forceinline__ void group_top2_merge(float& d1, float& d2, int& i1, int& i2) {
#pragma unroll
    for (int o = LPQ / 2; o > 0; o >>= 1) {
        float e1 = __shfl_xor(d1, o), e2 = __shfl_xor(d2, o);
        int j1 = __shfl_xor(i1, o), j2 = __shfl_xor(i2, o);
        // merge two sorted pairs
        bool first_mine = lex_lt_f(d1, i1, e1, j1);
        float w1 = first_mine ? d1 : e1; int k1 = first_mine ? i1 : j1;
        float x2 = first_mine ? d2 : d1; int y2 = first_mine ? i2 : i1;      // my next
        float x3 = first_mine ? e1 : e2; int y3 = first_mine ? j1 : j2;      // other's next
        bool sec_mine = lex_lt_f(x2, y2, x3, y3);
        d1 = w1; i1 = k1; d2 = sec_mine ? x2 : x3; i2 = sec_mine ? y2 : y3;
    }
}

// ---- S1d. direct answers: one 8-lane group per seeded query ("Direct answers") ------------------------
// The rule of direct_rule.hpp: every row within the query's seed distance dk lies in the box of ordering-grid cells
// [cell(q - rho), cell(q + rho)], so the top two by (distance, original row) over those cells' rows are the search's answer.
// sort_cnt[key] is the END row of cell `key` in the sorted copy (the counting sort leaves it so; its start is the end of
// key - 1).  A group whose range holds more than kDirectCells cells, or whose cells hold more than kDirectRows rows, or
// whose query has no finite dk or coordinates, writes nothing: the verdict is the group's, formed before any store.
// Lane l owns cells l, l + 8, .. of the range (x fastest); all their counters are loaded before the first is used.  The cells'
// rows, concatenated in cell order, are dealt over the lanes -- row r of the concatenation to lane r % 8 -- kDirectBatch
// per lane and trip, every load of a trip (x, y, z, perm) issued before the first compare; a row past the end reads the
// first row of the range and is masked.  The (start, end) table of a group's cells lives in LDS.
constexpr int kDirectBatch = 4;
constexpr int kDirectSlots = (kDirectCells + LPQ - 1) / LPQ;              // cells per lane
// The body of S1d, for its two callers: knn_direct_kernel reads the query qi = blockIdx.x * (kBlock / LPQ) + group and its
// seed distance D back from memory, seed_direct_kernel (kFused = true) hands them over in registers.  With kFused the
// query's cand_cnt word is stored here once, the mark or 0; otherwise seed_query_kernel has stored the 0.  A workgroup
// leaves its (answered, rows) pair in parts[blockIdx.x] with a plain store, whatever the slot held: the sums are formed by
// the next launch (query_order_ranked_kernel), so no counter of this launch is cleared and added to by different workgroups.
template <bool kFused>
__device__ __forceinline__ void direct_body(
    int qi, bool live, float qx, float qy, float qz, float D, const Prep* __restrict__ prep,
    const int32_t* __restrict__ sort_cnt, const float* __restrict__ ms, int M, const int32_t* __restrict__ perm, int idx_base,
    int32_t* __restrict__ idx, float* __restrict__ dist, int32_t* __restrict__ cand_cnt, int2* __restrict__ parts) {
    constexpr int kGroups = kBlock / LPQ, kTab = LPQ * kDirectSlots;
    __shared__ int s_end[kGroups][kTab], s_off[kGroups][kTab];          // per cell: end in the concatenation, sorted row - position
    __shared__ int s_n[2];
    const int lane = threadIdx.x & (LPQ - 1), grp = threadIdx.x / LPQ;
    if (threadIdx.x < 2) s_n[threadIdx.x] = 0;
    const float qv[3] = {qx, qy, qz}, s0[3] = {prep->sx0, prep->sy0, prep->sz0};
    DirectRange R;
    bool ok = direct_range(qv, D, s0, prep->inv_s, (1 << kSortBits) - 1, &R) && live;
    if (!ok) { for (int c = 0; c < 3; ++c) R.lo[c] = R.hi[c] = 0; }
    const int nx = R.hi[0] - R.lo[0] + 1, ny = R.hi[1] - R.lo[1] + 1;
    const int ncell = direct_cells(R);
    ok = ok && ncell <= kDirectCells;
    // the ends of the lane's cells and of the cells in front of them (key 0 has none: masked)
    int e0[kDirectSlots], e1[kDirectSlots]; bool has[kDirectSlots], first[kDirectSlots];
#pragma unroll
    for (int k = 0; k < kDirectSlots; ++k) {
        const int c = lane + LPQ * k;
        has[k] = ok && c < ncell;
        const int cc = has[k] ? c : 0;
        const int ix = R.lo[0] + cc % nx, iy = R.lo[1] + (cc / nx) % ny, iz = R.lo[2] + cc / (nx * ny);
        const int key = (int)(morton_spread((unsigned)ix) | (morton_spread((unsigned)iy) << 1) | (morton_spread((unsigned)iz) << 2));
        first[k] = key == 0;
        e0[k] = sort_cnt[max(key - 1, 0)]; e1[k] = sort_cnt[key];
    }
    // the concatenation's prefix over the cells in order c = lane + 8 k: a group scan per slot, the carry across slots
    int total = 0;
#pragma unroll
    for (int k = 0; k < kDirectSlots; ++k) {
        const int start = first[k] ? 0 : e0[k], n = has[k] ? max(e1[k] - start, 0) : 0;
        int inc = n;
#pragma unroll
        for (int o = 1; o < LPQ; o <<= 1) { const int y = __shfl_up(inc, o, LPQ); if (lane >= o) inc += y; }
        const int end = total + inc;
        s_end[grp][lane + LPQ * k] = end;
        s_off[grp][lane + LPQ * k] = start - (end - n);
        total += __shfl(inc, LPQ - 1, LPQ);
    }
    ok = ok && total <= kDirectRows;                      // the group's verdict: total is the same in its eight lanes
    const int rows = ok ? total : 0;
    __syncthreads();                                      // the tables (and the block's two counters, cleared above)
    float d1 = INFINITY, d2 = INFINITY; int i1 = -1, i2 = -1;
    int c = 0;                                            // the cell of the lane's current row: it only moves forward
    for (int r0 = 0; r0 < rows; r0 += LPQ * kDirectBatch) {
        float x[kDirectBatch], y[kDirectBatch], z[kDirectBatch]; int oj[kDirectBatch]; bool in[kDirectBatch];
#pragma unroll
        for (int t = 0; t < kDirectBatch; ++t) {
            const int r = r0 + LPQ * t + lane;
            in[t] = r < rows;
            const int rr = in[t] ? r : 0;
            if (in[t]) while (c < ncell - 1 && rr >= s_end[grp][c]) ++c;
            const int row = min(max(rr + s_off[grp][in[t] ? c : 0], 0), M - 1);
            x[t] = ms[row]; y[t] = ms[row + (size_t)M]; z[t] = ms[row + 2 * (size_t)M]; oj[t] = perm[row];
        }
#pragma unroll
        for (int t = 0; t < kDirectBatch; ++t) {
            const float d = point_d2(qx, qy, qz, x[t], y[t], z[t]);
            const bool in2 = in[t] && lex_lt_f(d, oj[t], d2, i2), in1 = in2 && lex_lt_f(d, oj[t], d1, i1);
            d2 = in1 ? d1 : (in2 ? d : d2); i2 = in1 ? i1 : (in2 ? oj[t] : i2);      // (selects: straight-line code)
            d1 = in1 ? d : d1; i1 = in1 ? oj[t] : i1;
        }
    }
    group_top2_merge(d1, d2, i1, i2);
    // Two real rows lie within dk, so both answers exist; were a prepared block ever inconsistent with that, the query would
    // simply take the walk.
    ok = ok && i2 >= 0;
    if (ok && lane == 0) {
        idx[(size_t)qi * 2] = i1 + idx_base; idx[(size_t)qi * 2 + 1] = i2 + idx_base;
        dist[(size_t)qi * 2] = d1; dist[(size_t)qi * 2 + 1] = d2;
        if (!kFused) cand_cnt[qi] = kDirectMark;
        atomicAdd(&s_n[0], 1); atomicAdd(&s_n[1], rows);
    }
    if (kFused && live && lane == 0) cand_cnt[qi] = ok ? kDirectMark : 0;
    __syncthreads();
    if (threadIdx.x == 0) parts[blockIdx.x] = make_int2(s_n[0], s_n[1]);
}
__global__ __launch_bounds__(kBlock) void knn_direct_kernel(
    const float* __restrict__ q, int Q, int ldq, const float* __restrict__ dk, const Prep* __restrict__ prep,
    const int32_t* __restrict__ sort_cnt, const float* __restrict__ ms, int M, const int32_t* __restrict__ perm, int idx_base,
    int32_t* __restrict__ idx, float* __restrict__ dist, int32_t* __restrict__ cand_cnt, int2* __restrict__ parts) {
    const int qi = blockIdx.x * (kBlock / LPQ) + threadIdx.x / LPQ;
    const bool live = qi < Q;
    const int qq = live ? qi : 0;
    direct_body<false>(qi, live, q[qq], q[qq + (size_t)ldq], q[qq + 2 * (size_t)ldq], dk[qq], prep, sort_cnt, ms, M, perm, idx_base, idx, dist,
                       cand_cnt, parts);
}
// S1 + S1d in ONE launch, for a seeded model: the seed phase and then, in the same group with the query and dk still in
// registers, the direct phase.  Same geometry as either kernel alone (one 8-lane group per query, grid ceil(8 Q / kBlock));
// same stores, same bits ("knn_seed_fused" = 1 runs the two launches instead: the A/B of one binary).
__global__ __launch_bounds__(kBlock, 8) void seed_direct_kernel(
    const float* __restrict__ q, int Q, int ldq, const Prep* __restrict__ prep, const int32_t* __restrict__ cnt,
    const float4* __restrict__ slots, unsigned* __restrict__ gthr, int32_t* __restrict__ cand_cnt, SearchCounters* __restrict__ ctr,
    float* __restrict__ ug_part, int32_t* __restrict__ ug_cnt, int ug_cells, float* __restrict__ dk_out, int32_t* __restrict__ qcnt,
    int32_t* __restrict__ qrank, const int32_t* __restrict__ sort_cnt, const float* __restrict__ ms, int M,
    const int32_t* __restrict__ perm, int idx_base, int32_t* __restrict__ idx, float* __restrict__ dist, int2* __restrict__ parts) {
    const SeedOut s = seed_body<true>(q, Q, ldq, prep, cnt, slots, 1, gthr, cand_cnt, ctr, ug_part, ug_cnt, ug_cells, dk_out, qcnt, qrank);
    direct_body<true>(s.qi, s.live, s.qx, s.qy, s.qz, s.dk, prep, sort_cnt, ms, M, perm, idx_base, idx, dist, cand_cnt, parts);
    if (s.live && (threadIdx.x & (LPQ - 1)) == 0 && qcnt) qrank[s.qi] = s.rank;
}

__global__ __launch_bounds__(kBlock) void knn_finalize_kernel(
    const float* __restrict__ q, int Q, int ldq, const float* __restrict__ ms, int M, const int32_t* __restrict__ perm,
    const Prep* __restrict__ prep, const unsigned* __restrict__ rm2_bits, const unsigned* __restrict__ gthr,
    const uint2* __restrict__ ent_all, const int32_t* __restrict__ cand_cnt, int cap, int idx_base,
    int32_t* __restrict__ idx, float* __restrict__ dist, int32_t* __restrict__ flag_list, int32_t* __restrict__ n_flag,
    const UgPrep* __restrict__ ug_prep, int32_t* __restrict__ ug_cnt, float4* __restrict__ ug_slots) {
    const int lane = threadIdx.x & (LPQ - 1);
    const int qi = blockIdx.x * (kBlock / LPQ) + (threadIdx.x / LPQ);
    if (qi >= Q) return;
    const float qx = q[qi], qy = q[qi + (size_t)ldq], qz = q[qi + 2 * (size_t)ldq];
    if (ug_prep && lane == 0) {                // the query grid of the Unique back-check (knn_points.hip): this query's cell
        const UgPrep P = *ug_prep;
        const int cell = (ug_cell1(qz, P.z0, P.inv_c, P.nz) * P.ny + ug_cell1(qy, P.y0, P.inv_c, P.ny)) * P.nx + ug_cell1(qx, P.x0, P.inv_c, P.nx);
        const int s = atomicAdd(&ug_cnt[cell], 1);
        if (s < kUgSlots) ug_slots[(size_t)cell * kUgSlots + s] = make_float4(qx, qy, qz, __int_as_float(qi));
    }
    const int listed = cand_cnt[qi];
    if (direct_answered(listed)) return;       // knn_direct_kernel wrote its answer (the whole group leaves: one query, one word)
    const int total = min(listed, cap);
    const uint2* ent = ent_all + (size_t)qi * cap;
    // pass 1: the two smallest approximate scores of the union (values only)
    float a1 = INFINITY, a2 = INFINITY;
    // An entry past the list's end re-reads the last one and is masked.  An empty list (total == 0) reads ent[0] of the
    // query's own workspace row, which nobody has written, on purpose: in bounds, and masked like the rest.
    uint2 own[kOwnEnt];
    const int last = max(total, 1) - 1;
#pragma unroll
    for (int k = 0; k < kOwnEnt; ++k) own[k] = ent[min(lane + LPQ * k, last)];
#pragma unroll
    for (int k = 0; k < kOwnEnt; ++k) {
        const float s = __uint_as_float(own[k].y);
        if (lane + LPQ * k < total && (int)own[k].x >= 0) { if (s < a2) { if (s < a1) { a2 = a1; a1 = s; } else a2 = s; } }
    }
    for (int e = lane + LPQ * kOwnEnt; e < total; e += LPQ) {
        const uint2 v = ent[e];
        const float s = __uint_as_float(v.y);
        if ((int)v.x >= 0) { if (s < a2) { if (s < a1) { a2 = a1; a1 = s; } else a2 = s; } }
    }
#pragma unroll
    for (int o = LPQ / 2; o > 0; o >>= 1) {
        float b1 = __shfl_xor(a1, o), b2 = __shfl_xor(a2, o);
        float n1 = fminf(a1, b1);
        float n2 = fminf(fmaxf(a1, b1), fminf(a2, b2));
        a1 = n1; a2 = n2;
    }
    // rounding bound (double arithmetic on the fp32 quantities the candidate kernel used)
    const double u = 5.9604644775390625e-08;                     // 2^-24
    const float cxf = prep->cx, cyf = prep->cy, czf = prep->cz, sg = prep->sigma;
    const float tx = qx - cxf, ty = qy - cyf, tz = qz - czf;       // the same q~ the candidate kernel formed
    const bool scored = scale_usable(prep) && fabsf(sg * tx) <= kQueryScaledMax && fabsf(sg * ty) <= kQueryScaledMax && fabsf(sg * tz) <= kQueryScaledMax;
    const double r2 = (double)tx * tx + (double)ty * ty + (double)tz * tz;
    const double r = sqrt(r2);
    const double Rm2 = (double)__uint_as_float(*rm2_bits);
    // scores from the f16-split matrix-core product (knn_mfma16.hip): 16 u r R_m for the two-term f16 representations
    // of Q and m (2^-22 relative each) and 32.1 u (R_m^2 + 2 r R_m) for sixteen fp32 accumulation steps of at most
    // one ulp each.
    const double Eab = score_error_bound(1, Rm2, r);
    // pass 2: exact distances of every candidate that can still reach the top-2
    const float cut = (float)((double)a2 + 2.0 * Eab + 16.0 * u * fabs((double)a2 + r2));
    const float cut_up = nextafterf(cut, INFINITY);              // float rounding of the cut must not exclude anything
    float d1 = INFINITY, d2 = INFINITY; int i1 = -1, i2 = -1;
    const bool all = !(a2 < INFINITY);                            // fewer than two scores: no cut
#pragma unroll
    for (int k = 0; k < kOwnEnt; ++k) {
        const int j = (int)own[k].x; const float sc = __uint_as_float(own[k].y);
        expand_flagged(group_flags(lane + LPQ * k < total && j >= 0 && (sc <= cut_up || all)), j, lane, qx, qy, qz, ms, M, perm, d1, d2, i1, i2);
    }
    for (int e0 = LPQ * kOwnEnt; e0 < total; e0 += LPQ) {        // (the trip count is the group's: every lane of it takes part in the ballot)
        const uint2 v = ent[min(e0 + lane, last)];
        const int j = (int)v.x; const float sc = __uint_as_float(v.y);
        expand_flagged(group_flags(e0 + lane < total && j >= 0 && (sc <= cut_up || all)), j, lane, qx, qy, qz, ms, M, perm, d1, d2, i1, i2);
    }
    group_top2_merge(d1, d2, i1, i2);
    // certificate
    const unsigned gword = gthr[qi];
    const float G = ord2f(gword);
    bool ok;
    if (!scored) ok = false;                                     // never scored on the matrix cores: redo exactly
    else if (M <= 2) ok = (i1 >= 0) && (M < 2 || i2 >= 0);       // nothing outside the lists when M <= KC
    else if (gword == 0xFFFFFFFFu) ok = true;                    // never published, never seeded: nothing was skipped, every point is a candidate
    else if (!(G < INFINITY)) ok = false;                        // a published +inf (scores overflowed): no bound, redo exactly
    else {
        double lower = (double)G + r2;
        double E = Eab + 16.0 * u * ((double)d2 + fabs(lower));
        ok = (i2 >= 0) && (lower - E > (double)d2);
    }
    if (lane == 0) {
        if (ok) {
            idx[(size_t)qi * 2] = i1 >= 0 ? i1 + idx_base : -1; idx[(size_t)qi * 2 + 1] = i2 >= 0 ? i2 + idx_base : -1;
            dist[(size_t)qi * 2] = d1; dist[(size_t)qi * 2 + 1] = d2;
        } else {
            int slot = atomicAdd(n_flag, 1);
            flag_list[slot] = qi;
        }
    }
}

// ---- S4. the unproven queries again, exactly: ONE launch --------------------------------------------------------
// few (<= kFew): work item = listed query, one workgroup each.  Phase A: its threads test the tile boxes against the query
// POINT with the rule of DESIGN 4.1 (D = the query's own dk: two real model points lie within it, every row of a skipped tile
// is strictly farther) and list the surviving tiles in LDS.  Phase B: the survivors' 64-row segments of the sorted copy are
// dealt over the four waves evenly, ranking by (distance, perm[row]).  Both phases issue a batch of loads before they use the
// first.  No partials cross workgroups.
// many: work item = (tile of kTailQ listed queries, chunk of the model); a lane owns four queries, the chunk streams
// through LDS -- knn2_points_kernel's loop (6 VALU per pair, the oracle's bits).  The workgroup that delivers the LAST
// partial of a tile (an arrival counter, cleared by S1) merges the partials by (distance, index) and writes the result.
// Partials cross workgroups through device-coherent accesses (relaxed agent-scope atomic stores / loads) and a relaxed
// counter: no agent-scope fence (it would write back / invalidate the XCD's L2).
constexpr int kFew = 1024;
constexpr int kTailGrid = 2048, kTailQ = 4 * kBlock;              // tiled form: 1024 queries per tile
constexpr int kTailList = 4 * kMTile;            // few-form: tile numbers the survivor list holds (the 16 KB of the many-form's LDS tile)
constexpr int kTailBoxes = 8, kTailSegs = 8;     // few-form: boxes per thread, and 64-row segments per wave, loaded before the first is used
struct Top2 { float d1, d2; int i1, i2; };
__device__ __forceinline__ void top2_insert(Top2& t, float d, int j) {
    // candidates arrive in ascending j, so strict '<' keeps the lowest index
    if (d < t.d2) {
        if (d < t.d1) { t.d2 = t.d1; t.i2 = t.i1; t.d1 = d; t.i1 = j; }
        else { t.d2 = d; t.i2 = j; }
    }
}
__device__ __forceinline__ void top2_wave_merge(float& d1, float& d2, int& i1, int& i2) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float e1 = __shfl_xor(d1, o), e2 = __shfl_xor(d2, o);
        int j1s = __shfl_xor(i1, o), j2s = __shfl_xor(i2, o);
        bool first_mine = lex_lt_f(d1, i1, e1, j1s);
        float w1 = first_mine ? d1 : e1; int k1 = first_mine ? i1 : j1s;
        float x2 = first_mine ? d2 : d1; int y2 = first_mine ? i2 : i1;
        float x3 = first_mine ? e1 : e2; int y3 = first_mine ? j1s : j2s;
        bool sec_mine = lex_lt_f(x2, y2, x3, y3);
        d1 = w1; i1 = k1; d2 = sec_mine ? x2 : x3; i2 = sec_mine ? y2 : y3;
    }
}
__global__ __launch_bounds__(kBlock) void knn_tail_kernel(
    const float* __restrict__ q, int ldq, const float* __restrict__ m, int M, int ldm, const float* __restrict__ ms /* sorted copy, ld = M */,
    const int32_t* __restrict__ perm, const float* __restrict__ tbox, const float* __restrict__ dk, int idx_base,
    const int32_t* __restrict__ flag_list, SearchCounters* __restrict__ ctr,
    int32_t* __restrict__ part_idx, float* __restrict__ part_dist /* many: [S][tiles * kTailQ][2] */,
    int32_t* __restrict__ idx, float* __restrict__ dist, int list_cap /* few: tiles per pass, 1 .. kTailList */) {
    const int nf = ctr->n_flag;
    if (nf <= 0) return;
    __shared__ float sd[kBlock / 64][2];
    __shared__ int si[kBlock / 64][2];
    __shared__ int s_last, s_nlist;
    __shared__ float4 tile[kMTile];
    int* const s_list = (int*)tile;                   // few: the surviving tiles of a pass (the many-form's LDS tile is free there)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (nf <= kFew) {
        const int n_tiles = (M + kT16 - 1) / kT16;
        for (int f = blockIdx.x; f < nf; f += gridDim.x) {
            const int qi = flag_list[f];
            const float qx = q[qi], qy = q[qi + (size_t)ldq], qz = q[qi + 2 * (size_t)ldq];
            // DESIGN 4.1's rule with the block box shrunk to the query itself and D its own seed distance: two real model
            // points lie within D, every row of a skipped tile is strictly farther.  No finite D, or a coordinate that
            // is not finite: every tile is scanned.
            const float D = dk[qi];
            const bool cullq = D < INFINITY && fabsf(qx) < INFINITY && fabsf(qy) < INFINITY && fabsf(qz) < INFINITY;
            const double qd[3] = {(double)qx, (double)qy, (double)qz};
            float d1 = INFINITY, d2 = INFINITY; int i1 = -1, i2 = -1;
            // A pass covers list_cap tiles, so its survivors always fit the list (one pass for up to 4 * kMTile tiles).
            for (int c0 = 0; c0 < n_tiles; c0 += list_cap) {
                const int c1 = min(c0 + list_cap, n_tiles);
                // phase A: all threads test the pass's tiles, kTailBoxes boxes per thread loaded before the first is judged
                // (a tile past the end loads the last one's box and is masked); survivors go to the list in any order
                __syncthreads();                                      // the previous pass's / query's readers are done with the list
                if (threadIdx.x == 0) s_nlist = cullq ? 0 : c1 - c0;
                __syncthreads();
                if (!cullq) {
                    for (int ct = c0 + threadIdx.x; ct < c1; ct += kBlock) s_list[ct - c0] = ct;
                } else {
                    for (int b0 = c0 + threadIdx.x; b0 < c1; b0 += kTailBoxes * kBlock) {
                        float2 bx[kTailBoxes][3];
#pragma unroll
                        for (int k = 0; k < kTailBoxes; ++k) {
                            const float2* p = (const float2*)(tbox + (size_t)min(b0 + k * kBlock, c1 - 1) * 6);
                            bx[k][0] = p[0]; bx[k][1] = p[1]; bx[k][2] = p[2];
                        }
#pragma unroll
                        for (int k = 0; k < kTailBoxes; ++k) {
                            const int ct = b0 + k * kBlock;
                            const float lo[3] = {bx[k][0].x, bx[k][0].y, bx[k][1].x}, hi[3] = {bx[k][1].y, bx[k][2].x, bx[k][2].y};
                            if (ct < c1 && !cull_skips(cull_gap2(lo, hi, qd, qd), D)) s_list[atomicAdd(&s_nlist, 1)] = ct;
                        }
                    }
                }
                __syncthreads();
                // phase B: the survivors' 64-row segments dealt over the waves, segment s to wave s % 4; a wave loads the rows
                // of kTailSegs segments before it compares (a row past M reads row M - 1 and is masked), and their perm words
                // in one more round only where some lane has a row that can still enter its top two
                const int n_seg = s_nlist * (kT16 / 64);
                for (int s0 = wave; s0 < n_seg; s0 += kTailSegs * (kBlock / 64)) {
                    int j[kTailSegs]; float x[kTailSegs], y[kTailSegs], z[kTailSegs];
#pragma unroll
                    for (int k = 0; k < kTailSegs; ++k) {
                        const int s = min(s0 + k * (kBlock / 64), n_seg - 1);
                        j[k] = s0 + k * (kBlock / 64) < n_seg ? s_list[s / (kT16 / 64)] * kT16 + (s % (kT16 / 64)) * 64 + lane : M;
                        const int jc = min(j[k], M - 1);
                        x[k] = ms[jc]; y[k] = ms[jc + (size_t)M]; z[k] = ms[jc + 2 * (size_t)M];
                    }
                    float d[kTailSegs]; bool any = false;
#pragma unroll
                    for (int k = 0; k < kTailSegs; ++k) {
                        d[k] = point_d2(qx, qy, qz, x[k], y[k], z[k]);
                        any = any || (j[k] < M && d[k] <= d2 && d[k] < INFINITY);
                    }
                    if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
                        int oj[kTailSegs];
#pragma unroll
                        for (int k = 0; k < kTailSegs; ++k) oj[k] = perm[min(j[k], M - 1)];
#pragma unroll
                        for (int k = 0; k < kTailSegs; ++k) {
                            // (distance, ORIGINAL row) order; +inf is never an answer
                            if (j[k] < M && d[k] <= d2 && d[k] < INFINITY && lex_lt_f(d[k], oj[k], d2, i2)) {
                                if (lex_lt_f(d[k], oj[k], d1, i1)) { d2 = d1; i2 = i1; d1 = d[k]; i1 = oj[k]; } else { d2 = d[k]; i2 = oj[k]; }
                            }
                        }
                    }
                }
            }
            top2_wave_merge(d1, d2, i1, i2);
            __syncthreads();                                          // the previous trip's readers are done with sd / si
            if (lane == 0) { sd[wave][0] = d1; sd[wave][1] = d2; si[wave][0] = i1; si[wave][1] = i2; }
            __syncthreads();
            if (threadIdx.x == 0) {
                Top2T<float> r{INFINITY, INFINITY, -1, -1};
                for (int k = 0; k < kBlock / 64; ++k) { top2_insert_lex_t(r, sd[k][0], si[k][0]); top2_insert_lex_t(r, sd[k][1], si[k][1]); }
                idx[(size_t)qi * 2] = r.i1 >= 0 ? r.i1 + idx_base : -1; idx[(size_t)qi * 2 + 1] = r.i2 >= 0 ? r.i2 + idx_base : -1;
                dist[(size_t)qi * 2] = r.d1; dist[(size_t)qi * 2 + 1] = r.d2;
            }
        }
        return;
    }
    // many: tiles of kTailQ listed queries x S chunks of the model
    const int n_qt = (nf + kTailQ - 1) / kTailQ;
    const int max_S = (M + kMTile - 1) / kMTile;
    int S = kTailGrid / n_qt; if (S < 1) S = 1; if (S > max_S) S = max_S; if (S < 1) S = 1;
    const int chunk = ((M + S - 1) / S + kMTile - 1) / kMTile * kMTile;
    S = M > 0 ? (M + chunk - 1) / chunk : 1;
    const size_t slots_cap = (size_t)n_qt * kTailQ;
    for (int w = blockIdx.x; w < n_qt * S; w += gridDim.x) {
        const int qt = w / S, s = w % S;
        const int m_begin = s * chunk, m_end = min(M, m_begin + chunk);
        float qx[4], qy[4], qz[4]; Top2 best[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int slot = qt * kTailQ + r * kBlock + threadIdx.x;
            const bool ok = slot < nf;
            const int qi = ok ? flag_list[slot] : 0;
            qx[r] = ok ? q[qi] : 0.0f; qy[r] = ok ? q[qi + (size_t)ldq] : 0.0f; qz[r] = ok ? q[qi + 2 * (size_t)ldq] : 0.0f;
            best[r] = Top2{INFINITY, INFINITY, -1, -1};
        }
        for (int t0 = m_begin; t0 < m_end; t0 += kMTile) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kMTile / kBlock; ++k) {
                const int j = t0 + k * kBlock + threadIdx.x;
                float4 v;
                if (j < m_end) { v.x = m[j]; v.y = m[j + (size_t)ldm]; v.z = m[j + 2 * (size_t)ldm]; v.w = 0.0f; }
                else { v.x = v.y = v.z = INFINITY; v.w = 0.0f; }     // padding never beats anything
                tile[k * kBlock + threadIdx.x] = v;
            }
            __syncthreads();
            const int cnt = min(kMTile, m_end - t0);
            const int nb = (cnt + 3) / 4 * 4;
            for (int jb = 0; jb < nb; jb += 4) {
                float4 mp[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) mp[u] = tile[jb + u];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float d[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) d[u] = point_d2(qx[r], qy[r], qz[r], mp[u].x, mp[u].y, mp[u].z);
                    const float mn = fminf(fminf(d[0], d[1]), fminf(d[2], d[3]));
                    if (mn < best[r].d2) {
                        const int j0 = t0 + jb;
#pragma unroll
                        for (int u = 0; u < 4; ++u) top2_insert(best[r], d[u], j0 + u);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int slot = qt * kTailQ + r * kBlock + threadIdx.x;
            if (slot < nf) {
                const size_t o = ((size_t)s * slots_cap + slot) * 2;
                __hip_atomic_store(&part_idx[o], best[r].i1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&part_idx[o + 1], best[r].i2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&part_dist[o], best[r].d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&part_dist[o + 1], best[r].d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(&ctr->done[qt], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == S - 1;
        __syncthreads();
        if (s_last) {                         // every chunk of this tile is in: a wave per listed query merges its S partials
            const int s_hi = min(nf, (qt + 1) * kTailQ);
            for (int slot = qt * kTailQ + wave; slot < s_hi; slot += kBlock / 64) {
                float d1 = INFINITY, d2 = INFINITY; int i1 = -1, i2 = -1;
                for (int s2 = lane; s2 < S; s2 += 64) {           // chunks ascend in model index; (distance, index) order throughout
                    const size_t p = ((size_t)s2 * slots_cap + slot) * 2;
                    const int a = __hip_atomic_load(&part_idx[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const int b = __hip_atomic_load(&part_idx[p + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const float da = __hip_atomic_load(&part_dist[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const float db = __hip_atomic_load(&part_dist[p + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (a >= 0 && lex_lt_f(da, a, d2, i2)) { if (lex_lt_f(da, a, d1, i1)) { d2 = d1; i2 = i1; d1 = da; i1 = a; } else { d2 = da; i2 = a; } }
                    if (b >= 0 && lex_lt_f(db, b, d2, i2)) { if (lex_lt_f(db, b, d1, i1)) { d2 = d1; i2 = i1; d1 = db; i1 = b; } else { d2 = db; i2 = b; } }
                }
                top2_wave_merge(d1, d2, i1, i2);
                if (lane == 0) {
                    const int qi = flag_list[slot];
                    idx[(size_t)qi * 2] = i1 >= 0 ? i1 + idx_base : -1; idx[(size_t)qi * 2 + 1] = i2 >= 0 ? i2 + idx_base : -1;
                    dist[(size_t)qi * 2] = d1; dist[(size_t)qi * 2 + 1] = d2;
                }
            }
        }
    }
}

// pcreg_debug_set("knn_stats", 1): one thread adds this search's counters to the process-wide sums (after S3, which
// leaves n_flag; nothing waits for the host)
__global__ void knn_stats_kernel(const SearchCounters* __restrict__ ctr, long long nominal, unsigned long long* __restrict__ stats) {
    if (threadIdx.x != 0) return;
    long long nv = 0;
    for (int k = 0; k < kVisitSlots; ++k) nv += ctr->visited[k];
    atomicAdd(&stats[0], 1ull); atomicAdd(&stats[1], (unsigned long long)nv);         // (searches on other streams add too)
    atomicAdd(&stats[2], (unsigned long long)nominal); atomicAdd(&stats[3], (unsigned long long)ctr->n_flag);
    atomicAdd(&stats[4], (unsigned long long)(unsigned)ctr->units); atomicAdd(&stats[5], 32ull * (unsigned long long)nv);
}

// pcreg_debug_set("knn_direct_stats", 1): this search's direct answers added to the process-wide sums (after S1b, which publishes them)
__global__ void knn_direct_stats_kernel(const SearchCounters* __restrict__ ctr, unsigned long long* __restrict__ stats) {
    if (threadIdx.x != 0) return;
    atomicAdd(&stats[0], 1ull); atomicAdd(&stats[1], (unsigned long long)(unsigned)ctr->n_direct);
    atomicAdd(&stats[2], (unsigned long long)(unsigned)ctr->direct_rows);
}

constexpr int kSeedMinM = 16 * 1024;            // below this the lists settle within the first tiles anyway
// the grid is sized on the device (about M/2 cells plus the margin layer); this is the capacity it may use
size_t seed_cell_cap(int M) { return std::min<size_t>((size_t)kSeedMaxCells, std::max<size_t>(4096, (size_t)M)); }

}  // namespace

// ---- a prepared model in device memory ---------------------------------------------------------------------------
// The prepared block, walked once.  sort_cnt and seed_cnt adjoin (model_bbox_partial_kernel clears both in one go), so the
// ordering grid's counters take exactly their bytes.
static size_t n_f16_tiles(int M) { return (size_t)((M > 0 ? M : 0) + kT16 - 1) / kT16; }
static size_t ubox_floats(int M) { return std::max<size_t>(n_f16_tiles(M), 1) * (kT16 / 64) * 6; }
// own_ubox = false: the caller keeps the units' boxes elsewhere (the search without a handle, below)
static ModelView model_layout(const float* m, int M, int ldm, void* block, size_t* bytes, bool own_ubox = true) {
    const size_t mm = (size_t)(M > 0 ? M : 1);
    WsWalk w(block);
    ModelView v{};
    v.m = m; v.M = M; v.ldm = ldm;
    v.prep = w.take_bytes(256);                                    // Prep
    v.rm2 = (unsigned*)w.take_bytes(256);                          // R_m^2 bits
    v.box_part = w.take<float>(512 * 6);                           // box partials
    v.tiles = w.take_bytes(align_up(knn_f16_prep_bytes(M), 256));  // f16 tiles
    v.sort_cnt = (int32_t*)w.take_bytes((size_t)kSortKeys * 4);    // ordering-grid counters
    v.seeded = M >= kSeedMinM && PCREG_EXP_ENV("PCREG_KNN_NOSEED", 0) == 0;
    if (M >= kSeedMinM) {                                          // seeding-grid counters and slots
        v.seed_cnt = w.take<int32_t>(seed_cell_cap(M));
        v.seed_slots = w.take_bytes(align_up(seed_cell_cap(M) * kSeedSlots * 16, 256));
    }
    v.perm = w.take<int32_t>(mm);
    v.ms = w.take<float>(mm * 3);                                  // sorted fp32 SoA copy
    v.tbox = w.take<float>(std::max<size_t>(n_f16_tiles(M), 1) * 6);       // one box per f16 tile
    if (own_ubox) v.ubox = w.take<float>(ubox_floats(M));                  // ... and per unit of 64 rows
    *bytes = w.bytes(); return v;
}
size_t model_prep_bytes(int M) { size_t b; (void)model_layout(nullptr, M, 0, nullptr, &b); return b; }
ModelView model_view(const float* m, int M, int ldm, void* block) { size_t b; return model_layout(m, M, ldm, block, &b); }
// enqueue the two preparation passes (P1, P2) on `st`
int launch_model_prepare(const ModelView& v, hipStream_t st) {
    PCREG_ARG(v.M >= 0 && v.ldm >= v.M);
    if (v.M == 0) return PCREG_OK;
    int nb = (v.M + kBlock * 16 - 1) / (kBlock * 16); if (nb > 512) nb = 512; if (nb < 1) nb = 1;
    hipLaunchKernelGGL(model_bbox_partial_kernel, dim3(nb), dim3(kBlock), 0, st, v.m, v.M, v.ldm, v.box_part, v.sort_cnt,
                       kSortKeys + (v.seeded ? (int)seed_cell_cap(v.M) : 0));
    hipLaunchKernelGGL(model_bbox_final_kernel, dim3(1), dim3(64), 0, st, v.box_part, nb, v.M, (int)seed_cell_cap(v.M), (Prep*)v.prep, v.rm2);
    // the rows in Morton order of their ordering-grid cells; everything below is built from the sorted copy
    int ob = (v.M + kBlock * 4 - 1) / (kBlock * 4); if (ob > 2048) ob = 2048;
    hipLaunchKernelGGL(model_order_count_kernel, dim3(ob), dim3(kBlock), 0, st, v.m, v.M, v.ldm, (const Prep*)v.prep, v.sort_cnt);
    hipLaunchKernelGGL(exclusive_scan_1wg_kernel, dim3(1), dim3(1024), 0, st, v.sort_cnt, kSortKeys);
    hipLaunchKernelGGL(model_order_scatter_kernel, dim3(ob), dim3(kBlock), 0, st, v.m, v.M, v.ldm, (const Prep*)v.prep, v.sort_cnt, v.perm, v.ms);
    PCREG_HIP(hipGetLastError());
    int rc = launch_prep_model_f16(v.ms, v.M, v.M, v.prep, v.rm2, v.tiles, v.seeded ? v.seed_cnt : nullptr, v.seed_slots, st);
    if (rc) return rc;
    hipLaunchKernelGGL(tile_box_kernel, dim3((unsigned)n_f16_tiles(v.M)), dim3(kBlock), 0, st, (const float*)v.ms, v.M, v.tbox, v.ubox);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

// ---- the per-call workspace of a search (and of the match stage that follows it) ----------------------------------
static constexpr int kTargetBlocks = 4096;
static size_t tail_many(size_t qq) { return (size_t)(kTailGrid + (qq + kTailQ - 1) / kTailQ) * kTailQ * 2; }     // the many-form's partials
SearchWs search_ws_layout(int Q, int M, void* base, size_t* bytes) {
    SearchWs s{};
    const size_t qq = (size_t)(Q > 0 ? Q : 1);
    int q_blocks, W;
    knn_f16_shape(Q > 0 ? Q : 1, M > 0 ? M : 1, kTargetBlocks, &q_blocks, &W);
    s.cap = W * KC;
    WsWalk w(base);
    s.ctr = w.take_bytes(align_up(sizeof(SearchCounters), 256));
    s.gthr = w.take<unsigned>(qq); s.flag_list = w.take<int32_t>(qq); s.cand_cnt = w.take<int32_t>(qq);
    s.cand_ent = w.take_bytes(align_up(qq * (size_t)(kF16MaxS * KC) * 8, 256));      // the call may see a smaller M than the sizing did
    // The tail's partials (many-form only; the few-form keeps none) and the visit plan (knn_plan_kernel: per query block the
    // number of tiles to visit, then their ascending list) share one slot: the plan is dead once the candidate kernel has run,
    // two launches before the tail writes a partial.
    const size_t many = tail_many(qq);
    const size_t plan_head = align_up((size_t)q_blocks * 4, 256) / 4, plan_list = (size_t)q_blocks * std::max<size_t>(n_f16_tiles(M), 1),
                 plan = plan_head + 2 * plan_list;                     // the list, then one unit mask per list position
    s.tail_idx = w.take<int32_t>(std::max(many, plan)); s.tail_dist = w.take<float>(many);
    s.n_vis = s.tail_idx; s.vis_list = s.tail_idx ? s.tail_idx + plan_head : nullptr;
    s.vis_mask = s.tail_idx ? (uint32_t*)(s.tail_idx + plan_head + plan_list) : nullptr;
    s.ug_cells = (int)ug_cells_cap(Q);
    s.ug_nparts = (int)((qq * 8 + kBlock - 1) / kBlock);
    s.ug_prep = w.take_bytes(256);
    s.ug_part = w.take<float>((size_t)s.ug_nparts * 6);
    s.ug_cnt = w.take<int32_t>((size_t)s.ug_cells);
    s.ug_slots = w.take_bytes(align_up((size_t)s.ug_cells * kUgSlots * 16, 256));
    s.qcnt = (int32_t*)w.take_bytes((size_t)kQueryKeys * 4);
    s.qperm = w.take<int32_t>(qq); s.dk = w.take<float>(qq);
    *bytes = w.bytes(); return s;
}
size_t search_ws_bytes(int Q, int M) { size_t b; (void)search_ws_layout(Q, M, nullptr, &b); return b; }

// S1..S4 against a prepared model.  with_grid: also build the query grid (the match stage with Unique needs it).
int launch_model_search(const ModelView& v, const float* q, int Q, int ldq, int32_t idx_base, int32_t* idx, float* dist,
                        void* ws, size_t ws_bytes, bool with_grid, bool timed, hipStream_t st) {
    PCREG_ARG(Q >= 0 && ldq >= Q && Q <= kMaxQTiles * 1024);
    if (Q == 0) return PCREG_OK;
    size_t need;
    SearchWs s = search_ws_layout(Q, v.M, ws, &need);
    if (ws_bytes < need) { set_error("search workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_WORKSPACE; }
    SearchCounters* ctr = (SearchCounters*)s.ctr;
    const bool grid = with_grid && v.M > 0;          // (an empty model matches nothing: the match stage never looks at the grid)
    const bool order = v.M > 0;                      // (an empty model: no prepared block, no candidate launch)
    if (order) PCREG_HIP(hipMemsetAsync(s.qcnt, 0, (size_t)kQueryKeys * 4, st));
    // S1d: the seeded queries whose cell range is small are answered and marked; the launches below skip them.  Not with
    // "knn_direct" = 1 (every query takes the tile walk: the A/B of one binary), and not while "knn_stats" collects: its
    // counters are defined over the walk of the whole query set.  S1 and S1d are one launch (seed_direct_kernel) unless
    // "knn_seed_fused" = 1 asks for the two.  The direct phase's per-workgroup (answered, rows) pairs go to the head of
    // cand_ent, which is dead from here to the candidate kernel (ug_nparts pairs of 8 bytes; a query's list is larger).
    const bool direct = v.seeded && v.M > 0 && debug_flag(kDbgKnnDirect) == 0 && debug_flag(kDbgKnnStats) == 0;
    const bool fused = direct && debug_flag(kDbgKnnSeedFused) == 0;
    int2* dparts = direct ? (int2*)s.cand_ent : nullptr;
    static_assert((size_t)kF16MaxS * KC * 8 >= sizeof(int2), "the direct phase's pairs fit the head of cand_ent");
    // (a query's place inside its cell waits in flag_list, which is free until knn_finalize_kernel lists the unproven queries)
    if (fused)
        hipLaunchKernelGGL(seed_direct_kernel, dim3(s.ug_nparts), dim3(kBlock), 0, st, q, Q, ldq, (const Prep*)v.prep, (const int32_t*)v.seed_cnt,
                           (const float4*)v.seed_slots, s.gthr, s.cand_cnt, ctr, grid ? s.ug_part : nullptr, grid ? s.ug_cnt : nullptr, s.ug_cells,
                           s.dk, s.qcnt, s.flag_list, (const int32_t*)v.sort_cnt, (const float*)v.ms, v.M, (const int32_t*)v.perm, (int)idx_base,
                           idx, dist, dparts);
    else
        hipLaunchKernelGGL(seed_query_kernel, dim3(s.ug_nparts), dim3(kBlock), 0, st, q, Q, ldq, (const Prep*)v.prep, (const int32_t*)v.seed_cnt,
                           (const float4*)v.seed_slots, (v.seeded && v.M > 0) ? 1 : 0, s.gthr, s.cand_cnt, ctr, grid ? s.ug_part : nullptr,
                           grid ? s.ug_cnt : nullptr, s.ug_cells, s.dk, order ? s.qcnt : nullptr, s.flag_list);
    if (direct && !fused)
        hipLaunchKernelGGL(knn_direct_kernel, dim3(s.ug_nparts), dim3(kBlock), 0, st, q, Q, ldq, (const float*)s.dk,
                           (const Prep*)v.prep, (const int32_t*)v.sort_cnt, (const float*)v.ms, v.M, (const int32_t*)v.perm, (int)idx_base, idx, dist,
                           s.cand_cnt, dparts);
    if (order)             // (also publishes the direct phase's sums in ctr: before the counters below and the plan read them)
        hipLaunchKernelGGL(query_order_ranked_kernel, dim3((Q + kBlock - 1) / kBlock), dim3(kBlock), 0, st, q, Q, ldq, (const Prep*)v.prep,
                           (const int32_t*)s.qcnt, (const int32_t*)s.flag_list, s.qperm, (const int2*)dparts, s.ug_nparts, ctr);
    if (unsigned long long* dstats = knn_direct_stats_dev())
        hipLaunchKernelGGL(knn_direct_stats_kernel, dim3(1), dim3(64), 0, st, (const SearchCounters*)ctr, dstats);
    int W = 1;
    const int variant = PCREG_EXP_ENV("PCREG_KNN_VARIANT", 40);      // 41: timing-only form of the candidate kernel (EXPERIMENTS builds)
    const int target_env = PCREG_EXP_ENV("PCREG_KNN_BLOCKS", 0);      // (any shape fits: the lists are sized for kF16MaxS workgroups)
    const int cull = (debug_flag(kDbgKnnNoCull) || PCREG_EXP_ENV("PCREG_KNN_NOCULL", 0)) ? 0 : 1;    // "knn_nocull": visit every tile
    int rc = launch_knn_candidates_f16(q, Q, ldq, s.qperm, s.dk, v.M, v.prep, v.tiles, v.tbox, v.ubox, cull, s.n_vis, s.vis_list, s.vis_mask, s.gthr, s.cand_ent, s.cand_cnt, ctr,
                                       target_env > 0 ? target_env : kTargetBlocks, variant == 41, timed, grid ? s.ug_part : nullptr,
                                       s.ug_nparts, s.ug_cells, grid ? s.ug_prep : nullptr, &W, st);
    if (rc) return rc;
    hipLaunchKernelGGL(knn_finalize_kernel, dim3((Q + kBlock / LPQ - 1) / (kBlock / LPQ)), dim3(kBlock), 0, st, q, Q, ldq, (const float*)v.ms, v.M,
                       (const int32_t*)v.perm, (const Prep*)v.prep, (const unsigned*)v.rm2, (const unsigned*)s.gthr, (const uint2*)s.cand_ent,
                       (const int32_t*)s.cand_cnt, W * KC, (int)idx_base, idx, dist, s.flag_list, &ctr->n_flag,
                       grid ? (const UgPrep*)s.ug_prep : nullptr, s.ug_cnt, (float4*)s.ug_slots);
    if (unsigned long long* stats = knn_stats_dev()) {
        const long long nominal = (long long)((Q + 511) / 512) * (long long)n_f16_tiles(v.M);
        hipLaunchKernelGGL(knn_stats_kernel, dim3(1), dim3(64), 0, st, (const SearchCounters*)ctr, nominal, stats);
    }
    if (PCREG_EXP_ENV("PCREG_KNN_DEBUG", 0)) {
        int32_t nf = 0, vis[kVisitSlots];
        PCREG_HIP(hipMemcpyAsync(&nf, &ctr->n_flag, 4, hipMemcpyDeviceToHost, st));
        PCREG_HIP(hipMemcpyAsync(vis, ctr->visited, sizeof(vis), hipMemcpyDeviceToHost, st)); PCREG_HIP(hipStreamSynchronize(st));
        long long nv = 0;
        for (int k = 0; k < kVisitSlots; ++k) nv += vis[k];
        const long long qb = (Q + 511) / 512, nt = (long long)n_f16_tiles(v.M);
        fprintf(stderr, "[pcreg] knn fast: Q=%d M=%d W=%d unproven=%d visited tile pairs=%lld of %lld (%.4f)%s\n", Q, v.M, W, nf, nv, qb * nt,
                qb * nt > 0 ? (double)nv / (double)(qb * nt) : 0.0, cull ? "" : " (culling off)");
    }
    const int dbg_cap = debug_flag(kDbgKnnTailCap);                  // "knn_tail_cap": n > 0 -- the few-form's passes cover n tiles each, same bits
    const int tail_cap = dbg_cap > 0 && dbg_cap < kTailList ? dbg_cap : kTailList;
    hipLaunchKernelGGL(knn_tail_kernel, dim3(kTailGrid), dim3(kBlock), 0, st, q, ldq, v.m, v.M, v.ldm, (const float*)v.ms, (const int32_t*)v.perm,
                       (const float*)v.tbox, (const float*)s.dk, (int)idx_base, (const int32_t*)s.flag_list, ctr, s.tail_idx, s.tail_dist, idx, dist, tail_cap);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

// S1b for another search (the k-nearest search, knn_k.hip): qcnt holds the per-parent-cell counts of the call's queries
int launch_query_order(const ModelView& v, const float* q, int Q, int ldq, int32_t* qcnt, int32_t* qperm, hipStream_t st) {
    hipLaunchKernelGGL(exclusive_scan_1wg_kernel, dim3(1), dim3(1024), 0, st, qcnt, kQueryKeys);
    hipLaunchKernelGGL(query_order_kernel, dim3((Q + kBlock - 1) / kBlock), dim3(kBlock), 0, st, q, Q, ldq, (const Prep*)v.prep, qcnt, qperm);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

// ---- test hooks: what a prepared model and the last search on a workspace hold (device-to-device copies) ------------
int model_export(const ModelView& v, int32_t* perm, float* sorted_soa, float* tile_box, float prep[24], hipStream_t st) {
    static_assert(sizeof(Prep) <= 24 * sizeof(float), "pcreg_debug_dev_model_export copies Prep into 24 words");
    if (prep) std::fill(prep, prep + 24, 0.0f);
    if (v.M == 0) return PCREG_OK;                   // nothing was prepared
    if (perm) PCREG_HIP(hipMemcpyAsync(perm, v.perm, (size_t)v.M * 4, hipMemcpyDeviceToDevice, st));
    if (sorted_soa) PCREG_HIP(hipMemcpyAsync(sorted_soa, v.ms, (size_t)v.M * 12, hipMemcpyDeviceToDevice, st));
    if (tile_box) PCREG_HIP(hipMemcpyAsync(tile_box, v.tbox, n_f16_tiles(v.M) * 24, hipMemcpyDeviceToDevice, st));
    if (prep) {
        PCREG_HIP(hipMemcpyAsync(prep, v.prep, sizeof(Prep), hipMemcpyDeviceToHost, st));
        PCREG_HIP(hipStreamSynchronize(st));
    }
    return PCREG_OK;
}
int search_export(const void* ws, size_t ws_bytes, int Q, int M, int32_t* qperm, float* dk, hipStream_t st) {
    PCREG_ARG(ws != nullptr && Q >= 0 && M >= 0);
    if (Q == 0) return PCREG_OK;
    size_t need;
    const SearchWs s = search_ws_layout(Q, M, const_cast<void*>(ws), &need);
    if (ws_bytes < need) { set_error("search workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_WORKSPACE; }
    if (qperm) PCREG_HIP(hipMemcpyAsync(qperm, s.qperm, (size_t)Q * 4, hipMemcpyDeviceToDevice, st));
    if (dk) PCREG_HIP(hipMemcpyAsync(dk, s.dk, (size_t)Q * 4, hipMemcpyDeviceToDevice, st));
    return PCREG_OK;
}

// ---- the search without a handle: prepare into the caller's workspace, then search ---------------------------------
// The model is prepared and searched within one call here, so the units' boxes (read by knn_plan_kernel only) go where the
// call's workspace has room that is still unused then: tail_dist, which nothing touches before knn_tail_kernel, three
// launches after the plan.  Only a model whose boxes outgrow that slot (tens of millions of rows) takes bytes of its own.
static bool ubox_in_tail(int Q, int M) { return ubox_floats(M) <= tail_many((size_t)(Q > 0 ? Q : 1)); }
size_t knn2_points_fast_workspace_bytes(int Q, int M) {
    size_t b; (void)model_layout(nullptr, M, 0, nullptr, &b, !ubox_in_tail(Q, M));
    return search_ws_bytes(Q, M) + b;
}

int launch_knn2_points_fast_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm, int32_t idx_base,
                                int32_t* idx, float* dist, void* ws, size_t ws_bytes, hipStream_t st, bool timed) {
    PCREG_ARG(Q >= 0 && M >= 0 && ldq >= Q && ldm >= M);
    if (Q == 0) return PCREG_OK;
    const size_t need = knn2_points_fast_workspace_bytes(Q, M);
    if (ws_bytes < need) { set_error("knn (fast) workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_WORKSPACE; }
    const size_t sb = search_ws_bytes(Q, M);
    size_t mb;
    ModelView v = model_layout(m, M, ldm, (char*)ws + sb, &mb, !ubox_in_tail(Q, M));
    if (!v.ubox) { size_t b2; v.ubox = search_ws_layout(Q, M, ws, &b2).tail_dist; }
    int rc = launch_model_prepare(v, st);
    if (rc) return rc;
    return launch_model_search(v, q, Q, ldq, idx_base, idx, dist, ws, sb, false, timed, st);
}

}  // namespace pcreg
