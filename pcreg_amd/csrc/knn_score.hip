// pcreg_amd/csrc/knn_score.hip -- score B candidate transforms of one query cloud against a PREPARED model: per transform the
// number of queries with a model row within a squared distance r2 and the sum of those squared distances (fitness and inlier
// RMSE are the caller's arithmetic on them), and on request the nearest row and its distance per (transform, query).
//
// Contract (include/pcreg.h): the transformed query is quick_tf_kernel's arithmetic in double on the widened fp32
// query, rounded once to fp32; the nearest row is the one with the smallest d = fmaf(dz,dz, fmaf(dy,dy, dx*dx)) among the rows
// with d <= r2 (inclusive; NaN never passes; +inf passes r2 = +inf only), ties to the lowest original row.  An all-zero
// transform (what a failed ransac leaves) scores nothing.  Exact by construction: every distance is the fp32 chain itself.
//
// The prepared model (knn_fast.hip) is used as it is.  Per batch of whole transforms (at most 4 Mi query slots):
//   C1  score_transform_kernel        the batch's transformed queries, one fp32 SoA [3][nb Q]; an empty transform's are NaN
//   C2  launch_query_cells + launch_query_order   ALL the batch's slots in one spatial order (knn_range.hip, knn_fast.hip)
//   C3  score_walk_kernel             range_walk_kernel's block box and visit rule (D = r2); four lanes per query keep their best
//                                     (d, row), combined by two shuffles; the result goes to slot [b][i]
//   C4  score_reduce_kernel           per (transform, chunk of 2048 queries): count and sum in query order, a fixed tree
//       score_total_kernel            per transform: its chunks in ascending order
// sum_d2 is a function of the inputs alone: no floating-point atomic, and no term's place depends on the batch or the walk.
//
// The refit (pcreg_model_refit_f32's contract) is the same chain with the walk's other instantiation, which also
// keeps the winning row's coordinates per slot, and two more steps per batch:
//   C5  refit_moments_kernel          per (transform, chunk of 2048 queries): the 27 moments of (model row, moved point) over the
//                                     chunk's hits in query order, shifted by the middle of the model's box; chunk_tail
//   C6  launch_refit_finish           per transform (ransac.hip): the chunks ascending, fit_moments / fit_3pt, step_compose
//
// The point-to-plane refit (pcreg_model_refit_plane_f32's contract) is the refit's chain up to C4 with the walk's
// `idx` pointed at a workspace block, so the winning ORIGINAL row per slot is kept beside its coordinates, and then
//   P5  plane_moments_kernel          per (transform, chunk of 2048 queries): the 28 sums of the plane pairs in query order -- a
//                                     hit whose row has a finite normal, gathered by that row -- and their number; chunk_tail
//   P6  plane_finish_kernel           per transform: finish_step with plane_fit (plane_fit.hpp) about the middle of the model's box
//
// The plane-to-plane refit (pcreg_model_refit_gicp_f32's contract) is the plane refit's chain and workspace with
//   G5  gicp_moments_kernel           in P5's place: a pair is weighted by W = (C_model + R C_query R^T)^-1 from the two normals
//                                     (gicp_pair.hpp); the 28 sums are info_pair.hpp's terms with C := W, unweighted; P6 follows
//
// What the three refits share with each other and with the NDT and coherent-point-drift steps (ndt.hip, cpd.hip) -- the moved
// point, the chunk tail, the hit prologue, the finish step, T * T_step and the empty rule -- is refit_step.hpp's.
#include "common.hpp"
#include "knn_fast_common.hpp"
#include "knn_walk.hpp"
#include "refit_step.hpp"
#include "plane_fit.hpp"
#include "gicp_pair.hpp"
#include "info_pair.hpp"
#include <climits>
#include <cmath>

namespace pcreg {

namespace {

constexpr int kScoreMaxSlots = kMaxQTiles * 1024;    // 4 Mi query slots per walk (and queries per call)
static_assert(kScanBlock == kBlock, "score_reduce_kernel's threads own kScanPer consecutive queries each");

// ---- C1. the transformed queries ----------------------------------------------------------------------------------------
// slot s = bl * Q + i of the batch: moved_point (refit_step.hpp) of [q_i, 1] * T_bl
__global__ __launch_bounds__(kBlock) void score_transform_kernel(const float* __restrict__ q, int Q, int ldq, const double* __restrict__ T,
                                                                 int n_slots, float* __restrict__ tq) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_slots) return;
    const int bl = s / Q, i = s - bl * Q;
    double t[16];
    const bool empty = load_transform(T, bl, t);
    float p[3];
    moved_point(t, (double)q[i], (double)q[i + (size_t)ldq], (double)q[i + 2 * (size_t)ldq], empty, p);
#pragma unroll
    for (int j = 0; j < 3; ++j) tq[s + (size_t)j * n_slots] = p[j];
}

// ---- C3. the walk -------------------------------------------------------------------------------------------------------
// range_walk_kernel's shape (knn_range.hip): workgroup (block qb, part p) owns slots qb * 512 + p * 64 + (tid >> 2), lane sub of
// a query scores rows sub, sub + 4, .. of every visited tile.  A tile is skipped by DESIGN 4.1's rule with D = r2 and the block's
// box: every row of a skipped tile has a computed d > r2 for every query of the block, so it holds no answer.  A lane admits
// d <= bnd, bnd = r2 until its first hit and its best d afterwards (still inclusive: an equal d with a lower row must win).
// best[slot's query] = the d of a hit, NaN for a miss (a hit's d is never NaN; with r2 = +inf it may be +inf).
// XYZ (the refit): the lane holds the row's float4 when it wins, so the winner's coordinates travel with (d, row) through the
// lane's updates and the two shuffles into win [3][Q] -- no gather through the inverse of perm afterwards.  A miss's are 0.
template <bool XYZ>
__global__ __launch_bounds__(kBlock) void score_walk_kernel(const float* __restrict__ q, int Q, const int32_t* __restrict__ qperm,
                                                            const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                            const float* __restrict__ tbox, int n_tiles, int cull, float r2,
                                                            float* __restrict__ best, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                            float* __restrict__ win, unsigned long long* __restrict__ stats) {
    __shared__ WalkLds lds;
    __shared__ float s_red[kBlock / 64][6];
    __shared__ float s_box[6];
    const int tid = threadIdx.x;
    const int qb = blockIdx.x / kWalkWgPerBlock, part = blockIdx.x % kWalkWgPerBlock;
    walk_block_box<6>(s_red, s_box, q, Q, Q, qperm, nullptr, qb);
    walk_count_search(stats, (unsigned long long)((Q + kWalkQBlock - 1) / kWalkQBlock) * (unsigned long long)n_tiles);
    const int sub = tid & (kWalkLanes - 1), ql = tid / kWalkLanes;
    const int slot = qb * kWalkQBlock + part * kWalkQPerWg + ql;
    const bool live = slot < Q;
    const int qi = live ? qperm[slot] : 0;
    const float qx = q[qi], qy = q[qi + (size_t)Q], qz = q[qi + 2 * (size_t)Q];
    float bnd = live ? r2 : -1.0f;                                // (a dead lane admits nothing: d is never negative)
    float bd = INFINITY; int br = INT_MAX;                        // the lane's best; br == INT_MAX: none yet
    float bx = 0.0f, by = 0.0f, bz = 0.0f;                        // XYZ: its coordinates
    walk_tiles(
        lds, 0, n_tiles, qx, qy, qz, part == 0 ? stats : nullptr,
        [&](int ct) {
            return !(cull != 0 && r2 < INFINITY && cull_skips(cull_gap2(tbox + (size_t)ct * 6, tbox + (size_t)ct * 6 + 3, s_box, s_box + 3), r2));
        },
        [&](int r) { return walk_row(ms, perm, M, r); },
        [](int) {},
        [&](int, const float4 (&p)[4], float (&d)[4]) {
            if (fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= bnd) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int row = __float_as_int(p[u].w);
                    if (d[u] <= bnd && (d[u] < bd || row < br)) {
                        bd = d[u]; br = row; bnd = bd;
                        if constexpr (XYZ) { bx = p[u].x; by = p[u].y; bz = p[u].z; }
                    }
                }
            }
        },
        [] {});
#pragma unroll
    for (int o = 1; o < kWalkLanes; o <<= 1) {
        const float od = __shfl_xor(bd, o);
        const int orow = __shfl_xor(br, o);
        if constexpr (XYZ) {
            const float ox = __shfl_xor(bx, o), oy = __shfl_xor(by, o), oz = __shfl_xor(bz, o);
            if (od < bd || (od == bd && orow < br)) { bx = ox; by = oy; bz = oz; }
        }
        if (od < bd || (od == bd && orow < br)) { bd = od; br = orow; }
    }
    if (live && sub == 0) {
        const bool hit = br != INT_MAX;
        best[qi] = hit ? bd : __int_as_float(0x7FC00000);
        if (idx) idx[qi] = hit ? br : -1;
        if (dist) dist[qi] = hit ? bd : INFINITY;
        if constexpr (XYZ) { win[qi] = bx; win[qi + (size_t)Q] = by; win[qi + 2 * (size_t)Q] = bz; }
    }
}

// every (transform, query) of a model without rows: a miss
__global__ __launch_bounds__(kBlock) void score_miss_kernel(size_t n, int32_t* __restrict__ idx, float* __restrict__ dist) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        if (idx) idx[i] = -1;
        if (dist) dist[i] = INFINITY;
    }
}

// ---- C4. count and sum --------------------------------------------------------------------------------------------------
// workgroup bl * chunks + c: queries c * 2048 .. of the batch's transform bl.  Thread t adds its kScanPer consecutive queries in
// query order, then chunk_sum's tree (chunk_scan.hpp): one fixed order per chunk, whatever the batch
__global__ __launch_bounds__(kBlock) void score_reduce_kernel(const float* __restrict__ best, int Q, int chunks, double* __restrict__ psum,
                                                              int32_t* __restrict__ pcnt) {
    const int bl = blockIdx.x / chunks, c = blockIdx.x - bl * chunks;
    const int i0 = c * kScanChunk + threadIdx.x * kScanPer;
    double sum = 0.0; int32_t cnt = 0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        if (i0 + u < Q) {
            const float d = best[(size_t)bl * Q + i0 + u];
            if (d == d) { sum += (double)d; ++cnt; }
        }
    }
    chunk_sum(sum, psum);
    chunk_sum(cnt, pcnt);
}
// thread bl: transform bl's chunks in ascending order
__global__ __launch_bounds__(kBlock) void score_total_kernel(const double* __restrict__ psum, const int32_t* __restrict__ pcnt, int nb, int chunks,
                                                             int32_t* __restrict__ n_close, double* __restrict__ sum_d2) {
    const int bl = blockIdx.x * kBlock + threadIdx.x;
    if (bl >= nb) return;
    double sum = 0.0; int32_t cnt = 0;
    for (int c = 0; c < chunks; ++c) { sum += psum[(size_t)bl * chunks + c]; cnt += pcnt[(size_t)bl * chunks + c]; }
    n_close[bl] = cnt;
    sum_d2[bl] = sum;
}

// ---- C5. the refit's moments --------------------------------------------------------------------------------------------
// workgroup bl * chunks + c, as score_reduce_kernel: thread t adds the hits among its kScanPer consecutive queries in query order
// into mom_accumulate's 27 sums (moments.hpp) of p = (model row, moved point), both widened to double; then chunk_tail
// (refit_step.hpp).  The shifted sums are taken about ONE origin for both sides, the same for
// every chunk, batch and call on a model: the middle of the model's box (Prep::cx, cy, cz), which the moved points lie around
// when the transform is any good.  (The shift only keeps digits; fit_moments adds it back.)
__global__ __launch_bounds__(kBlock) void refit_moments_kernel(const float* __restrict__ best, const float* __restrict__ tq, const float* __restrict__ win,
                                                               int Q, int S, int chunks, const Prep* __restrict__ prep, double* __restrict__ pmom) {
    const int bl = blockIdx.x / chunks, c = blockIdx.x - bl * chunks;
    const int i0 = c * kScanChunk + threadIdx.x * kScanPer;
    const double ox = (double)prep->cx, oy = (double)prep->cy, oz = (double)prep->cz;
    const double o[6] = {ox, oy, oz, ox, oy, oz};
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        if (i0 + u < Q) {
            const size_t s = (size_t)bl * Q + i0 + u;
            const float d = best[s];
            if (d == d) {
                const double p[6] = {(double)win[s], (double)win[s + (size_t)S], (double)win[s + 2 * (size_t)S],
                                     (double)tq[s],  (double)tq[s + (size_t)S],  (double)tq[s + 2 * (size_t)S]};
                mom_accumulate(acc, p, o);
            }
        }
    }
    chunk_tail<27>(acc, 0.0, pmom);
}
// a call without pairs (Q = 0 or a model without rows): every transform is empty; z: the method's per-transform outputs, or nulls
__global__ __launch_bounds__(kBlock) void refit_empty_kernel(int B, double* __restrict__ T_out, double* __restrict__ T_step, int32_t* __restrict__ empty,
                                                             RefitEmptyOuts z) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < 16 * B) { T_out[i] = 0.0; if (T_step) T_step[i] = 0.0; }
    if (i < B) {
        empty[i] = 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) if (z.d[k]) z.d[k][i] = 0.0;
        if (z.n) z.n[i] = 0;
    }
}

// ---- P5. the plane refit's sums -----------------------------------------------------------------------------------------
// workgroup bl * chunks + c and thread t as refit_moments_kernel.  A hit (best == best) with the winning original row `row` is a
// PLANE PAIR when normals[row], normals[row + ldn], normals[row + 2 ldn] are all finite.  The eight (best, row) loads of a thread
// are issued first (hit_rows) and the 24 gathers they address next, so the dependent loads are in flight together; then, in query
// order and in double on the widened values without contraction: e = p - m, r = (n_x e_x + n_y e_y) + n_z e_z, u = p - o,
// c = u x n, J = (c, n), and the 28 sums by fma -- A_ij (i <= j, row-major), g_i = J_i r, rr.  chunk_tail; the number of plane
// pairs through chunk_sum.
__global__ __launch_bounds__(kBlock) void plane_moments_kernel(const float* __restrict__ best, const float* __restrict__ tq, const float* __restrict__ win,
                                                               const int32_t* __restrict__ prow, const float* __restrict__ normals, int ldn, int M, int Q,
                                                               int S, int chunks, const Prep* __restrict__ prep, double* __restrict__ psums,
                                                               int32_t* __restrict__ pplane) {
    const int bl = blockIdx.x / chunks, c = blockIdx.x - bl * chunks;
    const int i0 = c * kScanChunk + threadIdx.x * kScanPer;
    const double ox = (double)prep->cx, oy = (double)prep->cy, oz = (double)prep->cz;
    int row[kScanPer];
    hit_rows(best, prow, bl, i0, Q, M, row);
    float nx[kScanPer], ny[kScanPer], nz[kScanPer];
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const int r = row[u] >= 0 ? row[u] : 0;
        const float qnan = __int_as_float(0x7FC00000);
        nx[u] = row[u] >= 0 ? normals[r] : qnan;
        ny[u] = row[u] >= 0 ? normals[r + (size_t)ldn] : qnan;
        nz[u] = row[u] >= 0 ? normals[r + 2 * (size_t)ldn] : qnan;
    }
    double acc[27], rr = 0.0;
    int32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const double n0 = (double)nx[u], n1 = (double)ny[u], n2 = (double)nz[u];
        if (plane_finite(n0) && plane_finite(n1) && plane_finite(n2)) {       // (a miss's are NaN)
            const size_t s = (size_t)bl * Q + i0 + u;
            const double m0 = (double)win[s], m1 = (double)win[s + (size_t)S], m2 = (double)win[s + 2 * (size_t)S];
            const double p0 = (double)tq[s], p1 = (double)tq[s + (size_t)S], p2 = (double)tq[s + 2 * (size_t)S];
            const double e0 = p0 - m0, e1 = p1 - m1, e2 = p2 - m2;
            const double r = (n0 * e0 + n1 * e1) + n2 * e2;
            const double u0 = p0 - ox, u1 = p1 - oy, u2 = p2 - oz;
            const double J[6] = {u1 * n2 - u2 * n1, u2 * n0 - u0 * n2, u0 * n1 - u1 * n0, n0, n1, n2};
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = i; j < 6; ++j) acc[plane_tri(i, j)] = fma(J[i], J[j], acc[plane_tri(i, j)]);
                acc[21 + i] = fma(J[i], r, acc[21 + i]);
            }
            rr = fma(r, r, rr);
            ++cnt;
        }
    }
    chunk_tail<kPlaneSums>(acc, rr, psums);
    chunk_sum(cnt, pplane);
}

// ---- G5. the plane-to-plane refit's sums --------------------------------------------------------------------------------
// workgroup bl * chunks + c and thread t as plane_moments_kernel, and its first step: hit_rows.  The 24 gathers of model normals
// they address and the thread's 24 query-normal loads are issued together next.  Then, in query order and in double on the
// widened values without contraction: gicp_pair (gicp_pair.hpp) gives W or drops the pair; e = p - m, u = p - o, and info_pair's
// terms (info_pair.hpp) with C := W and x := e, unweighted: A_ij (i <= j, row-major), g_i, and e . (W e) in the 28th place.
// chunk_tail; the number of pairs through chunk_sum.
__global__ __launch_bounds__(kBlock) void gicp_moments_kernel(const float* __restrict__ best, const float* __restrict__ tq, const float* __restrict__ win,
                                                              const int32_t* __restrict__ prow, const float* __restrict__ normals, int ldn, int M,
                                                              const float* __restrict__ qnormals, int ldnq, const double* __restrict__ T, double a, int Q,
                                                              int S, int chunks, const Prep* __restrict__ prep, double* __restrict__ psums,
                                                              int32_t* __restrict__ ppairs) {
    const int bl = blockIdx.x / chunks, c = blockIdx.x - bl * chunks;
    const int i0 = c * kScanChunk + threadIdx.x * kScanPer;
    const double o[3] = {(double)prep->cx, (double)prep->cy, (double)prep->cz};
    const double* __restrict__ Tb = T + (size_t)bl * 16;
    int row[kScanPer];
    hit_rows(best, prow, bl, i0, Q, M, row);
    float nm[kScanPer][3], nq[kScanPer][3];
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const int r = row[u] >= 0 ? row[u] : 0;
        const int i = row[u] >= 0 ? i0 + u : 0;                       // (a hit's query is below Q)
        const float qnan = __int_as_float(0x7FC00000);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            nm[u][k] = row[u] >= 0 ? normals[r + k * (size_t)ldn] : qnan;
            nq[u][k] = row[u] >= 0 ? qnormals[i + k * (size_t)ldnq] : qnan;
        }
    }
    double acc[27], rr = 0.0;
    int32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        double C[6];
        if (!gicp_pair(nm[u], nq[u], Tb, a, C)) continue;             // (a miss's normals are NaN)
        const size_t s = (size_t)bl * Q + i0 + u;
        const double m0 = (double)win[s], m1 = (double)win[s + (size_t)S], m2 = (double)win[s + 2 * (size_t)S];
        const double p0 = (double)tq[s], p1 = (double)tq[s + (size_t)S], p2 = (double)tq[s + 2 * (size_t)S];
        const double x[3] = {p0 - m0, p1 - m1, p2 - m2};
        const double uu[3] = {p0 - o[0], p1 - o[1], p2 - o[2]};
        double y[3], qq;
        info_pair<false>(C, x, uu, 1.0, acc, y, qq);
        rr = rr + qq;
        ++cnt;
    }
    chunk_tail<kPlaneSums>(acc, rr, psums);
    chunk_sum(cnt, ppairs);
}

// ---- P6. the plane refit's fit ------------------------------------------------------------------------------------------
// finish_step (refit_step.hpp) over the 28 sums and the plane counts: plane_fit about the origin the sums were taken about,
// unless T_in is all zero
__global__ __launch_bounds__(64) void plane_finish_kernel(const double* __restrict__ psums, const int32_t* __restrict__ pplane, int chunks,
                                                          const Prep* __restrict__ prep, const double* __restrict__ T_in, double* __restrict__ T_out,
                                                          double* __restrict__ T_step, int32_t* __restrict__ n_plane, double* __restrict__ sum_res2,
                                                          int32_t* __restrict__ empty) {
    const bool in_empty = transform_is_zero(T_in, blockIdx.x);
    const double o[3] = {(double)prep->cx, (double)prep->cy, (double)prep->cz};
    double sums[kPlaneSums];
    int cnt;
    finish_step<kPlaneSums, true>(psums, pplane, chunks, T_in, T_out, T_step, empty,
                                  [&](const double (&s)[kPlaneSums], int n, double (&T)[16]) { return !in_empty && plane_fit(s, n, o, T); }, sums, cnt);
    if (threadIdx.x == 0) { n_plane[blockIdx.x] = cnt; sum_res2[blockIdx.x] = sums[27]; }
}

// whole transforms per batch under a cap of `slots` query slots (at least one: Q <= kScoreMaxSlots)
int score_batch(int Q, int B, int slots) {
    const int per = slots / (Q > 0 ? Q : 1);
    return std::max(1, std::min(B, per));
}

// Workspace, S = max(nb Q, 1) slots and P = nb max(ceil(Q / 2048), 1) partials of a full batch of nb = max(1, min(B, floor(4 Mi /
// max(Q, 1)))) transforms: [per-parent-cell counters] [transformed queries, 3 S] [slot -> query, S] [best d per slot, S]
// [chunk sums, P] [chunk counts, P]:
// 131 328 + roundup(12 S, 256) + 2 roundup(4 S, 256) + roundup(8 P, 256) + roundup(4 P, 256) bytes
// The refit's is that followed by [winning rows' coordinates, 3 S] [chunk moments, 27 P]: + roundup(12 S, 256) + roundup(216 P, 256)
// The plane refit's is the refit's with 28 chunk sums instead of 27, followed by [winning row per slot, S] [chunk plane counts, P]:
// + roundup(12 S, 256) + roundup(224 P, 256) + roundup(4 S, 256) + roundup(4 P, 256)
// The plane-to-plane refit needs nothing more: it runs in the plane refit's layout, its pair counts in the plane counts' place.
// A trimmed call runs in its method's layout as it is: between the walk and the sums the per-parent-cell counters
// and the slot -> query block are dead, and the chunk counts are not written yet.  Its digit counters and select states (1040 bytes
// a transform) go into the larger of the first two, `trim_cap` transforms at a time (at least 126: 131 328 / 1040), its chunk tie
// counts into the chunk counts' place.
enum ScoreMode { kModeScore = 0, kModeRefit = 1, kModePlane = 2 };
struct ScoreWs { int32_t* qcnt; float* tq; int32_t* qperm; float* best; double* psum; int32_t* pcnt; float* win; double* pmom; int32_t* prow; int32_t* pplane;
                 char* trim_at; int trim_cap; };
constexpr size_t kTrimPer = 1024 + kTrimSelBytes;    // a transform's 256 digit counters and its select state
ScoreWs score_ws_layout(int Q, int B, ScoreMode mode, void* base, size_t* bytes) {
    ScoreWs s{};
    const int nb = score_batch(Q, B, kScoreMaxSlots);
    const size_t S = std::max((size_t)nb * (size_t)(Q > 0 ? Q : 0), (size_t)1), P = (size_t)nb * scan_chunks(Q);
    WsWalk w(base);
    s.qcnt = (int32_t*)w.take_bytes((size_t)kQueryKeys * 4 + 256);
    s.tq = w.take<float>(3 * S);
    s.qperm = w.take<int32_t>(S);
    s.best = w.take<float>(S);
    s.psum = w.take<double>(P);
    s.pcnt = w.take<int32_t>(P);
    if (mode != kModeScore) {
        s.win = w.take<float>(3 * S);
        s.pmom = w.take<double>((mode == kModePlane ? (size_t)kPlaneSums : (size_t)27) * P);
    }
    if (mode == kModePlane) {
        s.prow = w.take<int32_t>(S);
        s.pplane = w.take<int32_t>(P);
    }
    const size_t cells = (size_t)kQueryKeys * 4 + 256, order = align_up(S * sizeof(int32_t), (size_t)256);
    s.trim_at = order > cells ? (char*)s.qperm : (char*)s.qcnt;
    s.trim_cap = (int)std::min(std::max(order, cells) / kTrimPer, (size_t)nb);
    *bytes = w.bytes();
    return s;
}

// what the refit adds to a scoring call: the outputs per transform (T_step may be null)
struct RefitOut { double* T_out; double* T_step; int32_t* empty; };
// ... and what the plane refit takes and gives beyond that: a normal per ORIGINAL row, the plane pairs and their squared residuals
struct PlaneIo { const float* normals; int ldn; int32_t* n_plane; double* sum_res2; };
// ... and the plane-to-plane refit beyond that (with `plane`, whose n_plane then counts its pairs): a normal per query, 1 - epsilon
struct GicpIo { const float* qnormals; int ldnq; double a; };

// the chain of every call; `refit` null: scoring; `plane` (with refit) non-null: the point-to-plane fit instead of estimateTransform;
// `gicp` (with plane) non-null: the plane-to-plane sums instead of the point-to-plane ones, in the same workspace
int score_chain(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, float r2, int32_t* n_close, double* sum_d2,
                int32_t* idx, float* dist, const RefitOut* refit, const PlaneIo* plane, const GicpIo* gicp, const TrimIo* trim, void* ws,
                size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxSlots && r2 >= 0.0f);
    PCREG_ARG(!trim || (trim->keep_ratio > 0.0 && trim->keep_ratio <= 1.0));          // (a NaN fails both)
    size_t need;
    const ScoreWs s = score_ws_layout(Q, B, plane ? kModePlane : refit ? kModeRefit : kModeScore, ws, &need);
    if (ws_bytes < need) {
        set_error("bad argument: %s workspace too small: %zu < %zu", gicp ? "plane-to-plane refit" : plane ? "plane refit" : refit ? "refit" : "score", ws_bytes, need);
        return PCREG_E_ARG;
    }
    if (B == 0) return PCREG_OK;
    if (Q == 0 || v.M == 0) {                                     // every query misses
        PCREG_HIP(hipMemsetAsync(n_close, 0, sizeof(int32_t) * (size_t)B, st));
        PCREG_HIP(hipMemsetAsync(sum_d2, 0, sizeof(double) * (size_t)B, st));
        const size_t n = (size_t)B * Q;
        if (n > 0 && (idx || dist)) {
            hipLaunchKernelGGL(score_miss_kernel, dim3((unsigned)std::min((n + kBlock - 1) / kBlock, (size_t)4096)), dim3(kBlock), 0, st, n, idx, dist);
            PCREG_HIP(hipGetLastError());
        }
        if (refit) {
            RefitEmptyOuts z{};
            if (plane) { z.d[0] = plane->sum_res2; z.n = plane->n_plane; }
            int rc = launch_refit_empty(B, refit->T_out, refit->T_step, refit->empty, z, st);
            if (rc) return rc;
        }
        return trim ? launch_trim_empty(B, trim->n_within, trim->d2_cut, st) : PCREG_OK;
    }
    int32_t* const user_idx = idx;                                // (the trim writes misses into the CALLER's tables only)
    if (plane) idx = s.prow;                                      // the winning row per slot of ONE batch (S entries: only the walk may write it)
    const int dbg_slots = debug_flag(kDbgScoreBatchSlots);        // "score_batch_slots": a lower cap, same results
    const int nb_max = score_batch(Q, B, dbg_slots > 0 ? std::min(dbg_slots, kScoreMaxSlots) : kScoreMaxSlots);
    const int n_tiles = (v.M + kT16 - 1) / kT16, chunks = scan_chunks(Q);
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;          // "knn_nocull": visit every tile, same bits
    for (int b0 = 0; b0 < B; b0 += nb_max) {
        const int nb = std::min(nb_max, B - b0), S = nb * Q;
        const size_t at = plane ? 0 : (size_t)b0 * Q;             // (the caller's [B][Q] tables take the batch at b0; the workspace block is per batch)
        hipLaunchKernelGGL(score_transform_kernel, dim3((S + kBlock - 1) / kBlock), dim3(kBlock), 0, st, q, Q, ldq, T_dev + (size_t)b0 * 16, S, s.tq);
        int rc = launch_query_cells(v, s.tq, S, S, s.qcnt, st);
        if (!rc) rc = launch_query_order(v, s.tq, S, S, s.qcnt, s.qperm, st);
        if (rc) return rc;
        const dim3 walk_grid((unsigned)(((S + kWalkQBlock - 1) / kWalkQBlock) * kWalkWgPerBlock));
        if (refit)
            hipLaunchKernelGGL(score_walk_kernel<true>, walk_grid, dim3(kBlock), 0, st, (const float*)s.tq, S, (const int32_t*)s.qperm, (const float*)v.ms,
                               (const int32_t*)v.perm, v.M, (const float*)v.tbox, n_tiles, cull, r2, s.best, idx ? idx + at : nullptr,
                               dist ? dist + at : nullptr, s.win, knn_stats_dev());
        else
            hipLaunchKernelGGL(score_walk_kernel<false>, walk_grid, dim3(kBlock), 0, st, (const float*)s.tq, S, (const int32_t*)s.qperm, (const float*)v.ms,
                               (const int32_t*)v.perm, v.M, (const float*)v.tbox, n_tiles, cull, r2, s.best, idx ? idx + at : nullptr,
                               dist ? dist + at : nullptr, (float*)nullptr, knn_stats_dev());
        if (trim) {                                               // the kept pairs stay hits, the others become misses (knn_trim.hip)
            PCREG_HIP(hipGetLastError());
            for (int t0 = 0; t0 < nb; t0 += s.trim_cap) {       // (one round wherever a transform has 260 queries or more)
                const int nt = std::min(s.trim_cap, nb - t0);
                const size_t o = (size_t)t0 * Q;
                rc = launch_score_trim(s.best + o, Q, chunks, nt, trim->keep_ratio, (int32_t*)s.trim_at, s.trim_at + 1024 * (size_t)nt,
                                       s.pcnt + (size_t)t0 * chunks, user_idx ? user_idx + at + o : nullptr, dist ? dist + at + o : nullptr,
                                       trim->n_within ? trim->n_within + b0 + t0 : nullptr, trim->d2_cut ? trim->d2_cut + b0 + t0 : nullptr, st);
                if (rc) return rc;
            }
        }
        hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)(nb * chunks)), dim3(kBlock), 0, st, (const float*)s.best, Q, chunks, s.psum, s.pcnt);
        hipLaunchKernelGGL(score_total_kernel, dim3((nb + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const double*)s.psum, (const int32_t*)s.pcnt, nb,
                           chunks, n_close + b0, sum_d2 + b0);
        if (plane) {
            if (gicp)
                hipLaunchKernelGGL(gicp_moments_kernel, dim3((unsigned)(nb * chunks)), dim3(kBlock), 0, st, (const float*)s.best, (const float*)s.tq,
                                   (const float*)s.win, (const int32_t*)s.prow, plane->normals, plane->ldn, v.M, gicp->qnormals, gicp->ldnq,
                                   T_dev + (size_t)b0 * 16, gicp->a, Q, S, chunks, (const Prep*)v.prep, s.pmom, s.pplane);
            else
                hipLaunchKernelGGL(plane_moments_kernel, dim3((unsigned)(nb * chunks)), dim3(kBlock), 0, st, (const float*)s.best, (const float*)s.tq,
                                   (const float*)s.win, (const int32_t*)s.prow, plane->normals, plane->ldn, v.M, Q, S, chunks, (const Prep*)v.prep,
                                   s.pmom, s.pplane);
            PCREG_HIP(hipGetLastError());
            hipLaunchKernelGGL(plane_finish_kernel, dim3(nb), dim3(64), 0, st, (const double*)s.pmom, (const int32_t*)s.pplane, chunks, (const Prep*)v.prep,
                               T_dev + (size_t)b0 * 16, refit->T_out + (size_t)b0 * 16, refit->T_step ? refit->T_step + (size_t)b0 * 16 : nullptr,
                               plane->n_plane + b0, plane->sum_res2 + b0, refit->empty + b0);
        } else if (refit) {
            hipLaunchKernelGGL(refit_moments_kernel, dim3((unsigned)(nb * chunks)), dim3(kBlock), 0, st, (const float*)s.best, (const float*)s.tq,
                               (const float*)s.win, Q, S, chunks, (const Prep*)v.prep, s.pmom);
            PCREG_HIP(hipGetLastError());
            rc = launch_refit_finish(s.pmom, n_close + b0, s.best, s.tq, s.win, Q, S, chunks, nb, &((const Prep*)v.prep)->cx, T_dev + (size_t)b0 * 16,
                                     refit->T_out + (size_t)b0 * 16, refit->T_step ? refit->T_step + (size_t)b0 * 16 : nullptr, refit->empty + b0, st);
            if (rc) return rc;
        }
        PCREG_HIP(hipGetLastError());
    }
    return PCREG_OK;
}

}  // namespace

size_t score_ws_bytes(int Q, int B, int M) {
    (void)M;                                       // O(min(B Q, 4 Mi)) bytes, whatever M, r2 and the result
    if (Q < 0 || B < 0 || Q > kScoreMaxSlots) return 0;
    size_t b; (void)score_ws_layout(Q, B, kModeScore, nullptr, &b);
    return b;
}
size_t refit_ws_bytes(int Q, int B, int M) {
    (void)M;
    if (Q < 0 || B < 0 || Q > kScoreMaxSlots) return 0;
    size_t b; (void)score_ws_layout(Q, B, kModeRefit, nullptr, &b);
    return b;
}
size_t refit_plane_ws_bytes(int Q, int B, int M) {
    (void)M;
    if (Q < 0 || B < 0 || Q > kScoreMaxSlots) return 0;
    size_t b; (void)score_ws_layout(Q, B, kModePlane, nullptr, &b);
    return b;
}

int launch_refit_empty(int B, double* T_out, double* T_step, int32_t* empty, const RefitEmptyOuts& z, hipStream_t st) {
    hipLaunchKernelGGL(refit_empty_kernel, dim3((unsigned)((16 * (size_t)B + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, B, T_out, T_step, empty, z);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

int launch_model_score(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, float r2, int32_t* n_close,
                       double* sum_d2, int32_t* idx, float* dist, void* ws, size_t ws_bytes, hipStream_t st, const TrimIo* trim) {
    return score_chain(v, q, Q, ldq, T_dev, B, r2, n_close, sum_d2, idx, dist, nullptr, nullptr, nullptr, trim, ws, ws_bytes, st);
}

int launch_model_refit(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, float r2, double* T_out, double* T_step,
                       int32_t* n_close, double* sum_d2, int32_t* empty, void* ws, size_t ws_bytes, hipStream_t st, const TrimIo* trim) {
    const RefitOut out{T_out, T_step, empty};
    return score_chain(v, q, Q, ldq, T_dev, B, r2, n_close, sum_d2, nullptr, nullptr, &out, nullptr, nullptr, trim, ws, ws_bytes, st);
}

int launch_model_refit_plane(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, float r2, const float* normals, int ldn,
                             double* T_out, double* T_step, int32_t* n_close, double* sum_d2, int32_t* n_plane, double* sum_res2, int32_t* empty,
                             void* ws, size_t ws_bytes, hipStream_t st, const TrimIo* trim) {
    PCREG_ARG(ldn >= v.M && (normals || v.M == 0));
    const RefitOut out{T_out, T_step, empty};
    const PlaneIo plane{normals, ldn, n_plane, sum_res2};
    return score_chain(v, q, Q, ldq, T_dev, B, r2, n_close, sum_d2, nullptr, nullptr, &out, &plane, nullptr, trim, ws, ws_bytes, st);
}

// the plane refit's workspace, as it is: the same slots and partials, with the pairs' count in the plane count's place
size_t refit_gicp_ws_bytes(int Q, int B, int M) { return refit_plane_ws_bytes(Q, B, M); }

int launch_model_refit_gicp(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, float r2, const float* normals, int ldn,
                            const float* qnormals, int ldnq, double epsilon, double* T_out, double* T_step, int32_t* n_close, double* sum_d2,
                            int32_t* n_pairs, double* sum_res2, int32_t* empty, void* ws, size_t ws_bytes, hipStream_t st, const TrimIo* trim) {
    PCREG_ARG(ldn >= v.M && (normals || v.M == 0) && Q >= 0 && ldnq >= Q && (qnormals || Q == 0) && epsilon > 0.0 && epsilon <= 1.0);
    const RefitOut out{T_out, T_step, empty};
    const PlaneIo plane{normals, ldn, n_pairs, sum_res2};
    const GicpIo gicp{qnormals, ldnq, 1.0 - epsilon};
    return score_chain(v, q, Q, ldq, T_dev, B, r2, n_close, sum_d2, nullptr, nullptr, &out, &plane, &gicp, trim, ws, ws_bytes, st);
}

}  // namespace pcreg
