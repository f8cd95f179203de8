// pcreg_amd/csrc/ndt.hip -- the normal-distributions transform: a cloud summarised as one Gaussian per occupied voxel, and ONE
// Gauss-Newton step of B candidate transforms of a query cloud against that table.  The contract is pcreg_ndt's (include/pcreg.h);
// DESIGN 4.25.  A step needs no nearest-row walk: a moved point looks its voxel up in a sorted key array.
//
// THE TABLE (ndt_build; one-off, it reads two words back between its launches to size its buffers):
//   N1  launch_voxel_order        downsample.hip's D1 .. D6, unchanged: the rows ordered by voxel, the first record of every voxel
//   N2  ndt_gauss_kernel          in D7's place: thread v walks voxel v's sorted members in order -- ndt_gauss (ndt_gauss.hpp) gathers
//                                 them twice -- and writes the voxel's record and whether it holds a Gaussian
//   N3  ndt_count_kernel,         the chunk scan's compaction (chunk_scan.hpp) of the Gaussian voxels, ascending: record and key of
//       ndt_emit_kernel           Gaussian g; the last thread writes their number
// THE STEP (launch_ndt_refit; nothing is read on the host, no kernel waits for another workgroup):
//   S1  ndt_moments_kernel        per (transform, chunk of 2048 queries), thread t owns 8 consecutive queries: the moved points
//                                 (moved_point), the lookups, the pairs' 28 sums in (query, candidate) order (info_pair.hpp,
//                                 weighted), chunk_tail; the number of pairs through chunk_sum
//   S2  ndt_finish_kernel         per transform: finish_step with plane_fit (plane_fit.hpp) about the table's origin
// The step's skeleton -- the moved point, the chunk tail, the finish step, T * T_step and the empty rule -- is refit_step.hpp's
// (DESIGN 4.28).
// Integer adds and fp64 sums in one fixed tree only: no floating-point atomic, no result depends on the order in which
// workgroups run, the stream or what the workspace held.  There is no batching: the workspace is B x chunks partial sums.
#include "common.hpp"
#include "refit_step.hpp"
#include "plane_fit.hpp"
#include "info_pair.hpp"
#include "ndt_gauss.hpp"
#include <cmath>

namespace pcreg {

namespace {

typedef unsigned long long u64;
constexpr int kNdtBlock = 256;
constexpr double kNdtMaxCells = 2097152.0;           // 2^21 cells per axis: the grid's refusal, and the range of a candidate's cell
static_assert(kScanBlock == kNdtBlock && kScanPer == 8, "ndt_moments_kernel's threads own kScanPer consecutive queries each");
static_assert(sizeof(NdtRec) == 128, "one record, one line");

__device__ __forceinline__ u64 ndt_key(long long c0, long long c1, long long c2) { return ((u64)c0 << 42) | ((u64)c1 << 21) | (u64)c2; }
// pcreg_downsample_grid_f32's cell: IEEE subtraction and division in double (the file is built without contraction)
__device__ __forceinline__ double ndt_cell(float x, float lo, double step) { return floor(((double)x - (double)lo) / step); }

// ---- N2 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNdtBlock) void ndt_gauss_kernel(const float* __restrict__ pts, int ld, VoxelOrder ord, int n_vox, double step,
                                                              int min_points, NdtRec* __restrict__ rec, int32_t* __restrict__ flag) {
    const int v = blockIdx.x * kNdtBlock + threadIdx.x;
    if (v >= n_vox) return;
    const VoxelHdr* __restrict__ hdr = ord.hdr;
    const uint32_t* __restrict__ row = ord.row[hdr->passes & 1];
    const int s = ord.vstart[v], e = v + 1 < n_vox ? ord.vstart[v + 1] : hdr->n_live;
    const int count = e - s;
    NdtRec r{};
    const uint32_t r0 = row[s];                          // every member has the voxel's cell
    r.key = ndt_key((long long)ndt_cell(pts[r0], hdr->lo[0], step), (long long)ndt_cell(pts[r0 + (size_t)ld], hdr->lo[1], step),
                    (long long)ndt_cell(pts[r0 + 2 * (size_t)ld], hdr->lo[2], step));
    r.count = count;
    bool ok = false;
    if (count >= min_points)
        ok = ndt_gauss(count, [&](int i, float& x, float& y, float& z) {
                 const uint32_t ri = row[s + i];
                 x = pts[ri]; y = pts[ri + (size_t)ld]; z = pts[ri + 2 * (size_t)ld];
             }, r.mean, r.C);
    rec[v] = r;
    flag[v] = ok ? 1 : 0;
}

// ---- N3 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNdtBlock) void ndt_count_kernel(const int32_t* __restrict__ flag, int n_vox, int32_t* __restrict__ csum) {
    chunk_pred_count(n_vox, csum, [&](long long v) { return flag[v] != 0; });
}
__global__ __launch_bounds__(kNdtBlock) void ndt_emit_kernel(const int32_t* __restrict__ flag, const NdtRec* __restrict__ rec, int n_vox, int cap,
                                                             const int32_t* __restrict__ csum, u64* __restrict__ keys, NdtRec* __restrict__ out,
                                                             int32_t* __restrict__ n_gauss) {
    const int32_t at = chunk_pred_emit(n_vox, csum, [&](long long v) { return flag[v] != 0; }, [&](int32_t g, long long v) {
        if (g < cap) { out[g] = rec[v]; keys[g] = rec[v].key; }       // (g < cap always: a Gaussian has min_points live rows of its own)
    });
    if (chunk_is_last_thread()) *n_gauss = at;
}

// ---- S1 ---------------------------------------------------------------------------------------------------------------
struct NdtGrid { float lo[3]; float o[3]; double step; int G; };

// workgroup bl * chunks + c: queries c * 2048 .. of transform bl; thread t its 8 consecutive queries, QG at a time.  The group's
// QG * NB lookups run together: a branch-free binary search with a trip count fixed by G, every step's loads in flight at once,
// then the loads of the keys they end on.  The pairs follow in (query, candidate) order.
template <int NB, int QG>
__global__ __launch_bounds__(kNdtBlock) void ndt_moments_kernel(const float* __restrict__ q, int Q, int ldq, const double* __restrict__ T, NdtGrid g,
                                                                const u64* __restrict__ keys, const NdtRec* __restrict__ rec, double half_d2, int chunks,
                                                                double* __restrict__ psums, int32_t* __restrict__ pcnt) {
    const int bl = blockIdx.x / chunks, c = blockIdx.x - bl * chunks;
    const int i0 = c * kScanChunk + threadIdx.x * kScanPer;
    double t[16];
    const bool t_empty = load_transform(T, bl, t);
    const double o[3] = {(double)g.o[0], (double)g.o[1], (double)g.o[2]};
    double acc[27], se = 0.0;
    int32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int grp = 0; grp < kScanPer / QG; ++grp) {
        double p[QG][3];
        u64 want[QG][NB];
        int at[QG][NB];
#pragma unroll
        for (int u = 0; u < QG; ++u) {
            const int i = i0 + grp * QG + u;
            double x = 0.0, y = 0.0, z = 0.0;
            if (i < Q) { x = (double)q[i]; y = (double)q[i + (size_t)ldq]; z = (double)q[i + 2 * (size_t)ldq]; }
            float mp[3];
            moved_point(t, x, y, z, t_empty, mp);
            double cell[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float pf = i < Q ? mp[j] : __int_as_float(0x7FC00000);       // (a slot past Q: no point)
                p[u][j] = (double)pf;
                cell[j] = ndt_cell(pf, g.lo[j], g.step);
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                // candidate 0 the point's own cell, then -x +x -y +y -z +z
                const double c0 = cell[0] + (k == 1 ? -1.0 : k == 2 ? 1.0 : 0.0), c1 = cell[1] + (k == 3 ? -1.0 : k == 4 ? 1.0 : 0.0),
                             c2 = cell[2] + (k == 5 ? -1.0 : k == 6 ? 1.0 : 0.0);
                const bool in = c0 >= 0.0 && c0 < kNdtMaxCells && c1 >= 0.0 && c1 < kNdtMaxCells && c2 >= 0.0 && c2 < kNdtMaxCells;   // (NaN: false)
                want[u][k] = in ? ndt_key((long long)c0, (long long)c1, (long long)c2) : ~0ull;      // (no voxel has the all-ones key)
                at[u][k] = 0;
            }
        }
        for (int n = g.G; n > 1;) {                   // at .. at + n - 1 holds the last key <= want, if any does
            const int half = n >> 1;
#pragma unroll
            for (int u = 0; u < QG; ++u)
#pragma unroll
                for (int k = 0; k < NB; ++k) at[u][k] = keys[at[u][k] + half] <= want[u][k] ? at[u][k] + half : at[u][k];     // at + half < G
            n -= half;
        }
#pragma unroll
        for (int u = 0; u < QG; ++u)
#pragma unroll
            for (int k = 0; k < NB; ++k) at[u][k] = g.G > 0 && keys[at[u][k]] == want[u][k] ? at[u][k] : -1;
#pragma unroll
        for (int u = 0; u < QG; ++u) {
            const double uu[3] = {p[u][0] - o[0], p[u][1] - o[1], p[u][2] - o[2]};
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                if (at[u][k] < 0) continue;
                const NdtRec* __restrict__ r = rec + at[u][k];
                const double C[6] = {r->C[0], r->C[1], r->C[2], r->C[3], r->C[4], r->C[5]};
                const double x[3] = {p[u][0] - r->mean[0], p[u][1] - r->mean[1], p[u][2] - r->mean[2]};
                double y[3];
                const double e = exp(-(half_d2 * info_residual(C, x, y)));
                info_terms<true>(C, y, uu, e, acc);
                se = se + e;
                ++cnt;
            }
        }
    }
    chunk_tail<kPlaneSums>(acc, se, psums);
    chunk_sum(cnt, pcnt);
}

// ---- S2 ---------------------------------------------------------------------------------------------------------------
// finish_step (refit_step.hpp) over the 28 sums and the pair counts: plane_fit about the table's origin, unless T_in is all zero
__global__ __launch_bounds__(64) void ndt_finish_kernel(const double* __restrict__ psums, const int32_t* __restrict__ pcnt, int chunks, NdtGrid g,
                                                        const double* __restrict__ T_in, double* __restrict__ T_out, double* __restrict__ T_step,
                                                        int32_t* __restrict__ n_pairs, double* __restrict__ sum_e, int32_t* __restrict__ empty) {
    const bool in_empty = transform_is_zero(T_in, blockIdx.x);
    const double o[3] = {(double)g.o[0], (double)g.o[1], (double)g.o[2]};
    double sums[kPlaneSums];
    int cnt;
    finish_step<kPlaneSums, true>(psums, pcnt, chunks, T_in, T_out, T_step, empty,
                                  [&](const double (&s)[kPlaneSums], int n, double (&T)[16]) { return !in_empty && plane_fit(s, n, o, T); }, sums, cnt);
    if (threadIdx.x == 0) { n_pairs[blockIdx.x] = cnt; sum_e[blockIdx.x] = sums[27]; }
}

// Workspace of a step, P = B max(ceil(Q / 2048), 1) partials: [chunk sums, 28 P doubles] [chunk pair counts, P]:
// roundup(224 P, 256) + roundup(4 P, 256) bytes
struct NdtStepWs { double* psums; int32_t* pcnt; };
NdtStepWs ndt_step_ws_layout(int Q, int B, void* base, size_t* bytes) {
    NdtStepWs s{};
    const size_t P = (size_t)(B > 0 ? B : 0) * (size_t)scan_chunks(Q);
    WsWalk w(base);
    s.psums = w.take<double>((size_t)kPlaneSums * P);
    s.pcnt = w.take<int32_t>(P);
    *bytes = w.bytes();
    return s;
}

// What the build keeps beside downsample's workspace while it runs, n_vox voxels: a record and a flag per voxel, the chunk sums
struct NdtBuildWs { NdtRec* rec; int32_t* flag; int32_t* csum; };
NdtBuildWs ndt_build_ws_layout(int n_vox, void* base, size_t* bytes) {
    NdtBuildWs s{};
    const size_t nv = (size_t)std::max(n_vox, 1);
    WsWalk w(base);
    s.rec = w.take<NdtRec>(nv);
    s.flag = w.take<int32_t>(nv);
    s.csum = w.take<int32_t>((nv + kScanChunk - 1) / kScanChunk);
    *bytes = w.bytes();
    return s;
}

}  // namespace

int ndt_max_queries() { return 4 << 20; }

bool ndt_d2(double step, double outlier_ratio, double* d2) {
    if (!(outlier_ratio >= 0.0 && outlier_ratio < 1.0) || !(step > 0.0) || !std::isfinite(step)) return false;
    if (outlier_ratio == 0.0) { *d2 = 1.0; return true; }
    const double c1 = 10.0 * (1.0 - outlier_ratio), c2 = outlier_ratio / ((step * step) * step);
    const double d3 = -log(c2), d1 = -log(c1 + c2) - d3;
    const double v = -2.0 * log((-log(c1 * exp(-0.5) + c2) - d3) / d1);
    if (!(v > 0.0) || !std::isfinite(v)) return false;
    *d2 = v;
    return true;
}

size_t ndt_refit_ws_bytes(int Q, int B) {
    if (Q < 0 || B < 0 || Q > ndt_max_queries()) return 0;
    size_t b; (void)ndt_step_ws_layout(Q, B, nullptr, &b);
    return b;
}

// The table of n x 3 fp32 rows on the device; synchronises `st` twice (the voxel count, then the Gaussian count).  On success the
// view owns one device block (view->block).  A refused cloud: PCREG_E_ARG, nothing is kept.
int ndt_build(const float* pts, int n, int ld, double step, int min_points, hipStream_t st, NdtView* view) {
    PCREG_ARG(view && n >= 0 && ld >= n && std::isfinite(step) && step > 0.0 && min_points >= kNdtMinPointsLeast && (n == 0 || pts));
    *view = NdtView{};
    view->step = step;
    view->min_points = min_points;
    const size_t dsb = downsample_grid_ws_bytes(n);
    char* ws = nullptr;
    PCREG_HIP(hipMalloc((void**)&ws, dsb + 256));
    int32_t* word = (int32_t*)(ws + dsb);             // n_vox, info, n_gauss
    VoxelOrder ord{};
    int rc = launch_voxel_order(pts, n, ld, step, word, word + 1, ws, dsb, st, &ord);
    VoxelHdr hdr{};
    int32_t hw[2] = {0, 0};
    hipError_t he = hipSuccess;
    if (!rc) {
        he = hipMemcpyAsync(&hdr, ord.hdr, sizeof hdr, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(hw, word, sizeof hw, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
    }
    if (rc || he != hipSuccess) {
        (void)hipFree(ws);
        if (!rc) { set_error("the NDT table's voxel order failed: %s", hipGetErrorString(he)); rc = PCREG_E_HIP; }
        return rc;
    }
    if (hw[1] != 0) {
        (void)hipFree(ws);
        set_error("bad argument: the cloud spans 2^21 or more cells of this step along an axis");
        return PCREG_E_ARG;
    }
    const int n_vox = hw[0];
    view->n_vox = n_vox;
    if (n_vox == 0) {                                 // no live row: a table without Gaussians, lo and origin 0
        (void)hipFree(ws);
        return PCREG_OK;
    }
    for (int c = 0; c < 3; ++c) { view->lo[c] = hdr.lo[c]; view->o[c] = 0.5f * hdr.lo[c] + 0.5f * hdr.hi[c]; }
    const int cap = std::max(1, std::min(n_vox, hdr.n_live / min_points));
    size_t bb;
    (void)ndt_build_ws_layout(n_vox, nullptr, &bb);
    char *tmp = nullptr, *block = nullptr;
    const size_t keys_bytes = align_up(sizeof(u64) * (size_t)cap, 256);
    he = hipMalloc((void**)&tmp, bb);
    if (he == hipSuccess) he = hipMalloc((void**)&block, keys_bytes + sizeof(NdtRec) * (size_t)cap);
    if (he == hipSuccess) {
        const NdtBuildWs b = ndt_build_ws_layout(n_vox, tmp, &bb);
        u64* keys = (u64*)block;
        NdtRec* rec = (NdtRec*)(block + keys_bytes);
        const int vchunks = (n_vox + kScanChunk - 1) / kScanChunk;
        hipLaunchKernelGGL(ndt_gauss_kernel, dim3((n_vox + kNdtBlock - 1) / kNdtBlock), dim3(kNdtBlock), 0, st, pts, ld, ord, n_vox, step, min_points, b.rec,
                           b.flag);
        hipLaunchKernelGGL(ndt_count_kernel, dim3(vchunks), dim3(kNdtBlock), 0, st, (const int32_t*)b.flag, n_vox, b.csum);
        hipLaunchKernelGGL(ndt_emit_kernel, dim3(vchunks), dim3(kNdtBlock), 0, st, (const int32_t*)b.flag, (const NdtRec*)b.rec, n_vox, cap,
                           (const int32_t*)b.csum, keys, rec, word + 2);
        he = hipGetLastError();
        int32_t ng = 0;
        if (he == hipSuccess) he = hipMemcpyAsync(&ng, word + 2, sizeof ng, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he == hipSuccess) { view->keys = keys; view->rec = rec; view->G = ng; view->block = block; }
    }
    (void)hipFree(tmp);
    (void)hipFree(ws);
    if (he != hipSuccess) {
        (void)hipFree(block);
        *view = NdtView{};
        set_error("the NDT table's build failed: %s", hipGetErrorString(he));
        return PCREG_E_HIP;
    }
    return PCREG_OK;
}

int launch_ndt_refit(const NdtView& v, const float* q, int Q, int ldq, const double* T_dev, int B, int neighbors, double outlier_ratio, double* T_out,
                     double* T_step, int32_t* n_pairs, double* sum_e, int32_t* empty, void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(Q >= 0 && B >= 0 && ldq >= Q && Q <= ndt_max_queries() && (neighbors == 1 || neighbors == 7));
    double d2 = 0.0;
    PCREG_ARG(ndt_d2(v.step, outlier_ratio, &d2));
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T_dev && T_out && n_pairs && sum_e && empty && T_out != T_dev)));
    const int chunks = scan_chunks(Q);
    PCREG_ARG((long long)B * chunks <= 0x7FFFFFFF);
    size_t need;
    const NdtStepWs s = ndt_step_ws_layout(Q, B, ws, &need);
    if (ws_bytes < need || (need > 0 && !ws)) {
        set_error("bad argument: NDT refit workspace too small: %zu < %zu", ws_bytes, need);
        return PCREG_E_ARG;
    }
    if (B == 0) return PCREG_OK;
    NdtGrid g{};
    for (int c = 0; c < 3; ++c) { g.lo[c] = v.lo[c]; g.o[c] = v.o[c]; }
    g.step = v.step;
    g.G = v.G;
    const dim3 grid((unsigned)(B * chunks)), block(kNdtBlock);
    if (neighbors == 1)
        hipLaunchKernelGGL((ndt_moments_kernel<1, 4>), grid, block, 0, st, q, Q, ldq, T_dev, g, (const u64*)v.keys, (const NdtRec*)v.rec, d2 / 2.0, chunks,
                           s.psums, s.pcnt);
    else
        hipLaunchKernelGGL((ndt_moments_kernel<7, 1>), grid, block, 0, st, q, Q, ldq, T_dev, g, (const u64*)v.keys, (const NdtRec*)v.rec, d2 / 2.0, chunks,
                           s.psums, s.pcnt);
    PCREG_HIP(hipGetLastError());
    hipLaunchKernelGGL(ndt_finish_kernel, dim3(B), dim3(64), 0, st, (const double*)s.psums, (const int32_t*)s.pcnt, chunks, g, T_dev, T_out, T_step,
                       n_pairs, sum_e, empty);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
