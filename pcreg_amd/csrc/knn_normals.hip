// pcreg_amd/csrc/knn_normals.hip -- the surface normal of every row of a PREPARED model from its k nearest rows
// (3 <= k <= PCREG_KNN_MAX_K).  The contract is pcreg_model_normals_f32's (include/pcreg.h); DESIGN 4.15.
//
// The prepared model (knn_fast.hip) is used as it is: the sorted fp32 copy, perm, the tile boxes.  The queries are the sorted
// copy itself, so there is no query order and no limit on M.  A call is two launches:
//   N1  normals_seed_kernel      (knn_selfjoin.hpp) one wave per sorted row: the k-th smallest distance over the window of 64 consecutive sorted
//                                rows around it (k distinct finite rows lie within that distance: an upper bound of the true
//                                k-th distance; fewer than k finite rows leave +inf).  A non-finite row gets 0: it admits nothing
//   N2  normals_walk_kernel<KB>  selfjoin_klist_walk<KB> (knn_selfjoin.hpp): the (distance, row) k-list walk of tile a's rows
//                                against the tiles on EITHER side of a.  After it every
//                                lane of a row holds the row's list; the epilogue gathers the neighbours by original row from
//                                the model's own array and computes mean, sums, Jacobi, sign in double, all four lanes alike
//                                (no lane waits for another, nothing is shared), and lane 0 stores to the original-row slot
// Nothing is added across threads: the result is a function of (model rows, k, viewpoint) alone.
#include "knn_selfjoin.hpp"
#include "wave_math.hpp"
#include <cmath>

namespace pcreg {

namespace {

// N1, normals_seed_kernel, and the walk of N2 live in knn_selfjoin.hpp.

// ---- N2. the walk and the normal ---------------------------------------------------------------------------------------
// A non-finite row's own lanes admit nothing (its distances are NaN or +inf, its seed is 0): its list stays empty, n = 0.
template <int KB>
__global__ __launch_bounds__(kBlock) void normals_walk_kernel(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                              const float* __restrict__ m, int ldm, const float* __restrict__ tbox,
                                                              int n_tiles, int cull, int k, const float* __restrict__ dk, int has_vp,
                                                              double vx, double vy, double vz, float* __restrict__ normals, int ldn,
                                                              float* __restrict__ variation, unsigned long long* __restrict__ stats) {
    float ld[KB]; int li[KB];
    const WalkSelfRow q = selfjoin_klist_walk<KB>(ms, perm, M, tbox, n_tiles, cull, k, dk, stats, ld, li);
    const int row_i = q.row_i;

    // ---- the epilogue: every lane of the row holds the row's list, (distance, row) ascending ----
    // n: the neighbours found -- the first k entries that are a row at a finite distance (they form a prefix of the list)
    int n = 0;
#pragma unroll
    for (int s = 0; s < KB; ++s) n += (s < k && li[s] >= 0 && ld[s] < INFINITY) ? 1 : 0;
    constexpr int kChunk = KB < 8 ? KB : 8;                       // (a chunk past k is skipped: k is uniform)
    // 1. the mean: sums in list order
    double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
    for (int s0 = 0; s0 < KB; s0 += kChunk) {
        if (s0 < k) {
#pragma unroll
            for (int s = s0; s < s0 + kChunk; ++s) {
                const bool on = s < n;
                const size_t j = (size_t)(on ? li[s] : row_i);
                const double x = (double)m[j], y = (double)m[j + (size_t)ldm], z = (double)m[j + 2 * (size_t)ldm];
                sx = on ? sx + x : sx; sy = on ? sy + y : sy; sz = on ? sz + z : sz;
            }
        }
    }
    const double dn = (double)n;
    const double mx = sx / dn, my = sy / dn, mz = sz / dn;
    // 2. the six sums of products of the centred coordinates, in list order, not divided by n
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                 // xx, xy, xz, yy, yz, zz
#pragma unroll
    for (int s0 = 0; s0 < KB; s0 += kChunk) {
        if (s0 < k) {
#pragma unroll
            for (int s = s0; s < s0 + kChunk; ++s) {
                const bool on = s < n;
                const size_t j = (size_t)(on ? li[s] : row_i);
                const double x = (double)m[j] - mx, y = (double)m[j + (size_t)ldm] - my, z = (double)m[j + 2 * (size_t)ldm] - mz;
                a[0] = on ? a[0] + x * x : a[0]; a[1] = on ? a[1] + x * y : a[1]; a[2] = on ? a[2] + x * z : a[2];
                a[3] = on ? a[3] + y * y : a[3]; a[4] = on ? a[4] + y * z : a[4]; a[5] = on ? a[5] + z * z : a[5];
            }
        }
    }
    const float qnan = __int_as_float(0x7FC00000);
    float nx = qnan, ny = qnan, nz = qnan, var = qnan;
    if (n >= 3) {
        // 3. Jacobi; 4. the column of the smallest diagonal entry, ties to the lowest index
        double V[9];
        jacobi_sym3(a, V);
        const double l0 = a[0], l1 = a[3], l2 = a[5];
        int c = 0; double lmin = l0;
        if (l1 < lmin) { c = 1; lmin = l1; }
        if (l2 < lmin) { c = 2; lmin = l2; }
        const double tr = (l0 + l1) + l2;
        if (tr > 0.0) {
            // 5. each component rounded once to fp32
            nx = (float)(c == 0 ? V[0] : c == 1 ? V[1] : V[2]);
            ny = (float)(c == 0 ? V[3] : c == 1 ? V[4] : V[5]);
            nz = (float)(c == 0 ? V[6] : c == 1 ? V[7] : V[8]);
            var = (float)(lmin / tr);
            // the sign, decided on the rounded components; the negation is exact
            bool flip;
            if (has_vp) {
                const double s = ((double)nx * (vx - (double)q.qx) + (double)ny * (vy - (double)q.qy)) + (double)nz * (vz - (double)q.qz);
                flip = s < 0.0;
            } else {
                const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
                const float big = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
                flip = big < 0.0f;
            }
            if (flip) { nx = -nx; ny = -ny; nz = -nz; }
        }
    }
    if (q.in_model && (threadIdx.x & (kWalkLanes - 1)) == 0) {
        normals[(size_t)row_i] = nx;
        normals[(size_t)row_i + (size_t)ldn] = ny;
        normals[(size_t)row_i + 2 * (size_t)ldn] = nz;
        if (variation) variation[row_i] = var;
    }
}

// Workspace: [seed bound of every sorted row, M floats]: roundup(4 * max(M, 1), 256) bytes, whatever k
struct NormalsWs { float* dk; };
NormalsWs normals_ws_layout(int M, void* base, size_t* bytes) {
    NormalsWs s{};
    WsWalk w(base);
    s.dk = w.take<float>((size_t)(M > 0 ? M : 1));
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t normals_ws_bytes(int M, int k) {
    (void)k;                                                      // the lists live in registers
    size_t b; (void)normals_ws_layout(M, nullptr, &b);
    return b;
}

int launch_model_normals(const ModelView& v, int k, const double* viewpoint, float* normals, int ldn, float* variation, void* ws,
                         size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(k >= 3 && k <= kNKnnMaxK && ldn >= v.M && (normals || v.M == 0));
    size_t need;
    const NormalsWs s = normals_ws_layout(v.M, ws, &need);
    if (ws_bytes < need) { set_error("normals workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_WORKSPACE; }
    const int M = v.M;
    if (M == 0) return PCREG_OK;
    const int n_tiles = (M + kT16 - 1) / kT16;
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;          // "knn_nocull": visit every tile, same bits
    unsigned long long* stats = knn_stats_dev();                  // "knn_stats": searches, visited, nominal (n_tiles^2)
    const int has_vp = viewpoint ? 1 : 0;
    const double vx = viewpoint ? viewpoint[0] : 0.0, vy = viewpoint ? viewpoint[1] : 0.0, vz = viewpoint ? viewpoint[2] : 0.0;
    launch_selfjoin_seed(v, k, s.dk, st);
    klist_dispatch<kSelfKbMin>(k, [&](auto kb) {
        hipLaunchKernelGGL(normals_walk_kernel<kb.value>, dim3((unsigned)n_tiles * kWalkWgPerTile), dim3(kBlock), 0, st, (const float*)v.ms,
                           (const int32_t*)v.perm, M, v.m, v.ldm, (const float*)v.tbox, n_tiles, cull, k, (const float*)s.dk, has_vp, vx, vy, vz,
                           normals, ldn, variation, stats);
    });
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
