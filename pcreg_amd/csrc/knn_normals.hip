// pcreg_amd/csrc/knn_normals.hip -- the surface normal of every row of a PREPARED model from its k nearest rows
// (3 <= k <= PCREG_KNN_MAX_K).  The contract is pcreg_model_normals_f32's (include/pcreg.h); DESIGN 4.15.
//
// The prepared model (knn_fast.hip) is used as it is: the sorted fp32 copy, perm, the tile boxes.  The queries are the sorted
// copy itself, so there is no query order and no limit on M.  A call is two launches:
//   N1  normals_seed_kernel      (knn_selfjoin.hpp) one wave per sorted row: the k-th smallest distance over the window of 64 consecutive sorted
//                                rows around it (k distinct finite rows lie within that distance: an upper bound of the true
//                                k-th distance; fewer than k finite rows leave +inf).  A non-finite row gets 0: it admits nothing
//   N2  normals_walk_kernel<KB>  cluster_walk_kernel's shape with knn_k_kernel's body: workgroup (tile a, part p) owns 64 sorted
//                                rows of tile a, four lanes per row, each with a sorted list of KB >= k (distance, row) pairs in
//                                registers.  The block's box is tile a's, its bound D the largest seed over tile a's rows; a tile
//                                on EITHER side of a is visited unless DESIGN 4.1's rule skips it.  After the two merges every
//                                lane of a row holds the row's list; the epilogue gathers the neighbours by original row from
//                                the model's own array and computes mean, sums, Jacobi, sign in double, all four lanes alike
//                                (no lane waits for another, nothing is shared), and lane 0 stores to the original-row slot
// Nothing is added across threads: the result is a function of (model rows, k, viewpoint) alone.
#include "knn_selfjoin.hpp"
#include "wave_math.hpp"
#include <cmath>

namespace pcreg {

namespace {

// N1, normals_seed_kernel, and the helpers shared with the denoising walk live in knn_selfjoin.hpp.

// ---- N2. the walk and the normal ---------------------------------------------------------------------------------------
// A row enters a list only when d <= thr, thr = min(seed, the k-th entry of any of the row's four lists), each of which bounds
// the true k-th distance from above.  Non-finite rows are staged as no row at all (as the clustering walk does), and a
// non-finite row's own lanes admit nothing (its distances are NaN or +inf, its seed is 0).
template <int KB>
__global__ __launch_bounds__(kBlock) void normals_walk_kernel(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                              const float* __restrict__ m, int ldm, const float* __restrict__ tbox,
                                                              int n_tiles, int cull, int k, const float* __restrict__ dk, int has_vp,
                                                              double vx, double vy, double vz, float* __restrict__ normals, int ldn,
                                                              float* __restrict__ variation, unsigned long long* __restrict__ stats) {
    __shared__ WalkLds lds;
    __shared__ float s_red[kBlock / 64];
    const int tid = threadIdx.x;
    const int ta = blockIdx.x / kNWgPerTile, part = blockIdx.x % kNWgPerTile;
    if (stats && blockIdx.x == 0 && tid == 0) {
        atomicAdd(&stats[0], 1ull);
        atomicAdd(&stats[2], (unsigned long long)n_tiles * (unsigned long long)n_tiles);
    }
    // the block's box is tile a's; its bound the largest seed over ALL of tile a's rows (every workgroup forms the same value)
    float abox[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) abox[c] = tbox[(size_t)ta * 6 + c];
    const float D = selfjoin_tile_bound(dk, ta, M, s_red);
    // this thread's row
    const int rl = part * kWalkQPerWg + tid / kWalkLanes;         // the row's place inside tile a
    const long long srow = (long long)ta * kT16 + rl;
    const bool in_model = srow < M;
    const size_t sr = in_model ? (size_t)srow : 0;
    const float qx = ms[sr], qy = ms[sr + (size_t)M], qz = ms[sr + 2 * (size_t)M];
    const int row_i = perm[sr];
    float thr = in_model ? dk[sr] : -INFINITY;                    // (a dead lane admits nothing)
    if (!(thr == thr)) thr = INFINITY;
    float ld[KB]; int li[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) { ld[s] = INFINITY; li[s] = -1; }
    walk_tiles(
        lds, 0, n_tiles, qx, qy, qz, part == 0 ? stats : nullptr,
        [&](int ct) {
            return !(cull != 0 && D < INFINITY && cull_skips(cull_gap2(tbox + (size_t)ct * 6, tbox + (size_t)ct * 6 + 3, abox, abox + 3), D));
        },
        [&](int r) {                                              // a non-finite row is staged as no row at all
            if (r < M) {
                const float x = ms[r], y = ms[r + (size_t)M], z = ms[r + 2 * (size_t)M];
                if (nfinite3(x, y, z)) return make_float4(x, y, z, __int_as_float(perm[r]));
            }
            return walk_no_row();
        },
        [](int) {},
        [&](int, const float4 (&p)[4], float (&d)[4]) {
            if (fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= thr) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d[u] <= thr) {
                        klist_insert<KB>(ld, li, d[u], __float_as_int(p[u].w));
                        thr = fminf(thr, klist_kth_reg<KB>(ld, k));
                    }
                }
            }
        },
        [&] {
            thr = fminf(thr, __shfl_xor(thr, 1));                 // the row's four lanes share the tightest bound
            thr = fminf(thr, __shfl_xor(thr, 2));
        });
    klist_merge_xor<KB>(ld, li, 1);
    klist_merge_xor<KB>(ld, li, 2);

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
                const double s = ((double)nx * (vx - (double)qx) + (double)ny * (vy - (double)qy)) + (double)nz * (vz - (double)qz);
                flip = s < 0.0;
            } else {
                const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
                const float big = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
                flip = big < 0.0f;
            }
            if (flip) { nx = -nx; ny = -ny; nz = -nz; }
        }
    }
    if (in_model && (tid & (kWalkLanes - 1)) == 0) {
        normals[(size_t)row_i] = nx;
        normals[(size_t)row_i + (size_t)ldn] = ny;
        normals[(size_t)row_i + 2 * (size_t)ldn] = nz;
        if (variation) variation[row_i] = var;
    }
}

int nkb_of(int k) { return k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }

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
    hipLaunchKernelGGL(normals_seed_kernel, dim3((unsigned)((M + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, st, (const float*)v.ms, M, k,
                       s.dk);
    const dim3 grid((unsigned)n_tiles * kNWgPerTile);
#define PCREG_NORMALS_LAUNCH(KB_)                                                                                              \
    hipLaunchKernelGGL(normals_walk_kernel<KB_>, grid, dim3(kBlock), 0, st, (const float*)v.ms, (const int32_t*)v.perm, M, v.m, v.ldm, \
                       (const float*)v.tbox, n_tiles, cull, k, (const float*)s.dk, has_vp, vx, vy, vz, normals, ldn, variation, stats)
    switch (nkb_of(k)) {
        case 4: PCREG_NORMALS_LAUNCH(4); break;
        case 8: PCREG_NORMALS_LAUNCH(8); break;
        case 16: PCREG_NORMALS_LAUNCH(16); break;
        default: PCREG_NORMALS_LAUNCH(32); break;
    }
#undef PCREG_NORMALS_LAUNCH
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
