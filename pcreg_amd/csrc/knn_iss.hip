// pcreg_amd/csrc/knn_iss.hip -- ISS keypoints of a PREPARED model (Zhong's Intrinsic Shape Signatures; MATLAB's detectISSFeatures):
// the eigenvalues of every row's radius neighbourhood from EXACT integer sums, the saliency of the rows that pass the two ratio
// tests, and the rows no neighbour beats, ascending.  The contract is pcreg_model_iss_f32's (include/pcreg.h); DESIGN 4.20.
//
// The prepared model (knn_fast.hip) is used as it is, as the clustering and the normals use it.  A call is four launches:
//   I1  iss_scatter_kernel   the self-join walk over ALL tiles b that DESIGN 4.1's rule (D = r2_salient, the box of tile a) does not
//                            rule out; four lanes a row.  A hit quantises the fp32 difference to integers q and adds 1, q and the six
//                            products into the lane's integer accumulators.  The epilogue adds the four lanes (two xor shuffles),
//                            forms N = n S2 - S1 S1^T exactly in 128 bits, rounds each entry once to double, runs jacobi_sym3,
//                            applies the tests and stores n, the eigenvalues and the saliency at the ORIGINAL row
//   I2  iss_nonmax_kernel    the same walk with D = r2_nonmax, for the rows with a saliency > 0: a hit gathers the neighbour's
//                            saliency and applies the rule on the bit patterns (saliencies are >= 0: their order is their bits');
//                            the four lanes are OR-ed into one flag byte per original row
//   I3  iss_count_kernel     chunk_scan.hpp's predicate compaction over the flags: the count of every chunk of 2048 original rows
//   I4  iss_list_kernel      ... and the keypoint rows ascending, and their number
// The walks' row prologue, staging rule and visit rule are knn_walk.hpp's (walk_self_row, walk_row_finite, walk_visits).
// Every sum across hits is an INTEGER sum: no order of summation, no floating-point atomic.  Nothing synchronises; no workgroup
// waits for another.
#include "common.hpp"
#include "knn_fast_common.hpp"
#include "knn_walk.hpp"
#include "chunk_scan.hpp"
#include "wave_math.hpp"
#include <cmath>

namespace pcreg {

namespace {

constexpr int kIssMaxM = 1 << 26;                    // below it no sum overflows: |q| <= 2^18 + 1, so |S2| < 2^26 (2^18 + 1)^2 < 2^63

// ---- I1. the scatter ------------------------------------------------------------------------------------------------------
// scale = 2^(18 - e) as a float and back = 4^-(18 - e) as a double, e from r2 on the host (launch_model_iss).  dx * scale is exact
// (a power of two; a product below the normal range rounds to an integer 0 either way), rintf rounds to nearest even.
__global__ __launch_bounds__(kBlock) void iss_scatter_kernel(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                             const float* __restrict__ tbox, int n_tiles, int cull, float r2, float scale,
                                                             double back, double g21, double g32, int min_nb,
                                                             int32_t* __restrict__ n_out, double* __restrict__ eig,
                                                             double* __restrict__ sal, unsigned long long* __restrict__ stats) {
    __shared__ WalkLds lds;
    const int tid = threadIdx.x;
    const int ta = blockIdx.x / kWalkWgPerTile, part = blockIdx.x % kWalkWgPerTile;
    walk_count_search(stats, (unsigned long long)n_tiles * (unsigned long long)n_tiles);
    __builtin_assume(r2 < INFINITY);                              // (iss_args_ok: walk_visits' guard for an infinite D folds away)
    float abox[6];
    walk_tile_box(tbox, ta, abox);
    const WalkSelfRow q = walk_self_row(ms, perm, M, ta, part);
    const float rr = q.live ? r2 : -1.0f;                         // (a dead lane admits nothing: d is never negative)
    int n = 0;
    long long s1x = 0, s1y = 0, s1z = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    walk_tiles(
        lds, 0, n_tiles, q.qx, q.qy, q.qz, part == 0 ? stats : nullptr,
        [&](int ct) { return walk_visits(tbox, ct, abox, r2, cull); },
        [&](int r) { return walk_row_finite(ms, perm, M, r); },
        [](int) {},
        [&](int, const float4 (&p)[4], float (&d)[4]) {
            if (fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= rr) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d[u] <= rr) {
                        const int qa = (int)rintf((p[u].x - q.qx) * scale);
                        const int qb = (int)rintf((p[u].y - q.qy) * scale);
                        const int qc = (int)rintf((p[u].z - q.qz) * scale);
                        ++n;
                        s1x += qa; s1y += qb; s1z += qc;
                        sxx += (long long)qa * qa; sxy += (long long)qa * qb; sxz += (long long)qa * qc;
                        syy += (long long)qb * qb; syz += (long long)qb * qc; szz += (long long)qc * qc;
                    }
                }
            }
        },
        [] {});
    // the four lanes of the row: integers, so the order is immaterial
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
        n += __shfl_xor(n, o);
        s1x += __shfl_xor(s1x, o); s1y += __shfl_xor(s1y, o); s1z += __shfl_xor(s1z, o);
        sxx += __shfl_xor(sxx, o); sxy += __shfl_xor(sxy, o); sxz += __shfl_xor(sxz, o);
        syy += __shfl_xor(syy, o); syz += __shfl_xor(syz, o); szz += __shfl_xor(szz, o);
    }
    if (!q.in_model || (tid & (kWalkLanes - 1)) != 0) return;
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    double mu[3] = {qnan, qnan, qnan}, s = 0.0;
    if (n > 0) {
        const __int128 nn = n;
        double a[6], V[9];
        a[0] = i128_to_double(nn * sxx - (__int128)s1x * s1x);
        a[1] = i128_to_double(nn * sxy - (__int128)s1x * s1y);
        a[2] = i128_to_double(nn * sxz - (__int128)s1x * s1z);
        a[3] = i128_to_double(nn * syy - (__int128)s1y * s1y);
        a[4] = i128_to_double(nn * syz - (__int128)s1y * s1z);
        a[5] = i128_to_double(nn * szz - (__int128)s1z * s1z);
        jacobi_sym3(a, V);
        const double e0 = a[0], e1 = a[3], e2 = a[5];
        mu[0] = fmax(fmax(e0, e1), e2);
        mu[2] = fmin(fmin(e0, e1), e2);
        mu[1] = fmax(fmin(e0, e1), fmin(fmax(e0, e1), e2));       // the median of three
        const bool cand = n >= min_nb && mu[1] < g21 * mu[0] && mu[2] < g32 * mu[1] && mu[2] > 0.0;
        const double n2 = (double)((long long)n * (long long)n);
        const double l3 = (mu[2] / n2) * back;
        s = cand ? l3 : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) mu[c] = (mu[c] / n2) * back;
    }
    n_out[q.row_i] = n;
    sal[q.row_i] = s;
    if (eig) {
#pragma unroll
        for (int c = 0; c < 3; ++c) eig[(size_t)q.row_i * 3 + c] = mu[c];
    }
}

// ---- I2. the suppression ----------------------------------------------------------------------------------------------------
// sal is read as its bit patterns: every saliency is >= +0 and none is NaN, so s_j > s_i is the order of the 64-bit words.  The
// neighbour's saliency is GATHERED on a hit (sal[row_j], an 8-byte load): hits are a handful per visited tile and row, while staging
// the tile's 512 saliencies in begin_tile puts a dependent load between the walk's two barriers for every tile of every workgroup.
// Measured at 1 M rows: 6.25 ms with the gather, 7.76 ms with the tile's saliencies staged in LDS.
__global__ __launch_bounds__(kBlock) void iss_nonmax_kernel(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                            const float* __restrict__ tbox, int n_tiles, int cull, float r2,
                                                            const unsigned long long* __restrict__ sal, uint8_t* __restrict__ flag,
                                                            unsigned long long* __restrict__ stats) {
    __shared__ WalkLds lds;
    const int tid = threadIdx.x;
    const int ta = blockIdx.x / kWalkWgPerTile, part = blockIdx.x % kWalkWgPerTile;
    walk_count_search(stats, (unsigned long long)n_tiles * (unsigned long long)n_tiles);
    __builtin_assume(r2 < INFINITY);                              // (iss_args_ok: walk_visits' guard for an infinite D folds away)
    float abox[6];
    walk_tile_box(tbox, ta, abox);
    const WalkSelfRow q = walk_self_row(ms, perm, M, ta, part);
    const unsigned long long s_i = q.live ? sal[q.row_i] : 0ull;
    const bool work = s_i != 0ull;                                // a row with s == 0 is no keypoint whatever its neighbours
    const int any = __syncthreads_or(work ? 1 : 0);               // (uniform: a workgroup without such a row visits nothing)
    const float rr = work ? r2 : -1.0f;
    int beaten = 0;
    walk_tiles(
        lds, 0, n_tiles, q.qx, q.qy, q.qz, part == 0 ? stats : nullptr,
        [&](int ct) { return any != 0 && walk_visits(tbox, ct, abox, r2, cull); },
        [&](int r) { return walk_row_finite(ms, perm, M, r); },
        [](int) {},
        [&](int, const float4 (&p)[4], float (&d)[4]) {
            if (fminf(fminf(d[0], d[1]), fminf(d[2], d[3])) <= rr) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d[u] <= rr) {
                        const int row_j = __float_as_int(p[u].w);
                        const unsigned long long s_j = sal[row_j];
                        beaten |= (s_j > s_i || (s_j == s_i && row_j < q.row_i)) ? 1 : 0;      // (j == i: neither)
                    }
                }
            }
        },
        [] {});
    beaten |= __shfl_xor(beaten, 1);
    beaten |= __shfl_xor(beaten, 2);
    if (q.in_model && (tid & (kWalkLanes - 1)) == 0) flag[q.row_i] = (work && !beaten) ? 1 : 0;
}

// ---- I3, I4. the compaction of the flags (chunk_scan.hpp's predicate compaction over the original rows) ------------------------
__global__ __launch_bounds__(kScanBlock) void iss_count_kernel(const uint8_t* __restrict__ flag, int M, int32_t* __restrict__ pin) {
    chunk_pred_count(M, pin, [&](long long i) { return flag[i] != 0; });
}
__global__ __launch_bounds__(kScanBlock) void iss_list_kernel(const uint8_t* __restrict__ flag, int M, const int32_t* __restrict__ pin,
                                                              int32_t* __restrict__ keypoints, int32_t* __restrict__ n_keypoints) {
    const int32_t at = chunk_pred_emit(M, pin, [&](long long i) { return flag[i] != 0; },
                                       [&](int32_t at, long long i) { if (keypoints) keypoints[at] = (int32_t)i; });   // (no list: count only)
    if (chunk_is_last_thread()) *n_keypoints = at;
}

// M = 0: no row, no keypoint
__global__ void iss_empty_kernel(int32_t* __restrict__ n_keypoints) { *n_keypoints = 0; }

// Workspace, with R = max(M, 1) and C = max(ceil(M / 2048), 1): [keypoint flag of every original row, R bytes][flags per chunk, C
// int32]: roundup(R, 256) + roundup(4 C, 256) bytes, whatever the radii
struct IssWs { uint8_t* flag; int32_t* pin; int n_chunks; };
IssWs iss_ws_layout(int M, void* base, size_t* bytes) {
    IssWs s{};
    WsWalk w(base);
    const size_t R = (size_t)(M > 0 ? M : 1);
    s.n_chunks = (int)((R + kScanChunk - 1) / kScanChunk);
    s.flag = w.take<uint8_t>(R);
    s.pin = w.take<int32_t>((size_t)s.n_chunks);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t iss_ws_bytes(int M) {
    size_t b; (void)iss_ws_layout(M, nullptr, &b);
    return b;
}

bool iss_args_ok(float r2_salient, float r2_nonmax, double gamma21, double gamma32, int min_neighbors) {
    return std::isnormal(r2_salient) && r2_salient > 0.0f && std::isnormal(r2_nonmax) && r2_nonmax > 0.0f && std::isfinite(gamma21) &&
           gamma21 > 0.0 && std::isfinite(gamma32) && gamma32 > 0.0 && min_neighbors >= 1;
}
int iss_max_rows() { return kIssMaxM; }

int launch_model_iss(const ModelView& v, float r2_salient, float r2_nonmax, double gamma21, double gamma32, int min_neighbors,
                     int32_t* n_neighbors, double* eig, double* saliency, int32_t* keypoints, int32_t* n_keypoints, void* ws, size_t ws_bytes,
                     hipStream_t st) {
    PCREG_ARG(iss_args_ok(r2_salient, r2_nonmax, gamma21, gamma32, min_neighbors) && (n_keypoints || !keypoints));
    PCREG_ARG(v.M < kIssMaxM && ((n_neighbors && saliency) || v.M == 0));
    size_t need;
    const IssWs s = iss_ws_layout(v.M, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: iss workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M;
    if (M == 0) {
        if (n_keypoints) hipLaunchKernelGGL(iss_empty_kernel, dim3(1), dim3(1), 0, st, n_keypoints);
        PCREG_HIP(hipGetLastError());
        return PCREG_OK;
    }
    // r2 = f 2^e2, f in [0.5, 1); e = ceil(e2 / 2): every neighbour's |dx| <= sqrt(r2) (1 + 2^-23) < 2^e (1 + 2^-23), |q| <= 2^18 + 1
    int e2;
    (void)std::frexp(r2_salient, &e2);
    const int e = e2 >= 0 ? (e2 + 1) / 2 : -((-e2) / 2);
    const float scale = std::ldexp(1.0f, 18 - e);
    const double back = std::ldexp(1.0, -2 * (18 - e));
    const int n_tiles = (M + kT16 - 1) / kT16;
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;          // "knn_nocull": visit every tile, same bits
    unsigned long long* kstats = knn_stats_dev();                 // "knn_stats": searches, visited, nominal (n_tiles^2), per walk
    const dim3 grid((unsigned)n_tiles * kWalkWgPerTile);
    hipLaunchKernelGGL(iss_scatter_kernel, grid, dim3(kBlock), 0, st, (const float*)v.ms, (const int32_t*)v.perm, M, (const float*)v.tbox, n_tiles,
                       cull, r2_salient, scale, back, gamma21, gamma32, min_neighbors, n_neighbors, eig, saliency, kstats);
    if (n_keypoints) {
        hipLaunchKernelGGL(iss_nonmax_kernel, grid, dim3(kBlock), 0, st, (const float*)v.ms, (const int32_t*)v.perm, M, (const float*)v.tbox,
                           n_tiles, cull, r2_nonmax, (const unsigned long long*)saliency, s.flag, kstats);
        const dim3 cgrid((unsigned)s.n_chunks), cblock(kScanBlock);
        hipLaunchKernelGGL(iss_count_kernel, cgrid, cblock, 0, st, (const uint8_t*)s.flag, M, s.pin);
        hipLaunchKernelGGL(iss_list_kernel, cgrid, cblock, 0, st, (const uint8_t*)s.flag, M, (const int32_t*)s.pin, keypoints, n_keypoints);
    }
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
