// pcreg_amd/csrc/knn_fpfh.hip -- the FPFH descriptor (Rusu's fast point feature histogram, 33 numbers) of every row of a PREPARED
// model from its k nearest rows and a normal per row (3 <= k <= PCREG_KNN_MAX_K).  The contract is pcreg_model_fpfh_f32's
// (include/pcreg.h); DESIGN 4.19.
//
// The prepared model (knn_fast.hip) is used as it is, as the normals use it (knn_normals.hip).  A call is three launches:
//   F1  normals_seed_kernel    (knn_selfjoin.hpp) the seed bound of every sorted row with k
//   F2  fpfh_spfh_kernel<KB>   selfjoin_klist_walk<KB> (knn_selfjoin.hpp), the walk the normals use.  After it every
//                              lane of a row holds the row's list; the lanes store it, rows and fp32 squared distances, to the [M][k]
//                              table of the ORIGINAL row; then lane `sub` of the row takes list entries sub, sub + 4, ...: it gathers
//                              the neighbour's coordinates and normal by original row, forms the pair features in double and counts
//                              them into three histograms of eleven 5-bit fields, one 64-bit word each (a count is at most 31).  The
//                              four lanes' words are added (integers: no order), lane 0 stores the 33 uint8 counts
//   F3  fpfh_weight_kernel     one thread per (original row, feature): it reads the row's list from the table, gathers the neighbours'
//                              eleven counts in list order, forms acc, S_f and out in the contract's order and stores eleven doubles
// No floating-point value is added across threads: the result is a function of (model rows, normals, k) alone.  Nothing
// synchronises; no workgroup waits for another.
//
// WHY THE TABLE and not a second walk: F3 needs each row's neighbours and their fp32 distances again, after EVERY row's counts are
// known.  The table costs 8 k bytes a row written once and read once; a second walk costs the whole search again (the walk is the
// larger part of the call: DESIGN 4.19).
#include "knn_selfjoin.hpp"
#include "fpfh_pair.hpp"                             // dot3, fpfh_bin, fpfh_pair and the bin constants (shared with knn_fpfh_radius.hip)
#include <cmath>

namespace pcreg {

namespace {

constexpr int kFpfhBits = 5;                         // a histogram field: counts are <= k - 1 <= 31 (the row itself is no neighbour)
static_assert(kNKnnMaxK - 1 < (1 << kFpfhBits) && kFpfhBins * kFpfhBits <= 64, "eleven counts in one 64-bit word");

// the list moved N places towards its head, the empty entry (+inf, -1) entering at its end
template <int KB, int N>
__device__ __forceinline__ void klist_advance(float (&ld)[KB], int (&li)[KB], bool on) {
#pragma unroll
    for (int s = 0; s < KB; ++s) {
        const float d = s + N < KB ? ld[s + N < KB ? s + N : s] : INFINITY;
        const int i = s + N < KB ? li[s + N < KB ? s + N : s] : -1;
        ld[s] = on ? d : ld[s]; li[s] = on ? i : li[s];
    }
}

// ---- F2. the walk and the SPFH counts ------------------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(kBlock) void fpfh_spfh_kernel(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                           const float* __restrict__ m, int ldm, const float* __restrict__ tbox,
                                                           int n_tiles, int cull, int k, const float* __restrict__ dk,
                                                           const float* __restrict__ normals, int ldn, int32_t* __restrict__ lrow,
                                                           float* __restrict__ ldist, uint8_t* __restrict__ spfh,
                                                           unsigned long long* __restrict__ stats) {
    float ld[KB]; int li[KB];
    const WalkSelfRow q = selfjoin_klist_walk<KB>(ms, perm, M, tbox, n_tiles, cull, k, dk, stats, ld, li);
    const int row_i = q.row_i;
    const bool in_model = q.in_model;

    // ---- the epilogue: every lane of the row holds the row's list, (distance, row) ascending ----
    const int sub = threadIdx.x & (kWalkLanes - 1);
    // 1. the list to the table of the original row: lane sub stores places sub, sub + 4, ...
    if (in_model) {
        const size_t at = (size_t)row_i * (size_t)k;
#pragma unroll
        for (int s = 0; s < KB; ++s) {
            if (s < k && (s & (kWalkLanes - 1)) == sub) { lrow[at + s] = li[s]; ldist[at + s] = ld[s]; }
        }
    }
    // 2. lane sub's entries to the head of its list: place sub first, then every fourth
    klist_advance<KB, 1>(ld, li, (sub & 1) != 0);
    klist_advance<KB, 2>(ld, li, (sub & 2) != 0);
    const double pix = (double)q.qx, piy = (double)q.qy, piz = (double)q.qz;
    const size_t ri = (size_t)row_i;
    const double nix = (double)normals[ri], niy = (double)normals[ri + (size_t)ldn], niz = (double)normals[ri + 2 * (size_t)ldn];
    // 3. the pairs, one list entry a trip (k is uniform); a histogram is eleven 5-bit counts in one word: no indexed private array
    unsigned long long h1 = 0ull, h2 = 0ull, h3 = 0ull;
    for (int t = 0; t < k; t += kWalkLanes) {
        const int s = t + sub;
        const int j = li[0];
        const float d2 = ld[0];
        const bool nb = s < k && j >= 0 && d2 < INFINITY && d2 > 0.0f;                // a NEIGHBOUR: a row at a finite distance > 0
        const size_t rj = nb ? (size_t)j : ri;
        const double pjx = (double)m[rj], pjy = (double)m[rj + (size_t)ldm], pjz = (double)m[rj + 2 * (size_t)ldm];
        const double njx = (double)normals[rj], njy = (double)normals[rj + (size_t)ldn], njz = (double)normals[rj + 2 * (size_t)ldn];
        int b1, b2, b3;
        const bool on = fpfh_pair(pix, piy, piz, nix, niy, niz, pjx, pjy, pjz, njx, njy, njz, b1, b2, b3) && nb;
        const unsigned long long one = on ? 1ull : 0ull;
        h1 += one << (kFpfhBits * b1); h2 += one << (kFpfhBits * b2); h3 += one << (kFpfhBits * b3);
        klist_advance<KB, kWalkLanes>(ld, li, true);
    }
    // 4. the row's counts: the four lanes' words added (a field holds at most k - 1 <= 31 in all, so no carry crosses fields)
    h1 += __shfl_xor(h1, 1); h1 += __shfl_xor(h1, 2);
    h2 += __shfl_xor(h2, 1); h2 += __shfl_xor(h2, 2);
    h3 += __shfl_xor(h3, 1); h3 += __shfl_xor(h3, 2);
    if (in_model && sub == 0) {
        uint8_t* o = spfh + ri * (size_t)kFpfhDim;
        const unsigned long long mask = (1ull << kFpfhBits) - 1ull;
#pragma unroll
        for (int b = 0; b < kFpfhBins; ++b) {
            o[b] = (uint8_t)((h1 >> (kFpfhBits * b)) & mask);
            o[kFpfhBins + b] = (uint8_t)((h2 >> (kFpfhBits * b)) & mask);
            o[2 * kFpfhBins + b] = (uint8_t)((h3 >> (kFpfhBits * b)) & mask);
        }
    }
}

// ---- F3. the weighted sum of the neighbours' histograms --------------------------------------------------------------------
// Thread g serves feature g % 3 of original row g / 3: consecutive threads store consecutive runs of eleven doubles.  The eleven
// counts of a feature add up to m_j whichever feature it is (a contributing pair counts once in each), so a thread needs no
// other feature's counts.
__global__ __launch_bounds__(kBlock) void fpfh_weight_kernel(const float* __restrict__ m, int ldm, int M, int k, const int32_t* __restrict__ lrow,
                                                             const float* __restrict__ ldist, const uint8_t* __restrict__ spfh,
                                                             double* __restrict__ out) {
    const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long row = g / 3;
    if (row >= M) return;
    const int f = (int)(g - 3 * row);
    const size_t r = (size_t)row;
    const bool finite = finite3(m[r], m[r + (size_t)ldm], m[r + 2 * (size_t)ldm]);
    double acc[kFpfhBins];
#pragma unroll
    for (int b = 0; b < kFpfhBins; ++b) acc[b] = 0.0;
    const size_t at = r * (size_t)k;
    for (int s = 0; s < k; ++s) {
        const int j = lrow[at + s];
        const float d2 = ldist[at + s];
        if (j >= 0 && d2 < INFINITY && d2 > 0.0f) {               // a neighbour, in list order
            const uint8_t* c = spfh + (size_t)j * kFpfhDim + (size_t)f * kFpfhBins;
            int cnt[kFpfhBins], mj = 0;
#pragma unroll
            for (int b = 0; b < kFpfhBins; ++b) { cnt[b] = (int)c[b]; mj += cnt[b]; }
            if (mj > 0) {
                const double dm = (double)mj, w = (double)d2;
#pragma unroll
                for (int b = 0; b < kFpfhBins; ++b) acc[b] = acc[b] + ((double)cnt[b] / dm) / w;
            }
        }
    }
    double S = acc[0];
#pragma unroll
    for (int b = 1; b < kFpfhBins; ++b) S = S + acc[b];
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
    double* o = out + r * (size_t)kFpfhDim + (size_t)f * kFpfhBins;
#pragma unroll
    for (int b = 0; b < kFpfhBins; ++b) o[b] = !finite ? qnan : S > 0.0 ? (acc[b] / S) * 100.0 : 0.0;
}

// Workspace, with R = max(M, 1): [seed bound of every sorted row, R floats][the lists' rows by original row, R k int32][their fp32
// squared distances, R k floats][the SPFH counts, 33 R bytes (used when the caller wants none)]:
// roundup(4 R, 256) + 2 roundup(4 R k, 256) + roundup(33 R, 256) bytes
struct FpfhWs { float* dk; int32_t* lrow; float* ldist; uint8_t* spfh; };
FpfhWs fpfh_ws_layout(int M, int k, void* base, size_t* bytes) {
    FpfhWs s{};
    WsWalk w(base);
    const size_t R = (size_t)(M > 0 ? M : 1), K = (size_t)(k > 0 ? k : 0);
    s.dk = w.take<float>(R);
    s.lrow = w.take<int32_t>(R * K);
    s.ldist = w.take<float>(R * K);
    s.spfh = w.take<uint8_t>(R * (size_t)kFpfhDim);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t fpfh_ws_bytes(int M, int k) {
    size_t b; (void)fpfh_ws_layout(M, k, nullptr, &b);
    return b;
}

int launch_model_fpfh(const ModelView& v, int k, const float* normals, int ldn, double* fpfh, uint8_t* spfh, void* ws, size_t ws_bytes,
                      hipStream_t st) {
    PCREG_ARG(k >= 3 && k <= kNKnnMaxK && ldn >= v.M && ((normals && fpfh) || v.M == 0));
    size_t need;
    const FpfhWs s = fpfh_ws_layout(v.M, k, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: fpfh workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M;
    if (M == 0) return PCREG_OK;
    const int n_tiles = (M + kT16 - 1) / kT16;
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;          // "knn_nocull": visit every tile, same bits
    unsigned long long* stats = knn_stats_dev();                  // "knn_stats": searches, visited, nominal (n_tiles^2)
    uint8_t* counts = spfh ? spfh : s.spfh;
    launch_selfjoin_seed(v, k, s.dk, st);
    klist_dispatch<kSelfKbMin>(k, [&](auto kb) {
        hipLaunchKernelGGL(fpfh_spfh_kernel<kb.value>, dim3((unsigned)n_tiles * kWalkWgPerTile), dim3(kBlock), 0, st, (const float*)v.ms,
                           (const int32_t*)v.perm, M, v.m, v.ldm, (const float*)v.tbox, n_tiles, cull, k, (const float*)s.dk, normals, ldn, s.lrow,
                           s.ldist, counts, stats);
    });
    const unsigned long long threads = 3ull * (unsigned long long)M;
    hipLaunchKernelGGL(fpfh_weight_kernel, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, v.m, v.ldm, M, k,
                       (const int32_t*)s.lrow, (const float*)s.ldist, (const uint8_t*)counts, fpfh);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
