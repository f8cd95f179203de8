// pcreg_amd/csrc/fgr.hip -- fast global registration of B sets of matched pairs (pcreg_fgr_batched's contract, include/pcreg.h;
// DESIGN 4.30).  gfx950 only.  Two forms of one computation, chosen by n_cap on the host:
//   resident  ONE launch, a workgroup per registration: the tuple test, the box, the kept pairs staged in LDS (six doubles a
//             pair, SoA), every iteration, the counts and the ordered inlier list.  Nothing returns to the host between iterations.
//   chained   for n_cap above the resident capacity (or "fgr_chain"): a prologue (the same head, the pairs staged in the
//             workspace), per iteration a sums kernel over (registration, chunk) and refit_step.hpp's finish_step with one wave per
//             registration, then an epilogue (the same tail).
// Both run the same device functions on the same chunks of kScanChunk kept pairs -- fgr_chunk is the per-chunk body, its one
// definition, and the tree is refit_step.hpp's chunk_sums -- and add the chunks in ascending order, so they give the same bits.  fp64 throughout, no floating-point atomics,
// no sum whose order depends on scheduling; a chunk's 48 loads per thread are issued together, ahead of their use.
#include "common.hpp"
#include "refit_step.hpp"
#include "wave_math.hpp"
#include "fgr_pair.hpp"
#include <cmath>

namespace pcreg {
namespace {

constexpr int kBlock = kScanBlock;
constexpr int kFgrResident = 3328;                  // pairs: 48 x 3328 = 156 KiB of the 160 KiB of LDS; the kernels' small arrays take under 2 KiB
constexpr int kFgrState = 8;                        // doubles per registration of the chained form: mu, mu0, o[3], alive, n_kept, n_live
constexpr size_t kFgrMaxCells = (size_t)1 << 30;    // B x n_cap

struct FgrArgs {
    const double* p1; const double* p2; int ld; const int32_t* offsets; int B, n_cap;
    pcreg_fgr_opts o; const double* T0; const int32_t* tuple_idx;
    pcreg_fgr_result* out; int32_t* inlier_idx; uint8_t* kept;
    // the workspace (fgr_ws_layout)
    uint8_t* mask; int32_t* kidx; double* staged; double* state; double* Tpp; double* psums; int32_t* empty; int chunks;
};
struct FgrHead { int n_live, n_kept; double o[3]; double mu0; };

// ---- small workgroup helpers (kBlock threads) -----------------------------------------------------------------------------
// the place of a flagged thread among the workgroup's flagged threads, in thread order, behind `running`; -1 without the flag
__device__ __forceinline__ int compact_slot(bool flag, int& running) {
    __shared__ int s_w[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    int before = running;
    for (int w = 0; w < wave; ++w) before += s_w[w];
    const int tot = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
    __syncthreads();
    running += tot;
    return flag ? before + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
}
__device__ __forceinline__ void load_pair(const double* __restrict__ g1, const double* __restrict__ g2, size_t ld, int i, double (&p)[6]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { p[c] = g1[i + c * ld]; p[3 + c] = g2[i + c * ld]; }
}
// triple p of registration b (0-based out): the caller's table, or pcreg_ransac's built-in sampler (wave_math.hpp: sample3_builtin,
// the oracle's sample_table) with seed + b; clamped as ransac.hip's sample3 clamps.  n >= 3
__device__ __forceinline__ void fgr_triple(const FgrArgs& a, int b, int p, int n, int (&s)[3]) {
    if (a.tuple_idx) {
        const int32_t* t = a.tuple_idx + ((size_t)b * a.o.n_tuples + p) * 3;
        s[0] = t[0] - 1; s[1] = t[1] - 1; s[2] = t[2] - 1;
    } else {
        sample3_builtin(a.o.seed + (unsigned long long)b, (unsigned long long)p, n, s);
    }
    sample3_clamp(s, n);
}

// ---- the head: tuple test, kept pairs staged in ascending row order, box ------------------------------------------------------
// st [6][stride] receives the kept pairs, kidx their rows, mask [n] the kept flags (it is the working storage of the tuple test too)
__device__ __forceinline__ void fgr_head(const FgrArgs& a, int b, const double* __restrict__ g1, const double* __restrict__ g2, int n, double* st,
                                         int stride, int32_t* __restrict__ kidx, uint8_t* mask, FgrHead& h) {
    __shared__ double s_box[kBlock / 64][12];
    __shared__ int s_live[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t ld = (size_t)a.ld;
    const bool tuples = a.o.n_tuples > 0;
    if (tuples) {
        for (int i = tid; i < n; i += kBlock) mask[i] = 0;
        __syncthreads();
        if (n >= kFgrMinPairs) {
            const double s2 = a.o.tuple_scale * a.o.tuple_scale;
            for (int p = tid; p < a.o.n_tuples; p += kBlock) {
                int s[3];
                fgr_triple(a, b, p, n, s);
                double pa[6], pb[6], pc[6];
                load_pair(g1, g2, ld, s[0], pa); load_pair(g1, g2, ld, s[1], pb); load_pair(g1, g2, ld, s[2], pc);
                if (fgr_triple_ok(pa, pb, pc, s2)) { mask[s[0]] = 1; mask[s[1]] = 1; mask[s[2]] = 1; }     // (the same byte from any thread)
            }
        }
        __syncthreads();
    }
    double box[12];                                    // lo of p1, p2 (min) then -hi (min again)
#pragma unroll
    for (int c = 0; c < 12; ++c) box[c] = INFINITY;
    int running = 0, live = 0;
    for (int base = 0; base < n; base += kBlock) {
        const int i = base + tid;
        double p[6];
        bool lv = false, keep = false;
        if (i < n) {
            load_pair(g1, g2, ld, i, p);
            lv = fgr_live(p);
            keep = lv && (!tuples || mask[i] != 0);
        }
        live += lv ? 1 : 0;
        const int pos = compact_slot(keep, running);
        if (keep) {
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                st[(size_t)c * stride + pos] = p[c];
                box[c] = p[c] < box[c] ? p[c] : box[c];
                box[6 + c] = -p[c] < box[6 + c] ? -p[c] : box[6 + c];
            }
            kidx[pos] = i;
        }
        if (i < n) mask[i] = keep ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        live += __shfl_xor(live, o);
#pragma unroll
        for (int c = 0; c < 12; ++c) { const double v = __shfl_xor(box[c], o); box[c] = v < box[c] ? v : box[c]; }
    }
    if (lane == 0) {
        s_live[wave] = live;
#pragma unroll
        for (int c = 0; c < 12; ++c) s_box[wave][c] = box[c];
    }
    __syncthreads();                                   // (the staged pairs are visible behind it too)
    h.n_live = (s_live[0] + s_live[1]) + (s_live[2] + s_live[3]);
    h.n_kept = running;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        double v = s_box[0][c];
        for (int w = 1; w < kBlock / 64; ++w) v = s_box[w][c] < v ? s_box[w][c] : v;
        box[c] = v;
    }
    const double lo1[3] = {box[0], box[1], box[2]}, hi1[3] = {-box[6], -box[7], -box[8]};
    const double lo2[3] = {box[3], box[4], box[5]}, hi2[3] = {-box[9], -box[10], -box[11]};
#pragma unroll
    for (int c = 0; c < 3; ++c) h.o[c] = fgr_mid(lo1[c], hi1[c]);
    const double d1 = fgr_diag2(lo1, hi1), d2 = fgr_diag2(lo2, hi2);
    h.mu0 = a.o.mu0 != 0.0 ? a.o.mu0 : (d1 > d2 ? d1 : d2);
}

// ---- the per-chunk body, its one definition ------------------------------------------------------------------------------------
// Chunk c of the n_kept staged pairs: thread t adds pairs 2048 c + t, + 256, ... in that order; then refit_step.hpp's chunk_sums, the
// tree of chunk_tail<28>.  Thread k < 28 returns sum k of the chunk, the others 0.
__device__ __forceinline__ double fgr_chunk(const double* st, int stride, int c, int n_kept, const double (&T)[16], const double (&o)[3], double mu) {
    const int tid = threadIdx.x, k0 = c * kScanChunk + tid;
    double pr[kScanPer][6];
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const int k = k0 + u * kBlock;
#pragma unroll
        for (int e = 0; e < 6; ++e) pr[u][e] = k < n_kept ? st[(size_t)e * stride + k] : 0.0;
    }
    double acc[27], last = 0.0;
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u)
        if (k0 + u * kBlock < n_kept) fgr_pair_add(T, pr[u], o, mu, acc, last);
    __syncthreads();                                   // the chunk before this one has been read (the resident form comes here again)
    return chunk_sums<kPlaneSums>(acc, last);
}

// ---- the tail: cost, inliers and their ordered list -----------------------------------------------------------------------------
// the same chunks and trees for cost and sum_d2; inl receives the 1-based rows of the inliers, ascending
__device__ __forceinline__ void fgr_tail(const double* st, int stride, const int32_t* __restrict__ kidx, int n_kept, const double (&T)[16], double mu,
                                         double delta2, int32_t* __restrict__ inl, double& cost, double& sum_d2, int& n_inl) {
    __shared__ double s_e[kBlock / 64][2];
    const int tid = threadIdx.x;
    cost = 0.0; sum_d2 = 0.0;
    int running = 0;
    for (int c = 0; c * kScanChunk < n_kept; ++c) {
        const int k0 = c * kScanChunk + tid;
        double pr[kScanPer][6];
#pragma unroll
        for (int u = 0; u < kScanPer; ++u) {
            const int k = k0 + u * kBlock;
#pragma unroll
            for (int e = 0; e < 6; ++e) pr[u][e] = k < n_kept ? st[(size_t)e * stride + k] : 0.0;
        }
        double ac = 0.0, ad = 0.0;
        bool in[kScanPer];
#pragma unroll
        for (int u = 0; u < kScanPer; ++u) {
            in[u] = false;
            if (k0 + u * kBlock < n_kept) {
                double q[3], r[3];
                const double rr = fgr_rr(T, pr[u], q, r);
                ac = ac + fgr_weight(mu, rr) * rr;
                in[u] = rr <= delta2;
                if (in[u]) ad = ad + rr;
            }
        }
        ac = wave_sum(ac); ad = wave_sum(ad);
        __syncthreads();
        if ((tid & 63) == 0) { s_e[tid >> 6][0] = ac; s_e[tid >> 6][1] = ad; }
        __syncthreads();
        cost += ((s_e[0][0] + s_e[1][0]) + s_e[2][0]) + s_e[3][0];
        sum_d2 += ((s_e[0][1] + s_e[1][1]) + s_e[2][1]) + s_e[3][1];
#pragma unroll
        for (int u = 0; u < kScanPer; ++u) {
            const int pos = compact_slot(in[u], running);
            if (in[u]) inl[pos] = kidx[k0 + u * kBlock] + 1;
        }
    }
    n_inl = running;
}

__device__ __forceinline__ void write_failed(pcreg_fgr_result* __restrict__ out, int n, int n_live, int n_kept) {
    pcreg_fgr_result r;
#pragma unroll
    for (int e = 0; e < 16; ++e) r.T[e] = 0.0;
    r.mu0 = 0.0; r.mu_final = 0.0; r.cost = 0.0; r.sum_d2 = 0.0;
    r.failed = 1; r.n = n; r.n_live = n_live; r.n_kept = n_kept; r.n_inliers = 0; r.reserved = 0;
    *out = r;
}
__device__ __forceinline__ void write_result(pcreg_fgr_result* __restrict__ out, const double (&T)[16], double mu0, double mu, double cost, double sum_d2,
                                             int n, int n_live, int n_kept, int n_inl) {
    pcreg_fgr_result r;
#pragma unroll
    for (int e = 0; e < 16; ++e) r.T[e] = T[e];
    r.mu0 = mu0; r.mu_final = mu; r.cost = cost; r.sum_d2 = sum_d2;
    r.failed = 0; r.n = n; r.n_live = n_live; r.n_kept = n_kept; r.n_inliers = n_inl; r.reserved = 0;
    *out = r;
}
// registration b's rows; false (and the failed result written, the kept flags cleared) when it holds more than n_cap
__device__ __forceinline__ bool fgr_rows(const FgrArgs& a, int b, int& off, int& n, uint8_t*& mask) {
    off = a.offsets[b];
    n = a.offsets[b + 1] - off;
    if (n < 0) n = 0;
    mask = a.kept ? a.kept + off : a.mask + (size_t)b * a.n_cap;
    if (n <= a.n_cap) return true;
    if (a.kept) for (int i = threadIdx.x; i < n; i += kBlock) a.kept[off + i] = 0;
    if (threadIdx.x == 0) write_failed(a.out + b, n, 0, 0);
    return false;
}
__device__ __forceinline__ void start_transform(const FgrArgs& a, int b, double (&T)[16]) {
#pragma unroll
    for (int e = 0; e < 16; ++e) T[e] = a.T0 ? a.T0[(size_t)b * 16 + e] : ((e & 3) == (e >> 2) ? 1.0 : 0.0);
}

// ---- the resident form ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void fgr_resident_kernel(const FgrArgs a) {
    extern __shared__ double s_pairs[];                // [6][n]
    __shared__ double s_sum[kPlaneSums];
    const int b = blockIdx.x, tid = threadIdx.x;
    int off, n; uint8_t* mask;
    if (!fgr_rows(a, b, off, n, mask)) return;
    int32_t* kidx = a.kidx + (size_t)b * a.n_cap;
    FgrHead h;
    fgr_head(a, b, a.p1 + off, a.p2 + off, n, s_pairs, n, kidx, mask, h);
    if (h.n_kept < kFgrMinPairs) {
        if (tid == 0) write_failed(a.out + b, n, h.n_live, h.n_kept);
        return;
    }
    double T[16];
    start_transform(a, b, T);
    double mu = h.mu0;
    const int chunks = (h.n_kept + kScanChunk - 1) / kScanChunk;
    for (int it = 0; it < a.o.iterations; ++it) {
        if (it > 0 && it % a.o.decrease_every == 0) mu = fgr_mu_next(mu, a.o.division_factor, a.o.delta2);
        double tot = 0.0;
        for (int c = 0; c < chunks; ++c) tot += fgr_chunk(s_pairs, n, c, h.n_kept, T, h.o, mu);
        if (tid < kPlaneSums) s_sum[tid] = tot;
        __syncthreads();
        double sums[kPlaneSums];
#pragma unroll
        for (int k = 0; k < kPlaneSums; ++k) sums[k] = s_sum[k];
        __syncthreads();
        double S[16], Tn[16];
        if (!plane_fit(sums, 3 * h.n_kept, h.o, S)) {                      // (every thread holds the same sums: uniform)
            if (tid == 0) write_failed(a.out + b, n, h.n_live, h.n_kept);
            return;
        }
        fgr_compose(T, S, Tn);
#pragma unroll
        for (int e = 0; e < 16; ++e) T[e] = Tn[e];
    }
    double cost, sum_d2; int n_inl;
    fgr_tail(s_pairs, n, kidx, h.n_kept, T, mu, a.o.delta2, a.inlier_idx + off, cost, sum_d2, n_inl);
    if (tid == 0) write_result(a.out + b, T, h.mu0, mu, cost, sum_d2, n, h.n_live, h.n_kept, n_inl);
}

// ---- the chained form -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void fgr_prologue_kernel(const FgrArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    double* sb = a.state + (size_t)b * kFgrState;
    int off, n; uint8_t* mask;
    const bool rows_ok = fgr_rows(a, b, off, n, mask);
    FgrHead h{};
    if (rows_ok) fgr_head(a, b, a.p1 + off, a.p2 + off, n, a.staged + (size_t)b * 6 * a.n_cap, a.n_cap, a.kidx + (size_t)b * a.n_cap, mask, h);
    const bool alive = rows_ok && h.n_kept >= kFgrMinPairs;
    if (tid == 0) {
        sb[0] = h.mu0; sb[1] = h.mu0; sb[2] = h.o[0]; sb[3] = h.o[1]; sb[4] = h.o[2];
        sb[5] = alive ? 1.0 : 0.0; sb[6] = (double)h.n_kept; sb[7] = (double)h.n_live;
    }
    if (tid < 16) {
        double T[16];
        start_transform(a, b, T);
        double v = 0.0;
#pragma unroll
        for (int e = 0; e < 16; ++e) if (e == tid) v = T[e];
        a.Tpp[(size_t)b * 16 + tid] = v;
    }
}
__global__ __launch_bounds__(kBlock) void fgr_sums_kernel(const FgrArgs a, const double* __restrict__ T_in) {
    const int bl = blockIdx.x / a.chunks, c = blockIdx.x - bl * a.chunks;
    const double* sb = a.state + (size_t)bl * kFgrState;
    const int n_kept = sb[5] != 0.0 ? (int)sb[6] : 0;
    const double o[3] = {sb[2], sb[3], sb[4]};
    double T[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) T[e] = T_in[(size_t)bl * 16 + e];
    const double v = fgr_chunk(a.staged + (size_t)bl * 6 * a.n_cap, a.n_cap, c, n_kept, T, o, sb[0]);
    if (threadIdx.x < kPlaneSums) a.psums[(size_t)blockIdx.x * kPlaneSums + threadIdx.x] = v;
}
// the fit of iteration `it` and mu of the next one
__global__ __launch_bounds__(64) void fgr_finish_kernel(const FgrArgs a, const double* __restrict__ T_in, double* __restrict__ T_out, int it) {
    double* sb = a.state + (size_t)blockIdx.x * kFgrState;
    const bool alive = sb[5] != 0.0;
    const int n_kept = (int)sb[6];
    const double o[3] = {sb[2], sb[3], sb[4]};
    double sums[kPlaneSums];
    int cnt;
    const bool ok = finish_step<kPlaneSums, false>(a.psums, nullptr, a.chunks, T_in, T_out, nullptr, a.empty,
                                                   [&](const double (&s)[kPlaneSums], int, double (&T)[16]) { return alive && plane_fit(s, 3 * n_kept, o, T); },
                                                   sums, cnt);
    if (threadIdx.x == 0) {
        if (!ok) sb[5] = 0.0;
        else if (it + 1 < a.o.iterations && (it + 1) % a.o.decrease_every == 0) sb[0] = fgr_mu_next(sb[0], a.o.division_factor, a.o.delta2);
    }
}
__global__ __launch_bounds__(kBlock) void fgr_epilogue_kernel(const FgrArgs a, const double* __restrict__ T_fin) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* sb = a.state + (size_t)b * kFgrState;
    const int off = a.offsets[b];
    int n = a.offsets[b + 1] - off;
    if (n < 0) n = 0;
    if (n > a.n_cap) return;                           // (the prologue has answered)
    const int n_kept = (int)sb[6], n_live = (int)sb[7];
    if (sb[5] == 0.0) {
        if (tid == 0) write_failed(a.out + b, n, n_live, n_kept);
        return;
    }
    double T[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) T[e] = T_fin[(size_t)b * 16 + e];
    double cost, sum_d2; int n_inl;
    fgr_tail(a.staged + (size_t)b * 6 * a.n_cap, a.n_cap, a.kidx + (size_t)b * a.n_cap, n_kept, T, sb[0], a.o.delta2, a.inlier_idx + off, cost, sum_d2,
             n_inl);
    if (tid == 0) write_result(a.out + b, T, sb[1], sb[0], cost, sum_d2, n, n_live, n_kept, n_inl);
}

// Workspace, with C = max(B n_cap, 1) cells and P = B max(ceil(n_cap / 2048), 1) chunks: [kept flags, C bytes] [kept rows, C int32]
// [staged pairs, 6 C doubles] [state, 8 B doubles] [T ping and pong, 32 B doubles] [chunk sums, 28 P doubles] [empty, B int32], each
// rounded up to 256 bytes.  The resident form uses the first two only; one size serves both, so the key changes no call.
void fgr_ws_layout(int n_cap, int B, void* base, FgrArgs& a, size_t* bytes) {
    const size_t cells = std::max((size_t)B * (size_t)n_cap, (size_t)1);
    a.chunks = scan_chunks(n_cap);
    WsWalk w(base);
    a.mask = w.take<uint8_t>(cells);
    a.kidx = w.take<int32_t>(cells);
    a.staged = w.take<double>(6 * cells);
    a.state = w.take<double>((size_t)kFgrState * B);
    a.Tpp = w.take<double>((size_t)32 * B);
    a.psums = w.take<double>((size_t)kPlaneSums * B * a.chunks);
    a.empty = w.take<int32_t>((size_t)B);
    *bytes = w.bytes();
}

}  // namespace

bool fgr_args_ok(const pcreg_fgr_opts& o) {
    return o.delta2 >= 0.0 && std::isfinite(o.delta2) && o.iterations >= 1 && o.decrease_every >= 1 && o.division_factor > 1.0 &&
           std::isfinite(o.division_factor) && o.mu0 >= 0.0 && std::isfinite(o.mu0) && o.n_tuples >= 0 && o.tuple_scale > 0.0 && o.tuple_scale <= 1.0;
}
int fgr_resident_capacity() { return kFgrResident; }

size_t fgr_ws_bytes(int n_cap, int B, int iterations) {
    if (n_cap < 0 || B < 1 || iterations < 1 || (size_t)B * (size_t)n_cap > kFgrMaxCells) return 0;
    FgrArgs a{}; size_t b;
    fgr_ws_layout(n_cap, B, nullptr, a, &b);
    return b;
}

int launch_fgr(const double* p1, const double* p2, int ld, const int32_t* offsets, int B, int n_cap, const pcreg_fgr_opts& o, const double* T0,
               const int32_t* tuple_idx, pcreg_fgr_result* out, int32_t* inlier_idx, uint8_t* kept, void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(B >= 1 && n_cap >= 0 && ld >= 0 && fgr_args_ok(o) && (size_t)B * (size_t)n_cap <= kFgrMaxCells);
    FgrArgs a{};
    size_t need;
    fgr_ws_layout(n_cap, B, ws, a, &need);
    if (ws_bytes < need) {
        set_error("fast global registration workspace too small: %zu < %zu", ws_bytes, need);
        return PCREG_E_WORKSPACE;
    }
    a.p1 = p1; a.p2 = p2; a.ld = ld; a.offsets = offsets; a.B = B; a.n_cap = n_cap; a.o = o; a.T0 = T0;
    a.tuple_idx = o.n_tuples > 0 ? tuple_idx : nullptr;
    a.out = out; a.inlier_idx = inlier_idx; a.kept = kept;
    if (n_cap <= kFgrResident && !debug_flag(kDbgFgrChain)) {
        // (on every call: the attribute belongs to the device that is current, and setting it costs next to nothing)
        PCREG_HIP(hipFuncSetAttribute((const void*)fgr_resident_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 48 * kFgrResident));
        hipLaunchKernelGGL(fgr_resident_kernel, dim3((unsigned)B), dim3(kBlock), 48 * (size_t)std::max(n_cap, 1), st, a);
        PCREG_HIP(hipGetLastError());
        return PCREG_OK;
    }
    hipLaunchKernelGGL(fgr_prologue_kernel, dim3((unsigned)B), dim3(kBlock), 0, st, a);
    for (int it = 0; it < o.iterations; ++it) {
        const double* T_in = a.Tpp + (size_t)(it & 1) * 16 * B;
        double* T_out = a.Tpp + (size_t)((it + 1) & 1) * 16 * B;
        hipLaunchKernelGGL(fgr_sums_kernel, dim3((unsigned)((size_t)B * a.chunks)), dim3(kBlock), 0, st, a, T_in);
        hipLaunchKernelGGL(fgr_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, a, T_in, T_out, it);
    }
    hipLaunchKernelGGL(fgr_epilogue_kernel, dim3((unsigned)B), dim3(kBlock), 0, st, a, (const double*)(a.Tpp + (size_t)(o.iterations & 1) * 16 * B));
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
