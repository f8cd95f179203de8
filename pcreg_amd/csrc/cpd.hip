// pcreg_amd/csrc/cpd.hip -- one coherent-point-drift step of B candidate transforms of one query cloud against a PREPARED model
// (pcreg_model_refit_cpd_f32's contract, include/pcreg.h): every moved point is paired SOFTLY with every live
// model row by a Gaussian of their distance against a uniform outlier term, and the weighted rigid fit (cpd_fit.hpp) follows.
// The cost is B * Q * M pairs a step: this is for downsampled clouds (10^3 .. 10^4 points a side).
//
//   D0  launch_model_score at r2 = +inf   the SHIFT dmin [B][Q]: the scoring chain as it is (its walk, its culling, its batches);
//                                         sum_d2 is its sum, the same bits pcreg_model_score_f32 gives
//   D1  cpd_model_sums_kernel             one workgroup: the origin o (the middle of the live rows' box), then the live rows' number,
//                                         sum v and sum |v|^2, v = m - o, in double; thread t adds ORIGINAL rows t, t + 256, .. in
//                                         order, chunk_tail_few
// and per batch of whole transforms (at most 128 Ki query slots):
//   D2  cpd_query_sums_kernel             per (transform, chunk of 2048 queries): the moved points p' (moved_point: scoring's) into
//                                         tq, the live ones' number, sum u and sum |u|^2, u = p' - o; thread t adds its 8
//                                         consecutive queries in order, chunk_tail_few
//   D3  cpd_param_kernel                  thread per transform: the chunks ascending, the live count, sigma2 (the closed-form initial
//                                         value where sigma2_in == 0), h = 1 / (2 sigma2), k2 = (float)(-(h log2 e)), c
//   D4  cpd_weights_kernel                THE HOT PATH: per (transform, chunk, slice of the model's rows, ORIGINAL order): 8 queries a thread
//                                         in registers, the slice's LIVE rows staged 256 at a time through LDS (compacted by a
//                                         ballot, read at one address by all lanes: a broadcast), per pair three subtractions, the
//                                         distance, one exp2 and the five fp32 sums S, V[3], W of e, e (m - p'), e d2
//   D5  cpd_moments_kernel                per (transform, chunk): a query's slices added in ascending order in fp32, then in double
//                                         g, p and the 19 sums of cpd_fit.hpp in query order; chunk_tail
//   D6  cpd_finish_kernel                 per transform: finish_step with cpd_fit about the origin o
// The step's skeleton -- the moved point, the chunk tail, the finish step, T * T_step and the empty rule -- is refit_step.hpp's
// (DESIGN 4.28).
// Every sum's order is a function of (Q, M) alone: no floating-point atomic, the rows are read in their original order (the prepared
// model's sorted copy is placed by atomics and differs from one preparation to the next) and the slice count depends on M only, so a
// candidate's bits do not depend on B, on its place, on the batch, on the stream or on which handle holds the model.
#include "common.hpp"
#include "knn_fast_common.hpp"
#include "knn_walk.hpp"
#include "refit_step.hpp"
#include "cpd_fit.hpp"
#include <cmath>

namespace pcreg {

namespace {

constexpr int kCpdSlots = 128 << 10;              // query slots per batch of D2 .. D6
constexpr int kCpdTile = kBlock;                  // rows staged at a time
constexpr int kCpdMaxSlices = 32;
constexpr int kCpdPar = 6;                        // per transform: sigma2, h, c, ok, k2, -
constexpr int kCpdQSums = 4;                      // sum u (3), sum |u|^2
static_assert(kScanBlock == kBlock && kScanPer == 8, "a thread owns 8 queries of a chunk of 2048");

int cpd_batch(int Q, int B) { return std::max(1, std::min(B, kCpdSlots / (Q > 0 ? Q : 1))); }
// the slices of the model's rows: whole tiles of 256 rows, at most 32 slices -- a function of M alone
int cpd_slice_rows(int M) {
    const int tiles = std::max(1, (M + kCpdTile - 1) / kCpdTile);
    return kCpdTile * ((tiles + kCpdMaxSlices - 1) / kCpdMaxSlices);
}
int cpd_slices(int M) { const int sr = cpd_slice_rows(M); return std::max(1, (M + sr - 1) / sr); }

// ---- D1. the origin and the model's sums --------------------------------------------------------------------------------
// One workgroup, rows in ORIGINAL order (thread t: rows t, t + 256, ..), a row LIVE when its three coordinates are finite.
// Pass 1: the live rows' box (min and max are exact, whatever the order) and o = 0.5f lo + 0.5f hi in fp32 -- the prepared model's
// centre (Prep::cx, cy, cz: pcreg_model_refit_f32's origin) whenever that is finite; an infinite row spoils the prepared one, not this.
// Pass 2, about o, v = m - o: msum[0..2] = sum v, [3] = sum |v|^2 with |v|^2 = (v0 v0 + v1 v1) + v2 v2, [4] = the number of live rows
// (a double: exact), [5..7] = o.
__global__ __launch_bounds__(kBlock) void cpd_model_sums_kernel(const float* __restrict__ m, int M, int ldm, double* __restrict__ msum) {
    __shared__ float s_box[kBlock / 64][6];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int r = threadIdx.x; r < M; r += kBlock) {
        const float x = m[r], y = m[r + (size_t)ldm], z = m[r + 2 * (size_t)ldm];
        if (finite3(x, y, z)) {
            lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
            hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s_box[threadIdx.x >> 6][c] = lo[c]; s_box[threadIdx.x >> 6][3 + c] = hi[c]; }
    }
    __syncthreads();
    float of[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float l = fminf(fminf(s_box[0][c], s_box[1][c]), fminf(s_box[2][c], s_box[3][c]));
        const float h = fmaxf(fmaxf(s_box[0][3 + c], s_box[1][3 + c]), fmaxf(s_box[2][3 + c], s_box[3][3 + c]));
        of[c] = 0.5f * l + 0.5f * h;
    }
    const double ox = (double)of[0], oy = (double)of[1], oz = (double)of[2];
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < M; r += kBlock) {
        const float x = m[r], y = m[r + (size_t)ldm], z = m[r + 2 * (size_t)ldm];
        if (finite3(x, y, z)) {
            const double v0 = (double)x - ox, v1 = (double)y - oy, v2 = (double)z - oz;
            a[0] = a[0] + v0; a[1] = a[1] + v1; a[2] = a[2] + v2;
            a[3] = a[3] + ((v0 * v0 + v1 * v1) + v2 * v2);
            a[4] = a[4] + 1.0;
        }
    }
    chunk_tail_few(a, msum);                                      // (one workgroup: msum[0 .. 4])
    if (threadIdx.x == 0) { msum[5] = ox; msum[6] = oy; msum[7] = oz; }
}

// ---- D2. the moved points and the queries' sums -------------------------------------------------------------------------
// workgroup bl * chunks + c, thread t: queries c * 2048 + 8 t .. + 7.  p' is moved_point (refit_step.hpp), as in
// score_transform_kernel: an all-zero transform's are NaN.  A query is LIVE when its p' has three finite coordinates.
__global__ __launch_bounds__(kBlock) void cpd_query_sums_kernel(const float* __restrict__ q, int Q, int ldq, const double* __restrict__ T, int S, int chunks,
                                                                const double* __restrict__ msum, float* __restrict__ tq, double* __restrict__ pq,
                                                                int32_t* __restrict__ pql) {
    const int bl = blockIdx.x / chunks, c = blockIdx.x - bl * chunks;
    const int i0 = c * kScanChunk + threadIdx.x * kScanPer;
    const double ox = msum[5], oy = msum[6], oz = msum[7];
    double t[16];
    const bool empty = load_transform(T, bl, t);
    double a[kCpdQSums] = {0.0, 0.0, 0.0, 0.0};
    int32_t cnt = 0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const int i = i0 + u;
        if (i < Q) {
            const double x = (double)q[i], y = (double)q[i + (size_t)ldq], z = (double)q[i + 2 * (size_t)ldq];
            float p[3];
            moved_point(t, x, y, z, empty, p);
            const size_t s = (size_t)bl * Q + i;
            tq[s] = p[0]; tq[s + (size_t)S] = p[1]; tq[s + 2 * (size_t)S] = p[2];
            if (finite3(p[0], p[1], p[2])) {
                const double u0 = (double)p[0] - ox, u1 = (double)p[1] - oy, u2 = (double)p[2] - oz;
                a[0] = a[0] + u0; a[1] = a[1] + u1; a[2] = a[2] + u2;
                a[3] = a[3] + ((u0 * u0 + u1 * u1) + u2 * u2);
                ++cnt;
            }
        }
    }
    chunk_tail_few(a, pq);
    chunk_sum(cnt, pql);
}

// ---- D3. the parameters of a transform ----------------------------------------------------------------------------------
// thread bl.  ok = 0 (the candidate is empty and D4 / D5 skip it) for a T that is all zero or not finite, Ql < 3, Ml < 3, a
// sigma2_in that is negative or NaN, and a sigma2, h or k2 that is not a finite number above 0 (k2: below 0).
__global__ __launch_bounds__(kBlock) void cpd_param_kernel(const double* __restrict__ pq, const int32_t* __restrict__ pql, int nb, int chunks,
                                                           const double* __restrict__ msum, const double* __restrict__ T, const double* __restrict__ sigma2_in,
                                                           double w, double* __restrict__ par, int32_t* __restrict__ n_live) {
    const int bl = blockIdx.x * kBlock + threadIdx.x;
    if (bl >= nb) return;
    bool t_zero = true, t_fin = true;
    for (int e = 0; e < 16; ++e) { const double v = T[(size_t)bl * 16 + e]; t_zero = t_zero && v == 0.0; t_fin = t_fin && fit_cylinders_finite(v); }
    double su[3] = {0.0, 0.0, 0.0}, suu = 0.0;
    int32_t ql = 0;
    for (int c = 0; c < chunks; ++c) {
        const double* p = pq + ((size_t)bl * chunks + c) * kCpdQSums;
        su[0] = su[0] + p[0]; su[1] = su[1] + p[1]; su[2] = su[2] + p[2]; suu = suu + p[3];
        ql += pql[(size_t)bl * chunks + c];
    }
    const double ml = msum[4], dq = (double)ql;
    double s2 = sigma2_in[bl];
    bool ok = !t_zero && t_fin && ql >= 3 && ml >= 3.0 && s2 >= 0.0;
    if (ok && s2 == 0.0) {                                        // the mean squared distance over all live pairs, over 3
        const double mu[3] = {su[0] / dq, su[1] / dq, su[2] / dq}, mv[3] = {msum[0] / ml, msum[1] / ml, msum[2] / ml};
        s2 = ((suu / dq + msum[3] / ml) - 2.0 * ((mu[0] * mv[0] + mu[1] * mv[1]) + mu[2] * mv[2])) / 3.0;
    }
    ok = ok && s2 > 0.0 && fit_cylinders_finite(s2);
    const double h = ok ? 1.0 / (2.0 * s2) : 0.0;
    const float k2 = (float)(-(h * 1.4426950408889634));
    ok = ok && h > 0.0 && fit_cylinders_finite(h) && k2 < 0.0f && k2 > -INFINITY;
    double cc = 0.0;
    if (ok && w > 0.0) {
        const double tp = 6.283185307179586 * s2;
        cc = ((tp * sqrt(tp)) * (w / (1.0 - w))) * (ml / dq);
    }
    double* o = par + (size_t)bl * kCpdPar;
    o[0] = ok ? s2 : 0.0; o[1] = h; o[2] = cc; o[3] = ok ? 1.0 : 0.0; o[4] = (double)k2; o[5] = 0.0;
    n_live[bl] = ql;
}

// ---- D4. the weights ----------------------------------------------------------------------------------------------------
// workgroup ((bl * chunks + c) * n_slices + sl): queries c * 2048 + u * 256 + tid (u = 0 .. 7: coalesced) of transform bl against
// the original rows [sl * slice_rows, min(M, (sl + 1) * slice_rows)).  A tile of 256 rows is loaded one row a thread; the live ones
// are written to LDS in ascending order (a ballot per wave, the four waves' counts through LDS), so the pair loop meets live
// rows only and every lane reads the same address.  Per pair, fp32: dx = m - p' by component (the DIFFERENCE is what is summed:
// 170 units from the origin the coordinates would cancel), d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) -- the library's distance; the sign
// of dx does not reach it --, e = exp2((d2 - dmin) * k2) (v_exp_f32; the argument is <= 0 because dmin is the minimum of the same
// bits), S += e, V = fmaf(e, dx, V), W = fmaf(e, d2, W): a slice's sums run over its live rows in ascending original order from 0.
// part [n_slices][5][S]: S, Vx, Vy, Vz, W of (slice, slot).  A query that is not live computes garbage nobody reads.
__global__ __launch_bounds__(kBlock) void cpd_weights_kernel(const float* __restrict__ tq, const float* __restrict__ dmin, int Q, int S, int chunks,
                                                             int n_slices, int slice_rows, const float* __restrict__ m, int M, int ldm,
                                                             const double* __restrict__ par, float* __restrict__ part) {
    __shared__ float4 s_row[kCpdTile];
    __shared__ int s_cnt[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sl = blockIdx.x % n_slices, bc = blockIdx.x / n_slices;
    const int bl = bc / chunks, c = bc - bl * chunks;
    const double* pb = par + (size_t)bl * kCpdPar;
    if (pb[3] == 0.0) return;                                     // (the whole workgroup: an empty candidate's partials are never read)
    const float k2 = (float)pb[4];
    float px[kScanPer], py[kScanPer], pz[kScanPer], dm[kScanPer], aS[kScanPer], aX[kScanPer], aY[kScanPer], aZ[kScanPer], aW[kScanPer];
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const int i = c * kScanChunk + u * kBlock + tid;
        const bool in = i < Q;
        const size_t s = (size_t)bl * Q + (in ? i : 0);
        px[u] = in ? tq[s] : 0.0f; py[u] = in ? tq[s + (size_t)S] : 0.0f; pz[u] = in ? tq[s + 2 * (size_t)S] : 0.0f;
        dm[u] = in ? dmin[s] : 0.0f;
        aS[u] = 0.0f; aX[u] = 0.0f; aY[u] = 0.0f; aZ[u] = 0.0f; aW[u] = 0.0f;
    }
    const int r_begin = sl * slice_rows, r_end = min(M, r_begin + slice_rows);
    for (int r0 = r_begin; r0 < r_end; r0 += kCpdTile) {
        const int r = r0 + tid;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        bool lv = false;
        if (r < r_end) {
            x = m[r]; y = m[r + (size_t)ldm]; z = m[r + 2 * (size_t)ldm];
            lv = finite3(x, y, z);
        }
        const unsigned long long bal = __ballot(lv);
        __syncthreads();                                          // the tile before this one has been read
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int base = 0, n = 0;
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) { base += k < wave ? s_cnt[k] : 0; n += s_cnt[k]; }
        if (lv) s_row[base + __popcll(bal & ((1ull << lane) - 1ull))] = make_float4(x, y, z, 0.0f);
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            const float4 mr = s_row[j];
#pragma unroll
            for (int u = 0; u < kScanPer; ++u) {
                const float dx = mr.x - px[u], dy = mr.y - py[u], dz = mr.z - pz[u];
                const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                const float e = __builtin_amdgcn_exp2f((d - dm[u]) * k2);
                aS[u] = aS[u] + e;
                aX[u] = __builtin_fmaf(e, dx, aX[u]);
                aY[u] = __builtin_fmaf(e, dy, aY[u]);
                aZ[u] = __builtin_fmaf(e, dz, aZ[u]);
                aW[u] = __builtin_fmaf(e, d, aW[u]);
            }
        }
    }
    float* out = part + (size_t)sl * 5 * (size_t)S;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const int i = c * kScanChunk + u * kBlock + tid;
        if (i < Q) {
            const size_t s = (size_t)bl * Q + i;
            out[s] = aS[u]; out[s + (size_t)S] = aX[u]; out[s + 2 * (size_t)S] = aY[u]; out[s + 3 * (size_t)S] = aZ[u]; out[s + 4 * (size_t)S] = aW[u];
        }
    }
}

// ---- D5. the weighted sums ----------------------------------------------------------------------------------------------
// workgroup bl * chunks + c and thread t as plane_moments_kernel: its 8 consecutive queries in order.  Per live query: S, V, W each
// the slices' partials added in ascending slice order in fp32 from the first; then in double on the widened values, without
// contraction: out = c * exp(dmin * h) (0 when c == 0, whatever the exponential), g = 1 / (S + out), p = g * S, u = p' - o,
// gV = g * V, y = p * u + gV by component, uu = (u0 u0 + u1 u1) + u2 u2, gW = g * W, and cpd_fit.hpp's 19 sums, each sum = sum + term:
// p;  p * u_a;  y_a;  u_a * y_b;  p * uu;  (p * uu + 2 * ((u0 gV0 + u1 gV1) + u2 gV2)) + gW;  gW.
// chunk_tail on the 19.
__global__ __launch_bounds__(kBlock) void cpd_moments_kernel(const float* __restrict__ tq, const float* __restrict__ dmin, const float* __restrict__ part,
                                                             int n_slices, int Q, int S, int chunks, const double* __restrict__ par,
                                                             const double* __restrict__ msum, double* __restrict__ pmom) {
    const int bl = blockIdx.x / chunks, c = blockIdx.x - bl * chunks;
    const int i0 = c * kScanChunk + threadIdx.x * kScanPer;
    const double* pb = par + (size_t)bl * kCpdPar;
    const double h = pb[1], cc = pb[2];
    const bool ok = pb[3] != 0.0;
    const double ox = msum[5], oy = msum[6], oz = msum[7];
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const int i = i0 + u;
        if (!ok || i >= Q) continue;
        const size_t s = (size_t)bl * Q + i;
        const float p0 = tq[s], p1 = tq[s + (size_t)S], p2 = tq[s + 2 * (size_t)S];
        if (!finite3(p0, p1, p2)) continue;
        float fS = part[s], fX = part[s + (size_t)S], fY = part[s + 2 * (size_t)S], fZ = part[s + 3 * (size_t)S], fW = part[s + 4 * (size_t)S];
        for (int sl = 1; sl < n_slices; ++sl) {
            const float* ps = part + (size_t)sl * 5 * (size_t)S + s;
            fS = fS + ps[0]; fX = fX + ps[(size_t)S]; fY = fY + ps[2 * (size_t)S]; fZ = fZ + ps[3 * (size_t)S]; fW = fW + ps[4 * (size_t)S];
        }
        const double Sd = (double)fS, dmd = (double)dmin[s];
        const double outl = cc > 0.0 ? cc * exp(dmd * h) : 0.0;
        const double g = 1.0 / (Sd + outl), p = g * Sd;
        const double u0 = (double)p0 - ox, u1 = (double)p1 - oy, u2 = (double)p2 - oz;
        const double gV0 = g * (double)fX, gV1 = g * (double)fY, gV2 = g * (double)fZ, gW = g * (double)fW;
        const double y0 = p * u0 + gV0, y1 = p * u1 + gV1, y2 = p * u2 + gV2;
        const double uu = (u0 * u0 + u1 * u1) + u2 * u2;
        acc[0] = acc[0] + p;
        acc[1] = acc[1] + p * u0; acc[2] = acc[2] + p * u1; acc[3] = acc[3] + p * u2;
        acc[4] = acc[4] + y0; acc[5] = acc[5] + y1; acc[6] = acc[6] + y2;
        acc[7] = acc[7] + u0 * y0; acc[8] = acc[8] + u0 * y1; acc[9] = acc[9] + u0 * y2;
        acc[10] = acc[10] + u1 * y0; acc[11] = acc[11] + u1 * y1; acc[12] = acc[12] + u1 * y2;
        acc[13] = acc[13] + u2 * y0; acc[14] = acc[14] + u2 * y1; acc[15] = acc[15] + u2 * y2;
        acc[16] = acc[16] + p * uu;
        acc[17] = acc[17] + ((p * uu + 2.0 * ((u0 * gV0 + u1 * gV1) + u2 * gV2)) + gW);
        acc[18] = acc[18] + gW;
    }
    chunk_tail<kCpdSums>(acc, 0.0, pmom);
}

// ---- D6. the fit --------------------------------------------------------------------------------------------------------
// finish_step (refit_step.hpp) over the 19 sums: cpd_fit about the origin they were taken about, unless D3 refused the candidate.
// empty: sigma2_out = 0 beside the 32 zeros.
__global__ __launch_bounds__(64) void cpd_finish_kernel(const double* __restrict__ pmom, int chunks, const double* __restrict__ par,
                                                        const double* __restrict__ msum, const double* __restrict__ T_in, double* __restrict__ T_out,
                                                        double* __restrict__ T_step, double* __restrict__ sigma2_out, double* __restrict__ Np,
                                                        double* __restrict__ sum_res2, int32_t* __restrict__ empty) {
    const int bl = blockIdx.x;
    const bool in_ok = par[(size_t)bl * kCpdPar + 3] != 0.0;
    const double o[3] = {msum[5], msum[6], msum[7]};
    double sums[kCpdSums], sig = 0.0;
    int cnt;
    const bool ok = finish_step<kCpdSums, false>(pmom, nullptr, chunks, T_in, T_out, T_step, empty,
                                                 [&](const double (&s)[kCpdSums], int, double (&T)[16]) { return in_ok && cpd_fit(s, o, T, sig); }, sums, cnt);
    if (threadIdx.x == 0) { sigma2_out[bl] = ok ? sig : 0.0; Np[bl] = sums[0]; sum_res2[bl] = sums[18]; }
}

// Workspace, with nb = max(1, min(B, floor(128 Ki / max(Q, 1)))) transforms a batch, S = max(nb Q, 1) slots, P = nb max(ceil(Q / 2048),
// 1) partials and L = the slices of M (cpd_slices): [the scoring workspace of (Q, B)] [dmin, max(B Q, 1) floats] [hits per
// transform, max(B, 1) int32] [the model's sums, 8 doubles] [moved points, 3 S floats] [chunk query sums, 4 P doubles] [chunk live
// counts, P int32] [parameters, 6 nb doubles] [slice partials, 5 L S floats] [chunk sums, 19 P doubles]:
// score(Q, B) + roundup(4 max(B Q, 1), 256) + roundup(4 max(B, 1), 256) + 256 + roundup(12 S, 256) + roundup(32 P, 256) +
// roundup(4 P, 256) + roundup(48 nb, 256) + roundup(20 L S, 256) + roundup(152 P, 256) bytes
struct CpdWs { void* score; size_t score_bytes; float* dmin; int32_t* hits; double* msum; float* tq; double* pq; int32_t* pql; double* par; float* part; double* pmom; };
CpdWs cpd_ws_layout(int Q, int B, int M, void* base, size_t* bytes) {
    CpdWs s{};
    const int nb = cpd_batch(Q, B);
    const size_t S = std::max((size_t)nb * (size_t)(Q > 0 ? Q : 0), (size_t)1), P = (size_t)nb * scan_chunks(Q), L = (size_t)cpd_slices(M);
    WsWalk w(base);
    s.score_bytes = score_ws_bytes(Q, B, M);
    s.score = w.take_bytes(align_up(s.score_bytes, 256));
    s.dmin = w.take<float>(std::max((size_t)B * (size_t)(Q > 0 ? Q : 0), (size_t)1));
    s.hits = w.take<int32_t>(std::max((size_t)B, (size_t)1));
    s.msum = w.take<double>(8);
    s.tq = w.take<float>(3 * S);
    s.pq = w.take<double>(kCpdQSums * P);
    s.pql = w.take<int32_t>(P);
    s.par = w.take<double>((size_t)kCpdPar * nb);
    s.part = w.take<float>(5 * L * S);
    s.pmom = w.take<double>((size_t)kCpdSums * P);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t refit_cpd_ws_bytes(int Q, int B, int M) {
    if (Q < 0 || B < 0 || M < 0 || Q > (4 << 20)) return 0;
    size_t b; (void)cpd_ws_layout(Q, B, M, nullptr, &b);
    return b;
}

int launch_model_refit_cpd(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, const double* sigma2_in, double outlier,
                           double* T_out, double* T_step, double* sigma2_out, double* Np, double* sum_res2, double* sum_d2, int32_t* n_live,
                           int32_t* empty, void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(Q >= 0 && B >= 0 && ldq >= Q && Q <= (4 << 20) && outlier >= 0.0 && outlier < 1.0);
    size_t need;
    const CpdWs s = cpd_ws_layout(Q, B, v.M, ws, &need);
    if (ws_bytes < need) {
        set_error("bad argument: coherent-point-drift refit workspace too small: %zu < %zu", ws_bytes, need);
        return PCREG_E_ARG;
    }
    if (B == 0) return PCREG_OK;
    if (Q == 0 || v.M == 0) {
        return launch_refit_empty(B, T_out, T_step, empty, RefitEmptyOuts{{sigma2_out, Np, sum_res2, sum_d2}, n_live}, st);
    }
    int rc = launch_model_score(v, q, Q, ldq, T_dev, B, INFINITY, s.hits, sum_d2, nullptr, s.dmin, s.score, s.score_bytes, st);
    if (rc) return rc;
    const double* msum = s.msum;
    hipLaunchKernelGGL(cpd_model_sums_kernel, dim3(1), dim3(kBlock), 0, st, v.m, v.M, v.ldm, s.msum);
    PCREG_HIP(hipGetLastError());
    const int dbg_slots = debug_flag(kDbgScoreBatchSlots);        // "score_batch_slots": a lower cap here too, same results
    const int nb_max = dbg_slots > 0 ? std::max(1, std::min(cpd_batch(Q, B), dbg_slots / Q)) : cpd_batch(Q, B);
    const int chunks = scan_chunks(Q), n_slices = cpd_slices(v.M), slice_rows = cpd_slice_rows(v.M);
    for (int b0 = 0; b0 < B; b0 += nb_max) {
        const int nb = std::min(nb_max, B - b0), S = nb * Q;
        const double* Tb = T_dev + (size_t)b0 * 16;
        const float* dmin = s.dmin + (size_t)b0 * Q;
        hipLaunchKernelGGL(cpd_query_sums_kernel, dim3((unsigned)(nb * chunks)), dim3(kBlock), 0, st, q, Q, ldq, Tb, S, chunks, msum, s.tq, s.pq, s.pql);
        hipLaunchKernelGGL(cpd_param_kernel, dim3((nb + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const double*)s.pq, (const int32_t*)s.pql, nb, chunks,
                           msum, Tb, sigma2_in + b0, outlier, s.par, n_live + b0);
        hipLaunchKernelGGL(cpd_weights_kernel, dim3((unsigned)(nb * chunks * n_slices)), dim3(kBlock), 0, st, (const float*)s.tq, dmin, Q, S, chunks,
                           n_slices, slice_rows, v.m, v.M, v.ldm, (const double*)s.par, s.part);
        hipLaunchKernelGGL(cpd_moments_kernel, dim3((unsigned)(nb * chunks)), dim3(kBlock), 0, st, (const float*)s.tq, dmin, (const float*)s.part, n_slices,
                           Q, S, chunks, (const double*)s.par, msum, s.pmom);
        hipLaunchKernelGGL(cpd_finish_kernel, dim3(nb), dim3(64), 0, st, (const double*)s.pmom, chunks, (const double*)s.par, msum, Tb,
                           T_out + (size_t)b0 * 16, T_step ? T_step + (size_t)b0 * 16 : nullptr, sigma2_out + b0, Np + b0, sum_res2 + b0, empty + b0);
        PCREG_HIP(hipGetLastError());
    }
    return PCREG_OK;
}

}  // namespace pcreg
