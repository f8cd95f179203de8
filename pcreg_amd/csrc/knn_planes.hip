// pcreg_amd/csrc/knn_planes.hip -- MSAC plane fitting and plane extraction on a PREPARED model (MATLAB's pcfitplane and the
// fit / remove / fit-again loop of every segmentation example): up to P planes in one launch chain, nothing read on the host.
// The contract is pcreg_model_fit_planes_f32's (include/pcreg.h); DESIGN 4.21.
//
// The model's rows are read through v.m, by ORIGINAL row.  A call is two launches and then nine per round p:
//   Z   pl_reset_kernel      one workgroup: the state, the per-round sums and the P-sized outputs to zero
//   I   pl_init_kernel       labels = 0, the alive byte of every row (its three coordinates finite), the box of the finite rows by
//                            integer atomic min / max on order-preserving words
//   A1  pl_count_kernel      chunk_scan.hpp's first launch over the alive bytes
//   A2  pl_list_kernel       its second: the alive rows ascending, their coordinates packed behind them, their number nA
//   H   pl_hyp_kernel        one thread per trial: the three sample rows, the checks, n in double, its sign, (p0, nf, void); the
//                            trial's cost and count to zero
//   S   pl_score_kernel      THE HOT PATH: lane = trial.  A workgroup stages 2048 alive rows in LDS and each of its 256 lanes walks
//                            them with its own plane in registers (the LDS reads are wave-uniform: a broadcast, no bank conflict), so
//                            a (trial, row) pair costs no cross-lane step; one 64-bit and one 32-bit integer atomic per (chunk, trial)
//   B   pl_select_kernel     one workgroup: the smallest (cost, b) among the eligible trials; the stop rule; the diagnostics
//   R   pl_refit_kernel      the best trial's inliers: g = rint(d 2^(17 - e)), the ten integer sums by wave and LDS reduction, ten
//                            atomics a workgroup
//   E   pl_plane_kernel      one thread: N in 128 bits, jacobi_sym3, the sign, the centre, d4
//   C   pl_classify_kernel   the final fp32 classification: labels, alive bytes, the round's count and Q by integer atomics
//   F   pl_finish_kernel     one thread: counts, rmse, n_planes = p + 1
// Every sum across rows is an INTEGER sum: no order of summation, no floating-point atomic.  A device word says that extraction has
// ended; every later launch reads it and returns.  Nothing synchronises; no workgroup waits for another.
#include "common.hpp"
#include "knn_walk.hpp"                              // finite3
#include "chunk_scan.hpp"
#include "wave_math.hpp"
#include <cmath>

namespace pcreg {

namespace {

constexpr int kPlMaxM = 1 << 26;                     // below it no sum overflows: |g| <= 2^17, so |S2| <= 2^26 2^34 = 2^60
constexpr int kPlMaxPlanes = 64;
constexpr int kPlMaxTrials = 1 << 20;
constexpr int kPlBlock = 256;
constexpr int kPlChunk = kScanChunk;                 // alive rows per scoring workgroup
constexpr int kPlQMax = 1 << 20;

struct PlState {
    unsigned box[6];                                 // lo x y z, hi x y z of the finite rows as order-preserving words
    int done, nA;
    int best_b, best_count;
    long long best_cost;
    float p0[3], nf[3];                              // the best trial's plane (the refit's inlier test)
    float cf[3], nn[3];                              // (float)centre and (float)normal of the refit (the classification)
    long long sums[kPlMaxPlanes][10];                // per round: n, S1 x y z, S2 xx xy xz yy yz zz
    unsigned long long tot[kPlMaxPlanes][2];         // per round: count_p, Q_p
};

// ransac.hip's sampler hash
__device__ __forceinline__ unsigned long long pl_splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull; unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// a float as a word whose unsigned order is the float's, and back
__device__ __forceinline__ unsigned ord_of(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_back(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
// frexp's exponent of the largest axis extent of the finite rows (0 where there is none or it is zero)
__device__ __forceinline__ int pl_exponent(const PlState* __restrict__ st) {
    double D = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned lo = st->box[c], hi = st->box[3 + c];
        if (lo <= hi) D = fmax(D, (double)ord_back(hi) - (double)ord_back(lo));
    }
    int e = 0;
    if (D > 0.0) (void)frexp(D, &e);
    return e;
}
// a 128-bit integer rounded ONCE to double (knn_iss.hip's construction)
__device__ __forceinline__ double pl_i128_to_double(__int128 v) {
    const bool neg = v < 0;
    const unsigned __int128 u = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    const unsigned long long hi = (unsigned long long)(u >> 64), lo = (unsigned long long)u;
    double r;
    if (hi == 0) r = (double)lo;
    else {
        const int sh = __clzll((long long)hi);
        const unsigned long long top = sh ? (hi << sh) | (lo >> (64 - sh)) : hi;
        const unsigned long long rest = sh ? lo << sh : lo;
        r = ldexp((double)(top | (rest ? 1ull : 0ull)), 64 - sh);
    }
    return neg ? -r : r;
}
// the contract's scoring chain for one row: r2 of the row against (origin o, normal n), and its q
__device__ __forceinline__ float pl_r2(float x, float y, float z, float ox, float oy, float oz, float nx, float ny, float nz) {
    const float dx = x - ox, dy = y - oy, dz = z - oz;
    const float r = fmaf(nz, dz, fmaf(ny, dy, nx * dx));
    return r * r;
}
__device__ __forceinline__ int pl_q(float r2, float s) {     // min(2^20, rint(r2 s)); rint is monotone, so the cap may come first
    return (int)rintf(fminf(r2 * s, (float)kPlQMax));
}
// the sign rule: with a reference vector, negate when n . ref < 0; without, the component of largest magnitude positive
__device__ __forceinline__ double pl_dot_ref(const double n[3], double rx, double ry, double rz) {
    return (n[0] * rx + n[1] * ry) + n[2] * rz;
}
__device__ __forceinline__ bool pl_negate_largest(const double n[3]) {
    int c = 0;
    if (fabs(n[1]) > fabs(n[c])) c = 1;
    if (fabs(n[2]) > fabs(n[c])) c = 2;
    return n[c] < 0.0;
}

// ---- Z, I. reset and the alive rows ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlBlock) void pl_reset_kernel(PlState* __restrict__ st, int P, double* __restrict__ planes,
                                                            double* __restrict__ centres, int32_t* __restrict__ counts,
                                                            double* __restrict__ rmse, int32_t* __restrict__ n_planes,
                                                            int32_t* __restrict__ best_trial, long long* __restrict__ best_cost,
                                                            int32_t* __restrict__ best_count) {
    const int tid = threadIdx.x;
    unsigned* w = (unsigned*)st;
    for (int i = tid; i < (int)(sizeof(PlState) / 4); i += kPlBlock) w[i] = 0u;
    __syncthreads();
    if (tid < 3) { st->box[tid] = 0xFFFFFFFFu; st->box[3 + tid] = 0u; }
    for (int i = tid; i < P; i += kPlBlock) {
        if (planes) { planes[4 * i] = 0.0; planes[4 * i + 1] = 0.0; planes[4 * i + 2] = 0.0; planes[4 * i + 3] = 0.0; }
        if (centres) { centres[3 * i] = 0.0; centres[3 * i + 1] = 0.0; centres[3 * i + 2] = 0.0; }
        if (counts) counts[i] = 0;
        if (rmse) rmse[i] = 0.0;
        if (best_trial) best_trial[i] = 0;
        if (best_cost) best_cost[i] = 0;
        if (best_count) best_count[i] = 0;
    }
    if (tid == 0 && n_planes) *n_planes = 0;
}

__global__ __launch_bounds__(kPlBlock) void pl_init_kernel(const float* __restrict__ m, int M, int ldm, PlState* __restrict__ st,
                                                           uint8_t* __restrict__ alive, int32_t* __restrict__ labels) {
    __shared__ unsigned s[kPlBlock / 64][6];
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (int j = 0; j < kPlChunk / kPlBlock; ++j) {               // 2048 rows a workgroup: six atomics per 2048 rows
        const long long i = (long long)blockIdx.x * kPlChunk + (long long)j * kPlBlock + threadIdx.x;
        if (i < M) {
            const float x = m[i], y = m[i + (size_t)ldm], z = m[i + 2 * (size_t)ldm];
            const bool fin = finite3(x, y, z);
            alive[i] = fin ? 1 : 0;
            labels[i] = 0;
            if (fin) {
                const unsigned ox = ord_of(x), oy = ord_of(y), oz = ord_of(z);
                lo[0] = min(lo[0], ox); lo[1] = min(lo[1], oy); lo[2] = min(lo[2], oz);
                hi[0] = max(hi[0], ox); hi[1] = max(hi[1], oy); hi[2] = max(hi[2], oz);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = min(lo[c], (unsigned)__shfl_xor((int)lo[c], o));
            hi[c] = max(hi[c], (unsigned)__shfl_xor((int)hi[c], o));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s[threadIdx.x >> 6][c] = lo[c]; s[threadIdx.x >> 6][3 + c] = hi[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        unsigned v = s[0][c];
        for (int w = 1; w < kPlBlock / 64; ++w) v = c < 3 ? min(v, s[w][c]) : max(v, s[w][c]);
        if (c < 3) { if (v != 0xFFFFFFFFu) atomicMin(&st->box[c], v); }
        else if (v != 0u) atomicMax(&st->box[c], v);
    }
}

// ---- A1, A2. the alive list (chunk_scan.hpp's predicate compaction over the original rows) ------------------------------------------
__global__ __launch_bounds__(kScanBlock) void pl_count_kernel(const PlState* __restrict__ st, const uint8_t* __restrict__ alive, int M,
                                                              int32_t* __restrict__ pin) {
    if (st->done) return;
    chunk_pred_count(M, pin, [&](long long i) { return alive[i] != 0; });
}
__global__ __launch_bounds__(kScanBlock) void pl_list_kernel(PlState* __restrict__ st, const uint8_t* __restrict__ alive,
                                                             const float* __restrict__ m, int M, int ldm, const int32_t* __restrict__ pin,
                                                             int32_t* __restrict__ A, float* __restrict__ cx, float* __restrict__ cy,
                                                             float* __restrict__ cz) {
    if (st->done) return;
    const int32_t at = chunk_pred_emit(M, pin, [&](long long i) { return alive[i] != 0; }, [&](int32_t at, long long i) {
        A[at] = (int32_t)i;
        cx[at] = m[i]; cy[at] = m[i + (size_t)ldm]; cz[at] = m[i + 2 * (size_t)ldm];
    });
    if (chunk_is_last_thread()) st->nA = at;
}

// ---- H. the hypotheses ---------------------------------------------------------------------------------------------------------------
// hp0 / hnf are [3][B] floats, hvoid [B] bytes.  The cross product and the normalisation are in double, written so that no
// contraction can change them (the build has -ffp-contract=off as well)
__global__ __launch_bounds__(kPlBlock) void pl_hyp_kernel(const PlState* __restrict__ st, int p, int B, unsigned long long seed,
                                                          const int32_t* __restrict__ samples, int idx_base,
                                                          const uint8_t* __restrict__ alive, const int32_t* __restrict__ A,
                                                          const float* __restrict__ m, int M, int ldm, int use_ref, double rx, double ry,
                                                          double rz, double rlen, double cos_max, float* __restrict__ hp0,
                                                          float* __restrict__ hnf, uint8_t* __restrict__ hvoid,
                                                          unsigned long long* __restrict__ cost, int32_t* __restrict__ count) {
    if (st->done) return;
    const int b = blockIdx.x * kPlBlock + threadIdx.x;
    if (b >= B) return;
    const int nA = st->nA;
    long long idx[3] = {0, 0, 0};
    bool ok = true;
    if (samples) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            idx[j] = (long long)samples[((size_t)p * (size_t)B + (size_t)b) * 3 + j] - (long long)idx_base;
            if (idx[j] < 0 || idx[j] >= M) ok = false;
            else if (!alive[idx[j]]) ok = false;
        }
    } else if (nA > 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const unsigned long long h =
                pl_splitmix64(seed ^ pl_splitmix64(((unsigned long long)p * (unsigned long long)B + (unsigned long long)b) * 4ull + j));
            idx[j] = A[h % (unsigned long long)nA];
        }
    } else ok = false;
    if (ok && (idx[0] == idx[1] || idx[0] == idx[2] || idx[1] == idx[2])) ok = false;
    float p0[3] = {0.0f, 0.0f, 0.0f};
    double n[3] = {0.0, 0.0, 0.0};
    if (ok) {
        double q[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
#pragma unroll
            for (int c = 0; c < 3; ++c) q[j][c] = (double)m[idx[j] + (size_t)c * (size_t)ldm];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) p0[c] = (float)q[0][c];
        const double ax = q[1][0] - q[0][0], ay = q[1][1] - q[0][1], az = q[1][2] - q[0][2];
        const double bx = q[2][0] - q[0][0], by = q[2][1] - q[0][1], bz = q[2][2] - q[0][2];
        const double c0 = __dsub_rn(__dmul_rn(ay, bz), __dmul_rn(az, by));
        const double c1 = __dsub_rn(__dmul_rn(az, bx), __dmul_rn(ax, bz));
        const double c2 = __dsub_rn(__dmul_rn(ax, by), __dmul_rn(ay, bx));
        const double L2 = __dadd_rn(__dadd_rn(__dmul_rn(c0, c0), __dmul_rn(c1, c1)), __dmul_rn(c2, c2));
        if (!(L2 > 0.0) || !(L2 < (double)INFINITY)) ok = false;
        else {
            const double len = sqrt(L2);
            n[0] = c0 / len; n[1] = c1 / len; n[2] = c2 / len;
            if (use_ref) {
                double dot = pl_dot_ref(n, rx, ry, rz);
                if (dot < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; dot = -dot; }
                if (dot / rlen < cos_max) ok = false;
            } else if (pl_negate_largest(n)) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { hp0[(size_t)c * B + b] = p0[c]; hnf[(size_t)c * B + b] = (float)n[c]; }
    hvoid[b] = ok ? 0 : 1;
    cost[b] = 0ull;
    count[b] = 0;
}

// ---- S. the scoring: B x nA evaluations ------------------------------------------------------------------------------------------------
// blockIdx.x = chunk of kPlChunk alive rows, blockIdx.y = 256 trials.  The rows sit in LDS as three arrays; a lane reads four rows of
// an array with one 16-byte load whose address is the same in every lane.  Rows past nA are staged as NaN: they pass no test.  Per
// chunk the inliers' q add up to at most 2048 2^20 = 2^31, inside an unsigned word; the others' 2^20 are added by their number.
__global__ __launch_bounds__(kPlBlock) void pl_score_kernel(const PlState* __restrict__ st, const float* __restrict__ cx,
                                                            const float* __restrict__ cy, const float* __restrict__ cz,
                                                            const float* __restrict__ hp0, const float* __restrict__ hnf, int B, float t2,
                                                            float s, unsigned long long* __restrict__ cost, int32_t* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) float sx[kPlChunk];
    __shared__ __attribute__((aligned(16))) float sy[kPlChunk];
    __shared__ __attribute__((aligned(16))) float sz[kPlChunk];
    if (st->done) return;
    const int nA = st->nA;
    const long long r0 = (long long)blockIdx.x * kPlChunk;
    if (r0 >= nA) return;
    const int nrow = (int)min((long long)kPlChunk, (long long)nA - r0);
    const int tid = threadIdx.x;
    const float qnan = __uint_as_float(0x7FC00000u);
    for (int i = tid; i < kPlChunk; i += kPlBlock) {
        const bool in = i < nrow;
        sx[i] = in ? cx[r0 + i] : qnan; sy[i] = in ? cy[r0 + i] : qnan; sz[i] = in ? cz[r0 + i] : qnan;
    }
    __syncthreads();
    const int b = blockIdx.y * kPlBlock + tid;
    const int bb = min(b, B - 1);
    const float ox = hp0[bb], oy = hp0[(size_t)B + bb], oz = hp0[2 * (size_t)B + bb];
    const float nx = hnf[bb], ny = hnf[(size_t)B + bb], nz = hnf[2 * (size_t)B + bb];
    unsigned qs = 0u;
    int cnt = 0;
    const int n4 = (nrow + 3) & ~3;
    for (int i = 0; i < n4; i += 4) {
        const float4 X = *(const float4*)&sx[i], Y = *(const float4*)&sy[i], Z = *(const float4*)&sz[i];
        const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float r2 = pl_r2(xs[u], ys[u], zs[u], ox, oy, oz, nx, ny, nz);
            const bool in = r2 <= t2;
            qs += in ? (unsigned)pl_q(r2, s) : 0u;
            cnt += in ? 1 : 0;
        }
    }
    if (b < B) {
        atomicAdd(&cost[b], (unsigned long long)qs + ((unsigned long long)(nrow - cnt) << 20));
        atomicAdd(&count[b], cnt);
    }
}

// ---- B. the best trial ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlBlock) void pl_select_kernel(PlState* __restrict__ st, int p, int B, int min_inliers,
                                                             const uint8_t* __restrict__ hvoid, const unsigned long long* __restrict__ cost,
                                                             const int32_t* __restrict__ count, const float* __restrict__ hp0,
                                                             const float* __restrict__ hnf, int32_t* __restrict__ best_trial,
                                                             long long* __restrict__ best_cost, int32_t* __restrict__ best_count) {
    __shared__ unsigned long long sc[kPlBlock];
    __shared__ int sb[kPlBlock];
    if (st->done) return;
    const int tid = threadIdx.x;
    unsigned long long c = ~0ull;
    int bi = -1;
    for (int b = tid; b < B; b += kPlBlock) {              // ascending b per thread: the first of equal costs stays
        if (!hvoid[b] && count[b] >= 3 && cost[b] < c) { c = cost[b]; bi = b; }
    }
    sc[tid] = c; sb[tid] = bi;
    __syncthreads();
    for (int o = kPlBlock / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const unsigned long long c2 = sc[tid + o];
            const int b2 = sb[tid + o];
            if (b2 >= 0 && (sb[tid] < 0 || c2 < sc[tid] || (c2 == sc[tid] && b2 < sb[tid]))) { sc[tid] = c2; sb[tid] = b2; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int b = sb[0];
        const int n = b >= 0 ? count[b] : 0;
        const long long cb = b >= 0 ? (long long)sc[0] : 0ll;
        if (best_trial) best_trial[p] = b;
        if (best_cost) best_cost[p] = cb;
        if (best_count) best_count[p] = n;
        st->best_b = b; st->best_count = n; st->best_cost = cb;
        if (b < 0 || n < min_inliers) st->done = 1;
        else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { st->p0[k] = hp0[(size_t)k * B + b]; st->nf[k] = hnf[(size_t)k * B + b]; }
        }
    }
}

// ---- R, E. the refit -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlBlock) void pl_refit_kernel(PlState* __restrict__ st, int p, const float* __restrict__ cx,
                                                            const float* __restrict__ cy, const float* __restrict__ cz, float t2) {
    if (st->done) return;
    const int nA = st->nA;
    const long long k0 = (long long)blockIdx.x * kPlChunk;
    if (k0 >= nA) return;
    const float ox = st->p0[0], oy = st->p0[1], oz = st->p0[2], nx = st->nf[0], ny = st->nf[1], nz = st->nf[2];
    const double scale = ldexp(1.0, 17 - pl_exponent(st));
    long long a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < kPlChunk / kPlBlock; ++j) {
        const long long k = k0 + (long long)j * kPlBlock + threadIdx.x;
        if (k < nA) {
            const float x = cx[k], y = cy[k], z = cz[k];
            if (pl_r2(x, y, z, ox, oy, oz, nx, ny, nz) <= t2) {
                const long long gx = (long long)rint((double)(x - ox) * scale);
                const long long gy = (long long)rint((double)(y - oy) * scale);
                const long long gz = (long long)rint((double)(z - oz) * scale);
                a[0] += 1; a[1] += gx; a[2] += gy; a[3] += gz;
                a[4] += gx * gx; a[5] += gx * gy; a[6] += gx * gz; a[7] += gy * gy; a[8] += gy * gz; a[9] += gz * gz;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 10; ++c) a[c] += __shfl_xor(a[c], o);
    }
    __shared__ long long sw[kPlBlock / 64][10];                   // the four waves through LDS: ten atomics a workgroup
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 10; ++c) sw[threadIdx.x >> 6][c] = a[c];
    }
    __syncthreads();
    if (threadIdx.x < 10 && sw[0][0] + sw[1][0] + sw[2][0] + sw[3][0] != 0) {
        const int c = threadIdx.x;
        atomicAdd((unsigned long long*)&st->sums[p][c], (unsigned long long)(sw[0][c] + sw[1][c] + sw[2][c] + sw[3][c]));
    }
}

__global__ void pl_plane_kernel(PlState* __restrict__ st, int p, int use_ref, double rx, double ry, double rz,
                                double* __restrict__ planes, double* __restrict__ centres) {
    if (st->done) return;
    const long long* S = st->sums[p];
    const __int128 n = S[0];
    double a[6], V[9];
    a[0] = pl_i128_to_double(n * S[4] - (__int128)S[1] * S[1]);
    a[1] = pl_i128_to_double(n * S[5] - (__int128)S[1] * S[2]);
    a[2] = pl_i128_to_double(n * S[6] - (__int128)S[1] * S[3]);
    a[3] = pl_i128_to_double(n * S[7] - (__int128)S[2] * S[2]);
    a[4] = pl_i128_to_double(n * S[8] - (__int128)S[2] * S[3]);
    a[5] = pl_i128_to_double(n * S[9] - (__int128)S[3] * S[3]);
    jacobi_sym3(a, V);
    int c = 0;                                                    // the smallest eigenvalue, the first of equal ones
    if (a[3] < a[0]) c = 1;
    if (a[5] < (c == 1 ? a[3] : a[0])) c = 2;
    double nv[3] = {V[c], V[3 + c], V[6 + c]};
    const bool neg = use_ref ? pl_dot_ref(nv, rx, ry, rz) < 0.0 : pl_negate_largest(nv);
    if (neg) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
    const double back = ldexp(1.0, -(17 - pl_exponent(st)));
    const double nd = (double)S[0];
    double ctr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ctr[k] = (double)st->p0[k] + ((double)S[1 + k] / nd) * back;
    const double d4 = -((nv[0] * ctr[0] + nv[1] * ctr[1]) + nv[2] * ctr[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        planes[4 * p + k] = nv[k]; centres[3 * p + k] = ctr[k];
        st->nn[k] = (float)nv[k]; st->cf[k] = (float)ctr[k];
    }
    planes[4 * p + 3] = d4;
}

// ---- C, F. the classification ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlBlock) void pl_classify_kernel(PlState* __restrict__ st, int p, const int32_t* __restrict__ A,
                                                               const float* __restrict__ cx, const float* __restrict__ cy,
                                                               const float* __restrict__ cz, float t2, float s,
                                                               uint8_t* __restrict__ alive, int32_t* __restrict__ labels) {
    if (st->done) return;
    const int nA = st->nA;
    const long long k0 = (long long)blockIdx.x * kPlChunk;
    if (k0 >= nA) return;
    const float ox = st->cf[0], oy = st->cf[1], oz = st->cf[2], nx = st->nn[0], ny = st->nn[1], nz = st->nn[2];
    unsigned long long q = 0ull;
    int cnt = 0;
    for (int j = 0; j < kPlChunk / kPlBlock; ++j) {
        const long long k = k0 + (long long)j * kPlBlock + threadIdx.x;
        if (k < nA) {
            const float r2 = pl_r2(cx[k], cy[k], cz[k], ox, oy, oz, nx, ny, nz);
            if (r2 <= t2) {
                const int row = A[k];
                labels[row] = p + 1;
                alive[row] = 0;
                q += (unsigned long long)pl_q(r2, s);
                ++cnt;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { q += __shfl_xor(q, o); cnt += __shfl_xor(cnt, o); }
    __shared__ unsigned long long sw[kPlBlock / 64][2];
    if ((threadIdx.x & 63) == 0) { sw[threadIdx.x >> 6][0] = (unsigned long long)cnt; sw[threadIdx.x >> 6][1] = q; }
    __syncthreads();
    if (threadIdx.x < 2 && sw[0][0] + sw[1][0] + sw[2][0] + sw[3][0] != 0ull) {
        const int c = threadIdx.x;
        atomicAdd(&st->tot[p][c], sw[0][c] + sw[1][c] + sw[2][c] + sw[3][c]);
    }
}

__global__ void pl_finish_kernel(const PlState* __restrict__ st, int p, float t2, int32_t* __restrict__ counts, double* __restrict__ rmse,
                                 int32_t* __restrict__ n_planes) {
    if (st->done) return;
    const unsigned long long n = st->tot[p][0], Q = st->tot[p][1];
    counts[p] = (int32_t)n;
    rmse[p] = sqrt(((double)Q / (double)n) * ((double)t2 * 9.5367431640625e-07));      // 2^-20
    *n_planes = p + 1;
}

// Workspace, with R = max(M, 1), C = max(ceil(M / 2048), 1) and T = B: [state, roundup(sizeof, 256)][alive bytes, R][chunk counts,
// C int32][alive rows, R int32][their x, y, z, R floats each][p0 and nf, 3 T floats each][void bytes, T][cost, T uint64][count, T
// int32], every slot rounded up to 256 bytes
struct PlanesWs {
    PlState* st; uint8_t* alive; int32_t* pin; int32_t* A; float *cx, *cy, *cz; float *hp0, *hnf; uint8_t* hvoid;
    unsigned long long* cost; int32_t* count; int n_chunks;
};
PlanesWs planes_ws_layout(int M, int B, void* base, size_t* bytes) {
    PlanesWs s{};
    WsWalk w(base);
    const size_t R = (size_t)(M > 0 ? M : 1), T = (size_t)(B > 0 ? B : 1);
    s.n_chunks = (int)((R + kScanChunk - 1) / kScanChunk);
    s.st = w.take<PlState>(1);
    s.alive = w.take<uint8_t>(R);
    s.pin = w.take<int32_t>((size_t)s.n_chunks);
    s.A = w.take<int32_t>(R);
    s.cx = w.take<float>(R); s.cy = w.take<float>(R); s.cz = w.take<float>(R);
    s.hp0 = w.take<float>(3 * T); s.hnf = w.take<float>(3 * T);
    s.hvoid = w.take<uint8_t>(T);
    s.cost = w.take<unsigned long long>(T);
    s.count = w.take<int32_t>(T);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t planes_ws_bytes(int M, int B) {
    size_t b; (void)planes_ws_layout(M, B, nullptr, &b);
    return b;
}

bool planes_args_ok(float max_distance, const double* ref_vec, double max_angle, int max_planes, int n_trials, int min_inliers) {
    if (!(std::isnormal(max_distance) && max_distance > 0.0f)) return false;
    const float t2 = max_distance * max_distance;
    if (!(std::isnormal(t2))) return false;                      // (the square is the threshold: it must be a normal float too)
    if (max_planes < 1 || max_planes > kPlMaxPlanes || n_trials < 1 || n_trials > kPlMaxTrials || min_inliers < 3) return false;
    if (ref_vec) {
        for (int c = 0; c < 3; ++c) if (!std::isfinite(ref_vec[c])) return false;
        const double l2 = (ref_vec[0] * ref_vec[0] + ref_vec[1] * ref_vec[1]) + ref_vec[2] * ref_vec[2];
        if (!(l2 > 0.0) || !std::isfinite(l2)) return false;
        if (!(max_angle > 0.0 && max_angle <= 1.5707963267948966)) return false;
    }
    return true;
}
int planes_max_rows() { return kPlMaxM; }

int launch_model_fit_planes(const ModelView& v, float max_distance, const double* ref_vec, double max_angle, int max_planes, int n_trials,
                            int min_inliers, unsigned long long seed, const int32_t* samples, int32_t idx_base, int32_t* labels,
                            double* planes, double* centres, int32_t* counts, double* rmse, int32_t* n_planes, int32_t* best_trial,
                            int64_t* best_cost, int32_t* best_count, void* ws, size_t ws_bytes, hipStream_t stream) {
    PCREG_ARG(planes_args_ok(max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers) && n_planes);
    PCREG_ARG(v.M < kPlMaxM && ((labels && planes && centres && counts && rmse) || v.M == 0));
    size_t need;
    const PlanesWs s = planes_ws_layout(v.M, n_trials, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: fit_planes workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M, B = n_trials, P = max_planes;
    hipLaunchKernelGGL(pl_reset_kernel, dim3(1), dim3(kPlBlock), 0, stream, s.st, P, planes, centres, counts, rmse, n_planes, best_trial,
                       (long long*)best_cost, best_count);
    if (M == 0) { PCREG_HIP(hipGetLastError()); return PCREG_OK; }
    const float t2 = max_distance * max_distance;
    const float sc = (float)(1048576.0 / (double)t2);
    const int use_ref = ref_vec ? 1 : 0;
    const double rx = use_ref ? ref_vec[0] : 0.0, ry = use_ref ? ref_vec[1] : 0.0, rz = use_ref ? ref_vec[2] : 0.0;
    const double rlen = use_ref ? std::sqrt((rx * rx + ry * ry) + rz * rz) : 1.0;
    const double cos_max = use_ref ? std::cos(max_angle) : 0.0;
    hipLaunchKernelGGL(pl_init_kernel, dim3((unsigned)s.n_chunks), dim3(kPlBlock), 0, stream, v.m, M, v.ldm, s.st, s.alive, labels);
    const dim3 cgrid((unsigned)s.n_chunks), cblock(kScanBlock), bgrid((unsigned)((B + kPlBlock - 1) / kPlBlock));
    const dim3 sgrid((unsigned)s.n_chunks, (unsigned)((B + kPlBlock - 1) / kPlBlock));
    for (int p = 0; p < P; ++p) {
        hipLaunchKernelGGL(pl_count_kernel, cgrid, cblock, 0, stream, (const PlState*)s.st, (const uint8_t*)s.alive, M, s.pin);
        hipLaunchKernelGGL(pl_list_kernel, cgrid, cblock, 0, stream, s.st, (const uint8_t*)s.alive, v.m, M, v.ldm, (const int32_t*)s.pin, s.A, s.cx,
                           s.cy, s.cz);
        hipLaunchKernelGGL(pl_hyp_kernel, bgrid, dim3(kPlBlock), 0, stream, (const PlState*)s.st, p, B, seed, samples, (int)idx_base,
                           (const uint8_t*)s.alive, (const int32_t*)s.A, v.m, M, v.ldm, use_ref, rx, ry, rz, rlen, cos_max, s.hp0, s.hnf, s.hvoid,
                           s.cost, s.count);
        hipLaunchKernelGGL(pl_score_kernel, sgrid, dim3(kPlBlock), 0, stream, (const PlState*)s.st, (const float*)s.cx, (const float*)s.cy,
                           (const float*)s.cz, (const float*)s.hp0, (const float*)s.hnf, B, t2, sc, s.cost, s.count);
        hipLaunchKernelGGL(pl_select_kernel, dim3(1), dim3(kPlBlock), 0, stream, s.st, p, B, min_inliers, (const uint8_t*)s.hvoid,
                           (const unsigned long long*)s.cost, (const int32_t*)s.count, (const float*)s.hp0, (const float*)s.hnf, best_trial,
                           (long long*)best_cost, best_count);
        hipLaunchKernelGGL(pl_refit_kernel, cgrid, dim3(kPlBlock), 0, stream, s.st, p, (const float*)s.cx, (const float*)s.cy, (const float*)s.cz,
                           t2);
        hipLaunchKernelGGL(pl_plane_kernel, dim3(1), dim3(1), 0, stream, s.st, p, use_ref, rx, ry, rz, planes, centres);
        hipLaunchKernelGGL(pl_classify_kernel, cgrid, dim3(kPlBlock), 0, stream, s.st, p, (const int32_t*)s.A, (const float*)s.cx,
                           (const float*)s.cy, (const float*)s.cz, t2, sc, s.alive, labels);
        hipLaunchKernelGGL(pl_finish_kernel, dim3(1), dim3(1), 0, stream, (const PlState*)s.st, p, t2, counts, rmse, n_planes);
    }
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
