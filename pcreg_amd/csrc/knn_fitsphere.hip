// pcreg_amd/csrc/knn_fitsphere.hip -- MSAC sphere fitting and sphere extraction on a PREPARED model (MATLAB's pcfitsphere and the
// fit / remove / fit-again loop over it: the fiducial markers and ball tips of a scan): up to P spheres in one launch chain, nothing
// read on the host.  The contract is pcreg_model_fit_spheres_f32's (include/pcreg.h); DESIGN 4.22.  The shape is knn_planes.hip's
// (DESIGN 4.21); the geometry is new: the circumsphere of four rows, a radial residual with one correctly rounded fp32 root per
// (trial, row) pair, and an algebraic least-squares refit from seventeen exact integer sums (sphere_fit.hpp).
//
// The model's rows are read through v.m, by ORIGINAL row.  A call is two launches and then nine per round p:
//   Z   sf_reset_kernel      one workgroup: the state, the per-round sums and the P-sized outputs to zero
//   I   sf_init_kernel       labels = 0, the alive byte of every row (its three coordinates finite), the box of the finite rows by
//                            integer atomic min / max on order-preserving words
//   A1  sf_count_kernel      chunk_scan.hpp's first launch over the alive bytes
//   A2  sf_list_kernel       its second: the alive rows ascending, their coordinates packed behind them, their number nA
//   H   sf_hyp_kernel        one thread per trial: the four sample rows, the checks, the circumsphere in double, (p0, cf, Rf, void);
//                            the trial's cost and count to zero
//   S   sf_score_kernel      THE HOT PATH: lane = trial.  A workgroup stages 2048 alive rows in LDS and each of its 256 lanes walks
//                            them with its own sphere in registers (the LDS reads are wave-uniform: a broadcast, no bank conflict), so
//                            a (trial, row) pair costs no cross-lane step; one 64-bit and one 32-bit integer atomic per (chunk, trial)
//   B   sf_select_kernel     one workgroup: the smallest (cost, b) among the eligible trials; the stop rule; the diagnostics
//   R   sf_refit_kernel      the best trial's inliers: g = rint(d 2^(17 - e)), w = |g|^2 split at 2^18, the seventeen integer sums by
//                            wave and LDS reduction, seventeen atomics a workgroup
//   E   sf_solve_kernel      one thread: sum g w recombined, N and h in 128 bits, fit_spheres_solve, or the trial's own sphere
//   C   sf_classify_kernel   the final fp32 classification: labels, alive bytes, the round's count and Q by integer atomics
//   F   sf_finish_kernel     one thread: counts, rmse, n_spheres = p + 1
// Every sum across rows is an INTEGER sum: no order of summation, no floating-point atomic.  A device word says that extraction has
// ended; every later launch reads it and returns.  Nothing synchronises; no workgroup waits for another.
#include "common.hpp"
#include "knn_walk.hpp"                              // finite3
#include "chunk_scan.hpp"
#include "sphere_fit.hpp"
#include <cmath>

namespace pcreg {

namespace {

constexpr int kSfMaxM = 1 << 26;                     // below it no sum overflows: |g| <= 2^17, |g w_lo|, |g w_hi| < 2^35, 2^26 rows
constexpr int kSfMaxSpheres = 64;
constexpr int kSfMaxTrials = 1 << 20;
constexpr int kSfBlock = 256;
constexpr int kSfChunk = kScanChunk;                 // alive rows per scoring workgroup
constexpr int kSfQMax = 1 << 20;
constexpr int kSfSums = 17;                          // n, S1 x y z, S2 xx xy xz yy yz zz, sum w, sum g w_lo x y z, sum g w_hi x y z
constexpr int kSfSplit = 18;                         // w = w_hi 2^18 + w_lo

struct SfState {
    unsigned box[6];                                 // lo x y z, hi x y z of the finite rows as order-preserving words
    int done, nA;
    int best_b, best_count;
    long long best_cost;
    float p0[3];                                     // the best trial's first row (the refit's origin)
    float tc[3], tR;                                 // the best trial's sphere (the refit's inlier test)
    float cf[3], Rf;                                 // (float)centre and (float)R of the round's sphere (the classification)
    long long sums[kSfMaxSpheres][kSfSums];
    unsigned long long tot[kSfMaxSpheres][2];        // per round: count_p, Q_p
};

// ransac.hip's sampler hash
__device__ __forceinline__ unsigned long long sf_splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull; unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// a float as a word whose unsigned order is the float's, and back
__device__ __forceinline__ unsigned sf_ord_of(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sf_ord_back(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
// frexp's exponent of the largest axis extent of the finite rows (0 where there is none or it is zero)
__device__ __forceinline__ int sf_exponent(const SfState* __restrict__ st) {
    double D = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned lo = st->box[c], hi = st->box[3 + c];
        if (lo <= hi) D = fmax(D, (double)sf_ord_back(hi) - (double)sf_ord_back(lo));
    }
    int e = 0;
    if (D > 0.0) (void)frexp(D, &e);
    return e;
}
// a 128-bit integer rounded ONCE to double (knn_iss.hip's construction)
__device__ __forceinline__ double sf_i128_to_double(__int128 v) {
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
// the contract's scoring chain for one row against the sphere (centre c, radius R): r2, and its q.  The root is the correctly
// rounded fp32 one: the build keeps clang's default, under which sqrtf is exactly that (DESIGN 4.22 shows the instructions)
__device__ __forceinline__ float sf_r2(float x, float y, float z, float cx, float cy, float cz, float R) {
    const float dx = x - cx, dy = y - cy, dz = z - cz;
    const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    const float r = __builtin_sqrtf(d2) - R;
    return r * r;
}
__device__ __forceinline__ int sf_q(float r2, float s) {     // min(2^20, rint(r2 s)); rint is monotone, so the cap may come first
    return (int)rintf(fminf(r2 * s, (float)kSfQMax));
}
__device__ __forceinline__ bool sf_finite(double v) { return v - v == 0.0; }
__device__ __forceinline__ bool sf_finitef(float v) { return v - v == 0.0f; }

// ---- Z, I. reset and the alive rows ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSfBlock) void sf_reset_kernel(SfState* __restrict__ st, int P, double* __restrict__ spheres,
                                                            int32_t* __restrict__ counts, double* __restrict__ rmse,
                                                            int32_t* __restrict__ refit_used, int32_t* __restrict__ n_spheres,
                                                            int32_t* __restrict__ best_trial, long long* __restrict__ best_cost,
                                                            int32_t* __restrict__ best_count) {
    const int tid = threadIdx.x;
    unsigned* w = (unsigned*)st;
    for (int i = tid; i < (int)(sizeof(SfState) / 4); i += kSfBlock) w[i] = 0u;
    __syncthreads();
    if (tid < 3) { st->box[tid] = 0xFFFFFFFFu; st->box[3 + tid] = 0u; }
    for (int i = tid; i < P; i += kSfBlock) {
        if (spheres) { spheres[4 * i] = 0.0; spheres[4 * i + 1] = 0.0; spheres[4 * i + 2] = 0.0; spheres[4 * i + 3] = 0.0; }
        if (counts) counts[i] = 0;
        if (rmse) rmse[i] = 0.0;
        if (refit_used) refit_used[i] = 0;
        if (best_trial) best_trial[i] = 0;
        if (best_cost) best_cost[i] = 0;
        if (best_count) best_count[i] = 0;
    }
    if (tid == 0 && n_spheres) *n_spheres = 0;
}

__global__ __launch_bounds__(kSfBlock) void sf_init_kernel(const float* __restrict__ m, int M, int ldm, SfState* __restrict__ st,
                                                           uint8_t* __restrict__ alive, int32_t* __restrict__ labels) {
    __shared__ unsigned s[kSfBlock / 64][6];
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (int j = 0; j < kSfChunk / kSfBlock; ++j) {               // 2048 rows a workgroup: six atomics per 2048 rows
        const long long i = (long long)blockIdx.x * kSfChunk + (long long)j * kSfBlock + threadIdx.x;
        if (i < M) {
            const float x = m[i], y = m[i + (size_t)ldm], z = m[i + 2 * (size_t)ldm];
            const bool fin = finite3(x, y, z);
            alive[i] = fin ? 1 : 0;
            labels[i] = 0;
            if (fin) {
                const unsigned ox = sf_ord_of(x), oy = sf_ord_of(y), oz = sf_ord_of(z);
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
        for (int w = 1; w < kSfBlock / 64; ++w) v = c < 3 ? min(v, s[w][c]) : max(v, s[w][c]);
        if (c < 3) { if (v != 0xFFFFFFFFu) atomicMin(&st->box[c], v); }
        else if (v != 0u) atomicMax(&st->box[c], v);
    }
}

// ---- A1, A2. the alive list (chunk_scan.hpp's predicate compaction over the original rows) ------------------------------------------
__global__ __launch_bounds__(kScanBlock) void sf_count_kernel(const SfState* __restrict__ st, const uint8_t* __restrict__ alive, int M,
                                                              int32_t* __restrict__ pin) {
    if (st->done) return;
    chunk_pred_count(M, pin, [&](long long i) { return alive[i] != 0; });
}
__global__ __launch_bounds__(kScanBlock) void sf_list_kernel(SfState* __restrict__ st, const uint8_t* __restrict__ alive,
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
// hp0 is [3][B] floats, hsp [4][B] floats (cf x y z, Rf), hvoid [B] bytes.  The circumsphere is in double, every step one correctly
// rounded operation written so that no contraction can change it (the build has -ffp-contract=off as well)
__global__ __launch_bounds__(kSfBlock) void sf_hyp_kernel(const SfState* __restrict__ st, int p, int B, unsigned long long seed,
                                                          const int32_t* __restrict__ samples, int idx_base,
                                                          const uint8_t* __restrict__ alive, const int32_t* __restrict__ A,
                                                          const float* __restrict__ m, int M, int ldm, float min_radius, float max_radius,
                                                          float* __restrict__ hp0, float* __restrict__ hsp, uint8_t* __restrict__ hvoid,
                                                          unsigned long long* __restrict__ cost, int32_t* __restrict__ count) {
    if (st->done) return;
    const int b = blockIdx.x * kSfBlock + threadIdx.x;
    if (b >= B) return;
    const int nA = st->nA;
    long long idx[4] = {0, 0, 0, 0};
    bool ok = true;
    if (samples) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            idx[j] = (long long)samples[((size_t)p * (size_t)B + (size_t)b) * 4 + j] - (long long)idx_base;
            if (idx[j] < 0 || idx[j] >= M) ok = false;
            else if (!alive[idx[j]]) ok = false;
        }
    } else if (nA > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long h =
                sf_splitmix64(seed ^ sf_splitmix64(((unsigned long long)p * (unsigned long long)B + (unsigned long long)b) * 4ull + j));
            idx[j] = A[h % (unsigned long long)nA];
        }
    } else ok = false;
    if (ok && (idx[0] == idx[1] || idx[0] == idx[2] || idx[0] == idx[3] || idx[1] == idx[2] || idx[1] == idx[3] || idx[2] == idx[3]))
        ok = false;
    float p0[3] = {0.0f, 0.0f, 0.0f}, sp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) {
        double q[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int c = 0; c < 3; ++c) q[j][c] = (double)m[idx[j] + (size_t)c * (size_t)ldm];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) p0[c] = (float)q[0][c];
        double d[3][3], bb[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d[i][c] = __dsub_rn(q[i + 1][c], q[0][c]);
            bb[i] = __dadd_rn(__dadd_rn(__dmul_rn(d[i][0], d[i][0]), __dmul_rn(d[i][1], d[i][1])), __dmul_rn(d[i][2], d[i][2]));
        }
        double X[3][3];                                           // X1 = d2 x d3, X2 = d3 x d1, X3 = d1 x d2
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double* a = d[(i + 1) % 3];
            const double* c = d[(i + 2) % 3];
            X[i][0] = __dsub_rn(__dmul_rn(a[1], c[2]), __dmul_rn(a[2], c[1]));
            X[i][1] = __dsub_rn(__dmul_rn(a[2], c[0]), __dmul_rn(a[0], c[2]));
            X[i][2] = __dsub_rn(__dmul_rn(a[0], c[1]), __dmul_rn(a[1], c[0]));
        }
        const double det = __dadd_rn(__dadd_rn(__dmul_rn(d[0][0], X[0][0]), __dmul_rn(d[0][1], X[0][1])), __dmul_rn(d[0][2], X[0][2]));
        if (det == 0.0 || !sf_finite(det)) ok = false;
        else {
            const double den = __dmul_rn(2.0, det);
            double u[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double num = __dadd_rn(__dadd_rn(__dmul_rn(bb[0], X[0][c]), __dmul_rn(bb[1], X[1][c])), __dmul_rn(bb[2], X[2][c]));
                u[c] = __ddiv_rn(num, den);
            }
            const double R2 = __dadd_rn(__dadd_rn(__dmul_rn(u[0], u[0]), __dmul_rn(u[1], u[1])), __dmul_rn(u[2], u[2]));
            const double R = __dsqrt_rn(R2);
            if (!sf_finite(u[0]) || !sf_finite(u[1]) || !sf_finite(u[2]) || !sf_finite(R)) ok = false;
            else {
#pragma unroll
                for (int c = 0; c < 3; ++c) sp[c] = (float)__dadd_rn(q[0][c], u[c]);
                sp[3] = (float)R;
                if (!sf_finitef(sp[0]) || !sf_finitef(sp[1]) || !sf_finitef(sp[2]) || !sf_finitef(sp[3])) ok = false;
                else if (sp[3] < min_radius || sp[3] > max_radius) ok = false;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) hp0[(size_t)c * B + b] = p0[c];
#pragma unroll
    for (int c = 0; c < 4; ++c) hsp[(size_t)c * B + b] = ok ? sp[c] : 0.0f;
    hvoid[b] = ok ? 0 : 1;
    cost[b] = 0ull;
    count[b] = 0;
}

// ---- S. the scoring: B x nA evaluations ------------------------------------------------------------------------------------------------
// blockIdx.x = chunk of kSfChunk alive rows, blockIdx.y = 256 trials.  The rows sit in LDS as three arrays; a lane reads four rows of
// an array with one 16-byte load whose address is the same in every lane.  Rows past nA are staged as NaN: they pass no test.  Per
// chunk the inliers' q add up to at most 2048 2^20 = 2^31, inside an unsigned word; the others' 2^20 are added by their number.
__global__ __launch_bounds__(kSfBlock) void sf_score_kernel(const SfState* __restrict__ st, const float* __restrict__ cx,
                                                            const float* __restrict__ cy, const float* __restrict__ cz,
                                                            const float* __restrict__ hsp, int B, float t2, float s,
                                                            unsigned long long* __restrict__ cost, int32_t* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) float sx[kSfChunk];
    __shared__ __attribute__((aligned(16))) float sy[kSfChunk];
    __shared__ __attribute__((aligned(16))) float sz[kSfChunk];
    if (st->done) return;
    const int nA = st->nA;
    const long long r0 = (long long)blockIdx.x * kSfChunk;
    if (r0 >= nA) return;
    const int nrow = (int)min((long long)kSfChunk, (long long)nA - r0);
    const int tid = threadIdx.x;
    const float qnan = __uint_as_float(0x7FC00000u);
    for (int i = tid; i < kSfChunk; i += kSfBlock) {
        const bool in = i < nrow;
        sx[i] = in ? cx[r0 + i] : qnan; sy[i] = in ? cy[r0 + i] : qnan; sz[i] = in ? cz[r0 + i] : qnan;
    }
    __syncthreads();
    const int b = blockIdx.y * kSfBlock + tid;
    const int bb = min(b, B - 1);
    const float ox = hsp[bb], oy = hsp[(size_t)B + bb], oz = hsp[2 * (size_t)B + bb], R = hsp[3 * (size_t)B + bb];
    unsigned qs = 0u;
    int cnt = 0;
    const int n4 = (nrow + 3) & ~3;
    for (int i = 0; i < n4; i += 4) {
        const float4 X = *(const float4*)&sx[i], Y = *(const float4*)&sy[i], Z = *(const float4*)&sz[i];
        const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float r2 = sf_r2(xs[u], ys[u], zs[u], ox, oy, oz, R);
            const bool in = r2 <= t2;
            qs += in ? (unsigned)sf_q(r2, s) : 0u;
            cnt += in ? 1 : 0;
        }
    }
    if (b < B) {
        atomicAdd(&cost[b], (unsigned long long)qs + ((unsigned long long)(nrow - cnt) << 20));
        atomicAdd(&count[b], cnt);
    }
}

// ---- B. the best trial ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSfBlock) void sf_select_kernel(SfState* __restrict__ st, int p, int B, int min_inliers,
                                                             const uint8_t* __restrict__ hvoid, const unsigned long long* __restrict__ cost,
                                                             const int32_t* __restrict__ count, const float* __restrict__ hp0,
                                                             const float* __restrict__ hsp, int32_t* __restrict__ best_trial,
                                                             long long* __restrict__ best_cost, int32_t* __restrict__ best_count) {
    __shared__ unsigned long long sc[kSfBlock];
    __shared__ int sb[kSfBlock];
    if (st->done) return;
    const int tid = threadIdx.x;
    unsigned long long c = ~0ull;
    int bi = -1;
    for (int b = tid; b < B; b += kSfBlock) {              // ascending b per thread: the first of equal costs stays
        if (!hvoid[b] && count[b] >= 4 && cost[b] < c) { c = cost[b]; bi = b; }
    }
    sc[tid] = c; sb[tid] = bi;
    __syncthreads();
    for (int o = kSfBlock / 2; o > 0; o >>= 1) {
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
            for (int k = 0; k < 3; ++k) { st->p0[k] = hp0[(size_t)k * B + b]; st->tc[k] = hsp[(size_t)k * B + b]; }
            st->tR = hsp[3 * (size_t)B + b];
        }
    }
}

// ---- R, E. the refit -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSfBlock) void sf_refit_kernel(SfState* __restrict__ st, int p, const float* __restrict__ cx,
                                                            const float* __restrict__ cy, const float* __restrict__ cz, float t2) {
    if (st->done) return;
    const int nA = st->nA;
    const long long k0 = (long long)blockIdx.x * kSfChunk;
    if (k0 >= nA) return;
    const float ox = st->p0[0], oy = st->p0[1], oz = st->p0[2];
    const float sx = st->tc[0], sy = st->tc[1], sz = st->tc[2], sR = st->tR;
    const double scale = ldexp(1.0, 17 - sf_exponent(st));
    long long a[kSfSums];
#pragma unroll
    for (int c = 0; c < kSfSums; ++c) a[c] = 0;
    for (int j = 0; j < kSfChunk / kSfBlock; ++j) {
        const long long k = k0 + (long long)j * kSfBlock + threadIdx.x;
        if (k < nA) {
            const float x = cx[k], y = cy[k], z = cz[k];
            if (sf_r2(x, y, z, sx, sy, sz, sR) <= t2) {
                const long long gx = (long long)rint((double)(x - ox) * scale);
                const long long gy = (long long)rint((double)(y - oy) * scale);
                const long long gz = (long long)rint((double)(z - oz) * scale);
                const long long w = gx * gx + gy * gy + gz * gz;
                const long long wl = w & ((1ll << kSfSplit) - 1), wh = w >> kSfSplit;
                a[0] += 1; a[1] += gx; a[2] += gy; a[3] += gz;
                a[4] += gx * gx; a[5] += gx * gy; a[6] += gx * gz; a[7] += gy * gy; a[8] += gy * gz; a[9] += gz * gz;
                a[10] += w;
                a[11] += gx * wl; a[12] += gy * wl; a[13] += gz * wl;
                a[14] += gx * wh; a[15] += gy * wh; a[16] += gz * wh;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < kSfSums; ++c) a[c] += __shfl_xor(a[c], o);
    }
    __shared__ long long sw[kSfBlock / 64][kSfSums];              // the four waves through LDS: seventeen atomics a workgroup
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < kSfSums; ++c) sw[threadIdx.x >> 6][c] = a[c];
    }
    __syncthreads();
    if (threadIdx.x < kSfSums && sw[0][0] + sw[1][0] + sw[2][0] + sw[3][0] != 0) {
        const int c = threadIdx.x;
        atomicAdd((unsigned long long*)&st->sums[p][c], (unsigned long long)(sw[0][c] + sw[1][c] + sw[2][c] + sw[3][c]));
    }
}

__global__ void sf_solve_kernel(SfState* __restrict__ st, int p, float min_radius, float max_radius, double* __restrict__ spheres,
                                int32_t* __restrict__ refit_used) {
    if (st->done) return;
    const long long* S = st->sums[p];
    const __int128 n = S[0];
    double N6[6], h[3], S1[3];
    N6[0] = sf_i128_to_double(n * S[4] - (__int128)S[1] * S[1]);
    N6[1] = sf_i128_to_double(n * S[5] - (__int128)S[1] * S[2]);
    N6[2] = sf_i128_to_double(n * S[6] - (__int128)S[1] * S[3]);
    N6[3] = sf_i128_to_double(n * S[7] - (__int128)S[2] * S[2]);
    N6[4] = sf_i128_to_double(n * S[8] - (__int128)S[2] * S[3]);
    N6[5] = sf_i128_to_double(n * S[9] - (__int128)S[3] * S[3]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const __int128 gw = (__int128)S[14 + k] * ((__int128)1 << kSfSplit) + (__int128)S[11 + k];     // sum g w, recombined
        h[k] = sf_i128_to_double(n * gw - (__int128)S[1 + k] * (__int128)S[10]);
        S1[k] = (double)S[1 + k];
    }
    const double p0[3] = {(double)st->p0[0], (double)st->p0[1], (double)st->p0[2]};
    const double back = ldexp(1.0, -(17 - sf_exponent(st)));
    double ctr[3] = {(double)st->tc[0], (double)st->tc[1], (double)st->tc[2]}, R = (double)st->tR;
    const bool used = fit_spheres_solve(N6, h, S1, (double)S[10], (double)S[0], p0, back, min_radius, max_radius, ctr, R);
#pragma unroll
    for (int k = 0; k < 3; ++k) { spheres[4 * p + k] = ctr[k]; st->cf[k] = (float)ctr[k]; }
    spheres[4 * p + 3] = R;
    st->Rf = (float)R;
    refit_used[p] = used ? 1 : 0;
}

// ---- C, F. the classification ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSfBlock) void sf_classify_kernel(SfState* __restrict__ st, int p, const int32_t* __restrict__ A,
                                                               const float* __restrict__ cx, const float* __restrict__ cy,
                                                               const float* __restrict__ cz, float t2, float s,
                                                               uint8_t* __restrict__ alive, int32_t* __restrict__ labels) {
    if (st->done) return;
    const int nA = st->nA;
    const long long k0 = (long long)blockIdx.x * kSfChunk;
    if (k0 >= nA) return;
    const float ox = st->cf[0], oy = st->cf[1], oz = st->cf[2], R = st->Rf;
    unsigned long long q = 0ull;
    int cnt = 0;
    for (int j = 0; j < kSfChunk / kSfBlock; ++j) {
        const long long k = k0 + (long long)j * kSfBlock + threadIdx.x;
        if (k < nA) {
            const float r2 = sf_r2(cx[k], cy[k], cz[k], ox, oy, oz, R);
            if (r2 <= t2) {
                const int row = A[k];
                labels[row] = p + 1;
                alive[row] = 0;
                q += (unsigned long long)sf_q(r2, s);
                ++cnt;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { q += __shfl_xor(q, o); cnt += __shfl_xor(cnt, o); }
    __shared__ unsigned long long sw[kSfBlock / 64][2];
    if ((threadIdx.x & 63) == 0) { sw[threadIdx.x >> 6][0] = (unsigned long long)cnt; sw[threadIdx.x >> 6][1] = q; }
    __syncthreads();
    if (threadIdx.x < 2 && sw[0][0] + sw[1][0] + sw[2][0] + sw[3][0] != 0ull) {
        const int c = threadIdx.x;
        atomicAdd(&st->tot[p][c], sw[0][c] + sw[1][c] + sw[2][c] + sw[3][c]);
    }
}

__global__ void sf_finish_kernel(const SfState* __restrict__ st, int p, float t2, int32_t* __restrict__ counts, double* __restrict__ rmse,
                                 int32_t* __restrict__ n_spheres) {
    if (st->done) return;
    const unsigned long long n = st->tot[p][0], Q = st->tot[p][1];
    counts[p] = (int32_t)n;
    rmse[p] = sqrt(((double)Q / (double)n) * ((double)t2 * 9.5367431640625e-07));      // 2^-20
    *n_spheres = p + 1;
}

// Workspace, with R = max(M, 1), C = max(ceil(M / 2048), 1) and T = B: [state, roundup(sizeof, 256)][alive bytes, R][chunk counts,
// C int32][alive rows, R int32][their x, y, z, R floats each][p0, 3 T floats][cf and Rf, 4 T floats][void bytes, T][cost, T uint64]
// [count, T int32], every slot rounded up to 256 bytes
struct FitSpheresWs {
    SfState* st; uint8_t* alive; int32_t* pin; int32_t* A; float *cx, *cy, *cz; float *hp0, *hsp; uint8_t* hvoid;
    unsigned long long* cost; int32_t* count; int n_chunks;
};
FitSpheresWs fit_spheres_ws_layout(int M, int B, void* base, size_t* bytes) {
    FitSpheresWs s{};
    WsWalk w(base);
    const size_t R = (size_t)(M > 0 ? M : 1), T = (size_t)(B > 0 ? B : 1);
    s.n_chunks = (int)((R + kScanChunk - 1) / kScanChunk);
    s.st = w.take<SfState>(1);
    s.alive = w.take<uint8_t>(R);
    s.pin = w.take<int32_t>((size_t)s.n_chunks);
    s.A = w.take<int32_t>(R);
    s.cx = w.take<float>(R); s.cy = w.take<float>(R); s.cz = w.take<float>(R);
    s.hp0 = w.take<float>(3 * T); s.hsp = w.take<float>(4 * T);
    s.hvoid = w.take<uint8_t>(T);
    s.cost = w.take<unsigned long long>(T);
    s.count = w.take<int32_t>(T);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t fit_spheres_ws_bytes(int M, int B) {
    size_t b; (void)fit_spheres_ws_layout(M, B, nullptr, &b);
    return b;
}

bool fit_spheres_args_ok(float max_distance, float min_radius, float max_radius, int max_spheres, int n_trials, int min_inliers) {
    if (!(std::isnormal(max_distance) && max_distance > 0.0f)) return false;
    const float t2 = max_distance * max_distance;
    if (!(std::isnormal(t2))) return false;                      // (the square is the threshold: it must be a normal float too)
    if (!(min_radius >= 0.0f && min_radius <= max_radius)) return false;      // (a NaN fails; max_radius may be +inf)
    return max_spheres >= 1 && max_spheres <= kSfMaxSpheres && n_trials >= 1 && n_trials <= kSfMaxTrials && min_inliers >= 4;
}
int fit_spheres_max_rows() { return kSfMaxM; }

int launch_model_fit_spheres(const ModelView& v, float max_distance, float min_radius, float max_radius, int max_spheres, int n_trials,
                             int min_inliers, unsigned long long seed, const int32_t* samples, int32_t idx_base, int32_t* labels,
                             double* spheres, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_spheres, int32_t* best_trial,
                             int64_t* best_cost, int32_t* best_count, void* ws, size_t ws_bytes, hipStream_t stream) {
    PCREG_ARG(fit_spheres_args_ok(max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers) && n_spheres);
    PCREG_ARG(v.M < kSfMaxM && ((labels && spheres && counts && rmse && refit_used) || v.M == 0));
    size_t need;
    const FitSpheresWs s = fit_spheres_ws_layout(v.M, n_trials, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: fit_spheres workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M, B = n_trials, P = max_spheres;
    hipLaunchKernelGGL(sf_reset_kernel, dim3(1), dim3(kSfBlock), 0, stream, s.st, P, spheres, counts, rmse, refit_used, n_spheres, best_trial,
                       (long long*)best_cost, best_count);
    if (M == 0) { PCREG_HIP(hipGetLastError()); return PCREG_OK; }
    const float t2 = max_distance * max_distance;
    const float sc = (float)(1048576.0 / (double)t2);
    hipLaunchKernelGGL(sf_init_kernel, dim3((unsigned)s.n_chunks), dim3(kSfBlock), 0, stream, v.m, M, v.ldm, s.st, s.alive, labels);
    const dim3 cgrid((unsigned)s.n_chunks), cblock(kScanBlock), bgrid((unsigned)((B + kSfBlock - 1) / kSfBlock));
    const dim3 sgrid((unsigned)s.n_chunks, (unsigned)((B + kSfBlock - 1) / kSfBlock));
    for (int p = 0; p < P; ++p) {
        hipLaunchKernelGGL(sf_count_kernel, cgrid, cblock, 0, stream, (const SfState*)s.st, (const uint8_t*)s.alive, M, s.pin);
        hipLaunchKernelGGL(sf_list_kernel, cgrid, cblock, 0, stream, s.st, (const uint8_t*)s.alive, v.m, M, v.ldm, (const int32_t*)s.pin, s.A, s.cx,
                           s.cy, s.cz);
        hipLaunchKernelGGL(sf_hyp_kernel, bgrid, dim3(kSfBlock), 0, stream, (const SfState*)s.st, p, B, seed, samples, (int)idx_base,
                           (const uint8_t*)s.alive, (const int32_t*)s.A, v.m, M, v.ldm, min_radius, max_radius, s.hp0, s.hsp, s.hvoid, s.cost,
                           s.count);
        hipLaunchKernelGGL(sf_score_kernel, sgrid, dim3(kSfBlock), 0, stream, (const SfState*)s.st, (const float*)s.cx, (const float*)s.cy,
                           (const float*)s.cz, (const float*)s.hsp, B, t2, sc, s.cost, s.count);
        hipLaunchKernelGGL(sf_select_kernel, dim3(1), dim3(kSfBlock), 0, stream, s.st, p, B, min_inliers, (const uint8_t*)s.hvoid,
                           (const unsigned long long*)s.cost, (const int32_t*)s.count, (const float*)s.hp0, (const float*)s.hsp, best_trial,
                           (long long*)best_cost, best_count);
        hipLaunchKernelGGL(sf_refit_kernel, cgrid, dim3(kSfBlock), 0, stream, s.st, p, (const float*)s.cx, (const float*)s.cy, (const float*)s.cz,
                           t2);
        hipLaunchKernelGGL(sf_solve_kernel, dim3(1), dim3(1), 0, stream, s.st, p, min_radius, max_radius, spheres, refit_used);
        hipLaunchKernelGGL(sf_classify_kernel, cgrid, dim3(kSfBlock), 0, stream, s.st, p, (const int32_t*)s.A, (const float*)s.cx,
                           (const float*)s.cy, (const float*)s.cz, t2, sc, s.alive, labels);
        hipLaunchKernelGGL(sf_finish_kernel, dim3(1), dim3(1), 0, stream, (const SfState*)s.st, p, t2, counts, rmse, n_spheres);
    }
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
