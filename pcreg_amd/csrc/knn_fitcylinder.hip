// pcreg_amd/csrc/knn_fitcylinder.hip -- MSAC cylinder fitting and cylinder extraction on a PREPARED model with normals (MATLAB's
// pcfitcylinder and the fit / remove / fit-again loop over it: the instrument shafts, sleeves, trocars and rods of a surgical
// scene): up to P cylinders in one launch chain, nothing read on the host.  The contract is pcreg_model_fit_cylinders_f32's
// (include/pcreg.h); DESIGN 4.23.  The shape is knn_fitsphere.hip's; the geometry is new: a trial is two rows and
// their normals (the axis along n_0 x n_1, through the point where the two normal lines pass closest), the residual is radial
// about a line (a cross product and one correctly rounded fp32 root per (trial, row) pair), and the refit takes two exact passes:
// the axis from seven integer sums of the inliers' normals, the circle from eleven integer sums in the axis' cross-section
// (cylinder_fit.hpp).
//
// The model's rows and the normals are read by ORIGINAL row.  A call is two launches and then eleven per round p:
//   Z   cy_reset_kernel      one workgroup: the state, the per-round sums and the P-sized outputs to zero
//   I   cy_init_kernel       labels = 0, the alive byte of every row (its three coordinates finite), the usable-normal byte, the box
//                            of the finite rows by integer atomic min / max on order-preserving words
//   A1  cy_count_kernel      chunk_scan.hpp's first launch over the alive bytes
//   A2  cy_list_kernel       its second: the alive rows ascending, their coordinates packed behind them, their number nA
//   H   cy_hyp_kernel        one thread per trial: the two sample rows and their normals, the checks, the cylinder in double,
//                            (p0, af, wf, Rf, void); the trial's cost and count to zero
//   S   cy_score_kernel      THE HOT PATH: lane = trial.  A workgroup stages 2048 alive rows in LDS and each of its 256 lanes walks
//                            them with its own cylinder (seven floats) in registers; the LDS reads are wave-uniform; one 64-bit and
//                            one 32-bit integer atomic per (chunk, trial).  No normal is staged: scoring reads none
//   B   cy_select_kernel     one workgroup: the smallest (cost, b) among the eligible trials; the stop rule; the diagnostics
//   X   cy_axis_kernel       the best trial's inliers with a usable normal: gn = rint(n 2^16), seven integer sums, seven atomics a
//                            workgroup
//   W   cy_basis_kernel      one thread: fit_cylinders_basis (Jacobi, w, u, v)
//   O   cy_circle_kernel     the best trial's inliers: g = rint(d 2^(17 - e)) projected on (u, v) and rounded, eleven integer sums
//   E   cy_solve_kernel      one thread: N and h in 128 bits, fit_cylinders_circle, or the trial's own cylinder
//   C   cy_classify_kernel   the final fp32 classification: labels, alive bytes, the round's count and Q by integer atomics, the
//                            extent along the axis by integer atomic min / max on order-preserving words
//   F   cy_finish_kernel     one thread: counts, rmse, extents, n_cylinders = p + 1
// Every sum across rows is an INTEGER sum and min / max do not depend on order: no floating-point atomic.  A device word says that
// extraction has ended; every later launch reads it and returns.  Nothing synchronises; no workgroup waits for another.
#include "common.hpp"
#include "knn_walk.hpp"                              // finite3
#include "chunk_scan.hpp"
#include "cylinder_fit.hpp"
#include <cmath>

namespace pcreg {

namespace {

constexpr int kCyMaxM = 1 << 26;                     // below it no sum overflows (the bounds stand at CyState)
constexpr int kCyMaxCylinders = 64;
constexpr int kCyMaxTrials = 1 << 20;
constexpr int kCyBlock = 256;
constexpr int kCyChunk = kScanChunk;                 // alive rows per scoring workgroup
constexpr int kCyQMax = 1 << 20;
constexpr int kCyAxisSums = 7;                       // n_n, sum gn_a gn_b: xx xy xz yy yz zz
constexpr int kCyCircSums = 11;                      // n, sum xi, yi, sum xi xi, xi yi, yi yi, sum w2, sum xi w_lo, xi w_hi, yi w_lo, yi w_hi
constexpr int kCySplit = 18;                         // w2 = w_hi 2^18 + w_lo

// The sums' bounds at M < 2^26 rows.  Axis: |gn| <= 2^17 (|n_c| <= 2), so |gn_a gn_b| <= 2^34 and every sum is below 2^60.
// Circle: |g_c| <= 2^17 gives |g| <= sqrt(3) 2^17 and, (u, v) being orthonormal to rounding, |xi|, |yi| < 2^18 and
// w2 = xi^2 + yi^2 < 2^36, so w_lo, w_hi < 2^18: n < 2^26; |sum xi|, |sum yi| < 2^44; the three sums of products < 2^62;
// sum w2 < 2^62; |sum xi w_lo| .. |sum yi w_hi| < 2^62.  All inside a signed 64-bit word.
struct CyState {
    unsigned box[6];                                 // lo x y z, hi x y z of the finite rows as order-preserving words
    int done, nA;
    int best_b, best_count;
    long long best_cost;
    float p0[3];                                     // the best trial's first row (the circle pass' origin)
    float ta[3], tw[3], tR;                          // the best trial's cylinder (the refit's inlier test)
    float cf[3], wf[3], Rf;                          // (float)centre, (float)w and (float)R of the round's cylinder (the classification)
    int basis_ok;
    double w[3], u[3], v[3];                         // the refit's axis and the basis of its cross-section
    long long asums[kCyMaxCylinders][kCyAxisSums];
    long long csums[kCyMaxCylinders][kCyCircSums];
    unsigned long long tot[kCyMaxCylinders][2];      // per round: count_p, Q_p
    unsigned ext[kCyMaxCylinders][2];                // per round: h_lo, h_hi as order-preserving words
};
static_assert(sizeof(CyState) == 10944, "include/pcreg.h states the workspace formula with roundup(sizeof(CyState), 256) = 11008");

// ransac.hip's sampler hash
__device__ __forceinline__ unsigned long long cy_splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull; unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// a float as a word whose unsigned order is the float's, and back
__device__ __forceinline__ unsigned cy_ord_of(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cy_ord_back(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
// frexp's exponent of the largest axis extent of the finite rows (0 where there is none or it is zero)
__device__ __forceinline__ int cy_exponent(const CyState* __restrict__ st) {
    double D = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned lo = st->box[c], hi = st->box[3 + c];
        if (lo <= hi) D = fmax(D, (double)cy_ord_back(hi) - (double)cy_ord_back(lo));
    }
    int e = 0;
    if (D > 0.0) (void)frexp(D, &e);
    return e;
}
// a 128-bit integer rounded ONCE to double (knn_iss.hip's construction)
__device__ __forceinline__ double cy_i128_to_double(__int128 v) {
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
// the contract's scoring chain for one row against the cylinder (axis point a, unit axis w, radius R): r2, and its q.  The distance
// to the axis is |d x w|, not sqrt(|d|^2 - (d . w)^2), which cancels.  The root is the correctly rounded fp32 one: the build keeps
// clang's default, under which sqrtf is exactly that (DESIGN 4.22 "The root")
struct CyCyl { float ax, ay, az, wx, wy, wz, R; };
__device__ __forceinline__ float cy_r2(float x, float y, float z, const CyCyl& c) {
    const float dx = x - c.ax, dy = y - c.ay, dz = z - c.az;
    const float cx = fmaf(dy, c.wz, -(dz * c.wy));
    const float cy = fmaf(dz, c.wx, -(dx * c.wz));
    const float cz = fmaf(dx, c.wy, -(dy * c.wx));
    const float c2 = fmaf(cz, cz, fmaf(cy, cy, cx * cx));
    const float r = __builtin_sqrtf(c2) - c.R;
    return r * r;
}
__device__ __forceinline__ int cy_q(float r2, float s) {     // min(2^20, rint(r2 s)); rint is monotone, so the cap may come first
    return (int)rintf(fminf(r2 * s, (float)kCyQMax));
}
__device__ __forceinline__ bool cy_finite(double v) { return v - v == 0.0; }
__device__ __forceinline__ bool cy_finitef(float v) { return v - v == 0.0f; }
__device__ __forceinline__ bool cy_usable(float a, float b, float c) {        // finite and at most 2 in magnitude (a NaN fails)
    return fabsf(a) <= 2.0f && fabsf(b) <= 2.0f && fabsf(c) <= 2.0f;
}

// ---- Z, I. reset and the alive rows ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCyBlock) void cy_reset_kernel(CyState* __restrict__ st, int P, double* __restrict__ cylinders,
                                                            double* __restrict__ extents, int32_t* __restrict__ counts,
                                                            double* __restrict__ rmse, int32_t* __restrict__ refit_used,
                                                            int32_t* __restrict__ n_cylinders, int32_t* __restrict__ best_trial,
                                                            long long* __restrict__ best_cost, int32_t* __restrict__ best_count) {
    const int tid = threadIdx.x;
    unsigned* w = (unsigned*)st;
    for (int i = tid; i < (int)(sizeof(CyState) / 4); i += kCyBlock) w[i] = 0u;
    __syncthreads();
    if (tid < 3) { st->box[tid] = 0xFFFFFFFFu; st->box[3 + tid] = 0u; }
    if (tid < kCyMaxCylinders) st->ext[tid][0] = 0xFFFFFFFFu;                 // (ext[.][1] = 0 is the maximum's start already)
    for (int i = tid; i < P; i += kCyBlock) {
        if (cylinders) for (int c = 0; c < 7; ++c) cylinders[7 * i + c] = 0.0;
        if (extents) { extents[2 * i] = 0.0; extents[2 * i + 1] = 0.0; }
        if (counts) counts[i] = 0;
        if (rmse) rmse[i] = 0.0;
        if (refit_used) refit_used[i] = 0;
        if (best_trial) best_trial[i] = 0;
        if (best_cost) best_cost[i] = 0;
        if (best_count) best_count[i] = 0;
    }
    if (tid == 0 && n_cylinders) *n_cylinders = 0;
}

__global__ __launch_bounds__(kCyBlock) void cy_init_kernel(const float* __restrict__ m, int M, int ldm, const float* __restrict__ nrm,
                                                           int ldn, CyState* __restrict__ st, uint8_t* __restrict__ alive,
                                                           uint8_t* __restrict__ nok, int32_t* __restrict__ labels) {
    __shared__ unsigned s[kCyBlock / 64][6];
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (int j = 0; j < kCyChunk / kCyBlock; ++j) {               // 2048 rows a workgroup: six atomics per 2048 rows
        const long long i = (long long)blockIdx.x * kCyChunk + (long long)j * kCyBlock + threadIdx.x;
        if (i < M) {
            const float x = m[i], y = m[i + (size_t)ldm], z = m[i + 2 * (size_t)ldm];
            const bool fin = finite3(x, y, z);
            alive[i] = fin ? 1 : 0;
            nok[i] = cy_usable(nrm[i], nrm[i + (size_t)ldn], nrm[i + 2 * (size_t)ldn]) ? 1 : 0;
            labels[i] = 0;
            if (fin) {
                const unsigned ox = cy_ord_of(x), oy = cy_ord_of(y), oz = cy_ord_of(z);
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
        for (int w = 1; w < kCyBlock / 64; ++w) v = c < 3 ? min(v, s[w][c]) : max(v, s[w][c]);
        if (c < 3) { if (v != 0xFFFFFFFFu) atomicMin(&st->box[c], v); }
        else if (v != 0u) atomicMax(&st->box[c], v);
    }
}

// ---- A1, A2. the alive list (chunk_scan.hpp's predicate compaction over the original rows) ------------------------------------------
__global__ __launch_bounds__(kScanBlock) void cy_count_kernel(const CyState* __restrict__ st, const uint8_t* __restrict__ alive, int M,
                                                              int32_t* __restrict__ pin) {
    if (st->done) return;
    chunk_pred_count(M, pin, [&](long long i) { return alive[i] != 0; });
}
__global__ __launch_bounds__(kScanBlock) void cy_list_kernel(CyState* __restrict__ st, const uint8_t* __restrict__ alive,
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
// hp0 is [3][B] floats, hcy [7][B] floats (af x y z, wf x y z, Rf), hvoid [B] bytes.  The cylinder is in double, every step one
// correctly rounded operation written so that no contraction can change it (the build has -ffp-contract=off as well)
__device__ __forceinline__ void cy_cross_rn(const double a[3], const double b[3], double c[3]) {
    c[0] = __dsub_rn(__dmul_rn(a[1], b[2]), __dmul_rn(a[2], b[1]));
    c[1] = __dsub_rn(__dmul_rn(a[2], b[0]), __dmul_rn(a[0], b[2]));
    c[2] = __dsub_rn(__dmul_rn(a[0], b[1]), __dmul_rn(a[1], b[0]));
}
__device__ __forceinline__ double cy_dot_rn(const double a[3], const double b[3]) {
    return __dadd_rn(__dadd_rn(__dmul_rn(a[0], b[0]), __dmul_rn(a[1], b[1])), __dmul_rn(a[2], b[2]));
}
__global__ __launch_bounds__(kCyBlock) void cy_hyp_kernel(const CyState* __restrict__ st, int p, int B, unsigned long long seed,
                                                          const int32_t* __restrict__ samples, int idx_base,
                                                          const uint8_t* __restrict__ alive, const uint8_t* __restrict__ nok,
                                                          const int32_t* __restrict__ A, const float* __restrict__ m, int M, int ldm,
                                                          const float* __restrict__ nrm, int ldn, float min_radius, float max_radius,
                                                          int use_ref, double rx, double ry, double rz, double rlen, double cos_max,
                                                          float* __restrict__ hp0, float* __restrict__ hcy, uint8_t* __restrict__ hvoid,
                                                          unsigned long long* __restrict__ cost, int32_t* __restrict__ count) {
    if (st->done) return;
    const int b = blockIdx.x * kCyBlock + threadIdx.x;
    if (b >= B) return;
    const int nA = st->nA;
    long long idx[2] = {0, 0};
    bool ok = true;
    if (samples) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            idx[j] = (long long)samples[((size_t)p * (size_t)B + (size_t)b) * 2 + j] - (long long)idx_base;
            if (idx[j] < 0 || idx[j] >= M) ok = false;
            else if (!alive[idx[j]]) ok = false;
        }
    } else if (nA > 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned long long h =
                cy_splitmix64(seed ^ cy_splitmix64(((unsigned long long)p * (unsigned long long)B + (unsigned long long)b) * 4ull + j));
            idx[j] = A[h % (unsigned long long)nA];
        }
    } else ok = false;
    if (ok && idx[0] == idx[1]) ok = false;
    if (ok && (!nok[idx[0]] || !nok[idx[1]])) ok = false;
    float p0[3] = {0.0f, 0.0f, 0.0f}, cy[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (ok) {
        double q[2][3], n[2][3];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                q[j][c] = (double)m[idx[j] + (size_t)c * (size_t)ldm];
                n[j][c] = (double)nrm[idx[j] + (size_t)c * (size_t)ldn];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) p0[c] = (float)q[0][c];
        double W[3];
        cy_cross_rn(n[0], n[1], W);
        const double L2 = cy_dot_rn(W, W);
        if (!(L2 > 0.0) || !cy_finite(L2)) ok = false;
        else {
            const double len = __dsqrt_rn(L2);
            double w[3] = {__ddiv_rn(W[0], len), __ddiv_rn(W[1], len), __ddiv_rn(W[2], len)};
            if (use_ref) {
                double dot = __dadd_rn(__dadd_rn(__dmul_rn(w[0], rx), __dmul_rn(w[1], ry)), __dmul_rn(w[2], rz));
                if (dot < 0.0) { w[0] = -w[0]; w[1] = -w[1]; w[2] = -w[2]; dot = -dot; }
                if (__ddiv_rn(dot, rlen) < cos_max) ok = false;
            } else if (fit_cylinders_negate(w, false, 0.0, 0.0, 0.0)) { w[0] = -w[0]; w[1] = -w[1]; w[2] = -w[2]; }
            double d[3], mm[3], a[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = __dsub_rn(q[1][c], q[0][c]);
            cy_cross_rn(d, n[1], mm);
            const double num = cy_dot_rn(mm, W);                  // with the UNSIGNED W
            const double s = __ddiv_rn(num, L2);
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] = __dadd_rn(q[0][c], __dmul_rn(s, n[0][c]));
            const double R = __dmul_rn(fabs(s), __dsqrt_rn(cy_dot_rn(n[0], n[0])));
            if (!cy_finite(s) || !cy_finite(a[0]) || !cy_finite(a[1]) || !cy_finite(a[2]) || !cy_finite(R)) ok = false;
            else {
#pragma unroll
                for (int c = 0; c < 3; ++c) { cy[c] = (float)a[c]; cy[3 + c] = (float)w[c]; }
                cy[6] = (float)R;
                bool fin = true;
#pragma unroll
                for (int c = 0; c < 7; ++c) fin = fin && cy_finitef(cy[c]);
                if (!fin) ok = false;
                else if (cy[6] < min_radius || cy[6] > max_radius) ok = false;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) hp0[(size_t)c * B + b] = p0[c];
#pragma unroll
    for (int c = 0; c < 7; ++c) hcy[(size_t)c * B + b] = ok ? cy[c] : 0.0f;
    hvoid[b] = ok ? 0 : 1;
    cost[b] = 0ull;
    count[b] = 0;
}

// ---- S. the scoring: B x nA evaluations ------------------------------------------------------------------------------------------------
// blockIdx.x = chunk of kCyChunk alive rows, blockIdx.y = 256 trials.  The rows sit in LDS as three arrays; a lane reads four rows of
// an array with one 16-byte load whose address is the same in every lane.  Rows past nA are staged as NaN: they pass no test.  Per
// chunk the inliers' q add up to at most 2048 2^20 = 2^31, inside an unsigned word; the others' 2^20 are added by their number.
__global__ __launch_bounds__(kCyBlock) void cy_score_kernel(const CyState* __restrict__ st, const float* __restrict__ cx,
                                                            const float* __restrict__ cy, const float* __restrict__ cz,
                                                            const float* __restrict__ hcy, int B, float t2, float s,
                                                            unsigned long long* __restrict__ cost, int32_t* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) float sx[kCyChunk];
    __shared__ __attribute__((aligned(16))) float sy[kCyChunk];
    __shared__ __attribute__((aligned(16))) float sz[kCyChunk];
    if (st->done) return;
    const int nA = st->nA;
    const long long r0 = (long long)blockIdx.x * kCyChunk;
    if (r0 >= nA) return;
    const int nrow = (int)min((long long)kCyChunk, (long long)nA - r0);
    const int tid = threadIdx.x;
    const float qnan = __uint_as_float(0x7FC00000u);
    for (int i = tid; i < kCyChunk; i += kCyBlock) {
        const bool in = i < nrow;
        sx[i] = in ? cx[r0 + i] : qnan; sy[i] = in ? cy[r0 + i] : qnan; sz[i] = in ? cz[r0 + i] : qnan;
    }
    __syncthreads();
    const int b = blockIdx.y * kCyBlock + tid;
    const int bb = min(b, B - 1);
    const CyCyl c = {hcy[bb], hcy[(size_t)B + bb], hcy[2 * (size_t)B + bb], hcy[3 * (size_t)B + bb], hcy[4 * (size_t)B + bb],
                     hcy[5 * (size_t)B + bb], hcy[6 * (size_t)B + bb]};
    unsigned qs = 0u;
    int cnt = 0;
    const int n4 = (nrow + 3) & ~3;
    for (int i = 0; i < n4; i += 4) {
        const float4 X = *(const float4*)&sx[i], Y = *(const float4*)&sy[i], Z = *(const float4*)&sz[i];
        const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float r2 = cy_r2(xs[u], ys[u], zs[u], c);
            const bool in = r2 <= t2;
            qs += in ? (unsigned)cy_q(r2, s) : 0u;
            cnt += in ? 1 : 0;
        }
    }
    if (b < B) {
        atomicAdd(&cost[b], (unsigned long long)qs + ((unsigned long long)(nrow - cnt) << 20));
        atomicAdd(&count[b], cnt);
    }
}

// ---- B. the best trial ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCyBlock) void cy_select_kernel(CyState* __restrict__ st, int p, int B, int min_inliers,
                                                             const uint8_t* __restrict__ hvoid, const unsigned long long* __restrict__ cost,
                                                             const int32_t* __restrict__ count, const float* __restrict__ hp0,
                                                             const float* __restrict__ hcy, int32_t* __restrict__ best_trial,
                                                             long long* __restrict__ best_cost, int32_t* __restrict__ best_count) {
    __shared__ unsigned long long sc[kCyBlock];
    __shared__ int sb[kCyBlock];
    if (st->done) return;
    const int tid = threadIdx.x;
    unsigned long long c = ~0ull;
    int bi = -1;
    for (int b = tid; b < B; b += kCyBlock) {              // ascending b per thread: the first of equal costs stays
        if (!hvoid[b] && count[b] >= 4 && cost[b] < c) { c = cost[b]; bi = b; }
    }
    sc[tid] = c; sb[tid] = bi;
    __syncthreads();
    for (int o = kCyBlock / 2; o > 0; o >>= 1) {
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
            for (int k = 0; k < 3; ++k) {
                st->p0[k] = hp0[(size_t)k * B + b]; st->ta[k] = hcy[(size_t)k * B + b]; st->tw[k] = hcy[(size_t)(3 + k) * B + b];
            }
            st->tR = hcy[6 * (size_t)B + b];
        }
    }
}

// ---- X, W, O, E. the refit --------------------------------------------------------------------------------------------------------
// N signed 64-bit sums of a workgroup: the waves by shuffles, the four waves through LDS, N atomics a workgroup (none where the
// workgroup counted nothing: a[0] is the count)
template <int N>
__device__ __forceinline__ void cy_block_sums(long long (&a)[N], long long* __restrict__ dst) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < N; ++c) a[c] += __shfl_xor(a[c], o);
    }
    __shared__ long long sw[kCyBlock / 64][N];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) sw[threadIdx.x >> 6][c] = a[c];
    }
    __syncthreads();
    if (threadIdx.x < N && sw[0][0] + sw[1][0] + sw[2][0] + sw[3][0] != 0) {
        const int c = threadIdx.x;
        atomicAdd((unsigned long long*)&dst[c], (unsigned long long)(sw[0][c] + sw[1][c] + sw[2][c] + sw[3][c]));
    }
}
__device__ __forceinline__ CyCyl cy_trial_of(const CyState* __restrict__ st) {
    return CyCyl{st->ta[0], st->ta[1], st->ta[2], st->tw[0], st->tw[1], st->tw[2], st->tR};
}

__global__ __launch_bounds__(kCyBlock) void cy_axis_kernel(CyState* __restrict__ st, int p, const int32_t* __restrict__ A,
                                                           const float* __restrict__ cx, const float* __restrict__ cy,
                                                           const float* __restrict__ cz, const uint8_t* __restrict__ nok,
                                                           const float* __restrict__ nrm, int ldn, float t2) {
    if (st->done) return;
    const int nA = st->nA;
    const long long k0 = (long long)blockIdx.x * kCyChunk;
    if (k0 >= nA) return;
    const CyCyl tr = cy_trial_of(st);
    long long a[kCyAxisSums];
#pragma unroll
    for (int c = 0; c < kCyAxisSums; ++c) a[c] = 0;
    for (int j = 0; j < kCyChunk / kCyBlock; ++j) {
        const long long k = k0 + (long long)j * kCyBlock + threadIdx.x;
        if (k < nA && cy_r2(cx[k], cy[k], cz[k], tr) <= t2) {
            const int row = A[k];
            if (nok[row]) {
                const long long gx = (long long)rint((double)nrm[row] * 65536.0);
                const long long gy = (long long)rint((double)nrm[row + (size_t)ldn] * 65536.0);
                const long long gz = (long long)rint((double)nrm[row + 2 * (size_t)ldn] * 65536.0);
                a[0] += 1;
                a[1] += gx * gx; a[2] += gx * gy; a[3] += gx * gz; a[4] += gy * gy; a[5] += gy * gz; a[6] += gz * gz;
            }
        }
    }
    cy_block_sums<kCyAxisSums>(a, st->asums[p]);
}

__global__ void cy_basis_kernel(CyState* __restrict__ st, int p, int use_ref, double rx, double ry, double rz) {
    if (st->done) return;
    const long long* S = st->asums[p];
    const double A6[6] = {(double)S[1], (double)S[2], (double)S[3], (double)S[4], (double)S[5], (double)S[6]};
    double w[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
    const bool ok = fit_cylinders_basis(A6, S[0], use_ref != 0, rx, ry, rz, w, u, v);
    st->basis_ok = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { st->w[k] = w[k]; st->u[k] = u[k]; st->v[k] = v[k]; }
}

__global__ __launch_bounds__(kCyBlock) void cy_circle_kernel(CyState* __restrict__ st, int p, const float* __restrict__ cx,
                                                             const float* __restrict__ cy, const float* __restrict__ cz, float t2) {
    if (st->done || !st->basis_ok) return;
    const int nA = st->nA;
    const long long k0 = (long long)blockIdx.x * kCyChunk;
    if (k0 >= nA) return;
    const float ox = st->p0[0], oy = st->p0[1], oz = st->p0[2];
    const CyCyl tr = cy_trial_of(st);
    const double ux = st->u[0], uy = st->u[1], uz = st->u[2], vx = st->v[0], vy = st->v[1], vz = st->v[2];
    const double scale = ldexp(1.0, 17 - cy_exponent(st));
    long long a[kCyCircSums];
#pragma unroll
    for (int c = 0; c < kCyCircSums; ++c) a[c] = 0;
    for (int j = 0; j < kCyChunk / kCyBlock; ++j) {
        const long long k = k0 + (long long)j * kCyBlock + threadIdx.x;
        if (k < nA) {
            const float x = cx[k], y = cy[k], z = cz[k];
            if (cy_r2(x, y, z, tr) <= t2) {
                const double gx = rint((double)(x - ox) * scale), gy = rint((double)(y - oy) * scale), gz = rint((double)(z - oz) * scale);
                const double X = __dadd_rn(__dadd_rn(__dmul_rn(gx, ux), __dmul_rn(gy, uy)), __dmul_rn(gz, uz));
                const double Y = __dadd_rn(__dadd_rn(__dmul_rn(gx, vx), __dmul_rn(gy, vy)), __dmul_rn(gz, vz));
                const long long xi = (long long)rint(X), yi = (long long)rint(Y);
                const long long w = xi * xi + yi * yi;
                const long long wl = w & ((1ll << kCySplit) - 1), wh = w >> kCySplit;
                a[0] += 1; a[1] += xi; a[2] += yi;
                a[3] += xi * xi; a[4] += xi * yi; a[5] += yi * yi;
                a[6] += w;
                a[7] += xi * wl; a[8] += xi * wh; a[9] += yi * wl; a[10] += yi * wh;
            }
        }
    }
    cy_block_sums<kCyCircSums>(a, st->csums[p]);
}

__global__ void cy_solve_kernel(CyState* __restrict__ st, int p, float min_radius, float max_radius, double* __restrict__ cylinders,
                                int32_t* __restrict__ refit_used) {
    if (st->done) return;
    double ctr[3] = {(double)st->ta[0], (double)st->ta[1], (double)st->ta[2]};
    double w[3] = {(double)st->tw[0], (double)st->tw[1], (double)st->tw[2]}, R = (double)st->tR;
    bool used = false;
    if (st->basis_ok) {
        const long long* S = st->csums[p];
        const __int128 n = S[0];
        double N3[3], h[2];
        N3[0] = cy_i128_to_double(n * S[3] - (__int128)S[1] * S[1]);
        N3[1] = cy_i128_to_double(n * S[4] - (__int128)S[1] * S[2]);
        N3[2] = cy_i128_to_double(n * S[5] - (__int128)S[2] * S[2]);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const __int128 gw = (__int128)S[8 + 2 * k] * ((__int128)1 << kCySplit) + (__int128)S[7 + 2 * k];     // sum xi w2, recombined
            h[k] = cy_i128_to_double(n * gw - (__int128)S[1 + k] * (__int128)S[6]);
        }
        const double S1[2] = {(double)S[1], (double)S[2]};
        const double p0[3] = {(double)st->p0[0], (double)st->p0[1], (double)st->p0[2]};
        const double u[3] = {st->u[0], st->u[1], st->u[2]}, v[3] = {st->v[0], st->v[1], st->v[2]};
        const double back = ldexp(1.0, -(17 - cy_exponent(st)));
        used = fit_cylinders_circle(N3, h, S1, (double)S[6], (double)S[0], p0, u, v, back, min_radius, max_radius, ctr, R);
        if (used) { w[0] = st->w[0]; w[1] = st->w[1]; w[2] = st->w[2]; }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cylinders[7 * p + k] = ctr[k]; cylinders[7 * p + 3 + k] = w[k];
        st->cf[k] = (float)ctr[k]; st->wf[k] = (float)w[k];
    }
    cylinders[7 * p + 6] = R;
    st->Rf = (float)R;
    refit_used[p] = used ? 1 : 0;
}

// ---- C, F. the classification ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCyBlock) void cy_classify_kernel(CyState* __restrict__ st, int p, const int32_t* __restrict__ A,
                                                               const float* __restrict__ cx, const float* __restrict__ cy,
                                                               const float* __restrict__ cz, float t2, float s,
                                                               uint8_t* __restrict__ alive, int32_t* __restrict__ labels) {
    if (st->done) return;
    const int nA = st->nA;
    const long long k0 = (long long)blockIdx.x * kCyChunk;
    if (k0 >= nA) return;
    const CyCyl c = {st->cf[0], st->cf[1], st->cf[2], st->wf[0], st->wf[1], st->wf[2], st->Rf};
    unsigned long long q = 0ull;
    int cnt = 0;
    unsigned hlo = 0xFFFFFFFFu, hhi = 0u;
    for (int j = 0; j < kCyChunk / kCyBlock; ++j) {
        const long long k = k0 + (long long)j * kCyBlock + threadIdx.x;
        if (k < nA) {
            const float x = cx[k], y = cy[k], z = cz[k];
            const float r2 = cy_r2(x, y, z, c);
            if (r2 <= t2) {
                const int row = A[k];
                labels[row] = p + 1;
                alive[row] = 0;
                q += (unsigned long long)cy_q(r2, s);
                ++cnt;
                const float dx = x - c.ax, dy = y - c.ay, dz = z - c.az;
                const unsigned oh = cy_ord_of(fmaf(dz, c.wz, fmaf(dy, c.wy, dx * c.wx)));
                hlo = min(hlo, oh); hhi = max(hhi, oh);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        q += __shfl_xor(q, o); cnt += __shfl_xor(cnt, o);
        hlo = min(hlo, (unsigned)__shfl_xor((int)hlo, o)); hhi = max(hhi, (unsigned)__shfl_xor((int)hhi, o));
    }
    __shared__ unsigned long long sw[kCyBlock / 64][2];
    __shared__ unsigned sh[kCyBlock / 64][2];
    if ((threadIdx.x & 63) == 0) {
        sw[threadIdx.x >> 6][0] = (unsigned long long)cnt; sw[threadIdx.x >> 6][1] = q;
        sh[threadIdx.x >> 6][0] = hlo; sh[threadIdx.x >> 6][1] = hhi;
    }
    __syncthreads();
    if (sw[0][0] + sw[1][0] + sw[2][0] + sw[3][0] == 0ull) return;
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        atomicAdd(&st->tot[p][k], sw[0][k] + sw[1][k] + sw[2][k] + sw[3][k]);
    } else if (threadIdx.x == 2) atomicMin(&st->ext[p][0], min(min(sh[0][0], sh[1][0]), min(sh[2][0], sh[3][0])));
    else if (threadIdx.x == 3) atomicMax(&st->ext[p][1], max(max(sh[0][1], sh[1][1]), max(sh[2][1], sh[3][1])));
}

__global__ void cy_finish_kernel(const CyState* __restrict__ st, int p, float t2, int32_t* __restrict__ counts, double* __restrict__ rmse,
                                 double* __restrict__ extents, int32_t* __restrict__ n_cylinders) {
    if (st->done) return;
    const unsigned long long n = st->tot[p][0], Q = st->tot[p][1];
    counts[p] = (int32_t)n;
    rmse[p] = sqrt(((double)Q / (double)n) * ((double)t2 * 9.5367431640625e-07));      // 2^-20
    extents[2 * p] = (double)cy_ord_back(st->ext[p][0]);          // (a round that labelled no row leaves NaN here, as in rmse)
    extents[2 * p + 1] = (double)cy_ord_back(st->ext[p][1]);
    *n_cylinders = p + 1;
}

// Workspace, with R = max(M, 1), C = max(ceil(M / 2048), 1) and T = B: [state, roundup(sizeof, 256)][alive bytes, R][usable-normal
// bytes, R][chunk counts, C int32][alive rows, R int32][their x, y, z, R floats each][p0, 3 T floats][af, wf and Rf, 7 T floats]
// [void bytes, T][cost, T uint64][count, T int32], every slot rounded up to 256 bytes
struct FitCylindersWs {
    CyState* st; uint8_t *alive, *nok; int32_t* pin; int32_t* A; float *cx, *cy, *cz; float *hp0, *hcy; uint8_t* hvoid;
    unsigned long long* cost; int32_t* count; int n_chunks;
};
FitCylindersWs fit_cylinders_ws_layout(int M, int B, void* base, size_t* bytes) {
    FitCylindersWs s{};
    WsWalk w(base);
    const size_t R = (size_t)(M > 0 ? M : 1), T = (size_t)(B > 0 ? B : 1);
    s.n_chunks = (int)((R + kScanChunk - 1) / kScanChunk);
    s.st = w.take<CyState>(1);
    s.alive = w.take<uint8_t>(R);
    s.nok = w.take<uint8_t>(R);
    s.pin = w.take<int32_t>((size_t)s.n_chunks);
    s.A = w.take<int32_t>(R);
    s.cx = w.take<float>(R); s.cy = w.take<float>(R); s.cz = w.take<float>(R);
    s.hp0 = w.take<float>(3 * T); s.hcy = w.take<float>(7 * T);
    s.hvoid = w.take<uint8_t>(T);
    s.cost = w.take<unsigned long long>(T);
    s.count = w.take<int32_t>(T);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t fit_cylinders_ws_bytes(int M, int B) {
    size_t b; (void)fit_cylinders_ws_layout(M, B, nullptr, &b);
    return b;
}

bool fit_cylinders_args_ok(float max_distance, float min_radius, float max_radius, const double* ref_vec, double max_angle,
                           int max_cylinders, int n_trials, int min_inliers) {
    if (!(std::isnormal(max_distance) && max_distance > 0.0f)) return false;
    const float t2 = max_distance * max_distance;
    if (!(std::isnormal(t2))) return false;                      // (the square is the threshold: it must be a normal float too)
    if (!(min_radius >= 0.0f && min_radius <= max_radius)) return false;      // (a NaN fails; max_radius may be +inf)
    if (ref_vec) {                                               // (pcreg_model_fit_planes_f32's rules)
        for (int c = 0; c < 3; ++c) if (!std::isfinite(ref_vec[c])) return false;
        const double l2 = (ref_vec[0] * ref_vec[0] + ref_vec[1] * ref_vec[1]) + ref_vec[2] * ref_vec[2];
        if (!(l2 > 0.0) || !std::isfinite(l2)) return false;
        if (!(max_angle > 0.0 && max_angle <= 1.5707963267948966)) return false;
    }
    return max_cylinders >= 1 && max_cylinders <= kCyMaxCylinders && n_trials >= 1 && n_trials <= kCyMaxTrials && min_inliers >= 4;
}
int fit_cylinders_max_rows() { return kCyMaxM; }

int launch_model_fit_cylinders(const ModelView& v, float max_distance, float min_radius, float max_radius, const double* ref_vec,
                               double max_angle, const float* normals, int ldn, int max_cylinders, int n_trials, int min_inliers,
                               unsigned long long seed, const int32_t* samples, int32_t idx_base, int32_t* labels, double* cylinders,
                               double* extents, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_cylinders,
                               int32_t* best_trial, int64_t* best_cost, int32_t* best_count, void* ws, size_t ws_bytes,
                               hipStream_t stream) {
    PCREG_ARG(fit_cylinders_args_ok(max_distance, min_radius, max_radius, ref_vec, max_angle, max_cylinders, n_trials, min_inliers) &&
              n_cylinders);
    PCREG_ARG(v.M < kCyMaxM && ((labels && cylinders && extents && counts && rmse && refit_used && normals && ldn >= v.M) || v.M == 0));
    size_t need;
    const FitCylindersWs s = fit_cylinders_ws_layout(v.M, n_trials, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: fit_cylinders workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M, B = n_trials, P = max_cylinders;
    hipLaunchKernelGGL(cy_reset_kernel, dim3(1), dim3(kCyBlock), 0, stream, s.st, P, cylinders, extents, counts, rmse, refit_used,
                       n_cylinders, best_trial, (long long*)best_cost, best_count);
    if (M == 0) { PCREG_HIP(hipGetLastError()); return PCREG_OK; }
    const float t2 = max_distance * max_distance;
    const float sc = (float)(1048576.0 / (double)t2);
    const int use_ref = ref_vec ? 1 : 0;
    const double rx = use_ref ? ref_vec[0] : 0.0, ry = use_ref ? ref_vec[1] : 0.0, rz = use_ref ? ref_vec[2] : 0.0;
    const double rlen = use_ref ? std::sqrt((rx * rx + ry * ry) + rz * rz) : 1.0;
    const double cos_max = use_ref ? std::cos(max_angle) : 0.0;
    hipLaunchKernelGGL(cy_init_kernel, dim3((unsigned)s.n_chunks), dim3(kCyBlock), 0, stream, v.m, M, v.ldm, normals, ldn, s.st, s.alive,
                       s.nok, labels);
    const dim3 cgrid((unsigned)s.n_chunks), cblock(kScanBlock), bgrid((unsigned)((B + kCyBlock - 1) / kCyBlock));
    const dim3 sgrid((unsigned)s.n_chunks, (unsigned)((B + kCyBlock - 1) / kCyBlock));
    for (int p = 0; p < P; ++p) {
        hipLaunchKernelGGL(cy_count_kernel, cgrid, cblock, 0, stream, (const CyState*)s.st, (const uint8_t*)s.alive, M, s.pin);
        hipLaunchKernelGGL(cy_list_kernel, cgrid, cblock, 0, stream, s.st, (const uint8_t*)s.alive, v.m, M, v.ldm, (const int32_t*)s.pin, s.A, s.cx,
                           s.cy, s.cz);
        hipLaunchKernelGGL(cy_hyp_kernel, bgrid, dim3(kCyBlock), 0, stream, (const CyState*)s.st, p, B, seed, samples, (int)idx_base,
                           (const uint8_t*)s.alive, (const uint8_t*)s.nok, (const int32_t*)s.A, v.m, M, v.ldm, normals, ldn, min_radius,
                           max_radius, use_ref, rx, ry, rz, rlen, cos_max, s.hp0, s.hcy, s.hvoid, s.cost, s.count);
        hipLaunchKernelGGL(cy_score_kernel, sgrid, dim3(kCyBlock), 0, stream, (const CyState*)s.st, (const float*)s.cx, (const float*)s.cy,
                           (const float*)s.cz, (const float*)s.hcy, B, t2, sc, s.cost, s.count);
        hipLaunchKernelGGL(cy_select_kernel, dim3(1), dim3(kCyBlock), 0, stream, s.st, p, B, min_inliers, (const uint8_t*)s.hvoid,
                           (const unsigned long long*)s.cost, (const int32_t*)s.count, (const float*)s.hp0, (const float*)s.hcy, best_trial,
                           (long long*)best_cost, best_count);
        hipLaunchKernelGGL(cy_axis_kernel, cgrid, dim3(kCyBlock), 0, stream, s.st, p, (const int32_t*)s.A, (const float*)s.cx,
                           (const float*)s.cy, (const float*)s.cz, (const uint8_t*)s.nok, normals, ldn, t2);
        hipLaunchKernelGGL(cy_basis_kernel, dim3(1), dim3(1), 0, stream, s.st, p, use_ref, rx, ry, rz);
        hipLaunchKernelGGL(cy_circle_kernel, cgrid, dim3(kCyBlock), 0, stream, s.st, p, (const float*)s.cx, (const float*)s.cy,
                           (const float*)s.cz, t2);
        hipLaunchKernelGGL(cy_solve_kernel, dim3(1), dim3(1), 0, stream, s.st, p, min_radius, max_radius, cylinders, refit_used);
        hipLaunchKernelGGL(cy_classify_kernel, cgrid, dim3(kCyBlock), 0, stream, s.st, p, (const int32_t*)s.A, (const float*)s.cx,
                           (const float*)s.cy, (const float*)s.cz, t2, sc, s.alive, labels);
        hipLaunchKernelGGL(cy_finish_kernel, dim3(1), dim3(1), 0, stream, (const CyState*)s.st, p, t2, counts, rmse, extents, n_cylinders);
    }
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
