// pcreg_amd/csrc/knn_fitsphere.hip -- MSAC sphere fitting and sphere extraction on a PREPARED model (MATLAB's pcfitsphere and the
// fit / remove / fit-again loop over it: the fiducial markers and ball tips of a scan): up to P spheres in one launch chain, nothing
// read on the host.  The contract is pcreg_model_fit_spheres_f32's (include/pcreg.h); DESIGN 4.22.
//
// The extraction skeleton is msac_extract.hpp's: a call is two launches and then nine per round p.  This file holds the sphere: the
// circumsphere of four rows, a radial residual with one correctly rounded fp32 root per (trial, row) pair, and an algebraic
// least-squares refit from seventeen exact integer sums (sphere_fit.hpp):
//   Z   sf_reset_kernel      msac_reset, and spheres and refit_used to zero
//   H   sf_hyp_kernel        one thread per trial: the four sample rows, the checks, the circumsphere in double, (p0, cf, Rf, void);
//                            the trial's cost and count to zero
//   R   sf_refit_kernel      the best trial's inliers: g = rint(d 2^(17 - e)), w = |g|^2 split at 2^18, the seventeen integer sums,
//                            seventeen atomics a workgroup
//   E   sf_solve_kernel      one thread: sum g w recombined, N and h in 128 bits, fit_spheres_solve, or the trial's own sphere
// and SphereShape: the residual of a row against (centre, R), where a trial's four floats lie, and which the state keeps.
#include "msac_extract.hpp"
#include "sphere_fit.hpp"

namespace pcreg {

namespace {

constexpr int kSfSums = 17;                          // n, S1 x y z, S2 xx xy xz yy yz zz, sum w, sum g w_lo x y z, sum g w_hi x y z
constexpr int kSfSplit = 18;                         // w = w_hi 2^18 + w_lo

struct SfState {
    MsacHead head;
    float p0[3];                                     // the best trial's first row (the refit's origin)
    float tc[3], tR;                                 // the best trial's sphere (the refit's inlier test)
    float cf[3], Rf;                                 // (float)centre and (float)R of the round's sphere (the classification)
    long long sums[kMsacMaxShapes][kSfSums];         // no overflow below 2^26 rows: |g| <= 2^17, |g w_lo|, |g w_hi| < 2^35
};
static_assert(sizeof(SfState) == 9824, "include/pcreg.h states the workspace formula with roundup(sizeof(SfState), 256) = 9984");

struct SphereShape {
    using State = SfState;
    using Tally = MsacNoTally;
    using Row = MsacNoRow;
    static constexpr int kSamples = 4, kMinCount = 4, kParams = 4;
    static constexpr bool kRowBytes = false;
    struct Trial { float cx, cy, cz, R; };
    // everything a trial scores with is in the parameter array (cf x y z, Rf); hp0 is only the refit's origin
    static __device__ __forceinline__ Trial load(const float* __restrict__, const float* __restrict__ hsp, size_t B, int b) {
        return Trial{hsp[b], hsp[B + b], hsp[2 * B + b], hsp[3 * B + b]};
    }
    // the contract's scoring chain for one row against the sphere (centre c, radius R).  The root is the correctly rounded fp32
    // one: the build keeps clang's default, under which sqrtf is exactly that (DESIGN 4.22 shows the instructions)
    static __device__ __forceinline__ float r2(float x, float y, float z, const Trial& t) {
        const float dx = x - t.cx, dy = y - t.cy, dz = z - t.cz;
        const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const float r = __builtin_sqrtf(d2) - t.R;
        return r * r;
    }
    static __device__ __forceinline__ void keep(State* __restrict__ st, const float* __restrict__ hp0, const float* __restrict__ hsp,
                                                size_t B, int b) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { st->p0[k] = hp0[k * B + b]; st->tc[k] = hsp[k * B + b]; }
        st->tR = hsp[3 * B + b];
    }
    static __device__ __forceinline__ Trial kept(const State* __restrict__ st) { return Trial{st->tc[0], st->tc[1], st->tc[2], st->tR}; }
    static __device__ __forceinline__ Trial fitted(const State* __restrict__ st) { return Trial{st->cf[0], st->cf[1], st->cf[2], st->Rf}; }
};

__global__ __launch_bounds__(kMsacBlock) void sf_reset_kernel(SfState* __restrict__ st, int P, MsacOut o, double* __restrict__ spheres,
                                                              int32_t* __restrict__ refit_used) {
    msac_reset(st, P, o);
    for (int i = threadIdx.x; i < P; i += kMsacBlock) {
        if (spheres) { spheres[4 * i] = 0.0; spheres[4 * i + 1] = 0.0; spheres[4 * i + 2] = 0.0; spheres[4 * i + 3] = 0.0; }
        if (refit_used) refit_used[i] = 0;
    }
}

// ---- H. the hypotheses ---------------------------------------------------------------------------------------------------------------
// hp0 is [3][B] floats, hsp [4][B] floats (cf x y z, Rf), hvoid [B] bytes.  The circumsphere is in double, every step one correctly
// rounded operation written so that no contraction can change it (the build has -ffp-contract=off as well)
__global__ __launch_bounds__(kMsacBlock) void sf_hyp_kernel(const MsacHead* __restrict__ st, int p, int B, unsigned long long seed,
                                                            const int32_t* __restrict__ samples, int idx_base,
                                                            const uint8_t* __restrict__ alive, const int32_t* __restrict__ A,
                                                            const float* __restrict__ m, int M, int ldm, float min_radius,
                                                            float max_radius, float* __restrict__ hp0, float* __restrict__ hsp,
                                                            uint8_t* __restrict__ hvoid, unsigned long long* __restrict__ cost,
                                                            int32_t* __restrict__ count) {
    if (st->done) return;
    const int b = blockIdx.x * kMsacBlock + threadIdx.x;
    if (b >= B) return;
    long long idx[SphereShape::kSamples];
    bool ok = msac_draw<SphereShape::kSamples>(st, p, B, b, seed, samples, idx_base, alive, A, M, idx);
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
        if (det == 0.0 || !msac_finite(det)) ok = false;
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
            if (!msac_finite(u[0]) || !msac_finite(u[1]) || !msac_finite(u[2]) || !msac_finite(R)) ok = false;
            else {
#pragma unroll
                for (int c = 0; c < 3; ++c) sp[c] = (float)__dadd_rn(q[0][c], u[c]);
                sp[3] = (float)R;
                if (!msac_finitef(sp[0]) || !msac_finitef(sp[1]) || !msac_finitef(sp[2]) || !msac_finitef(sp[3])) ok = false;
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

// ---- R, E. the refit -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMsacBlock) void sf_refit_kernel(SfState* __restrict__ st, int p, const float* __restrict__ cx,
                                                              const float* __restrict__ cy, const float* __restrict__ cz, float t2) {
    if (st->head.done) return;
    const int nA = st->head.nA;
    const long long k0 = (long long)blockIdx.x * kMsacChunk;
    if (k0 >= nA) return;
    const float ox = st->p0[0], oy = st->p0[1], oz = st->p0[2];
    const SphereShape::Trial tr = SphereShape::kept(st);
    const double scale = ldexp(1.0, 17 - msac_exponent(&st->head));
    long long a[kSfSums];
#pragma unroll
    for (int c = 0; c < kSfSums; ++c) a[c] = 0;
    for (int j = 0; j < kMsacChunk / kMsacBlock; ++j) {
        const long long k = k0 + (long long)j * kMsacBlock + threadIdx.x;
        if (k < nA) {
            const float x = cx[k], y = cy[k], z = cz[k];
            if (SphereShape::r2(x, y, z, tr) <= t2) {
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
    msac_block_sums<kSfSums>(a, st->sums[p]);
}

__global__ void sf_solve_kernel(SfState* __restrict__ st, int p, float min_radius, float max_radius, double* __restrict__ spheres,
                                int32_t* __restrict__ refit_used) {
    if (st->head.done) return;
    const long long* S = st->sums[p];
    const __int128 n = S[0];
    double N6[6], h[3], S1[3];
    N6[0] = i128_to_double(n * S[4] - (__int128)S[1] * S[1]);
    N6[1] = i128_to_double(n * S[5] - (__int128)S[1] * S[2]);
    N6[2] = i128_to_double(n * S[6] - (__int128)S[1] * S[3]);
    N6[3] = i128_to_double(n * S[7] - (__int128)S[2] * S[2]);
    N6[4] = i128_to_double(n * S[8] - (__int128)S[2] * S[3]);
    N6[5] = i128_to_double(n * S[9] - (__int128)S[3] * S[3]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const __int128 gw = (__int128)S[14 + k] * ((__int128)1 << kSfSplit) + (__int128)S[11 + k];     // sum g w, recombined
        h[k] = i128_to_double(n * gw - (__int128)S[1 + k] * (__int128)S[10]);
        S1[k] = (double)S[1 + k];
    }
    const double p0[3] = {(double)st->p0[0], (double)st->p0[1], (double)st->p0[2]};
    const double back = ldexp(1.0, -(17 - msac_exponent(&st->head)));
    double ctr[3] = {(double)st->tc[0], (double)st->tc[1], (double)st->tc[2]}, R = (double)st->tR;
    const bool used = fit_spheres_solve(N6, h, S1, (double)S[10], (double)S[0], p0, back, min_radius, max_radius, ctr, R);
#pragma unroll
    for (int k = 0; k < 3; ++k) { spheres[4 * p + k] = ctr[k]; st->cf[k] = (float)ctr[k]; }
    spheres[4 * p + 3] = R;
    st->Rf = (float)R;
    refit_used[p] = used ? 1 : 0;
}

}  // namespace

size_t fit_spheres_ws_bytes(int M, int B) {
    size_t b; (void)msac_ws_layout<SphereShape>(M, B, nullptr, &b);
    return b;
}

bool fit_spheres_args_ok(float max_distance, float min_radius, float max_radius, int max_spheres, int n_trials, int min_inliers) {
    return msac_args_ok(max_distance, max_spheres, n_trials, min_inliers, SphereShape::kMinCount) && msac_radii_ok(min_radius, max_radius);
}
int fit_spheres_max_rows() { return kMsacMaxM; }

int launch_model_fit_spheres(const ModelView& v, float max_distance, float min_radius, float max_radius, int max_spheres, int n_trials,
                             int min_inliers, unsigned long long seed, const int32_t* samples, int32_t idx_base, int32_t* labels,
                             double* spheres, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_spheres, int32_t* best_trial,
                             int64_t* best_cost, int32_t* best_count, void* ws, size_t ws_bytes, hipStream_t stream) {
    PCREG_ARG(fit_spheres_args_ok(max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers) && n_spheres);
    PCREG_ARG(v.M < kMsacMaxM && ((labels && spheres && counts && rmse && refit_used) || v.M == 0));
    size_t need;
    const MsacWs<SphereShape> s = msac_ws_layout<SphereShape>(v.M, n_trials, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: fit_spheres workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M, B = n_trials, P = max_spheres;
    const MsacOut o{labels, counts, rmse, n_spheres, best_trial, (long long*)best_cost, best_count};
    hipLaunchKernelGGL(sf_reset_kernel, dim3(1), dim3(kMsacBlock), 0, stream, s.st, P, o, spheres, refit_used);
    if (M == 0) { PCREG_HIP(hipGetLastError()); return PCREG_OK; }
    msac_launch_rounds(
        s, v, max_distance, P, B, min_inliers, o, nullptr, 0, MsacNoHook{},
        [&](int p, float) {
            hipLaunchKernelGGL(sf_hyp_kernel, msac_trial_grid(B), dim3(kMsacBlock), 0, stream, (const MsacHead*)&s.st->head, p, B, seed,
                               samples, (int)idx_base, (const uint8_t*)s.alive, (const int32_t*)s.A, v.m, M, v.ldm, min_radius, max_radius,
                               s.hp0, s.par, s.hvoid, s.cost, s.count);
        },
        [&](int p, float t2) {
            hipLaunchKernelGGL(sf_refit_kernel, msac_chunk_grid(s.n_chunks), dim3(kMsacBlock), 0, stream, s.st, p, (const float*)s.cx,
                               (const float*)s.cy, (const float*)s.cz, t2);
            hipLaunchKernelGGL(sf_solve_kernel, dim3(1), dim3(1), 0, stream, s.st, p, min_radius, max_radius, spheres, refit_used);
        },
        stream);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
