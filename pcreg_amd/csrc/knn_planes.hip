// pcreg_amd/csrc/knn_planes.hip -- MSAC plane fitting and plane extraction on a PREPARED model (MATLAB's pcfitplane and the
// fit / remove / fit-again loop of every segmentation example): up to P planes in one launch chain, nothing read on the host.
// The contract is pcreg_model_fit_planes_f32's (include/pcreg.h); DESIGN 4.21.
//
// The extraction skeleton is msac_extract.hpp's: a call is two launches and then nine per round p.  This file holds the plane:
//   Z   pl_reset_kernel      msac_reset, and planes and centres to zero
//   H   pl_hyp_kernel        one thread per trial: the three sample rows, the checks, n in double, its sign, (p0, nf, void); the
//                            trial's cost and count to zero
//   R   pl_refit_kernel      the best trial's inliers: g = rint(d 2^(17 - e)), the ten integer sums, ten atomics a workgroup
//   E   pl_plane_kernel      one thread: N in 128 bits, jacobi_sym3, the sign, the centre, d4
// and PlaneShape: the residual of a row against (origin, normal), where a trial's six floats lie, and which the state keeps.
#include "msac_extract.hpp"

namespace pcreg {

namespace {

struct PlState {
    MsacHead head;
    float p0[3], nf[3];                              // the best trial's plane (the refit's inlier test)
    float cf[3], nn[3];                              // (float)centre and (float)normal of the refit (the classification)
    long long sums[kMsacMaxShapes][10];              // per round: n, S1 x y z, S2 xx xy xz yy yz zz; |g| <= 2^17, so |S2| <= 2^26 2^34
};
static_assert(sizeof(PlState) == 6240, "include/pcreg.h states the workspace formula with roundup(sizeof(PlState), 256) = 6400");

struct PlaneShape {
    using State = PlState;
    using Tally = MsacNoTally;
    using Row = MsacNoRow;
    static constexpr int kSamples = 3, kMinCount = 3, kParams = 3;
    static constexpr bool kRowBytes = false;
    struct Trial { float ox, oy, oz, nx, ny, nz; };
    // a trial scores from its first row and its normal: the origin from hp0, three floats from the parameter array
    static __device__ __forceinline__ Trial load(const float* __restrict__ hp0, const float* __restrict__ hnf, size_t B, int b) {
        return Trial{hp0[b], hp0[B + b], hp0[2 * B + b], hnf[b], hnf[B + b], hnf[2 * B + b]};
    }
    // the contract's scoring chain for one row: r2 of the row against (origin o, normal n)
    static __device__ __forceinline__ float r2(float x, float y, float z, const Trial& t) {
        const float dx = x - t.ox, dy = y - t.oy, dz = z - t.oz;
        const float r = fmaf(t.nz, dz, fmaf(t.ny, dy, t.nx * dx));
        return r * r;
    }
    static __device__ __forceinline__ void keep(State* __restrict__ st, const float* __restrict__ hp0, const float* __restrict__ hnf,
                                                size_t B, int b) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { st->p0[k] = hp0[k * B + b]; st->nf[k] = hnf[k * B + b]; }
    }
    static __device__ __forceinline__ Trial kept(const State* __restrict__ st) {
        return Trial{st->p0[0], st->p0[1], st->p0[2], st->nf[0], st->nf[1], st->nf[2]};
    }
    static __device__ __forceinline__ Trial fitted(const State* __restrict__ st) {
        return Trial{st->cf[0], st->cf[1], st->cf[2], st->nn[0], st->nn[1], st->nn[2]};
    }
};

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

__global__ __launch_bounds__(kMsacBlock) void pl_reset_kernel(PlState* __restrict__ st, int P, MsacOut o, double* __restrict__ planes,
                                                              double* __restrict__ centres) {
    msac_reset(st, P, o);
    for (int i = threadIdx.x; i < P; i += kMsacBlock) {
        if (planes) { planes[4 * i] = 0.0; planes[4 * i + 1] = 0.0; planes[4 * i + 2] = 0.0; planes[4 * i + 3] = 0.0; }
        if (centres) { centres[3 * i] = 0.0; centres[3 * i + 1] = 0.0; centres[3 * i + 2] = 0.0; }
    }
}

// ---- H. the hypotheses ---------------------------------------------------------------------------------------------------------------
// hp0 / hnf are [3][B] floats, hvoid [B] bytes.  The cross product and the normalisation are in double, written so that no
// contraction can change them (the build has -ffp-contract=off as well)
__global__ __launch_bounds__(kMsacBlock) void pl_hyp_kernel(const MsacHead* __restrict__ st, int p, int B, unsigned long long seed,
                                                            const int32_t* __restrict__ samples, int idx_base,
                                                            const uint8_t* __restrict__ alive, const int32_t* __restrict__ A,
                                                            const float* __restrict__ m, int M, int ldm, MsacRef ref,
                                                            float* __restrict__ hp0, float* __restrict__ hnf, uint8_t* __restrict__ hvoid,
                                                            unsigned long long* __restrict__ cost, int32_t* __restrict__ count) {
    if (st->done) return;
    const int b = blockIdx.x * kMsacBlock + threadIdx.x;
    if (b >= B) return;
    long long idx[PlaneShape::kSamples];
    bool ok = msac_draw<PlaneShape::kSamples>(st, p, B, b, seed, samples, idx_base, alive, A, M, idx);
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
            if (ref.use) {
                double dot = pl_dot_ref(n, ref.x, ref.y, ref.z);
                if (dot < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; dot = -dot; }
                if (dot / ref.len < ref.cos_max) ok = false;
            } else if (pl_negate_largest(n)) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { hp0[(size_t)c * B + b] = p0[c]; hnf[(size_t)c * B + b] = (float)n[c]; }
    hvoid[b] = ok ? 0 : 1;
    cost[b] = 0ull;
    count[b] = 0;
}

// ---- R, E. the refit -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMsacBlock) void pl_refit_kernel(PlState* __restrict__ st, int p, const float* __restrict__ cx,
                                                              const float* __restrict__ cy, const float* __restrict__ cz, float t2) {
    if (st->head.done) return;
    const int nA = st->head.nA;
    const long long k0 = (long long)blockIdx.x * kMsacChunk;
    if (k0 >= nA) return;
    const PlaneShape::Trial tr = PlaneShape::kept(st);
    const double scale = ldexp(1.0, 17 - msac_exponent(&st->head));
    long long a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < kMsacChunk / kMsacBlock; ++j) {
        const long long k = k0 + (long long)j * kMsacBlock + threadIdx.x;
        if (k < nA) {
            const float x = cx[k], y = cy[k], z = cz[k];
            if (PlaneShape::r2(x, y, z, tr) <= t2) {
                const long long gx = (long long)rint((double)(x - tr.ox) * scale);
                const long long gy = (long long)rint((double)(y - tr.oy) * scale);
                const long long gz = (long long)rint((double)(z - tr.oz) * scale);
                a[0] += 1; a[1] += gx; a[2] += gy; a[3] += gz;
                a[4] += gx * gx; a[5] += gx * gy; a[6] += gx * gz; a[7] += gy * gy; a[8] += gy * gz; a[9] += gz * gz;
            }
        }
    }
    msac_block_sums<10>(a, st->sums[p]);
}

__global__ void pl_plane_kernel(PlState* __restrict__ st, int p, int use_ref, double rx, double ry, double rz,
                                double* __restrict__ planes, double* __restrict__ centres) {
    if (st->head.done) return;
    const long long* S = st->sums[p];
    const __int128 n = S[0];
    double a[6], V[9];
    a[0] = i128_to_double(n * S[4] - (__int128)S[1] * S[1]);
    a[1] = i128_to_double(n * S[5] - (__int128)S[1] * S[2]);
    a[2] = i128_to_double(n * S[6] - (__int128)S[1] * S[3]);
    a[3] = i128_to_double(n * S[7] - (__int128)S[2] * S[2]);
    a[4] = i128_to_double(n * S[8] - (__int128)S[2] * S[3]);
    a[5] = i128_to_double(n * S[9] - (__int128)S[3] * S[3]);
    jacobi_sym3(a, V);
    int c = 0;                                                    // the smallest eigenvalue, the first of equal ones
    if (a[3] < a[0]) c = 1;
    if (a[5] < (c == 1 ? a[3] : a[0])) c = 2;
    double nv[3] = {V[c], V[3 + c], V[6 + c]};
    const bool neg = use_ref ? pl_dot_ref(nv, rx, ry, rz) < 0.0 : pl_negate_largest(nv);
    if (neg) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
    const double back = ldexp(1.0, -(17 - msac_exponent(&st->head)));
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

}  // namespace

size_t planes_ws_bytes(int M, int B) {
    size_t b; (void)msac_ws_layout<PlaneShape>(M, B, nullptr, &b);
    return b;
}

bool planes_args_ok(float max_distance, const double* ref_vec, double max_angle, int max_planes, int n_trials, int min_inliers) {
    return msac_args_ok(max_distance, max_planes, n_trials, min_inliers, PlaneShape::kMinCount) && msac_ref_ok(ref_vec, max_angle);
}
int planes_max_rows() { return kMsacMaxM; }

int launch_model_fit_planes(const ModelView& v, float max_distance, const double* ref_vec, double max_angle, int max_planes, int n_trials,
                            int min_inliers, unsigned long long seed, const int32_t* samples, int32_t idx_base, int32_t* labels,
                            double* planes, double* centres, int32_t* counts, double* rmse, int32_t* n_planes, int32_t* best_trial,
                            int64_t* best_cost, int32_t* best_count, void* ws, size_t ws_bytes, hipStream_t stream) {
    PCREG_ARG(planes_args_ok(max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers) && n_planes);
    PCREG_ARG(v.M < kMsacMaxM && ((labels && planes && centres && counts && rmse) || v.M == 0));
    size_t need;
    const MsacWs<PlaneShape> s = msac_ws_layout<PlaneShape>(v.M, n_trials, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: fit_planes workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M, B = n_trials, P = max_planes;
    const MsacOut o{labels, counts, rmse, n_planes, best_trial, (long long*)best_cost, best_count};
    hipLaunchKernelGGL(pl_reset_kernel, dim3(1), dim3(kMsacBlock), 0, stream, s.st, P, o, planes, centres);
    if (M == 0) { PCREG_HIP(hipGetLastError()); return PCREG_OK; }
    const MsacRef ref = msac_ref(ref_vec, max_angle);
    msac_launch_rounds(
        s, v, max_distance, P, B, min_inliers, o, nullptr, 0, MsacNoHook{},
        [&](int p, float) {
            hipLaunchKernelGGL(pl_hyp_kernel, msac_trial_grid(B), dim3(kMsacBlock), 0, stream, (const MsacHead*)&s.st->head, p, B, seed,
                               samples, (int)idx_base, (const uint8_t*)s.alive, (const int32_t*)s.A, v.m, M, v.ldm, ref, s.hp0, s.par,
                               s.hvoid, s.cost, s.count);
        },
        [&](int p, float t2) {
            hipLaunchKernelGGL(pl_refit_kernel, msac_chunk_grid(s.n_chunks), dim3(kMsacBlock), 0, stream, s.st, p, (const float*)s.cx,
                               (const float*)s.cy, (const float*)s.cz, t2);
            hipLaunchKernelGGL(pl_plane_kernel, dim3(1), dim3(1), 0, stream, s.st, p, ref.use, ref.x, ref.y, ref.z, planes, centres);
        },
        stream);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
