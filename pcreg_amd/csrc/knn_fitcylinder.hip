// pcreg_amd/csrc/knn_fitcylinder.hip -- MSAC cylinder fitting and cylinder extraction on a PREPARED model with normals (MATLAB's
// pcfitcylinder and the fit / remove / fit-again loop over it: the instrument shafts, sleeves, trocars and rods of a surgical
// scene): up to P cylinders in one launch chain, nothing read on the host.  The contract is pcreg_model_fit_cylinders_f32's
// (include/pcreg.h); DESIGN 4.23.
//
// The extraction skeleton is msac_extract.hpp's: a call is two launches and then eleven per round p.  This file holds the
// cylinder: a trial is two rows and their normals (the axis along n_0 x n_1, through the point where the two normal lines pass
// closest), the residual is radial about a line (a cross product and one correctly rounded fp32 root per (trial, row) pair), and
// the refit takes two exact passes (cylinder_fit.hpp).  The normals are read by ORIGINAL row; scoring reads none:
//   Z   cy_reset_kernel      msac_reset, the extents' starting words, and cylinders, extents and refit_used to zero
//   I   CyRow                the usable-normal byte of every row
//   H   cy_hyp_kernel        one thread per trial: the two sample rows and their normals, the checks, the cylinder in double,
//                            (p0, af, wf, Rf, void); the trial's cost and count to zero
//   X   cy_axis_kernel       the best trial's inliers with a usable normal: gn = rint(n 2^16), seven integer sums
//   W   cy_basis_kernel      one thread: fit_cylinders_basis (Jacobi, w, u, v)
//   O   cy_circle_kernel     the best trial's inliers: g = rint(d 2^(17 - e)) projected on (u, v) and rounded, eleven integer sums
//   E   cy_solve_kernel      one thread: N and h in 128 bits, fit_cylinders_circle, or the trial's own cylinder
//   C   CyExtent             the extent of a round's inliers along the axis by integer atomic min / max on order-preserving words
//   F   CyFinishHook         the extents
// and CylinderShape: the residual, where a trial's seven floats lie, and which the state keeps.
#include "msac_extract.hpp"
#include "cylinder_fit.hpp"

namespace pcreg {

namespace {

constexpr int kCyAxisSums = 7;                       // n_n, sum gn_a gn_b: xx xy xz yy yz zz
constexpr int kCyCircSums = 11;                      // n, sum xi, yi, sum xi xi, xi yi, yi yi, sum w2, sum xi w_lo, xi w_hi, yi w_lo, yi w_hi
constexpr int kCySplit = 18;                         // w2 = w_hi 2^18 + w_lo

// The sums' bounds at M < 2^26 rows.  Axis: |gn| <= 2^17 (|n_c| <= 2), so |gn_a gn_b| <= 2^34 and every sum is below 2^60.
// Circle: |g_c| <= 2^17 gives |g| <= sqrt(3) 2^17 and, (u, v) being orthonormal to rounding, |xi|, |yi| < 2^18 and
// w2 = xi^2 + yi^2 < 2^36, so w_lo, w_hi < 2^18: n < 2^26; |sum xi|, |sum yi| < 2^44; the three sums of products < 2^62;
// sum w2 < 2^62; |sum xi w_lo| .. |sum yi w_hi| < 2^62.  All inside a signed 64-bit word.
struct CyState {
    MsacHead head;
    float p0[3];                                     // the best trial's first row (the circle pass' origin)
    float ta[3], tw[3], tR;                          // the best trial's cylinder (the refit's inlier test)
    float cf[3], wf[3], Rf;                          // (float)centre, (float)w and (float)R of the round's cylinder (the classification)
    int basis_ok;
    double w[3], u[3], v[3];                         // the refit's axis and the basis of its cross-section
    long long asums[kMsacMaxShapes][kCyAxisSums];
    long long csums[kMsacMaxShapes][kCyCircSums];
    unsigned ext[kMsacMaxShapes][2];                 // per round: h_lo, h_hi as order-preserving words
};
static_assert(sizeof(CyState) == 10944, "include/pcreg.h states the workspace formula with roundup(sizeof(CyState), 256) = 11008");

// the classification's extent along the axis: h = (row - centre) . w of every inlier, min and max a workgroup
struct CyExtent {
    unsigned hlo = 0xFFFFFFFFu, hhi = 0u;
    template <class Trial>
    __device__ __forceinline__ void add(float x, float y, float z, const Trial& c) {
        const float dx = x - c.ax, dy = y - c.ay, dz = z - c.az;
        const unsigned oh = ord_of(fmaf(dz, c.wz, fmaf(dy, c.wy, dx * c.wx)));
        hlo = min(hlo, oh); hhi = max(hhi, oh);
    }
    __device__ __forceinline__ void wave() {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            hlo = min(hlo, (unsigned)__shfl_xor((int)hlo, o)); hhi = max(hhi, (unsigned)__shfl_xor((int)hhi, o));
        }
    }
    __device__ __forceinline__ unsigned (*lds())[2] {
        __shared__ unsigned sh[kMsacBlock / 64][2];
        return sh;
    }
    __device__ __forceinline__ void stage() {
        if ((threadIdx.x & 63) == 0) { lds()[threadIdx.x >> 6][0] = hlo; lds()[threadIdx.x >> 6][1] = hhi; }
    }
    __device__ __forceinline__ void commit(CyState* __restrict__ st, int p) {    // (behind the barrier, threads 2 and up)
        unsigned (*sh)[2] = lds();
        if (threadIdx.x == 2) atomicMin(&st->ext[p][0], min(min(sh[0][0], sh[1][0]), min(sh[2][0], sh[3][0])));
        else if (threadIdx.x == 3) atomicMax(&st->ext[p][1], max(max(sh[0][1], sh[1][1]), max(sh[2][1], sh[3][1])));
    }
};

// I's row byte: a normal is usable where it is finite and at most 2 in magnitude (a NaN fails)
struct CyRow {
    static __device__ __forceinline__ bool usable(float a, float b, float c) { return fabsf(a) <= 2.0f && fabsf(b) <= 2.0f && fabsf(c) <= 2.0f; }
    static __device__ __forceinline__ void row(const float* __restrict__ nrm, int ldn, uint8_t* __restrict__ nok, long long i) {
        nok[i] = usable(nrm[i], nrm[i + (size_t)ldn], nrm[i + 2 * (size_t)ldn]) ? 1 : 0;      // (three loads, whatever the first says)
    }
};

struct CylinderShape {
    using State = CyState;
    using Tally = CyExtent;
    using Row = CyRow;
    static constexpr int kSamples = 2, kMinCount = 4, kParams = 7;
    static constexpr bool kRowBytes = true;          // the usable-normal byte
    struct Trial { float ax, ay, az, wx, wy, wz, R; };
    // everything a trial scores with is in the parameter array (af x y z, wf x y z, Rf); hp0 is only the circle pass' origin
    static __device__ __forceinline__ Trial load(const float* __restrict__, const float* __restrict__ hcy, size_t B, int b) {
        return Trial{hcy[b], hcy[B + b], hcy[2 * B + b], hcy[3 * B + b], hcy[4 * B + b], hcy[5 * B + b], hcy[6 * B + b]};
    }
    // the contract's scoring chain for one row against the cylinder (axis point a, unit axis w, radius R).  The distance to the
    // axis is |d x w|, not sqrt(|d|^2 - (d . w)^2), which cancels.  The root is the correctly rounded fp32 one: the build keeps
    // clang's default, under which sqrtf is exactly that (DESIGN 4.22 "The root")
    static __device__ __forceinline__ float r2(float x, float y, float z, const Trial& c) {
        const float dx = x - c.ax, dy = y - c.ay, dz = z - c.az;
        const float cx = fmaf(dy, c.wz, -(dz * c.wy));
        const float cy = fmaf(dz, c.wx, -(dx * c.wz));
        const float cz = fmaf(dx, c.wy, -(dy * c.wx));
        const float c2 = fmaf(cz, cz, fmaf(cy, cy, cx * cx));
        const float r = __builtin_sqrtf(c2) - c.R;
        return r * r;
    }
    static __device__ __forceinline__ void keep(State* __restrict__ st, const float* __restrict__ hp0, const float* __restrict__ hcy,
                                                size_t B, int b) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { st->p0[k] = hp0[k * B + b]; st->ta[k] = hcy[k * B + b]; st->tw[k] = hcy[(3 + k) * B + b]; }
        st->tR = hcy[6 * B + b];
    }
    static __device__ __forceinline__ Trial kept(const State* __restrict__ st) {
        return Trial{st->ta[0], st->ta[1], st->ta[2], st->tw[0], st->tw[1], st->tw[2], st->tR};
    }
    static __device__ __forceinline__ Trial fitted(const State* __restrict__ st) {
        return Trial{st->cf[0], st->cf[1], st->cf[2], st->wf[0], st->wf[1], st->wf[2], st->Rf};
    }
};

// F's hook: the extents (a round that labelled no row leaves NaN here, as in rmse)
struct CyFinishHook {
    const CyState* st; double* extents;
    __device__ void operator()(long long p) const {
        extents[2 * p] = (double)ord_back(st->ext[p][0]);
        extents[2 * p + 1] = (double)ord_back(st->ext[p][1]);
    }
};

__global__ __launch_bounds__(kMsacBlock) void cy_reset_kernel(CyState* __restrict__ st, int P, MsacOut o, double* __restrict__ cylinders,
                                                              double* __restrict__ extents, int32_t* __restrict__ refit_used) {
    msac_reset(st, P, o);
    if (threadIdx.x < kMsacMaxShapes) st->ext[threadIdx.x][0] = 0xFFFFFFFFu;  // (ext[.][1] = 0 is the maximum's start already)
    for (int i = threadIdx.x; i < P; i += kMsacBlock) {
        if (cylinders) for (int c = 0; c < 7; ++c) cylinders[7 * i + c] = 0.0;
        if (extents) { extents[2 * i] = 0.0; extents[2 * i + 1] = 0.0; }
        if (refit_used) refit_used[i] = 0;
    }
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
__global__ __launch_bounds__(kMsacBlock) void cy_hyp_kernel(const MsacHead* __restrict__ st, int p, int B, unsigned long long seed,
                                                            const int32_t* __restrict__ samples, int idx_base,
                                                            const uint8_t* __restrict__ alive, const uint8_t* __restrict__ nok,
                                                            const int32_t* __restrict__ A, const float* __restrict__ m, int M, int ldm,
                                                            const float* __restrict__ nrm, int ldn, float min_radius, float max_radius,
                                                            MsacRef ref, float* __restrict__ hp0, float* __restrict__ hcy,
                                                            uint8_t* __restrict__ hvoid, unsigned long long* __restrict__ cost,
                                                            int32_t* __restrict__ count) {
    if (st->done) return;
    const int b = blockIdx.x * kMsacBlock + threadIdx.x;
    if (b >= B) return;
    long long idx[CylinderShape::kSamples];
    bool ok = msac_draw<CylinderShape::kSamples>(st, p, B, b, seed, samples, idx_base, alive, A, M, idx);
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
        if (!(L2 > 0.0) || !msac_finite(L2)) ok = false;
        else {
            const double len = __dsqrt_rn(L2);
            double w[3] = {__ddiv_rn(W[0], len), __ddiv_rn(W[1], len), __ddiv_rn(W[2], len)};
            if (ref.use) {
                double dot = __dadd_rn(__dadd_rn(__dmul_rn(w[0], ref.x), __dmul_rn(w[1], ref.y)), __dmul_rn(w[2], ref.z));
                if (dot < 0.0) { w[0] = -w[0]; w[1] = -w[1]; w[2] = -w[2]; dot = -dot; }
                if (__ddiv_rn(dot, ref.len) < ref.cos_max) ok = false;
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
            if (!msac_finite(s) || !msac_finite(a[0]) || !msac_finite(a[1]) || !msac_finite(a[2]) || !msac_finite(R)) ok = false;
            else {
#pragma unroll
                for (int c = 0; c < 3; ++c) { cy[c] = (float)a[c]; cy[3 + c] = (float)w[c]; }
                cy[6] = (float)R;
                bool fin = true;
#pragma unroll
                for (int c = 0; c < 7; ++c) fin = fin && msac_finitef(cy[c]);
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

// ---- X, W, O, E. the refit --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMsacBlock) void cy_axis_kernel(CyState* __restrict__ st, int p, const int32_t* __restrict__ A,
                                                             const float* __restrict__ cx, const float* __restrict__ cy,
                                                             const float* __restrict__ cz, const uint8_t* __restrict__ nok,
                                                             const float* __restrict__ nrm, int ldn, float t2) {
    if (st->head.done) return;
    const int nA = st->head.nA;
    const long long k0 = (long long)blockIdx.x * kMsacChunk;
    if (k0 >= nA) return;
    const CylinderShape::Trial tr = CylinderShape::kept(st);
    long long a[kCyAxisSums];
#pragma unroll
    for (int c = 0; c < kCyAxisSums; ++c) a[c] = 0;
    for (int j = 0; j < kMsacChunk / kMsacBlock; ++j) {
        const long long k = k0 + (long long)j * kMsacBlock + threadIdx.x;
        if (k < nA && CylinderShape::r2(cx[k], cy[k], cz[k], tr) <= t2) {
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
    msac_block_sums<kCyAxisSums>(a, st->asums[p]);
}

__global__ void cy_basis_kernel(CyState* __restrict__ st, int p, int use_ref, double rx, double ry, double rz) {
    if (st->head.done) return;
    const long long* S = st->asums[p];
    const double A6[6] = {(double)S[1], (double)S[2], (double)S[3], (double)S[4], (double)S[5], (double)S[6]};
    double w[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
    const bool ok = fit_cylinders_basis(A6, S[0], use_ref != 0, rx, ry, rz, w, u, v);
    st->basis_ok = ok ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { st->w[k] = w[k]; st->u[k] = u[k]; st->v[k] = v[k]; }
}

__global__ __launch_bounds__(kMsacBlock) void cy_circle_kernel(CyState* __restrict__ st, int p, const float* __restrict__ cx,
                                                               const float* __restrict__ cy, const float* __restrict__ cz, float t2) {
    if (st->head.done || !st->basis_ok) return;
    const int nA = st->head.nA;
    const long long k0 = (long long)blockIdx.x * kMsacChunk;
    if (k0 >= nA) return;
    const float ox = st->p0[0], oy = st->p0[1], oz = st->p0[2];
    const CylinderShape::Trial tr = CylinderShape::kept(st);
    const double ux = st->u[0], uy = st->u[1], uz = st->u[2], vx = st->v[0], vy = st->v[1], vz = st->v[2];
    const double scale = ldexp(1.0, 17 - msac_exponent(&st->head));
    long long a[kCyCircSums];
#pragma unroll
    for (int c = 0; c < kCyCircSums; ++c) a[c] = 0;
    for (int j = 0; j < kMsacChunk / kMsacBlock; ++j) {
        const long long k = k0 + (long long)j * kMsacBlock + threadIdx.x;
        if (k < nA) {
            const float x = cx[k], y = cy[k], z = cz[k];
            if (CylinderShape::r2(x, y, z, tr) <= t2) {
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
    msac_block_sums<kCyCircSums>(a, st->csums[p]);
}

__global__ void cy_solve_kernel(CyState* __restrict__ st, int p, float min_radius, float max_radius, double* __restrict__ cylinders,
                                int32_t* __restrict__ refit_used) {
    if (st->head.done) return;
    double ctr[3] = {(double)st->ta[0], (double)st->ta[1], (double)st->ta[2]};
    double w[3] = {(double)st->tw[0], (double)st->tw[1], (double)st->tw[2]}, R = (double)st->tR;
    bool used = false;
    if (st->basis_ok) {
        const long long* S = st->csums[p];
        const __int128 n = S[0];
        double N3[3], h[2];
        N3[0] = i128_to_double(n * S[3] - (__int128)S[1] * S[1]);
        N3[1] = i128_to_double(n * S[4] - (__int128)S[1] * S[2]);
        N3[2] = i128_to_double(n * S[5] - (__int128)S[2] * S[2]);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const __int128 gw = (__int128)S[8 + 2 * k] * ((__int128)1 << kCySplit) + (__int128)S[7 + 2 * k];     // sum xi w2, recombined
            h[k] = i128_to_double(n * gw - (__int128)S[1 + k] * (__int128)S[6]);
        }
        const double S1[2] = {(double)S[1], (double)S[2]};
        const double p0[3] = {(double)st->p0[0], (double)st->p0[1], (double)st->p0[2]};
        const double u[3] = {st->u[0], st->u[1], st->u[2]}, v[3] = {st->v[0], st->v[1], st->v[2]};
        const double back = ldexp(1.0, -(17 - msac_exponent(&st->head)));
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

}  // namespace

size_t fit_cylinders_ws_bytes(int M, int B) {
    size_t b; (void)msac_ws_layout<CylinderShape>(M, B, nullptr, &b);
    return b;
}

bool fit_cylinders_args_ok(float max_distance, float min_radius, float max_radius, const double* ref_vec, double max_angle,
                           int max_cylinders, int n_trials, int min_inliers) {
    return msac_args_ok(max_distance, max_cylinders, n_trials, min_inliers, CylinderShape::kMinCount) &&
           msac_radii_ok(min_radius, max_radius) && msac_ref_ok(ref_vec, max_angle);
}
int fit_cylinders_max_rows() { return kMsacMaxM; }

int launch_model_fit_cylinders(const ModelView& v, float max_distance, float min_radius, float max_radius, const double* ref_vec,
                               double max_angle, const float* normals, int ldn, int max_cylinders, int n_trials, int min_inliers,
                               unsigned long long seed, const int32_t* samples, int32_t idx_base, int32_t* labels, double* cylinders,
                               double* extents, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_cylinders,
                               int32_t* best_trial, int64_t* best_cost, int32_t* best_count, void* ws, size_t ws_bytes,
                               hipStream_t stream) {
    PCREG_ARG(fit_cylinders_args_ok(max_distance, min_radius, max_radius, ref_vec, max_angle, max_cylinders, n_trials, min_inliers) &&
              n_cylinders);
    PCREG_ARG(v.M < kMsacMaxM && ((labels && cylinders && extents && counts && rmse && refit_used && normals && ldn >= v.M) || v.M == 0));
    size_t need;
    const MsacWs<CylinderShape> s = msac_ws_layout<CylinderShape>(v.M, n_trials, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: fit_cylinders workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M, B = n_trials, P = max_cylinders;
    const MsacOut o{labels, counts, rmse, n_cylinders, best_trial, (long long*)best_cost, best_count};
    hipLaunchKernelGGL(cy_reset_kernel, dim3(1), dim3(kMsacBlock), 0, stream, s.st, P, o, cylinders, extents, refit_used);
    if (M == 0) { PCREG_HIP(hipGetLastError()); return PCREG_OK; }
    const MsacRef ref = msac_ref(ref_vec, max_angle);
    const dim3 cgrid = msac_chunk_grid(s.n_chunks), block(kMsacBlock);
    msac_launch_rounds(
        s, v, max_distance, P, B, min_inliers, o, normals, ldn, CyFinishHook{s.st, extents},
        [&](int p, float) {
            hipLaunchKernelGGL(cy_hyp_kernel, msac_trial_grid(B), block, 0, stream, (const MsacHead*)&s.st->head, p, B, seed, samples,
                               (int)idx_base, (const uint8_t*)s.alive, (const uint8_t*)s.rowb, (const int32_t*)s.A, v.m, M, v.ldm, normals,
                               ldn, min_radius, max_radius, ref, s.hp0, s.par, s.hvoid, s.cost, s.count);
        },
        [&](int p, float t2) {
            hipLaunchKernelGGL(cy_axis_kernel, cgrid, block, 0, stream, s.st, p, (const int32_t*)s.A, (const float*)s.cx, (const float*)s.cy,
                               (const float*)s.cz, (const uint8_t*)s.rowb, normals, ldn, t2);
            hipLaunchKernelGGL(cy_basis_kernel, dim3(1), dim3(1), 0, stream, s.st, p, ref.use, ref.x, ref.y, ref.z);
            hipLaunchKernelGGL(cy_circle_kernel, cgrid, block, 0, stream, s.st, p, (const float*)s.cx, (const float*)s.cy, (const float*)s.cz,
                               t2);
            hipLaunchKernelGGL(cy_solve_kernel, dim3(1), dim3(1), 0, stream, s.st, p, min_radius, max_radius, cylinders, refit_used);
        },
        stream);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
