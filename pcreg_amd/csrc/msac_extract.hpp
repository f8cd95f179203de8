// pcreg_amd/csrc/msac_extract.hpp -- the MSAC extraction skeleton, its one definition: what the plane, sphere and cylinder fitters
// of a PREPARED model share (knn_planes.hip, knn_fitsphere.hip, knn_fitcylinder.hip).  A call is two launches
// and then, per round p, eight launches of the skeleton's and the shape's refit stage between B and C:
//   Z   the shape's reset kernel    one workgroup: msac_reset (the state, the common P-sized outputs), then the shape's own outputs
//   I   msac_init_kernel<Row>       labels = 0, the alive byte of every row (its three coordinates finite), the shape's row bytes, the
//                                   box of the finite rows by integer atomic min / max on order-preserving words
//   A1  msac_count_kernel           chunk_scan.hpp's first launch over the alive bytes
//   A2  msac_list_kernel            its second: the alive rows ascending, their coordinates packed behind them, their number nA
//   H   the shape's hyp kernel      one thread per trial: msac_draw, the shape's geometry, (p0, parameters, void); cost, count = 0
//   S   msac_score_kernel<Shape>    THE HOT PATH: lane = trial.  A workgroup stages 2048 alive rows in LDS and each of its 256 lanes
//                                   walks them with its own trial in registers (the LDS reads are wave-uniform: a broadcast, no bank
//                                   conflict), so a (trial, row) pair costs no cross-lane step; one 64-bit and one 32-bit integer
//                                   atomic per (chunk, trial)
//   B   msac_select_kernel<Shape>   one workgroup: the smallest (cost, b) among the eligible trials; the stop rule; the diagnostics
//   ..  the shape's refit stage     integer sums of the best trial's inliers (msac_block_sums) and one-thread solves
//   C   msac_classify_kernel<Shape> the final fp32 classification: labels, alive bytes, the round's count and Q by integer atomics,
//                                   the shape's tally
//   F   msac_finish_kernel          one thread: counts, rmse, the finish hook, n_shapes = p + 1
// Every sum across rows is an INTEGER sum: no order of summation, no floating-point atomic.  A device word says that extraction has
// ended; every later launch reads it and returns.  Nothing synchronises; no workgroup waits for another.
//
// A Shape supplies:
//   State                      a struct whose FIRST member is `MsacHead head`; the rest is the shape's own
//   kSamples, kMinCount        rows per trial; the least count a trial needs to be eligible (and the least min_inliers)
//   kParams, kRowBytes         floats per trial in the parameter array; whether the workspace holds a second byte per row
//   Trial, load(hp0, par, B, b)   a trial's scoring registers, and how they are read from the [3][B] origins and [kParams][B] parameters
//   r2(x, y, z, trial)         the contract's fp32 residual chain
//   keep(st, hp0, par, B, b)   the winner's floats into the state;  fitted(st): the refitted shape the classification tests
//   Tally                      per-inlier accumulation of the classification beside count and Q (MsacNoTally: none)
//   Row                        row(aux, ldaux, rowb, i): what the init kernel does per row beside the alive byte, from the shape's
//                              per-row input [3][ldaux] into its row bytes (MsacNoRow: nothing)
#pragma once
#include "common.hpp"
#include "knn_walk.hpp"                              // finite3
#include "chunk_scan.hpp"
#include "wave_math.hpp"                             // splitmix64, i128_to_double
#include <cmath>

namespace pcreg {
namespace {

constexpr int kMsacMaxM = 1 << 26;                   // below it no refit sum overflows (each shape states its bounds)
constexpr int kMsacMaxShapes = 64;
constexpr int kMsacMaxTrials = 1 << 20;
constexpr int kMsacBlock = 256;
constexpr int kMsacChunk = kScanChunk;               // alive rows per scoring workgroup
constexpr int kMsacQMax = 1 << 20;

struct MsacHead {
    unsigned box[6];                                 // lo x y z, hi x y z of the finite rows as order-preserving words
    int done, nA;
    int best_b, best_count;
    long long best_cost;
    unsigned long long tot[kMsacMaxShapes][2];       // per round: count_p, Q_p
};
// the outputs every shape has (device pointers; labels, counts, rmse are required where M > 0, the diagnostics may be null)
struct MsacOut {
    int32_t* labels; int32_t* counts; double* rmse; int32_t* n_shapes; int32_t* best_trial; long long* best_cost; int32_t* best_count;
};
struct MsacNoHook { __device__ void operator()(long long) const {} };
struct MsacNoRow { static __device__ __forceinline__ void row(const float*, int, uint8_t*, long long) {} };
struct MsacNoTally {
    template <class Trial> __device__ void add(float, float, float, const Trial&) {}
    __device__ void wave() {}
    __device__ void stage() {}
    template <class State> __device__ void commit(State*, int) {}
};

// a float as a word whose unsigned order is the float's, and back
__device__ __forceinline__ unsigned ord_of(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_back(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
// frexp's exponent of the largest axis extent of the finite rows (0 where there is none or it is zero)
__device__ __forceinline__ int msac_exponent(const MsacHead* __restrict__ st) {
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
__device__ __forceinline__ int msac_q(float r2, float s) {   // min(2^20, rint(r2 s)); rint is monotone, so the cap may come first
    return (int)rintf(fminf(r2 * s, (float)kMsacQMax));
}
__device__ __forceinline__ bool msac_finite(double v) { return v - v == 0.0; }
__device__ __forceinline__ bool msac_finitef(float v) { return v - v == 0.0f; }

// N signed 64-bit sums of a workgroup: the waves by shuffles, the four waves through LDS, N atomics a workgroup (none where the
// workgroup counted nothing: a[0] is the count)
template <int N>
__device__ __forceinline__ void msac_block_sums(long long (&a)[N], long long* __restrict__ dst) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < N; ++c) a[c] += __shfl_xor(a[c], o);
    }
    __shared__ long long sw[kMsacBlock / 64][N];
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

// ---- Z, I. reset and the alive rows ----------------------------------------------------------------------------------------------
// the body of a shape's reset kernel (one workgroup): the whole state to zero, the empty box, the common outputs to zero.  Ends
// behind a barrier's zeroing, so the caller may go on to write its own state words
template <class State>
__device__ __forceinline__ void msac_reset(State* __restrict__ st, int P, const MsacOut& o) {
    const int tid = threadIdx.x;
    unsigned* w = (unsigned*)st;
    for (int i = tid; i < (int)(sizeof(State) / 4); i += kMsacBlock) w[i] = 0u;
    __syncthreads();
    if (tid < 3) { st->head.box[tid] = 0xFFFFFFFFu; st->head.box[3 + tid] = 0u; }
    for (int i = tid; i < P; i += kMsacBlock) {
        if (o.counts) o.counts[i] = 0;
        if (o.rmse) o.rmse[i] = 0.0;
        if (o.best_trial) o.best_trial[i] = 0;
        if (o.best_cost) o.best_cost[i] = 0;
        if (o.best_count) o.best_count[i] = 0;
    }
    if (tid == 0 && o.n_shapes) *o.n_shapes = 0;
}

// (aux and rowb are kernel arguments, not members of a hook object, so that they are __restrict__ like every other array here)
template <class Row>
__global__ __launch_bounds__(kMsacBlock) void msac_init_kernel(const float* __restrict__ m, int M, int ldm, MsacHead* __restrict__ st,
                                                               uint8_t* __restrict__ alive, int32_t* __restrict__ labels,
                                                               const float* __restrict__ aux, int ldaux, uint8_t* __restrict__ rowb) {
    __shared__ unsigned s[kMsacBlock / 64][6];
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (int j = 0; j < kMsacChunk / kMsacBlock; ++j) {           // 2048 rows a workgroup: six atomics per 2048 rows
        const long long i = (long long)blockIdx.x * kMsacChunk + (long long)j * kMsacBlock + threadIdx.x;
        if (i < M) {
            const float x = m[i], y = m[i + (size_t)ldm], z = m[i + 2 * (size_t)ldm];
            const bool fin = finite3(x, y, z);
            alive[i] = fin ? 1 : 0;
            Row::row(aux, ldaux, rowb, i);
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
        for (int w = 1; w < kMsacBlock / 64; ++w) v = c < 3 ? min(v, s[w][c]) : max(v, s[w][c]);
        if (c < 3) { if (v != 0xFFFFFFFFu) atomicMin(&st->box[c], v); }
        else if (v != 0u) atomicMax(&st->box[c], v);
    }
}

// ---- A1, A2. the alive list (chunk_scan.hpp's predicate compaction over the original rows) ------------------------------------------
__global__ __launch_bounds__(kScanBlock) void msac_count_kernel(const MsacHead* __restrict__ st, const uint8_t* __restrict__ alive, int M,
                                                                int32_t* __restrict__ pin) {
    if (st->done) return;
    chunk_pred_count(M, pin, [&](long long i) { return alive[i] != 0; });
}
__global__ __launch_bounds__(kScanBlock) void msac_list_kernel(MsacHead* __restrict__ st, const uint8_t* __restrict__ alive,
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

// ---- H. the sample rows of trial b of round p ------------------------------------------------------------------------------------------
// From the table (K entries a trial, each in range and alive) or by the hash over the alive list; false where they are not K
// distinct usable rows.  The hash index steps by FOUR a trial whatever K is: the published draw (include/pcreg.h)
template <int K>
__device__ __forceinline__ bool msac_draw(const MsacHead* __restrict__ st, int p, int B, int b, unsigned long long seed,
                                          const int32_t* __restrict__ samples, int idx_base, const uint8_t* __restrict__ alive,
                                          const int32_t* __restrict__ A, int M, long long (&idx)[K]) {
    const int nA = st->nA;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < K; ++j) idx[j] = 0;
    if (samples) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            idx[j] = (long long)samples[((size_t)p * (size_t)B + (size_t)b) * K + j] - (long long)idx_base;
            if (idx[j] < 0 || idx[j] >= M) ok = false;
            else if (!alive[idx[j]]) ok = false;
        }
    } else if (nA > 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const unsigned long long h =
                splitmix64(seed ^ splitmix64(((unsigned long long)p * (unsigned long long)B + (unsigned long long)b) * 4ull + j));
            idx[j] = A[h % (unsigned long long)nA];
        }
    } else ok = false;
#pragma unroll
    for (int i = 0; i < K; ++i) {
#pragma unroll
        for (int j = i + 1; j < K; ++j) if (idx[i] == idx[j]) ok = false;
    }
    return ok;
}

// ---- S. the scoring: B x nA evaluations ------------------------------------------------------------------------------------------------
// blockIdx.x = chunk of kMsacChunk alive rows, blockIdx.y = 256 trials.  The rows sit in LDS as three arrays; a lane reads four rows
// of an array with one 16-byte load whose address is the same in every lane.  Rows past nA are staged as NaN: they pass no test.  Per
// chunk the inliers' q add up to at most 2048 2^20 = 2^31, inside an unsigned word; the others' 2^20 are added by their number.
// Lanes b >= B of the last trial block walk trial B - 1 and add nothing.
template <class Shape>
__global__ __launch_bounds__(kMsacBlock) void msac_score_kernel(const MsacHead* __restrict__ st, const float* __restrict__ cx,
                                                                const float* __restrict__ cy, const float* __restrict__ cz,
                                                                const float* __restrict__ hp0, const float* __restrict__ par, int B,
                                                                float t2, float s, unsigned long long* __restrict__ cost,
                                                                int32_t* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) float sx[kMsacChunk];
    __shared__ __attribute__((aligned(16))) float sy[kMsacChunk];
    __shared__ __attribute__((aligned(16))) float sz[kMsacChunk];
    if (st->done) return;
    const int nA = st->nA;
    const long long r0 = (long long)blockIdx.x * kMsacChunk;
    if (r0 >= nA) return;
    const int nrow = (int)min((long long)kMsacChunk, (long long)nA - r0);
    const int tid = threadIdx.x;
    const float qnan = __uint_as_float(0x7FC00000u);
    for (int i = tid; i < kMsacChunk; i += kMsacBlock) {
        const bool in = i < nrow;
        sx[i] = in ? cx[r0 + i] : qnan; sy[i] = in ? cy[r0 + i] : qnan; sz[i] = in ? cz[r0 + i] : qnan;
    }
    __syncthreads();
    const int b = blockIdx.y * kMsacBlock + tid;
    const int bb = min(b, B - 1);
    const typename Shape::Trial tr = Shape::load(hp0, par, (size_t)B, bb);
    unsigned qs = 0u;
    int cnt = 0;
    const int n4 = (nrow + 3) & ~3;
    for (int i = 0; i < n4; i += 4) {
        const float4 X = *(const float4*)&sx[i], Y = *(const float4*)&sy[i], Z = *(const float4*)&sz[i];
        const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float r2 = Shape::r2(xs[u], ys[u], zs[u], tr);
            const bool in = r2 <= t2;
            qs += in ? (unsigned)msac_q(r2, s) : 0u;
            cnt += in ? 1 : 0;
        }
    }
    if (b < B) {
        atomicAdd(&cost[b], (unsigned long long)qs + ((unsigned long long)(nrow - cnt) << 20));
        atomicAdd(&count[b], cnt);
    }
}

// ---- B. the best trial ------------------------------------------------------------------------------------------------------------------
template <class Shape>
__global__ __launch_bounds__(kMsacBlock) void msac_select_kernel(typename Shape::State* __restrict__ st, int p, int B, int min_inliers,
                                                                 const uint8_t* __restrict__ hvoid,
                                                                 const unsigned long long* __restrict__ cost,
                                                                 const int32_t* __restrict__ count, const float* __restrict__ hp0,
                                                                 const float* __restrict__ par, int32_t* __restrict__ best_trial,
                                                                 long long* __restrict__ best_cost, int32_t* __restrict__ best_count) {
    __shared__ unsigned long long sc[kMsacBlock];
    __shared__ int sb[kMsacBlock];
    if (st->head.done) return;
    const int tid = threadIdx.x;
    unsigned long long c = ~0ull;
    int bi = -1;
    for (int b = tid; b < B; b += kMsacBlock) {            // ascending b per thread: the first of equal costs stays
        if (!hvoid[b] && count[b] >= Shape::kMinCount && cost[b] < c) { c = cost[b]; bi = b; }
    }
    sc[tid] = c; sb[tid] = bi;
    __syncthreads();
    for (int o = kMsacBlock / 2; o > 0; o >>= 1) {
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
        st->head.best_b = b; st->head.best_count = n; st->head.best_cost = cb;
        if (b < 0 || n < min_inliers) st->head.done = 1;
        else Shape::keep(st, hp0, par, (size_t)B, b);
    }
}

// ---- C, F. the classification ------------------------------------------------------------------------------------------------------------
// A workgroup that labelled nothing returns after its barrier (every thread reads the same LDS words) and issues no atomic
template <class Shape>
__global__ __launch_bounds__(kMsacBlock) void msac_classify_kernel(typename Shape::State* __restrict__ st, int p,
                                                                   const int32_t* __restrict__ A, const float* __restrict__ cx,
                                                                   const float* __restrict__ cy, const float* __restrict__ cz, float t2,
                                                                   float s, uint8_t* __restrict__ alive, int32_t* __restrict__ labels) {
    if (st->head.done) return;
    const int nA = st->head.nA;
    const long long k0 = (long long)blockIdx.x * kMsacChunk;
    if (k0 >= nA) return;
    const typename Shape::Trial c = Shape::fitted(st);
    unsigned long long q = 0ull;
    int cnt = 0;
    typename Shape::Tally tally;
    for (int j = 0; j < kMsacChunk / kMsacBlock; ++j) {
        const long long k = k0 + (long long)j * kMsacBlock + threadIdx.x;
        if (k < nA) {
            const float x = cx[k], y = cy[k], z = cz[k];
            const float r2 = Shape::r2(x, y, z, c);
            if (r2 <= t2) {
                const int row = A[k];
                labels[row] = p + 1;
                alive[row] = 0;
                q += (unsigned long long)msac_q(r2, s);
                ++cnt;
                tally.add(x, y, z, c);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { q += __shfl_xor(q, o); cnt += __shfl_xor(cnt, o); }
    tally.wave();
    __shared__ unsigned long long sw[kMsacBlock / 64][2];
    if ((threadIdx.x & 63) == 0) { sw[threadIdx.x >> 6][0] = (unsigned long long)cnt; sw[threadIdx.x >> 6][1] = q; }
    tally.stage();
    __syncthreads();
    if (sw[0][0] + sw[1][0] + sw[2][0] + sw[3][0] == 0ull) return;
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        atomicAdd(&st->head.tot[p][k], sw[0][k] + sw[1][k] + sw[2][k] + sw[3][k]);
    } else tally.commit(st, p);
}

template <class FinishHook>
__global__ void msac_finish_kernel(const MsacHead* __restrict__ st, int p, float t2, int32_t* __restrict__ counts,
                                   double* __restrict__ rmse, int32_t* __restrict__ n_shapes, FinishHook fin) {
    if (st->done) return;
    const unsigned long long n = st->tot[p][0], Q = st->tot[p][1];
    counts[p] = (int32_t)n;
    rmse[p] = sqrt(((double)Q / (double)n) * ((double)t2 * 9.5367431640625e-07));      // 2^-20
    fin(p);
    *n_shapes = p + 1;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------
// Workspace, with R = max(M, 1), C = max(ceil(M / 2048), 1) and T = B: [state, roundup(sizeof, 256)][alive bytes, R][the shape's
// row bytes, R, where it has them][chunk counts, C int32][alive rows, R int32][their x, y, z, R floats each][p0, 3 T floats]
// [parameters, kParams T floats][void bytes, T][cost, T uint64][count, T int32], every slot rounded up to 256 bytes
template <class Shape>
struct MsacWs {
    typename Shape::State* st; uint8_t *alive, *rowb; int32_t* pin; int32_t* A; float *cx, *cy, *cz; float *hp0, *par; uint8_t* hvoid;
    unsigned long long* cost; int32_t* count; int n_chunks;
};
template <class Shape>
MsacWs<Shape> msac_ws_layout(int M, int B, void* base, size_t* bytes) {
    MsacWs<Shape> s{};
    WsWalk w(base);
    const size_t R = (size_t)(M > 0 ? M : 1), T = (size_t)(B > 0 ? B : 1);
    s.n_chunks = (int)((R + kScanChunk - 1) / kScanChunk);
    s.st = w.take<typename Shape::State>(1);
    s.alive = w.take<uint8_t>(R);
    if (Shape::kRowBytes) s.rowb = w.take<uint8_t>(R);
    s.pin = w.take<int32_t>((size_t)s.n_chunks);
    s.A = w.take<int32_t>(R);
    s.cx = w.take<float>(R); s.cy = w.take<float>(R); s.cz = w.take<float>(R);
    s.hp0 = w.take<float>(3 * T); s.par = w.take<float>((size_t)Shape::kParams * T);
    s.hvoid = w.take<uint8_t>(T);
    s.cost = w.take<unsigned long long>(T);
    s.count = w.take<int32_t>(T);
    *bytes = w.bytes();
    return s;
}

inline bool msac_args_ok(float max_distance, int max_shapes, int n_trials, int min_inliers, int min_count) {
    if (!(std::isnormal(max_distance) && max_distance > 0.0f)) return false;
    const float t2 = max_distance * max_distance;
    if (!(std::isnormal(t2))) return false;                      // (the square is the threshold: it must be a normal float too)
    return max_shapes >= 1 && max_shapes <= kMsacMaxShapes && n_trials >= 1 && n_trials <= kMsacMaxTrials && min_inliers >= min_count;
}
inline bool msac_radii_ok(float min_radius, float max_radius) {  // (a NaN fails; max_radius may be +inf)
    return min_radius >= 0.0f && min_radius <= max_radius;
}
inline bool msac_ref_ok(const double* ref_vec, double max_angle) {
    if (!ref_vec) return true;
    for (int c = 0; c < 3; ++c) if (!std::isfinite(ref_vec[c])) return false;
    const double l2 = (ref_vec[0] * ref_vec[0] + ref_vec[1] * ref_vec[1]) + ref_vec[2] * ref_vec[2];
    if (!(l2 > 0.0) || !std::isfinite(l2)) return false;
    return max_angle > 0.0 && max_angle <= 1.5707963267948966;
}
// the reference vector as the kernels take it: its length, and the cosine a trial's direction must reach
struct MsacRef { int use; double x, y, z, len, cos_max; };
inline MsacRef msac_ref(const double* ref_vec, double max_angle) {
    if (!ref_vec) return MsacRef{0, 0.0, 0.0, 0.0, 1.0, 0.0};
    const double rx = ref_vec[0], ry = ref_vec[1], rz = ref_vec[2];
    return MsacRef{1, rx, ry, rz, std::sqrt((rx * rx + ry * ry) + rz * rz), std::cos(max_angle)};
}

inline dim3 msac_chunk_grid(int n_chunks) { return dim3((unsigned)n_chunks); }
inline dim3 msac_trial_grid(int B) { return dim3((unsigned)((B + kMsacBlock - 1) / kMsacBlock)); }

// Everything behind the reset: I, and P rounds of A1 A2 H S B (refit) C F.  hyp(p, t2) launches the shape's hypothesis kernel and
// refit(p, t2) its refit stage; aux [3][ldaux] is the per-row input of Shape::Row (or null), fin the device hook of F
template <class Shape, class FinishHook, class Hyp, class Refit>
void msac_launch_rounds(const MsacWs<Shape>& s, const ModelView& v, float max_distance, int P, int B, int min_inliers, const MsacOut& o,
                        const float* aux, int ldaux, FinishHook fin, Hyp hyp, Refit refit, hipStream_t stream) {
    const int M = v.M;
    const float t2 = max_distance * max_distance;
    const float sc = (float)(1048576.0 / (double)t2);
    MsacHead* head = &s.st->head;
    const dim3 cgrid = msac_chunk_grid(s.n_chunks), cblock(kScanBlock), block(kMsacBlock);
    const dim3 sgrid((unsigned)s.n_chunks, msac_trial_grid(B).x);
    hipLaunchKernelGGL(msac_init_kernel<typename Shape::Row>, cgrid, block, 0, stream, v.m, M, v.ldm, head, s.alive, o.labels, aux, ldaux,
                       s.rowb);
    for (int p = 0; p < P; ++p) {
        hipLaunchKernelGGL(msac_count_kernel, cgrid, cblock, 0, stream, (const MsacHead*)head, (const uint8_t*)s.alive, M, s.pin);
        hipLaunchKernelGGL(msac_list_kernel, cgrid, cblock, 0, stream, head, (const uint8_t*)s.alive, v.m, M, v.ldm, (const int32_t*)s.pin,
                           s.A, s.cx, s.cy, s.cz);
        hyp(p, t2);
        hipLaunchKernelGGL(msac_score_kernel<Shape>, sgrid, block, 0, stream, (const MsacHead*)head, (const float*)s.cx, (const float*)s.cy,
                           (const float*)s.cz, (const float*)s.hp0, (const float*)s.par, B, t2, sc, s.cost, s.count);
        hipLaunchKernelGGL(msac_select_kernel<Shape>, dim3(1), block, 0, stream, s.st, p, B, min_inliers, (const uint8_t*)s.hvoid,
                           (const unsigned long long*)s.cost, (const int32_t*)s.count, (const float*)s.hp0, (const float*)s.par,
                           o.best_trial, o.best_cost, o.best_count);
        refit(p, t2);
        hipLaunchKernelGGL(msac_classify_kernel<Shape>, cgrid, block, 0, stream, s.st, p, (const int32_t*)s.A, (const float*)s.cx,
                           (const float*)s.cy, (const float*)s.cz, t2, sc, s.alive, o.labels);
        hipLaunchKernelGGL(msac_finish_kernel<FinishHook>, dim3(1), dim3(1), 0, stream, (const MsacHead*)head, p, t2, o.counts, o.rmse,
                           o.n_shapes, fin);
    }
}

}  // namespace
}  // namespace pcreg
