// pcreg_amd/csrc/knn_fps.hip -- farthest point sampling of a PREPARED model: K rows, each the live row farthest from all rows chosen
// before it, the covering radius with every row, and per row its nearest sample.  The contract is pcreg_model_fps_f32's
// (include/pcreg.h); DESIGN 4.29.
//
// The prepared model (knn_fast.hip) is used as it is: the rows in spatial order (ms, perm), a box per 512-row tile (tbox) and per
// 64-row unit (ubox).  A call is two launches:
//   F1  fps_kernel           ONE workgroup of 1024 threads runs all the steps.  D (the distance of every sorted row to the sample
//                            set), L (its nearest sample) and one (max D, original row, sorted row) record per unit live in the
//                            workspace; the same record and the box of every TILE live in LDS.  A step judges every tile from LDS
//                            by the culling rule (cull_rule.hpp) against the tile's max D, then the units of the visited tiles by
//                            the same rule (a wave takes the unit records and boxes of eight visited tiles in one round of
//                            loads), updates the rows of the visited units one lane a row, four units at a time, and reduces
//                            the tile table to the next sample.
//   F2  fps_scatter_kernel   D and L from sorted to ORIGINAL row order (min_dist, label), chip-wide.
// WHY A SKIPPED TILE (UNIT) KEEPS ITS BITS: the rule certifies that every fp32 distance from the sample to a point of the box exceeds
// the record's max D, which is >= every D[i] inside.  So no d < D[i] holds, neither D nor L of any row in it changes, and the record
// stays the true maximum.  A record whose max D is +inf certifies nothing and its tile (unit) is visited.
// The steps are strictly sequential and no workgroup waits for another, so one workgroup runs them: a launch per sample would cost
// K launch latencies.  Nothing synchronises; there is no atomic on a result.
#include "knn_walk.hpp"
#include <climits>
#include <cmath>

namespace pcreg {

namespace {

constexpr int kFpsBlock = 1024;                           // ONE workgroup: 16 waves
constexpr int kFpsWaves = kFpsBlock / 64;
constexpr int kFpsUnits = kT16 / 64;                      // units per tile
constexpr int kFpsMaxTiles = 4096;                        // the LDS tile table: 36 bytes a tile, 144 KiB of the CU's 160
constexpr int kFpsMaxRows = kFpsMaxTiles * kT16;          // 2^21 rows
constexpr int kFpsFly = 4;                                // visited units a wave updates at a time
constexpr int kFpsLdsHead = 64 + kFpsWaves * 16;          // FpsCtl, then one record per wave
static_assert(kFpsUnits == 8 && kFpsMaxRows == (1 << 21), "a wave judges the units of eight tiles in one ballot; the documented cap");
static_assert(kFpsLdsHead + 36 * kFpsMaxTiles <= 160 * 1024, "the tile table fits the CU's LDS");

// (max D, original row, sorted row) of a unit, a tile, a wave's tiles or the model.  The order: larger D first, then the LOWER
// original row.  Original rows are distinct, so the order is total on live records; a record without a live row is kFpsNone
// for every lane alike.
struct FpsRec { float d; int32_t orow; int32_t srow; };
#define kFpsNone (FpsRec{-1.0f, INT_MAX, 0})
__device__ __forceinline__ bool fps_better(const FpsRec& a, const FpsRec& b) { return a.d > b.d || (a.d == b.d && a.orow < b.orow); }
// the best record of a wave, in every lane (a butterfly over a total order: every lane ends with the same record)
__device__ __forceinline__ FpsRec fps_wave_best(FpsRec v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const FpsRec w{__shfl_xor(v.d, o), __shfl_xor(v.orow, o), __shfl_xor(v.srow, o)};
        if (fps_better(w, v)) v = w;
    }
    return v;
}

// what every thread reads after a barrier: the sample of the step about to run (mx = the D it was chosen with) and the prologue's verdict
struct FpsCtl { float mx; int32_t orow, srow; float x, y, z; int32_t mode; };
enum { kFpsRefused = 0, kFpsRun = 1, kFpsEmpty = 2 };     // (also the workspace word F2 reads)

// is the box visited for the sample s?  rec.d < 0: no live row inside, nothing to measure.
__device__ __forceinline__ bool fps_visits(const float* box, const float (&s)[3], float mx, int cull) {
    return mx >= 0.0f && !(cull != 0 && mx < INFINITY && cull_skips(cull_gap2(box, box + 3, s, s), mx));
}

struct FpsRow { float x, y, z, D; int32_t o; };

__global__ __launch_bounds__(kFpsBlock) void fps_kernel(const float* __restrict__ ms, const int32_t* __restrict__ perm, int M,
                                                        const float* __restrict__ tbox, const float* __restrict__ ubox, int n_tiles, int K,
                                                        int start, float stop_d2, int cull, int32_t* __restrict__ idx,
                                                        float* __restrict__ dist, int32_t* __restrict__ n_out, float* __restrict__ cover_d2,
                                                        int32_t* __restrict__ info, float* __restrict__ D, int32_t* __restrict__ L,
                                                        int4* __restrict__ urec, int32_t* __restrict__ flag,
                                                        unsigned long long* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    FpsCtl* ctl = (FpsCtl*)smem;
    FpsRec* s_wave = (FpsRec*)(smem + 64);
    float* t_d = (float*)(smem + kFpsLdsHead);
    int32_t* t_orow = (int32_t*)t_d + n_tiles;
    int32_t* t_srow = t_orow + n_tiles;
    float* t_box = (float*)(t_srow + n_tiles);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float qnan = __int_as_float(0x7FC00000);

    // ---- the prologue: K = 0 or M = 0 (kernel arguments: uniform) ends here; else the start row's place in the sorted order ----
    if (K == 0 || M == 0) {
        if (tid == 0) {
            *n_out = 0; *flag = kFpsEmpty;
            if (cover_d2) *cover_d2 = qnan;
            if (info) *info = 0;
        }
        return;
    }
    for (int t = tid; t < n_tiles * 6; t += kFpsBlock) t_box[t] = tbox[t];
    {
        // start >= 0: the sorted row whose original row it is; start = -1: the lowest live original row
        int bo = INT_MAX, bs = 0;
        for (int r = tid; r < M; r += kFpsBlock) {
            const int o = perm[r];
            const bool cand = start >= 0 ? o == start : finite3(ms[r], ms[r + (size_t)M], ms[r + 2 * (size_t)M]);
            if (cand && o < bo) { bo = o; bs = r; }
        }
        FpsRec b = fps_wave_best(FpsRec{bo < INT_MAX ? 0.0f : -1.0f, bo, bs});
        if (lane == 0) s_wave[wave] = b;
        __syncthreads();
        if (wave == 0) {
            b = fps_wave_best(s_wave[lane & (kFpsWaves - 1)]);
            if (lane == 0) {
                const float x = ms[b.srow], y = ms[b.srow + (size_t)M], z = ms[b.srow + 2 * (size_t)M];
                ctl->mx = INFINITY; ctl->orow = b.orow; ctl->srow = b.srow; ctl->x = x; ctl->y = y; ctl->z = z;
                ctl->mode = b.d < 0.0f ? (start >= 0 ? kFpsRefused : kFpsEmpty) : finite3(x, y, z) ? kFpsRun : kFpsRefused;
            }
        }
        __syncthreads();
    }
    const int mode = ctl->mode;                                   // one LDS word behind a barrier: uniform
    if (mode != kFpsRun) {
        if (tid == 0) {
            *n_out = 0; *flag = mode;
            if (mode == kFpsEmpty && cover_d2) *cover_d2 = qnan;  // no live row
            if (info) *info = mode == kFpsEmpty ? 0 : 1;          // a dead start row: nothing else is written
        }
        return;
    }

    // this lane's row of unit u: the loads of one trip, issued together
    auto load_row = [&](int u, bool first) {
        FpsRow p{qnan, qnan, qnan, INFINITY, -1};
        const int r = u * 64 + lane;
        if (r < M) {
            p.x = ms[r]; p.y = ms[r + (size_t)M]; p.z = ms[r + 2 * (size_t)M]; p.o = perm[r];
            if (!first) p.D = D[r];
        }
        return p;
    };

    // ---- the steps.  WORKGROUP UNIFORMITY: every thread runs the same number of trips of this loop and meets the same two barriers a
    // trip.  The loop has ONE exit, below its second barrier, taken on j, K and stop_d2 (kernel arguments and a counter every thread
    // advances alike) and on ctl->mx, one LDS word that wave 0 wrote before that barrier; the sample is read from ctl in the same way.
    // Between the barriers control flow differs by WAVE only (which tiles and units it visits: ballots, so uniform inside a wave) and
    // holds no barrier.  ctl is written between barrier 1 and 2 and read behind barrier 2 (and at the loop's head, before the next
    // barrier 1); s_wave is written before barrier 1 and read between 1 and 2: no word is written while another thread may read it.
    unsigned long long touched = 0;
    int j = 0;
    for (;;) {
        const float s[3] = {ctl->x, ctl->y, ctl->z};
        const bool first = j == 0;                                // the first step visits everything and reads no D
        if (tid == 0) {
            if (idx) idx[j] = ctl->orow;
            if (dist) dist[j] = ctl->mx;
        }
        FpsRec best = kFpsNone;
        // wave w owns tiles w, w + 16, ...: neighbours in the spatial order go to different waves.  Lane l judges tile t0 + 16 l + w.
        for (int t0 = 0; t0 < n_tiles; t0 += kFpsBlock) {
            const int t = t0 + lane * kFpsWaves + wave;
            FpsRec trec = kFpsNone;
            bool tv = false;
            if (t < n_tiles) {
                if (first) tv = true;
                else {
                    trec = FpsRec{t_d[t], t_orow[t], t_srow[t]};
                    tv = fps_visits(t_box + (size_t)t * 6, s, trec.d, cull);
                }
            }
            if (!tv && fps_better(trec, best)) best = trec;       // a visited tile's record is formed anew below
            unsigned long long tbal = __builtin_amdgcn_ballot_w64(tv);
            while (tbal) {                                        // (wave-uniform)
                // up to EIGHT visited tiles a trip: lane (k, u) = (lane >> 3, lane & 7) judges unit u of the k-th of them, so the unit
                // records and boxes of all eight are one round of loads
                int myb = -1;
#pragma unroll
                for (int k = 0; k < 64 / kFpsUnits; ++k) {
                    if (tbal) {
                        const int tb = (int)__ffsll((long long)tbal) - 1;
                        tbal &= tbal - 1;
                        if ((lane >> 3) == k) myb = tb;
                    }
                }
                const int vt = myb >= 0 ? t0 + myb * kFpsWaves + wave : -1;
                const int gu = vt * kFpsUnits + (lane & (kFpsUnits - 1));       // this lane's unit, model-wide
                FpsRec ur = kFpsNone;
                bool uv = false;
                if (vt >= 0) {
                    if (first) uv = true;
                    else {
                        const int4 raw = urec[gu];
                        ur = FpsRec{__int_as_float(raw.x), raw.y, raw.z};
                        uv = fps_visits(ubox + (size_t)gu * 6, s, ur.d, cull);
                    }
                }
                unsigned long long ubal = __builtin_amdgcn_ballot_w64(uv);
                // kFpsFly visited units a trip: their loads are in flight together and their reductions interleave
                while (ubal) {                                    // (wave-uniform)
                    int p[kFpsFly], u[kFpsFly];                   // the lane that judged the unit; the unit, model-wide
                    FpsRow row[kFpsFly] = {};
#pragma unroll
                    for (int q = 0; q < kFpsFly; ++q) {
                        p[q] = u[q] = -1;
                        if (ubal) {
                            p[q] = (int)__ffsll((long long)ubal) - 1;
                            ubal &= ubal - 1;
                            u[q] = __shfl(gu, p[q]);
                            row[q] = load_row(u[q], first);
                        }
                    }
                    FpsRec me[kFpsFly];
#pragma unroll
                    for (int q = 0; q < kFpsFly; ++q) {
                        me[q] = kFpsNone;
                        const int r = u[q] * 64 + lane;
                        if (u[q] >= 0 && r < M) {
                            const FpsRow& c = row[q];
                            const bool live = finite3(c.x, c.y, c.z);
                            const float d = point_d2(c.x, c.y, c.z, s[0], s[1], s[2]);
                            float Dn = c.D;
                            if (first) {
                                const bool lt = live && d < INFINITY;
                                D[r] = live ? d : qnan;           // (d is +inf when it is not below +inf)
                                L[r] = lt ? 1 : 0;
                                Dn = d;
                            } else if (live && d < c.D) {
                                D[r] = d; L[r] = j + 1;
                                Dn = d;
                            }
                            if (live) { me[q] = FpsRec{Dn, c.o, r}; ++touched; }
                        }
                    }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
                        for (int q = 0; q < kFpsFly; ++q) {
                            const FpsRec w{__shfl_xor(me[q].d, o), __shfl_xor(me[q].orow, o), __shfl_xor(me[q].srow, o)};
                            if (fps_better(w, me[q])) me[q] = w;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < kFpsFly; ++q) {
                        if (u[q] >= 0) {
                            if (lane == p[q]) ur = me[q];
                            if (lane == 0) urec[u[q]] = make_int4(__float_as_int(me[q].d), me[q].orow, me[q].srow, 0);
                        }
                    }
                }
                // the tiles' records anew from their eight unit records: a butterfly inside each group of eight lanes
                FpsRec nt = ur;
#pragma unroll
                for (int o = 1; o < kFpsUnits; o <<= 1) {
                    const FpsRec w{__shfl_xor(nt.d, o), __shfl_xor(nt.orow, o), __shfl_xor(nt.srow, o)};
                    if (fps_better(w, nt)) nt = w;
                }
                if (vt >= 0 && (lane & (kFpsUnits - 1)) == 0) {
                    t_d[vt] = nt.d; t_orow[vt] = nt.orow; t_srow[vt] = nt.srow;
                    if (fps_better(nt, best)) best = nt;
                }
            }
        }
        best = fps_wave_best(best);
        if (lane == 0) s_wave[wave] = best;
        __syncthreads();                                          // barrier 1
        if (wave == 0) {
            const FpsRec g = fps_wave_best(s_wave[lane & (kFpsWaves - 1)]);
            if (lane == 0) {
                ctl->mx = g.d; ctl->orow = g.orow; ctl->srow = g.srow;
                ctl->x = ms[g.srow]; ctl->y = ms[g.srow + (size_t)M]; ctl->z = ms[g.srow + 2 * (size_t)M];
            }
        }
        __syncthreads();                                          // barrier 2
        ++j;
        if (j == K || !(ctl->mx > stop_d2)) break;
    }
    if (tid == 0) {
        *n_out = j; *flag = kFpsRun;
        if (cover_d2) *cover_d2 = ctl->mx;
        if (info) *info = 0;
    }
    if (stats) {                                                  // "knn_stats": [0] steps, [1] rows measured
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) touched += __shfl_xor(touched, o);
        if (lane == 0) atomicAdd(&stats[1], touched);
        if (tid == 0) atomicAdd(&stats[0], (unsigned long long)j);
    }
}

// F2: by original row.  flag: kFpsRefused writes nothing, kFpsEmpty (no step ran) NaN and 0
__global__ __launch_bounds__(kBlock) void fps_scatter_kernel(const int32_t* __restrict__ perm, int M, const float* __restrict__ D,
                                                             const int32_t* __restrict__ L, const int32_t* __restrict__ flag,
                                                             float* __restrict__ min_dist, int32_t* __restrict__ label) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= M) return;
    const int f = *flag;
    if (f == kFpsRefused) return;
    const int o = perm[r];
    if (min_dist) min_dist[o] = f == kFpsRun ? D[r] : __int_as_float(0x7FC00000);
    if (label) label[o] = f == kFpsRun ? L[r] : 0;
}

// Workspace, with R = max(M, 1) and U = 8 max(ceil(M / 512), 1): [D of every sorted row, R floats][L, R int32][unit records, U of 16
// bytes][the word F2 reads: 256 bytes]: 2 roundup(4 R, 256) + roundup(16 U, 256) + 256 bytes, whatever K
struct FpsWs { float* D; int32_t* L; int4* urec; int32_t* flag; };
FpsWs fps_ws_layout(int M, void* base, size_t* bytes) {
    FpsWs s{};
    WsWalk w(base);
    const size_t R = (size_t)(M > 0 ? M : 1);
    const size_t U = (size_t)kFpsUnits * std::max<size_t>((R + kT16 - 1) / kT16, 1);
    s.D = w.take<float>(R);
    s.L = w.take<int32_t>(R);
    s.urec = w.take<int4>(U);
    s.flag = (int32_t*)w.take_bytes(256);
    *bytes = w.bytes();
    return s;
}

}  // namespace

int fps_max_rows() { return kFpsMaxRows; }
bool fps_args_ok(int M, int K, int start, float stop_d2) {
    return K >= 0 && M >= 0 && M <= kFpsMaxRows && (M == 0 || (start >= -1 && start < M)) && stop_d2 >= 0.0f;      // (a NaN fails)
}
size_t fps_ws_bytes(int M, int K) {
    (void)K;                                                      // the outputs are the caller's
    if (M < 0 || M > kFpsMaxRows) return 0;
    size_t b; (void)fps_ws_layout(M, nullptr, &b);
    return b;
}

int launch_model_fps(const ModelView& v, int K, int start, float stop_d2, int32_t* idx, float* dist, int32_t* n_out, float* cover_d2,
                     float* min_dist, int32_t* label, int32_t* info, void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(n_out != nullptr && fps_args_ok(v.M, K, start, stop_d2));
    size_t need;
    const FpsWs s = fps_ws_layout(v.M, ws, &need);
    if (ws_bytes < need) { set_error("bad argument: fps workspace too small: %zu < %zu", ws_bytes, need); return PCREG_E_ARG; }
    const int M = v.M;
    const int n_tiles = (M + kT16 - 1) / kT16;
    const int cull = debug_flag(kDbgKnnNoCull) ? 0 : 1;          // "knn_nocull": visit every tile and unit, same bits
    static bool attr_set = false;
    if (!attr_set) {
        PCREG_HIP(hipFuncSetAttribute((const void*)fps_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kFpsLdsHead + 36 * kFpsMaxTiles));
        attr_set = true;
    }
    const size_t lds = (size_t)kFpsLdsHead + 36 * (size_t)n_tiles;
    hipLaunchKernelGGL(fps_kernel, dim3(1), dim3(kFpsBlock), lds, st, (const float*)v.ms, (const int32_t*)v.perm, M, (const float*)v.tbox,
                       (const float*)v.ubox, n_tiles, K, start, stop_d2, cull, idx, dist, n_out, cover_d2, info, s.D, s.L, s.urec, s.flag,
                       fps_stats_dev());
    if (M > 0 && (min_dist || label))
        hipLaunchKernelGGL(fps_scatter_kernel, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (const int32_t*)v.perm, M,
                           (const float*)s.D, (const int32_t*)s.L, (const int32_t*)s.flag, min_dist, label);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
