// pcreg_amd/csrc/api.hip -- the C ABI of libpcreg_hip.so (include/pcreg.h).
//
// Host tier: stage the caller's MATLAB-layout host arrays into HBM, enqueue the
// kernels on the library stream, copy the results back.  Device tier: thin argument
// checks around the launchers.  There is deliberately no CPU fallback anywhere in
// this file: without a gfx950 device every compute entry point fails with
// PCREG_E_NODEVICE.
#include "common.hpp"
#include <atomic>
#include <cstdarg>
#include <cmath>
#include <mutex>
#include <algorithm>
#include <functional>
#include <initializer_list>
#include <vector>

namespace pcreg {

static thread_local char g_err[512] = "no error";
void set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

constexpr int kKnnMaxK = PCREG_KNN_MAX_K;        // (named here so that no argument message spells the macro)
constexpr int kKnnMaxQ = 4 << 20;                  // queries per k-nearest call: the top-2 search's limit
constexpr int kRangeMaxQ = 4 << 20;                // queries per radius-search call: the same limit
constexpr int kScoreMaxQ = 4 << 20;                // queries per transform-scoring call: the same limit
static std::mutex g_mu;
static int g_device_ok = -1;          // -1 unknown, 0 ok, else error code
static hipStream_t g_stream = nullptr;

int ensure_device() {
    if (g_device_ok == 0) return PCREG_OK;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no HIP device available (%s); libpcreg_hip has no CPU fallback",
                  e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        (void)hipGetLastError();
        return PCREG_E_NODEVICE;
    }
    int dev = 0;
    PCREG_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    PCREG_HIP(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; libpcreg_hip is built for gfx950 only", dev, prop.gcnArchName);
        return PCREG_E_NODEVICE;
    }
    if (!g_stream) PCREG_HIP(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    g_device_ok = 0;
    return PCREG_OK;
}

int Scratch::get(int slot, size_t bytes, void** out) {
    if (slot < 0 || slot >= kSlots) { set_error("scratch slot %d out of range", slot); return PCREG_E_ARG; }
    if (bytes == 0) bytes = 256;
    if (size[slot] < bytes) {
        if (ptr[slot]) { PCREG_HIP(hipFree(ptr[slot])); ptr[slot] = nullptr; size[slot] = 0; }
        size_t want = align_up(bytes + bytes / 4, 4096);       // grow geometrically
        PCREG_HIP(hipMalloc(&ptr[slot], want));
        size[slot] = want;
    }
    *out = ptr[slot];
    return PCREG_OK;
}
void Scratch::release_all() {
    for (int i = 0; i < kSlots; ++i) if (ptr[i]) { (void)hipFree(ptr[i]); ptr[i] = nullptr; size[i] = 0; }
}
Scratch& scratch() { static Scratch s; return s; }

}  // namespace pcreg

using namespace pcreg;

#define GUARD()                                                     \
    std::lock_guard<std::mutex> lock__(g_mu);                       \
    do { int rc__ = ensure_device(); if (rc__) return rc__; } while (0)
#define TRY(expr) do { int rc__ = (expr); if (rc__) return rc__; } while (0)

namespace pcreg {
static std::atomic<int> g_debug[kDbgCount];
int debug_flag(DebugKey k) { return g_debug[k].load(std::memory_order_relaxed); }
// one block of device counters behind a debug key: allocated (zeroed) at the first use while the key is on
struct Counters { DebugKey key; int n; unsigned long long* dev; };
static Counters g_match_stats{kDbgMatchStats, 8, nullptr}, g_knn_stats{kDbgKnnStats, 6, nullptr}, g_ransac_stats{kDbgRansacStats, 5, nullptr},
                g_cluster_stats{kDbgClusterStats, 4, nullptr}, g_desc_stats{kDbgDescStats, 10, nullptr},
                g_knn_direct_stats{kDbgKnnDirectStats, 3, nullptr}, g_fps_stats{kDbgKnnStats, 2, nullptr};
static unsigned long long* counters_dev(Counters& c) {
    if (!debug_flag(c.key)) return nullptr;
    if (!c.dev) {
        if (hipMalloc((void**)&c.dev, c.n * sizeof(unsigned long long)) != hipSuccess) { c.dev = nullptr; return nullptr; }
        (void)hipMemset(c.dev, 0, c.n * sizeof(unsigned long long));
    }
    return c.dev;
}
// words [first, first + count) of the block (count < 0: all of it); a reset clears those words only
static int counters_read(const Counters& c, long long* out, int reset, int first = 0, int count = -1) {
    PCREG_ARG(out != nullptr);
    if (count < 0) count = c.n - first;
    for (int k = 0; k < count; ++k) out[k] = 0;
    if (!c.dev) return PCREG_OK;                               // the key was never on
    PCREG_HIP(hipDeviceSynchronize());
    unsigned long long h[8];
    PCREG_HIP(hipMemcpy(h, c.dev + first, count * sizeof h[0], hipMemcpyDeviceToHost));
    for (int k = 0; k < count; ++k) out[k] = (long long)h[k];
    if (reset) PCREG_HIP(hipMemset(c.dev + first, 0, count * sizeof h[0]));
    return PCREG_OK;
}
unsigned long long* match_stats_dev() { return counters_dev(g_match_stats); }
unsigned long long* knn_stats_dev() { return counters_dev(g_knn_stats); }
unsigned long long* ransac_stats_dev() { return counters_dev(g_ransac_stats); }
unsigned long long* cluster_stats_dev() { return counters_dev(g_cluster_stats); }
unsigned long long* desc_stats_dev() { return counters_dev(g_desc_stats); }
unsigned long long* knn_direct_stats_dev() { return counters_dev(g_knn_direct_stats); }
unsigned long long* fps_stats_dev() { return counters_dev(g_fps_stats); }
}

extern "C" {

int pcreg_debug_set(const char* key, int value) {
    static const char* const names[pcreg::kDbgCount] = {"knn_exact", "match_exact", "match_force_fallback", "ransac_fused", "ransac_nolane",
                                                        "ransac_f64score", "ransac_resident_f64", "align_times", "align_shape", "seg_debug",
                                                        "seg_batched", "seg_wave_finalize", "match_stats", "final_batch_mb", "knn_nocull",
                                                        "knn_stats", "ransac_pass2", "ransac_stats", "range_sort_cap", "cluster_noskip",
                                                        "cluster_stats", "knn_tail_cap", "score_batch_slots", "fpfh_radius_lanes", "desc_stats",
                                                        // "knn_direct": 0 (the default) answers eligible queries from their ordering-grid
                                                        // cells, 1 sends every query through the tile walk (same bits: the A/B of one
                                                        // binary).  While "knn_stats" is on every query takes the walk too: those counters
                                                        // are defined over the walk of the whole query set.  "knn_direct_stats" only counts.
                                                        // "knn_seed_fused": 0 (the default) seeds and answers directly in one launch, 1 in
                                                        // two (same bits: the A/B of one binary).
                                                        // "ransac_bhand": 0 (the default) hands the bounded second pass's long walks to
                                                        // its block-parallel finish, 1 walks every refit to its stop (same bits).
                                                        // "fgr_chain": 1 runs fast global registration's chained form whatever the size
                                                        // (same bits).
                                                        "knn_direct", "knn_direct_stats", "knn_seed_fused", "ransac_bhand", "fgr_chain"};
    PCREG_ARG(key != nullptr);
    for (int k = 0; k < pcreg::kDbgCount; ++k)
        if (!strcmp(key, names[k])) { pcreg::g_debug[k].store(value, std::memory_order_relaxed); return PCREG_OK; }
    pcreg::set_error("pcreg_debug_set: unknown key '%s'", key);
    return PCREG_E_ARG;
}

int pcreg_debug_match_stats(long long out[8], int reset) { return pcreg::counters_read(pcreg::g_match_stats, out, reset); }
int pcreg_debug_knn_stats(long long out[4], int reset) { return pcreg::counters_read(pcreg::g_knn_stats, out, reset, 0, 4); }
int pcreg_debug_knn_unit_stats(long long out[2], int reset) { return pcreg::counters_read(pcreg::g_knn_stats, out, reset, 4, 2); }
int pcreg_debug_knn_direct_stats(long long out[3], int reset) { return pcreg::counters_read(pcreg::g_knn_direct_stats, out, reset); }
int pcreg_debug_fps_stats(long long out[2], int reset) { return pcreg::counters_read(pcreg::g_fps_stats, out, reset); }
int pcreg_debug_ransac_stats(long long out[3], int reset) { return pcreg::counters_read(pcreg::g_ransac_stats, out, reset, 0, 3); }
int pcreg_debug_ransac_handover(long long out[3], int reset) {
    TRY(pcreg::counters_read(pcreg::g_ransac_stats, out, reset, 3, 2));
    out[2] = pcreg::ransac_handover_blocks();
    return PCREG_OK;
}
int pcreg_debug_cluster_stats(long long out[4], int reset) { return pcreg::counters_read(pcreg::g_cluster_stats, out, reset); }
int pcreg_debug_desc_stats(long long out[10], int reset) {     // (a read stages 8 words: the last two with a second one)
    PCREG_ARG(out != nullptr);
    TRY(pcreg::counters_read(pcreg::g_desc_stats, out, reset, 0, 8));
    return pcreg::counters_read(pcreg::g_desc_stats, out + 8, reset, 8, 2);
}

const char* pcreg_last_error(void) { return g_err; }
const char* pcreg_version(void) { return "pcreg-hip 0.1 (gfx950)"; }

int pcreg_device_count(int* count) {
    PCREG_ARG(count != nullptr);
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) { *count = 0; (void)hipGetLastError(); }
    return PCREG_OK;
}

// page-locked staging of the host tier's result lists (pairs_fetch_*) and the event their counts are waited on
static void*  g_pin[2] = {nullptr, nullptr};
static size_t g_pin_bytes[2] = {0, 0};
static hipEvent_t g_pairs_ev = nullptr;

int pcreg_set_device(int ordinal) {
    std::lock_guard<std::mutex> lock(g_mu);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { set_error("no HIP device available"); (void)hipGetLastError(); return PCREG_E_NODEVICE; }
    PCREG_ARG(ordinal >= 0 && ordinal < count);
    scratch().release_all();
    if (g_stream) { (void)hipStreamDestroy(g_stream); g_stream = nullptr; }
    if (g_pairs_ev) { (void)hipEventDestroy(g_pairs_ev); g_pairs_ev = nullptr; }
    for (int k = 0; k < 2; ++k) if (g_pin[k]) { (void)hipHostFree(g_pin[k]); g_pin[k] = nullptr; g_pin_bytes[k] = 0; }
    g_device_ok = -1;
    PCREG_HIP(hipSetDevice(ordinal));
    return ensure_device();
}

int pcreg_device_name(char* buf, int cap) {
    PCREG_ARG(buf != nullptr && cap > 0);
    GUARD();
    int dev = 0; PCREG_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop; PCREG_HIP(hipGetDeviceProperties(&prop, dev));
    snprintf(buf, (size_t)cap, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return PCREG_OK;
}

// ------------------------------------------------------------------ host tier
int pcreg_estimate_transform(const double* pts1, const double* pts2, int n, int ld, double T[16], int* empty) {
    PCREG_ARG(pts1 && pts2 && T && empty && n >= 0 && ld >= n);
    GUARD();
    for (int k = 0; k < 16; ++k) T[k] = 0.0;
    *empty = 1;
    if (n < 3) return PCREG_OK;          // rank(pts1) < 3 -> [] (estimateTransform.m:11-14)
    Stage st{scratch()};
    double *d1, *d2, *dT;
    TRY(st.take(3 * (size_t)n, &d1));
    TRY(st.take(3 * (size_t)n, &d2));
    TRY(st.take(32, &dT));                                  // T [16] | empty, 128 bytes in
    TRY(upload_cols(pts1, n, ld, 3, d1, g_stream));
    TRY(upload_cols(pts2, n, ld, 3, d2, g_stream));
    int32_t* dE = (int32_t*)(dT + 16);
    TRY(launch_estimate_transform(d1, d2, n, n, dT, dE, g_stream));
    int32_t e = 1;
    PCREG_HIP(hipMemcpyAsync(T, dT, sizeof(double) * 16, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(&e, dE, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    *empty = e;
    return PCREG_OK;
}

int pcreg_calc_dists(const double T[16], const double* pts1, const double* pts2, int n, int ld, double* d) {
    PCREG_ARG(T && pts1 && pts2 && d && n >= 0 && ld >= n);
    GUARD();
    if (n == 0) return PCREG_OK;
    Stage st{scratch()};
    double *d1, *d2, *dT, *dd;
    TRY(st.take(3 * (size_t)n, &d1));
    TRY(st.take(3 * (size_t)n, &d2));
    TRY(st.take(16, &dT));
    TRY(st.take((size_t)n, &dd));
    TRY(upload_cols(pts1, n, ld, 3, d1, g_stream));
    TRY(upload_cols(pts2, n, ld, 3, d2, g_stream));
    PCREG_HIP(hipMemcpyAsync(dT, T, sizeof(double) * 16, hipMemcpyHostToDevice, g_stream));
    TRY(launch_calc_dists(dT, d1, d2, n, n, dd, g_stream));
    PCREG_HIP(hipMemcpyAsync(d, dd, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}

static int ransac_host(const double* pts1, const double* pts2, int total, int ld, const int32_t* offsets, int B,
                       const pcreg_ransac_opts* o, const int32_t* sample_idx, double* T, int32_t* inlier_idx,
                       int32_t* n_inliers, int32_t* num_success, int32_t* max_inliers, int32_t* failed,
                       int32_t* iter_inl, int32_t* iter_inl_ref) {
    PCREG_ARG(o->iterNum >= 1 && o->minPtNum >= 3);
    PCREG_ARG(o->minPtNum == 3 || sample_idx != nullptr);
    int max_n = 0;
    for (int b = 0; b < B; ++b) { int nb = offsets[b + 1] - offsets[b]; PCREG_ARG(nb >= 0); if (nb > max_n) max_n = nb; }
    PCREG_ARG(offsets[0] == 0 && offsets[B] == total);
    size_t hyps = (size_t)o->iterNum * B;
    size_t wsb = ransac_workspace_bytes(o->iterNum, B, max_n);
    Stage st{scratch()};
    double *d1, *d2; int32_t *dOff, *dInl, *dS, *dI1, *dI2; pcreg_dev_ransac_result* dOut; char* ws;
    size_t tot = (size_t)(total > 0 ? total : 1);
    TRY(st.take(3 * tot, &d1));
    TRY(st.take(3 * tot, &d2));
    TRY(st.take((size_t)B + 1, &dOff));
    TRY(st.take((size_t)B, &dOut));
    TRY(st.take(tot, &dInl));
    TRY(st.take(wsb, &ws));
    // the optional tables behind everything else, taken (empty) on every path: each keeps its slot
    TRY(st.take(sample_idx ? hyps * o->minPtNum : 0, &dS));
    TRY(st.take(iter_inl ? hyps : 0, &dI1));
    TRY(st.take(iter_inl_ref ? hyps : 0, &dI2));
    if (!sample_idx) dS = nullptr;
    if (!iter_inl) dI1 = nullptr;
    if (!iter_inl_ref) dI2 = nullptr;
    if (sample_idx) PCREG_HIP(hipMemcpyAsync(dS, sample_idx, sizeof(int32_t) * hyps * o->minPtNum, hipMemcpyHostToDevice, g_stream));
    TRY(upload_cols(pts1, total, ld, 3, d1, g_stream));
    TRY(upload_cols(pts2, total, ld, 3, d2, g_stream));
    PCREG_HIP(hipMemcpyAsync(dOff, offsets, sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice, g_stream));
    TRY(launch_ransac(d1, d2, total, dOff, nullptr, max_n, B, *o, dS, dOut, dInl, dI1, dI2, ws, wsb, g_stream));
    std::vector<pcreg_dev_ransac_result> res((size_t)B);
    PCREG_HIP(hipMemcpyAsync(res.data(), dOut, sizeof(pcreg_dev_ransac_result) * (size_t)B, hipMemcpyDeviceToHost, g_stream));
    if (total > 0) PCREG_HIP(hipMemcpyAsync(inlier_idx, dInl, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, g_stream));
    if (iter_inl) PCREG_HIP(hipMemcpyAsync(iter_inl, dI1, sizeof(int32_t) * hyps, hipMemcpyDeviceToHost, g_stream));
    if (iter_inl_ref) PCREG_HIP(hipMemcpyAsync(iter_inl_ref, dI2, sizeof(int32_t) * hyps, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    for (int b = 0; b < B; ++b) {
        memcpy(T + 16 * (size_t)b, res[b].T, sizeof(double) * 16);
        n_inliers[b] = res[b].n_inliers; num_success[b] = res[b].num_success;
        max_inliers[b] = res[b].max_inliers; failed[b] = res[b].failed;
    }
    return PCREG_OK;
}

int pcreg_ransac(const double* pts1, const double* pts2, int n, int ld, const pcreg_ransac_opts* opts,
                 const int32_t* sample_idx, double T[16], int32_t* inlier_idx, int* n_inliers, int* num_success,
                 int* max_inliers, int* failed, int32_t* iter_inl, int32_t* iter_inl_ref) {
    PCREG_ARG(pts1 && pts2 && opts && T && inlier_idx && n_inliers && num_success && max_inliers && failed);
    PCREG_ARG(n >= 0 && ld >= n);
    GUARD();
    int32_t offsets[2] = {0, n};
    int32_t ni = 0, ns = 0, mi = 0, fl = 1;
    TRY(ransac_host(pts1, pts2, n, ld, offsets, 1, opts, sample_idx, T, inlier_idx, &ni, &ns, &mi, &fl, iter_inl, iter_inl_ref));
    *n_inliers = ni; *num_success = ns; *max_inliers = mi; *failed = fl;
    return PCREG_OK;
}

int pcreg_ransac_batched(const double* pts1, const double* pts2, int total, int ld, const int32_t* offsets, int B,
                         const pcreg_ransac_opts* opts, const int32_t* sample_idx, double* T, int32_t* inlier_idx,
                         int32_t* n_inliers, int32_t* num_success, int32_t* max_inliers, int32_t* failed) {
    PCREG_ARG(pts1 && pts2 && offsets && opts && T && inlier_idx && n_inliers && num_success && max_inliers && failed);
    PCREG_ARG(total >= 0 && ld >= total && B >= 1);
    GUARD();
    return ransac_host(pts1, pts2, total, ld, offsets, B, opts, sample_idx, T, inlier_idx, n_inliers, num_success,
                       max_inliers, failed, nullptr, nullptr);
}

int pcreg_fgr_resident_capacity(void) { return fgr_resident_capacity(); }

int pcreg_fgr_batched(const double* pts1, const double* pts2, int total, int ld, const int32_t* offsets, int B, const pcreg_fgr_opts* opts,
                      const double* T0, const int32_t* tuple_idx, pcreg_fgr_result* out, int32_t* inlier_idx, uint8_t* kept) {
    PCREG_ARG(pts1 && pts2 && offsets && opts && out && inlier_idx);
    PCREG_ARG(total >= 0 && ld >= total && B >= 1);
    PCREG_ARG(fgr_args_ok(*opts));
    PCREG_ARG(offsets[0] == 0 && offsets[B] == total);
    int max_n = 0;
    for (int b = 0; b < B; ++b) {
        PCREG_ARG(offsets[b + 1] >= offsets[b]);
        max_n = std::max(max_n, offsets[b + 1] - offsets[b]);
    }
    GUARD();
    const size_t wsb = fgr_ws_bytes(max_n, B, opts->iterations);
    PCREG_ARG(wsb != 0);
    const size_t tot = (size_t)(total > 0 ? total : 1), ntab = (size_t)B * (size_t)opts->n_tuples * 3;
    Stage st{scratch()};
    double *d1, *d2, *dT0; int32_t *dOff, *dInl, *dTab; uint8_t* dKept; pcreg_fgr_result* dOut; char* ws;
    TRY(st.take(3 * tot, &d1));
    TRY(st.take(3 * tot, &d2));
    TRY(st.take((size_t)B + 1, &dOff));
    TRY(st.take((size_t)B, &dOut));
    TRY(st.take(tot, &dInl));
    TRY(st.take(wsb, &ws));
    // the optional buffers behind everything else, taken (empty) on every path: each keeps its slot
    TRY(st.take(T0 ? 16 * (size_t)B : 0, &dT0));
    TRY(st.take(tuple_idx ? ntab : 0, &dTab));
    TRY(st.take(kept ? tot : 0, &dKept));
    if (!T0) dT0 = nullptr;
    if (!tuple_idx || ntab == 0) dTab = nullptr;
    if (!kept) dKept = nullptr;
    if (dT0) PCREG_HIP(hipMemcpyAsync(dT0, T0, sizeof(double) * 16 * (size_t)B, hipMemcpyHostToDevice, g_stream));
    if (dTab) PCREG_HIP(hipMemcpyAsync(dTab, tuple_idx, sizeof(int32_t) * ntab, hipMemcpyHostToDevice, g_stream));
    TRY(upload_cols(pts1, total, ld, 3, d1, g_stream));
    TRY(upload_cols(pts2, total, ld, 3, d2, g_stream));
    PCREG_HIP(hipMemcpyAsync(dOff, offsets, sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice, g_stream));
    TRY(launch_fgr(d1, d2, total, dOff, B, max_n, *opts, dT0, dTab, dOut, dInl, dKept, ws, wsb, g_stream));
    PCREG_HIP(hipMemcpyAsync(out, dOut, sizeof(pcreg_fgr_result) * (size_t)B, hipMemcpyDeviceToHost, g_stream));
    if (total > 0) PCREG_HIP(hipMemcpyAsync(inlier_idx, dInl, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, g_stream));
    if (kept && total > 0) PCREG_HIP(hipMemcpyAsync(kept, dKept, (size_t)total, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}

int pcreg_knn2_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm, int32_t* idx, float* dist) {
    PCREG_ARG(q && m && idx && dist && Q >= 0 && M >= 0 && ldq >= Q && ldm >= M);
    GUARD();
    if (Q == 0) return PCREG_OK;
    Stage st{scratch()};
    float *dq, *dm, *dd; int32_t* di; char* ws;
    size_t wsb = knn2_points_workspace_bytes(Q, M);
    TRY(st.take(3 * (size_t)Q, &dq));
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(2 * (size_t)Q, &di));
    TRY(st.take(2 * (size_t)Q, &dd));
    TRY(st.take(wsb, &ws));
    TRY(upload_cols(q, Q, ldq, 3, dq, g_stream));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    TRY(launch_knn2_points_f32(dq, Q, Q, dm, M, M, 0, di, dd, ws, wsb, g_stream));
    PCREG_HIP(hipMemcpyAsync(idx, di, sizeof(int32_t) * 2 * (size_t)Q, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(dist, dd, sizeof(float) * 2 * (size_t)Q, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}

// ---- prepared models ---------------------------------------------------------------------------------------------
}  // extern "C" (the handle types are C++ structs behind opaque C names)
struct pcreg_dev_model { pcreg::ModelView v; void* block; };
struct pcreg_model { pcreg_dev_model* dm; float* d_m; int M; };
extern "C" {

static int dev_model_create(const float* m, int M, int ldm, hipStream_t st, pcreg_dev_model** out) {
    *out = nullptr;
    void* block = nullptr;
    PCREG_HIP(hipMalloc(&block, model_prep_bytes(M)));
    pcreg_dev_model* h = new pcreg_dev_model{model_view(m, M, ldm, block), block};
    int rc = launch_model_prepare(h->v, st);
    if (rc) { (void)hipFree(block); delete h; return rc; }
    *out = h;
    return PCREG_OK;
}

int pcreg_dev_model_create(const float* m, int M, int ldm, void* stream, pcreg_dev_model** model) {
    PCREG_ARG(model != nullptr && M >= 0 && ldm >= M && (M == 0 || m != nullptr));
    GUARD();
    return dev_model_create(m, M, ldm, (hipStream_t)stream, model);
}
int pcreg_dev_model_destroy(pcreg_dev_model* model) {
    if (!model) return PCREG_OK;
    std::lock_guard<std::mutex> lock(g_mu);
    (void)hipDeviceSynchronize();                 // searches that still read the prepared block
    (void)hipFree(model->block);
    delete model;
    return PCREG_OK;
}
int pcreg_debug_dev_model_export(const pcreg_dev_model* model, int32_t* perm, float* sorted_soa, float* tile_box, float prep[24],
                                 void* stream) {
    PCREG_ARG(model != nullptr);
    GUARD();
    return model_export(model->v, perm, sorted_soa, tile_box, prep, (hipStream_t)stream);
}
int pcreg_debug_search_export(const void* ws, size_t ws_bytes, int Q, int M, int32_t* qperm, float* dk, void* stream) {
    GUARD();
    return search_export(ws, ws_bytes, Q, M, qperm, dk, (hipStream_t)stream);
}
size_t pcreg_dev_model_search_workspace(int Q, int M) { return search_ws_bytes(Q, M); }
int pcreg_dev_model_search_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, int32_t idx_base, int32_t* idx,
                               float* dist, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && q && idx && dist && workspace);
    GUARD();
    return launch_model_search(model->v, q, Q, ldq, idx_base, idx, dist, workspace, workspace_bytes, true, true, (hipStream_t)stream);
}
size_t pcreg_dev_model_knn_workspace(int Q, int M, int k) { return knn_k_ws_bytes(Q, M, k); }
int pcreg_dev_model_knn_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, int k, int32_t idx_base, int32_t* idx,
                            float* dist, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && q && idx && dist && workspace && k >= 1 && k <= kKnnMaxK && Q >= 0 && ldq >= Q && Q <= kKnnMaxQ);
    GUARD();
    return launch_model_knn(model->v, q, Q, ldq, k, idx_base, idx, dist, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_range_workspace(int Q, int M) { return range_ws_bytes(Q, M); }
int pcreg_dev_model_range_count_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, float r2, int32_t* counts,
                                    int64_t* seg_off, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && q && counts && seg_off && workspace && Q >= 0 && ldq >= Q && Q <= kRangeMaxQ && r2 >= 0.0f);
    GUARD();
    return launch_model_range_count(model->v, q, Q, ldq, r2, counts, seg_off, workspace, workspace_bytes, (hipStream_t)stream);
}
int pcreg_dev_model_range_fill_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, float r2, int32_t idx_base,
                                   const int64_t* seg_off, int64_t capacity, int32_t* idx, float* dist, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && q && seg_off && workspace && Q >= 0 && ldq >= Q && Q <= kRangeMaxQ && r2 >= 0.0f && capacity >= 0 &&
              (capacity == 0 || (idx && dist)));
    GUARD();
    return launch_model_range_fill(model->v, q, Q, ldq, r2, idx_base, seg_off, capacity, idx, dist, workspace, workspace_bytes,
                                   (hipStream_t)stream);
}
size_t pcreg_dev_model_score_workspace(int Q, int B, int M) { return score_ws_bytes(Q, B, M); }
int pcreg_dev_model_score_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const double* T_dev, int B, float r2,
                              int32_t* n_close, double* sum_d2, int32_t* idx, float* dist, void* workspace, size_t workspace_bytes,
                              void* stream) {
    PCREG_ARG(model && workspace && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f);
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T_dev && n_close && sum_d2)));
    PCREG_ARG(workspace_bytes >= score_ws_bytes(Q, B, 0));                   // (the size does not depend on M)
    GUARD();
    return launch_model_score(model->v, q, Q, ldq, T_dev, B, r2, n_close, sum_d2, idx, dist, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_refit_workspace(int Q, int B, int M) { return refit_ws_bytes(Q, B, M); }
int pcreg_dev_model_refit_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const double* T_dev, int B, float r2,
                              double* T_out, double* T_step, int32_t* n_close, double* sum_d2, int32_t* empty, void* workspace,
                              size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f);
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T_dev && T_out && T_out != T_dev && n_close && sum_d2 && empty)));
    PCREG_ARG(workspace_bytes >= refit_ws_bytes(Q, B, 0));                   // (the size does not depend on M)
    GUARD();
    return launch_model_refit(model->v, q, Q, ldq, T_dev, B, r2, T_out, T_step, n_close, sum_d2, empty, workspace, workspace_bytes,
                              (hipStream_t)stream);
}
size_t pcreg_dev_model_refit_plane_workspace(int Q, int B, int M) { return refit_plane_ws_bytes(Q, B, M); }
int pcreg_dev_model_refit_plane_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const double* T_dev, int B, float r2,
                                    const float* normals, int ldn, double* T_out, double* T_step, int32_t* n_close, double* sum_d2,
                                    int32_t* n_plane, double* sum_res2, int32_t* empty, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f && normals && ldn >= 0);
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T_dev && T_out && T_out != T_dev && n_close && sum_d2 && n_plane && sum_res2 && empty)));
    PCREG_ARG(workspace_bytes >= refit_plane_ws_bytes(Q, B, 0));             // (the size does not depend on M)
    PCREG_ARG(ldn >= model->v.M);                                            // (host data of the handle: refused before the device, as the rest)
    GUARD();
    return launch_model_refit_plane(model->v, q, Q, ldq, T_dev, B, r2, normals, ldn, T_out, T_step, n_close, sum_d2, n_plane, sum_res2, empty,
                                    workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_refit_gicp_workspace(int Q, int B, int M) { return refit_gicp_ws_bytes(Q, B, M); }
int pcreg_dev_model_refit_gicp_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const double* T_dev, int B, float r2,
                                   const float* normals, int ldn, const float* qnormals, int ldnq, double epsilon, double* T_out, double* T_step,
                                   int32_t* n_close, double* sum_d2, int32_t* n_pairs, double* sum_res2, int32_t* empty, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f && normals && ldn >= 0);
    PCREG_ARG(ldnq >= Q && (Q == 0 || qnormals) && epsilon > 0.0 && epsilon <= 1.0);                      // (a NaN epsilon fails both)
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T_dev && T_out && T_out != T_dev && n_close && sum_d2 && n_pairs && sum_res2 && empty)));
    PCREG_ARG(workspace_bytes >= refit_gicp_ws_bytes(Q, B, 0));              // (the size does not depend on M)
    PCREG_ARG(ldn >= model->v.M);                                            // (host data of the handle: refused before the device, as the rest)
    GUARD();
    return launch_model_refit_gicp(model->v, q, Q, ldq, T_dev, B, r2, normals, ldn, qnormals, ldnq, epsilon, T_out, T_step, n_close, sum_d2,
                                   n_pairs, sum_res2, empty, workspace, workspace_bytes, (hipStream_t)stream);
}
// the trimmed twins: the same checks and launchers, with the trim request; n_within and d2_cut may be null
#define TRIM_RATIO_OK(x) ((x) > 0.0 && (x) <= 1.0)                           /* (a NaN fails both) */
int pcreg_dev_model_score_trimmed_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const double* T_dev, int B, float r2,
                                      double keep_ratio, int32_t* n_close, double* sum_d2, int32_t* idx, float* dist, void* workspace,
                                      size_t workspace_bytes, void* stream, int32_t* n_within, float* d2_cut) {
    PCREG_ARG(model && workspace && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f && TRIM_RATIO_OK(keep_ratio));
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T_dev && n_close && sum_d2)));
    PCREG_ARG(workspace_bytes >= score_ws_bytes(Q, B, 0));   // (the untrimmed size: it does not depend on M)
    GUARD();
    const TrimIo trim{keep_ratio, n_within, d2_cut};
    return launch_model_score(model->v, q, Q, ldq, T_dev, B, r2, n_close, sum_d2, idx, dist, workspace, workspace_bytes, (hipStream_t)stream, &trim);
}
int pcreg_dev_model_refit_trimmed_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const double* T_dev, int B, float r2,
                                      double keep_ratio, double* T_out, double* T_step, int32_t* n_close, double* sum_d2, int32_t* empty,
                                      void* workspace, size_t workspace_bytes, void* stream, int32_t* n_within, float* d2_cut) {
    PCREG_ARG(model && workspace && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f && TRIM_RATIO_OK(keep_ratio));
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T_dev && T_out && T_out != T_dev && n_close && sum_d2 && empty)));
    PCREG_ARG(workspace_bytes >= refit_ws_bytes(Q, B, 0));   // (the untrimmed size: it does not depend on M)
    GUARD();
    const TrimIo trim{keep_ratio, n_within, d2_cut};
    return launch_model_refit(model->v, q, Q, ldq, T_dev, B, r2, T_out, T_step, n_close, sum_d2, empty, workspace, workspace_bytes,
                              (hipStream_t)stream, &trim);
}
int pcreg_dev_model_refit_plane_trimmed_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const double* T_dev, int B, float r2,
                                            double keep_ratio, const float* normals, int ldn, double* T_out, double* T_step, int32_t* n_close,
                                            double* sum_d2, int32_t* n_plane, double* sum_res2, int32_t* empty, void* workspace,
                                            size_t workspace_bytes, void* stream, int32_t* n_within, float* d2_cut) {
    PCREG_ARG(model && workspace && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f && normals && ldn >= 0 && TRIM_RATIO_OK(keep_ratio));
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T_dev && T_out && T_out != T_dev && n_close && sum_d2 && n_plane && sum_res2 && empty)));
    PCREG_ARG(workspace_bytes >= refit_plane_ws_bytes(Q, B, 0));   // (the untrimmed size: it does not depend on M)
    PCREG_ARG(ldn >= model->v.M);
    GUARD();
    const TrimIo trim{keep_ratio, n_within, d2_cut};
    return launch_model_refit_plane(model->v, q, Q, ldq, T_dev, B, r2, normals, ldn, T_out, T_step, n_close, sum_d2, n_plane, sum_res2, empty,
                                    workspace, workspace_bytes, (hipStream_t)stream, &trim);
}
int pcreg_dev_model_refit_gicp_trimmed_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const double* T_dev, int B, float r2,
                                           double keep_ratio, const float* normals, int ldn, const float* qnormals, int ldnq, double epsilon,
                                           double* T_out, double* T_step, int32_t* n_close, double* sum_d2, int32_t* n_pairs, double* sum_res2,
                                           int32_t* empty, void* workspace, size_t workspace_bytes, void* stream, int32_t* n_within, float* d2_cut) {
    PCREG_ARG(model && workspace && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f && normals && ldn >= 0 && TRIM_RATIO_OK(keep_ratio));
    PCREG_ARG(ldnq >= Q && (Q == 0 || qnormals) && epsilon > 0.0 && epsilon <= 1.0);
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T_dev && T_out && T_out != T_dev && n_close && sum_d2 && n_pairs && sum_res2 && empty)));
    PCREG_ARG(workspace_bytes >= refit_gicp_ws_bytes(Q, B, 0));   // (the untrimmed size: it does not depend on M)
    PCREG_ARG(ldn >= model->v.M);
    GUARD();
    const TrimIo trim{keep_ratio, n_within, d2_cut};
    return launch_model_refit_gicp(model->v, q, Q, ldq, T_dev, B, r2, normals, ldn, qnormals, ldnq, epsilon, T_out, T_step, n_close, sum_d2,
                                   n_pairs, sum_res2, empty, workspace, workspace_bytes, (hipStream_t)stream, &trim);
}
size_t pcreg_dev_model_refit_cpd_workspace(int Q, int B, int M) { return refit_cpd_ws_bytes(Q, B, M); }
int pcreg_dev_model_refit_cpd_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const double* T_dev, int B, const double* sigma2_in,
                                  double outlier, double* T_out, double* T_step, double* sigma2_out, double* Np, double* sum_res2, double* sum_d2,
                                  int32_t* n_live, int32_t* empty, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ);
    PCREG_ARG(outlier >= 0.0 && outlier < 1.0);                              // (a NaN fails both)
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T_dev && sigma2_in && T_out && T_out != T_dev && sigma2_out && Np && sum_res2 && sum_d2 && n_live && empty)));
    PCREG_ARG(workspace_bytes >= refit_cpd_ws_bytes(Q, B, model->v.M));      // (host data of the handle: refused before the device, as the rest)
    GUARD();
    return launch_model_refit_cpd(model->v, q, Q, ldq, T_dev, B, sigma2_in, outlier, T_out, T_step, sigma2_out, Np, sum_res2, sum_d2, n_live, empty,
                                  workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_cluster_workspace(int M) { return cluster_ws_bytes(M); }
int pcreg_dev_model_cluster_f32(const pcreg_dev_model* model, float r2, int32_t* label, int32_t* n_clusters, int32_t* first, int32_t* sizes,
                                void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && label && n_clusters && workspace && r2 >= 0.0f);
    GUARD();
    return launch_model_cluster(model->v, r2, label, n_clusters, first, sizes, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_dbscan_workspace(int M) { return dbscan_ws_bytes(M); }
int pcreg_dev_model_dbscan_f32(const pcreg_dev_model* model, float r2, int minpts, int32_t* label, int32_t* n_clusters, uint8_t* core,
                               int32_t* count, int32_t* first, int32_t* sizes, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && label && n_clusters && workspace && r2 >= 0.0f && minpts >= 1);
    GUARD();
    return launch_model_dbscan(model->v, r2, minpts, label, n_clusters, core, count, first, sizes, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_normals_workspace(int M, int k) { return normals_ws_bytes(M, k); }
int pcreg_dev_model_normals_f32(const pcreg_dev_model* model, int k, const double* viewpoint, float* normals, int ldn, float* variation,
                                void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && k >= 3 && k <= kKnnMaxK && ldn >= model->v.M && (normals || model->v.M == 0));
    GUARD();
    return launch_model_normals(model->v, k, viewpoint, normals, ldn, variation, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_denoise_workspace(int M, int k) { return denoise_ws_bytes(M, k); }
int pcreg_dev_model_denoise_f32(const pcreg_dev_model* model, int k, double threshold, double* mean_dist, int32_t* inliers, int32_t* n_inliers,
                                double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && k >= 1 && k <= kKnnMaxK - 1 && std::isfinite(threshold) && threshold >= 0.0 && (n_inliers || !inliers));
    PCREG_ARG(workspace_bytes >= denoise_ws_bytes(0, k));                    // (the smallest any model needs; the launcher checks this model's)
    GUARD();
    return launch_model_denoise(model->v, k, threshold, mean_dist, inliers, n_inliers, stats, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_fps_workspace(int M, int K) { return fps_ws_bytes(M, K); }
int pcreg_dev_model_fps_f32(const pcreg_dev_model* model, int K, int start, float stop_d2, int32_t* idx, float* dist, int32_t* n_out,
                            float* cover_d2, float* min_dist, int32_t* label, int32_t* info, void* workspace, size_t workspace_bytes,
                            void* stream) {
    PCREG_ARG(model && n_out && workspace && fps_args_ok(model->v.M, K, start, stop_d2));      // (host data of the handle: refused before the device)
    PCREG_ARG(workspace_bytes >= fps_ws_bytes(model->v.M, K));
    GUARD();
    return launch_model_fps(model->v, K, start, stop_d2, idx, dist, n_out, cover_d2, min_dist, label, info, workspace, workspace_bytes,
                            (hipStream_t)stream);
}
size_t pcreg_dev_model_fpfh_workspace(int M, int k) { return fpfh_ws_bytes(M, k); }
int pcreg_dev_model_fpfh_f32(const pcreg_dev_model* model, int k, const float* normals, int ldn, double* fpfh, uint8_t* spfh, void* workspace,
                             size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && k >= 3 && k <= kKnnMaxK && ldn >= model->v.M && ((normals && fpfh) || model->v.M == 0));
    PCREG_ARG(workspace_bytes >= fpfh_ws_bytes(model->v.M, k));
    GUARD();
    return launch_model_fpfh(model->v, k, normals, ldn, fpfh, spfh, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_fpfh_radius_workspace(int M, int64_t capacity) { return fpfh_radius_ws_bytes(M, capacity); }
int pcreg_dev_model_fpfh_radius_count_f32(const pcreg_dev_model* model, float r2, int32_t* counts, int64_t* seg_off, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && seg_off && (counts || model->v.M == 0) && r2 >= 0.0f && model->v.M <= fpfh_radius_max_rows());
    PCREG_ARG(workspace_bytes >= fpfh_radius_ws_bytes(model->v.M, 0));
    GUARD();
    return launch_model_fpfh_radius_count(model->v, r2, counts, seg_off, workspace, workspace_bytes, (hipStream_t)stream);
}
int pcreg_dev_model_fpfh_radius_f32(const pcreg_dev_model* model, float r2, int max_neighbors, const float* normals, int ldn, const int64_t* seg_off,
                                    int64_t capacity, double* fpfh, uint32_t* spfh, int32_t* n_neighbors, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    PCREG_ARG(model && workspace && seg_off && r2 >= 0.0f && max_neighbors >= 0 && capacity >= 0 && model->v.M <= fpfh_radius_max_rows() &&
              ldn >= model->v.M && ((normals && fpfh) || model->v.M == 0));
    PCREG_ARG(workspace_bytes >= fpfh_radius_ws_bytes(model->v.M, capacity));
    GUARD();
    return launch_model_fpfh_radius(model->v, r2, max_neighbors, normals, ldn, seg_off, capacity, fpfh, spfh, n_neighbors, workspace, workspace_bytes,
                                    (hipStream_t)stream);
}
size_t pcreg_dev_model_iss_workspace(int M) { return iss_ws_bytes(M); }
int pcreg_dev_model_iss_f32(const pcreg_dev_model* model, float r2_salient, float r2_nonmax, double gamma21, double gamma32, int min_neighbors,
                            int32_t* n_neighbors, double* eig, double* saliency, int32_t* keypoints, int32_t* n_keypoints, void* workspace,
                            size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && iss_args_ok(r2_salient, r2_nonmax, gamma21, gamma32, min_neighbors) && (n_keypoints || !keypoints));
    PCREG_ARG(workspace_bytes >= iss_ws_bytes(0));                           // (the smallest any model needs; the launcher checks this model's)
    GUARD();
    return launch_model_iss(model->v, r2_salient, r2_nonmax, gamma21, gamma32, min_neighbors, n_neighbors, eig, saliency, keypoints, n_keypoints,
                            workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_fit_planes_workspace(int M, int n_trials) { return planes_ws_bytes(M, n_trials); }
int pcreg_dev_model_fit_planes_f32(const pcreg_dev_model* model, float max_distance, const double* ref_vec, double max_angle, int max_planes,
                                   int n_trials, int min_inliers, uint64_t seed, const int32_t* samples, int32_t idx_base, int32_t* labels,
                                   double* planes, double* centres, int32_t* counts, double* rmse, int32_t* n_planes, int32_t* best_trial,
                                   int64_t* best_cost, int32_t* best_count, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && n_planes && planes_args_ok(max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers));
    PCREG_ARG(workspace_bytes >= planes_ws_bytes(0, n_trials));                // (the smallest any model needs; the launcher checks this model's)
    GUARD();
    return launch_model_fit_planes(model->v, max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers, seed, samples, idx_base, labels,
                                   planes, centres, counts, rmse, n_planes, best_trial, best_cost, best_count, workspace, workspace_bytes,
                                   (hipStream_t)stream);
}
size_t pcreg_dev_model_fit_spheres_workspace(int M, int n_trials) { return fit_spheres_ws_bytes(M, n_trials); }
int pcreg_dev_model_fit_spheres_f32(const pcreg_dev_model* model, float max_distance, float min_radius, float max_radius, int max_spheres,
                                    int n_trials, int min_inliers, uint64_t seed, const int32_t* samples, int32_t idx_base, int32_t* labels,
                                    double* spheres, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_spheres,
                                    int32_t* best_trial, int64_t* best_cost, int32_t* best_count, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    PCREG_ARG(model && workspace && n_spheres && fit_spheres_args_ok(max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers));
    PCREG_ARG(workspace_bytes >= fit_spheres_ws_bytes(0, n_trials));           // (the smallest any model needs; the launcher checks this model's)
    GUARD();
    return launch_model_fit_spheres(model->v, max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers, seed, samples, idx_base,
                                    labels, spheres, counts, rmse, refit_used, n_spheres, best_trial, best_cost, best_count, workspace,
                                    workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_model_fit_cylinders_workspace(int M, int n_trials) { return fit_cylinders_ws_bytes(M, n_trials); }
int pcreg_dev_model_fit_cylinders_f32(const pcreg_dev_model* model, float max_distance, float min_radius, float max_radius,
                                      const double* ref_vec, double max_angle, const float* normals_dev, int ldn, int max_cylinders,
                                      int n_trials, int min_inliers, uint64_t seed, const int32_t* samples, int32_t idx_base,
                                      int32_t* labels, double* cylinders, double* extents, int32_t* counts, double* rmse,
                                      int32_t* refit_used, int32_t* n_cylinders, int32_t* best_trial, int64_t* best_cost,
                                      int32_t* best_count, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(model && workspace && n_cylinders &&
              fit_cylinders_args_ok(max_distance, min_radius, max_radius, ref_vec, max_angle, max_cylinders, n_trials, min_inliers));
    PCREG_ARG(normals_dev || model->v.M == 0);
    PCREG_ARG(workspace_bytes >= fit_cylinders_ws_bytes(0, n_trials));         // (the smallest any model needs; the launcher checks this model's)
    GUARD();
    return launch_model_fit_cylinders(model->v, max_distance, min_radius, max_radius, ref_vec, max_angle, normals_dev, ldn, max_cylinders,
                                      n_trials, min_inliers, seed, samples, idx_base, labels, cylinders, extents, counts, rmse, refit_used,
                                      n_cylinders, best_trial, best_cost, best_count, workspace, workspace_bytes, (hipStream_t)stream);
}
int pcreg_dev_model_match_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const int32_t* idx, const float* dist,
                              float thr_abs, float max_ratio, int unique, void* workspace, size_t workspace_bytes, uint32_t* pairs,
                              double* pts1, double* pts2, int32_t* n_pairs, void* stream) {
    PCREG_ARG(model && q && idx && dist && workspace && n_pairs);
    GUARD();
    return launch_match_finish(model->v, q, Q, ldq, idx, dist, thr_abs, max_ratio, unique, workspace, workspace_bytes, pairs, pts1, pts2,
                               n_pairs, (hipStream_t)stream);
}
int pcreg_dev_model_match_table_f32(const pcreg_dev_model* model, int32_t m_lo, int M_total, const float* q, int Q, int ldq,
                                    const int32_t* idx, const float* dist, float thr_abs, float max_ratio, int unique,
                                    void* workspace, size_t workspace_bytes, int32_t* table, void* stream) {
    PCREG_ARG(model && q && idx && dist && workspace && table);
    GUARD();
    return launch_match_table(model->v, m_lo, M_total, q, Q, ldq, idx, dist, thr_abs, max_ratio, unique, workspace, workspace_bytes, table,
                              (hipStream_t)stream);
}
int pcreg_dev_match_from_table_f32(const float* q, int Q, int ldq, int M_total, const int32_t* idx, const float* dist, float thr_abs,
                                   float max_ratio, const int32_t* table, void* workspace, size_t workspace_bytes, uint32_t* pairs,
                                   double* pts1, double* pts2, int32_t* n_pairs, void* stream) {
    PCREG_ARG(q && idx && dist && table && workspace && n_pairs);
    GUARD();
    return launch_match_from_table(q, Q, ldq, M_total, idx, dist, thr_abs, max_ratio, table, workspace, workspace_bytes, pairs, pts1, pts2,
                                   n_pairs, (hipStream_t)stream);
}

// matchFeatures' chain on raw points against a prepared model: upload the surface, search (4 launches), match (1)
static int match_points_on_view(Stage& st, const ModelView& v, const float* q, int Q, int ldq, float thr_abs, float max_ratio, int unique,
                                uint32_t* pairs, int* P) {
    *P = 0;
    if (Q == 0 || v.M == 0) return PCREG_OK;
    float *dq, *dd; int32_t *di, *n_pairs; char* ws; uint32_t* dpairs;
    const size_t wsb = search_ws_bytes(Q, v.M);
    TRY(st.take(3 * (size_t)Q, &dq));
    TRY(st.take(2 * (size_t)Q, &di));
    TRY(st.take(2 * (size_t)Q, &dd));
    TRY(st.take(wsb, &ws));
    TRY(st.take(1, &n_pairs));
    TRY(st.take(2 * (size_t)Q, &dpairs));
    TRY(upload_cols(q, Q, ldq, 3, dq, g_stream));
    TRY(launch_model_search(v, dq, Q, Q, 0, di, dd, ws, wsb, true, true, g_stream));
    TRY(launch_match_finish(v, dq, Q, Q, di, dd, thr_abs, max_ratio, unique, ws, wsb, dpairs, nullptr, nullptr, n_pairs, g_stream));
    int32_t np = 0;
    PCREG_HIP(hipMemcpyAsync(&np, n_pairs, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    if (np > 0) PCREG_HIP(hipMemcpy(pairs, dpairs, sizeof(uint32_t) * 2 * (size_t)np, hipMemcpyDeviceToHost));
    *P = np;
    return PCREG_OK;
}

int pcreg_model_create(const float* m, int M, int ldm, pcreg_model** model) {
    PCREG_ARG(model != nullptr && M >= 0 && ldm >= M && (M == 0 || m != nullptr));
    GUARD();
    *model = nullptr;
    float* d_m = nullptr;
    PCREG_HIP(hipMalloc((void**)&d_m, sizeof(float) * 3 * (size_t)(M > 0 ? M : 1)));
    int rc = upload_cols(m, M, ldm, 3, d_m, g_stream);
    pcreg_dev_model* dm = nullptr;
    if (!rc) rc = dev_model_create(d_m, M, M > 0 ? M : 1, g_stream, &dm);
    if (!rc && hipStreamSynchronize(g_stream) != hipSuccess) { set_error("model preparation failed"); rc = PCREG_E_HIP; }
    if (rc) { if (dm) { (void)hipFree(dm->block); delete dm; } (void)hipFree(d_m); return rc; }
    *model = new pcreg_model{dm, d_m, M};
    return PCREG_OK;
}
int pcreg_model_destroy(pcreg_model* model) {
    if (!model) return PCREG_OK;
    std::lock_guard<std::mutex> lock(g_mu);
    (void)hipDeviceSynchronize();
    if (model->dm) { (void)hipFree(model->dm->block); delete model->dm; }
    (void)hipFree(model->d_m);
    delete model;
    return PCREG_OK;
}
int pcreg_model_size(const pcreg_model* model, int* M) {
    PCREG_ARG(model && M);
    *M = model->M;
    return PCREG_OK;
}
int pcreg_model_match_points_f32(pcreg_model* model, const float* q, int Q, int ldq, float thr_abs, float max_ratio, int unique,
                                 uint32_t* pairs, int* P) {
    PCREG_ARG(model && model->dm && q && pairs && P && Q >= 0 && ldq >= Q);
    GUARD();
    Stage st{scratch()};
    return match_points_on_view(st, model->dm->v, q, Q, ldq, thr_abs, max_ratio, unique, pairs, P);
}

// the k nearest rows on a prepared model: upload the queries, search, copy [Q][k] back
static int knn_on_view(Stage& st, const ModelView& v, const float* q, int Q, int ldq, int k, int32_t* idx, float* dist) {
    if (Q == 0) return PCREG_OK;
    float *dq, *dd; int32_t* di; char* ws;
    const size_t wsb = knn_k_ws_bytes(Q, v.M, k), nk = (size_t)Q * k;
    TRY(st.take(3 * (size_t)Q, &dq));
    TRY(st.take(nk, &di));
    TRY(st.take(nk, &dd));
    TRY(st.take(wsb, &ws));
    TRY(upload_cols(q, Q, ldq, 3, dq, g_stream));
    TRY(launch_model_knn(v, dq, Q, Q, k, 0, di, dd, ws, wsb, g_stream));
    PCREG_HIP(hipMemcpyAsync(idx, di, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(dist, dd, sizeof(float) * nk, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}
int pcreg_model_knn_f32(pcreg_model* model, const float* q, int Q, int ldq, int k, int32_t* idx, float* dist) {
    PCREG_ARG(model && q && idx && dist && k >= 1 && k <= kKnnMaxK && Q >= 0 && ldq >= Q && Q <= kKnnMaxQ);
    PCREG_ARG(model->dm != nullptr);
    GUARD();
    Stage st{scratch()};
    return knn_on_view(st, model->dm->v, q, Q, ldq, k, idx, dist);
}
int pcreg_knn_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm, int k, int32_t* idx, float* dist) {
    PCREG_ARG(q && m && idx && dist && k >= 1 && k <= kKnnMaxK && Q >= 0 && M >= 0 && ldq >= Q && ldm >= M && Q <= kKnnMaxQ);
    GUARD();
    if (Q == 0) return PCREG_OK;
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return knn_on_view(st, v, q, Q, ldq, k, idx, dist);
}

// rangesearch on a prepared model: upload the queries, count + scan, read seg_off (the total), then fill + order when the
// caller's capacity holds the total.  The two result buffers are taken last, and taken (empty) on the count-only path too.
static int range_on_view(Stage& st, const ModelView& v, const float* q, int Q, int ldq, float r2, int64_t capacity, int64_t* seg_off,
                         int32_t* idx, float* dist) {
    float *dq, *dd; int32_t *dc, *di; int64_t* ds; char* ws;
    const size_t wsb = range_ws_bytes(Q, v.M);
    TRY(st.take(3 * (size_t)Q, &dq));
    TRY(st.take((size_t)Q, &dc));
    TRY(st.take((size_t)Q + 1, &ds));
    TRY(st.take(wsb, &ws));
    TRY(upload_cols(q, Q, ldq, 3, dq, g_stream));
    TRY(launch_model_range_count(v, dq, Q, Q, r2, dc, ds, ws, wsb, g_stream));
    PCREG_HIP(hipMemcpyAsync(seg_off, ds, sizeof(int64_t) * ((size_t)Q + 1), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    const int64_t total = seg_off[Q];
    const bool fill = total > 0 && total <= capacity;
    TRY(st.take(fill ? (size_t)total : 0, &di));
    TRY(st.take(fill ? (size_t)total : 0, &dd));
    if (!fill) return PCREG_OK;
    TRY(launch_model_range_fill(v, dq, Q, Q, r2, 0, ds, total, di, dd, ws, wsb, g_stream));
    PCREG_HIP(hipMemcpyAsync(idx, di, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(dist, dd, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}
int pcreg_model_range_f32(pcreg_model* model, const float* q, int Q, int ldq, float r2, int64_t capacity, int64_t* seg_off, int32_t* idx,
                          float* dist) {
    PCREG_ARG(model && q && seg_off && Q >= 0 && ldq >= Q && Q <= kRangeMaxQ && r2 >= 0.0f && capacity >= 0 && (capacity == 0 || (idx && dist)));
    PCREG_ARG(model->dm != nullptr);
    GUARD();
    Stage st{scratch()};
    return range_on_view(st, model->dm->v, q, Q, ldq, r2, capacity, seg_off, idx, dist);
}
int pcreg_range_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm, float r2, int64_t capacity, int64_t* seg_off,
                           int32_t* idx, float* dist) {
    PCREG_ARG(q && m && seg_off && Q >= 0 && M >= 0 && ldq >= Q && ldm >= M && Q <= kRangeMaxQ && r2 >= 0.0f && capacity >= 0 &&
              (capacity == 0 || (idx && dist)));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return range_on_view(st, v, q, Q, ldq, r2, capacity, seg_off, idx, dist);
}

// B transforms scored against a prepared model: upload the queries and the transforms, score, read the 12 B bytes of counts
// and sums back, and the [B][Q] rows and distances when the caller asked for them
// (`keep`: the trimmed twin's ratio and its two outputs, each of which may be null -- DESIGN 4.32; null: the untrimmed call)
struct HostTrim { double keep_ratio; int32_t* n_within; float* d2_cut; };
static int model_score_host(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, const HostTrim* keep,
                            int32_t* n_close, double* sum_d2, int32_t* idx, float* dist) {
    PCREG_ARG(model && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f);
    PCREG_ARG(!keep || TRIM_RATIO_OK(keep->keep_ratio));
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T && n_close && sum_d2)));
    PCREG_ARG(model->dm != nullptr);
    GUARD();
    if (B == 0) return PCREG_OK;
    Stage st{scratch()};
    const ModelView& v = model->dm->v;
    const size_t wsb = score_ws_bytes(Q, B, v.M), bq = (size_t)B * Q;
    float *dq, *dd, *dc; double *dT, *ds; int32_t *dn, *di, *dw; char* ws;
    TRY(st.take(3 * (size_t)Q, &dq));
    TRY(st.take(16 * (size_t)B, &dT));
    TRY(st.take((size_t)B, &dn));
    TRY(st.take((size_t)B, &ds));
    TRY(st.take(idx ? bq : 0, &di));
    TRY(st.take(dist ? bq : 0, &dd));
    TRY(st.take(wsb, &ws));
    TRY(st.take(keep ? (size_t)B : 0, &dw));
    TRY(st.take(keep ? (size_t)B : 0, &dc));
    TRY(upload_cols(q, Q, ldq, 3, dq, g_stream));
    PCREG_HIP(hipMemcpyAsync(dT, T, sizeof(double) * 16 * (size_t)B, hipMemcpyHostToDevice, g_stream));
    const TrimIo trim{keep ? keep->keep_ratio : 1.0, dw, dc};
    TRY(launch_model_score(v, dq, Q, Q, dT, B, r2, dn, ds, idx ? di : nullptr, dist ? dd : nullptr, ws, wsb, g_stream, keep ? &trim : nullptr));
    if (keep && keep->n_within) PCREG_HIP(hipMemcpyAsync(keep->n_within, dw, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, g_stream));
    if (keep && keep->d2_cut) PCREG_HIP(hipMemcpyAsync(keep->d2_cut, dc, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(n_close, dn, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(sum_d2, ds, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, g_stream));
    if (idx && bq) PCREG_HIP(hipMemcpyAsync(idx, di, sizeof(int32_t) * bq, hipMemcpyDeviceToHost, g_stream));
    if (dist && bq) PCREG_HIP(hipMemcpyAsync(dist, dd, sizeof(float) * bq, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}

int pcreg_model_score_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, int32_t* n_close,
                          double* sum_d2, int32_t* idx, float* dist) {
    return model_score_host(model, q, Q, ldq, T, B, r2, nullptr, n_close, sum_d2, idx, dist);
}
int pcreg_model_score_trimmed_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, double keep_ratio,
                                  int32_t* n_close, double* sum_d2, int32_t* idx, float* dist, int32_t* n_within, float* d2_cut) {
    const HostTrim keep{keep_ratio, n_within, d2_cut};
    return model_score_host(model, q, Q, ldq, T, B, r2, &keep, n_close, sum_d2, idx, dist);
}

// The staging of every "B transforms refitted `steps` times" entry: the queries and the transforms are uploaded once, the steps
// run on the device, each step's T_out the next one's input, and ONE result block is read back -- the last step's.  A block is
// `cols` doubles' room per transform and starts with T_out (16 B doubles); two blocks take turns, because a step may not write
// over its input.  The takes keep the Stage rule (every take before the first use) and each entry's order: take_inputs, the
// entry's own inputs, take_blocks, the entry's own workspaces; then upload, the entry's own uploads, run.
struct RefitCol { void* dst; int word; size_t bytes; };            // B elements of `bytes` bytes from 4-byte word `word` x B of the block (dst null: not wanted)
struct RefitStaging {
    Stage st{scratch()};
    size_t nQ, nB; int cols;
    float* dq = nullptr; double *dT = nullptr, *dout = nullptr; char* ws = nullptr;
    RefitStaging(int Q, int B, int cols_) : nQ((size_t)Q), nB((size_t)B), cols(cols_) {}
    int take_inputs() {
        TRY(st.take(3 * nQ, &dq));
        return st.take(16 * nB, &dT);
    }
    int take_blocks(size_t wsb) {
        TRY(st.take(2 * (size_t)cols * nB, &dout));
        return st.take(wsb, &ws);
    }
    int upload(const float* q, int ldq, const double* T) {
        TRY(upload_cols(q, (int)nQ, ldq, 3, dq, g_stream));
        PCREG_HIP(hipMemcpyAsync(dT, T, sizeof(double) * 16 * nB, hipMemcpyHostToDevice, g_stream));
        return PCREG_OK;
    }
    // step(in, blk): one launch that reads the transforms at `in` (dT, then the block before) and fills the block `blk`
    int run(int steps, const std::function<int(const double*, double*)>& step, std::initializer_list<RefitCol> table) {
        const double* in = dT;
        double* blk = dout;
        for (int s = 0; s < steps; ++s) {
            blk = dout + (size_t)(s & 1) * cols * nB;
            TRY(step(in, blk));
            in = blk;
        }
        std::vector<double> host((size_t)cols * nB);
        PCREG_HIP(hipMemcpyAsync(host.data(), blk, sizeof(double) * host.size(), hipMemcpyDeviceToHost, g_stream));
        PCREG_HIP(hipStreamSynchronize(g_stream));
        for (const RefitCol& c : table) if (c.dst) memcpy(c.dst, (const char*)host.data() + 4 * (size_t)c.word * nB, c.bytes * nB);
        return PCREG_OK;
    }
};

// B transforms refitted `steps` times on their close pairs; the block: [T_out 16 B doubles][sum_d2 B doubles][n_close B int32]
// [empty B int32], and in every refit's trimmed twin one more column at the end: [n_within B int32][d2_cut B float]
static int model_refit_host(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, const HostTrim* keep, int steps,
                            double* T_out, int32_t* n_close, double* sum_d2, int32_t* empty) {
    PCREG_ARG(model && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f && steps >= 1);
    PCREG_ARG(!keep || TRIM_RATIO_OK(keep->keep_ratio));
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T && T_out && n_close && sum_d2 && empty)));
    PCREG_ARG(model->dm != nullptr);
    GUARD();
    if (B == 0) return PCREG_OK;
    const ModelView& v = model->dm->v;
    const size_t wsb = refit_ws_bytes(Q, B, v.M), nB = (size_t)B;
    RefitStaging rs(Q, B, keep ? 19 : 18);                                 // 17 B doubles and 2 B int32 (and the trim's column)
    TRY(rs.take_inputs());
    TRY(rs.take_blocks(wsb));
    TRY(rs.upload(q, ldq, T));
    return rs.run(steps, [&](const double* in, double* blk) {
        int32_t* ib = (int32_t*)(blk + 17 * nB);
        const TrimIo trim{keep ? keep->keep_ratio : 1.0, ib + 2 * nB, (float*)(ib + 3 * nB)};
        return launch_model_refit(v, rs.dq, Q, Q, in, B, r2, blk, nullptr, ib, blk + 16 * nB, ib + nB, rs.ws, wsb, g_stream, keep ? &trim : nullptr);
    }, {{T_out, 0, 128}, {sum_d2, 32, 8}, {n_close, 34, 4}, {empty, 35, 4}, {keep ? keep->n_within : nullptr, 36, 4}, {keep ? keep->d2_cut : nullptr, 37, 4}});
}
int pcreg_model_refit_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, int steps, double* T_out,
                          int32_t* n_close, double* sum_d2, int32_t* empty) {
    return model_refit_host(model, q, Q, ldq, T, B, r2, nullptr, steps, T_out, n_close, sum_d2, empty);
}
int pcreg_model_refit_trimmed_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, double keep_ratio, int steps,
                                  double* T_out, int32_t* n_close, double* sum_d2, int32_t* empty, int32_t* n_within, float* d2_cut) {
    const HostTrim keep{keep_ratio, n_within, d2_cut};
    return model_refit_host(model, q, Q, ldq, T, B, r2, &keep, steps, T_out, n_close, sum_d2, empty);
}

// B transforms refitted `steps` times by the point-to-plane step, with the normals uploaded once (or computed once on the device
// by the normals chain, k nearest rows and no viewpoint) before the first step; the block: [T_out 16 B doubles][sum_d2 B]
// [sum_res2 B][n_close B int32][n_plane B int32][empty B int32]
static int model_refit_plane_host(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, const HostTrim* keep, int steps,
                                  const float* normals, int ldn, int k, double* T_out, int32_t* n_close, double* sum_d2, int32_t* n_plane,
                                  double* sum_res2, int32_t* empty) {
    PCREG_ARG(model && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f && steps >= 1);
    PCREG_ARG(!keep || TRIM_RATIO_OK(keep->keep_ratio));
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T && T_out && n_close && sum_d2 && n_plane && sum_res2 && empty)));
    PCREG_ARG(normals ? ldn >= 0 : (k >= 3 && k <= kKnnMaxK));
    PCREG_ARG(model->dm != nullptr && (!normals || ldn >= model->M));
    GUARD();
    if (B == 0) return PCREG_OK;
    const ModelView& v = model->dm->v;
    const int M = v.M;
    const size_t wsb = refit_plane_ws_bytes(Q, B, M), nwsb = normals || M == 0 ? 0 : normals_ws_bytes(M, k), nB = (size_t)B;
    RefitStaging rs(Q, B, keep ? 21 : 20);                                 // 18 B doubles and 3 B int32 (a word of padding, then the trim's column)
    float* dn; char* nws;
    TRY(rs.take_inputs());
    TRY(rs.st.take(3 * (size_t)(M > 0 ? M : 1), &dn));
    TRY(rs.take_blocks(wsb));
    TRY(rs.st.take(nwsb, &nws));
    TRY(rs.upload(q, ldq, T));
    if (normals) TRY(upload_cols(normals, M, ldn, 3, dn, g_stream));
    else if (M > 0) TRY(launch_model_normals(v, k, nullptr, dn, M, nullptr, nws, nwsb, g_stream));
    return rs.run(steps, [&](const double* in, double* blk) {
        int32_t* ib = (int32_t*)(blk + 18 * nB);
        const TrimIo trim{keep ? keep->keep_ratio : 1.0, ib + 4 * nB, (float*)(ib + 5 * nB)};
        return launch_model_refit_plane(v, rs.dq, Q, Q, in, B, r2, dn, M > 0 ? M : 1, blk, nullptr, ib, blk + 16 * nB, ib + nB, blk + 17 * nB, ib + 2 * nB,
                                        rs.ws, wsb, g_stream, keep ? &trim : nullptr);
    }, {{T_out, 0, 128}, {sum_d2, 32, 8}, {sum_res2, 34, 8}, {n_close, 36, 4}, {n_plane, 37, 4}, {empty, 38, 4},
        {keep ? keep->n_within : nullptr, 40, 4}, {keep ? keep->d2_cut : nullptr, 41, 4}});
}
int pcreg_model_refit_plane_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, int steps,
                                const float* normals, int ldn, int k, double* T_out, int32_t* n_close, double* sum_d2, int32_t* n_plane,
                                double* sum_res2, int32_t* empty) {
    return model_refit_plane_host(model, q, Q, ldq, T, B, r2, nullptr, steps, normals, ldn, k, T_out, n_close, sum_d2, n_plane, sum_res2, empty);
}
int pcreg_model_refit_plane_trimmed_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, double keep_ratio,
                                        int steps, const float* normals, int ldn, int k, double* T_out, int32_t* n_close, double* sum_d2,
                                        int32_t* n_plane, double* sum_res2, int32_t* empty, int32_t* n_within, float* d2_cut) {
    const HostTrim keep{keep_ratio, n_within, d2_cut};
    return model_refit_plane_host(model, q, Q, ldq, T, B, r2, &keep, steps, normals, ldn, k, T_out, n_close, sum_d2, n_plane, sum_res2, empty);
}

// B transforms refitted `steps` times by the plane-to-plane step: pcreg_model_refit_plane_f32's result block, with the
// query normals beside the model normals -- each uploaded once, or computed once on the device by the normals chain (k nearest
// rows, no viewpoint; the queries' from a prepared model of q that lives in the staging and goes with it)
static int model_refit_gicp_host(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, const HostTrim* keep, int steps,
                                 const float* normals, int ldn, const float* qnormals, int ldnq, int k, double epsilon, double* T_out,
                                 int32_t* n_close, double* sum_d2, int32_t* n_pairs, double* sum_res2, int32_t* empty) {
    PCREG_ARG(model && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && r2 >= 0.0f && steps >= 1);
    PCREG_ARG(!keep || TRIM_RATIO_OK(keep->keep_ratio));
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T && T_out && n_close && sum_d2 && n_pairs && sum_res2 && empty)));
    PCREG_ARG(epsilon > 0.0 && epsilon <= 1.0);                               // (a NaN epsilon fails both)
    PCREG_ARG((normals && qnormals) || (k >= 3 && k <= kKnnMaxK));
    PCREG_ARG((!normals || ldn >= 0) && (!qnormals || ldnq >= Q));
    PCREG_ARG(model->dm != nullptr && (!normals || ldn >= model->M));
    GUARD();
    if (B == 0) return PCREG_OK;
    const ModelView& v = model->dm->v;
    const int M = v.M;
    const bool own_q = !qnormals && Q > 0;
    const size_t wsb = refit_gicp_ws_bytes(Q, B, M), nB = (size_t)B;
    const size_t nwsb = std::max(normals || M == 0 ? (size_t)0 : normals_ws_bytes(M, k), own_q ? normals_ws_bytes(Q, k) : (size_t)0);
    RefitStaging rs(Q, B, keep ? 21 : 20);                                 // 18 B doubles and 3 B int32 (a word of padding, then the trim's column)
    float *dn, *dnq; char *nws, *qblock;
    TRY(rs.take_inputs());
    TRY(rs.st.take(3 * (size_t)(M > 0 ? M : 1), &dn));
    TRY(rs.st.take(3 * (size_t)(Q > 0 ? Q : 1), &dnq));
    TRY(rs.take_blocks(wsb));
    TRY(rs.st.take(nwsb, &nws));
    TRY(rs.st.take(own_q ? model_prep_bytes(Q) : 0, &qblock));
    TRY(rs.upload(q, ldq, T));
    if (normals) TRY(upload_cols(normals, M, ldn, 3, dn, g_stream));
    else if (M > 0) TRY(launch_model_normals(v, k, nullptr, dn, M, nullptr, nws, nwsb, g_stream));
    if (qnormals) TRY(upload_cols(qnormals, Q, ldnq, 3, dnq, g_stream));
    else if (own_q) {
        const ModelView qv = model_view(rs.dq, Q, Q, qblock);
        TRY(launch_model_prepare(qv, g_stream));
        TRY(launch_model_normals(qv, k, nullptr, dnq, Q, nullptr, nws, nwsb, g_stream));
    }
    return rs.run(steps, [&](const double* in, double* blk) {
        int32_t* ib = (int32_t*)(blk + 18 * nB);
        const TrimIo trim{keep ? keep->keep_ratio : 1.0, ib + 4 * nB, (float*)(ib + 5 * nB)};
        return launch_model_refit_gicp(v, rs.dq, Q, Q, in, B, r2, dn, M > 0 ? M : 1, dnq, Q > 0 ? Q : 1, epsilon, blk, nullptr, ib, blk + 16 * nB, ib + nB,
                                       blk + 17 * nB, ib + 2 * nB, rs.ws, wsb, g_stream, keep ? &trim : nullptr);
    }, {{T_out, 0, 128}, {sum_d2, 32, 8}, {sum_res2, 34, 8}, {n_close, 36, 4}, {n_pairs, 37, 4}, {empty, 38, 4},
        {keep ? keep->n_within : nullptr, 40, 4}, {keep ? keep->d2_cut : nullptr, 41, 4}});
}
int pcreg_model_refit_gicp_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, int steps,
                               const float* normals, int ldn, const float* qnormals, int ldnq, int k, double epsilon, double* T_out,
                               int32_t* n_close, double* sum_d2, int32_t* n_pairs, double* sum_res2, int32_t* empty) {
    return model_refit_gicp_host(model, q, Q, ldq, T, B, r2, nullptr, steps, normals, ldn, qnormals, ldnq, k, epsilon, T_out, n_close, sum_d2, n_pairs,
                                 sum_res2, empty);
}
int pcreg_model_refit_gicp_trimmed_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, float r2, double keep_ratio,
                                       int steps, const float* normals, int ldn, const float* qnormals, int ldnq, int k, double epsilon,
                                       double* T_out, int32_t* n_close, double* sum_d2, int32_t* n_pairs, double* sum_res2, int32_t* empty,
                                       int32_t* n_within, float* d2_cut) {
    const HostTrim keep{keep_ratio, n_within, d2_cut};
    return model_refit_gicp_host(model, q, Q, ldq, T, B, r2, &keep, steps, normals, ldn, qnormals, ldnq, k, epsilon, T_out, n_close, sum_d2, n_pairs,
                                 sum_res2, empty);
}

// B transforms refitted `steps` times by the coherent-point-drift step; the block: [T_out 16 B doubles][sigma2_out B][Np B]
// [sum_res2 B][sum_d2 B][n_live B int32][empty B int32].  A step reads its transforms AND its sigma2 from the block before it.
int pcreg_model_refit_cpd_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T, int B, const double* sigma2_in, double outlier,
                              int steps, double* T_out, double* sigma2_out, double* Np, double* sum_res2, double* sum_d2, int32_t* n_live,
                              int32_t* empty) {
    PCREG_ARG(model && Q >= 0 && B >= 0 && ldq >= Q && Q <= kScoreMaxQ && steps >= 1);
    PCREG_ARG(outlier >= 0.0 && outlier < 1.0);                              // (a NaN fails both)
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T && sigma2_in && T_out && sigma2_out && Np && sum_res2 && sum_d2 && n_live && empty)));
    PCREG_ARG(model->dm != nullptr);
    GUARD();
    if (B == 0) return PCREG_OK;
    const ModelView& v = model->dm->v;
    const size_t wsb = refit_cpd_ws_bytes(Q, B, v.M), nB = (size_t)B;
    RefitStaging rs(Q, B, 21);                                             // 20 B doubles and 2 B int32
    double* dsig;
    TRY(rs.take_inputs());
    TRY(rs.st.take(nB, &dsig));
    TRY(rs.take_blocks(wsb));
    TRY(rs.upload(q, ldq, T));
    PCREG_HIP(hipMemcpyAsync(dsig, sigma2_in, sizeof(double) * nB, hipMemcpyHostToDevice, g_stream));
    return rs.run(steps, [&](const double* in, double* blk) {
        const double* sig = in == rs.dT ? dsig : in + 16 * nB;             // (the first step's, then the sigma2_out beside the T_out it reads)
        int32_t* ib = (int32_t*)(blk + 20 * nB);
        return launch_model_refit_cpd(v, rs.dq, Q, Q, in, B, sig, outlier, blk, nullptr, blk + 16 * nB, blk + 17 * nB, blk + 18 * nB, blk + 19 * nB, ib,
                                      ib + nB, rs.ws, wsb, g_stream);
    }, {{T_out, 0, 128}, {sigma2_out, 32, 8}, {Np, 34, 8}, {sum_res2, 36, 8}, {sum_d2, 38, 8}, {n_live, 40, 4}, {empty, 41, 4}});
}

// clusterPoints on a prepared model: label the rows on the device, read the labels back, and form the CSR lists on the host by
// one stable counting pass (rows ascend inside a cluster because they are placed in ascending order)
static int cluster_on_view(Stage& st, const ModelView& v, float r2, int32_t* label, int32_t* n_clusters, int32_t* cl_off, int32_t* members) {
    const int M = v.M;
    *n_clusters = 0;
    if (cl_off) cl_off[0] = 0;
    if (M == 0) return PCREG_OK;
    int32_t *dl, *dn; char* ws;
    const size_t wsb = cluster_ws_bytes(M);
    TRY(st.take((size_t)M, &dl));
    TRY(st.take(1, &dn));
    TRY(st.take(wsb, &ws));
    TRY(launch_model_cluster(v, r2, dl, dn, nullptr, nullptr, ws, wsb, g_stream));
    int32_t nc = 0;
    PCREG_HIP(hipMemcpyAsync(label, dl, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(&nc, dn, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    *n_clusters = nc;
    if (!cl_off) return PCREG_OK;
    for (int c = 0; c <= nc; ++c) cl_off[c] = 0;
    for (int i = 0; i < M; ++i) ++cl_off[label[i] + 1];
    for (int c = 0; c < nc; ++c) cl_off[c + 1] += cl_off[c];
    std::vector<int32_t> at(cl_off, cl_off + nc);
    for (int i = 0; i < M; ++i) members[at[label[i]]++] = i;
    return PCREG_OK;
}
int pcreg_model_cluster_f32(pcreg_model* model, float r2, int32_t* label, int32_t* n_clusters, int32_t* cl_off, int32_t* members) {
    PCREG_ARG(model && n_clusters && r2 >= 0.0f && (members || !cl_off || model->M == 0) && (cl_off || !members));
    PCREG_ARG(model->dm != nullptr && (label || model->M == 0));
    GUARD();
    Stage st{scratch()};
    return cluster_on_view(st, model->dm->v, r2, label, n_clusters, cl_off, members);
}
int pcreg_cluster_points_f32(const float* m, int M, int ldm, float r2, int32_t* label, int32_t* n_clusters, int32_t* cl_off, int32_t* members) {
    PCREG_ARG(n_clusters && M >= 0 && ldm >= M && (M == 0 || (m && label)) && r2 >= 0.0f && (members || !cl_off || M == 0) && (cl_off || !members));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return cluster_on_view(st, v, r2, label, n_clusters, cl_off, members);
}

// DBSCAN on a prepared model: label, core and count on the device, read back; the CSR lists on the host as
// cluster_on_view forms them, over the clusters only: a noise row (label -1) is in no list
static int dbscan_on_view(Stage& st, const ModelView& v, float r2, int minpts, int32_t* label, int32_t* n_clusters, uint8_t* core, int32_t* count,
                          int32_t* cl_off, int32_t* members) {
    const int M = v.M;
    *n_clusters = 0;
    if (cl_off) cl_off[0] = 0;
    if (M == 0) return PCREG_OK;
    int32_t *dl, *dn, *dc = nullptr; uint8_t* dk = nullptr; char* ws;
    const size_t wsb = dbscan_ws_bytes(M);
    TRY(st.take((size_t)M, &dl));
    TRY(st.take(1, &dn));
    if (core) TRY(st.take((size_t)M, &dk));
    if (count) TRY(st.take((size_t)M, &dc));
    TRY(st.take(wsb, &ws));
    TRY(launch_model_dbscan(v, r2, minpts, dl, dn, dk, dc, nullptr, nullptr, ws, wsb, g_stream));
    int32_t nc = 0;
    PCREG_HIP(hipMemcpyAsync(label, dl, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(&nc, dn, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    if (core) PCREG_HIP(hipMemcpyAsync(core, dk, (size_t)M, hipMemcpyDeviceToHost, g_stream));
    if (count) PCREG_HIP(hipMemcpyAsync(count, dc, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    *n_clusters = nc;
    if (!cl_off) return PCREG_OK;
    for (int c = 0; c <= nc; ++c) cl_off[c] = 0;
    for (int i = 0; i < M; ++i) if (label[i] >= 0) ++cl_off[label[i] + 1];
    for (int c = 0; c < nc; ++c) cl_off[c + 1] += cl_off[c];
    std::vector<int32_t> at(cl_off, cl_off + nc);
    for (int i = 0; i < M; ++i) if (label[i] >= 0) members[at[label[i]]++] = i;
    return PCREG_OK;
}
int pcreg_model_dbscan_f32(pcreg_model* model, float r2, int minpts, int32_t* label, int32_t* n_clusters, uint8_t* core, int32_t* count,
                           int32_t* cl_off, int32_t* members) {
    PCREG_ARG(model && n_clusters && r2 >= 0.0f && minpts >= 1 && (members || !cl_off || model->M == 0) && (cl_off || !members));
    PCREG_ARG(model->dm != nullptr && (label || model->M == 0));
    GUARD();
    Stage st{scratch()};
    return dbscan_on_view(st, model->dm->v, r2, minpts, label, n_clusters, core, count, cl_off, members);
}
int pcreg_dbscan_points_f32(const float* m, int M, int ldm, float r2, int minpts, int32_t* label, int32_t* n_clusters, uint8_t* core,
                            int32_t* count, int32_t* cl_off, int32_t* members) {
    PCREG_ARG(n_clusters && M >= 0 && ldm >= M && (M == 0 || (m && label)) && r2 >= 0.0f && minpts >= 1 && (members || !cl_off || M == 0) &&
              (cl_off || !members));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return dbscan_on_view(st, v, r2, minpts, label, n_clusters, core, count, cl_off, members);
}

// normals of a prepared model's own rows: compute on the device (compact, ld = M), read back into the caller's leading dimension
static int normals_on_view(Stage& st, const ModelView& v, int k, const double* viewpoint, float* normals, int ldn, float* variation) {
    const int M = v.M;
    if (M == 0) return PCREG_OK;
    float *dn, *dv; char* ws;
    const size_t wsb = normals_ws_bytes(M, k);
    TRY(st.take(3 * (size_t)M, &dn));
    TRY(st.take(variation ? (size_t)M : 0, &dv));
    TRY(st.take(wsb, &ws));
    TRY(launch_model_normals(v, k, viewpoint, dn, M, variation ? dv : nullptr, ws, wsb, g_stream));
    if (ldn == M) PCREG_HIP(hipMemcpyAsync(normals, dn, sizeof(float) * 3 * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    else PCREG_HIP(hipMemcpy2DAsync(normals, sizeof(float) * (size_t)ldn, dn, sizeof(float) * (size_t)M, sizeof(float) * (size_t)M, 3,
                                    hipMemcpyDeviceToHost, g_stream));
    if (variation) PCREG_HIP(hipMemcpyAsync(variation, dv, sizeof(float) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}
int pcreg_model_normals_f32(pcreg_model* model, int k, const double* viewpoint, float* normals, int ldn, float* variation) {
    PCREG_ARG(model && k >= 3 && k <= kKnnMaxK && ldn >= model->M && (normals || model->M == 0));
    PCREG_ARG(model->dm != nullptr);
    GUARD();
    Stage st{scratch()};
    return normals_on_view(st, model->dm->v, k, viewpoint, normals, ldn, variation);
}
int pcreg_point_normals_f32(const float* m, int M, int ldm, int k, const double* viewpoint, float* normals, int ldn, float* variation) {
    PCREG_ARG(M >= 0 && ldm >= M && k >= 3 && k <= kKnnMaxK && ldn >= M && (M == 0 || (m && normals)));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return normals_on_view(st, v, k, viewpoint, normals, ldn, variation);
}

// pcdenoise on a prepared model's own rows: the chain on the device, ONE read of the count and the statistic (with the mean
// distances behind them), then the inlier rows the count names
static int denoise_on_view(Stage& st, const ModelView& v, int k, double threshold, double* mean_dist, int32_t* inliers, int32_t* n_inliers,
                           double* stats) {
    const int M = v.M;
    if (n_inliers) *n_inliers = 0;
    if (M == 0) {
        if (stats) { stats[0] = stats[1] = stats[2] = std::nan(""); stats[3] = 0.0; }
        return PCREG_OK;
    }
    double *dmd, *dstats; int32_t *dinl, *dn; char* ws;
    const size_t wsb = denoise_ws_bytes(M, k);
    TRY(st.take(mean_dist ? (size_t)M : 0, &dmd));
    TRY(st.take(inliers ? (size_t)M : 0, &dinl));
    TRY(st.take(1, &dn));
    TRY(st.take(4, &dstats));
    TRY(st.take(wsb, &ws));
    TRY(launch_model_denoise(v, k, threshold, mean_dist ? dmd : nullptr, inliers ? dinl : nullptr, n_inliers ? dn : nullptr, dstats, ws, wsb, g_stream));
    int32_t n = 0;
    if (n_inliers) PCREG_HIP(hipMemcpyAsync(&n, dn, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    if (stats) PCREG_HIP(hipMemcpyAsync(stats, dstats, sizeof(double) * 4, hipMemcpyDeviceToHost, g_stream));
    if (mean_dist) PCREG_HIP(hipMemcpyAsync(mean_dist, dmd, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));                   // the count fixes how many rows come back
    if (inliers && n > 0) {
        PCREG_HIP(hipMemcpyAsync(inliers, dinl, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g_stream));
        PCREG_HIP(hipStreamSynchronize(g_stream));
    }
    if (n_inliers) *n_inliers = n;
    return PCREG_OK;
}
int pcreg_model_denoise_f32(pcreg_model* model, int k, double threshold, double* mean_dist, int32_t* inliers, int32_t* n_inliers, double* stats) {
    PCREG_ARG(model && k >= 1 && k <= kKnnMaxK - 1 && std::isfinite(threshold) && threshold >= 0.0 && (n_inliers || !inliers));
    PCREG_ARG(model->dm != nullptr);
    GUARD();
    Stage st{scratch()};
    return denoise_on_view(st, model->dm->v, k, threshold, mean_dist, inliers, n_inliers, stats);
}
int pcreg_point_denoise_f32(const float* m, int M, int ldm, int k, double threshold, double* mean_dist, int32_t* inliers, int32_t* n_inliers,
                            double* stats) {
    PCREG_ARG(M >= 0 && ldm >= M && k >= 1 && k <= kKnnMaxK - 1 && std::isfinite(threshold) && threshold >= 0.0 && (M == 0 || m) &&
              (n_inliers || !inliers));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return denoise_on_view(st, v, k, threshold, mean_dist, inliers, n_inliers, stats);
}

// farthest point sampling of a prepared model's own rows: the two launches on the device, ONE read of the three words (count, info,
// cover), then the rows the count names and the per-row outputs; a dead start row (info = 1) is refused with nothing written
static int fps_on_view(Stage& st, const ModelView& v, int K, int start, float stop_d2, int32_t* idx, float* dist, int32_t* n_out,
                       float* cover_d2, float* min_dist, int32_t* label) {
    const int M = v.M;
    int32_t *didx, *dword, *dlabel; float *ddist, *dmin; char* ws;
    const size_t wsb = fps_ws_bytes(M, K);
    TRY(st.take(idx ? (size_t)K : 0, &didx));
    TRY(st.take(dist ? (size_t)K : 0, &ddist));
    TRY(st.take(4, &dword));                                     // n_out, info, cover_d2
    TRY(st.take(min_dist ? (size_t)M : 0, &dmin));
    TRY(st.take(label ? (size_t)M : 0, &dlabel));
    TRY(st.take(wsb, &ws));
    TRY(launch_model_fps(v, K, start, stop_d2, idx ? didx : nullptr, dist ? ddist : nullptr, dword, (float*)(dword + 2), min_dist ? dmin : nullptr,
                         label ? dlabel : nullptr, dword + 1, ws, wsb, g_stream));
    int32_t w[4] = {0, 0, 0, 0};
    PCREG_HIP(hipMemcpyAsync(w, dword, sizeof w, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));                   // the count fixes how many rows come back
    if (w[1] != 0) {
        set_error("bad argument: start = %d is a row with a non-finite coordinate", start);
        return PCREG_E_ARG;
    }
    const int32_t n = w[0];
    if (idx && n > 0) PCREG_HIP(hipMemcpyAsync(idx, didx, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g_stream));
    if (dist && n > 0) PCREG_HIP(hipMemcpyAsync(dist, ddist, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, g_stream));
    if (min_dist && M > 0) PCREG_HIP(hipMemcpyAsync(min_dist, dmin, sizeof(float) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    if (label && M > 0) PCREG_HIP(hipMemcpyAsync(label, dlabel, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    *n_out = n;
    if (cover_d2) memcpy(cover_d2, &w[2], sizeof(float));
    return PCREG_OK;
}
int pcreg_model_fps_f32(pcreg_model* model, int K, int start, float stop_d2, int32_t* idx, float* dist, int32_t* n_out, float* cover_d2,
                        float* min_dist, int32_t* label) {
    PCREG_ARG(model && n_out && fps_args_ok(model->M, K, start, stop_d2));
    PCREG_ARG(model->dm != nullptr);
    GUARD();
    Stage st{scratch()};
    return fps_on_view(st, model->dm->v, K, start, stop_d2, idx, dist, n_out, cover_d2, min_dist, label);
}
int pcreg_point_fps_f32(const float* m, int M, int ldm, int K, int start, float stop_d2, int32_t* idx, float* dist, int32_t* n_out,
                        float* cover_d2, float* min_dist, int32_t* label) {
    PCREG_ARG(n_out && M >= 0 && ldm >= M && (M == 0 || m) && fps_args_ok(M, K, start, stop_d2));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return fps_on_view(st, v, K, start, stop_d2, idx, dist, n_out, cover_d2, min_dist, label);
}

// FPFH of a prepared model's own rows: the normals uploaded once (or computed by the normals chain with k_normals and the
// viewpoint), the chain on the device, ONE read of the [M][33] block (and the counts), transposed into the caller's columns
static int fpfh_on_view(Stage& st, const ModelView& v, int k, const float* normals, int ldn, int k_normals, const double* viewpoint, double* fpfh,
                        int ldf, uint8_t* spfh) {
    const int M = v.M;
    if (M == 0) return PCREG_OK;
    float* dn; double* dout; uint8_t* dsp; char *ws, *nws;
    const size_t wsb = fpfh_ws_bytes(M, k), nwsb = normals ? 0 : normals_ws_bytes(M, k_normals), n33 = 33 * (size_t)M;
    TRY(st.take(3 * (size_t)M, &dn));
    TRY(st.take(n33, &dout));
    TRY(st.take(spfh ? n33 : 0, &dsp));
    TRY(st.take(wsb, &ws));
    TRY(st.take(nwsb, &nws));
    if (normals) TRY(upload_cols(normals, M, ldn, 3, dn, g_stream));
    else TRY(launch_model_normals(v, k_normals, viewpoint, dn, M, nullptr, nws, nwsb, g_stream));
    TRY(launch_model_fpfh(v, k, dn, M, dout, spfh ? dsp : nullptr, ws, wsb, g_stream));
    std::vector<double> host(n33);
    PCREG_HIP(hipMemcpyAsync(host.data(), dout, sizeof(double) * n33, hipMemcpyDeviceToHost, g_stream));
    if (spfh) PCREG_HIP(hipMemcpyAsync(spfh, dsp, n33, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    for (int b = 0; b < 33; ++b)
        for (int i = 0; i < M; ++i) fpfh[(size_t)i + (size_t)b * (size_t)ldf] = host[(size_t)i * 33 + b];
    return PCREG_OK;
}
int pcreg_model_fpfh_f32(pcreg_model* model, int k, const float* normals, int ldn, int k_normals, const double* viewpoint, double* fpfh, int ldf,
                         uint8_t* spfh) {
    PCREG_ARG(model && k >= 3 && k <= kKnnMaxK && ldf >= model->M && (fpfh || model->M == 0));
    PCREG_ARG(normals ? ldn >= model->M : (k_normals >= 3 && k_normals <= kKnnMaxK));
    PCREG_ARG(model->dm != nullptr);
    GUARD();
    Stage st{scratch()};
    return fpfh_on_view(st, model->dm->v, k, normals, ldn, k_normals, viewpoint, fpfh, ldf, spfh);
}
int pcreg_point_fpfh_f32(const float* m, int M, int ldm, int k, const float* normals, int ldn, int k_normals, const double* viewpoint,
                         double* fpfh, int ldf, uint8_t* spfh) {
    PCREG_ARG(M >= 0 && ldm >= M && k >= 3 && k <= kKnnMaxK && ldf >= M && (M == 0 || (m && fpfh)));
    PCREG_ARG(normals ? ldn >= M : (k_normals >= 3 && k_normals <= kKnnMaxK));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return fpfh_on_view(st, v, k, normals, ldn, k_normals, viewpoint, fpfh, ldf, spfh);
}

// FPFH from radius neighbourhoods on a prepared model: the normals uploaded once (or computed by the normals chain), the count,
// ONE read of the total, then the lists' workspace is taken (last: its size is data) and fill + R1 + R2 run; ONE read of the
// [M][33] block (and the counts asked for), transposed into the caller's columns
static int fpfh_radius_on_view(Stage& st, const ModelView& v, float r2, int max_neighbors, const float* normals, int ldn, int k_normals,
                               const double* viewpoint, double* fpfh, int ldf, uint32_t* spfh, int32_t* n_neighbors) {
    const int M = v.M;
    if (M == 0) return PCREG_OK;
    float* dn; double* dout; uint32_t* dsp; int32_t *dc, *dnn; int64_t* ds; char *cws, *nws, *ws;
    const size_t cwsb = fpfh_radius_ws_bytes(M, 0), nwsb = normals ? 0 : normals_ws_bytes(M, k_normals), n33 = 33 * (size_t)M;
    TRY(st.take(3 * (size_t)M, &dn));
    TRY(st.take(n33, &dout));
    TRY(st.take(spfh ? n33 : 0, &dsp));
    TRY(st.take(n_neighbors ? (size_t)M : 0, &dnn));
    TRY(st.take((size_t)M, &dc));
    TRY(st.take((size_t)M + 1, &ds));
    TRY(st.take(cwsb, &cws));
    TRY(st.take(nwsb, &nws));
    if (normals) TRY(upload_cols(normals, M, ldn, 3, dn, g_stream));
    else TRY(launch_model_normals(v, k_normals, viewpoint, dn, M, nullptr, nws, nwsb, g_stream));
    TRY(launch_model_fpfh_radius_count(v, r2, dc, ds, cws, cwsb, g_stream));
    int64_t total = 0;
    PCREG_HIP(hipMemcpyAsync(&total, ds + M, sizeof(int64_t), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    const size_t wsb = fpfh_radius_ws_bytes(M, total);
    const int rc = st.take(wsb, &ws);
    if (rc) {
        (void)hipGetLastError();
        set_error("out of device memory: the radius neighbourhoods hold %lld (row, neighbour) pairs in all and need %zu bytes", (long long)total, wsb);
        return rc;
    }
    TRY(launch_model_fpfh_radius(v, r2, max_neighbors, dn, M, ds, total, dout, spfh ? dsp : nullptr, n_neighbors ? dnn : nullptr, ws, wsb, g_stream));
    std::vector<double> host(n33);
    PCREG_HIP(hipMemcpyAsync(host.data(), dout, sizeof(double) * n33, hipMemcpyDeviceToHost, g_stream));
    if (spfh) PCREG_HIP(hipMemcpyAsync(spfh, dsp, sizeof(uint32_t) * n33, hipMemcpyDeviceToHost, g_stream));
    if (n_neighbors) PCREG_HIP(hipMemcpyAsync(n_neighbors, dnn, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    for (int b = 0; b < 33; ++b)
        for (int i = 0; i < M; ++i) fpfh[(size_t)i + (size_t)b * (size_t)ldf] = host[(size_t)i * 33 + b];
    return PCREG_OK;
}
int pcreg_model_fpfh_radius_f32(pcreg_model* model, float r2, int max_neighbors, const float* normals, int ldn, int k_normals,
                                const double* viewpoint, double* fpfh, int ldf, uint32_t* spfh, int32_t* n_neighbors) {
    PCREG_ARG(model && r2 >= 0.0f && max_neighbors >= 0 && model->M <= fpfh_radius_max_rows() && ldf >= model->M && (fpfh || model->M == 0));
    PCREG_ARG(normals ? ldn >= model->M : (k_normals >= 3 && k_normals <= kKnnMaxK));
    PCREG_ARG(model->dm != nullptr);
    GUARD();
    Stage st{scratch()};
    return fpfh_radius_on_view(st, model->dm->v, r2, max_neighbors, normals, ldn, k_normals, viewpoint, fpfh, ldf, spfh, n_neighbors);
}
int pcreg_point_fpfh_radius_f32(const float* m, int M, int ldm, float r2, int max_neighbors, const float* normals, int ldn, int k_normals,
                                const double* viewpoint, double* fpfh, int ldf, uint32_t* spfh, int32_t* n_neighbors) {
    PCREG_ARG(M >= 0 && ldm >= M && r2 >= 0.0f && max_neighbors >= 0 && M <= fpfh_radius_max_rows() && ldf >= M && (M == 0 || (m && fpfh)));
    PCREG_ARG(normals ? ldn >= M : (k_normals >= 3 && k_normals <= kKnnMaxK));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return fpfh_radius_on_view(st, v, r2, max_neighbors, normals, ldn, k_normals, viewpoint, fpfh, ldf, spfh, n_neighbors);
}

// ISS keypoints of a prepared model's own rows: the chain on the device, ONE read of the count (with the per-row outputs behind
// it), then the keypoint rows the count names
static int iss_on_view(Stage& st, const ModelView& v, float r2s, float r2n, double g21, double g32, int min_nb, int32_t* n_neighbors, double* eig,
                       double* saliency, int32_t* keypoints, int32_t* n_keypoints) {
    const int M = v.M;
    if (n_keypoints) *n_keypoints = 0;
    if (M == 0) return PCREG_OK;
    double *deig, *dsal; int32_t *dnn, *dkp, *dn; char* ws;
    const size_t wsb = iss_ws_bytes(M);
    TRY(st.take((size_t)M, &dnn));
    TRY(st.take(eig ? 3 * (size_t)M : 0, &deig));
    TRY(st.take((size_t)M, &dsal));
    TRY(st.take(keypoints ? (size_t)M : 0, &dkp));
    TRY(st.take(1, &dn));
    TRY(st.take(wsb, &ws));
    TRY(launch_model_iss(v, r2s, r2n, g21, g32, min_nb, dnn, eig ? deig : nullptr, dsal, keypoints ? dkp : nullptr, n_keypoints ? dn : nullptr, ws, wsb,
                         g_stream));
    int32_t n = 0;
    if (n_keypoints) PCREG_HIP(hipMemcpyAsync(&n, dn, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(n_neighbors, dnn, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(saliency, dsal, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    if (eig) PCREG_HIP(hipMemcpyAsync(eig, deig, sizeof(double) * 3 * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));                   // the count fixes how many rows come back
    if (keypoints && n > 0) {
        PCREG_HIP(hipMemcpyAsync(keypoints, dkp, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g_stream));
        PCREG_HIP(hipStreamSynchronize(g_stream));
    }
    if (n_keypoints) *n_keypoints = n;
    return PCREG_OK;
}
int pcreg_model_iss_f32(pcreg_model* model, float r2_salient, float r2_nonmax, double gamma21, double gamma32, int min_neighbors,
                        int32_t* n_neighbors, double* eig, double* saliency, int32_t* keypoints, int32_t* n_keypoints) {
    PCREG_ARG(model && iss_args_ok(r2_salient, r2_nonmax, gamma21, gamma32, min_neighbors) && (n_keypoints || !keypoints));
    PCREG_ARG(model->dm != nullptr && model->M < iss_max_rows() && ((n_neighbors && saliency) || model->M == 0));
    GUARD();
    Stage st{scratch()};
    return iss_on_view(st, model->dm->v, r2_salient, r2_nonmax, gamma21, gamma32, min_neighbors, n_neighbors, eig, saliency, keypoints, n_keypoints);
}
int pcreg_point_iss_f32(const float* m, int M, int ldm, float r2_salient, float r2_nonmax, double gamma21, double gamma32, int min_neighbors,
                        int32_t* n_neighbors, double* eig, double* saliency, int32_t* keypoints, int32_t* n_keypoints) {
    PCREG_ARG(M >= 0 && ldm >= M && M < iss_max_rows() && iss_args_ok(r2_salient, r2_nonmax, gamma21, gamma32, min_neighbors) &&
              (M == 0 || (m && n_neighbors && saliency)) && (n_keypoints || !keypoints));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return iss_on_view(st, v, r2_salient, r2_nonmax, gamma21, gamma32, min_neighbors, n_neighbors, eig, saliency, keypoints, n_keypoints);
}

// plane extraction on a prepared model's own rows: the chain on the device, then ONE read of everything
static int planes_on_view(Stage& st, const ModelView& v, float t, const double* ref_vec, double max_angle, int P, int B, int min_inliers,
                          uint64_t seed, const int32_t* samples, int32_t* labels, double* planes, double* centres, int32_t* counts, double* rmse,
                          int32_t* n_planes, int32_t* best_trial, int64_t* best_cost, int32_t* best_count) {
    const int M = v.M;
    *n_planes = 0;
    if (M == 0) {
        for (int i = 0; i < P; ++i) {
            if (planes) for (int c = 0; c < 4; ++c) planes[4 * i + c] = 0.0;
            if (centres) for (int c = 0; c < 3; ++c) centres[3 * i + c] = 0.0;
            if (counts) counts[i] = 0;
            if (rmse) rmse[i] = 0.0;
            if (best_trial) best_trial[i] = 0;
            if (best_cost) best_cost[i] = 0;
            if (best_count) best_count[i] = 0;
        }
        return PCREG_OK;
    }
    int32_t *dlab, *dcnt, *dnp, *dbt, *dbn, *dsmp; double *dpl, *dce, *drm; int64_t* dbc; char* ws;
    const size_t wsb = planes_ws_bytes(M, B), ns = samples ? (size_t)P * (size_t)B * 3 : 0;
    TRY(st.take((size_t)M, &dlab));
    TRY(st.take(4 * (size_t)P, &dpl));
    TRY(st.take(3 * (size_t)P, &dce));
    TRY(st.take((size_t)P, &dcnt));
    TRY(st.take((size_t)P, &drm));
    TRY(st.take(1, &dnp));
    TRY(st.take((size_t)P, &dbt));
    TRY(st.take((size_t)P, &dbc));
    TRY(st.take((size_t)P, &dbn));
    TRY(st.take(ns, &dsmp));
    TRY(st.take(wsb, &ws));
    if (samples) PCREG_HIP(hipMemcpyAsync(dsmp, samples, sizeof(int32_t) * ns, hipMemcpyHostToDevice, g_stream));
    TRY(launch_model_fit_planes(v, t, ref_vec, max_angle, P, B, min_inliers, seed, samples ? dsmp : nullptr, 1, dlab, dpl, dce, dcnt, drm, dnp, dbt,
                                dbc, dbn, ws, wsb, g_stream));
    PCREG_HIP(hipMemcpyAsync(labels, dlab, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(planes, dpl, sizeof(double) * 4 * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(centres, dce, sizeof(double) * 3 * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(counts, dcnt, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(rmse, drm, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(n_planes, dnp, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    if (best_trial) PCREG_HIP(hipMemcpyAsync(best_trial, dbt, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    if (best_cost) PCREG_HIP(hipMemcpyAsync(best_cost, dbc, sizeof(int64_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    if (best_count) PCREG_HIP(hipMemcpyAsync(best_count, dbn, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}
int pcreg_model_fit_planes_f32(pcreg_model* model, float max_distance, const double* ref_vec, double max_angle, int max_planes, int n_trials,
                               int min_inliers, uint64_t seed, const int32_t* samples, int32_t* labels, double* planes, double* centres,
                               int32_t* counts, double* rmse, int32_t* n_planes, int32_t* best_trial, int64_t* best_cost, int32_t* best_count) {
    PCREG_ARG(model && n_planes && planes_args_ok(max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers));
    PCREG_ARG(model->dm != nullptr && model->M < planes_max_rows() && ((labels && planes && centres && counts && rmse) || model->M == 0));
    GUARD();
    Stage st{scratch()};
    return planes_on_view(st, model->dm->v, max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers, seed, samples, labels, planes,
                          centres, counts, rmse, n_planes, best_trial, best_cost, best_count);
}
int pcreg_point_fit_planes_f32(const float* m, int M, int ldm, float max_distance, const double* ref_vec, double max_angle, int max_planes,
                               int n_trials, int min_inliers, uint64_t seed, const int32_t* samples, int32_t* labels, double* planes,
                               double* centres, int32_t* counts, double* rmse, int32_t* n_planes, int32_t* best_trial, int64_t* best_cost,
                               int32_t* best_count) {
    PCREG_ARG(M >= 0 && ldm >= M && M < planes_max_rows() && n_planes &&
              planes_args_ok(max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers) &&
              (M == 0 || (m && labels && planes && centres && counts && rmse)));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return planes_on_view(st, v, max_distance, ref_vec, max_angle, max_planes, n_trials, min_inliers, seed, samples, labels, planes, centres, counts,
                          rmse, n_planes, best_trial, best_cost, best_count);
}

// sphere extraction on a prepared model's own rows: the chain on the device, then ONE read of everything
static int fit_spheres_on_view(Stage& st, const ModelView& v, float t, float min_radius, float max_radius, int P, int B, int min_inliers,
                               uint64_t seed, const int32_t* samples, int32_t* labels, double* spheres, int32_t* counts, double* rmse,
                               int32_t* refit_used, int32_t* n_spheres, int32_t* best_trial, int64_t* best_cost, int32_t* best_count) {
    const int M = v.M;
    *n_spheres = 0;
    if (M == 0) {
        for (int i = 0; i < P; ++i) {
            if (spheres) for (int c = 0; c < 4; ++c) spheres[4 * i + c] = 0.0;
            if (counts) counts[i] = 0;
            if (rmse) rmse[i] = 0.0;
            if (refit_used) refit_used[i] = 0;
            if (best_trial) best_trial[i] = 0;
            if (best_cost) best_cost[i] = 0;
            if (best_count) best_count[i] = 0;
        }
        return PCREG_OK;
    }
    int32_t *dlab, *dcnt, *dru, *dnp, *dbt, *dbn, *dsmp; double *dsp, *drm; int64_t* dbc; char* ws;
    const size_t wsb = fit_spheres_ws_bytes(M, B), ns = samples ? (size_t)P * (size_t)B * 4 : 0;
    TRY(st.take((size_t)M, &dlab));
    TRY(st.take(4 * (size_t)P, &dsp));
    TRY(st.take((size_t)P, &dcnt));
    TRY(st.take((size_t)P, &drm));
    TRY(st.take((size_t)P, &dru));
    TRY(st.take(1, &dnp));
    TRY(st.take((size_t)P, &dbt));
    TRY(st.take((size_t)P, &dbc));
    TRY(st.take((size_t)P, &dbn));
    TRY(st.take(ns, &dsmp));
    TRY(st.take(wsb, &ws));
    if (samples) PCREG_HIP(hipMemcpyAsync(dsmp, samples, sizeof(int32_t) * ns, hipMemcpyHostToDevice, g_stream));
    TRY(launch_model_fit_spheres(v, t, min_radius, max_radius, P, B, min_inliers, seed, samples ? dsmp : nullptr, 1, dlab, dsp, dcnt, drm, dru, dnp,
                                 dbt, dbc, dbn, ws, wsb, g_stream));
    PCREG_HIP(hipMemcpyAsync(labels, dlab, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(spheres, dsp, sizeof(double) * 4 * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(counts, dcnt, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(rmse, drm, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(refit_used, dru, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(n_spheres, dnp, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    if (best_trial) PCREG_HIP(hipMemcpyAsync(best_trial, dbt, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    if (best_cost) PCREG_HIP(hipMemcpyAsync(best_cost, dbc, sizeof(int64_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    if (best_count) PCREG_HIP(hipMemcpyAsync(best_count, dbn, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}
int pcreg_model_fit_spheres_f32(pcreg_model* model, float max_distance, float min_radius, float max_radius, int max_spheres, int n_trials,
                                int min_inliers, uint64_t seed, const int32_t* samples, int32_t* labels, double* spheres, int32_t* counts,
                                double* rmse, int32_t* refit_used, int32_t* n_spheres, int32_t* best_trial, int64_t* best_cost,
                                int32_t* best_count) {
    PCREG_ARG(model && n_spheres && fit_spheres_args_ok(max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers));
    PCREG_ARG(model->dm != nullptr && model->M < fit_spheres_max_rows() &&
              ((labels && spheres && counts && rmse && refit_used) || model->M == 0));
    GUARD();
    Stage st{scratch()};
    return fit_spheres_on_view(st, model->dm->v, max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers, seed, samples, labels,
                               spheres, counts, rmse, refit_used, n_spheres, best_trial, best_cost, best_count);
}
int pcreg_point_fit_spheres_f32(const float* m, int M, int ldm, float max_distance, float min_radius, float max_radius, int max_spheres,
                                int n_trials, int min_inliers, uint64_t seed, const int32_t* samples, int32_t* labels, double* spheres,
                                int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_spheres, int32_t* best_trial,
                                int64_t* best_cost, int32_t* best_count) {
    PCREG_ARG(M >= 0 && ldm >= M && M < fit_spheres_max_rows() && n_spheres &&
              fit_spheres_args_ok(max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers) &&
              (M == 0 || (m && labels && spheres && counts && rmse && refit_used)));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return fit_spheres_on_view(st, v, max_distance, min_radius, max_radius, max_spheres, n_trials, min_inliers, seed, samples, labels, spheres,
                               counts, rmse, refit_used, n_spheres, best_trial, best_cost, best_count);
}

// cylinder extraction on a prepared model's own rows: the normals uploaded once (or computed by the normals chain with k_normals and
// no viewpoint), the chain on the device, then ONE read of everything
static int fit_cylinders_on_view(Stage& st, const ModelView& v, float t, float min_radius, float max_radius, const double* ref_vec,
                                 double max_angle, const float* normals, int ldn, int k_normals, int P, int B, int min_inliers,
                                 uint64_t seed, const int32_t* samples, int32_t* labels, double* cylinders, double* extents,
                                 int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_cylinders, int32_t* best_trial,
                                 int64_t* best_cost, int32_t* best_count) {
    const int M = v.M;
    *n_cylinders = 0;
    if (M == 0) {
        for (int i = 0; i < P; ++i) {
            if (cylinders) for (int c = 0; c < 7; ++c) cylinders[7 * i + c] = 0.0;
            if (extents) { extents[2 * i] = 0.0; extents[2 * i + 1] = 0.0; }
            if (counts) counts[i] = 0;
            if (rmse) rmse[i] = 0.0;
            if (refit_used) refit_used[i] = 0;
            if (best_trial) best_trial[i] = 0;
            if (best_cost) best_cost[i] = 0;
            if (best_count) best_count[i] = 0;
        }
        return PCREG_OK;
    }
    int32_t *dlab, *dcnt, *dru, *dnp, *dbt, *dbn, *dsmp; double *dcy, *dex, *drm; int64_t* dbc; float* dn; char *ws, *nws;
    const size_t wsb = fit_cylinders_ws_bytes(M, B), nwsb = normals ? 0 : normals_ws_bytes(M, k_normals);
    const size_t ns = samples ? (size_t)P * (size_t)B * 2 : 0;
    TRY(st.take(3 * (size_t)M, &dn));
    TRY(st.take((size_t)M, &dlab));
    TRY(st.take(7 * (size_t)P, &dcy));
    TRY(st.take(2 * (size_t)P, &dex));
    TRY(st.take((size_t)P, &dcnt));
    TRY(st.take((size_t)P, &drm));
    TRY(st.take((size_t)P, &dru));
    TRY(st.take(1, &dnp));
    TRY(st.take((size_t)P, &dbt));
    TRY(st.take((size_t)P, &dbc));
    TRY(st.take((size_t)P, &dbn));
    TRY(st.take(ns, &dsmp));
    TRY(st.take(wsb, &ws));
    TRY(st.take(nwsb, &nws));
    if (normals) TRY(upload_cols(normals, M, ldn, 3, dn, g_stream));
    else TRY(launch_model_normals(v, k_normals, nullptr, dn, M, nullptr, nws, nwsb, g_stream));
    if (samples) PCREG_HIP(hipMemcpyAsync(dsmp, samples, sizeof(int32_t) * ns, hipMemcpyHostToDevice, g_stream));
    TRY(launch_model_fit_cylinders(v, t, min_radius, max_radius, ref_vec, max_angle, dn, M, P, B, min_inliers, seed, samples ? dsmp : nullptr, 1,
                                   dlab, dcy, dex, dcnt, drm, dru, dnp, dbt, dbc, dbn, ws, wsb, g_stream));
    PCREG_HIP(hipMemcpyAsync(labels, dlab, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(cylinders, dcy, sizeof(double) * 7 * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(extents, dex, sizeof(double) * 2 * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(counts, dcnt, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(rmse, drm, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(refit_used, dru, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(n_cylinders, dnp, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    if (best_trial) PCREG_HIP(hipMemcpyAsync(best_trial, dbt, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    if (best_cost) PCREG_HIP(hipMemcpyAsync(best_cost, dbc, sizeof(int64_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    if (best_count) PCREG_HIP(hipMemcpyAsync(best_count, dbn, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}
int pcreg_model_fit_cylinders_f32(pcreg_model* model, float max_distance, float min_radius, float max_radius, const double* ref_vec,
                                  double max_angle, const float* normals, int ldn, int k_normals, int max_cylinders, int n_trials,
                                  int min_inliers, uint64_t seed, const int32_t* samples, int32_t* labels, double* cylinders,
                                  double* extents, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_cylinders,
                                  int32_t* best_trial, int64_t* best_cost, int32_t* best_count) {
    PCREG_ARG(model && n_cylinders &&
              fit_cylinders_args_ok(max_distance, min_radius, max_radius, ref_vec, max_angle, max_cylinders, n_trials, min_inliers));
    PCREG_ARG(normals ? ldn >= model->M : (k_normals >= 3 && k_normals <= kKnnMaxK));
    PCREG_ARG(model->dm != nullptr && model->M < fit_cylinders_max_rows() &&
              ((labels && cylinders && extents && counts && rmse && refit_used) || model->M == 0));
    GUARD();
    Stage st{scratch()};
    return fit_cylinders_on_view(st, model->dm->v, max_distance, min_radius, max_radius, ref_vec, max_angle, normals, ldn, k_normals,
                                 max_cylinders, n_trials, min_inliers, seed, samples, labels, cylinders, extents, counts, rmse, refit_used,
                                 n_cylinders, best_trial, best_cost, best_count);
}
int pcreg_point_fit_cylinders_f32(const float* m, int M, int ldm, float max_distance, float min_radius, float max_radius,
                                  const double* ref_vec, double max_angle, const float* normals, int ldn, int k_normals, int max_cylinders,
                                  int n_trials, int min_inliers, uint64_t seed, const int32_t* samples, int32_t* labels, double* cylinders,
                                  double* extents, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_cylinders,
                                  int32_t* best_trial, int64_t* best_cost, int32_t* best_count) {
    PCREG_ARG(M >= 0 && ldm >= M && M < fit_cylinders_max_rows() && n_cylinders &&
              fit_cylinders_args_ok(max_distance, min_radius, max_radius, ref_vec, max_angle, max_cylinders, n_trials, min_inliers) &&
              (M == 0 || (m && labels && cylinders && extents && counts && rmse && refit_used)));
    PCREG_ARG(normals ? ldn >= M : (k_normals >= 3 && k_normals <= kKnnMaxK));
    GUARD();
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)(M > 0 ? M : 1), &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M > 0 ? M : 1, block);
    TRY(launch_model_prepare(v, g_stream));
    return fit_cylinders_on_view(st, v, max_distance, min_radius, max_radius, ref_vec, max_angle, normals, ldn, k_normals, max_cylinders,
                                 n_trials, min_inliers, seed, samples, labels, cylinders, extents, counts, rmse, refit_used, n_cylinders,
                                 best_trial, best_cost, best_count);
}

// a NaN anywhere in an n x 3 column-major matrix (the host tier's unique refuses it: MATLAB's unique keeps every NaN row apart)
static bool has_nan3(const double* a, int n, int ld) {
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < n; ++i)
            if (a[i + (size_t)c * ld] != a[i + (size_t)c * ld]) return true;
    return false;
}
int pcreg_unique_rows3(const double* A, int n, int ld, int32_t* ia, int* n_unique) {
    PCREG_ARG(n_unique && n >= 0 && ld >= n && (n == 0 || (A && ia)));
    PCREG_ARG(!has_nan3(A, n, ld));
    GUARD();
    *n_unique = 0;
    if (n == 0) return PCREG_OK;
    Stage st{scratch()};
    double* dA; int32_t *dn, *dia, *dnu; char* ws;
    const size_t wsb = unique_rows3_ws_bytes(n);
    TRY(st.take(3 * (size_t)n, &dA));
    TRY(st.take(1, &dn));
    TRY(st.take((size_t)n, &dia));
    TRY(st.take(1, &dnu));
    TRY(st.take(wsb, &ws));
    const int32_t n32 = n;
    TRY(upload_cols(A, n, ld, 3, dA, g_stream));
    PCREG_HIP(hipMemcpyAsync(dn, &n32, sizeof(int32_t), hipMemcpyHostToDevice, g_stream));
    TRY(launch_unique_rows3(dA, dn, n, n, 1, dia, dnu, ws, wsb, g_stream));
    int32_t nu = 0;
    PCREG_HIP(hipMemcpyAsync(ia, dia, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(&nu, dnu, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    *n_unique = nu;
    return PCREG_OK;
}
// pcdownsample(pts, 'gridAverage', step): one upload, the chain, one read of (n_out, info), then one read of the results
int pcreg_downsample_grid_f32(const float* pts, int n, int ld, double step, float* out, int ldo, int32_t* count, int32_t* label, int* n_out) {
    PCREG_ARG(n_out && n >= 0 && ld >= n && ldo >= n && std::isfinite(step) && step > 0.0 && (n == 0 || (pts && out)));
    GUARD();
    *n_out = 0;
    if (n == 0) return PCREG_OK;
    Stage st{scratch()};
    float *dp, *dout; int32_t *dcount, *dlabel, *dword; char* ws;
    const size_t wsb = downsample_grid_ws_bytes(n);
    TRY(st.take(3 * (size_t)n, &dp));
    TRY(st.take(3 * (size_t)n, &dout));
    TRY(st.take(count ? (size_t)n : 0, &dcount));
    TRY(st.take(label ? (size_t)n : 0, &dlabel));
    TRY(st.take(2, &dword));                                    // n_out, info
    TRY(st.take(wsb, &ws));
    TRY(upload_cols(pts, n, ld, 3, dp, g_stream));
    TRY(launch_downsample_grid(dp, n, n, step, dout, n, count ? dcount : nullptr, label ? dlabel : nullptr, dword, dword + 1, ws, wsb, g_stream));
    int32_t word[2] = {0, 0};
    PCREG_HIP(hipMemcpyAsync(word, dword, sizeof word, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    if (word[1] != 0) { set_error("bad argument: the cloud spans 2^21 or more cells of this step along an axis"); return PCREG_E_ARG; }
    const size_t no = (size_t)word[0];
    if (no == 0) return PCREG_OK;                                // no live row: nothing else is written
    PCREG_HIP(hipMemcpy2DAsync(out, sizeof(float) * (size_t)ldo, dout, sizeof(float) * (size_t)n, sizeof(float) * no, 3, hipMemcpyDeviceToHost, g_stream));
    if (count) PCREG_HIP(hipMemcpyAsync(count, dcount, sizeof(int32_t) * no, hipMemcpyDeviceToHost, g_stream));
    if (label) PCREG_HIP(hipMemcpyAsync(label, dlabel, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    *n_out = word[0];
    return PCREG_OK;
}
int pcreg_aggregate_matches(const double* pts1, const double* pts2, int n, int ld, double* out1, double* out2, int ldo, int32_t* ia, int* n_out) {
    PCREG_ARG(n_out && n >= 0 && ld >= n && ldo >= n && (n == 0 || (pts1 && pts2 && out1 && out2)));
    PCREG_ARG(!has_nan3(pts1, n, ld) && !has_nan3(pts2, n, ld));
    GUARD();
    *n_out = 0;
    if (n == 0) return PCREG_OK;
    Stage st{scratch()};
    double *d1, *d2, *o1, *o2; int32_t *dn, *dia, *dno; char* ws;
    const size_t wsb = aggregate_matches_ws_bytes(n);
    TRY(st.take(3 * (size_t)n, &d1));
    TRY(st.take(3 * (size_t)n, &d2));
    TRY(st.take(1, &dn));
    TRY(st.take(3 * (size_t)n, &o1));
    TRY(st.take(3 * (size_t)n, &o2));
    TRY(st.take((size_t)n, &dia));
    TRY(st.take(1, &dno));
    TRY(st.take(wsb, &ws));
    const int32_t n32 = n;
    TRY(upload_cols(pts1, n, ld, 3, d1, g_stream));
    TRY(upload_cols(pts2, n, ld, 3, d2, g_stream));
    PCREG_HIP(hipMemcpyAsync(dn, &n32, sizeof(int32_t), hipMemcpyHostToDevice, g_stream));
    TRY(launch_aggregate_matches(d1, d2, dn, n, n, o1, o2, n, 1, dia, dno, ws, wsb, g_stream));
    int32_t no = 0;
    PCREG_HIP(hipMemcpyAsync(&no, dno, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));                   // the count fixes how many rows come back
    if (no > 0) {
        const size_t w = sizeof(double) * (size_t)no;
        PCREG_HIP(hipMemcpy2DAsync(out1, sizeof(double) * (size_t)ldo, o1, sizeof(double) * (size_t)n, w, 3, hipMemcpyDeviceToHost, g_stream));
        PCREG_HIP(hipMemcpy2DAsync(out2, sizeof(double) * (size_t)ldo, o2, sizeof(double) * (size_t)n, w, 3, hipMemcpyDeviceToHost, g_stream));
        if (ia) PCREG_HIP(hipMemcpyAsync(ia, dia, sizeof(int32_t) * (size_t)no, hipMemcpyDeviceToHost, g_stream));
        PCREG_HIP(hipStreamSynchronize(g_stream));
    }
    *n_out = no;
    return PCREG_OK;
}

int pcreg_match_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm, float thr_abs,
                           float max_ratio, int unique, uint32_t* pairs, int* P) {
    PCREG_ARG(q && m && pairs && P && Q >= 0 && M >= 0 && ldq >= Q && ldm >= M);
    GUARD();
    *P = 0;
    if (Q == 0 || M == 0) return PCREG_OK;
    Stage st{scratch()};
    float* dm; char* block;
    TRY(st.take(3 * (size_t)M, &dm));
    TRY(st.take(model_prep_bytes(M), &block));
    TRY(upload_cols(m, M, ldm, 3, dm, g_stream));
    const ModelView v = model_view(dm, M, M, block);
    TRY(launch_model_prepare(v, g_stream));
    return match_points_on_view(st, v, q, Q, ldq, thr_abs, max_ratio, unique, pairs, P);
}

// the matcher's own buffers, staged in front of the rows it will read: its workspace meets the same slot whether the rows are
// uploaded as they are (matchFeatures) or made by the preprocessing (getMatches)
struct MatchStage { char* ws; size_t wsb; uint32_t* dpairs; double* dmet; int32_t* dcnt; };
static int match_stage(Stage& st, int Q, int M, int Dp, MatchStage* m) {
    m->wsb = match_features_workspace_bytes(Q, M, Dp);
    TRY(st.take(m->wsb, &m->ws));
    TRY(st.take(2 * (size_t)Q, &m->dpairs));
    TRY(st.take((size_t)Q, &m->dmet));
    return st.take(1, &m->dcnt);
}
// the matcher on prepared rows dS [Q][Dp], dM [M][Dp] (column-major, ld = rows; normalized in place unless prenormalized) -> pairs on the host
static int match_rows(const MatchStage& m, double* dS, int Q, double* dM, int M, int Dp, const pcreg_match_opts* o, uint32_t* pairs, double* metric, int* P) {
    if (!o->prenormalized) {
        TRY(launch_normalize_rows2(dS, Q, Q, dM, M, M, Dp, g_stream));
    }
    TRY(launch_match_features(dS, Q, Q, dM, M, M, Dp, *o, m.dpairs, metric ? m.dmet : nullptr, m.dcnt, m.ws, m.wsb, g_stream));
    int32_t np = 0;
    PCREG_HIP(hipMemcpyAsync(&np, m.dcnt, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    if (np > 0) {
        PCREG_HIP(hipMemcpy(pairs, m.dpairs, sizeof(uint32_t) * 2 * (size_t)np, hipMemcpyDeviceToHost));
        if (metric) PCREG_HIP(hipMemcpy(metric, m.dmet, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost));
    }
    *P = np;
    return PCREG_OK;
}

// raw descriptor matrices on the device (column-major, ld = rows) -> getMatches.m:22-56 -> pairs on the host.  rawS / rawM are not
// modified: the preprocessing writes its own copies.
static int match_dev_raw(Stage& st, const double* rawS, int Q, const double* rawM, int M, int D, const pcreg_match_opts* o, uint32_t* pairs, double* metric, int* P) {
    *P = 0;
    if (Q == 0 || M == 0) return PCREG_OK;
    const int Dp = D + (o->unnormalize ? 1 : 0);
    MatchStage m;
    double *dS, *dM, *pws;
    const size_t pwn = (size_t)Q + M + 1;
    TRY(match_stage(st, Q, M, Dp, &m));
    TRY(st.take((size_t)Q * Dp, &dS));
    TRY(st.take((size_t)M * Dp, &dM));
    TRY(st.take(pwn, &pws));
    TRY(launch_preprocess(rawS, Q, Q, rawM, M, M, D, *o, dS, dM, pws, sizeof(double) * pwn, g_stream));
    return match_rows(m, dS, Q, dM, M, Dp, o, pairs, metric, P);
}

static int match_host(const double* f1, int Q, int ld1, const double* f2, int M, int ld2, int D,
                      const pcreg_match_opts* o, bool preprocess, uint32_t* pairs, double* metric, int* P) {
    *P = 0;
    if (Q == 0 || M == 0) return PCREG_OK;
    Stage st{scratch()};
    double *dS, *dM;                                  // the raw matrices (getMatches) or the rows themselves (matchFeatures)
    TRY(st.take((size_t)Q * D, &dS));
    TRY(st.take((size_t)M * D, &dM));
    TRY(upload_cols(f1, Q, ld1, D, dS, g_stream));
    TRY(upload_cols(f2, M, ld2, D, dM, g_stream));
    if (preprocess) return match_dev_raw(st, dS, Q, dM, M, D, o, pairs, metric, P);
    MatchStage m;
    TRY(match_stage(st, Q, M, D, &m));
    return match_rows(m, dS, Q, dM, M, D, o, pairs, metric, P);
}

// ---- resident descriptor sets (host tier): one surface set against hundreds of row subsets of one model set
// (completeExperimentFast.m:101-150) without re-uploading ~28 MB of doubles per sphere
// The powered rows + row scalars of a MODEL of the segmented matcher (SegPreparedModel), valid for the getMatches options they
// were made with: made at the first use, remade when the options change (caller holds the library lock).
struct PreparedRows { double* P = nullptr; int cm = -1; double factor = 0.0; };
static int prepared_rows(PreparedRows& c, const double* rows, int n, int D, const pcreg_match_opts& o, SegPreparedModel* out);
struct pcreg_desc_set {
    double* d; int n, D;            // n x D column-major on the device (ld = n), as uploaded
    double* rows;                   // the dense row-major copy the segmented matcher reads, made at its first use
    PreparedRows prep;              // the set as a model of the segmented matcher
};

__global__ void gather_cols_kernel(const double* __restrict__ src, int n_src, int D, const int32_t* __restrict__ rows, int n, double* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, d = blockIdx.y;
    if (i < n) dst[i + (size_t)d * n] = src[rows[i] + (size_t)d * n_src];
}

int pcreg_desc_set_create(const double* desc, int n, int ld, int D, pcreg_desc_set** set) {
    PCREG_ARG(set != nullptr && n >= 0 && D >= 1 && ld >= n && (n == 0 || desc != nullptr));
    GUARD();
    *set = nullptr;
    double* d = nullptr;
    PCREG_HIP(hipMalloc((void**)&d, sizeof(double) * (size_t)(n > 0 ? n : 1) * D));
    int rc = upload_cols(desc, n, ld, D, d, g_stream);
    if (!rc && hipStreamSynchronize(g_stream) != hipSuccess) { set_error("descriptor upload failed"); rc = PCREG_E_HIP; }
    if (rc) { (void)hipFree(d); return rc; }
    *set = new pcreg_desc_set{d, n, D, nullptr, {}};
    return PCREG_OK;
}
int pcreg_desc_set_destroy(pcreg_desc_set* set) {
    if (!set) return PCREG_OK;
    std::lock_guard<std::mutex> lock(g_mu);
    (void)hipDeviceSynchronize();
    (void)hipFree(set->d);
    if (set->rows) (void)hipFree(set->rows);
    if (set->prep.P) (void)hipFree(set->prep.P);
    delete set;
    return PCREG_OK;
}
int pcreg_desc_set_size(const pcreg_desc_set* set, int* n, int* D) {
    PCREG_ARG(set && n && D);
    *n = set->n; *D = set->D;
    return PCREG_OK;
}
int pcreg_get_matches_on_sets(const pcreg_desc_set* surface, const pcreg_desc_set* model, const int32_t* model_rows, int n_rows,
                              const pcreg_match_opts* par, uint32_t* pairs, double* metric, int* P) {
    PCREG_ARG(surface && model && par && pairs && P && surface->D == model->D && n_rows >= 0 && (model_rows || n_rows == 0));
    PCREG_ARG(par->metric == PCREG_METRIC_SAD || par->metric == PCREG_METRIC_SSD);
    GUARD();
    *P = 0;
    const int Q = surface->n, D = surface->D;
    if (model_rows) for (int k = 0; k < n_rows; ++k) PCREG_ARG(model_rows[k] >= 0 && model_rows[k] < model->n);
    Stage st{scratch()};
    double* rawM; int32_t* drows;                     // taken (empty) without a row list too: the matcher's buffers keep their slots
    TRY(st.take(model_rows ? (size_t)n_rows * D : 0, &rawM));
    TRY(st.take(model_rows ? (size_t)n_rows : 0, &drows));
    if (!model_rows) return match_dev_raw(st, surface->d, Q, model->d, model->n, D, par, pairs, metric, P);      // descModel(:, :)
    if (Q == 0 || n_rows == 0) return PCREG_OK;
    PCREG_HIP(hipMemcpyAsync(drows, model_rows, sizeof(int32_t) * (size_t)n_rows, hipMemcpyHostToDevice, g_stream));
    hipLaunchKernelGGL(gather_cols_kernel, dim3((n_rows + 255) / 256, D), dim3(256), 0, g_stream, model->d, model->n, D, (const int32_t*)drows, n_rows, rawM);   // descModel(rows, :)
    PCREG_HIP(hipGetLastError());
    return match_dev_raw(st, surface->d, Q, rawM, n_rows, D, par, pairs, metric, P);
}

int pcreg_match_features(const double* f1, int Q, int ld1, const double* f2, int M, int ld2, int D,
                         const pcreg_match_opts* opts, uint32_t* pairs, double* metric, int* P) {
    PCREG_ARG(f1 && f2 && opts && pairs && P && Q >= 0 && M >= 0 && D >= 1 && ld1 >= Q && ld2 >= M);
    PCREG_ARG(opts->metric == PCREG_METRIC_SAD || opts->metric == PCREG_METRIC_SSD);
    GUARD();
    return match_host(f1, Q, ld1, f2, M, ld2, D, opts, false, pairs, metric, P);
}

int pcreg_get_matches(const double* descSurface, int Q, int ldS, const double* descModel, int M, int ldM, int D,
                      const pcreg_match_opts* par, uint32_t* pairs, double* metric, int* P) {
    PCREG_ARG(descSurface && descModel && par && pairs && P && Q >= 0 && M >= 0 && D >= 1 && ldS >= Q && ldM >= M);
    PCREG_ARG(par->metric == PCREG_METRIC_SAD || par->metric == PCREG_METRIC_SSD);
    GUARD();
    return match_host(descSurface, Q, ldS, descModel, M, ldM, D, par, true, pairs, metric, P);
}

// getLocalPoints.m:8-35, host tier.  *n_out = rows returned; 0 is MATLAB's [] (a gate failed, or nothing inside)
int pcreg_get_local_points(const double* pts, int N, int ld, double R, const double c[3], double min_points, double max_points,
                           int single_mode, double* pts_sphere, double* dists, int* n_out) {
    PCREG_ARG(pts && c && pts_sphere && n_out && N >= 0 && ld >= N && single_mode >= 0 && single_mode <= 2);
    GUARD();
    *n_out = 0;
    if (N == 0) return PCREG_OK;
    Stage st{scratch()};
    double *dp, *dout, *dd; int32_t* dt; char* ws;
    TRY(st.take(3 * (size_t)N, &dp));
    TRY(st.take(3 * (size_t)N, &dout));
    TRY(st.take((size_t)N, &dd));
    TRY(st.take(2, &dt));
    TRY(st.take(local_points_workspace_bytes(N), &ws));
    TRY(upload_cols(pts, N, ld, 3, dp, g_stream));
    TRY(launch_local_points(dp, N, N, R, c, single_mode, dout, N, dd, dt, ws, local_points_workspace_bytes(N), g_stream));
    int32_t tot[2] = {0, 0};
    PCREG_HIP(hipMemcpyAsync(tot, dt, sizeof(tot), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    // :17 the box count against min_points, :31 the sphere count against both gates (comparisons as MATLAB makes them: inf allowed)
    if ((double)tot[0] < min_points || (double)tot[1] < min_points || (double)tot[1] > max_points || tot[1] == 0) return PCREG_OK;
    const size_t n = (size_t)tot[1];
    for (int k = 0; k < 3; ++k)
        PCREG_HIP(hipMemcpyAsync(pts_sphere + (size_t)k * n, dout + (size_t)k * N, sizeof(double) * n, hipMemcpyDeviceToHost, g_stream));
    if (dists) PCREG_HIP(hipMemcpyAsync(dists, dd, sizeof(double) * n, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    *n_out = tot[1];
    return PCREG_OK;
}

// ---- the pair lists of a segmented call on their way back --------------------------------------------------------------------
// The device holds [S][vs][2] with the first n_pairs[z] pairs of row z valid (vs = the surface's rows: Unique's capacity); a sphere
// keeps a few hundred of its ~2000 slots, so copying the array as it is moved 5 MB of mostly nothing into pageable memory (~0.5 ms
// of the 7 ms sweep).  Now: the counts go to a page-locked buffer FIRST (begin: right behind the matcher, in front of whatever the
// caller launches next), the host waits for them alone (enqueue), packs the columns that hold pairs on the device and fetches that
// block through page-locked memory; finish() deals it into the caller's array (same layout; slots past n_pairs[z] are not written).
static int pinned_get(int k, size_t bytes, void** out) {
    if (g_pin_bytes[k] < bytes) {
        if (g_pin[k]) { PCREG_HIP(hipHostFree(g_pin[k])); g_pin[k] = nullptr; g_pin_bytes[k] = 0; }
        const size_t want = align_up(bytes + bytes / 4, 4096);
        PCREG_HIP(hipHostMalloc(&g_pin[k], want, hipHostMallocDefault));
        g_pin_bytes[k] = want;
    }
    *out = g_pin[k];
    return PCREG_OK;
}
struct PairFetch { int32_t* h_np = nullptr; void* h_packed = nullptr; int m = 0; bool whole = false; };
static int pairs_fetch_begin(const int32_t* dn, int S, PairFetch& f) {
    void* h;
    TRY(pinned_get(0, sizeof(int32_t) * (size_t)S, &h));
    f.h_np = (int32_t*)h;
    if (!g_pairs_ev) PCREG_HIP(hipEventCreateWithFlags(&g_pairs_ev, hipEventDisableTiming));
    PCREG_HIP(hipMemcpyAsync(f.h_np, dn, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipEventRecord(g_pairs_ev, g_stream));
    return PCREG_OK;
}
static int pairs_fetch_enqueue(Stage& st, PairFetch& f, const uint32_t* dp, size_t vs, int S, uint32_t* pairs_all) {
    PCREG_HIP(hipEventSynchronize(g_pairs_ev));
    int m = 0;
    for (int z = 0; z < S; ++z) m = std::max(m, (int)f.h_np[z]);
    f.m = m;
    if (m == 0) return PCREG_OK;
    if ((size_t)m * 2 > vs) {                         // most slots hold pairs: the array as it is
        f.whole = true;
        PCREG_HIP(hipMemcpyAsync(pairs_all, dp, sizeof(uint32_t) * (size_t)S * vs * 2, hipMemcpyDeviceToHost, g_stream));
        return PCREG_OK;
    }
    char* packed;
    const size_t row = sizeof(uint32_t) * 2 * (size_t)m;
    TRY(st.take(row * (size_t)S, &packed));
    TRY(pinned_get(1, row * (size_t)S, &f.h_packed));
    PCREG_HIP(hipMemcpy2DAsync(packed, row, dp, sizeof(uint32_t) * 2 * vs, row, (size_t)S, hipMemcpyDeviceToDevice, g_stream));
    PCREG_HIP(hipMemcpyAsync(f.h_packed, packed, row * (size_t)S, hipMemcpyDeviceToHost, g_stream));
    return PCREG_OK;
}
// after the stream has been synchronised
static void pairs_fetch_finish(const PairFetch& f, size_t vs, int S, uint32_t* pairs_all, int32_t* n_pairs) {
    for (int z = 0; z < S; ++z) {
        n_pairs[z] = f.h_np[z];
        if (!f.whole && f.m > 0 && f.h_np[z] > 0)
            memcpy(pairs_all + (size_t)z * vs * 2, (const char*)f.h_packed + sizeof(uint32_t) * 2 * (size_t)f.m * z, sizeof(uint32_t) * 2 * (size_t)f.h_np[z]);
    }
}

// the set's rows as the segmented matcher wants them (dense row-major), transposed once per set (caller holds the library lock)
static int desc_set_rows(const pcreg_desc_set* cs, const double** out) {
    pcreg_desc_set* s = const_cast<pcreg_desc_set*>(cs);
    if (!s->rows) {
        double* r = nullptr;
        PCREG_HIP(hipMalloc((void**)&r, sizeof(double) * (size_t)(s->n > 0 ? s->n : 1) * s->D));
        const int rc = s->n > 0 ? launch_transpose_rows(s->d, s->n, s->n, s->D, r, g_stream) : PCREG_OK;
        if (rc) { (void)hipFree(r); return rc; }
        s->rows = r;
    }
    *out = s->rows;
    return PCREG_OK;
}
static int prepared_rows(PreparedRows& c, const double* rows, int n, int D, const pcreg_match_opts& o, SegPreparedModel* out) {
    const size_t r_off = (size_t)(n > 0 ? n : 1) * D;
    const bool have = c.P && c.cm == o.change_metric && (!o.change_metric || c.factor == o.metric_factor);
    if (!have) {
        if (!c.P) PCREG_HIP(hipMalloc((void**)&c.P, segmented_prepared_model_bytes(n, D)));
        c.cm = -1;                                               // not valid until the launch below has been enqueued
        TRY(launch_segmented_prepare_model(rows, n, D, o, c.P, c.P + r_off, g_stream));
        c.cm = o.change_metric; c.factor = o.metric_factor;
    }
    *out = SegPreparedModel{c.P, c.P + r_off, n, D, c.cm, c.factor};
    return PCREG_OK;
}
// the set as the segmented matcher's prepared model for these options
static int desc_set_prepared(const pcreg_desc_set* cs, const pcreg_match_opts& o, SegPreparedModel* out) {
    const double* rows;
    TRY(desc_set_rows(cs, &rows));
    return prepared_rows(const_cast<pcreg_desc_set*>(cs)->prep, rows, cs->n, cs->D, o, out);
}

// The segment list of a segmented call: offsets from 0, no negative length, every row inside the model.  *tot = 0 on return:
// nothing to match, n_pairs is all zero already.
static int check_segments(const int32_t* seg_rows, const int32_t* seg_off, int S, int Q, int VM, int32_t* n_pairs, int* n_max, int* tot) {
    PCREG_ARG(seg_off[0] == 0);
    *n_max = 0;
    for (int z = 0; z < S; ++z) { const int n = seg_off[z + 1] - seg_off[z]; PCREG_ARG(n >= 0); if (n > *n_max) *n_max = n; }
    *tot = seg_off[S];
    PCREG_ARG(*tot == 0 || seg_rows);
    for (int k = 0; k < *tot; ++k) PCREG_ARG(seg_rows[k] >= 0 && seg_rows[k] < VM);
    if (Q == 0 || VM == 0 || *tot == 0) { for (int z = 0; z < S; ++z) n_pairs[z] = 0; *tot = 0; }
    return PCREG_OK;
}
// the segmented matcher on dense rows rS [Q][D], rM [VM][D] (on the model's prepared rows where the set keeps them) and its
// pair lists back on the host
static int segmented_run(Stage& st, const double* rS, int Q, const double* rM, int VM, int D, const int32_t* seg_rows, const int32_t* seg_off,
                         int S, int tot, int n_max, const pcreg_match_opts* par, const pcreg_desc_set* model_set, uint32_t* pairs_all,
                         int32_t* n_pairs) {
    const size_t q = (size_t)Q;
    int32_t *dr, *doff, *dn; uint32_t* dp; char* ws;
    TRY(st.take((size_t)tot, &dr));
    TRY(st.take((size_t)S + 1, &doff));
    TRY(st.take((size_t)S * q * 2, &dp));
    TRY(st.take((size_t)S, &dn));
    const size_t wsb = get_matches_segmented_workspace_bytes(Q, VM, D, S, tot, n_max);
    TRY(st.take(wsb, &ws));
    PCREG_HIP(hipMemcpyAsync(dr, seg_rows, sizeof(int32_t) * (size_t)tot, hipMemcpyHostToDevice, g_stream));
    PCREG_HIP(hipMemcpyAsync(doff, seg_off, sizeof(int32_t) * ((size_t)S + 1), hipMemcpyHostToDevice, g_stream));
    SegPreparedModel prep;
    if (model_set) TRY(desc_set_prepared(model_set, *par, &prep));
    TRY(launch_get_matches_segmented(rS, Q, rM, VM, D, dr, doff, S, tot, n_max, *par, dp, nullptr, dn, ws, wsb, g_stream, model_set ? &prep : nullptr));
    PairFetch pf;
    TRY(pairs_fetch_begin(dn, S, pf));
    TRY(pairs_fetch_enqueue(st, pf, dp, q, S, pairs_all));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    pairs_fetch_finish(pf, q, S, pairs_all, n_pairs);
    return PCREG_OK;
}

// getMatches for S row subsets of one model set, host tier (the parfor of completeExperimentFast.m:131-149 as ONE call)
int pcreg_get_matches_segmented(const double* descSurface, int Q, int ldS, const double* descModel, int VM, int ldM, int D,
                                const int32_t* seg_rows, const int32_t* seg_off, int S, const pcreg_match_opts* par,
                                uint32_t* pairs_all, int32_t* n_pairs) {
    PCREG_ARG(descSurface && descModel && seg_off && par && pairs_all && n_pairs && Q >= 0 && VM >= 0 && D >= 1 && S >= 0 && ldS >= Q && ldM >= VM);
    PCREG_ARG(S <= 65535);
    if (par->metric != PCREG_METRIC_SAD) { set_error("pcreg_get_matches_segmented: Metric must be SAD (call pcreg_get_matches per segment for SSD)"); return PCREG_E_ARG; }
    GUARD();
    if (S == 0) return PCREG_OK;
    int n_max, tot;
    TRY(check_segments(seg_rows, seg_off, S, Q, VM, n_pairs, &n_max, &tot));
    if (tot == 0) return PCREG_OK;
    const size_t q = (size_t)Q, vm = (size_t)VM;
    Stage st{scratch()};
    double *fS, *fM, *rS, *rM;
    TRY(st.take(q * D, &fS));
    TRY(st.take(vm * D, &fM));
    TRY(st.take(q * D, &rS));
    TRY(st.take(vm * D, &rM));
    TRY(upload_cols(descSurface, Q, ldS, D, fS, g_stream));
    TRY(upload_cols(descModel, VM, ldM, D, fM, g_stream));
    TRY(launch_transpose_rows(fS, Q, Q, D, rS, g_stream));          // MATLAB's n x D -> dense rows
    TRY(launch_transpose_rows(fM, VM, VM, D, rM, g_stream));
    return segmented_run(st, rS, Q, rM, VM, D, seg_rows, seg_off, S, tot, n_max, par, nullptr, pairs_all, n_pairs);
}

int pcreg_get_matches_segmented_on_sets(const pcreg_desc_set* surface, const pcreg_desc_set* model, const int32_t* seg_rows,
                                        const int32_t* seg_off, int S, const pcreg_match_opts* par, uint32_t* pairs_all, int32_t* n_pairs) {
    PCREG_ARG(surface && model && seg_off && par && pairs_all && n_pairs && S >= 0 && surface->D == model->D);
    PCREG_ARG(S <= 65535);
    if (par->metric != PCREG_METRIC_SAD) { set_error("pcreg_get_matches_segmented_on_sets: Metric must be SAD (call pcreg_get_matches_on_sets per segment for SSD)"); return PCREG_E_ARG; }
    GUARD();
    if (S == 0) return PCREG_OK;
    const int Q = surface->n, VM = model->n, D = surface->D;
    int n_max, tot;
    TRY(check_segments(seg_rows, seg_off, S, Q, VM, n_pairs, &n_max, &tot));
    if (tot == 0) return PCREG_OK;
    const double *rS, *rM;
    TRY(desc_set_rows(surface, &rS));
    TRY(desc_set_rows(model, &rM));
    Stage st{scratch()};
    double* none;                                     // the four matrices pcreg_get_matches_segmented stages live in the sets: their slots
    for (int k = 0; k < 4; ++k) TRY(st.take(0, &none));      // are taken empty, so that the run's pairs and workspace meet the same slots
    return segmented_run(st, rS, Q, rM, VM, D, seg_rows, seg_off, S, tot, n_max, par, model, pairs_all, n_pairs);
}

// n x 3 column-major host doubles -> [n][3] on the device (what the sphere kernels and the gather read)
static int upload_points_aos(const double* host, int n, int ld, double* cols_tmp, double* aos, hipStream_t st) {
    if (n <= 0) return PCREG_OK;
    TRY(upload_cols(host, n, ld, 3, cols_tmp, st));
    return launch_transpose_rows(cols_tmp, n, n, 3, aos, st);
}
int pcreg_sphere_counts(const double* featModel, int VM, int ldM, const double* centres, int S, int ldC, double R, int32_t* counts) {
    PCREG_ARG(VM >= 0 && S >= 0 && ldM >= VM && ldC >= S && (VM == 0 || featModel) && (S == 0 || (centres && counts)));
    GUARD();
    if (S == 0) return PCREG_OK;
    if (VM == 0) { for (int i = 0; i < S; ++i) counts[i] = 0; return PCREG_OK; }
    Stage st{scratch()};
    double *tmp, *fm, *tc, *cen; int32_t* cnt;
    TRY(st.take(3 * (size_t)VM, &tmp));
    TRY(st.take(3 * (size_t)VM, &fm));
    TRY(st.take(3 * (size_t)S, &tc));
    TRY(st.take(3 * (size_t)S, &cen));
    TRY(st.take((size_t)S, &cnt));
    TRY(upload_points_aos(featModel, VM, ldM, tmp, fm, g_stream));
    TRY(upload_points_aos(centres, S, ldC, tc, cen, g_stream));
    TRY(launch_sphere_counts(fm, VM, cen, S, R, cnt, g_stream));
    PCREG_HIP(hipMemcpyAsync(counts, cnt, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}

// ---- the sphere sweep (completeExperimentFast.m:46-225) at the host tier ------------------------------------------------------
// no host array is freed under a pending copy: whatever way a call leaves, the stream is drained first (unless it just was)
struct DrainAtExit { bool armed = true; ~DrainAtExit() { if (armed) (void)hipStreamSynchronize(g_stream); } };

// a sweep's spheres: the caller's per-sphere counts and the segment tables made of them, off [S + 1] (rows in front of sphere i), roff
// the same as int64
struct SphereSegs { const int32_t* num_desc; int S; std::vector<int32_t> off; std::vector<int64_t> roff; int n_max, tot; };
static int sphere_segs(const int32_t* num_desc, int S, int VM, SphereSegs* g) {
    g->num_desc = num_desc; g->S = S; g->n_max = 0;
    g->off.assign((size_t)S + 1, 0); g->roff.assign((size_t)S, 0);
    for (int i = 0; i < S; ++i) {
        PCREG_ARG(num_desc[i] >= 0 && num_desc[i] <= VM && (long long)g->off[i] + num_desc[i] < 2147483647LL);
        g->off[i + 1] = g->off[i] + num_desc[i]; g->roff[i] = g->off[i]; g->n_max = std::max(g->n_max, num_desc[i]);
    }
    g->tot = g->off[S];
    return PCREG_OK;
}
// where a sphere head leaves the model side: the caller's segment tables and gathered keypoints, and the row lists the head stages
struct SphereDst { int32_t* off; int64_t* roff; double* feat_all; int32_t* rows; };
// The model side of a sweep (:52-125) behind the upload of the model keypoints fm [VM][3]: the centres go up, the segment tables to
// d->off / d->roff, every sphere's row list to d->rows and its keypoints to d->feat_all.  The counts and the lists come back and the
// counts are held against num_desc BEFORE anything reads the lists: the select clips at a segment's capacity, so behind a count that
// is too large the tail of the segment is unwritten.  The stream is synchronised on return (g's tables may go).  `who`: the public entry.
static int sphere_head(Stage& st, const char* who, const SphereSegs& g, const double* fm, int VM, const double* centres, int ldC, double R_desc,
                       SphereDst* d, int32_t* model_rows) {
    const int S = g.S;
    double *tc, *cen; int32_t* nsel;
    TRY(st.take(3 * (size_t)S, &tc));
    TRY(st.take(3 * (size_t)S, &cen));
    TRY(st.take((size_t)S, &nsel));
    TRY(st.take((size_t)g.tot, &d->rows));
    std::vector<int32_t> h_nsel((size_t)S);
    DrainAtExit drain;
    TRY(upload_points_aos(centres, S, ldC, tc, cen, g_stream));
    PCREG_HIP(hipMemcpyAsync(d->off, g.off.data(), sizeof(int32_t) * ((size_t)S + 1), hipMemcpyHostToDevice, g_stream));
    PCREG_HIP(hipMemcpyAsync(d->roff, g.roff.data(), sizeof(int64_t) * (size_t)S, hipMemcpyHostToDevice, g_stream));
    TRY(launch_sphere_select_batched(fm, VM, cen, S, R_desc, d->off, d->rows, d->feat_all, nsel, g_stream));
    PCREG_HIP(hipMemcpyAsync(h_nsel.data(), nsel, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(model_rows, d->rows, sizeof(int32_t) * (size_t)g.tot, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    drain.armed = false;
    for (int i = 0; i < S; ++i)
        if (h_nsel[i] != g.num_desc[i]) { set_error("%s: num_desc[%d] = %d, but the sphere holds %d keypoints (pass pcreg_sphere_counts' values)", who, i, g.num_desc[i], h_nsel[i]); return PCREG_E_ARG; }
    return PCREG_OK;
}

// The surface side of a sweep.  Its buffers are staged first by both entries, so that each meets the same slot with and without
// a sphere model; the pairs, the counts and the matcher's workspace come behind six others, in the slots segmented_run gives
// them in pcreg_get_matches_segmented{,_on_sets}.  tmp: column-major temporary of tmp_rows keypoints.
struct SweepStage {
    double *tmp, *fs; uint32_t* dp; int32_t* dn; char* ws; size_t wsb;
    int32_t* tidx; double* p12; pcreg_dev_ransac_result* res; int32_t* inl; char* rws; size_t rwsb;      // tidx: trial_idx [S] | offsets [S + 1] | n_trials
};
static int sweep_stage(Stage& st, int S, int VS, int tmp_rows, size_t wsb, const pcreg_ransac_opts* coef, SweepStage* b) {
    const size_t vs = (size_t)VS, ld = (size_t)S * vs;
    b->wsb = wsb; b->rwsb = ransac_workspace_bytes(coef->iterNum, S, VS);
    TRY(st.take(3 * (size_t)tmp_rows, &b->tmp));
    TRY(st.take(3 * vs, &b->fs));
    TRY(st.take(3 * (size_t)S + 2, &b->tidx));
    TRY(st.take((size_t)S, &b->res));
    TRY(st.take(ld, &b->inl));
    TRY(st.take(b->rwsb, &b->rws));
    TRY(st.take((size_t)S * vs * 2, &b->dp));
    TRY(st.take((size_t)S, &b->dn));
    TRY(st.take(b->wsb, &b->ws));
    return st.take(6 * ld, &b->p12);
}
// :166-216 behind the matcher (pairs in b.dp, counts in b.dn): the putative threshold, the trial spheres' correspondences, one
// batched ransac (registration t: seed + t), the pair lists and the trials' results back on the host
static int sweep_tail(Stage& st, const SweepStage& b, int S, int VS, const double* feat_all, const int64_t* roff, int putative_thresh,
                      const pcreg_ransac_opts* coef, uint32_t* pairs_all, int32_t* n_pairs, int32_t* trial, int* n_trials, double* T,
                      int32_t* num_success, int32_t* max_inliers, int32_t* failed) {
    const size_t vs = (size_t)VS, ld = (size_t)S * vs;
    int32_t *toff = b.tidx + S, *nt = b.tidx + 2 * (size_t)S + 1;
    TRY(launch_sweep_plan(b.dn, S, putative_thresh, b.tidx, toff, nt, g_stream));
    double *p1 = b.p12, *p2 = b.p12 + 3 * ld;
    PCREG_HIP(hipMemsetAsync(b.p12, 0, sizeof(double) * 6 * ld, g_stream));
    TRY(launch_sweep_gather(b.dp, VS, b.dn, b.tidx, toff, nt, S, b.fs, feat_all, roff, p1, p2, (int)ld, g_stream));
    PairFetch pf;
    TRY(pairs_fetch_begin(b.dn, S, pf));          // the counts leave in front of the RANSAC launch; the lists are packed while it runs
    PCREG_HIP(hipMemsetAsync(b.res, 0, sizeof(pcreg_dev_ransac_result) * (size_t)S, g_stream));
    TRY(launch_ransac(p1, p2, (int)ld, toff, nullptr, VS, S, *coef, nullptr, b.res, b.inl, nullptr, nullptr, b.rws, b.rwsb, g_stream));
    std::vector<int32_t> h_tr((size_t)S);
    std::vector<pcreg_dev_ransac_result> h_res((size_t)S);
    int32_t h_nt = 0;
    TRY(pairs_fetch_enqueue(st, pf, b.dp, vs, S, pairs_all));
    PCREG_HIP(hipMemcpyAsync(h_tr.data(), b.tidx, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(&h_nt, nt, sizeof(int32_t), hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(h_res.data(), b.res, sizeof(pcreg_dev_ransac_result) * (size_t)S, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    pairs_fetch_finish(pf, vs, S, pairs_all, n_pairs);
    *n_trials = h_nt;
    for (int t = 0; t < h_nt; ++t) {
        trial[t] = h_tr[t];
        const pcreg_dev_ransac_result& r = h_res[t];
        for (int k = 0; k < 16; ++k) T[(size_t)t * 16 + k] = r.failed ? 0.0 : r.T[k];
        num_success[t] = r.num_success; max_inliers[t] = r.max_inliers; failed[t] = r.failed;
    }
    return PCREG_OK;
}

int pcreg_sphere_sweep(const pcreg_desc_set* surface, const pcreg_desc_set* model, const double* featSurface, int ldS, const double* featModel, int ldM,
                       const double* centres, int S, int ldC, const int32_t* num_desc, double R_desc, const pcreg_match_opts* par, int putative_thresh,
                       const pcreg_ransac_opts* coef, int32_t* model_rows, uint32_t* pairs_all, int32_t* n_pairs, int32_t* trial, int* n_trials,
                       double* T, int32_t* num_success, int32_t* max_inliers, int32_t* failed) {
    PCREG_ARG(surface && model && featSurface && featModel && par && coef && n_trials && S >= 0 && surface->D == model->D);
    PCREG_ARG(S == 0 || (centres && num_desc && model_rows && pairs_all && n_pairs && trial && T && num_success && max_inliers && failed));
    PCREG_ARG(S <= 65535 && ldC >= S && ldS >= surface->n && ldM >= model->n && coef->minPtNum == 3 && coef->iterNum >= 1);
    if (par->metric != PCREG_METRIC_SAD) { set_error("pcreg_sphere_sweep: Metric must be SAD (every driver of the reference uses it)"); return PCREG_E_ARG; }
    GUARD();
    *n_trials = 0;
    if (S == 0) return PCREG_OK;
    const int VS = surface->n, VM = model->n, D = surface->D;
    SphereSegs g;
    TRY(sphere_segs(num_desc, S, VM, &g));
    const int tot = g.tot;
    if (VS == 0 || VM == 0 || tot == 0) { for (int i = 0; i < S; ++i) n_pairs[i] = 0; return PCREG_OK; }
    const size_t ld = (size_t)S * (size_t)VS;
    PCREG_ARG(ld <= 0x7FFFFFFFull);                              // the packed correspondences are indexed with int
    Stage st{scratch()};
    SweepStage b;
    TRY(sweep_stage(st, S, VS, std::max(VM, VS), get_matches_segmented_workspace_bytes(VS, VM, D, S, tot, g.n_max), coef, &b));
    double* fm; SphereDst d;
    TRY(st.take(3 * (size_t)VM, &fm));
    TRY(st.take((size_t)S + 1, &d.off));
    TRY(st.take((size_t)S, &d.roff));
    TRY(st.take(3 * (size_t)tot, &d.feat_all));
    const double *rS, *rM;
    TRY(desc_set_rows(surface, &rS));
    TRY(desc_set_rows(model, &rM));
    // :52-125: the keypoints, the spheres' row lists and their keypoints back to back
    TRY(upload_points_aos(featModel, VM, ldM, b.tmp, fm, g_stream));
    TRY(upload_points_aos(featSurface, VS, ldS, b.tmp, b.fs, g_stream));
    TRY(sphere_head(st, "pcreg_sphere_sweep", g, fm, VM, centres, ldC, R_desc, &d, model_rows));
    // :131-149: getMatches of the surface against every sphere's rows
    SegPreparedModel prep;
    TRY(desc_set_prepared(model, *par, &prep));
    TRY(launch_get_matches_segmented(rS, VS, rM, VM, D, d.rows, d.off, S, tot, g.n_max, *par, b.dp, nullptr, b.dn, b.ws, b.wsb, g_stream, &prep));
    return sweep_tail(st, b, S, VS, d.feat_all, d.roff, putative_thresh, coef, pairs_all, n_pairs, trial, n_trials, T, num_success, max_inliers, failed);
}

// ---- the sphere sweep's model side as a handle: one model, many surfaces ----------------------------------------------------
// Everything of pcreg_sphere_sweep that does not depend on the surface: the spheres' row lists and gathered keypoints, the model
// set restricted to the union of those rows (the lists renumbered into it) and, per set of getMatches options, its powered rows.
struct pcreg_sphere_model {
    int S, VMu, D, tot, n_max;
    int32_t *seg_off, *rows_u; int64_t* roff; double *feat_all, *desc_u;
    PreparedRows prep;
};
static void sphere_model_free(pcreg_sphere_model* m) {
    if (!m) return;
    void* p[] = {m->seg_off, m->rows_u, m->roff, m->feat_all, m->desc_u, m->prep.P};
    for (void* q : p) if (q) (void)hipFree(q);
    delete m;
}
int pcreg_sphere_model_create(const pcreg_desc_set* model, const double* featModel, int ldM, const double* centres, int S, int ldC,
                              const int32_t* num_desc, double R_desc, int32_t* model_rows, pcreg_sphere_model** out) {
    PCREG_ARG(model && featModel && out && S >= 0 && S <= 65535 && ldC >= S && ldM >= model->n && (S == 0 || (centres && num_desc && model_rows)));
    GUARD();
    *out = nullptr;
    const int VM = model->n, D = model->D;
    SphereSegs g;
    TRY(sphere_segs(num_desc, S, VM, &g));
    const int tot = g.tot;
    pcreg_sphere_model* m = new pcreg_sphere_model{S, 0, D, tot, g.n_max, nullptr, nullptr, nullptr, nullptr, nullptr, {}};
    auto fail = [&](int rc) { sphere_model_free(m); return rc; };
    if (S == 0 || tot == 0 || VM == 0) { *out = m; return PCREG_OK; }
    int rc = PCREG_OK;
    if (hipMalloc((void**)&m->seg_off, sizeof(int32_t) * ((size_t)S + 1)) != hipSuccess || hipMalloc((void**)&m->roff, sizeof(int64_t) * (size_t)S) != hipSuccess ||
        hipMalloc((void**)&m->rows_u, sizeof(int32_t) * (size_t)tot) != hipSuccess || hipMalloc((void**)&m->feat_all, sizeof(double) * 3 * (size_t)tot) != hipSuccess) {
        set_error("pcreg_sphere_model_create: out of device memory"); return fail(PCREG_E_HIP);
    }
    Stage st{scratch()};
    double *tmp, *fm; int32_t *duni, *nd;
    SphereDst d{m->seg_off, m->roff, m->feat_all, nullptr};
    if ((rc = st.take(3 * (size_t)VM, &tmp)) || (rc = st.take(3 * (size_t)VM, &fm)) || (rc = upload_points_aos(featModel, VM, ldM, tmp, fm, g_stream)) ||
        (rc = sphere_head(st, "pcreg_sphere_model_create", g, fm, VM, centres, ldC, R_desc, &d, model_rows)))
        return fail(rc);
    // the union of the spheres' rows (ascending) and the lists renumbered into it
    std::vector<int32_t> uni(model_rows, model_rows + tot);
    std::sort(uni.begin(), uni.end());
    uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
    std::vector<int32_t> ren((size_t)tot);
    for (int k = 0; k < tot; ++k) ren[k] = (int32_t)(std::lower_bound(uni.begin(), uni.end(), model_rows[k]) - uni.begin());
    m->VMu = (int)uni.size();
    const double* rM;
    if ((rc = desc_set_rows(model, &rM))) return fail(rc);
    if ((rc = st.take(uni.size(), &duni)) || (rc = st.take(1, &nd))) return fail(rc);
    if (hipMalloc((void**)&m->desc_u, sizeof(double) * uni.size() * (size_t)D) != hipSuccess) { set_error("pcreg_sphere_model_create: out of device memory"); return fail(PCREG_E_HIP); }
    const int32_t nu = m->VMu;
    if (hipMemcpyAsync(duni, uni.data(), sizeof(int32_t) * uni.size(), hipMemcpyHostToDevice, g_stream) != hipSuccess ||
        hipMemcpyAsync(nd, &nu, sizeof(int32_t), hipMemcpyHostToDevice, g_stream) != hipSuccess ||
        hipMemcpyAsync(m->rows_u, ren.data(), sizeof(int32_t) * (size_t)tot, hipMemcpyHostToDevice, g_stream) != hipSuccess) { set_error("copy failed"); return fail(PCREG_E_HIP); }
    if ((rc = launch_gather_rows_f64(rM, D, duni, nd, m->VMu, m->desc_u, g_stream))) return fail(rc);
    if (hipStreamSynchronize(g_stream) != hipSuccess) { set_error("pcreg_sphere_model_create failed"); return fail(PCREG_E_HIP); }          // the host vectors go out of scope
    *out = m;
    return PCREG_OK;
}
int pcreg_sphere_model_destroy(pcreg_sphere_model* m) {
    if (!m) return PCREG_OK;
    std::lock_guard<std::mutex> lock(g_mu);
    (void)hipDeviceSynchronize();
    sphere_model_free(m);
    return PCREG_OK;
}
int pcreg_sphere_sweep_on_model(pcreg_sphere_model* m, const pcreg_desc_set* surface, const double* featSurface, int ldS, const pcreg_match_opts* par,
                                int putative_thresh, const pcreg_ransac_opts* coef, uint32_t* pairs_all, int32_t* n_pairs, int32_t* trial, int* n_trials,
                                double* T, int32_t* num_success, int32_t* max_inliers, int32_t* failed) {
    PCREG_ARG(m && surface && featSurface && par && coef && n_trials && surface->D == m->D && ldS >= surface->n && coef->minPtNum == 3 && coef->iterNum >= 1);
    PCREG_ARG(m->S == 0 || (pairs_all && n_pairs && trial && T && num_success && max_inliers && failed));
    if (par->metric != PCREG_METRIC_SAD) { set_error("pcreg_sphere_sweep_on_model: Metric must be SAD"); return PCREG_E_ARG; }
    GUARD();
    *n_trials = 0;
    const int S = m->S, VS = surface->n, D = m->D, tot = m->tot;
    if (S == 0) return PCREG_OK;
    if (VS == 0 || tot == 0 || m->VMu == 0) { for (int i = 0; i < S; ++i) n_pairs[i] = 0; return PCREG_OK; }
    const size_t ld = (size_t)S * (size_t)VS;
    PCREG_ARG(ld <= 0x7FFFFFFFull);
    Stage st{scratch()};
    SweepStage b;
    TRY(sweep_stage(st, S, VS, VS, get_matches_segmented_workspace_bytes(VS, m->VMu, D, S, tot, m->n_max), coef, &b));
    const double* rS;
    TRY(desc_set_rows(surface, &rS));
    SegPreparedModel prep;
    TRY(prepared_rows(m->prep, m->desc_u, m->VMu, D, *par, &prep));
    TRY(upload_points_aos(featSurface, VS, ldS, b.tmp, b.fs, g_stream));
    TRY(launch_get_matches_segmented(rS, VS, m->desc_u, m->VMu, D, m->rows_u, m->seg_off, S, tot, m->n_max, *par, b.dp, nullptr, b.dn, b.ws, b.wsb, g_stream, &prep));
    return sweep_tail(st, b, S, VS, m->feat_all, m->roff, putative_thresh, coef, pairs_all, n_pairs, trial, n_trials, T, num_success, max_inliers, failed);
}

int pcreg_align_points_knn_batched(const double* pts, int total, int ld, const int32_t* offsets, int B, int C1, int C2,
                                   double* aligned, double* coeff, double* c, int32_t* status) {
    PCREG_ARG(pts && offsets && aligned && coeff && c && status && total >= 0 && ld >= total && B >= 0);
    GUARD();
    if (B == 0) return PCREG_OK;
    int max_n = 0;
    for (int b = 0; b < B; ++b) { int nb = offsets[b + 1] - offsets[b]; PCREG_ARG(nb >= 0); if (nb > max_n) max_n = nb; }
    PCREG_ARG(offsets[0] == 0 && offsets[B] == total);
    size_t tot = (size_t)(total > 0 ? total : 1);
    Stage st{scratch()};
    double *dp, *da, *dco, *dc; int32_t *doff, *dst;
    TRY(st.take(3 * tot, &dp));
    TRY(st.take(3 * tot, &da));
    TRY(st.take((size_t)B + 1, &doff));
    TRY(st.take(9 * (size_t)B, &dco));
    TRY(st.take(3 * (size_t)B, &dc));
    TRY(st.take((size_t)B, &dst));
    TRY(upload_cols(pts, total, ld, 3, dp, g_stream));
    PCREG_HIP(hipMemcpyAsync(doff, offsets, sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice, g_stream));
    PCREG_HIP(hipMemsetAsync(dco, 0, sizeof(double) * 9 * (size_t)B, g_stream));
    PCREG_HIP(hipMemsetAsync(dc, 0, sizeof(double) * 3 * (size_t)B, g_stream));
    PCREG_HIP(hipMemsetAsync(da, 0, sizeof(double) * 3 * tot, g_stream));
    TRY(launch_align_points_knn(dp, total, doff, B, max_n, C1, C2, da, total, dco, dc, dst, g_stream));
    if (total > 0) PCREG_HIP(hipMemcpyAsync(aligned, da, sizeof(double) * 3 * (size_t)total, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(coeff, dco, sizeof(double) * 9 * (size_t)B, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(c, dc, sizeof(double) * 3 * (size_t)B, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(status, dst, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}

int pcreg_dev_align_points_knn_batched(const double* pts, int total, int ld, const int32_t* offsets, int B, int max_n,
                                       int C1, int C2, double* aligned, double* coeff, double* c, int32_t* status,
                                       void* stream) {
    PCREG_ARG(pts && offsets && aligned && coeff && c && status && total >= 0 && ld >= total && B >= 0 && max_n >= 0);
    GUARD();
    if (B == 0) return PCREG_OK;
    return launch_align_points_knn(pts, ld, offsets, B, max_n, C1, C2, aligned, ld, coeff, c, status, (hipStream_t)stream);
}

int pcreg_align_points_knn(const double* pts, int n, int ld, int C1, int C2, double* aligned, double coeff[9],
                           double c[3]) {
    PCREG_ARG(pts && aligned && coeff && c && n >= 2 && ld >= n);
    int32_t offsets[2] = {0, n};
    int32_t status = 0;
    // compact the input so that "total == ld" holds for the batched entry point
    if (ld != n) {
        std::vector<double> tmp((size_t)n * 3);
        for (int k = 0; k < 3; ++k) memcpy(tmp.data() + (size_t)k * n, pts + (size_t)k * ld, sizeof(double) * (size_t)n);
        TRY(pcreg_align_points_knn_batched(tmp.data(), n, n, offsets, 1, C1, C2, aligned, coeff, c, &status));
    } else {
        TRY(pcreg_align_points_knn_batched(pts, n, n, offsets, 1, C1, C2, aligned, coeff, c, &status));
    }
    if (status != 0) { set_error("AlignPoints_KNN: support too small"); return PCREG_E_ARG; }
    return PCREG_OK;
}

// pts / sample_pts: double arrays (single data widened exactly by the caller); single_mode: see launch_descriptors
static int descriptors_host(const double* pts, int P, int ld, const double* sample_pts, int S, int lds, const pcreg_desc_opts* options,
                            int single_mode, double* feat, double* desc, int* V) {
    *V = 0;
    if (P == 0 || S == 0) return PCREG_OK;
    Stage st{scratch()};
    double *dp, *dk, *dfeat, *ddesc; int32_t* dV; char* ws;
    size_t wsb = descriptors_workspace_bytes(P, S);
    TRY(st.take(3 * (size_t)P, &dp));
    TRY(st.take(3 * (size_t)S, &dk));
    TRY(st.take(3 * (size_t)S, &dfeat));
    TRY(st.take(PCREG_DESC_LEN * (size_t)S, &ddesc));
    TRY(st.take(2, &dV));                                   // V | the over-capacity flag
    TRY(st.take(wsb, &ws));
    TRY(upload_cols(pts, P, ld, 3, dp, g_stream));
    TRY(upload_cols(sample_pts, S, lds, 3, dk, g_stream));
    TRY(launch_descriptors(dp, P, P, dk, S, S, *options, single_mode, dfeat, ddesc, nullptr, nullptr, dV, dV + 1, ws, wsb, g_stream));
    int32_t hv[2] = {0, 0};
    PCREG_HIP(hipMemcpyAsync(hv, dV, sizeof hv, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    if (hv[1] != 0) { set_error("a support holds %d points: more than the %d an LDS-resident support may have (lower max_pts)", hv[1], 8191); return PCREG_E_ARG; }
    if (hv[0] > 0) {
        PCREG_HIP(hipMemcpy(feat, dfeat, sizeof(double) * 3 * (size_t)hv[0], hipMemcpyDeviceToHost));
        PCREG_HIP(hipMemcpy(desc, ddesc, sizeof(double) * PCREG_DESC_LEN * (size_t)hv[0], hipMemcpyDeviceToHost));
    }
    *V = hv[0];
    return PCREG_OK;
}

int pcreg_spatial_histogram_descriptors(const double* pts, int P, int ld, const double* sample_pts, int S, int lds,
                                        const pcreg_desc_opts* options, double* feat, double* desc, int* V) {
    PCREG_ARG(pts && sample_pts && options && feat && desc && V && P >= 0 && S >= 0 && ld >= P && lds >= S);
    GUARD();
    return descriptors_host(pts, P, ld, sample_pts, S, lds, options, 0, feat, desc, V);
}

// ---- `single` inputs (clouds read by pcread are single: upsampleMesh.m:21, GetPointcloudFromModel.m:269) ----------------
// AlignPoints_KNN keeps its class (AlignPoints_KNN.m:17,59: everything derives from pts): the float -> double widening is
// exact, the arithmetic is the double kernel's, the outputs are rounded once to float.
int pcreg_align_points_knn_f32(const float* pts, int n, int ld, int C1, int C2, float* aligned, float coeff[9], float c[3]) {
    PCREG_ARG(pts && aligned && coeff && c && n >= 2 && ld >= n);
    std::vector<double> in((size_t)n * 3), out((size_t)n * 3);
    for (int k = 0; k < 3; ++k) for (int i = 0; i < n; ++i) in[(size_t)k * n + i] = (double)pts[(size_t)k * ld + i];
    double co[9], cc[3];
    TRY(pcreg_align_points_knn(in.data(), n, n, C1, C2, out.data(), co, cc));
    for (size_t i = 0; i < (size_t)n * 3; ++i) aligned[i] = (float)out[i];
    for (int i = 0; i < 9; ++i) coeff[i] = (float)co[i];
    for (int i = 0; i < 3; ++i) c[i] = (float)cc[i];
    return PCREG_OK;
}

// getSpacialHistogramDescriptors with a `single` cloud and / or `single` keypoints.  The OUTPUTS are double whatever the
// inputs (getSpacialHistogramDescriptors.m:61-62 preallocates desc / feat with nan(...) and assigns into them).  What runs in
// single inside MATLAB and is element-wise -- hence reproducible -- is reproduced: getLocalPoints.m:8-31's open box test,
// pts_cube - c, sqrt(x^2 + y^2 + z^2), dists < R and with them WHICH keypoints survive and which points form a support;
// the support's coordinates are MATLAB's single pts_rel values.  mean / pca / the histogram then run in double on those
// values (the summation order of MATLAB's single mean and pca is not knowable: INTEGRATION.md).
int pcreg_spatial_histogram_descriptors_mixed(const void* pts, int pts_is_single, int P, int ld, const void* sample_pts,
                                              int sample_is_single, int S, int lds, const pcreg_desc_opts* options,
                                              double* feat, double* desc, int* V) {
    PCREG_ARG(pts && sample_pts && options && feat && desc && V && P >= 0 && S >= 0 && ld >= P && lds >= S);
    GUARD();
    std::vector<double> p, k;
    const double* pp = (const double*)pts; const double* kk = (const double*)sample_pts;
    int lp = ld, lk = lds;
    if (pts_is_single) {
        p.resize((size_t)P * 3);
        for (int c = 0; c < 3; ++c) for (int i = 0; i < P; ++i) p[(size_t)c * P + i] = (double)((const float*)pts)[(size_t)c * ld + i];
        pp = p.data(); lp = P;
    }
    if (sample_is_single) {
        k.resize((size_t)S * 3);
        for (int c = 0; c < 3; ++c) for (int i = 0; i < S; ++i) k[(size_t)c * S + i] = (double)((const float*)sample_pts)[(size_t)c * lds + i];
        kk = k.data(); lk = S;
    }
    const int mode = sample_is_single ? 1 : (pts_is_single ? 2 : 0);
    return descriptors_host(pp, P, lp, kk, S, lk, options, mode, feat, desc, V);
}
int pcreg_spatial_histogram_descriptors_f32(const float* pts, int P, int ld, const float* sample_pts, int S, int lds,
                                            const pcreg_desc_opts* options, double* feat, double* desc, int* V) {
    return pcreg_spatial_histogram_descriptors_mixed(pts, 1, P, ld, sample_pts, 1, S, lds, options, feat, desc, V);
}

// ------------------------------------------------------------------ device tier
size_t pcreg_dev_knn2_points_f32_workspace(int Q, int M) { return knn2_points_workspace_bytes(Q, M); }

int pcreg_dev_knn2_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm, int32_t idx_base,
                              int32_t* idx, float* dist, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(q && m && idx && dist && workspace);
    GUARD();
    return launch_knn2_points_f32(q, Q, ldq, m, M, ldm, idx_base, idx, dist, workspace, workspace_bytes, (hipStream_t)stream);
}

int pcreg_dev_merge_top2_f32(const int32_t* idx_in, const float* dist_in, int R, int Q, int32_t* idx, float* dist,
                             void* stream) {
    PCREG_ARG(idx_in && dist_in && idx && dist);
    GUARD();
    return launch_merge_top2_f32(idx_in, dist_in, R, Q, idx, dist, (hipStream_t)stream);
}

int pcreg_dev_merge_top2_strided_f32(const int32_t* idx_in, const float* dist_in, int R, int Q, size_t rank_stride,
                                     int32_t* idx, float* dist, void* stream) {
    PCREG_ARG(idx_in && dist_in && idx && dist);
    GUARD();
    return launch_merge_top2_f32(idx_in, dist_in, R, Q, idx, dist, (hipStream_t)stream, rank_stride);
}

int pcreg_dev_merge_topk_f32(const int32_t* idx_in, const float* dist_in, int R, int Q, int k, size_t rank_stride, int32_t* idx,
                             float* dist, void* stream) {
    PCREG_ARG(idx_in && dist_in && idx && dist && k >= 1 && k <= kKnnMaxK && R >= 1 && Q >= 0 &&
              (rank_stride == 0 || rank_stride >= (size_t)Q * k));
    GUARD();
    return launch_merge_topk_f32(idx_in, dist_in, R, Q, k, rank_stride, idx, dist, (hipStream_t)stream);
}

size_t pcreg_dev_ransac_workspace(int n_cap, int iterNum) { return ransac_workspace_bytes(iterNum, 1, n_cap); }

int pcreg_dev_ransac(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld,
                     const pcreg_ransac_opts* opts, const int32_t* sample_idx, pcreg_dev_ransac_result* out,
                     int32_t* inlier_idx, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(pts1 && pts2 && opts && out && inlier_idx && workspace && n_cap >= 0 && ld >= n_cap);
    GUARD();
    return launch_ransac(pts1, pts2, ld, nullptr, n_dev, n_cap, 1, *opts, sample_idx, out, inlier_idx, nullptr, nullptr,
                         workspace, workspace_bytes, (hipStream_t)stream);
}


int pcreg_dev_ransac_partial(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld,
                             const pcreg_ransac_opts* opts, const int32_t* sample_idx, int hyp_begin, int hyp_count,
                             pcreg_dev_ransac_part* part, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(pts1 && pts2 && opts && part && workspace && n_cap >= 0 && ld >= n_cap);
    GUARD();
    return launch_ransac_partial(pts1, pts2, ld, n_dev, n_cap, *opts, sample_idx, hyp_begin, hyp_count, part, workspace,
                                 workspace_bytes, (hipStream_t)stream);
}
int pcreg_dev_ransac_finish(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld,
                            const pcreg_ransac_opts* opts, const pcreg_dev_ransac_part* combined,
                            pcreg_dev_ransac_result* out, int32_t* inlier_idx, void* stream) {
    PCREG_ARG(pts1 && pts2 && opts && combined && out && inlier_idx && n_cap >= 0 && ld >= n_cap);
    GUARD();
    return launch_ransac_finish(pts1, pts2, ld, n_dev, n_cap, *opts, combined, out, inlier_idx, (hipStream_t)stream);
}

int pcreg_dev_ransac_finish_parts(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld,
                                  const pcreg_ransac_opts* opts, const pcreg_dev_ransac_part* parts, int n_parts,
                                  pcreg_dev_ransac_result* out, int32_t* inlier_idx, void* stream) {
    PCREG_ARG(pts1 && pts2 && opts && parts && n_parts >= 1 && out && inlier_idx && n_cap >= 0 && ld >= n_cap);
    GUARD();
    return launch_ransac_finish(pts1, pts2, ld, n_dev, n_cap, *opts, parts, out, inlier_idx, (hipStream_t)stream, n_parts);
}

// live timing of the search's dominant kernel (HIP events on the launch stream), for bench.py's roofline
int pcreg_dev_search_kernel_timing(int enable) { GUARD(); knn_f16_timing_enable(enable != 0); return PCREG_OK; }
int pcreg_dev_search_kernel_ms(float* mean_ms, int* launches) {
    PCREG_ARG(mean_ms && launches);
    GUARD();
    return knn_f16_timing_read(mean_ms, launches);
}

// ---- descriptor stage, resident (speedyDescriptors.m:59 -> getMatches -> ransac without leaving HBM)
size_t pcreg_dev_spatial_histogram_descriptors_workspace(int P, int S) { return descriptors_workspace_bytes(P, S); }

int pcreg_dev_spatial_histogram_descriptors(const double* pts, int P, int ld, const double* sample_pts, int S, int lds,
                                            const pcreg_desc_opts* options, double* feat, double* desc, int32_t* counters,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(pts && sample_pts && options && feat && desc && counters && workspace && P >= 1 && S >= 1 && ld >= P && lds >= S);
    GUARD();
    return launch_descriptors(pts, P, ld, sample_pts, S, lds, *options, 0, feat, desc, nullptr, nullptr, counters, counters + 1, workspace,
                              workspace_bytes, (hipStream_t)stream);
}

int pcreg_dev_spatial_histogram_descriptors_rows_u16(const double* pts, int P, int ld, const double* sample_pts, int S, int lds,
                                                     const pcreg_desc_opts* options, int single_mode, double* feat, uint16_t* rows,
                                                     int32_t* row_index, int32_t* counters, void* workspace, size_t workspace_bytes,
                                                     void* stream) {
    PCREG_ARG(pts && sample_pts && options && feat && rows && row_index && counters && workspace && P >= 1 && S >= 1 && ld >= P && lds >= S);
    GUARD();
    return launch_descriptors(pts, P, ld, sample_pts, S, lds, *options, single_mode, feat, nullptr, rows, row_index, counters, counters + 1,
                              workspace, workspace_bytes, (hipStream_t)stream);
}

static constexpr int kLayoutRowMajorU16 = 1000;      // internal: dense uint16 rows (pcreg_dev_get_matches_rows_u16)
static size_t dev_get_matches_layout(int Q, int M, int D, int Dp, size_t off[6]) {
    size_t q = (size_t)(Q > 0 ? Q : 1), m = (size_t)(M > 0 ? M : 1), b = 0;
    off[0] = b; b += align_up(q * D * sizeof(double), 256);            // raw surface, feature-major
    off[1] = b; b += align_up(m * D * sizeof(double), 256);            // raw model
    off[2] = b; b += align_up(q * Dp * sizeof(double), 256);           // working copies
    off[3] = b; b += align_up(m * Dp * sizeof(double), 256);
    off[4] = b; b += align_up((q + m + 1) * sizeof(double), 256);      // preprocess
    off[5] = b; b += match_features_workspace_bytes(Q, M, Dp);
    return b;
}
size_t pcreg_dev_get_matches_workspace(int Q, int M, int D) {
    size_t off[6];
    return dev_get_matches_layout(Q, M, D, D + 1, off);
}

static int dev_get_matches_impl(const void* descSurface, int Q, int ldS, const void* descModel, int M, int ldM, int D,
                                int layout, const pcreg_match_opts* par, uint32_t* pairs, double* metric, int32_t* n_pairs,
                                void* workspace, size_t workspace_bytes, hipStream_t st, const int32_t* idxS = nullptr,
                                const int32_t* idxM = nullptr) {
    if (Q == 0 || M == 0) { PCREG_HIP(hipMemsetAsync(n_pairs, 0, sizeof(int32_t), st)); return PCREG_OK; }
    const int Dp = D + (par->unnormalize ? 1 : 0);
    size_t off[6];
    size_t need = dev_get_matches_layout(Q, M, D, D + 1, off);
    if (workspace_bytes < need) { set_error("get_matches workspace too small: %zu < %zu", workspace_bytes, need); return PCREG_E_WORKSPACE; }
    char* w = (char*)workspace;
    double *rawS = (double*)(w + off[0]), *rawM = (double*)(w + off[1]), *fS = (double*)(w + off[2]), *fM = (double*)(w + off[3]);
    const double *inS = (const double*)descSurface, *inM = (const double*)descModel;
    int ls = ldS, lm = ldM;
    if (layout == PCREG_LAYOUT_ROW_MAJOR) {        // [row][D] (ld = row pitch) -> feature-major
        if (ldS != D || ldM != D) { set_error("row-major descriptors must be dense (ld == D)"); return PCREG_E_ARG; }
        TRY(launch_transpose_rows((const double*)descSurface, D, D, Q, rawS, st));
        TRY(launch_transpose_rows((const double*)descModel, D, D, M, rawM, st));
        inS = rawS; inM = rawM; ls = Q; lm = M;
    } else if (layout == kLayoutRowMajorU16) {     // dense u16 rows (counts) -> feature-major doubles, exactly
        TRY(launch_widen_rows_u16((const uint16_t*)descSurface, idxS, Q, D, rawS, st));
        TRY(launch_widen_rows_u16((const uint16_t*)descModel, idxM, M, D, rawM, st));
        inS = rawS; inM = rawM; ls = Q; lm = M;
    }
    // getMatches.m:24-37 always works on private copies (the caller's descriptors stay untouched)
    TRY(launch_preprocess(inS, Q, ls, inM, M, lm, D, *par, fS, fM, w + off[4], align_up(((size_t)Q + M + 1) * sizeof(double), 256), st));
    if (!par->prenormalized) {
        TRY(launch_normalize_rows2(fS, Q, Q, fM, M, M, Dp, st));
    }
    return launch_match_features(fS, Q, Q, fM, M, M, Dp, *par, pairs, metric, n_pairs, w + off[5], workspace_bytes - off[5], st);
}

int pcreg_dev_get_matches(const double* descSurface, int Q, int ldS, const double* descModel, int M, int ldM, int D,
                          int layout, const pcreg_match_opts* par, uint32_t* pairs, double* metric, int32_t* n_pairs,
                          void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(descSurface && descModel && par && pairs && n_pairs && workspace && Q >= 0 && M >= 0 && D >= 1);
    PCREG_ARG(layout == PCREG_LAYOUT_FEATURE_MAJOR || layout == PCREG_LAYOUT_ROW_MAJOR);
    PCREG_ARG(layout == PCREG_LAYOUT_ROW_MAJOR ? (ldS >= D && ldM >= D) : (ldS >= Q && ldM >= M));
    PCREG_ARG(par->metric == PCREG_METRIC_SAD || par->metric == PCREG_METRIC_SSD);
    GUARD();
    return dev_get_matches_impl(descSurface, Q, ldS, descModel, M, ldM, D, layout, par, pairs, metric, n_pairs, workspace,
                                workspace_bytes, (hipStream_t)stream);
}

int pcreg_dev_get_matches_rows_u16(const uint16_t* rowsSurface, const int32_t* indexSurface, int Q, const uint16_t* rowsModel,
                                   const int32_t* indexModel, int M, int D, const pcreg_match_opts* par, uint32_t* pairs, double* metric,
                                   int32_t* n_pairs, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(rowsSurface && rowsModel && par && pairs && n_pairs && workspace && Q >= 0 && M >= 0 && D >= 1);
    PCREG_ARG(par->metric == PCREG_METRIC_SAD || par->metric == PCREG_METRIC_SSD);
    GUARD();
    return dev_get_matches_impl(rowsSurface, Q, D, rowsModel, M, D, D, kLayoutRowMajorU16, par, pairs, metric, n_pairs, workspace,
                                workspace_bytes, (hipStream_t)stream, indexSurface, indexModel);
}

int pcreg_dev_gather_matched_rows(const uint32_t* pairs, const int32_t* n_pairs, int cap, const double* featSurface,
                                  const double* featModel, double* pts1, double* pts2, void* stream) {
    PCREG_ARG(pairs && n_pairs && featSurface && featModel && pts1 && pts2 && cap >= 0);
    GUARD();
    return launch_gather_matched_rows(pairs, n_pairs, cap, featSurface, featModel, pts1, pts2, (hipStream_t)stream);
}


// ---- sphere-sweep driver pieces (completeExperimentFast.m:46-225, :291, :356-394), device tier
int pcreg_dev_sphere_counts(const double* feat, int V, const double* centres, int S, double R, int32_t* counts, void* stream) {
    PCREG_ARG(feat && centres && counts && V >= 0 && S >= 0);
    GUARD();
    return launch_sphere_counts(feat, V, centres, S, R, counts, (hipStream_t)stream);
}
int pcreg_dev_sphere_select_batched(const double* feat, int V, const double* centres, int S, double R, const int32_t* seg_off,
                                    int32_t* idx, double* feat_out, int32_t* n_out, void* stream) {
    PCREG_ARG(feat && centres && seg_off && idx && V >= 0 && S >= 0);
    GUARD();
    return launch_sphere_select_batched(feat, V, centres, S, R, seg_off, idx, feat_out, n_out, (hipStream_t)stream);
}
size_t pcreg_dev_get_matches_segmented_workspace(int Q, int VM, int D, int S, int total_rows, int max_rows) {
    return get_matches_segmented_workspace_bytes(Q, VM, D, S, total_rows, max_rows);
}
int pcreg_dev_get_matches_segmented(const double* descSurface, int Q, const double* descModel, int VM, int D, const int32_t* seg_rows,
                                    const int32_t* seg_off, int S, int total_rows, int max_rows, const pcreg_match_opts* par,
                                    uint32_t* pairs_all, double* metric_all, int32_t* n_pairs, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    PCREG_ARG(descSurface && descModel && seg_rows && seg_off && par && pairs_all && n_pairs && workspace);
    PCREG_ARG(Q >= 0 && VM >= 0 && D >= 1 && S >= 0 && S <= 65535 && total_rows >= 0 && max_rows >= 0 && max_rows <= total_rows);
    if (par->metric != PCREG_METRIC_SAD) { set_error("pcreg_dev_get_matches_segmented: Metric must be SAD (one pcreg_dev_get_matches call per segment handles SSD)"); return PCREG_E_ARG; }
    GUARD();
    return launch_get_matches_segmented(descSurface, Q, descModel, VM, D, seg_rows, seg_off, S, total_rows, max_rows, *par, pairs_all,
                                        metric_all, n_pairs, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_segmented_model_bytes(int VM, int D) { return segmented_prepared_model_bytes(VM, D); }
int pcreg_dev_segmented_model_prepare(const double* descModel, int VM, int D, const pcreg_match_opts* par, void* prepared, size_t prepared_bytes, void* stream) {
    PCREG_ARG(descModel && par && prepared && VM >= 0 && D >= 1 && prepared_bytes >= segmented_prepared_model_bytes(VM, D));
    GUARD();
    double* P = (double*)prepared;
    return launch_segmented_prepare_model(descModel, VM, D, *par, P, P + (size_t)(VM > 0 ? VM : 1) * D, (hipStream_t)stream);
}
int pcreg_dev_get_matches_segmented_prepared(const double* descSurface, int Q, const double* descModel, int VM, int D, const void* prepared,
                                             int prepared_change_metric, double prepared_metric_factor, const int32_t* seg_rows,
                                             const int32_t* seg_off, int S, int total_rows, int max_rows, const pcreg_match_opts* par,
                                             uint32_t* pairs_all, double* metric_all, int32_t* n_pairs, void* workspace, size_t workspace_bytes,
                                             void* stream) {
    PCREG_ARG(descSurface && descModel && prepared && seg_rows && seg_off && par && pairs_all && n_pairs && workspace);
    PCREG_ARG(Q >= 0 && VM >= 0 && D >= 1 && S >= 0 && S <= 65535 && total_rows >= 0 && max_rows >= 0 && max_rows <= total_rows);
    if (par->metric != PCREG_METRIC_SAD) { set_error("pcreg_dev_get_matches_segmented_prepared: Metric must be SAD"); return PCREG_E_ARG; }
    GUARD();
    const double* P = (const double*)prepared;
    const SegPreparedModel prep{P, P + (size_t)(VM > 0 ? VM : 1) * D, VM, D, prepared_change_metric, prepared_metric_factor};
    return launch_get_matches_segmented(descSurface, Q, descModel, VM, D, seg_rows, seg_off, S, total_rows, max_rows, *par, pairs_all,
                                        metric_all, n_pairs, workspace, workspace_bytes, (hipStream_t)stream, &prep);
}
size_t pcreg_dev_sphere_select_workspace(int V) { return sphere_select_workspace_bytes(V); }
int pcreg_dev_sphere_select(const double* feat, int V, const double centre[3], double R, int32_t* idx, int32_t* n_out,
                            void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(feat && centre && idx && n_out && workspace && V >= 0);
    GUARD();
    return launch_sphere_select(feat, V, centre, R, idx, n_out, workspace, workspace_bytes, (hipStream_t)stream);
}
int pcreg_dev_gather_rows_f64(const double* src, int D, const int32_t* idx, const int32_t* n, int cap, double* dst, void* stream) {
    PCREG_ARG(src && idx && n && dst && D >= 1 && cap >= 0);
    GUARD();
    return launch_gather_rows_f64(src, D, idx, n, cap, dst, (hipStream_t)stream);
}
int pcreg_dev_sweep_plan(const int32_t* n_pairs, int S, int putative_thresh, int32_t* trial_idx, int32_t* offsets, int32_t* n_trials, void* stream) {
    PCREG_ARG(n_pairs && trial_idx && offsets && n_trials && S >= 0);
    GUARD();
    return launch_sweep_plan(n_pairs, S, putative_thresh, trial_idx, offsets, n_trials, (hipStream_t)stream);
}
int pcreg_dev_sweep_gather(const uint32_t* pairs_all, int VS, const int32_t* n_pairs, const int32_t* trial_idx, const int32_t* offsets,
                           const int32_t* n_trials, int S, const double* featSurface, const double* featCur_all, const int64_t* row_off,
                           double* pts1, double* pts2, int ld, void* stream) {
    PCREG_ARG(pairs_all && n_pairs && trial_idx && offsets && n_trials && featSurface && featCur_all && row_off && pts1 && pts2 && S >= 0 && VS >= 0 && ld >= 0);
    GUARD();
    return launch_sweep_gather(pairs_all, VS, n_pairs, trial_idx, offsets, n_trials, S, featSurface, featCur_all, row_off, pts1, pts2, ld, (hipStream_t)stream);
}
size_t pcreg_dev_ransac_batched_workspace(int n_cap, int iterNum, int B) { return ransac_workspace_bytes(iterNum, B > 0 ? B : 1, n_cap); }
int pcreg_dev_ransac_batched(const double* pts1, const double* pts2, int ld, const int32_t* offsets, int B, int n_cap,
                             const pcreg_ransac_opts* opts, pcreg_dev_ransac_result* out, int32_t* inlier_idx,
                             void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(pts1 && pts2 && offsets && opts && out && inlier_idx && workspace && B >= 1 && n_cap >= 0 && ld >= 0);
    PCREG_ARG(opts->minPtNum == 3);                    // the built-in sampler, seed + b for registration b
    GUARD();
    return launch_ransac(pts1, pts2, ld, offsets, nullptr, n_cap, B, *opts, nullptr, out, inlier_idx, nullptr, nullptr,
                         workspace, workspace_bytes, (hipStream_t)stream);
}

size_t pcreg_dev_fgr_batched_workspace(int n_cap, int B, int iterations) { return fgr_ws_bytes(n_cap, B, iterations); }
int pcreg_dev_fgr_batched(const double* pts1, const double* pts2, int ld, const int32_t* offsets, int B, int n_cap, const pcreg_fgr_opts* opts,
                          const double* T0, const int32_t* tuple_idx, pcreg_fgr_result* out, int32_t* inlier_idx, uint8_t* kept, void* workspace,
                          size_t workspace_bytes, void* stream) {
    PCREG_ARG(pts1 && pts2 && offsets && opts && out && inlier_idx && workspace && B >= 1 && n_cap >= 0 && ld >= 0);
    PCREG_ARG(fgr_args_ok(*opts));
    GUARD();
    return launch_fgr(pts1, pts2, ld, offsets, B, n_cap, *opts, T0, opts->n_tuples > 0 ? tuple_idx : nullptr, out, inlier_idx, kept, workspace,
                      workspace_bytes, (hipStream_t)stream);
}

int pcreg_dev_quick_tf(const double* pts, int n, int ld, const double T[16], double* out, int ldo, void* stream) {
    PCREG_ARG(pts && T && out && n >= 0 && ld >= n && ldo >= n);
    GUARD();
    return launch_quick_tf(pts, n, ld, T, out, ldo, (hipStream_t)stream);
}
int pcreg_dev_refine_by_distance(const double* pts1, const double* pts2, const int32_t* n_dev, int cap, int ld, double maxDist,
                                 double* T16, int32_t* info, void* stream) {
    PCREG_ARG(pts1 && pts2 && n_dev && T16 && info && cap >= 0 && ld >= cap);
    GUARD();
    return launch_refine_by_distance(pts1, pts2, n_dev, cap, ld, maxDist, T16, info, (hipStream_t)stream);
}
size_t pcreg_dev_unique_rows3_workspace(int n_cap) { return unique_rows3_ws_bytes(n_cap); }
int pcreg_dev_unique_rows3_f64(const double* A, const int32_t* n_dev, int n_cap, int ld, int32_t idx_base, int32_t* ia, int32_t* n_unique,
                               void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(n_dev && n_unique && workspace && n_cap >= 0 && ld >= n_cap && (n_cap == 0 || (A && ia)));
    PCREG_ARG(workspace_bytes >= unique_rows3_ws_bytes(n_cap));
    GUARD();
    return launch_unique_rows3(A, n_dev, n_cap, ld, idx_base, ia, n_unique, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t pcreg_dev_downsample_grid_workspace(int n) { return downsample_grid_ws_bytes(n); }
int pcreg_dev_downsample_grid_chunk(void) { return downsample_grid_chunk(); }
int pcreg_dev_downsample_grid_f32(const float* pts, int n, int ld, double step, float* out, int ldo, int32_t* count, int32_t* label, int32_t* n_out,
                                  int32_t* info, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(n_out && info && workspace && n >= 0 && ld >= n && ldo >= n && std::isfinite(step) && step > 0.0 && (n == 0 || (pts && out)));
    PCREG_ARG(workspace_bytes >= downsample_grid_ws_bytes(n));
    GUARD();
    return launch_downsample_grid(pts, n, ld, step, out, ldo, count, label, n_out, info, workspace, workspace_bytes, (hipStream_t)stream);
}
// ---- the normal-distributions transform (ndt.hip) ---------------------------------------------------------------
}  // extern "C" (the handle types are C++ structs behind opaque C names)
struct pcreg_dev_ndt { pcreg::NdtView v; };
struct pcreg_ndt { pcreg_dev_ndt* d; };
extern "C" {

static int dev_ndt_create(const float* pts, int n, int ld, double step, int min_points, hipStream_t st, pcreg_dev_ndt** out) {
    *out = nullptr;
    NdtView v{};
    TRY(ndt_build(pts, n, ld, step, min_points, st, &v));
    *out = new pcreg_dev_ndt{v};
    return PCREG_OK;
}
// the table's Gaussians copied out (host pointers, each or NULL); the device is idle behind it
static int dev_ndt_get(const pcreg_dev_ndt* h, int32_t* cells, int32_t* counts, double* means, double* C, float* lo, float* origin) {
    const NdtView& v = h->v;
    for (int c = 0; c < 3; ++c) { if (lo) lo[c] = v.lo[c]; if (origin) origin[c] = v.o[c]; }
    if (v.G == 0 || !(cells || counts || means || C)) return PCREG_OK;
    std::vector<NdtRec> rec((size_t)v.G);
    PCREG_HIP(hipMemcpy(rec.data(), v.rec, sizeof(NdtRec) * (size_t)v.G, hipMemcpyDeviceToHost));
    for (size_t g = 0; g < (size_t)v.G; ++g) {
        const NdtRec& r = rec[g];
        if (cells) { cells[3 * g] = (int32_t)(r.key >> 42); cells[3 * g + 1] = (int32_t)((r.key >> 21) & 0x1FFFFF); cells[3 * g + 2] = (int32_t)(r.key & 0x1FFFFF); }
        if (counts) counts[g] = r.count;
        if (means) for (int c = 0; c < 3; ++c) means[3 * g + c] = r.mean[c];
        if (C) for (int c = 0; c < 6; ++c) C[6 * g + c] = r.C[c];
    }
    return PCREG_OK;
}

int pcreg_dev_ndt_create(const float* pts, int n, int ld, double step, int min_points, void* stream, pcreg_dev_ndt** ndt) {
    PCREG_ARG(ndt != nullptr && n >= 0 && ld >= n && (n == 0 || pts != nullptr) && std::isfinite(step) && step > 0.0 && min_points >= 3);
    GUARD();
    return dev_ndt_create(pts, n, ld, step, min_points, (hipStream_t)stream, ndt);
}
int pcreg_dev_ndt_destroy(pcreg_dev_ndt* ndt) {
    if (!ndt) return PCREG_OK;
    std::lock_guard<std::mutex> lock(g_mu);
    (void)hipDeviceSynchronize();                 // steps that still read the table
    (void)hipFree(ndt->v.block);
    delete ndt;
    return PCREG_OK;
}
int pcreg_dev_ndt_size(const pcreg_dev_ndt* ndt, int* n_voxels, int* n_gaussians) {
    PCREG_ARG(ndt && n_voxels && n_gaussians);
    *n_voxels = ndt->v.n_vox;
    *n_gaussians = ndt->v.G;
    return PCREG_OK;
}
int pcreg_dev_ndt_get(const pcreg_dev_ndt* ndt, int32_t* cells, int32_t* counts, double* means, double* C, float* lo, float* origin) {
    PCREG_ARG(ndt != nullptr);
    GUARD();
    return dev_ndt_get(ndt, cells, counts, means, C, lo, origin);
}
size_t pcreg_dev_ndt_refit_workspace(int Q, int B) { return ndt_refit_ws_bytes(Q, B); }
int pcreg_dev_ndt_refit_f32(const pcreg_dev_ndt* ndt, const float* q, int Q, int ldq, const double* T_dev, int B, int neighbors, double outlier_ratio,
                            double* T_out, double* T_step, int32_t* n_pairs, double* sum_e, int32_t* empty, void* workspace, size_t workspace_bytes,
                            void* stream) {
    PCREG_ARG(ndt != nullptr);
    GUARD();
    return launch_ndt_refit(ndt->v, q, Q, ldq, T_dev, B, neighbors, outlier_ratio, T_out, T_step, n_pairs, sum_e, empty, workspace, workspace_bytes,
                            (hipStream_t)stream);
}

// the host tier: the cloud is uploaded for the build and freed behind it; the handle keeps the table
int pcreg_ndt_create(const float* pts, int n, int ld, double step, int min_points, pcreg_ndt** ndt) {
    PCREG_ARG(ndt != nullptr && n >= 0 && ld >= n && (n == 0 || pts != nullptr) && std::isfinite(step) && step > 0.0 && min_points >= 3);
    GUARD();
    *ndt = nullptr;
    float* dp = nullptr;
    PCREG_HIP(hipMalloc((void**)&dp, sizeof(float) * 3 * (size_t)(n > 0 ? n : 1)));
    int rc = upload_cols(pts, n, ld, 3, dp, g_stream);
    pcreg_dev_ndt* d = nullptr;
    if (!rc) rc = dev_ndt_create(dp, n, n > 0 ? n : 1, step, min_points, g_stream, &d);       // (synchronises the stream)
    (void)hipFree(dp);
    if (rc) return rc;
    *ndt = new pcreg_ndt{d};
    return PCREG_OK;
}
int pcreg_ndt_destroy(pcreg_ndt* ndt) {
    if (!ndt) return PCREG_OK;
    const int rc = pcreg_dev_ndt_destroy(ndt->d);
    delete ndt;
    return rc;
}
int pcreg_ndt_size(const pcreg_ndt* ndt, int* n_voxels, int* n_gaussians) {
    PCREG_ARG(ndt != nullptr);
    return pcreg_dev_ndt_size(ndt->d, n_voxels, n_gaussians);
}
int pcreg_ndt_get(const pcreg_ndt* ndt, int32_t* cells, int32_t* counts, double* means, double* C, float* lo, float* origin) {
    PCREG_ARG(ndt != nullptr);
    GUARD();
    return dev_ndt_get(ndt->d, cells, counts, means, C, lo, origin);
}
// B transforms stepped `steps` times (RefitStaging); the block: [T_out 16 B doubles][sum_e B][n_pairs B int32][empty B int32]
int pcreg_ndt_refit_f32(pcreg_ndt* ndt, const float* q, int Q, int ldq, const double* T, int B, int neighbors, double outlier_ratio, int steps,
                        double* T_out, int32_t* n_pairs, double* sum_e, int32_t* empty) {
    double d2;
    PCREG_ARG(ndt && Q >= 0 && B >= 0 && ldq >= Q && Q <= ndt_max_queries() && steps >= 1 && (neighbors == 1 || neighbors == 7));
    PCREG_ARG(ndt_d2(ndt->d->v.step, outlier_ratio, &d2));
    PCREG_ARG((Q == 0 || q) && (B == 0 || (T && T_out && n_pairs && sum_e && empty)));
    GUARD();
    if (B == 0) return PCREG_OK;
    const size_t wsb = ndt_refit_ws_bytes(Q, B), nB = (size_t)B;
    RefitStaging rs(Q, B, 18);                                             // 17 B doubles and 2 B int32
    TRY(rs.take_inputs());
    TRY(rs.take_blocks(wsb));
    TRY(rs.upload(q, ldq, T));
    return rs.run(steps, [&](const double* in, double* blk) {
        int32_t* ib = (int32_t*)(blk + 17 * nB);
        return launch_ndt_refit(ndt->d->v, rs.dq, Q, Q, in, B, neighbors, outlier_ratio, blk, nullptr, ib, blk + 16 * nB, ib + nB, rs.ws, wsb, g_stream);
    }, {{T_out, 0, 128}, {sum_e, 32, 8}, {n_pairs, 34, 4}, {empty, 35, 4}});
}

size_t pcreg_dev_aggregate_matches_workspace(int n_cap) { return aggregate_matches_ws_bytes(n_cap); }
int pcreg_dev_aggregate_matches(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld, double* out1, double* out2,
                                int ldo, int32_t idx_base, int32_t* ia, int32_t* n_out, void* workspace, size_t workspace_bytes, void* stream) {
    PCREG_ARG(n_dev && n_out && workspace && n_cap >= 0 && ld >= n_cap && ldo >= n_cap && (n_cap == 0 || (pts1 && pts2 && out1 && out2)));
    PCREG_ARG(workspace_bytes >= aggregate_matches_ws_bytes(n_cap));
    GUARD();
    return launch_aggregate_matches(pts1, pts2, n_dev, n_cap, ld, out1, out2, ldo, idx_base, ia, n_out, workspace, workspace_bytes,
                                    (hipStream_t)stream);
}
int pcreg_dev_estimate_transform_indexed(const double* pts1, const double* pts2, int ld, const int32_t* idx, int32_t idx_base,
                                         const int32_t* n_idx_dev, int cap, double* T16, int32_t* info, void* stream) {
    PCREG_ARG(n_idx_dev && T16 && info && cap >= 0 && ld >= cap && (cap == 0 || (pts1 && pts2 && idx)));
    GUARD();
    return launch_estimate_transform_indexed(pts1, pts2, ld, idx, idx_base, n_idx_dev, cap, T16, info, (hipStream_t)stream);
}
int pcreg_dev_quick_tf_batched(const double* pts, int n, int ld, const double* T_dev, int K, double* out, int ldo, double* limits, void* stream) {
    PCREG_ARG(T_dev && K >= 0 && n >= 0 && ld >= n && ldo >= n && (n == 0 || (pts && out)));
    GUARD();
    return launch_quick_tf_batched(pts, n, ld, T_dev, K, out, ldo, limits, (hipStream_t)stream);
}
int pcreg_dev_final_close_refine_batched(const uint32_t* pairs, const int32_t* n_pairs, const double* feat, const int32_t* kp_off,
                                         const double* featCur_all, const int32_t* seg_off, int K, double maxDist, int32_t* n_close,
                                         double* precision, double* T16, int32_t* empty, void* stream) {
    PCREG_ARG(pairs && n_pairs && feat && kp_off && featCur_all && seg_off && n_close && precision && T16 && empty && K >= 0);
    GUARD();
    return launch_final_close_refine_batched(pairs, n_pairs, feat, kp_off, featCur_all, seg_off, K, maxDist, n_close, precision, T16, empty,
                                             (hipStream_t)stream);
}
int pcreg_dev_final_pick_apply(const double* precision, const double* T16, const int32_t* empty, int K, const double* pts_tform_all, int n, int ld,
                               double* out, int ldo, int32_t* best, void* stream) {
    PCREG_ARG(precision && T16 && empty && best && K >= 1 && n >= 0 && ld >= n && ldo >= n && (n == 0 || (pts_tform_all && out)));
    GUARD();
    return launch_final_pick_apply(precision, T16, empty, K, pts_tform_all, n, ld, out, ldo, best, (hipStream_t)stream);
}

// ---- the final stage of completeExperimentFast.m:280-394 at the host tier ------------------------------------------------------
int pcreg_final_stage_limits(const double* pts, int N, int ld, const double* T, int K, double* limits) {
    PCREG_ARG(pts && T && limits && N >= 1 && ld >= N);
    if (K < 1) { set_error("pcreg_final_stage_limits: K = %d clusters (at least one)", K); return PCREG_E_ARG; }
    GUARD();
    const size_t n = (size_t)N, k = (size_t)K;
    Stage st{scratch()};
    double *dp, *dT, *tf, *lim;
    TRY(st.take(3 * n, &dp));
    TRY(st.take(16 * k, &dT));
    TRY(st.take(3 * n * k, &tf));
    TRY(st.take(6 * k, &lim));
    TRY(upload_cols(pts, N, ld, 3, dp, g_stream));
    PCREG_HIP(hipMemcpyAsync(dT, T, sizeof(double) * 16 * k, hipMemcpyHostToDevice, g_stream));
    TRY(launch_quick_tf_batched(dp, N, N, dT, K, tf, N, lim, g_stream));
    PCREG_HIP(hipMemcpyAsync(limits, lim, sizeof(double) * 6 * k, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    return PCREG_OK;
}

// the bound on the clusters' fp64 descriptors held at once (debug key "final_batch_mb" lowers it for the tests)
static size_t final_stage_bound() {
    const int mb = debug_flag(kDbgFinalBatchMB);
    return mb > 0 ? (size_t)mb << 20 : (size_t)4 << 30;
}

int pcreg_final_stage(const pcreg_desc_set* model, const double* featModel, int ldM, const double* pts, int N, int ld, const double* locs,
                      const double* T, int K, const double* keypoints, const int32_t* kp_off, const pcreg_desc_opts* desc_opts,
                      const pcreg_match_opts* par, double R_desc, double maxDist, int32_t* num_keypoints, int32_t* num_desc,
                      int32_t* num_matches, int32_t* num_close, double* precision, int32_t* best, double T_refine[16], int32_t* refine_empty,
                      double* pts_final, uint32_t* pairs) {
    // every caller-supplied size is checked before anything is enqueued
    PCREG_ARG(model && pts && locs && T && kp_off && desc_opts && par && num_keypoints && num_desc && num_matches && num_close && precision);
    PCREG_ARG(best && T_refine && refine_empty && pts_final && N >= 1 && ld >= N && ldM >= model->n && (model->n == 0 || featModel));
    if (K < 1) { set_error("pcreg_final_stage: K = %d clusters (at least one)", K); return PCREG_E_ARG; }
    if (kp_off[0] != 0) { set_error("pcreg_final_stage: kp_off[0] = %d (must be 0)", kp_off[0]); return PCREG_E_ARG; }
    for (int k = 0; k < K; ++k)
        if (kp_off[k + 1] < kp_off[k]) { set_error("pcreg_final_stage: kp_off decreases at %d (%d -> %d)", k, kp_off[k], kp_off[k + 1]); return PCREG_E_ARG; }
    const int total = kp_off[K];
    PCREG_ARG(total == 0 || keypoints);
    if (model->D != PCREG_DESC_LEN) {
        set_error("pcreg_final_stage: the model set has D = %d columns, the descriptors have %d", model->D, PCREG_DESC_LEN);
        return PCREG_E_ARG;
    }
    if (par->metric != PCREG_METRIC_SAD) { set_error("pcreg_final_stage: Metric must be SAD (as in pcreg_sphere_sweep)"); return PCREG_E_ARG; }
    PCREG_ARG(desc_opts->R > 0 && desc_opts->k > 0 && desc_opts->min_pts >= 0);
    GUARD();
    const int VM = model->n, D = model->D;
    const size_t n = (size_t)N, k1 = (size_t)K, tot = (size_t)(total > 0 ? total : 1);
    pcreg_desc_opts o = *desc_opts;
    o.ALIGN_POINTS = 0;                                                       // :300 "this false is the key"

    // consecutive batches of clusters whose fp64 descriptors (7.84 KB per keypoint drawn) fit the bound together; a cluster
    // larger than the bound runs alone
    const size_t bound = final_stage_bound(), row_bytes = sizeof(double) * (size_t)D;
    std::vector<int> cut{0};
    size_t acc = 0, batch_rows = 1;
    int S_max = 1;
    for (int k = 0; k < K; ++k) {
        const size_t b = row_bytes * (size_t)(kp_off[k + 1] - kp_off[k]);
        if (k > cut.back() && acc + b > bound) { cut.push_back(k); acc = 0; }
        acc += b;
        S_max = std::max(S_max, kp_off[k + 1] - kp_off[k]);
    }
    cut.push_back(K);
    const int nbatch = (int)cut.size() - 1;
    for (int b = 0; b < nbatch; ++b) batch_rows = std::max(batch_rows, (size_t)(kp_off[cut[b + 1]] - kp_off[cut[b]]));

    Stage st{scratch()};
    double *tmp, *dp, *dT, *dkp, *fm, *cen, *tf, *feat, *desc, *dprec, *dpf; char* ws; int32_t* counters; uint32_t* dpairs;
    const size_t wsb = descriptors_workspace_bytes(N, S_max);
    // int32 block: counters [2K] | n_in [K] | nsel [K] | n_pairs [K] | n_close [K] | empty [K] | best | kp_off [K + 1] | seg_off [K + nbatch]
    const size_t ni = 7 * k1 + 1 + (k1 + 1) + (k1 + (size_t)nbatch);
    TRY(st.take(3 * (size_t)std::max({N, VM, K}), &tmp));
    TRY(st.take(3 * n, &dp));
    TRY(st.take(16 * k1, &dT));
    TRY(st.take(3 * tot, &dkp));
    TRY(st.take(3 * (size_t)std::max(VM, 1), &fm));
    TRY(st.take(3 * k1, &cen));
    TRY(st.take(3 * n * k1, &tf));
    TRY(st.take(3 * tot, &feat));
    TRY(st.take((size_t)D * batch_rows, &desc));
    TRY(st.take(wsb, &ws));
    TRY(st.take(ni, &counters));
    TRY(st.take(17 * k1, &dprec));                          // precision [K] | T16 [K][16]
    TRY(st.take(2 * tot, &dpairs));
    TRY(st.take(3 * n, &dpf));                              // the final surface
    int32_t *n_in = counters + 2 * k1, *nsel = n_in + k1, *n_pairs = nsel + k1, *n_close = n_pairs + k1, *empty = n_close + k1, *dbest = empty + k1;
    int32_t *dkpoff = dbest + 1, *dseg = dkpoff + (k1 + 1);
    double* dT16 = dprec + k1;
    const double* rM = nullptr;
    if (VM > 0) TRY(desc_set_rows(model, &rM));
    std::vector<int32_t> seg_h(k1 + (size_t)nbatch, 0);       // per batch its running sums
    std::vector<int32_t> h_cnt(2 * k1), h_in(k1), h_res(3 * k1 + 1);
    std::vector<double> h_T16(16 * k1);
    DrainAtExit drain;

    // upload; :291 pts_tform = quickTF(ptsSurface, invertTF(transCur)) for every cluster in one launch
    TRY(upload_cols(pts, N, ld, 3, dp, g_stream));
    PCREG_HIP(hipMemcpyAsync(dT, T, sizeof(double) * 16 * k1, hipMemcpyHostToDevice, g_stream));
    TRY(upload_cols(keypoints, total, total, 3, dkp, g_stream));
    TRY(upload_points_aos(featModel, VM, ldM, tmp, fm, g_stream));
    TRY(upload_points_aos(locs, K, K, tmp, cen, g_stream));
    PCREG_HIP(hipMemcpyAsync(dkpoff, kp_off, sizeof(int32_t) * (k1 + 1), hipMemcpyHostToDevice, g_stream));
    PCREG_HIP(hipMemsetAsync(counters, 0, sizeof(int32_t) * 7 * k1, g_stream));
    PCREG_HIP(hipMemsetAsync(dpairs, 0, sizeof(uint32_t) * 2 * tot, g_stream));
    TRY(launch_quick_tf_batched(dp, N, N, dT, K, tf, N, nullptr, g_stream));

    size_t seg_pos = 0;
    for (int b = 0; b < nbatch; ++b) {
        const int k0 = cut[b], kb = cut[b + 1], nb = kb - k0, r0 = kp_off[k0];
        // :309-310 descriptors of every moved surface WITHOUT local alignment (keypoints: the caller's draw, :297)
        for (int k = k0; k < kb; ++k) {
            const int S = kp_off[k + 1] - kp_off[k];
            if (S == 0) continue;
            TRY(launch_descriptors(tf + (size_t)k * 3 * n, N, N, dkp + kp_off[k], S, total, o, 0, feat + (size_t)kp_off[k] * 3,
                                   desc + (size_t)(kp_off[k] - r0) * D, nullptr, nullptr, counters + 2 * k, counters + 2 * k + 1, ws, wsb, g_stream));
        }
        // :319 the model keypoints inside every cluster's sphere, counted
        if (VM > 0) TRY(launch_sphere_counts(fm, VM, cen + (size_t)k0 * 3, nb, R_desc, n_in + k0, g_stream));
        // ---- the sizes: V_k, the over-capacity flags, the sphere counts (one synchronisation per batch)
        PCREG_HIP(hipMemcpyAsync(h_cnt.data() + 2 * (size_t)k0, counters + 2 * (size_t)k0, sizeof(int32_t) * 2 * nb, hipMemcpyDeviceToHost, g_stream));
        PCREG_HIP(hipMemcpyAsync(h_in.data() + k0, n_in + k0, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, g_stream));
        PCREG_HIP(hipStreamSynchronize(g_stream));
        int n_max = 0, v_max = 0;
        int32_t* sh = seg_h.data() + seg_pos;
        sh[0] = 0;
        for (int k = k0; k < kb; ++k) {
            if (h_cnt[2 * k + 1]) {
                set_error("a support holds %d points: more than an LDS-resident support may have (lower max_pts)", h_cnt[2 * k + 1]);
                return PCREG_E_ARG;
            }
            sh[k - k0 + 1] = sh[k - k0] + h_in[k];
            n_max = std::max(n_max, (int)h_in[k]); v_max = std::max(v_max, (int)h_cnt[2 * k]);
        }
        const int tot_b = sh[nb];
        int32_t* dsb = dseg + seg_pos;
        seg_pos += (size_t)nb + 1;
        // sized from the counts just read: a copy of the walk per batch, so that every batch meets the same four slots
        Stage bst = st;
        int32_t* rows; double *featCur, *descCur; char* mws;
        size_t off6[6];
        const size_t mwsb = dev_get_matches_layout(std::max(v_max, 1), std::max(n_max, 1), D, D + 1, off6);
        TRY(bst.take((size_t)std::max(tot_b, 1), &rows));
        TRY(bst.take(3 * (size_t)std::max(tot_b, 1), &featCur));
        TRY(bst.take((size_t)D * (size_t)std::max(n_max, 1), &descCur));
        TRY(bst.take(mwsb, &mws));
        PCREG_HIP(hipMemcpyAsync(dsb, sh, sizeof(int32_t) * ((size_t)nb + 1), hipMemcpyHostToDevice, g_stream));
        if (VM > 0) TRY(launch_sphere_select_batched(fm, VM, cen + (size_t)k0 * 3, nb, R_desc, dsb, rows, featCur, nsel + k0, g_stream));
        // :321-344 descCur = descModel_noLRF(mask, :), matches = getMatches(desc, descCur, par)
        for (int k = k0; k < kb; ++k) {
            const int v = h_cnt[2 * k], m = h_in[k];
            if (v == 0 || m == 0) continue;
            TRY(launch_gather_rows_f64(rM, D, rows + sh[k - k0], nsel + k, m, descCur, g_stream));
            TRY(dev_get_matches_impl(desc + (size_t)(kp_off[k] - r0) * D, v, D, descCur, m, D, D, PCREG_LAYOUT_ROW_MAJOR, par,
                                     dpairs + (size_t)kp_off[k] * 2, nullptr, n_pairs + k, mws, mwsb, g_stream));
        }
        // :357-391 the close matches, the precision and the refined transform of every cluster of the batch
        TRY(launch_final_close_refine_batched(dpairs, n_pairs + k0, feat, dkpoff + k0, featCur, dsb, nb, maxDist, n_close + k0, dprec + k0,
                                              dT16 + (size_t)k0 * 16, empty + k0, g_stream));
    }
    // :381-394 the best cluster, invertTF(T_refine), the final surface -- on the device
    TRY(launch_final_pick_apply(dprec, dT16, empty, K, tf, N, N, dpf, N, dbest, g_stream));
    // ---- the results (one synchronisation)
    PCREG_HIP(hipMemcpyAsync(h_res.data(), n_pairs, sizeof(int32_t) * (3 * k1 + 1), hipMemcpyDeviceToHost, g_stream));   // n_pairs | n_close | empty | best
    PCREG_HIP(hipMemcpyAsync(precision, dprec, sizeof(double) * k1, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(h_T16.data(), dT16, sizeof(double) * 16 * k1, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipMemcpyAsync(pts_final, dpf, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, g_stream));
    if (pairs && total > 0) PCREG_HIP(hipMemcpyAsync(pairs, dpairs, sizeof(uint32_t) * 2 * (size_t)total, hipMemcpyDeviceToHost, g_stream));
    PCREG_HIP(hipStreamSynchronize(g_stream));
    for (int k = 0; k < K; ++k) {
        num_keypoints[k] = h_cnt[2 * k]; num_desc[k] = h_in[k];
        num_matches[k] = h_res[k]; num_close[k] = h_res[k1 + k];
    }
    const int bsel = h_res[3 * k1];
    *best = bsel;
    *refine_empty = h_res[2 * k1 + bsel];
    memcpy(T_refine, h_T16.data() + (size_t)bsel * 16, sizeof(double) * 16);
    return PCREG_OK;
}

}  // extern "C"
