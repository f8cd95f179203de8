// pcreg_amd/csrc/common.hpp -- shared host-side helpers of libpcreg_hip (gfx950 only).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <string>
#include "../../include/pcreg.h"

namespace pcreg {

void set_error(const char* fmt, ...);
int  ensure_device();   // PCREG_OK or PCREG_E_NODEVICE / PCREG_E_HIP

#define PCREG_HIP(call)                                                                  \
    do {                                                                                 \
        hipError_t e__ = (call);                                                         \
        if (e__ != hipSuccess) {                                                         \
            ::pcreg::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),   \
                               __FILE__, __LINE__);                                      \
            return PCREG_E_HIP;                                                          \
        }                                                                                \
    } while (0)

#define PCREG_ARG(cond)                                                                  \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            ::pcreg::set_error("bad argument: %s (%s:%d)", #cond, __FILE__, __LINE__);   \
            return PCREG_E_ARG;                                                          \
        }                                                                                \
    } while (0)

// Grow-only device scratch owned by the host tier (one per process; MEX calls arrive
// on MATLAB's interpreter thread).  Slots keep independent
// buffers alive across one call.
struct Scratch {
    static constexpr int kSlots = 24;     // the longest chain is pcreg_sphere_sweep's: 14 of its own, 4 of the sphere head, 1 of the pair fetch
    void*  ptr[kSlots]  = {};
    size_t size[kSlots] = {};
    int get(int slot, size_t bytes, void** out);
    void release_all();
};
Scratch& scratch();
// one host-tier call's walk over a Scratch: buffers are taken in order, so a helper that is handed the walk
// continues behind its caller's buffers and cannot collide with them
struct Stage {
    Scratch& s; int next = 0;
    template <class T> int take(size_t count, T** out) {       // PCREG_OK / PCREG_E_*; count 0 still yields a valid pointer
        void* p = nullptr;
        const int rc = s.get(next, count * sizeof(T), &p);
        if (rc == PCREG_OK) ++next;
        *out = (T*)p;
        return rc;
    }
};

// Switches.  Two kinds, and NEITHER reads the environment in the default build (a stray variable in a MATLAB worker's
// environment must not change which kernels run):
//  * result-preserving A/B switches (the direct-form search, the exhaustive fp64 SAD, the forced fallback of the certified
//    matcher, the fused / fp64-only RANSAC kernels, ...): process-wide integers set through pcreg_debug_set(key, value) --
//    the entry the parity tests call to run both sides of a certified path inside one process; every setting gives the same
//    indices and counts;
//  * experiment / debug switches that change the launch shape, print, synchronise, write files or INVALIDATE results
//    (timing-only kernels): environment variables that exist only in a build with -DPCREG_EXPERIMENTS (`make EXPERIMENTS=1`);
//    the default library compiles them to their default value.
enum DebugKey {
    kDbgKnnExact = 0,          // "knn_exact": direct-form fp32 search instead of the certified f16 matrix-core path
    kDbgMatchExact,            // "match_exact": exhaustive fp64 SAD instead of the certified u16 path
    kDbgMatchForceFallback,    // "match_force_fallback": 1 = every query takes the exact fallback, 2 = also skip the refine
    kDbgRansacFused,           // "ransac_fused": n >= 4096 on the fused tiled kernel instead of the staged chain
    kDbgRansacNoLane,          // "ransac_nolane": refit sums by the fp64 sweep kernel instead of the int8 matrix-core kernel
    kDbgRansacF64Score,        // "ransac_f64score": no fp32 screen in the staged chain
    kDbgRansacResidentF64,     // "ransac_resident_f64": the round-3 fp64 LDS-resident kernel instead of ransac_hyp32_kernel
    kDbgAlignTimes,            // "align_times": per-phase timestamps of align_points_knn (host read-back)
    kDbgAlignShape,            // "align_shape": launch-shape override of align_points_knn
    kDbgSegDebug,              // "seg_debug": histogram dump of the segmented matcher
    kDbgSegBatched,            // "seg_batched": the segmented matcher runs its bounded-workspace (batched) form whatever the size
    kDbgSegWaveFinalize,       // "seg_wave_finalize": the segmented matcher's forward re-rank as one wave per query (rounds 2-3) instead of pick / pairs / decide
    kDbgMatchStats,            // "match_stats": the certified matcher counts what it proves / re-scores / hands on (pcreg_debug_match_stats)
    kDbgFinalBatchMB,          // "final_batch_mb": pcreg_final_stage's descriptor memory bound in MB instead of 4 GB (0 = the default)
    kDbgKnnNoCull,             // "knn_nocull": the point search's candidate kernel visits every model tile (no culling)
    kDbgKnnStats,              // "knn_stats": the point search counts what it visits (pcreg_debug_knn_stats)
    kDbgRansacPass2,           // "ransac_pass2": the staged chain's second scoring pass -- 0 by shape (bounded_pays), 1 always the full pass,
                               // 2 always the bounded pass where it is allowed
    kDbgRansacStats,           // "ransac_stats": the bounded pass counts what it scans (pcreg_debug_ransac_stats)
    kDbgRangeSortCap,          // "range_sort_cap": n > 0 -- the radius search orders segments longer than n rows by its in-place
                               // large-segment path (0 = the default capacity)
    kDbgClusterNoSkip,         // "cluster_noskip": the clustering walk unites on every hit (no "same root" early-out)
    kDbgClusterStats,          // "cluster_stats": the clustering walk counts hits and compare-and-swaps (pcreg_debug_cluster_stats)
    kDbgKnnTailCap,            // "knn_tail_cap": n > 0 -- the point search's exact tail (few-form) lists the surviving tiles of n tiles per
                               // pass instead of its LDS list's capacity
    kDbgScoreBatchSlots,       // "score_batch_slots": n > 0 -- the transform scoring batches whole transforms under n query slots instead
                               // of 4 Mi (at least one transform a batch), to reach its batch loop at a small size
    kDbgFpfhRadiusLanes,       // "fpfh_radius_lanes": 4 or 16 -- the radius FPFH's SPFH kernel walks a row's segment with that many lanes
                               // instead of 64 (a wave); the counts are integers, so every setting gives the same bits
    kDbgDescStats,             // "desc_stats": the descriptor kernel counts the rare branches it takes (pcreg_debug_desc_stats)
    kDbgKnnDirect,             // "knn_direct": 0 = the two-nearest search answers the seeded queries with a small cell range from their
                               // ordering-grid cells (knn_direct_kernel), 1 = every query takes the tile walk; same bits
    kDbgKnnDirectStats,        // "knn_direct_stats": the direct answers are counted (pcreg_debug_knn_direct_stats); forces nothing
    kDbgKnnSeedFused,          // "knn_seed_fused": 0 = seeding and the direct answers are one launch (seed_direct_kernel), 1 = two launches
                               // (seed_query_kernel, knn_direct_kernel); same bits
    kDbgRansacBHand,           // "ransac_bhand": 0 = the bounded second pass hands the refits still undecided after kBHand blocks to its
                               // block-parallel finish (rs_bfinish_kernel), 1 = it walks every refit to its stop; same bits
    kDbgFgrChain,              // "fgr_chain": 1 = fast global registration runs its chained form (a sums and a finish launch per iteration)
                               // whatever the size instead of the resident kernel; same bits
    kDbgCount
};
int debug_flag(DebugKey k);
// Device counters of the certified SAD matcher (match_sad16.hip), or null while "match_stats" is off:
//   [0] queries finalised   [1] candidates re-scored exactly (fp64)   [2] queries the certificate left unproven
//   [3] queries handed to the exhaustive exact-rows kernel   [4] Unique back-check items (segmented form)
//   [5] back-check items handed to the exhaustive kernel   [6] matcher calls   [7] segments
unsigned long long* match_stats_dev();
// Device counters of the point search (knn_fast.hip), or null while "knn_stats" is off:
//   [0] searches   [1] visited (query block, model tile) pairs   [2] nominal pairs (q_blocks x n_tiles)   [3] queries sent to the tail
//   [4] (wave, 64-row unit) pairs scored inside the visited tiles   [5] 32 x visited pairs (pcreg_debug_knn_unit_stats reads [4], [5])
unsigned long long* knn_stats_dev();
// Device counters of the direct answers (knn_fast.hip: knn_direct_kernel), or null while "knn_direct_stats" is off:
//   [0] two-nearest searches   [1] queries answered from their ordering-grid cells   [2] rows ranked for them
unsigned long long* knn_direct_stats_dev();
// Device counters of the farthest point sampling (knn_fps.hip), or null while "knn_stats" is off:
//   [0] steps run   [1] rows measured against a sample (pcreg_debug_fps_stats)
unsigned long long* fps_stats_dev();
// Device counters of the staged RANSAC chain's bounded second pass (ransac.hip), or null while "ransac_stats" is off:
//   [0] bounded passes run   [1] (refit, 512-correspondence block) units scanned, seed refits included   [2] units a full pass scans
//   [3] refits handed over to the finish   [4] units the finish scored, also part of [1] (pcreg_debug_ransac_handover reads [3], [4])
unsigned long long* ransac_stats_dev();
// Device counters of the clustering walk (knn_cluster.hip), or null while "cluster_stats" is off:
//   [0] calls   [1] hits   [2] compare-and-swap attempts   [3] failed attempts
unsigned long long* cluster_stats_dev();
// Device counters of the descriptor kernel (descriptors.hip), or null while "desc_stats" is off -- keypoints that:
//   [0] reached the K-nearest selection   [1] selected by bisection (a crowded bin)   [2] counted the tie group with the full pass
//   [3] ranked a tie group by original index   [4] retook every vote in fp64   [5] were re-binned literally (> 128 deferred points);
//   [6] points that reached bin_literal   [7] (wave, chunk) pairs re-tested past the kept ballots
//   [8] the last call's grid subdivision, fx << 16 | fy << 8 | fz (stored, not added)
//   [9] deferred points binned one by one in fp64 (the supports with at most 128 of them)
// While the key is on, launch_descriptors runs desc_kernel's counting instantiation; the default one holds no counting code.
unsigned long long* desc_stats_dev();
#ifdef PCREG_EXPERIMENTS
static inline int pcreg_env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static inline const char* pcreg_env_str(const char* name) { return getenv(name); }
#define PCREG_EXP_ENV(name, dflt) pcreg_env_int(name, dflt)
#define PCREG_EXP_STR(name) pcreg_env_str(name)
#else
#define PCREG_EXP_ENV(name, dflt) (dflt)
#define PCREG_EXP_STR(name) ((const char*)nullptr)
#endif

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// One walk over a caller-allocated workspace: a layout function takes its buffers in order; the size
// function runs it with base == nullptr (measure only: every pointer null), the launcher with the caller's block.
struct WsWalk {
    char* base; size_t off = 0;
    explicit WsWalk(void* b) : base((char*)b) {}
    void* take_bytes(size_t bytes) { void* p = base ? base + off : nullptr; off += bytes; return p; }   // the fixed 256 / 512 / 1024 slots
    template <class T> T* take(size_t count, size_t align = 256) { return (T*)take_bytes(align_up(count * sizeof(T), align)); }
    size_t bytes() const { return off; }
};

// copy an n x cols column-major host matrix (leading dimension ld) to a compact device
// matrix (leading dimension n)
template <typename T>
static int upload_cols(const T* host, int n, int ld, int cols, T* dev, hipStream_t st) {
    if (n <= 0 || cols <= 0) return PCREG_OK;
    if (ld == n) { PCREG_HIP(hipMemcpyAsync(dev, host, sizeof(T) * (size_t)n * cols, hipMemcpyHostToDevice, st)); }
    else PCREG_HIP(hipMemcpy2DAsync(dev, sizeof(T) * (size_t)n, host, sizeof(T) * (size_t)ld, sizeof(T) * (size_t)n, cols, hipMemcpyHostToDevice, st));
    return PCREG_OK;
}

// ---- kernel launchers implemented in the .hip files (device pointers, async) --------
struct RansacDims { int n_cap; int iters; int B; };

size_t ransac_workspace_bytes(int iters, int B, int n_cap);
int ransac_handover_blocks();      // kBHand: blocks the bounded second pass walks before it hands over
int launch_ransac(const double* p1, const double* p2, int ld, const int32_t* offsets /*B+1 dev or null*/,
                  const int32_t* n_dev /*single registration: device n, or null*/, int n_cap, int B,
                  const pcreg_ransac_opts& o, const int32_t* sample_idx_dev,
                  pcreg_dev_ransac_result* out /*B*/, int32_t* inlier_idx, int32_t* iter_inl /*B*iters or null*/,
                  int32_t* iter_inl_ref, void* ws, size_t ws_bytes, hipStream_t st);
int launch_ransac_partial(const double* p1, const double* p2, int ld, const int32_t* n_dev, int n_cap,
                          const pcreg_ransac_opts& o, const int32_t* sample_idx_dev, int hyp_begin, int hyp_count,
                          pcreg_dev_ransac_part* part, void* ws, size_t ws_bytes, hipStream_t st);
int launch_ransac_finish(const double* p1, const double* p2, int ld, const int32_t* n_dev, int n_cap,
                         const pcreg_ransac_opts& o, const pcreg_dev_ransac_part* combined,
                         pcreg_dev_ransac_result* out, int32_t* inlier_idx, hipStream_t st, int n_parts = 1);
int launch_estimate_transform(const double* p1, const double* p2, int n, int ld, double* T16_dev,
                              int32_t* empty_dev, hipStream_t st);
int launch_calc_dists(const double* T16_dev, const double* p1, const double* p2, int n, int ld,
                      double* d, hipStream_t st);

// a prepared model (knn_fast.hip): pointers into one device block of model_prep_bytes(M) bytes + the caller's points
struct ModelView {
    const float* m; int M, ldm;
    void* prep; unsigned* rm2; float* box_part; void* tiles; int32_t* seed_cnt; void* seed_slots; int seeded;
    // the rows in spatial order: perm[sorted row] = row of m, an fp32 SoA copy (ld = M), one box per f16 tile; the
    // ordering grid's counters
    int32_t* perm; float* ms; float* tbox; int32_t* sort_cnt;
    float* ubox;               // one box per UNIT of 64 consecutive sorted rows, [n_tiles * 8][6]; an empty unit holds (+inf, -inf)
};
size_t model_prep_bytes(int M);
ModelView model_view(const float* m, int M, int ldm, void* block);
int launch_model_prepare(const ModelView& v, hipStream_t st);
// the per-call workspace of a search and of the match stage that follows it
struct SearchWs {
    void* ctr; unsigned* gthr; int32_t* flag_list; int32_t* cand_cnt; void* cand_ent; int cap;
    int32_t* tail_idx; float* tail_dist;
    void* ug_prep; float* ug_part; int32_t* ug_cnt; void* ug_slots; int ug_cells, ug_nparts;
    int32_t* qcnt; int32_t* qperm; float* dk;          // the call's query order (counters, slot -> query) and seed distances
    int32_t* n_vis; int32_t* vis_list;                 // the visit plan: tiles to visit per query block, [q_blocks] and [q_blocks][n_tiles] (inside tail_idx's slot)
    uint32_t* vis_mask;                                // ... and per list position the units each candidate wave scores, [q_blocks][n_tiles] (same slot)
};
SearchWs search_ws_layout(int Q, int M, void* base, size_t* bytes);
size_t search_ws_bytes(int Q, int M);
// test hooks (pcreg_debug_dev_model_export, pcreg_debug_search_export): copies out of a prepared model / a search workspace
int model_export(const ModelView& v, int32_t* perm, float* sorted_soa, float* tile_box, float prep[24], hipStream_t st);
int search_export(const void* ws, size_t ws_bytes, int Q, int M, int32_t* qperm, float* dk, hipStream_t st);
int launch_model_search(const ModelView& v, const float* q, int Q, int ldq, int32_t idx_base, int32_t* idx, float* dist,
                        void* ws, size_t ws_bytes, bool with_grid, bool timed, hipStream_t st);
// S1b alone (scan of the per-parent-cell counts qcnt [kQueryKeys], then the slots qperm [Q]) for a search of its own
int launch_query_order(const ModelView& v, const float* q, int Q, int ldq, int32_t* qcnt, int32_t* qperm, hipStream_t st);
// the k nearest model rows per query (knn_k.hip): idx / dist [Q][k], (distance, original row) order, exact fp32
size_t knn_k_ws_bytes(int Q, int M, int k);
int launch_model_knn(const ModelView& v, const float* q, int Q, int ldq, int k, int32_t idx_base, int32_t* idx, float* dist,
                     void* ws, size_t ws_bytes, hipStream_t st);
int launch_merge_topk_f32(const int32_t* idx_in, const float* dist_in, int R, int Q, int k, size_t rank_stride, int32_t* idx, float* dist,
                          hipStream_t st);
// rows within a squared radius per query (knn_range.hip): count + scan, then fill + order; one workspace size serves both
size_t range_ws_bytes(int Q, int M);
int launch_model_range_count(const ModelView& v, const float* q, int Q, int ldq, float r2, int32_t* counts, int64_t* seg_off, void* ws,
                             size_t ws_bytes, hipStream_t st);
int launch_model_range_fill(const ModelView& v, const float* q, int Q, int ldq, float r2, int32_t idx_base, const int64_t* seg_off,
                            int64_t capacity, int32_t* idx, float* dist, void* ws, size_t ws_bytes, hipStream_t st);
// the radius search's R1 alone: the per-parent-cell counts of the queries, into a cleared qcnt [kQueryKeys + 64] (knn_range.hip)
int launch_query_cells(const ModelView& v, const float* q, int Q, int ldq, int32_t* qcnt, hipStream_t st);
// B transforms of one query cloud scored against the model (knn_score.hip): per transform the queries with a row within r2 and
// the sum of their squared distances; idx / dist [B][Q] (either may be null) the nearest such row, -1 / +inf for none
// `trim` (every launcher below that takes one; null: none, and nothing more is launched): keep only each transform's closest
// pairs (knn_trim.hip) -- keep_ratio in (0, 1]; n_within [B] the pairs within r2, d2_cut [B] the largest kept d,
// either may be null.  The workspace is the untrimmed call's: the pass works in blocks that are dead between the walk and the sums
struct TrimIo { double keep_ratio; int32_t* n_within; float* d2_cut; };
constexpr size_t kTrimSelBytes = 16;               // the select state of a transform (knn_trim.hip)
// ... the pass itself on nb transforms' best [nb][Q] (Q > 0, chunks = ceil(Q / 2048)): hist [nb][256], sel [nb] states, tie [nb chunks];
// idx / dist the caller's tables at the batch's first transform, or null; n_within / d2_cut at it too, or null
int launch_score_trim(float* best, int Q, int chunks, int nb, double keep_ratio, int32_t* hist, void* sel, int32_t* tie, int32_t* idx, float* dist,
                      int32_t* n_within, float* d2_cut, hipStream_t st);
// ... and of a call without pairs: n_within = 0, d2_cut = +inf
int launch_trim_empty(int B, int32_t* n_within, float* d2_cut, hipStream_t st);
size_t score_ws_bytes(int Q, int B, int M);
int launch_model_score(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, float r2, int32_t* n_close,
                       double* sum_d2, int32_t* idx, float* dist, void* ws, size_t ws_bytes, hipStream_t st, const TrimIo* trim = nullptr);
// the same B transforms each refitted on its close pairs (knn_score.hip): T_step = estimateTransform(model rows, moved
// points) over the queries with a row within r2, T_out = T * T_step, empty[b] = 1 and zeros where there is no fit; n_close and
// sum_d2 are launch_model_score's bits.  T_step may be null; T_out may not alias T_dev
size_t refit_ws_bytes(int Q, int B, int M);
int launch_model_refit(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, float r2, double* T_out, double* T_step,
                       int32_t* n_close, double* sum_d2, int32_t* empty, void* ws, size_t ws_bytes, hipStream_t st, const TrimIo* trim = nullptr);
// ... its last step per batch of nb transforms (ransac.hip, where fit_moments and fit_3pt live): chunk moments pmom [nb][chunks][27]
// about origin[0..2], the batch's per-slot buffers best / tq / win (ld S), n_close [nb] already totalled
int launch_refit_finish(const double* pmom, const int32_t* n_close, const float* best, const float* tq, const float* win, int Q, int S, int chunks,
                        int nb, const float* origin, const double* T_in, double* T_out, double* T_step, int32_t* empty, hipStream_t st);
// a refit call without pairs (Q = 0 or no rows), whatever the method (knn_score.hip): every transform empty = 1 with 32 zeros,
// and a zero in each of the method's per-transform outputs that is not null
struct RefitEmptyOuts { double* d[4]; int32_t* n; };
int launch_refit_empty(int B, double* T_out, double* T_step, int32_t* empty, const RefitEmptyOuts& z, hipStream_t st);
// the same chain with the point-to-plane fit in estimateTransform's place (knn_score.hip, plane_fit.hpp): normals
// [3][ldn] on the device by ORIGINAL row; n_plane the pairs whose row has a finite normal, sum_res2 their squared plane residuals
size_t refit_plane_ws_bytes(int Q, int B, int M);
int launch_model_refit_plane(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, float r2, const float* normals, int ldn,
                             double* T_out, double* T_step, int32_t* n_close, double* sum_d2, int32_t* n_plane, double* sum_res2, int32_t* empty,
                             void* ws, size_t ws_bytes, hipStream_t st, const TrimIo* trim = nullptr);
// the same chain with the plane-to-plane (generalized ICP) sums in the point-to-plane ones' place (knn_score.hip, gicp_pair.hpp; DESIGN
// 4.26): qnormals [3][ldnq] on the device by query; n_pairs the pairs both of whose normals are finite and whose S factorises,
// sum_res2 their e . (W e).  The workspace is the plane refit's
size_t refit_gicp_ws_bytes(int Q, int B, int M);
int launch_model_refit_gicp(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, float r2, const float* normals, int ldn,
                            const float* qnormals, int ldnq, double epsilon, double* T_out, double* T_step, int32_t* n_close, double* sum_d2,
                            int32_t* n_pairs, double* sum_res2, int32_t* empty, void* ws, size_t ws_bytes, hipStream_t st, const TrimIo* trim = nullptr);
// one coherent-point-drift step of the same B transforms (cpd.hip, cpd_fit.hpp): every moved point against every live
// model row, B Q M pairs; sigma2_in [B] on the device (0: the closed-form initial value), outlier in [0, 1); sum_d2 the scoring chain's
// at r2 = +inf (the shift), n_live the queries whose moved point is finite.  T_step may be null; T_out may not alias T_dev
size_t refit_cpd_ws_bytes(int Q, int B, int M);
int launch_model_refit_cpd(const ModelView& v, const float* q, int Q, int ldq, const double* T_dev, int B, const double* sigma2_in, double outlier,
                           double* T_out, double* T_step, double* sigma2_out, double* Np, double* sum_res2, double* sum_d2, int32_t* n_live,
                           int32_t* empty, void* ws, size_t ws_bytes, hipStream_t st);
// connected components of "distance <= r2" over the model's own rows (knn_cluster.hip): walk + union-find, flatten, number
size_t cluster_ws_bytes(int M);
int launch_model_cluster(const ModelView& v, float r2, int32_t* label, int32_t* n_clusters, int32_t* first, int32_t* sizes, void* ws,
                         size_t ws_bytes, hipStream_t st);
// DBSCAN over the model's own rows: count walk, core union walk, flatten, number, border walk, label.  label [M],
// core [M] (or null), count [M] (or null), first / sizes [M] (or null) by ORIGINAL row / cluster, n_clusters one int32 -- device
// pointers.  The launcher and the union-find's kernels are knn_cluster.hip's; the two walks without a union are knn_dbscan.hip's:
//   enqueue_dbscan_count   cnt_sorted[sorted row] = the row's neighbours, itself included (0 for a non-finite row); then, by
//                          ORIGINAL row, cnt[i] the same, parent[i] = i, first / sizes cleared
//   enqueue_dbscan_border  after the flatten: parent[i] of a non-core row with a core neighbour = the smallest root among them
size_t dbscan_ws_bytes(int M);
int launch_model_dbscan(const ModelView& v, float r2, int minpts, int32_t* label, int32_t* n_clusters, uint8_t* core, int32_t* count,
                        int32_t* first, int32_t* sizes, void* ws, size_t ws_bytes, hipStream_t st);
void enqueue_dbscan_count(const ModelView& v, float r2, int cull, int32_t* cnt_sorted, int32_t* cnt, int32_t* parent, int32_t* first,
                          int32_t* sizes, hipStream_t st);
void enqueue_dbscan_border(const ModelView& v, float r2, int cull, const int32_t* cnt_sorted, int minpts, int32_t* parent, hipStream_t st);
// the surface normal of every model row from its k nearest rows (knn_normals.hip): normals [3][ldn] and variation [M]
// (or null) by ORIGINAL row; viewpoint: three host doubles or null
size_t normals_ws_bytes(int M, int k);
int launch_model_normals(const ModelView& v, int k, const double* viewpoint, float* normals, int ldn, float* variation, void* ws,
                         size_t ws_bytes, hipStream_t st);
// statistical outlier removal over the model's own rows (knn_denoise.hip): mean_dist [M] by ORIGINAL row, inliers
// [<= M] ascending with n_inliers, stats [4] = thr, mu, sd, nf -- device pointers, each may be null (inliers needs n_inliers)
size_t denoise_ws_bytes(int M, int k);
int launch_model_denoise(const ModelView& v, int k, double threshold, double* mean_dist, int32_t* inliers, int32_t* n_inliers, double* stats,
                         void* ws, size_t ws_bytes, hipStream_t st);
// farthest point sampling of the model's own rows (knn_fps.hip): idx / dist [K] in selection order, n_out, cover_d2 and
// info single device words, min_dist / label [M] by ORIGINAL row -- device pointers, each may be null except n_out.  fps_args_ok and
// fps_max_rows are the argument rules every tier checks before it touches the device
size_t fps_ws_bytes(int M, int K);
bool fps_args_ok(int M, int K, int start, float stop_d2);
int fps_max_rows();
int launch_model_fps(const ModelView& v, int K, int start, float stop_d2, int32_t* idx, float* dist, int32_t* n_out, float* cover_d2,
                     float* min_dist, int32_t* label, int32_t* info, void* ws, size_t ws_bytes, hipStream_t st);
// the FPFH descriptor of every model row from its k nearest rows and a normal per row (knn_fpfh.hip): normals [3][ldn]
// on the device by ORIGINAL row; fpfh [M][33] doubles and spfh [M][33] uint8 counts (or null), row-major by ORIGINAL row
size_t fpfh_ws_bytes(int M, int k);
int launch_model_fpfh(const ModelView& v, int k, const float* normals, int ldn, double* fpfh, uint8_t* spfh, void* ws, size_t ws_bytes,
                      hipStream_t st);
// the FPFH descriptor of every model row from the rows within a squared radius (knn_fpfh_radius.hip): the count call is
// the radius search's with the model's own rows as the queries; the second call fills the lists into the workspace and runs the
// two kernels.  normals [3][ldn] by ORIGINAL row; fpfh [M][33] doubles, spfh [M][33] uint32 counts (or null) and n_neighbors [M]
// (or null), row-major by ORIGINAL row.  fpfh_radius_max_rows is the per-call row limit every tier checks before the device
size_t fpfh_radius_ws_bytes(int M, int64_t capacity);
int fpfh_radius_max_rows();
int launch_model_fpfh_radius_count(const ModelView& v, float r2, int32_t* counts, int64_t* seg_off, void* ws, size_t ws_bytes, hipStream_t st);
int launch_model_fpfh_radius(const ModelView& v, float r2, int max_neighbors, const float* normals, int ldn, const int64_t* seg_off,
                             int64_t capacity, double* fpfh, uint32_t* spfh, int32_t* n_neighbors, void* ws, size_t ws_bytes, hipStream_t st);
// ISS keypoints of the model's own rows (knn_iss.hip): n_neighbors [M], eig [M][3] (or null) and saliency [M] by ORIGINAL
// row, keypoints [<= M] ascending with n_keypoints (both may be null; keypoints needs n_keypoints) -- device pointers.  iss_args_ok
// and iss_max_rows are the argument rules every tier checks before it touches the device
size_t iss_ws_bytes(int M);
bool iss_args_ok(float r2_salient, float r2_nonmax, double gamma21, double gamma32, int min_neighbors);
int iss_max_rows();
int launch_model_iss(const ModelView& v, float r2_salient, float r2_nonmax, double gamma21, double gamma32, int min_neighbors,
                     int32_t* n_neighbors, double* eig, double* saliency, int32_t* keypoints, int32_t* n_keypoints, void* ws, size_t ws_bytes,
                     hipStream_t st);
// MSAC plane fitting and extraction over the model's own rows (knn_planes.hip): labels [M] by ORIGINAL row, planes [P][4],
// centres [P][3], counts [P], rmse [P], n_planes and the diagnostics best_trial / best_cost / best_count [P] (each may be null) --
// device pointers; ref_vec three HOST doubles or null; samples [P][B][3] on the device or null.  planes_args_ok and planes_max_rows
// are the argument rules every tier checks before it touches the device
size_t planes_ws_bytes(int M, int B);
bool planes_args_ok(float max_distance, const double* ref_vec, double max_angle, int max_planes, int n_trials, int min_inliers);
int planes_max_rows();
int launch_model_fit_planes(const ModelView& v, float max_distance, const double* ref_vec, double max_angle, int max_planes, int n_trials,
                            int min_inliers, unsigned long long seed, const int32_t* samples, int32_t idx_base, int32_t* labels,
                            double* planes, double* centres, int32_t* counts, double* rmse, int32_t* n_planes, int32_t* best_trial,
                            int64_t* best_cost, int32_t* best_count, void* ws, size_t ws_bytes, hipStream_t st);
// MSAC sphere fitting and extraction over the model's own rows (knn_fitsphere.hip): labels [M] by ORIGINAL row, spheres
// [P][4] (cx, cy, cz, R), counts [P], rmse [P], refit_used [P], n_spheres and the diagnostics best_trial / best_cost / best_count [P]
// (each may be null) -- device pointers; samples [P][B][4] on the device or null.  fit_spheres_args_ok and fit_spheres_max_rows are
// the argument rules every tier checks before it touches the device
size_t fit_spheres_ws_bytes(int M, int B);
bool fit_spheres_args_ok(float max_distance, float min_radius, float max_radius, int max_spheres, int n_trials, int min_inliers);
int fit_spheres_max_rows();
int launch_model_fit_spheres(const ModelView& v, float max_distance, float min_radius, float max_radius, int max_spheres, int n_trials,
                             int min_inliers, unsigned long long seed, const int32_t* samples, int32_t idx_base, int32_t* labels,
                             double* spheres, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_spheres, int32_t* best_trial,
                             int64_t* best_cost, int32_t* best_count, void* ws, size_t ws_bytes, hipStream_t st);
// MSAC cylinder fitting and extraction over the model's own rows and their normals (knn_fitcylinder.hip): normals
// [3][ldn] on the device by ORIGINAL row, labels [M], cylinders [P][7] (cx, cy, cz, wx, wy, wz, R), extents [P][2], counts [P], rmse
// [P], refit_used [P], n_cylinders and the diagnostics best_trial / best_cost / best_count [P] (each may be null) -- device pointers;
// samples [P][B][2] on the device or null; ref_vec three HOST doubles or null.  fit_cylinders_args_ok and fit_cylinders_max_rows
// are the argument rules every tier checks before it touches the device
size_t fit_cylinders_ws_bytes(int M, int B);
bool fit_cylinders_args_ok(float max_distance, float min_radius, float max_radius, const double* ref_vec, double max_angle,
                           int max_cylinders, int n_trials, int min_inliers);
int fit_cylinders_max_rows();
int launch_model_fit_cylinders(const ModelView& v, float max_distance, float min_radius, float max_radius, const double* ref_vec,
                               double max_angle, const float* normals, int ldn, int max_cylinders, int n_trials, int min_inliers,
                               unsigned long long seed, const int32_t* samples, int32_t idx_base, int32_t* labels, double* cylinders,
                               double* extents, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_cylinders,
                               int32_t* best_trial, int64_t* best_cost, int32_t* best_count, void* ws, size_t ws_bytes, hipStream_t st);
// unique(A, 'rows') of n x 3 doubles and the aggregation of matches on it (unique_rows.hip): tile sort, merge passes, compaction
size_t unique_rows3_ws_bytes(int n_cap);
int launch_unique_rows3(const double* A, const int32_t* n_dev, int n_cap, int ld, int32_t idx_base, int32_t* ia, int32_t* n_unique, void* ws,
                        size_t ws_bytes, hipStream_t st);
size_t aggregate_matches_ws_bytes(int n_cap);
int launch_aggregate_matches(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld, double* out1, double* out2, int ldo,
                             int32_t idx_base, int32_t* ia, int32_t* n_out, void* ws, size_t ws_bytes, hipStream_t st);
// pcdownsample(pc, 'gridAverage', step) of n x 3 fp32 rows (downsample.hip): limits, keys, a stable radix sort of (key, row)
// records, heads + chunk scan, ordered means.  n_out and info are single device words; count and label may be null
size_t downsample_grid_ws_bytes(int n);
int downsample_grid_chunk();                        // records per workgroup of the sort (the tests' T)
int launch_downsample_grid(const float* pts, int n, int ld, double step, float* out, int ldo, int32_t* count, int32_t* label, int32_t* n_out,
                           int32_t* info, void* ws, size_t ws_bytes, hipStream_t st);
// ... its chain up to the voxel order (D1 .. D6), for another consumer of the order (ndt.hip): the header the device derives, the
// two buffers of rows of which hdr->passes & 1 picks the sorted one (live rows first, by voxel, ascending row inside a voxel) and
// the first record of every voxel; *n_out voxels.  The workspace is launch_downsample_grid's
struct VoxelHdr {
    float lo[3], hi[3];
    int32_t w[3];                                    // bits of the largest cell index per axis
    int32_t used;                                    // key bits the sort orders by: w0 + w1 + w2 (+ 1 with a dead row)
    int32_t passes;                                  // ceil(used / 8)
    int32_t info;                                    // 1: refused
    int32_t n_live;
};
struct VoxelOrder { const VoxelHdr* hdr; const uint32_t* row[2]; const int32_t* vstart; };
int launch_voxel_order(const float* pts, int n, int ld, double step, int32_t* n_out, int32_t* info, void* ws, size_t ws_bytes, hipStream_t st,
                       VoxelOrder* order);
// The normal-distributions transform (ndt.hip, ndt_gauss.hpp).  A table: the Gaussian voxels of a cloud ascending by
// key = c0 << 42 | c1 << 21 | c2, one 128-byte record each and the keys once more on their own (what a lookup searches); lo, the
// origin o = 0.5f lo + 0.5f hi and the step of the grid.  ndt_build reads back twice; launch_ndt_refit is one asynchronous step.
struct NdtRec { unsigned long long key; int32_t count; int32_t pad; double mean[3]; double C[6]; double fill[5]; };
struct NdtView { const unsigned long long* keys; const NdtRec* rec; int G, n_vox, min_points; double step; float lo[3], o[3]; void* block; };
int ndt_build(const float* pts, int n, int ld, double step, int min_points, hipStream_t st, NdtView* view);
int ndt_max_queries();
bool ndt_d2(double step, double outlier_ratio, double* d2);      // false: outlier_ratio outside [0, 1)
size_t ndt_refit_ws_bytes(int Q, int B);
int launch_ndt_refit(const NdtView& v, const float* q, int Q, int ldq, const double* T_dev, int B, int neighbors, double outlier_ratio, double* T_out,
                     double* T_step, int32_t* n_pairs, double* sum_e, int32_t* empty, void* ws, size_t ws_bytes, hipStream_t st);
// the match stage on a finished search (knn_points.hip): threshold + ratio + Unique (query grid of the search's workspace)
// + ordered compaction in ONE launch; the two halves around the multi-GPU table exchange
int launch_match_finish(const ModelView& v, const float* q, int Q, int ldq, const int32_t* idx, const float* dist, float thr,
                        float ratio, int unique, void* ws, size_t ws_bytes, uint32_t* pairs, double* pts1, double* pts2,
                        int32_t* n_pairs, hipStream_t st);
int launch_match_table(const ModelView& v, int32_t m_lo, int M_total, const float* q, int Q, int ldq, const int32_t* idx,
                       const float* dist, float thr, float ratio, int unique, void* ws, size_t ws_bytes, int32_t* table,
                       hipStream_t st);
int launch_match_from_table(const float* q, int Q, int ldq, int M_total, const int32_t* idx, const float* dist, float thr,
                            float ratio, const int32_t* table, void* ws, size_t ws_bytes, uint32_t* pairs, double* pts1,
                            double* pts2, int32_t* n_pairs, hipStream_t st);

size_t knn2_points_workspace_bytes(int Q, int M);
int launch_knn2_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm,
                           int32_t idx_base, int32_t* idx, float* dist, void* ws, size_t ws_bytes,
                           hipStream_t st, bool timed = true);
int launch_merge_top2_f32(const int32_t* idx_in, const float* dist_in, int R, int Q, int32_t* idx,
                          float* dist, hipStream_t st, size_t rank_stride = 0);
// generic-D descriptor matching (fp64)
size_t match_features_workspace_bytes(int Q, int M, int D);
int launch_preprocess(const double* dS, int Q, int ldS, const double* dM, int M, int ldM, int D,
                      const pcreg_match_opts& o, double* outS, double* outM, void* ws, size_t ws_bytes,
                      hipStream_t st);
int launch_normalize_rows(double* f, int n, int ld, int D, hipStream_t st);
int launch_normalize_rows2(double* f, int n, int ld, double* f2, int n2, int ld2, int D, hipStream_t st);
int launch_match_features(const double* fS, int Q, int ldS, const double* fM, int M, int ldM, int D,
                          const pcreg_match_opts& o, uint32_t* pairs, double* metric, int32_t* P_dev,
                          void* ws, size_t ws_bytes, hipStream_t st);

// fast global registration of B sets of matched pairs (fgr.hip, fgr_pair.hpp): pcreg_dev_fgr_batched's arguments.
// fgr_args_ok is the argument rule every tier checks before it touches the device
bool fgr_args_ok(const pcreg_fgr_opts& o);
int fgr_resident_capacity();
size_t fgr_ws_bytes(int n_cap, int B, int iterations);
int launch_fgr(const double* p1, const double* p2, int ld, const int32_t* offsets, int B, int n_cap, const pcreg_fgr_opts& o, const double* T0,
               const int32_t* tuple_idx, pcreg_fgr_result* out, int32_t* inlier_idx, uint8_t* kept, void* ws, size_t ws_bytes, hipStream_t st);

// sphere-sweep driver pieces (sweep.hip) and the final refine (ransac.hip)
int launch_sphere_counts(const double* feat, int V, const double* centres, int S, double R, int32_t* counts, hipStream_t st);
size_t sphere_select_workspace_bytes(int V);
int launch_sphere_select(const double* feat, int V, const double c[3], double R, int32_t* idx, int32_t* n_out, void* ws, size_t ws_bytes,
                         hipStream_t st);
int launch_gather_rows_f64(const double* src, int D, const int32_t* idx, const int32_t* n, int cap, double* dst, hipStream_t st);
int launch_quick_tf(const double* pts, int n, int ld, const double T[16], double* out, int ldo, hipStream_t st);
int launch_refine_by_distance(const double* p1, const double* p2, const int32_t* n_dev, int cap, int ld, double maxDist,
                              double* T16_dev, int32_t* info_dev, hipStream_t st);
int launch_estimate_transform_indexed(const double* p1, const double* p2, int ld, const int32_t* idx, int32_t idx_base, const int32_t* n_idx_dev,
                                      int cap, double* T16_dev, int32_t* info_dev, hipStream_t st);
// the final stage batched over its K clusters (sweep.hip, ransac.hip)
int launch_quick_tf_batched(const double* pts, int n, int ld, const double* T_dev, int K, double* out, int ldo, double* limits, hipStream_t st);
int launch_final_close_refine_batched(const uint32_t* pairs, const int32_t* n_pairs, const double* feat, const int32_t* kp_off,
                                      const double* featCur_all, const int32_t* seg_off, int K, double maxDist, int32_t* n_close,
                                      double* precision, double* T16, int32_t* empty, hipStream_t st);
int launch_final_pick_apply(const double* precision, const double* T16, const int32_t* empty, int K, const double* pts_all, int n, int ld,
                            double* out, int ldo, int32_t* best, hipStream_t st);

void knn_f16_timing_enable(bool on);
int knn_f16_timing_read(float* mean_ms, int* launches);
int launch_transpose_rows(const double* f, int n, int ld, int D, double* out, hipStream_t st);
int launch_widen_rows_u16(const uint16_t* rows, const int32_t* index, int n, int D, double* featmajor, hipStream_t st);   // rows[index[i]] (u16) -> feature-major f64
size_t local_points_workspace_bytes(int N);
int launch_local_points(const double* pts, int N, int ld, double R, const double c[3], int mode, double* out, int ldo, double* dists,
                        int32_t* totals, void* ws, size_t ws_bytes, hipStream_t st);
int launch_sphere_select_batched(const double* feat, int V, const double* centres, int S, double R, const int32_t* seg_off, int32_t* idx,
                                 double* feat_out, int32_t* n_out, hipStream_t st);
size_t get_matches_segmented_workspace_bytes(int Q, int VM, int D, int S, int tot, int n_max);
// The model side of the segmented matcher that does not depend on the surface or the segments: the powered rows and the six
// scalars per row (segp_rows_kernel).  A caller that matches MANY surfaces against one immutable model set (the host tier's
// descriptor sets) prepares them once: P [VM][D], r [6][VM]; valid for the (change_metric, metric_factor) they were made with.
struct SegPreparedModel { const double* P; const double* r; int VM, D, change_metric; double metric_factor; };
size_t segmented_prepared_model_bytes(int VM, int D);          // doubles of P and r together, in bytes
int launch_segmented_prepare_model(const double* descM_rows, int VM, int D, const pcreg_match_opts& o, double* P, double* r, hipStream_t st);
int launch_get_matches_segmented(const double* descS, int Q, const double* descM, int VM, int D, const int32_t* seg_rows,
                                 const int32_t* seg_off, int S, int tot, int n_max, const pcreg_match_opts& o, uint32_t* pairs_all,
                                 double* metric_all, int32_t* n_pairs, void* ws, size_t ws_bytes, hipStream_t st,
                                 const SegPreparedModel* prepared = nullptr);
int launch_sweep_plan(const int32_t* n_pairs, int S, int thresh, int32_t* trial_idx, int32_t* offsets, int32_t* n_trials, hipStream_t st);
int launch_sweep_gather(const uint32_t* pairs_all, int VS, const int32_t* n_pairs, const int32_t* trial_idx, const int32_t* offsets,
                        const int32_t* n_trials, int S, const double* featS, const double* featCur_all, const int64_t* row_off,
                        double* p1, double* p2, int ld, hipStream_t st);
int launch_gather_matched_rows(const uint32_t* pairs, const int32_t* n_pairs, int cap, const double* featS, const double* featM,
                               double* pts1, double* pts2, hipStream_t st);

int launch_align_points_knn(const double* pts, int ld, const int32_t* offsets_dev, int B, int max_n,
                            int C1, int C2, double* aligned, int ld_out, double* coeff, double* c,
                            int32_t* status, hipStream_t st);


// spatial-histogram descriptors (cfg 4)
size_t descriptors_workspace_bytes(int P, int S);
int launch_descriptors(const double* pts, int P, int ld, const double* kp, int S, int ldk, const pcreg_desc_opts& o, int single_mode,
                       double* feat, double* desc_f64, uint16_t* rows_u16, int32_t* row_index, int32_t* V_dev, int32_t* err_dev,
                       void* ws, size_t ws_bytes, hipStream_t st);

}  // namespace pcreg
