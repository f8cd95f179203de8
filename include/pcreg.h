/* include/pcreg.h -- C ABI of libpcreg_hip.so: the MI355X (gfx950) implementation of
 * the PCReg correspondence-search + RANSAC rigid-alignment hot path.
 *
 * The reference (LCJebe/PCReg) is pure MATLAB and has no FFI layer; the boundary it
 * exposes for this path is the set of MATLAB function signatures below.  Each entry
 * point names the reference function it replaces (file:line in the reference tree);
 * INTEGRATION.md shows the MEX binding a maintainer adds on the MATLAB side.
 *
 * Conventions (MATLAB's, so a MEX shim passes mxGetPr() pointers straight through):
 *   - matrices are column-major with an explicit leading dimension `ld` (>= rows);
 *     a point set is n x 3: x = p[i], y = p[i+ld], z = p[i+2*ld];
 *   - T is a column-major 4x4 used as [p 1]*T (quickTF.m:5-7): rotation in
 *     T(1:3,1:3), translation in T(4,1:3);
 *   - indices that cross the boundary are 1-based, pairs are uint32 like matchFeatures';
 *   - every function returns 0 on success or a PCREG_E_* code; pcreg_last_error()
 *     gives the text.  "RANSAC found nothing" is NOT an error: it is reported through
 *     *failed = 1 with T zeroed, mirroring ransac.m:77-89 (empty T, zeros).
 *   - there is no CPU fallback: without a usable HIP device every compute entry
 *     point returns PCREG_E_NODEVICE.
 *
 * Two tiers:
 *   pcreg_*      host tier  -- pointers are HOST memory (what MEX hands over); the call
 *                              stages to HBM, runs the kernels, copies results back.
 *   pcreg_dev_*  device tier -- pointers are DEVICE memory and work is enqueued on the
 *                              caller's HIP stream (passed as void*); nothing
 *                              synchronises.  Used by resident pipelines, the
 *                              multi-GPU host code and bench.py.
 */
#ifndef PCREG_H
#define PCREG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCREG_OK            0
#define PCREG_E_ARG         1   /* bad argument (null pointer, negative size, ld < n ...) */
#define PCREG_E_HIP         2   /* a HIP runtime call failed                              */
#define PCREG_E_NODEVICE    3   /* no usable gfx950 device                                */
#define PCREG_E_WORKSPACE   4   /* caller's workspace too small (device tier)             */

/* largest k of the k-nearest point searches (pcreg_knn_points_f32, pcreg_model_knn_f32, pcreg_dev_model_knn_f32) */
#define PCREG_KNN_MAX_K 32

#define PCREG_METRIC_SAD 0
#define PCREG_METRIC_SSD 1

/* ransacCoef of ransac.m:7-12,23-34 (+ the build's sampler seed). */
typedef struct pcreg_ransac_opts {
    int32_t  minPtNum;     /* ransac.m:23; estimateTransform needs >= 3              */
    int32_t  iterNum;      /* ransac.m:24                                            */
    double   thDist;       /* ransac.m:26; compared with the SQUARED distance         */
    double   thInlrRatio;  /* ransac.m:25; thInlr = round(thInlrRatio*ptNum), :28     */
    int32_t  REFINE;       /* ransac.m:29                                            */
    int32_t  VERBOSE;      /* ransac.m:30-34; printing is done by the host wrappers   */
    uint64_t seed;         /* used only when sample_idx == NULL (built-in sampler)    */
} pcreg_ransac_opts;

/* `par` of getMatches.m:5-9,22,35,51-56 + matchFeatures' Prenormalized. */
typedef struct pcreg_match_opts {
    int32_t metric;          /* PCREG_METRIC_SAD | PCREG_METRIC_SSD   (par.Metric)     */
    double  matchThreshold;  /* percent, par.MatchThreshold                            */
    double  maxRatio;        /* par.MaxRatio                                           */
    int32_t unique;          /* par.Unique                                             */
    int32_t prenormalized;   /* matchFeatures 'Prenormalized' (getMatches passes 0)    */
    int32_t unnormalize;     /* par.UNNORMALIZE, getMatches.m:22-26                    */
    double  norm_factor;     /* par.norm_factor                                        */
    int32_t change_metric;   /* par.CHANGE_METRIC, getMatches.m:35-37                  */
    double  metric_factor;   /* par.metric_factor                                      */
} pcreg_match_opts;

/* ---- library ------------------------------------------------------------------- */
const char* pcreg_last_error(void);
const char* pcreg_version(void);
int  pcreg_device_count(int* count);
int  pcreg_set_device(int ordinal);          /* one process per GPU: call once per rank */
int  pcreg_device_name(char* buf, int cap);  /* e.g. "gfx950:..."                       */
/* Test hook, not part of the reference's interface: selects the OTHER side of a certified fast path (process-wide), so that
 * the parity tests can run both sides inside one process.  Every setting returns the same indices and counts.  Keys:
 * "knn_exact", "match_exact", "match_force_fallback" (1, 2), "ransac_fused", "ransac_nolane", "ransac_f64score",
 * "ransac_resident_f64", "align_times", "align_shape", "seg_debug", "seg_batched", "seg_wave_finalize", "match_stats", "final_batch_mb" (the
 * descriptor memory bound of pcreg_final_stage in MB instead of 4 GB, to exercise its batches), "knn_nocull" (the point search
 * visits every model tile), "knn_stats" (counters for pcreg_debug_knn_stats), "ransac_pass2" (the staged RANSAC
 * chain's second scoring pass: 1 always the full pass, 2 always the bounded pass where allowed; 0 chooses by shape),
 * "ransac_stats" (counters for pcreg_debug_ransac_stats), "range_sort_cap" (n > 0: the radius search orders segments longer
 * than n rows by its in-place large-segment path), "cluster_noskip" (the clustering walk unites on every hit instead of
 * skipping a hit whose row already shows the lane's root), "cluster_stats" (counters for pcreg_debug_cluster_stats),
 * "knn_tail_cap" (n > 0: the point search's exact tail lists the surviving tiles of n tiles per pass), "score_batch_slots"
 * (n > 0: pcreg_dev_model_score_f32 and pcreg_dev_model_refit_f32 batch whole transforms under n query slots instead of 4 Mi, one transform at least), "fpfh_radius_lanes" (4 or 16: the radius FPFH counts a
 * row's pairs with that many lanes instead of 64), "desc_stats" (counters for pcreg_debug_desc_stats), "knn_direct"
 * (1: the two-nearest search sends every query through the tile walk instead of answering the seeded queries with a small
 * cell range from their ordering-grid cells; while "knn_stats" is on every query takes the walk as well, because those counters
 * are defined over the walk of the whole query set), "knn_direct_stats" (counters for pcreg_debug_knn_direct_stats; it forces
 * nothing), "knn_seed_fused" (1: the two-nearest search seeds and answers directly in two launches instead of one; same
 * bits), "ransac_bhand" (1: the staged RANSAC chain's bounded second pass walks every refit to its stop instead of handing
 * the refits still undecided after a few blocks to its block-parallel finish; same bits), "fgr_chain" (1: fast global
 * registration runs its chained form, a sums and a finish launch per iteration, whatever the size; same bits); value 0
 * restores the default.  The library reads NO
 * environment variable (tests/test_abi.py greps the binary).  PCREG_E_ARG for an unknown key. */
int  pcreg_debug_set(const char* key, int value);
/* With pcreg_debug_set("match_stats", 1): the counters of the certified SAD matcher summed over the calls since the last
 * reset -- out[0] queries finalised, [1] candidates re-scored exactly (fp64), [2] queries the certificate left unproven,
 * [3] queries handed to the exhaustive exact-rows kernel, [4] Unique back-check items (segmented form), [5] back-check items
 * handed to the exhaustive kernel, [6] matcher calls, [7] segments.  Synchronises the device.  bench.py reports them so that
 * a throughput figure says how much of it the certificates carried. */
int  pcreg_debug_match_stats(long long out[8], int reset);
/* With pcreg_debug_set("knn_stats", 1): the counters of the point search against a prepared model summed over the searches
 * since the last reset -- out[0] searches, [1] (query block, model tile) pairs the candidate kernel visited, [2] nominal
 * pairs (query blocks of 512 x tiles of 512 rows), [3] queries the certificate sent to the exhaustive tail.  Off: no extra
 * work; on: one small launch per search, no host sync.  The read synchronises the device. */
int  pcreg_debug_knn_stats(long long out[4], int reset);
/* With pcreg_debug_set("knn_stats", 1): inside the visited tiles the candidate kernel scores 64-row units per wave of 128
 * queries -- out[0] the (wave, unit) pairs scored, summed over the searches since the last reset, [1] 32 x the
 * visited (query block, tile) pairs, which is what it scores without the unit rule.  Resets these two only; the read
 * synchronises the device. */
int  pcreg_debug_knn_unit_stats(long long out[2], int reset);
/* With pcreg_debug_set("knn_direct_stats", 1): the direct answers of the two-nearest search summed over the
 * searches since the last reset -- out[0] searches, [1] queries that were eligible and answered from their ordering-grid
 * cells, [2] the rows ranked for them.  The key does not change which path a query takes.  Off: no extra work; on: one small
 * launch per search, no host sync.  The read synchronises the device. */
int  pcreg_debug_knn_direct_stats(long long out[3], int reset);
/* With pcreg_debug_set("knn_stats", 1): the farthest point sampling summed over the calls since the last reset --
 * out[0] steps run (the sum of n_out), [1] live rows measured against a sample; without culling that is nf x n_out.  Off: no
 * extra work.  The read synchronises the device. */
int  pcreg_debug_fps_stats(long long out[2], int reset);
/* With pcreg_debug_set("ransac_stats", 1): the counters of the staged RANSAC chain's bounded second pass summed over the calls
 * since the last reset -- out[0] bounded passes run, [1] (refit, 512-correspondence block) units scanned (seed refits
 * included), [2] the units a full pass scans.  Off: no extra work.  The read synchronises the device. */
int  pcreg_debug_ransac_stats(long long out[3], int reset);
/* With pcreg_debug_set("ransac_stats", 1): the handover of the bounded second pass summed over the calls since the
 * last reset -- out[0] refits handed over to the finish, [1] (refit, 512-correspondence block) units the finish scored (they
 * are part of pcreg_debug_ransac_stats' out[1] as well).  out[2] is no counter: the number of blocks a refit is walked before
 * it is handed over, whether or not the key is on.  Resets its two counters only; the read synchronises the device. */
int  pcreg_debug_ransac_handover(long long out[3], int reset);
/* With pcreg_debug_set("cluster_stats", 1): the counters of the clustering walk summed over the calls since the last reset --
 * out[0] calls, [1] hits (scored row pairs within the radius), [2] compare-and-swap attempts on the union-find, [3] attempts
 * that failed (another lane had merged first).  Off: no extra work.  The read synchronises the device.  (The walk's visited and
 * nominal (tile, tile) pairs are counted by "knn_stats".) */
int  pcreg_debug_cluster_stats(long long out[4], int reset);
/* With pcreg_debug_set("desc_stats", 1): which of its rarely taken branches the descriptor kernel took, summed over the
 * keypoints of the calls since the last reset -- out[0] keypoints that passed the size gates and reached the K-nearest
 * selection, [1] selections that fell back to the bisection (more than 256 keys in the K-th key's bin), [2] selections that
 * counted the tie group with a pass over every key (the group straddles a bin border, or the bin is crowded), [3] selections
 * that ranked a tie group by original index (part of it is kept), [4] keypoints whose sign votes were all retaken in fp64
 * (more than 128 votes fp32 could not certify), [5] keypoints whose whole support was binned again in fp64 (more than 128
 * deferred points), [6] points that took the literal sqrt / acos / atan2 path, [7] (wave, 64-candidate chunk) pairs re-tested
 * past the kept ballots, [8] the grid subdivision of the LAST call, fx << 16 | fy << 8 | fz (stored, not added), [9] deferred
 * points binned one by one in fp64 (supports with at most 128 of them: the others count in [5]).  While the key is on the
 * descriptor calls run a second instantiation of the kernel that holds the counting code (same source, same results); off,
 * they run the default one, which holds none.  The read synchronises the device.  The tests use the counters to prove that a
 * scene reached the branch it was built for, and run every such scene on both instantiations. */
int  pcreg_debug_desc_stats(long long out[10], int reset);

/* ---- host tier ------------------------------------------------------------------ */

/* estimateTransform.m:2  T = estimateTransform(pts1, pts2), [pts2,1]*T = [pts1,1].
 * *empty = 1 reproduces the `T = []` return of estimateTransform.m:11-14. */
int pcreg_estimate_transform(const double* pts1, const double* pts2, int n, int ld,
                             double T[16], int* empty);

/* getInliersRANSAC.m:46  d = calcDists(T, pts1, pts2): squared distances, length n. */
int pcreg_calc_dists(const double T[16], const double* pts1, const double* pts2, int n, int ld,
                     double* d);

/* ransac.m:1  [T, inlierIdx, numSuccess, maxInliers, ratio] = ransac(pts1, pts2,
 * ransacCoef, @estimateTransform, @calcDists).
 * sample_idx: [iterNum][minPtNum] 1-based indices, hypothesis-major (pass the
 * transpose of a MATLAB iterNum x minPtNum table, i.e. minPtNum x iterNum
 * column-major), replacing `randperm(ptNum)(1:minPtNum)` of ransac.m:42-43; NULL
 * selects the built-in counter-based sampler seeded by opts->seed.
 * inlier_idx has capacity n (1-based, ascending); iter_inl / iter_inl_ref (optional,
 * may be NULL, length iterNum) receive inlrNum / inlrNum_refined of ransac.m:36-37. */
int pcreg_ransac(const double* pts1, const double* pts2, int n, int ld,
                 const pcreg_ransac_opts* opts, const int32_t* sample_idx,
                 double T[16], int32_t* inlier_idx, int* n_inliers, int* num_success,
                 int* max_inliers, int* failed, int32_t* iter_inl, int32_t* iter_inl_ref);

/* The same for B independent registrations in one launch (the parfor of
 * completeExperimentFast.m:201-225).  Registration b owns rows
 * [offsets[b], offsets[b+1]) of the concatenated pts1/pts2 (total = offsets[B]) and
 * the sample table rows [b*iterNum, (b+1)*iterNum) (or seed + b).  Outputs are
 * arrays of length B (T: 16*B); inlier_idx is concatenated with the same offsets. */
int pcreg_ransac_batched(const double* pts1, const double* pts2, int total, int ld,
                         const int32_t* offsets, int B, const pcreg_ransac_opts* opts,
                         const int32_t* sample_idx, double* T, int32_t* inlier_idx,
                         int32_t* n_inliers, int32_t* num_success, int32_t* max_inliers,
                         int32_t* failed);

/* Fast global registration (Zhou, Park, Koltun 2016; MATLAB's pcregisterfgr) of B sets of matched pairs, laid out as
 * pcreg_ransac_batched has them: pts1 / pts2 n x 3 column-major doubles with leading dimension ld, registration b owns rows
 * [offsets[b], offsets[b+1]); T is MATLAB's 4 x 4, column-major, [pts2, 1] * T = [pts1, 1].  No samples and no hypotheses: a
 * Geman-McClure weight per pair is annealed from "every pair counts" to "only pairs within sqrt(delta2) count" and a six-unknown
 * rigid step is solved at every stage, so the result depends on nothing but the inputs.
 *
 * THE CONTRACT, per registration b, in double throughout and uncontracted (csrc/fgr_pair.hpp holds every per-pair formula):
 *  1. A pair is LIVE when its six coordinates are finite.  Dead pairs are never kept and take no part in anything.
 *  2. The tuple test (n_tuples > 0).  Triple p = the three pair indices that pcreg_ransac's built-in sampler gives hypothesis p
 *     with seed `seed + b`, or row p of the caller's tuple_idx [B][n_tuples][3] (1-based, each index clamped to [1, n] as pcreg_ransac
 *     clamps its table).  It passes when its three pairs are live and each edge (i, j) has s2 * a < b && s2 * b < a with a =
 *     |pts1_i - pts1_j|^2, b = |pts2_i - pts2_j|^2 (each (dx dx + dy dy) + dz dz) and s2 = tuple_scale^2.  A pair is KEPT when it
 *     belongs to at least one passing triple: no multiplicity, no stop at a number of passes.  n_tuples == 0 keeps every live pair.
 *  3. Fewer than 3 kept pairs: failed = 1, T sixteen zeros, mu0 = mu_final = cost = sum_d2 = 0 and n_inliers = 0 -- what a failed
 *     pcreg_ransac leaves; n_live and n_kept still say why.  So does a registration of more than n_cap rows (device tier), with
 *     n_live = n_kept = 0.
 *  4. o = the middle of the box of the kept pts1 rows, 0.5 lo + 0.5 hi per axis.
 *  5. opts->mu0 == 0 means mu0 = the larger squared diagonal of the boxes of the kept pts1 and of the kept pts2 rows.
 *  6. T = T0[b] (NULL: the identity), mu = mu0.  For it = 0 .. iterations - 1: when it > 0 && it % decrease_every == 0, mu =
 *     max(mu / division_factor, delta2); every kept pair k (ascending row order) has q = [pts2_k 1] * T, each component
 *     ((x T[4j] + y T[4j+1]) + z T[4j+2]) + T[4j+3], r = q - pts1_k, rr = (r0 r0 + r1 r1) + r2 r2, t = mu / (mu + rr), w = t t,
 *     u = q - o, and adds w times the 28 terms of the three plane pairs (normal e_c, residual r_c) to plane_fit.hpp's sums;
 *     plane_fit(sums, 3 n_kept, o) gives T_step and T <- T * T_step.  A fit that answers "empty" ends the registration as in 3.
 *  7. Results: T, failed, n (rows), n_live, n_kept, mu0, mu_final, cost = the sum of w rr under the final T and mu_final,
 *     n_inliers = the kept pairs with rr <= delta2 under the final T and sum_d2 the sum of their rr; inlier_idx (capacity total,
 *     the rows' layout: registration b's list starts at offsets[b]) 1-based within the registration, ascending; kept (optional,
 *     total bytes, the rows' layout) 1 for a kept pair.
 * THE SUM ORDER.  Kept pair k belongs to chunk k / 2048; thread t of the chunk's 256 adds pairs 2048 c + t, + 256, ... in that
 * order from 0.0; the 64 lanes of a wave are added by the xor butterfly at distances 32, 16, 8, 4, 2, 1; the four waves as
 * ((w0 + w1) + w2) + w3; the chunks ascending from 0.0.  cost and sum_d2 are summed the same way.  Nothing depends on B, on a
 * registration's place in the batch, on the stream, on what the workspace held or on which of the two kernel forms ran
 * (pcreg_debug_set("fgr_chain", 1) forces the chained form, which otherwise serves n_cap above pcreg_fgr_resident_capacity()).
 *
 * Argument rules (PCREG_E_ARG): delta2 >= 0, iterations >= 1, decrease_every >= 1, division_factor > 1, mu0 >= 0, n_tuples >= 0,
 * 0 < tuple_scale <= 1, all finite; offsets ascending from 0 to total <= ld (host tier). */
typedef struct pcreg_fgr_opts {
    double   delta2;           /* the squared distance at which a pair stops counting; compared with SQUARED distances */
    int32_t  iterations;
    int32_t  decrease_every;
    double   division_factor;
    double   mu0;              /* 0: the default of rule 5 */
    int32_t  n_tuples;         /* 0: no tuple test */
    int32_t  reserved;         /* 0 */
    double   tuple_scale;
    uint64_t seed;             /* of the built-in triples (tuple_idx == NULL) */
} pcreg_fgr_opts;
typedef struct pcreg_fgr_result {
    double  T[16];
    double  mu0, mu_final, cost, sum_d2;
    int32_t failed, n, n_live, n_kept, n_inliers, reserved;
} pcreg_fgr_result;
/* the largest n_cap the resident form serves (its kept pairs are staged in LDS, six doubles a pair) */
int pcreg_fgr_resident_capacity(void);
/* Host tier: one upload and one read.  T0 [B][16] or NULL, tuple_idx [B][n_tuples][3] or NULL, kept [total] or NULL. */
int pcreg_fgr_batched(const double* pts1, const double* pts2, int total, int ld, const int32_t* offsets, int B,
                      const pcreg_fgr_opts* opts, const double* T0, const int32_t* tuple_idx, pcreg_fgr_result* out,
                      int32_t* inlier_idx, uint8_t* kept);

/* fp32 3-D point search (the "KNN" of BASELINE.json's metric): for each query the two
 * nearest model points, squared distance fmaf(dz,dz,fmaf(dy,dy,dx*dx)), ties to the
 * lowest index.  idx [Q][2] 0-based (-1 when M < 2), dist [Q][2]. */
int pcreg_knn2_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm,
                          int32_t* idx, float* dist);

/* matchFeatures' filter chain on raw fp32 points (Prenormalized, SSD, absolute
 * threshold thr_abs on the squared distance, ratio test, optional Unique back-check).
 * pairs: capacity Q x 2, ROW-major [k][0]=query, [k][1]=model, 1-based, ascending
 * query.  *P receives the number of pairs. */
int pcreg_match_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm,
                           float thr_abs, float max_ratio, int unique,
                           uint32_t* pairs, int* P);

/* The same against a model that is uploaded and prepared ONCE (host tier of the handle below): MATLAB keeps the
 * handle as a uint64 and matches any number of surfaces against it (completeExperimentFast.m:131-149). */
typedef struct pcreg_model pcreg_model;
int pcreg_model_create(const float* m, int M, int ldm, pcreg_model** model);
int pcreg_model_destroy(pcreg_model* model);
int pcreg_model_size(const pcreg_model* model, int* M);         /* the number of rows the handle was created with */
int pcreg_model_match_points_f32(pcreg_model* model, const float* q, int Q, int ldq, float thr_abs, float max_ratio,
                                 int unique, uint32_t* pairs, int* P);
/* MATLAB's [Idx, D] = knnsearch(model, q, 'K', k) / findNearestNeighbors(ptCloud, p, K) against the handle: for each query the
 * k (1 <= k <= PCREG_KNN_MAX_K) model rows with the smallest fp32 squared distance fmaf(dz,dz,fmaf(dy,dy,dx*dx)), ordered by
 * (distance, row), ties to the lowest row.  idx [Q][k] 0-based (-1 past M), dist [Q][k] squared (+inf past M), both
 * row-major.  Exact: the same bits as a brute force; for k = 1, 2 the columns of the top-2 search. */
int pcreg_model_knn_f32(pcreg_model* model, const float* q, int Q, int ldq, int k, int32_t* idx, float* dist);
/* The same without a handle (knnsearch(m, q, 'K', k)): uploads and prepares the model for this call only. */
int pcreg_knn_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm, int k, int32_t* idx, float* dist);
/* MATLAB's [Idx, D] = rangesearch(model, q, r) / findNeighborsInRadius against the handle, with the SQUARED radius r2 = r^2:
 * model row j belongs to query i iff its fp32 squared distance fmaf(dz,dz,fmaf(dy,dy,dx*dx)) <= r2 (inclusive; a NaN distance
 * never passes, so a non-finite query has an empty segment at a finite r2; with r2 = +inf an overflowed distance passes too).
 * Query i's rows are seg_off[i] .. seg_off[i + 1] of idx (0-based) / dist (squared), ordered by (distance, row), ties to the
 * lowest row.  Exact: the same bits as a brute force.  seg_off [Q + 1] is always written (seg_off[Q] = total).  idx / dist
 * (capacity elements; may be NULL when capacity == 0) are written iff total <= capacity: call once with capacity 0 to size
 * them.  PCREG_OK in both cases.  r2 NaN or negative, Q above 4 Mi, a negative capacity: PCREG_E_ARG. */
int pcreg_model_range_f32(pcreg_model* model, const float* q, int Q, int ldq, float r2, int64_t capacity,
                          int64_t* seg_off, int32_t* idx, float* dist);
/* The same without a handle (rangesearch(m, q, r)): uploads and prepares the model for this call only. */
int pcreg_range_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm, float r2, int64_t capacity,
                           int64_t* seg_off, int32_t* idx, float* dist);
/* How well do B candidate transforms put a cloud on the model?  THE CONTRACT of every tier (device, host, MEX, Python):
 * inputs -- a prepared model; Q query points q in fp32, column-major with leading dimension ldq; B transforms T of 16 doubles
 * each, column-major 4 x 4, used as quickTF.m uses them ([q, 1] * T); a squared radius r2 >= 0 (+inf allowed).
 * Per pair (b, i): the TRANSFORMED QUERY is q[i] widened to double, ((x*T[4j] + y*T[4j+1]) + z*T[4j+2]) + T[4j+3] for j = 0, 1, 2
 * (left to right, no contraction: quick_tf's arithmetic), each coordinate rounded once to fp32.  With the point search's
 * distance d = fmaf(dz,dz,fmaf(dy,dy,dx*dx)) it has THE NEAREST ROW WITHIN THE RADIUS: the model row with the smallest d among
 * the rows with d <= r2 (inclusive), ties to the lowest original row; a NaN d never passes, an overflowed d passes r2 = +inf
 * only.  idx[b * Q + i] is that row (0-based) or -1 when there is none, dist[b * Q + i] its d or +inf: the same bits as a
 * brute force.  A transform whose 16 numbers are all zero is the EMPTY transform a failed ransac leaves (ransac.hip: ransac_emit_result
 * and the last slice of ransac_select_multi_kernel store 0.0 into all 16 entries of T when `failed` is set): it scores nothing, every idx -1 and every dist +inf.
 * Per transform b: n_close[b] the number of i with a row, sum_d2[b] the sum of their d in double -- a function of the inputs
 * only (a fixed order: chunks of 2048 queries in query order through a fixed tree, then the chunks ascending; no
 * floating-point atomic), the same bits on every call.  Fitness is n_close / Q and the inlier RMSE sqrt(sum_d2 / n_close):
 * the callers' arithmetic.  idx and dist may be NULL (each on its own); then only 12 B bytes come back.
 * Q = 0: n_close and sum_d2 are 0 for every b.  B = 0: nothing is written.  A model without rows: every query misses.
 * PCREG_E_ARG: r2 NaN or negative, Q above 4 Mi, a negative B or Q, ldq < Q. */
int pcreg_model_score_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T /* host [B][16] */, int B, float r2,
                          int32_t* n_close, double* sum_d2, int32_t* idx, float* dist);
/* Refit B candidate transforms on their close dense pairs: completeExperimentFast.m:383-394's T_refine on the whole cloud, for every
 * candidate at once.  THE CONTRACT of every tier (device, host, MEX, Python):
 * inputs -- those of pcreg_model_score_f32 (a prepared model, Q fp32 points column-major with ldq, B transforms of 16 doubles used
 * as quickTF.m uses them, a squared radius r2 >= 0, +inf allowed).
 * THE PAIRS of transform b are exactly scoring's: for every query i whose TRANSFORMED QUERY p' (that contract: double arithmetic
 * without contraction, rounded once to fp32) has a NEAREST ROW WITHIN THE RADIUS (d <= r2 inclusive, ties to the lowest original
 * row, a NaN d never passes), the pair (that model row, p'), taken in ascending i, both sides widened to double.
 * Per transform b:  n_close[b] and sum_d2[b] are THE SAME BITS pcreg_model_score_f32 returns for the same inputs.
 * T_step[b] = estimateTransform(pts1 = the model rows, pts2 = the moved points), this library's estimateTransform
 * ([pts2, 1] * T = [pts1, 1]; the rank test of estimateTransform.m:11-14; exactly three pairs by the synthetic fourth point of
 * :18-37; more by the moments of the pairs; no reflection fix), so that quickTF(quickTF(q, T[b]), T_step[b]) lies on the model --
 * the map the reference obtains as invertTF(T_refine) at :391-394 (the arguments in this order save the inversion).
 * T_out[b] = T[b] * T_step[b] in double, entry (r, c) -- at [r + 4 c] of the 16 -- being
 * ((T(r,0) S(0,c) + T(r,1) S(1,c)) + T(r,2) S(2,c)) + T(r,3) S(3,c), left to right, no contraction.
 * empty[b] = 1 and all 16 entries of T_step[b] and of T_out[b] are 0.0 when estimateTransform is empty (the rank test fails, or
 * the rotation is undefined), when there are fewer than three pairs, or when T[b] is itself the empty (all-zero) transform: the
 * form in which a failed ransac and pcreg_refine_by_distance report a failed fit, so a failed candidate stays failed when the
 * step is repeated.  Otherwise empty[b] = 0.
 * Everything is a function of the inputs only: the moment sums take a fixed order (per chunk of 2048 queries in query order
 * through a fixed tree, then the chunks ascending, as sum_d2 does), shifted by one origin per model (the middle of the model's
 * bounding box as the handle holds it in fp32, for both sides); no floating-point atomic; batching, culling and the order in
 * which the walk meets the queries change nothing.
 * Q = 0 or a model without rows: every transform is empty, the counts 0.  B = 0: nothing is written.
 * THIS entry runs `steps` >= 1 such steps on the device, each step's T_out the next one's T, with one upload and one read:
 * T_out is the last step's, and so are n_close, sum_d2 and empty -- the counts therefore describe the transform that went INTO
 * the last step (T itself when steps = 1), not T_out.  PCREG_E_ARG: pcreg_model_score_f32's cases, and steps < 1. */
int pcreg_model_refit_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T /* host [B][16] */, int B, float r2,
                          int steps, double* T_out /* [B][16] */, int32_t* n_close, double* sum_d2, int32_t* empty);
/* Refit B candidate transforms by ONE LINEARISED POINT-TO-PLANE STEP on their close dense pairs (`steps` of them in this entry):
 * what pcreg_model_refit_f32 does with estimateTransform, done with the planes through the model rows instead, so that a pair may
 * be the wrong partner ALONG the surface as long as it is nearly the right one ACROSS it.  A step, not an ICP policy: no
 * convergence test, no weighting, no robust kernel (pcreg_model_refit_plane_trimmed_f32 keeps each candidate's closest pairs).  THE CONTRACT of every tier (device, host, MEX, Python):
 * inputs -- those of pcreg_model_refit_f32 (a prepared model, Q fp32 points column-major with ldq, B transforms of 16 doubles used
 * as quickTF.m uses them, a squared radius r2 >= 0, +inf allowed), and NORMALS: M x 3 fp32 column-major with leading dimension
 * ldn >= M, indexed by ORIGINAL row -- exactly what pcreg_model_normals_f32 and pcreg_dev_model_normals_f32 write.  A normal is
 * used as it is: not renormalised, no variation threshold.  A row with any non-finite normal component offers no plane (so a
 * caller drops the rows it distrusts by setting them to NaN).  THE SIGN of a normal cannot matter: every sum below is even in n,
 * and negating n negates products and sums exactly, so the outputs are the same bits.
 * THE PAIRS of transform b are exactly scoring's (pcreg_model_score_f32, pcreg_model_refit_f32): query i has a pair when its
 * TRANSFORMED QUERY p' (double arithmetic without contraction, rounded once to fp32) has a NEAREST ROW WITHIN THE RADIUS (d <= r2
 * inclusive, ties to the lowest original row, a NaN d never passes).  n_close[b] and sum_d2[b] are THE SAME BITS
 * pcreg_model_score_f32 returns.  A PLANE PAIR is a pair whose row has three finite normal components; n_plane[b] their number.
 * PER PLANE PAIR, in double on the widened fp32 values, without contraction except where fma is written; o the origin
 * pcreg_model_refit_f32 uses (the middle of the model's bounding box as the handle holds it in fp32: 0.5f * lo + 0.5f * hi per coordinate), m the model row, p = p' the
 * moved point, n the normal:
 *   e = p - m (by component);  r = (n_x e_x + n_y e_y) + n_z e_z;  u = p - o;
 *   c = u x n:  c_x = u_y n_z - u_z n_y,  c_y = u_z n_x - u_x n_z,  c_z = u_x n_y - u_y n_x;   J = (c_x, c_y, c_z, n_x, n_y, n_z).
 * THE 28 SUMS, each acc = fma(a, b, acc) over the plane pairs in ascending query order:
 *   [0..20] A_ij = sum J_i J_j for i <= j, the upper triangle row-major (A_00 A_01 .. A_05 A_11 .. A_55);
 *   [21..26] g_i = sum J_i r;   [27] rr = sum r r.
 * Their order is sum_d2's and the refit's moments': a thread adds its 8 consecutive queries in query order; the wave's butterfly
 * (lane l + lane l ^ o for o = 32, 16, .., 1) follows; the four waves of a chunk of 2048 queries are added in ascending order,
 * ((w0 + w1) + w2) + w3; the chunks are added in ascending order starting from 0.  No floating-point atomic; batching, culling and
 * the order in which the walk meets the queries change nothing.
 * THE FIT minimises sum (r + w . c + t . n)^2 over the small rotation vector w and the translation t: A x = -g, x = (w, t).  In
 * double, without contraction, in this order:
 *   1. s_i = sqrt(A_ii), i = 0 .. 5.
 *   2. C_ij = A_ij / (s_i * s_j) for i != j (the product first, j < i: A_ji / (s_j * s_i)); C_ii = 1.
 *   3. Cholesky C = L L^T row by row: for i = 0 .. 5 { for j = 0 .. i-1 { v = C_ij; for k = 0 .. j-1: v = v - L_ik * L_jk;
 *      L_ij = v / L_jj }  p_i = 1; for k = 0 .. i-1: p_i = p_i - L_ik * L_ik;  L_ii = sqrt(p_i) }.
 *   4. L y = -g / s: for i = 0 .. 5 { v = (-g_i) / s_i; for k = 0 .. i-1: v = v - L_ik * y_k;  y_i = v / L_ii }.
 *   5. L^T z = y: for i = 5 .. 0 { v = y_i; for k = i+1 .. 5: v = v - L_ki * z_k;  z_i = v / L_ii }.
 *   6. x_i = z_i / s_i.
 * THE ROTATION is exact (a rigid motion whatever the size of w) and uses only + - * / sqrt: the Cayley / quaternion form
 *   h = w / 2;  S = sqrt(1 + ((h_x h_x + h_y h_y) + h_z h_z));  (a, b, c, d) = (1 / S, h_x / S, h_y / S, h_z / S);
 *   R00 = 1 - 2 (c c + d d)   R01 = 2 (b c - a d)       R02 = 2 (b d + a c)
 *   R10 = 2 (b c + a d)       R11 = 1 - 2 (b b + d d)   R12 = 2 (c d - a b)
 *   R20 = 2 (b d - a c)       R21 = 2 (c d + a b)       R22 = 1 - 2 (b b + c c).
 * THE STEP moves p to R (p - o) + o + t.  In the library's layout (new_j = x T[4j] + y T[4j+1] + z T[4j+2] + T[4j+3]):
 *   T_step[4j + i] = R(j, i);   T_step[4j + 3] = (o_j + t_j) - ((R(j,0) o_x + R(j,1) o_y) + R(j,2) o_z);
 *   T_step[12..14] = 0, T_step[15] = 1;   T_out = T * T_step by pcreg_model_refit_f32's product.
 * OUTPUTS per transform: T_out, (at the device tier) T_step, n_close, sum_d2, n_plane, sum_res2 = rr, empty.  The plane RMSE of
 * the transform that went in is sqrt(sum_res2 / n_plane): the caller's arithmetic.
 * EMPTY: empty[b] = 1 and all 32 numbers of T_step[b] and T_out[b] are 0.0 when T[b] is the all-zero transform; when n_plane < 6;
 * when some A_ii is not a finite number above 0; when some pivot p_i is not above 2^-26 (below that the solve has lost half of a
 * double's digits, and a direction the planes do not constrain must not be invented: for a flat model in-plane sliding has
 * A_ii = 0, for parallel planes a pivot vanishes); when x or T_step is not finite.  A failed candidate stays failed when the step
 * is repeated.  Otherwise empty[b] = 0.  The counts and sums are reported either way.
 * Q = 0 or a model without rows: every transform is empty, the counts and sums 0.  B = 0: nothing is written.
 * THIS entry runs `steps` >= 1 such steps on the device with one upload and one read, as pcreg_model_refit_f32 does: T_out is the
 * last step's, and the counts, sum_res2 and empty describe the transform that went INTO the last step.  normals == NULL: the
 * normals are computed once on the device by pcreg_model_normals_f32's chain with this k (its range) and no viewpoint (the sign is
 * immaterial); ldn is ignored.  normals given: k is ignored and they are uploaded once, whatever `steps`.
 * PCREG_E_ARG: pcreg_model_refit_f32's cases; ldn < M with normals given; k outside 3 .. PCREG_KNN_MAX_K with normals NULL. */
int pcreg_model_refit_plane_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T /* host [B][16] */, int B, float r2,
                                int steps, const float* normals /* host M x 3, or NULL */, int ldn, int k, double* T_out /* [B][16] */,
                                int32_t* n_close, double* sum_d2, int32_t* n_plane, double* sum_res2, int32_t* empty);
/* The PLANE-TO-PLANE step of a refinement (generalized ICP; what MATLAB's pcregistericp offers as Metric = 'planeToPlane'), beside
 * pcreg_model_refit_f32 (point to point) and pcreg_model_refit_plane_f32 (point to plane): every pair is weighted by the inverse of
 * the sum of two regularised covariances, one per side, each flat along its own surface normal.  A pair so pulls fully ACROSS
 * either surface and about half as hard ALONG them, so the matrix stays definite where the point-to-plane step has nothing to
 * hold on to (a flat model).  A step, not an ICP policy: no convergence test, no robust kernel (pcreg_model_refit_gicp_trimmed_f32 keeps
 * each candidate's closest pairs), no claim of pcregistericp's bits.
 * THE CONTRACT of every tier (device, host, MEX, Python):
 * inputs -- those of pcreg_model_refit_plane_f32 (a prepared model, Q fp32 points column-major with ldq, B transforms of 16 doubles
 * used as quickTF.m uses them, r2 >= 0 with +inf allowed, the model's NORMALS M x 3 fp32 column-major by ORIGINAL row with
 * ldn >= M), the QUERY NORMALS Q x 3 fp32 column-major by query index with ldnq >= Q -- exactly what the normals entry points write
 * for a model made of the queries -- and EPSILON, a double in (0, 1] (1e-3 where a default is offered): the covariance of a side
 * is C = I - (1 - epsilon) n n^T, eigenvalues (1, 1, epsilon) for a unit normal, epsilon along it.  Normals are used as given and
 * are not renormalised.
 * THE PAIRS are scoring's, word for word (pcreg_model_refit_plane_f32: the transformed query p', the nearest row within the
 * radius, ties to the lowest original row); n_close[b] and sum_d2[b] are THE SAME BITS pcreg_model_score_f32 returns.  A
 * PLANE-TO-PLANE PAIR is a pair in which the model row's normal n and the query's normal nq each have three finite components and
 * the 3 x 3 matrix S below factorises with three pivots that are finite and above 0; n_pairs[b] their number.
 * PER PAIR (pcreg_amd/csrc/gicp_pair.hpp holds the one definition), in double on the widened fp32 values, without contraction;
 * a = 1 - epsilon, computed once on the host:
 *   1. the moved normal v_j = (nq_x T[4j] + nq_y T[4j+1]) + nq_z T[4j+2], j = 0, 1, 2: quickTF's chain without the translation; v
 *      stays in double.
 *   2. S = 2 I - a (n n^T + v v^T), which is C_model + R C_query R^T:  t_ij = n_i * n_j + v_i * v_j;  S_ii = 2.0 - a * t_ii;
 *      S_ij = 0.0 - a * t_ij for i < j.
 *   3. S = L L^T:  p0 = S_xx;  l00 = sqrt(p0);  l10 = S_xy / l00;  l20 = S_xz / l00;  p1 = S_yy - l10 * l10;  l11 = sqrt(p1);
 *      l21 = (S_yz - l20 * l10) / l11;  p2 = (S_zz - l20 * l20) - l21 * l21;  l22 = sqrt(p2).  The pair is dropped as soon as a
 *      pivot p_k is not a finite number above 0.
 *   4. M = L^-1:  m00 = 1.0 / l00;  m11 = 1.0 / l11;  m22 = 1.0 / l22;  m10 = -(l10 * m00) / l11;  m21 = -(l21 * m11) / l22;
 *      m20 = -(l20 * m00 + l21 * m10) / l22.
 *   5. W = S^-1 = M^T M:  W_xx = (m00 * m00 + m10 * m10) + m20 * m20;  W_xy = m10 * m11 + m20 * m21;  W_xz = m20 * m22;
 *      W_yy = m11 * m11 + m21 * m21;  W_yz = m21 * m22;  W_zz = m22 * m22.
 *   6. e = p - m and u = p - o (o, m, p as in pcreg_model_refit_plane_f32), and pcreg_ndt_refit_f32's PER PAIR terms with C := W
 *      and x := e:  y = W e,  qq = (e_0 y_0 + e_1 y_1) + e_2 y_2,  a_ij = J_i^T W J_j,  h_i = J_i . y.
 * THE SIGN of either set of normals cannot matter: n and v enter S through the products n_i n_j and v_i v_j alone, and negating nq
 * negates v exactly, so negating a normal gives the same bits.  With unit normals the eigenvalues of S lie in [2 epsilon, 2];
 * epsilon = 1 gives S = 2 I exactly (an unweighted point-to-point Gauss-Newton step).  A normal much longer than 1 makes S
 * indefinite and the pair is dropped.
 * THE 28 SUMS over the plane-to-plane pairs in ascending query order, each sum = sum + term (fma(1, term, sum)):
 *   [0..20] A_ij for i <= j, the upper triangle row-major;  [21..26] g_i accumulates h_i;  [27] sum_res2 accumulates qq = e^T W e.
 * Their order is pcreg_model_refit_plane_f32's: a thread adds its 8 consecutive queries in order, the wave's butterfly follows,
 * the four waves of a chunk of 2048 queries in ascending order, the chunks in ascending order from 0.  No floating-point atomic.
 * THE FIT is pcreg_model_refit_plane_f32's, unchanged, on these 28 sums with n_pairs in n_plane's place: the scaled Cholesky, the
 * pivot floor 2^-26, the Cayley rotation, T_step about o, T_out = T * T_step.  EMPTY by its rules: empty[b] = 1 and 32 zeros for
 * the all-zero T[b], n_pairs < 6, an A_ii not a finite number above 0, a pivot not above 2^-26, a non-finite x or T_step.  The
 * counts and sums are reported either way; a failed candidate stays failed when the step is repeated.
 * Q = 0 or a model without rows: every transform is empty, the counts and sums 0.  B = 0: nothing is written.
 * THIS entry runs `steps` >= 1 such steps on the device with one upload and one read, with pcreg_model_refit_plane_f32's staging
 * and its meaning of the outputs.  normals == NULL: the model's normals are computed once on the device with this k, as there.
 * qnormals == NULL: the query normals are computed once on the device from a temporary prepared model of q, with the same k and no
 * viewpoint; the temporary is released before the call returns.  Both given: k is ignored.
 * PCREG_E_ARG: pcreg_model_refit_plane_f32's cases (k is checked when either set is NULL); ldnq < Q with qnormals given; epsilon NaN
 * or outside (0, 1]. */
int pcreg_model_refit_gicp_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T /* host [B][16] */, int B, float r2,
                               int steps, const float* normals /* host M x 3, or NULL */, int ldn,
                               const float* qnormals /* host Q x 3, or NULL */, int ldnq, int k, double epsilon,
                               double* T_out /* [B][16] */, int32_t* n_close, double* sum_d2, int32_t* n_pairs, double* sum_res2,
                               int32_t* empty);
/* TRIMMED scoring and refits: the four entries above with one more control, the one pcregistericp calls InlierRatio --
 * of each transform's candidate pairs only the closest fraction is kept.  It is the robust choice of pairs the steps above say
 * they lack: on partly overlapping clouds a radius large enough to reach from the start pose also admits wrong partners, and
 * the far share of the pairs is where they sit.  No claim of pcregistericp's bits.
 * THE CONTRACT of every tier (device, host, MEX, Python):
 * inputs -- those of the untrimmed entry, and keep_ratio, a double in (0, 1].
 * THE CANDIDATE PAIRS of transform b are pcreg_model_score_f32's, unchanged: every query with a model row within r2, its nearest
 * such row and the fp32 d of that pair.  n_within[b] is their number, and
 *   keep = n_within == 0 ? 0 : min(n_within, max(1, (int)floor(keep_ratio * (double)n_within + 0.5)))
 * in double, the product rounded first and then the sum (no contraction).
 * THE KEPT PAIRS are the `keep` first candidate pairs in the order (d ascending, query index i ascending).  d is never negative
 * and never NaN for a pair, so its bit pattern orders as an unsigned integer (+inf, which r2 = +inf admits, comes last).
 * Equivalently: every pair with d < d2_cut[b] is kept, and among the pairs with d == d2_cut[b] the lowest i until `keep` is
 * reached.  d2_cut[b] is the largest kept d, or +inf when keep is 0.  (What a sort and a truncation give.)
 * EVERYTHING ELSE is the untrimmed entry's contract applied to the kept pairs, in ascending i: n_close and sum_d2 count and sum the
 * kept pairs in the same fixed order and tree; T_step, T_out and empty follow the same rules (fewer than three kept pairs, or the
 * all-zero T, give empty); n_plane / n_pairs and sum_res2 are taken among the kept pairs.  For scoring, idx / dist hold -1 / +inf
 * at trimmed slots, as at misses.  With steps > 1 every step trims anew, and all outputs describe the transform that went into
 * the last step.
 * keep_ratio = 1.0 keeps everything: every output then has the untrimmed entry's bits, and n_within == n_close.
 * r2 = +inf is allowed: InlierRatio with no distance at all.
 * Everything is a function of the inputs alone: the selection is an exact radix select on integer counts, no floating-point
 * atomic anywhere, and batching, culling, walk order and workgroup order change nothing.
 * n_within and d2_cut are [B]; either may be NULL.  Q = 0 or a model without rows: n_within = 0, d2_cut = +inf.
 * PCREG_E_ARG: the untrimmed entry's cases, and keep_ratio NaN, <= 0 or > 1. */
int pcreg_model_score_trimmed_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T /* host [B][16] */, int B, float r2,
                                  double keep_ratio, int32_t* n_close, double* sum_d2, int32_t* idx /* [B][Q] or NULL */,
                                  float* dist /* [B][Q] or NULL */, int32_t* n_within /* [B] or NULL */, float* d2_cut /* [B] or NULL */);
int pcreg_model_refit_trimmed_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T /* host [B][16] */, int B, float r2,
                                  double keep_ratio, int steps, double* T_out /* [B][16] */, int32_t* n_close, double* sum_d2,
                                  int32_t* empty, int32_t* n_within /* [B] or NULL */, float* d2_cut /* [B] or NULL */);
int pcreg_model_refit_plane_trimmed_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T /* host [B][16] */, int B,
                                        float r2, double keep_ratio, int steps, const float* normals /* host M x 3, or NULL */, int ldn,
                                        int k, double* T_out /* [B][16] */, int32_t* n_close, double* sum_d2, int32_t* n_plane,
                                        double* sum_res2, int32_t* empty, int32_t* n_within /* [B] or NULL */,
                                        float* d2_cut /* [B] or NULL */);
int pcreg_model_refit_gicp_trimmed_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T /* host [B][16] */, int B,
                                       float r2, double keep_ratio, int steps, const float* normals /* host M x 3, or NULL */, int ldn,
                                       const float* qnormals /* host Q x 3, or NULL */, int ldnq, int k, double epsilon,
                                       double* T_out /* [B][16] */, int32_t* n_close, double* sum_d2, int32_t* n_pairs, double* sum_res2,
                                       int32_t* empty, int32_t* n_within /* [B] or NULL */, float* d2_cut /* [B] or NULL */);
/* The COHERENT-POINT-DRIFT step of a refinement (rigid CPD; what MATLAB users reach for as pcregistercpd with Transform = 'Rigid'),
 * beside the three ICP steps and pcreg_ndt_refit_f32: every moved point is paired SOFTLY with EVERY live model row by a Gaussian
 * of their distance against a uniform outlier term, and the Gaussian's variance is annealed by its own closed form.  No radius, no
 * normals, no voxel size; a wide capture range; with a small variance it turns into the point-to-point step.  A step, not
 * pcregistercpd: no convergence test, no scale, no affine or non-rigid variant, no fast Gauss transform, no claim of its bits.
 * THE COST is B * Q * M pairs a step: this is for downsampled clouds (10^3 .. 10^4 points a side); nothing guards the size.
 * THE CONTRACT of every tier (device, host, MEX, Python):
 * inputs -- a prepared model of M rows, Q fp32 points column-major with ldq, B transforms of 16 doubles used as quickTF.m uses
 * them, sigma2_in [B] doubles (0 asks for the initial value below), and the OUTLIER weight w, a double in [0, 1).
 * ROLES: the moved queries are the DATA, the model rows the CENTROIDS of an equal-weight isotropic mixture plus a uniform term
 * (the reverse of Myronenko's roles; for a rigid motion without scale the same objective, and the right one for a surface that
 * is a crop of its model: every surface point has a partner, most model rows have none).
 * LIVE: a model row with three finite coordinates, and a query whose moved point p' has three finite coordinates (so a query
 * with a non-finite coordinate takes no part, and under an all-zero T[b] none does); Ml and Ql[b] their numbers, n_live[b] = Ql.
 * PER transform b and live query i:  p' is scoring's moved point, word for word (pcreg_model_score_f32: double arithmetic
 * without contraction, rounded once to fp32).  Against a live row m_j, in fp32: dx = m_j - p' by component,
 * d2_ij = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) -- the library's distance.  dmin_i = its minimum over the live rows: THE SAME BITS
 * pcreg_model_score_f32 reports as the nearest distance with r2 = +inf, taken from that chain; sum_d2[b] is that chain's sum.
 * With h = 1 / (2 sigma2) in double and k2 = (float)(-(h * log2(e))):
 *   e_ij = exp2((d2_ij - dmin_i) * k2) in fp32, in (0, 1] (the device's exp2 is within a unit or two in the last place; a result
 *   below 2^-126 may be 0);  S_i = sum_j e_ij >= 1;  V_i = sum_j e_ij (m_j - p'_i) by fmaf(e, dx, V);  W_i = sum_j fmaf(e, d2, W).
 * THE SHIFT by dmin_i is part of the contract: no 0 / 0 can arise.  The fp32 sums run over the live rows in ascending ORIGINAL row
 * order, in L = ceil(M / R) slices of R = 256 ceil(ceil(M / 256) / 32) rows (at most 32 slices; the last one shorter): a
 * slice's sum is sequential from 0, and the slices are added in ascending order from the first.
 * Then in double on the widened values, without contraction:
 *   c = ((2 pi sigma2) * sqrt(2 pi sigma2)) * (w / (1 - w)) * (Ml / Ql), or 0 when w == 0;  out_i = c * exp(dmin_i * h), or 0 when
 *   c == 0;  g_i = 1 / (S_i + out_i);  p_i = g_i * S_i.
 * With w = 0 every live query has p_i = 1 however far the model is.  With w > 0 a far query's exp may overflow to +inf, which
 * gives g_i = 0: the right limit.
 * THE 19 SUMS over the live queries, doubles, about the origin o -- the middle of the LIVE rows' box, 0.5f lo + 0.5f hi in fp32:
 * pcreg_model_refit_f32's origin whenever that is finite (an infinite row spoils that one, not this) -- with
 * u_i = p'_i - o, y_i = p_i u_i + g_i V_i (the weighted model side) and uu = (u0 u0 + u1 u1) + u2 u2:
 *   Np = sum p_i;  sum p_i u_i (3);  sum y_i (3);  sum u_i (x) y_i (9);  sum p_i uu;
 *   sum ((p_i uu + 2 ((u0 gV0 + u1 gV1) + u2 gV2)) + g_i W_i);  sum_res2 = sum g_i W_i, the weighted squared residual of the transform
 *   that went in.
 * Their order is pcreg_model_refit_plane_f32's: a thread adds its 8 consecutive queries in order, the wave's butterfly follows, the
 * four waves of a chunk of 2048 queries in ascending order, the chunks in ascending order from 0.  No floating-point atomic; every
 * order depends on (Q, M) alone.
 * THE FIT (pcreg_amd/csrc/cpd_fit.hpp holds the one definition): the weighted means, the centred 3 x 3 cross-covariance A, the
 * rotation R that maximises tr(A' R) WITH the determinant correction (coherent point drift's rule; estimateTransform.m has none)
 * from the Jacobi of A' A in a fixed operation order, t from the means, T_step about o, T_out = T * T_step by
 * pcreg_model_refit_f32's product, and
 *   sigma2_out = (weighted |m - mean|^2 - 2 tr(A' R) + weighted |p' - mean|^2) / (3 Np).
 * THE INITIAL VARIANCE: sigma2_in[b] == 0 asks for the mean squared distance over ALL (live query, live row) pairs divided by 3,
 * in closed form from eight sums about o -- sum u, sum uu over the live queries (the 19 sums' order) and sum v, sum vv, v = m - o,
 * over the live rows (thread t of 256 adds original rows t, t + 256, .. in order, then the butterfly and the four waves ascending):
 *   sigma2 = ((sum uu / Ql + sum vv / Ml) - 2 (mean u . mean v)) / 3.
 * EMPTY: empty[b] = 1, T_out[b] (and T_step[b]) sixteen 0.0 and sigma2_out[b] = 0 when T[b] is all zero or not finite; Ql < 3 or
 * Ml < 3; sigma2_in[b] is negative or NaN; sigma2, h or k2 is not finite and non-zero; Np is not a finite number above 0; the
 * second largest singular value of A is not above 2^-26 times the largest (a rotation the data does not determine is not
 * invented); sigma2_out is not a finite number above 0; T_step is not finite.  n_live and sum_d2 are reported either way, Np and
 * sum_res2 whenever the candidate got as far as its sums (0 otherwise).  A failed candidate stays failed when the step is repeated.
 * Q = 0 or a model without rows: every transform is empty, the counts and sums 0.  B = 0: nothing is written.
 * THIS entry runs `steps` >= 1 such steps on the device with one upload and one read; each step's sigma2_out is the next one's
 * sigma2_in, and Np, sum_res2, sum_d2 and n_live describe the transform that went INTO the last step.
 * DETERMINISM: the outputs of a candidate are the same bits on every call, at any position b, for any B, on any stream,
 * whatever the batching and whichever handle holds the model.
 * PCREG_E_ARG: pcreg_model_refit_f32's cases; outlier NaN or outside [0, 1); steps < 1. */
int pcreg_model_refit_cpd_f32(pcreg_model* model, const float* q, int Q, int ldq, const double* T /* host [B][16] */, int B,
                              const double* sigma2_in /* host [B] */, double outlier, int steps, double* T_out /* [B][16] */,
                              double* sigma2_out /* [B] */, double* Np /* [B] */, double* sum_res2 /* [B] */, double* sum_d2 /* [B] */,
                              int32_t* n_live /* [B] */, int32_t* empty /* [B] */);
/* clusterPoints.m:16-45  clusters = clusterPoints(pts, r) against the handle, with the SQUARED radius r2 = r^2: the connected
 * components of the graph in which rows i != j of the model are adjacent iff their fp32 squared distance
 * fmaf(dz,dz,fmaf(dy,dy,dx*dx)) <= r2 (inclusive; a NaN distance never passes; with r2 = +inf an overflowed distance between
 * finite rows passes).  A row with a non-finite coordinate has no neighbour and is a cluster of its own.  Clusters are numbered
 * 0, 1, .. in ascending order of their smallest row.  label [M]: the cluster of every row; *n_clusters their number (0 for
 * M = 0).  cl_off [M + 1] / members [M] (both or neither may be NULL; with M = 0 label and members may be): the clusters in CSR form, cluster c is
 * members[cl_off[c] .. cl_off[c + 1]), 0-based rows ascending; cl_off[0 .. n_clusters] is written.  Exact and deterministic: a
 * function of (model rows, r2) only.  r2 NaN or negative: PCREG_E_ARG. */
int pcreg_model_cluster_f32(pcreg_model* model, float r2, int32_t* label, int32_t* n_clusters, int32_t* cl_off, int32_t* members);
/* The same without a handle (clusterPoints(m, r)): uploads and prepares the cloud for this call only. */
int pcreg_cluster_points_f32(const float* m, int M, int ldm, float r2, int32_t* label, int32_t* n_clusters, int32_t* cl_off,
                             int32_t* members);
/* DBSCAN of the handle's rows -- MATLAB's dbscan(X, epsilon, minpts), scikit-learn's DBSCAN(eps, min_samples) -- with the SQUARED
 * radius r2 = epsilon^2 as a float and minpts >= 1.  THE CONTRACT of every tier (device, host, MEX, Python):
 *   NEIGHBOUR  rows i and j (j may equal i) are neighbours iff both are finite and fmaf(dz,dz,fmaf(dy,dy,dx*dx)) <= r2 in fp32:
 *              pcreg_model_cluster_f32's predicate, inclusive; a finite row is its own neighbour; a row with a non-finite
 *              coordinate has no neighbour, not even itself.
 *   COUNT      count[i] = the neighbours of row i, itself included: an exact integer, 0 for a non-finite row.
 *   CORE       core[i] = count[i] >= minpts.
 *   CLUSTERS   the connected components of the graph over the CORE rows in which two core rows are adjacent iff they are
 *              neighbours, numbered 0, 1, .. in ascending order of their smallest core row.
 *   BORDER     a row that is not core and has a core neighbour belongs to the smallest-numbered cluster among its core
 *              neighbours (what the sequential loops of MATLAB and scikit-learn give it).  It starts no cluster, joins no two
 *              clusters and does not affect the numbering.
 *   NOISE      every other row: label -1.  A non-finite row is always noise.
 * label [M] (0-based, -1 for noise); *n_clusters (0 for M = 0); core [M] (0 / 1) and count [M]: either may be NULL.  cl_off
 * [M + 1] / members [M] (both or neither may be NULL; with M = 0 label and members may be): the clusters in CSR form over the clusters ONLY, cluster c is
 * members[cl_off[c] .. cl_off[c + 1]), 0-based rows ascending, border rows included, noise rows in no cluster;
 * cl_off[0 .. n_clusters] is written.  minpts > M: all noise.  With minpts = 1 on finite rows the labels are
 * pcreg_model_cluster_f32's bit for bit.  Exact and deterministic: a function of (model rows, r2, minpts) only.
 * PCREG_E_ARG: r2 NaN or negative; minpts < 1; a NULL n_clusters; a NULL label with M > 0; one of cl_off / members alone. */
int pcreg_model_dbscan_f32(pcreg_model* model, float r2, int minpts, int32_t* label, int32_t* n_clusters, uint8_t* core, int32_t* count,
                           int32_t* cl_off, int32_t* members);
/* The same without a handle: uploads and prepares the cloud (M x 3 column-major, ldm >= M) for this call only. */
int pcreg_dbscan_points_f32(const float* m, int M, int ldm, float r2, int minpts, int32_t* label, int32_t* n_clusters, uint8_t* core,
                            int32_t* count, int32_t* cl_off, int32_t* members);
/* The surface normal of every row of the model from its k nearest rows (MATLAB's pcnormals(ptCloud, k); the third PCA axis
 * AlignPoints_KNN.m:29-34 takes of a neighbourhood).  THE CONTRACT of every tier (device, host, MEX, Python):
 * inputs -- a prepared model of M rows; k with 3 <= k <= PCREG_KNN_MAX_K; a viewpoint of three doubles on the host, or NULL.
 * THE NEIGHBOURHOOD of row i is what pcreg_model_knn_f32 returns for query = row i and the same k: the k model rows with the
 * smallest fp32 fmaf(dz,dz,fmaf(dy,dy,dx*dx)), ordered by (distance, original row), ties to the lowest row; row i itself is in
 * it at distance 0.  A row with a non-finite coordinate is never a neighbour (nor is a row whose computed distance overflows to
 * +inf), and its own neighbourhood is empty.  n <= k is the number of neighbours found; n < k only when the model has fewer than
 * k finite rows.
 * THE ARITHMETIC is double throughout, on the widened fp32 coordinates, without contraction, the neighbours taken in (distance,
 * row) order: (1) the mean, each coordinate summed in that order and divided by n; (2) the six sums xx, xy, xz, yy, yz, zz of
 * the products of the centred coordinates, in that order, NOT divided by n; (3) the library's cyclic Jacobi on that symmetric
 * matrix (jacobi_sym3, as it is); (4) the eigenvector column of the smallest of the three diagonal entries, ties to the lowest
 * index; (5) each component rounded once to fp32, not renormalised.
 * THE SIGN is decided on the rounded components, widened again.  With a viewpoint v and p the row:
 * s = ((nx*(vx-px) + ny*(vy-py)) + nz*(vz-pz)) in double, and the normal is negated iff s < 0.  Without one: the component of
 * largest magnitude, the first of equals in x, y, z order, is made non-negative.  Negation is exact, so the two forms differ by
 * sign only, bit for bit.
 * variation[i] (may be NULL) = lambda_min / ((lambda_0 + lambda_1) + lambda_2) of the diagonal Jacobi leaves, rounded to fp32:
 * the surface variation by which a caller judges a normal.
 * Normal and variation are NaN when n < 3 (so for a non-finite row) and when the trace is not positive (coincident neighbours).
 * A collinear neighbourhood gets whatever Jacobi gives: deterministic, judged by the caller through the variation.
 * normals: M x 3 fp32 column-major with leading dimension ldn >= M, indexed by ORIGINAL row; variation [M].  M = 0 writes nothing.
 * The result is a function of (model rows, k, viewpoint) only: no floating-point atomic; culling, the call and the stream change
 * no bit.  PCREG_E_ARG: k outside 3 .. PCREG_KNN_MAX_K, ldn < M. */
int pcreg_model_normals_f32(pcreg_model* model, int k, const double* viewpoint /* host, 3 or NULL */, float* normals, int ldn,
                            float* variation /* or NULL */);
/* The same without a handle (pcnormals(m, k)): uploads and prepares the cloud for this call only. */
int pcreg_point_normals_f32(const float* m, int M, int ldm, int k, const double* viewpoint, float* normals, int ldn, float* variation);
/* Statistical outlier removal over the rows of the model (MATLAB's pcdenoise(ptCloud, 'NumNeighbors', k, 'Threshold', t); PCL's
 * StatisticalOutlierRemoval).  THE CONTRACT of every tier (device, host, MEX, Python):
 * inputs -- a prepared model of M rows; k = NumNeighbors with 1 <= k <= PCREG_KNN_MAX_K - 1 (the list holds k + 1 entries, the
 * row itself among them); threshold t, a finite double >= 0.
 * THE NEIGHBOURHOOD of row i is what pcreg_model_knn_f32 returns for query = row i with k + 1: the k + 1 smallest fp32
 * fmaf(dz,dz,fmaf(dy,dy,dx*dx)) among the finite rows, the first of them always 0 (the row itself, or a coincident row).  A row
 * with a non-finite coordinate is never a neighbour and has none; a distance that overflows to +inf is no neighbour.  Only the
 * multiset of the distances matters, not which row a tied distance belongs to.  n <= k + 1 is the number found; n < k + 1 only
 * when the model has fewer than k + 1 finite rows.
 * THE MEAN DISTANCE d_i, in double without contraction: each of the n squared distances widened to double, its double square
 * root (correctly rounded), the roots added in ascending order from 0.0 (the leading 0 adds nothing, which is how MATLAB drops
 * the first column), the sum divided by (double)(n - 1).  n <= 1, and so a non-finite row, gives d_i = NaN.
 * THE STATISTIC.  nf: the rows with a finite d_i.  mu: their sum / nf.  sd: MATLAB's std, two passes --
 * sqrt(sum of (d_i - mu)^2 / (nf - 1)), 0 when nf = 1.  thr = mu + t * sd (a product, then a sum).  nf = 0 gives mu, sd and thr NaN.
 * THE ORDER OF THE TWO SUMS is a function of M alone.  The rows are cut into chunks of 2048 consecutive ORIGINAL rows.  Inside a
 * chunk, part p (0 .. 255) adds its terms for rows 8 p .. 8 p + 7 of the chunk in ascending order from 0.0, a row that is not
 * finite (or past M) adding nothing; the 256 parts are added by the TREE: within each group of 64 consecutive parts, pairwise at
 * distance 32, then 16, 8, 4, 2, 1 (every part ends with its group's sum), then the four group sums as (g0 + g1) + (g2 + g3).
 * The chunk sums are added likewise: part p adds chunks p, p + 256, ... in ascending order from 0.0, then the same tree.  No
 * floating-point atomic anywhere.
 * THE RESULT.  Row i is an inlier iff d_i <= thr on the RETURNED doubles (NaN on either side: no inlier), so a caller restates
 * the mask to the bit from mean_dist and stats[0].
 * outputs, each may be NULL -- mean_dist [M], by ORIGINAL row; inliers [capacity M]: the 0-based original rows of the inliers,
 * ascending, *n_inliers of them (inliers given needs n_inliers; n_inliers alone counts); stats [4] = {thr, mu, sd, (double) nf}.
 * M = 0 writes *n_inliers = 0, stats = {NaN, NaN, NaN, 0} and nothing else.
 * The result is a function of (model rows, k, t) only: culling, the call, the stream and the workspace's previous contents change
 * no bit.  PCREG_E_ARG: k outside 1 .. PCREG_KNN_MAX_K - 1, t negative or not finite, model NULL, inliers without n_inliers. */
int pcreg_model_denoise_f32(pcreg_model* model, int k, double threshold, double* mean_dist /* [M] or NULL */,
                            int32_t* inliers /* [M] or NULL */, int32_t* n_inliers /* or NULL */, double* stats /* [4] or NULL */);
/* The same without a handle (pcdenoise(m, ...)): uploads and prepares the cloud for this call only.  Also PCREG_E_ARG: M < 0,
 * ldm < M, m NULL with M > 0. */
int pcreg_point_denoise_f32(const float* m, int M, int ldm, int k, double threshold, double* mean_dist, int32_t* inliers,
                            int32_t* n_inliers, double* stats);
/* Farthest point sampling of the rows of the model: at most K rows, each the live row farthest from all rows chosen before it, with
 * the covering radius at every row (PointNet++'s sampling layer; Open3D's farthest_point_down_sample).  THE CONTRACT of every tier
 * (device, host, MEX, Python):
 * inputs -- a prepared model of M fp32 rows, M <= PCREG_FPS_MAX_ROWS; K >= 0, the capacity of idx / dist and the most samples wanted;
 * start, a 0-based ORIGINAL row with 0 <= start < M, or -1 for the lowest live original row; stop_d2, a float >= 0 and not NaN
 * (+inf is allowed and gives one sample).
 * A row is LIVE when its three coordinates are finite.  Dead rows are never samples and never measured; nf is the live count.
 * THE DISTANCE is the point search's: fmaf(dz,dz, fmaf(dy,dy, dx*dx)) with fp32 differences; it is sign-symmetric.
 * THE STATE: D[i] = +inf and L[i] = 0 for every live row i.
 * THE LOOP: s_0 = start (or the lowest live row).  For j = 0, 1, ...:
 *   1. idx[j] = s_j; dist[j] is the value D[s_j] had when s_j was chosen; dist[0] = +inf.
 *   2. For every live i, d = the distance of row i and row s_j; when d < D[i] (strictly), D[i] = d and L[i] = j + 1.
 *   3. (mx, r): the largest D[i] over the live rows, ties to the LOWEST ORIGINAL row.
 *   4. Stop with *n_out = j + 1 when j + 1 == K or when !(mx > stop_d2); otherwise s_{j+1} = r.
 * So: with stop_d2 = 0 the loop ends by itself once every live row coincides with a sample (squared distances that underflow to 0
 * included); a row never repeats in idx; dist[1..] is non-increasing; +inf distances (overflow) are ordinary values.
 * outputs, each may be NULL except n_out -- idx [K]: int32 original rows in selection order, 0-based (1-based at the MEX / MATLAB
 * edge); dist [K]: fp32, squared; *n_out; *cover_d2: one fp32, the mx of the last step -- after the call every live row is within
 * sqrt(cover_d2) of a sample; min_dist [M]: fp32 by original row, the final D, NaN for a dead row; label [M]: int32 by original row,
 * the final L: the 1-based position in idx of the nearest sample, ties to the EARLIEST sample, 0 for a dead row (and for a live row
 * whose every distance overflowed to +inf, which the strict < never labels).  Only idx[0 .. n_out) and dist[0 .. n_out) are written.
 * K = 0, M = 0 or nf = 0: *n_out = 0; cover_d2, min_dist and label are still written, as NaN / NaN / 0 for whatever rows exist;
 * nothing else is written.  (K = 0 is judged first: it does not look at the start row.)
 * The result is a function of (model rows, K, start, stop_d2) only: culling, the call, the stream and the workspace's previous
 * contents change no bit.
 * PCREG_E_ARG before anything runs: K < 0, start outside -1 .. M - 1 with M > 0, stop_d2 negative or NaN, model NULL, n_out NULL,
 * M > PCREG_FPS_MAX_ROWS.  A start row that is DEAD is known only on the device: PCREG_E_ARG after the run, with a message that names
 * start and no output written. */
#define PCREG_FPS_MAX_ROWS 2097152               /* 2^21: 4096 tiles of 512 rows, the tile table one workgroup's LDS holds */
int pcreg_model_fps_f32(pcreg_model* model, int K, int start, float stop_d2, int32_t* idx /* [K] or NULL */, float* dist /* [K] or NULL */,
                        int32_t* n_out, float* cover_d2 /* or NULL */, float* min_dist /* [M] or NULL */, int32_t* label /* [M] or NULL */);
/* The same without a handle: uploads and prepares the cloud for this call only.  Also PCREG_E_ARG: M < 0, ldm < M, m NULL with
 * M > 0. */
int pcreg_point_fps_f32(const float* m, int M, int ldm, int K, int start, float stop_d2, int32_t* idx, float* dist, int32_t* n_out,
                        float* cover_d2, float* min_dist, int32_t* label);
/* The FPFH descriptor of every row of the model (MATLAB's extractFPFHFeatures(ptCloud, 'NumNeighbors', k)): 33 numbers a row from
 * its k nearest rows and a normal per row.  The name and the pair features are Rusu's (Fast Point Feature Histograms, ICRA 2009);
 * the weighting and the normalisation have the form common implementations use.  THE CONTRACT of every tier (device, host, MEX,
 * Python) is THIS TEXT, not any library's source; MATLAB's bits are not knowable here.
 * inputs -- a prepared model of M fp32 rows; k with 3 <= k <= PCREG_KNN_MAX_K; normals, M x 3 fp32 column-major with ldn >= M, by
 * ORIGINAL row, exactly what pcreg_model_normals_f32 writes, used as they are (not renormalised).  Unlike the plane refit, THE SIGN
 * of a normal matters here: orient the normals with a viewpoint.
 * THE NEIGHBOURHOOD of row i is what pcreg_model_knn_f32 returns for query = row i with this k, in its (distance, original row)
 * order.  The NEIGHBOURS of i are the list entries with a row and a finite fp32 squared distance d2 > 0: entries at distance 0 (the
 * row itself, coincident rows) are not neighbours.  A row with a non-finite coordinate is never a neighbour and has no
 * neighbourhood.  At most k - 1 <= 31 neighbours: the row itself takes a place of its list.
 * THE PAIR (i, j), j a neighbour of i.  All arithmetic is double on the widened fp32 values, without contraction; every three-term
 * sum is (x + y) + z; sqrt and division are correctly rounded.  d = p_j - p_i; len = sqrt((dx dx + dy dy) + dz dz);
 * a_i = ((n_i.x dx + n_i.y dy) + n_i.z dz) / len; a_j the same with n_j.  If |a_i| < |a_j| (strictly) the source is j: ns = n_j,
 * nt = n_i, d <- -d, f3 = -a_j; otherwise, a tie included, the source is i: ns = n_i, nt = n_j, f3 = a_i.  v = d x ns;
 * vl = sqrt(v . v); v <- v / vl componentwise; w = ns x v; f2 = v . nt; f1 = atan2(w . nt, ns . nt).
 * The pair CONTRIBUTES unless len or vl is not > 0, or any of f1, f2, f3 is NaN, or either normal has a non-finite component.
 * Bins, eleven a feature: b1 = floor(11 ((f1 + pi) / (2 pi))), b2 = floor(11 ((f2 + 1) 0.5)), b3 = floor(11 ((f3 + 1) 0.5)), each
 * clamped to 0 .. 10 (pi the double nearest to it).
 * SPFH of row i: integer counts c_i[33], f1's eleven bins, then f2's, then f3's, over the contributing pairs; m_i their number (the
 * sum of the first eleven counts, and of each other eleven).
 * FPFH of row i: acc[b] = the sum over the neighbours j of i, in list order, with m_j > 0, of (c_j[b] / m_j) / d2_ij, d2_ij the
 * list's fp32 SQUARED distance widened to double (the conventional weight: the inverse of the squared distance, as the common
 * implementations take it); the row's own SPFH is not added.  Per feature f: S_f = the sum of its eleven acc in bin order from the
 * first; S_f > 0: out[b] = (acc[b] / S_f) * 100 (the division first, so a histogram of one bin is exactly 100); otherwise out[b] = 0.
 * A row with a non-finite coordinate gets 33 NaN; a row whose neighbourhood yields nothing gets 33 zeros (fewer than 2 finite
 * distinct rows, all rows coincident).
 * outputs -- fpfh: M x 33 double column-major with ldf >= M, by ORIGINAL row; spfh (may be NULL): the SPFH counts, uint8 [M][33]
 * ROW-major by original row.  M = 0 writes nothing.
 * normals == NULL: they are computed in the call by pcreg_model_normals_f32's chain with k_normals (its range) and the viewpoint
 * (three host doubles or NULL); ldn is ignored.  normals given: they are uploaded once; k_normals and viewpoint are ignored.
 * The result is a function of (model rows, normals, k) only: no floating-point atomic, no sum across threads; culling, the call,
 * the stream and the workspace's previous contents change no bit.  PCREG_E_ARG, before anything runs: k outside
 * 3 .. PCREG_KNN_MAX_K; ldn < M with normals given; k_normals outside its range with normals NULL; ldf < M; model NULL; fpfh NULL
 * with M > 0. */
int pcreg_model_fpfh_f32(pcreg_model* model, int k, const float* normals /* host M x 3, or NULL */, int ldn, int k_normals,
                         const double* viewpoint /* host, 3 or NULL */, double* fpfh /* M x 33, ld ldf */, int ldf,
                         uint8_t* spfh /* [M][33] or NULL */);
/* The same without a handle (extractFPFHFeatures(m, ...)): uploads and prepares the cloud for this call only.  Also PCREG_E_ARG:
 * M < 0, ldm < M, m NULL with M > 0. */
int pcreg_point_fpfh_f32(const float* m, int M, int ldm, int k, const float* normals, int ldn, int k_normals, const double* viewpoint,
                         double* fpfh, int ldf, uint8_t* spfh);
/* The FPFH descriptor of every row of the model from the rows within a radius (MATLAB's extractFPFHFeatures(ptCloud, 'Radius', r),
 * and with max_neighbors its 'NumNeighbors' beyond the k-nearest list's PCREG_KNN_MAX_K: the n nearest rows within the radius).  THE
 * CONTRACT of every tier (device, host, MEX, Python) is THIS TEXT; everything it does not restate is
 * pcreg_model_fpfh_f32's above: the normals and their sign, the pair features and their arithmetic, the bins, S_f, the output.
 * inputs -- a prepared model of M fp32 rows, M <= 4 Mi (the radius search's queries per call: this call sends the rows as ONE
 * batch); r2, the SQUARED radius as pcreg_model_range_f32 takes it (a float >= 0; +inf allowed); max_neighbors n >= 0; normals as
 * pcreg_model_fpfh_f32 takes them.
 * THE NEIGHBOURHOOD of row i is what pcreg_model_range_f32 returns for query = row i at r2, in its (distance, original row) order:
 * the radius is inclusive and the distances are the fp32 chain's.  The NEIGHBOURS of i are the entries with a finite squared
 * distance d2 > 0: the row itself and coincident rows are not neighbours, and they do not count against n.  With n > 0 only the
 * first n neighbours in that order COUNT (the n nearest within the radius; a row with fewer uses what is there); with n = 0 all of
 * them count.  A row with a non-finite coordinate has no neighbourhood and is nobody's neighbour.
 * SPFH of row i: the integer counts c_i[33] over the contributing pairs (i, j), j a counted neighbour; m_i their number.  A count
 * may reach M - 1, so the counts are uint32.
 * FPFH of row i: acc[b] = the sum over the counted neighbours j of i with m_j > 0, in list order, of (c_j[b] / m_j) / d2_ij; S_f,
 * out[b] = (acc[b] / S_f) * 100, 33 NaN for a row with a non-finite coordinate and 33 zeros for an empty neighbourhood (r2 = 0
 * included) exactly as there.  With a radius that covers the cloud, no coincident rows and n = k - 1 the result is
 * pcreg_model_fpfh_f32's at k, bit for bit.
 * outputs -- fpfh: M x 33 double column-major with ldf >= M, by ORIGINAL row; spfh (may be NULL): the SPFH counts, uint32 [M][33]
 * ROW-major by original row; n_neighbors (may be NULL): int32 [M], the neighbours counted for row i, 0 for a non-finite row.
 * M = 0 writes nothing.  normals == NULL / given: as pcreg_model_fpfh_f32.
 * The call counts the neighbourhoods, reads their total once, and holds the lists on the device: 8 bytes per (row, neighbour) pair
 * within the radius (max_neighbors does not shrink that).  When the device cannot hold them the call returns PCREG_E_HIP and
 * pcreg_last_error() names the total.
 * The result is a function of (model rows, normals, r2, max_neighbors) only: no floating-point atomic, no floating-point sum
 * across threads; culling, the call, the stream and the workspace's previous contents change no bit.  PCREG_E_ARG, before anything
 * runs: r2 NaN or negative; max_neighbors < 0; M > 4 Mi; ldn < M with normals given; k_normals outside 3 .. PCREG_KNN_MAX_K with
 * normals NULL; ldf < M; model NULL; fpfh NULL with M > 0. */
int pcreg_model_fpfh_radius_f32(pcreg_model* model, float r2, int max_neighbors, const float* normals /* host M x 3, or NULL */, int ldn,
                                int k_normals, const double* viewpoint /* host, 3 or NULL */, double* fpfh /* M x 33, ld ldf */, int ldf,
                                uint32_t* spfh /* [M][33] or NULL */, int32_t* n_neighbors /* [M] or NULL */);
/* The same without a handle: uploads and prepares the cloud for this call only.  Also PCREG_E_ARG: M < 0, ldm < M, m NULL with
 * M > 0. */
int pcreg_point_fpfh_radius_f32(const float* m, int M, int ldm, float r2, int max_neighbors, const float* normals, int ldn, int k_normals,
                                const double* viewpoint, double* fpfh, int ldf, uint32_t* spfh, int32_t* n_neighbors);
/* ISS keypoints of the rows of the model (MATLAB's detectISSFeatures(ptCloud, 'SalientRadius', rs, 'NonMaxRadius', rn, 'Threshold21',
 * g21, 'Threshold32', g32, 'MinNeighbors', n); Zhong's Intrinsic Shape Signatures, ICCV Workshops 2009; PCL's ISSKeypoint3D, Open3D's
 * compute_iss_keypoints).  THE CONTRACT of every tier (device, host, MEX, Python) is THIS TEXT, not any library's
 * source; MATLAB's bits are not knowable here.
 * inputs -- a prepared model of M fp32 rows, M < 2^26; r2_salient and r2_nonmax, SQUARED radii as floats, each finite, normal and
 * > 0 (a wrapper that takes radii squares them in double and rounds the square once to single); gamma21 and gamma32, finite doubles
 * > 0; min_neighbors >= 1.
 * THE NEIGHBOURHOOD of row i at r2 is every row j, i itself included, with d = fmaf(dz, dz, fmaf(dy, dy, dx*dx)) <= r2, dx = m_j - m_i
 * in fp32: the predicate of pcreg_model_range_f32 and pcreg_model_cluster_f32, inclusive, and NaN never passes.  A row with a
 * non-finite coordinate is in no neighbourhood and has none: its n = 0, its eigenvalues are NaN, its saliency is 0.
 * THE EXACT SCATTER.  Let e2 be the binary exponent of r2_salient (frexp: r2 = f 2^e2, f in [0.5, 1)) and e = ceil(e2 / 2).  Per
 * neighbour and component q = rint(dx 2^(18 - e)), round-to-nearest-even of the exactly scaled fp32 difference, so |q| <= 2^18 + 1.
 * Over the neighbourhood n, S1[3] = sum q and S2[6] = sum q_a q_b are integers, summed exactly in 64 bits (M < 2^26 keeps them
 * there).  N = n S2 - S1 S1^T is formed exactly and each of its six entries is rounded ONCE to double.  Nothing here depends on the
 * order of summation.
 * THE EIGENVALUES.  mu1 >= mu2 >= mu3 are the eigenvalues of N in double by cyclic Jacobi, sorted.  Reported:
 * lambda_c = (mu_c / (double)(n n)) * 4^-(18 - e), in that order of operations -- the eigenvalues of the covariance about the
 * neighbourhood's mean, in the model's units.
 * THE CANDIDATE.  Row i is a candidate iff n >= min_neighbors and mu2 < gamma21 * mu1 and mu3 < gamma32 * mu2 and mu3 > 0 (products
 * in double, no division).  Saliency s_i = lambda_3 for a candidate, else 0.  A neighbourhood in a coordinate plane or on a
 * coordinate axis gives mu3 == 0 exactly: the integer sums have exact zeros there.
 * THE KEYPOINT.  Row i is a keypoint iff s_i > 0 and no row j != i of its r2_nonmax neighbourhood has s_j > s_i, or s_j == s_i with
 * j < i (original rows).  Coincident rows are neighbours of each other.  A caller restates the list to the bit from the returned
 * saliencies and the fp32 predicate.
 * outputs -- n_neighbors [M] int32; eig [M][3] double ROW-major, descending (may be NULL); saliency [M] double; keypoints [capacity
 * M]: the 0-based original rows of the keypoints, ascending, *n_keypoints of them (keypoints given needs n_keypoints; n_keypoints
 * alone counts; both NULL skips the suppression).  M = 0 writes *n_keypoints = 0 and nothing else.
 * The result is a function of (model rows, parameters) only: the in-cell order of the prepared model, culling, the call, the stream
 * and the workspace's previous contents change no bit, and a permutation of the rows permutes the per-row outputs.
 * PCREG_E_ARG, before anything runs: a radius that is zero, negative, subnormal, infinite or NaN; a gamma that is not finite or not
 * > 0; min_neighbors < 1; M >= 2^26; model NULL; n_neighbors or saliency NULL with M > 0; keypoints without n_keypoints. */
int pcreg_model_iss_f32(pcreg_model* model, float r2_salient, float r2_nonmax, double gamma21, double gamma32, int min_neighbors,
                        int32_t* n_neighbors /* [M] */, double* eig /* [M][3] or NULL */, double* saliency /* [M] */,
                        int32_t* keypoints /* [M] or NULL */, int32_t* n_keypoints /* or NULL */);
/* The same without a handle (detectISSFeatures(m, ...)): uploads and prepares the cloud for this call only.  Also PCREG_E_ARG:
 * M < 0, ldm < M, m NULL with M > 0. */
int pcreg_point_iss_f32(const float* m, int M, int ldm, float r2_salient, float r2_nonmax, double gamma21, double gamma32,
                        int min_neighbors, int32_t* n_neighbors, double* eig, double* saliency, int32_t* keypoints,
                        int32_t* n_keypoints);

/* MSAC plane fitting and plane extraction over the rows of the model (MATLAB's pcfitplane(ptCloud, maxDistance[, referenceVector,
 * maxAngularDistance]) and the loop that follows it: fit, take the inliers out, fit again -- up to max_planes times in one call).
 * THE CONTRACT of every tier (device, host, MEX, Python) is THIS TEXT; MATLAB's bits are not knowable here
 * (INTEGRATION.md).
 * inputs -- a prepared model of M fp32 rows, M < 2^26; max_distance t, a float, finite, normal and > 0, whose square
 * t2 = fl32(t * t) is a normal float too; s = (float)(2^20 / (double)t2); ref_vec, three doubles or NULL, and with it max_angle in
 * (0, pi/2] radians (ignored without it); max_planes P in 1 .. 64; n_trials B in 1 .. 2^20; min_inliers >= 3; seed; samples, int32
 * [P][B][3] or NULL: 1-BASED original rows at this tier.
 * ALIVE ROWS.  Initially the rows whose three coordinates are finite.  A non-finite row is never alive, never an inlier, label 0.
 * THE QUANTISATION SCALE.  D is the largest axis extent (hi - lo of the fp32 limits, in double) of the finite rows and e frexp's
 * exponent of D (D = f 2^e, f in [0.5, 1)).  D == 0 or no finite row: every trial is void and there is no plane.
 * ROUND p = 0 .. P - 1, over the alive set A_p listed ascending by original row, nA rows.
 * Trial b has rows i_j, j = 0 .. 2: from samples[p][b][j] when the table is given, else i_j = A_p[h_j % nA] with
 * h_j = splitmix64(seed ^ splitmix64(((uint64)p * B + b) * 4 + j)) and splitmix64(x): x += 0x9E3779B97F4A7C15; z = x;
 * z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31), all modulo 2^64.
 * A trial is VOID if an index is out of range, a row is not alive, two indices are equal, or, with a = p1 - p0 and b = p2 - p0 in
 * double and c = a x b, each component fl(fl(a_u b_v) - fl(a_v b_u)) in double without contraction, L2 = (cx cx + cy cy) + cz cz is
 * not > 0 or not finite.  n = c / sqrt(L2), three divisions.  THE SIGN of n: with ref_vec, dot = (nx rx + ny ry) + nz rz, n is
 * negated when dot < 0, and the trial is void when |dot| / |ref| < cos(max_angle), |ref| = sqrt((rx rx + ry ry) + rz rz);
 * without it, n is negated so that its component of largest magnitude is positive, the first in x, y, z order winning a tie.
 * SCORING, per alive row, in fp32: nf = (float)n; d = row - p0 componentwise; r = fmaf(nf.z, d.z, fmaf(nf.y, d.y, nf.x * d.x));
 * r2 = r * r; the row is an inlier iff r2 <= t2 (NaN never passes); q = min(2^20, (int)rintf(r2 * s)) for an inlier, 2^20
 * otherwise.  cost_b is the sum of q and count_b the number of inliers: integers, so no bit depends on the order of summation.
 * THE BEST TRIAL is, among the non-void trials with count >= 3, the one of smallest cost, ties to the smallest b.  No such trial,
 * or its count < min_inliers: extraction ends with n_planes = p.  The diagnostics of that last round are still recorded
 * (best_trial = -1, cost and count 0 where no trial was eligible).
 * THE REFIT, on the best trial's inliers: g = rint((double)d * 2^(17 - e)) per component (|g| <= 2^17); n, S1[3] = sum g and
 * S2[6] = sum g_a g_b are 64-bit integers; N = n S2 - S1 S1^T exactly in 128 bits, each entry rounded once to double
 * (pcreg_model_iss_f32's construction).  The normal is the eigenvector of N's smallest eigenvalue by cyclic Jacobi in double
 * (the first of equal eigenvalues in x, y, z order of the rotated diagonal), signed by the rule above; the angle test is not
 * repeated.  centre = (double)p0 + ((double)S1 / (double)n) * 2^-(17 - e); d4 = -((nx cx + ny cy) + nz cz).
 * THE FINAL CLASSIFICATION, over the alive rows: the same fp32 chain with (float)normal and row - (float)centre.  The passing
 * rows get label p + 1 and leave the alive set; count_p is their number, Q_p the sum of their q, and
 * rmse_p = sqrt(((double)Q_p / count_p) * ((double)t2 * 2^-20)).
 * outputs -- labels [M] int32 by original row (0: no plane); planes [P][4] double ROW-major (nx, ny, nz, d4); centres [P][3];
 * counts [P] int32; rmse [P]; *n_planes; the diagnostics best_trial [P] int32 (0-based), best_cost [P] int64, best_count [P] int32,
 * each may be NULL.  Entries of rounds that did not run are zero.  M = 0 writes *n_planes = 0 and zeros.
 * The result is a function of (original rows, parameters) only: the call, the stream and the workspace's previous contents
 * change no bit.
 * PCREG_E_ARG, before anything runs: M >= 2^26; t or t2 zero, negative, subnormal, infinite or NaN; P, B or min_inliers out of
 * range; ref_vec not finite or zero; max_angle out of range with ref_vec; model or n_planes NULL; labels, planes, centres, counts
 * or rmse NULL with M > 0; a sample table entry is never an error (the trial is void). */
int pcreg_model_fit_planes_f32(pcreg_model* model, float max_distance, const double* ref_vec /* [3] or NULL */, double max_angle,
                               int max_planes, int n_trials, int min_inliers, uint64_t seed, const int32_t* samples /* [P][B][3] or NULL */,
                               int32_t* labels /* [M] */, double* planes /* [P][4] */, double* centres /* [P][3] */,
                               int32_t* counts /* [P] */, double* rmse /* [P] */, int32_t* n_planes, int32_t* best_trial /* or NULL */,
                               int64_t* best_cost /* or NULL */, int32_t* best_count /* or NULL */);
/* The same without a handle (pcfitplane(m, ...)): uploads and prepares the cloud for this call only.  Also PCREG_E_ARG:
 * M < 0, ldm < M, m NULL with M > 0. */
int pcreg_point_fit_planes_f32(const float* m, int M, int ldm, float max_distance, const double* ref_vec, double max_angle, int max_planes,
                               int n_trials, int min_inliers, uint64_t seed, const int32_t* samples, int32_t* labels, double* planes,
                               double* centres, int32_t* counts, double* rmse, int32_t* n_planes, int32_t* best_trial,
                               int64_t* best_cost, int32_t* best_count);

/* MSAC sphere fitting and sphere extraction over the rows of the model (MATLAB's pcfitsphere(ptCloud, maxDistance) and the loop over
 * it: fit, take the inliers out, fit again -- up to max_spheres times in one call; the fiducial markers and ball tips of a scan).
 * THE CONTRACT of every tier (device, host, MEX, Python) is THIS TEXT; MATLAB's bits are not knowable here
 * (INTEGRATION.md).
 * inputs -- a prepared model of M fp32 rows, M < 2^26; max_distance t under pcreg_model_fit_planes_f32's rules (a float, finite,
 * normal and > 0, whose square t2 = fl32(t * t) is a normal float too; s = (float)(2^20 / (double)t2)); min_radius and max_radius,
 * floats with 0 <= min_radius <= max_radius, max_radius may be +inf, both compared as floats; max_spheres P in 1 .. 64; n_trials B
 * in 1 .. 2^20; min_inliers >= 4; seed; samples, int32 [P][B][4] or NULL: 1-BASED original rows at this tier.
 * ALIVE ROWS.  Initially the rows whose three coordinates are finite.  A non-finite row is never alive, never an inlier, label 0.
 * THE QUANTISATION SCALE.  D is the largest axis extent (hi - lo of the fp32 limits, in double) of the finite rows and e frexp's
 * exponent of D (D = f 2^e, f in [0.5, 1)); e = 0 where D == 0 or there is no finite row.
 * ROUND p = 0 .. P - 1, over the alive set A_p listed ascending by original row, nA rows.
 * Trial b has rows i_j, j = 0 .. 3: from samples[p][b][j] when the table is given, else i_j = A_p[h_j % nA] with
 * h_j = splitmix64(seed ^ splitmix64(((uint64)p * B + b) * 4 + j)), splitmix64 as at pcreg_model_fit_planes_f32.
 * THE TRIAL'S SPHERE, the circumsphere of its four rows p_0 .. p_3, in double, every step ONE correctly rounded operation, no
 * contraction, in this order: d_i = (double)p_i - (double)p_0, i = 1, 2, 3; b_i = (d_ix d_ix + d_iy d_iy) + d_iz d_iz; the cross
 * products X1 = d_2 x d_3, X2 = d_3 x d_1, X3 = d_1 x d_2, each component fl(fl(a_u c_v) - fl(a_v c_u)) of a x c;
 * det = (d_1x X1x + d_1y X1y) + d_1z X1z; u = ((b_1 X1 + b_2 X2) + b_3 X3) / (2 det) component by component;
 * R2 = (ux ux + uy uy) + uz uz; R = sqrt(R2); in fp32 cf = (float)((double)p_0 + u) and Rf = (float)R.
 * A trial is VOID if an index is out of range, a row is not alive, any two of the four indices are equal, det is zero or not
 * finite, a component of u, R, a component of cf or Rf is not finite, or Rf < min_radius or Rf > max_radius.
 * SCORING, per alive row, in fp32: d = row - cf componentwise; d2 = fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x)); rho = the correctly
 * rounded fp32 square root of d2; r = rho - Rf; r2 = r * r; the row is an inlier iff r2 <= t2 (NaN never passes);
 * q = min(2^20, (int)rintf(r2 * s)) for an inlier, 2^20 otherwise.  cost_b is the sum of q and count_b the number of inliers:
 * integers, so no bit depends on the order of summation.
 * THE BEST TRIAL is, among the non-void trials with count >= 4, the one of smallest cost, ties to the smallest b.  No such trial,
 * or its count < min_inliers: extraction ends with n_spheres = p.  The diagnostics of that last round are still recorded
 * (best_trial = -1, cost and count 0 where no trial was eligible).
 * THE REFIT, on the best trial's inliers: g = rint((double)(row - p_0) * 2^(17 - e)) per component, the difference taken in fp32
 * (|g| <= 2^17); w = gx gx + gy gy + gz gz < 2^36, split as w = w_hi 2^18 + w_lo; seventeen signed 64-bit sums: n, S1[3] = sum g,
 * S2[6] = sum g_a g_b, sum w, sum g w_lo [3] and sum g w_hi [3] (each below 2^61 at 2^26 rows).  sum g w is recombined in 128 bits;
 * N = n S2 - S1 S1^T and h = n (sum g w) - S1 (sum w) exactly in 128 bits, each entry rounded once to double.  N a = h is solved by
 * the 3 x 3 Cholesky factorisation of pcreg_amd/csrc/sphere_fit.hpp, in the order written there: L00 = sqrt(N00); L10 = N01 / L00;
 * L20 = N02 / L00; L11 = sqrt(N11 - L10 L10); L21 = (N12 - L20 L10) / L11; L22 = sqrt((N22 - L20 L20) - L21 L21); y0 = h0 / L00;
 * y1 = (h1 - L10 y0) / L11; y2 = ((h2 - L20 y0) - L21 y1) / L22; a2 = y2 / L22; a1 = (y1 - L21 a2) / L11;
 * a0 = ((y0 - L10 a1) - L20 a2) / L00.  Then c_g = a / 2; beta = ((double)sum w - ((a0 S1x + a1 S1y) + a2 S1z)) / n;
 * R_g^2 = beta + ((c_gx c_gx + c_gy c_gy) + c_gz c_gz); centre = (double)p_0 + c_g 2^-(17 - e); R = sqrt(R_g^2) 2^-(17 - e).
 * The refit is USED iff every radicand of the factorisation is a finite number above 0, R_g^2 is a finite number above 0, centre
 * and R are finite and min_radius <= (float)R <= max_radius.  Otherwise the round's sphere is the trial's own ((double)cf,
 * (double)Rf) and refit_used[p] = 0.
 * THE FINAL CLASSIFICATION, over the alive rows: the scoring chain with (float)centre and (float)R.  The passing rows get label
 * p + 1 and leave the alive set; count_p is their number, Q_p the sum of their q, and
 * rmse_p = sqrt(((double)Q_p / count_p) * ((double)t2 * 2^-20)).
 * outputs -- labels [M] int32 by original row (0: no sphere); spheres [P][4] double ROW-major (cx, cy, cz, R); counts [P] int32;
 * rmse [P]; refit_used [P] int32; *n_spheres; the diagnostics best_trial [P] int32 (0-based), best_cost [P] int64, best_count [P]
 * int32, each may be NULL.  Entries of rounds that did not run are zero.  M = 0 writes *n_spheres = 0 and zeros.
 * Every sum across rows is an integer sum, so every output is the same bits on every call and on every stream, whatever the
 * workspace held before; under a caller's sample table (mapped with the rows) they are also the same bits for ANY ORDER OF THE
 * ROWS, labels following their rows.
 * PCREG_E_ARG, before anything runs: M >= 2^26; t or t2 zero, negative, subnormal, infinite or NaN; min_radius negative or NaN,
 * max_radius below min_radius or NaN; P, B or min_inliers out of range; model or n_spheres NULL; labels, spheres, counts, rmse or
 * refit_used NULL with M > 0; a sample table entry is never an error (the trial is void). */
int pcreg_model_fit_spheres_f32(pcreg_model* model, float max_distance, float min_radius, float max_radius, int max_spheres, int n_trials,
                                int min_inliers, uint64_t seed, const int32_t* samples /* [P][B][4] or NULL */, int32_t* labels /* [M] */,
                                double* spheres /* [P][4] */, int32_t* counts /* [P] */, double* rmse /* [P] */,
                                int32_t* refit_used /* [P] */, int32_t* n_spheres, int32_t* best_trial /* or NULL */,
                                int64_t* best_cost /* or NULL */, int32_t* best_count /* or NULL */);
/* The same without a handle (pcfitsphere(m, ...)): uploads and prepares the cloud for this call only.  Also PCREG_E_ARG:
 * M < 0, ldm < M, m NULL with M > 0. */
int pcreg_point_fit_spheres_f32(const float* m, int M, int ldm, float max_distance, float min_radius, float max_radius, int max_spheres,
                                int n_trials, int min_inliers, uint64_t seed, const int32_t* samples, int32_t* labels, double* spheres,
                                int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_spheres, int32_t* best_trial,
                                int64_t* best_cost, int32_t* best_count);

/* MSAC cylinder fitting and cylinder extraction over the rows of the model and their normals (MATLAB's pcfitcylinder(ptCloud,
 * maxDistance[, referenceVector, maxAngularDistance]) and the loop over it: fit, take the inliers out, fit again -- up to
 * max_cylinders times in one call; the instrument shafts, sleeves, trocars and rods of a scan).  THE CONTRACT of every tier (device,
 * host, MEX, Python) is THIS TEXT; MATLAB's bits are not knowable here.
 * inputs -- a prepared model of M fp32 rows, M < 2^26; max_distance t, t2 and s, min_radius and max_radius, max_cylinders P in
 * 1 .. 64, n_trials B in 1 .. 2^20, min_inliers >= 4 and seed under pcreg_model_fit_spheres_f32's rules; ref_vec (three doubles or
 * NULL) and max_angle (radians) under pcreg_model_fit_planes_f32's rules (finite, nonzero, 0 < max_angle <= pi / 2; max_angle is
 * not read without ref_vec): here they bound the AXIS; normals, host M x 3 fp32 column-major with leading dimension ldn >= M, or
 * NULL: then they are computed once in the call by pcreg_model_normals_f32's chain with k_normals (3 .. 32) and no viewpoint;
 * samples, int32 [P][B][2] or NULL: 1-BASED original rows at this tier.
 * ALIVE ROWS, THE QUANTISATION SCALE e and THE ROUND STRUCTURE are pcreg_model_fit_spheres_f32's: initially the rows whose three
 * coordinates are finite; e frexp's exponent of the largest axis extent of the finite rows; round p = 0 .. P - 1 over the alive set
 * A_p listed ascending by original row, nA rows.
 * USABLE NORMALS.  A row's normal is usable iff its three components are finite and each is at most 2 in magnitude.  The normals
 * are used as given, not renormalised.  A row with an unusable normal stays alive and may be an inlier (scoring reads no normal);
 * it is void as a sample and is left out of the axis sums.
 * Trial b has rows i_0, i_1: from samples[p][b][j] when the table is given, else i_j = A_p[h_j % nA] with
 * h_j = splitmix64(seed ^ splitmix64(((uint64)p * B + b) * 4 + j)), j = 0, 1, splitmix64 as at pcreg_model_fit_planes_f32.
 * THE TRIAL'S CYLINDER, from p_0, p_1 and their normals n_0, n_1 widened to double, every step ONE correctly rounded operation, no
 * contraction, in this order: W = n_0 x n_1, each component fl(fl(a b) - fl(c d)); L2 = (Wx Wx + Wy Wy) + Wz Wz; w = W / sqrt(L2),
 * three divisions; THE SIGN of w: with ref_vec, dot = (wx rx + wy ry) + wz rz, w is negated when dot < 0, and the trial is void
 * when |dot| / |ref| < cos(max_angle) (|ref| = sqrt((rx rx + ry ry) + rz rz)); without it the component of largest magnitude is
 * made positive, the first of equals in x, y, z order.  d = p_1 - p_0; m = d x n_1; num = (mx Wx + my Wy) + mz Wz with the
 * UNSIGNED W; s = num / L2; the axis point a = p_0 + s n_0 component by component, fl(p + fl(s n));
 * R = |s| sqrt((n_0x n_0x + n_0y n_0y) + n_0z n_0z); in fp32 af = (float)a, wf = (float)w, Rf = (float)R.
 * A trial is VOID if an index is out of range, a row is not alive, the two indices are equal, a normal is unusable, L2 is not a
 * finite number above 0, any of s, a, R, af, wf, Rf is not finite, Rf < min_radius or Rf > max_radius, or the angle test fails.
 * THE SIGN OF A NORMAL CHANGES NO BIT of any of this: negation is exact, W and num change sign together or not at all, and the
 * refit below takes only products of two components of one normal.
 * SCORING, per alive row, in fp32: d = row - af componentwise; the cross product with the axis cx = fmaf(d.y, wf.z, -(d.z * wf.y)),
 * cy = fmaf(d.z, wf.x, -(d.x * wf.z)), cz = fmaf(d.x, wf.y, -(d.y * wf.x)); c2 = fmaf(cz, cz, fmaf(cy, cy, cx * cx)); rho = the
 * correctly rounded fp32 square root of c2; r = rho - Rf; r2 = r * r; the row is an inlier iff r2 <= t2 (NaN never passes);
 * q = min(2^20, (int)rintf(r2 * s)) for an inlier, 2^20 otherwise.  cost_b is the sum of q and count_b the number of inliers.
 * THE BEST TRIAL and THE STOP RULE are pcreg_model_fit_spheres_f32's: among the non-void trials with count >= 4 the one of smallest
 * cost, ties to the smallest b; no such trial, or its count < min_inliers: extraction ends with n_cylinders = p, the diagnostics of
 * that last round still recorded (best_trial = -1, cost and count 0 where no trial was eligible).
 * THE REFIT, in two exact passes over the best trial's inliers (pcreg_amd/csrc/cylinder_fit.hpp, in the order written there).
 * PASS 1, THE AXIS, over the inliers with a usable normal: gn = rint((double)n_c 2^16) per component (|gn| <= 2^17); their number
 * n_n and the six sums of gn_a gn_b (xx xy xz yy yz zz) are signed 64-bit integers (each below 2^60 at 2^26 rows), each rounded
 * once to double; the library's cyclic Jacobi on that matrix, without centring (a cylinder's normals are perpendicular to its axis,
 * so the axis minimises sum (n . w)^2), in cylinder_fit.hpp's form: jacobi_sym3's sweeps, operation for operation, with the
 * cosine of a rotation c = 1 / sqrt(t t + 1) as two correctly rounded operations; the eigenvector column of the smallest diagonal
 * entry, ties to the lowest index; signed by the rule above (the angle test is not repeated).  The basis of the cross-section: e_k
 * the coordinate axis of w's smallest-magnitude component, first of equals; u = (w x e_k) / |w x e_k|; v = w x u.
 * PASS 2, THE CIRCLE, over all inliers: g = rint((double)(row - p_0) 2^(17 - e)) per component, the difference taken in fp32;
 * X = (gx ux + gy uy) + gz uz and Y likewise with v, in double without contraction; xi = rint(X), yi = rint(Y);
 * w2 = xi xi + yi yi < 2^36, split as w2 = w_hi 2^18 + w_lo; eleven signed 64-bit sums: n, sum xi, sum yi, sum xi xi, sum xi yi,
 * sum yi yi, sum w2, sum xi w_lo, sum xi w_hi, sum yi w_lo, sum yi w_hi.  N = n S2 - S1 S1^T (2 x 2) and
 * h = n (sum xi w2, sum yi w2) - S1 (sum w2) exactly in 128 bits, each entry rounded once to double.  N a = h by the 2 x 2
 * Cholesky factorisation: L00 = sqrt(N00); L10 = N01 / L00; L11 = sqrt(N11 - L10 L10); y0 = h0 / L00; y1 = (h1 - L10 y0) / L11;
 * a1 = y1 / L11; a0 = (y0 - L10 a1) / L00.  Then c2 = a / 2; beta = ((double)sum w2 - (a0 S1x + a1 S1y)) / n;
 * R_g^2 = beta + (c2x c2x + c2y c2y); centre = (double)p_0 + (c2x u + c2y v) 2^-(17 - e); R = sqrt(R_g^2) 2^-(17 - e).
 * The refit is USED iff n_n >= 2, Jacobi's output, every radicand and R_g^2 are finite and the radicands and R_g^2 above 0,
 * centre, w and R are finite and min_radius <= (float)R <= max_radius.  Otherwise the round's cylinder is the trial's own
 * ((double)af, (double)wf, (double)Rf) and refit_used[p] = 0.
 * THE FINAL CLASSIFICATION, over the alive rows: the scoring chain with (float)centre, (float)w and (float)R.  The passing rows get
 * label p + 1 and leave the alive set; count_p is their number, Q_p the sum of their q,
 * rmse_p = sqrt(((double)Q_p / count_p) * ((double)t2 * 2^-20)); h = fmaf(d.z, wf.z, fmaf(d.y, wf.y, d.x * wf.x)) of the passing
 * rows gives h_lo and h_hi, its minimum and maximum (NaN, like rmse, where count_p is 0).
 * outputs -- labels [M] int32 by original row (0: no cylinder); cylinders [P][7] double ROW-major (cx, cy, cz, wx, wy, wz, R);
 * extents [P][2] double ((double)h_lo, (double)h_hi): the end points of the axis are c + h_lo w and c + h_hi w; counts [P] int32;
 * rmse [P]; refit_used [P] int32; *n_cylinders; the diagnostics best_trial [P] int32 (0-based), best_cost [P] int64, best_count
 * [P] int32, each may be NULL.  Entries of rounds that did not run are zero.  M = 0 writes *n_cylinders = 0 and zeros.
 * Every sum across rows is an integer sum and min / max do not depend on order, so every output is the same bits on every call and
 * on every stream, whatever the workspace held before; under a caller's sample table (mapped with the rows) they are also the same
 * bits for ANY ORDER OF THE ROWS, labels following their rows.
 * PCREG_E_ARG, before anything runs: pcreg_model_fit_spheres_f32's cases (with cylinders, extents among the outputs that may not
 * be NULL with M > 0); ref_vec with a non-finite component or of zero length, or max_angle outside (0, pi / 2] with ref_vec given;
 * normals given with ldn < M, normals NULL with k_normals outside 3 .. 32; a sample table entry is never an error. */
int pcreg_model_fit_cylinders_f32(pcreg_model* model, float max_distance, float min_radius, float max_radius,
                                  const double* ref_vec /* 3 or NULL */, double max_angle, const float* normals /* M x 3 or NULL */,
                                  int ldn, int k_normals, int max_cylinders, int n_trials, int min_inliers, uint64_t seed,
                                  const int32_t* samples /* [P][B][2] or NULL */, int32_t* labels /* [M] */,
                                  double* cylinders /* [P][7] */, double* extents /* [P][2] */, int32_t* counts /* [P] */,
                                  double* rmse /* [P] */, int32_t* refit_used /* [P] */, int32_t* n_cylinders,
                                  int32_t* best_trial /* or NULL */, int64_t* best_cost /* or NULL */, int32_t* best_count /* or NULL */);
/* The same without a handle (pcfitcylinder(m, ...)): uploads and prepares the cloud for this call only.  Also PCREG_E_ARG:
 * M < 0, ldm < M, m NULL with M > 0. */
int pcreg_point_fit_cylinders_f32(const float* m, int M, int ldm, float max_distance, float min_radius, float max_radius,
                                  const double* ref_vec, double max_angle, const float* normals, int ldn, int k_normals, int max_cylinders,
                                  int n_trials, int min_inliers, uint64_t seed, const int32_t* samples, int32_t* labels, double* cylinders,
                                  double* extents, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_cylinders,
                                  int32_t* best_trial, int64_t* best_cost, int32_t* best_count);

/* [C, ia] = unique(A, 'rows') for n x 3 doubles (column-major, leading dimension ld >= n), the primitive of completeExperiment.m:439-443.
 * Rows are ordered lexicographically by column 1, 2, 3 as numbers (-0 == +0, -inf < finite < +inf); among equal rows the one with
 * the smallest index represents its run (MATLAB's default 'first').  ia [n]: the 1-based indices of the representatives in sorted
 * row order, *n_unique of them; C = A(ia, :) is the caller's gather and carries the representative's bits.  n = 0 is valid.  A row
 * that holds a NaN is refused with PCREG_E_ARG (MATLAB treats every NaN as distinct; the device order does not, see below).  The
 * result is a pure function of the input. */
int pcreg_unique_rows3(const double* A, int n, int ld, int32_t* ia, int* n_unique);
/* completeExperiment.m:440-443 on the stacked putative matches (pts1 / pts2 n x 3 column-major, leading dimension ld):
 *   [pts1, ia1] = unique(pts1, 'rows'); pts2 = pts2(ia1, :); [pts2, ia2] = unique(pts2, 'rows'); pts1 = pts1(ia2, :);
 * out1 / out2 (n x 3, leading dimension ldo >= n): the *n_out surviving pairs, sorted by the MODEL point (pts2) -- the order
 * ransac's sampler indexes; ia [n] or NULL: the composed 1-based index ia1(ia2) of every surviving pair in the input.  NaN rows
 * on either side: PCREG_E_ARG. */
int pcreg_aggregate_matches(const double* pts1, const double* pts2, int n, int ld, double* out1, double* out2, int ldo, int32_t* ia,
                            int* n_out);

/* Voxel-grid average downsampling (MATLAB's pcdownsample(pc, 'gridAverage', step); what made the _DS3 clouds of
 * completeExperimentFast.m:13).  THE CONTRACT of every tier (device, host, MEX, Python):
 * inputs -- pts: n x 3 fp32 column-major with leading dimension ld >= n; step: a double on the host, finite and > 0.
 * A ROW IS LIVE when its three coordinates are finite; a dead row belongs to no voxel.
 * THE GRID: all grid arithmetic is double on the widened fp32 values, IEEE subtraction and division, no contraction, no reciprocal.
 * lo[d] is the fp32 minimum of coordinate d over the live rows; the cell of a live row is
 * c[d] = (int64) floor(((double)x[d] - (double)lo[d]) / step).  A cloud whose largest cell index along an axis is >= 2^21 is refused.
 * A VOXEL is a distinct (c0, c1, c2).  The output rows are the voxels in ascending lexicographic order of (c0, c1, c2), column 0
 * most significant -- the order of unique(cells, 'rows').
 * THE MEAN, per voxel and per coordinate: a double sum of the widened coordinates of its rows, taken in ascending original row
 * order, starting from 0.0; divided by the count in double; rounded once to fp32.
 * outputs -- out: capacity n x 3 column-major with leading dimension ldo >= n, the first *n_out rows are written; count [n_out]
 * (or NULL): the rows of every voxel; label [n] (or NULL): the 1-based output row of every input row, 0 for a dead row (the hook by
 * which a caller averages colours or normals alongside); *n_out.  n = 0, or no live row, gives *n_out = 0 and writes nothing else.
 * The result is a pure function of (pts, step): no floating-point atomic; the order in which workgroups run, the stream and the
 * workspace's previous contents change no bit.
 * PCREG_E_ARG before anything runs: step not finite or <= 0, ld < n, ldo < n, n < 0, pts / out NULL with n > 0, n_out NULL; and,
 * after the device has found it, a cloud with 2^21 or more cells along an axis (nothing is written, *n_out = 0). */
int pcreg_downsample_grid_f32(const float* pts, int n, int ld, double step, float* out, int ldo, int32_t* count /* or NULL */,
                              int32_t* label /* or NULL */, int* n_out);

/* The normal-distributions transform: a cloud summarised once as one Gaussian per occupied voxel (the TABLE), and candidate
 * transforms of a query cloud refined against it by Gauss-Newton steps that need no nearest-row search -- the refinement MATLAB
 * offers as pcregisterndt, beside pcreg_model_refit_f32 (point to point) and pcreg_model_refit_plane_f32 (point to plane).
 * It is a STEP, not a registration policy: no convergence test, no line search, no multi-resolution schedule, and no claim of
 * pcregisterndt's bits.  The step is the Gauss-Newton, iteratively re-weighted form (each pair's Mahalanobis residual weighted
 * by its current likelihood), so the matrix is a sum of positive semi-definite terms and the point-to-plane solve applies.
 * THE CONTRACT of every tier (device, host, Python):
 * THE TABLE is built from (pts: n x 3 fp32 column-major with leading dimension ld >= n; step: a double, finite and > 0;
 * min_points: an int >= 3, 6 where a default is offered).
 * THE GRID is pcreg_downsample_grid_f32's, word for word: a row is live when its three coordinates are finite; lo[d] is the fp32
 * minimum of coordinate d over the live rows; the cell of a live row is c[d] = (int64) floor(((double)x[d] - (double)lo[d]) / step),
 * IEEE subtraction and division in double; a cloud whose largest cell index along an axis is >= 2^21 is refused (PCREG_E_ARG, no
 * handle); a voxel is a distinct (c0, c1, c2), and the voxels are taken in ascending lexicographic order, c0 most significant.
 * A GAUSSIAN, per voxel with count >= min_points, everything in double on the widened fp32 values, the members in ascending
 * original row order, no contraction:
 *   1. mean: per coordinate s = 0.0, s = s + x_i in order; mean = s / (double)count (pcreg_downsample_grid_f32's mean before its
 *      rounding to fp32).
 *   2. the six central second moments (xx xy xz yy yz zz): m_ab = 0.0; per member d = x_i - mean by component, m_ab = m_ab + d_a * d_b
 *      (a product, then an addition); cov_ab = m_ab / (double)(count - 1).
 *   3. eigenvalues l_0, l_1, l_2 and eigenvectors v_k of cov by the library's cyclic Jacobi in its exactly-rounded form (the one
 *      pcreg_model_fit_cylinders_f32 uses: at most 60 sweeps over (0,1), (0,2), (1,2), the cosine c = 1 / sqrt(t t + 1)).
 *   4. lmax = the largest l_k.  The voxel is VOID -- it holds no Gaussian -- when some l_k is not finite or lmax is not above 0 (all
 *      members equal).  Otherwise every l_k below 0.01 * lmax is raised to 0.01 * lmax, which bounds the condition number of C by
 *      100: a flat or a thin voxel keeps a finite pull along its degenerate axes.
 *   5. C = sum_k v_k v_k^T / l_k, per entry a <= b: C_ab = ((v_0a * v_0b) / l_0 + (v_1a * v_1b) / l_1) + (v_2a * v_2b) / l_2.
 * The table holds the Gaussian voxels only, ascending: cell (c0, c1, c2), count, mean[3], C[6] (xx xy xz yy yz zz).  The handle
 * also keeps lo, step and the ORIGIN o = 0.5f * lo + 0.5f * hi per coordinate in fp32, hi the fp32 maximum of the live rows
 * (pcreg_model_refit_plane_f32's rule).  n = 0 or no live row: a table without voxels; lo and o are 0.
 * THE STEP takes q (Q fp32 points column-major, ldq >= Q), B transforms of 16 doubles used as quickTF.m uses them, neighbors (1 or
 * 7) and outlier_ratio (a double in [0, 1), 0.55 where a default is offered).
 * THE MOVED POINT p of (transform b, query i) is scoring's TRANSFORMED QUERY (pcreg_model_score_f32: the chain in double, rounded
 * once to fp32).  The all-zero transform moves nothing: it has no pair.
 * THE PAIRS of a moved point: cell[d] = floor(((double)p[d] - (double)lo[d]) / step).  The CANDIDATE voxels are that cell
 * (neighbors = 1), or that cell followed by its six face neighbours in the order -x, +x, -y, +y, -z, +z (neighbors = 7).  A
 * candidate with a cell coordinate outside [0, 2^21) -- a non-finite coordinate of p leaves every candidate there -- is skipped,
 * and so is one that is not a Gaussian of the table.  Every remaining (point, voxel) is a PAIR; n_pairs[b] their number.
 * PER PAIR, in double, no contraction except where fma is written; p widened, o the origin, (mean, C) the voxel's;
 * cross(a, b) = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x), every component fl(fl(..) - fl(..)):
 *   x = p - mean;  u = p - o;  y = C x, y_a = (C_a0 x_0 + C_a1 x_1) + C_a2 x_2;  qq = (x_0 y_0 + x_1 y_1) + x_2 y_2;
 *   e = exp(-((d2 / 2) * qq)), the device's double exp;
 *   the Jacobian of p under a small rotation w about o and a translation t is J = (c_0, c_1, c_2, I), c_i = e_i x u, so that
 *   J_i . v = cross(u, v)_i for i < 3 and v_(i-3) for i >= 3:
 *   W_a = cross(u, row a of C), a = 0, 1, 2;   M_j = cross(u, (W_0[j], W_1[j], W_2[j])), j = 0, 1, 2;   gy = cross(u, y);
 *   a_ij = J_i^T C J_j:  M_j[i] for i <= j < 3;  W_(j-3)[i] for i < 3 <= j;  C_(i-3)(j-3) for 3 <= i <= j;
 *   h_i = J_i . y:  gy[i] for i < 3;  y_(i-3) for i >= 3.
 * THE 28 SUMS over the pairs in ascending (query, candidate) order:
 *   [0..20] A_ij = fma(e, a_ij, A_ij), i <= j, the upper triangle row-major;  [21..26] g_i = fma(e, h_i, g_i);  [27] sum_e = sum_e + e.
 * Their order is pcreg_model_refit_plane_f32's: a thread adds its 8 consecutive queries in order, the wave's butterfly follows,
 * the four waves of a chunk of 2048 queries in ascending order, the chunks in ascending order from 0.  No floating-point atomic.
 * d2, once per call on the host in double with res = step:  c1 = 10 (1 - outlier_ratio);  c2 = outlier_ratio / ((res res) res);
 *   d3 = -log(c2);  d1 = -log(c1 + c2) - d3;  d2 = -2 log((-log(c1 exp(-0.5) + c2) - d3) / d1).  outlier_ratio = 0 means d2 = 1: an
 *   unweighted Mahalanobis fit apart from the factor e.
 * THE FIT is pcreg_model_refit_plane_f32's, unchanged, on these 28 sums with n_pairs in n_plane's place (its 28th sum is reported,
 * not used): A x = -g by the scaled Cholesky, the Cayley rotation, T_step about o, T_out = T * T_step.  EMPTY by its rules:
 * empty[b] = 1 and 32 zeros for the all-zero T[b], n_pairs < 6, an A_ii not a finite number above 0, a pivot not above 2^-26, a
 * non-finite x or T_step.  n_pairs and sum_e are reported either way.  Q = 0 or a table without Gaussians: every transform is
 * empty, n_pairs 0 and sum_e 0.0.  B = 0: nothing is written.
 * Everything is a function of the inputs only: no floating-point atomic; the order in which workgroups run, the stream and the
 * workspace's previous contents change no bit (the step has no batching).
 * pcreg_ndt_create uploads the cloud, builds the table on the device and keeps only the table.  pcreg_ndt_size: the occupied voxels
 * and the Gaussians among them.  pcreg_ndt_get copies out, each pointer or NULL: cells [G][3] int32, counts [G], means [G][3],
 * C [G][6] row-major per Gaussian, lo [3], origin [3].  pcreg_ndt_refit_f32 runs `steps` >= 1 steps on the device with one upload
 * and one read, each step's T_out the next one's T; n_pairs, sum_e and empty describe the transform that went INTO the last step.
 * PCREG_E_ARG: n < 0, ld < n, pts NULL with n > 0, step not finite or <= 0, min_points < 3, a refused cloud; for the step Q < 0 or
 * above 4 Mi, B < 0, ldq < Q, neighbors not 1 or 7, outlier_ratio outside [0, 1) or NaN, steps < 1, a NULL handle, a NULL q with
 * Q > 0, a NULL T or output with B > 0. */
typedef struct pcreg_ndt pcreg_ndt;
int pcreg_ndt_create(const float* pts, int n, int ld, double step, int min_points, pcreg_ndt** ndt);
int pcreg_ndt_destroy(pcreg_ndt* ndt);
int pcreg_ndt_size(const pcreg_ndt* ndt, int* n_voxels, int* n_gaussians);
int pcreg_ndt_get(const pcreg_ndt* ndt, int32_t* cells, int32_t* counts, double* means, double* C, float* lo, float* origin);
int pcreg_ndt_refit_f32(pcreg_ndt* ndt, const float* q, int Q, int ldq, const double* T /* host [B][16] */, int B, int neighbors,
                        double outlier_ratio, int steps, double* T_out /* [B][16] */, int32_t* n_pairs, double* sum_e, int32_t* empty);

/* getLocalPoints.m:8-35  [pts_sphere, dists] = getLocalPoints(pts, R, c, min_points, max_points): the points of the cloud strictly
 * inside the open box AND the open ball of radius R around c, RELATIVE to c, in the cloud's order; [] when the box holds fewer
 * than min_points (:17) or the ball fewer than min_points / more than max_points (:31).  pts: N x 3 column-major (ld >= N).
 * pts_sphere: capacity N x 3, written as n_out x 3 column-major with leading dimension *n_out; dists (or NULL): capacity N;
 * *n_out = rows returned, 0 for MATLAB's [].  single_mode as in pcreg_spatial_histogram_descriptors_mixed (0 double; 1 keypoint
 * single, 2 only the cloud single: MATLAB's element-wise single arithmetic, values passed exactly widened, outputs are those single
 * values widened). */
int pcreg_get_local_points(const double* pts, int N, int ld, double R, const double c[3], double min_points, double max_points,
                           int single_mode, double* pts_sphere, double* dists, int* n_out);

/* getMatches for S row subsets of ONE model descriptor set in one call: segment s = getMatches(descSurface,
 * descModel(rows_s + 1, :), par) with rows_s = seg_rows[seg_off[s] .. seg_off[s+1]) (0-based, ascending, HOST arrays) -- the
 * per-sphere calls that completeExperimentFast.m:131-149 runs under parfor.  Descriptors as MATLAB holds them (n x D
 * column-major doubles, ld >= n).  pairs_all [S][Q][2]: segment s's pairs start at pairs_all + s*Q*2, n_pairs[s] of them,
 * 1-based, the model index counting within the segment like the per-sphere call's.  Same pairs as S calls of
 * pcreg_get_matches (the powered columns and the approximate scores are computed once for all segments).
 * Metric SAD; S <= 65535. */
int pcreg_get_matches_segmented(const double* descSurface, int Q, int ldS, const double* descModel, int VM, int ldM, int D,
                                const int32_t* seg_rows, const int32_t* seg_off, int S, const pcreg_match_opts* par,
                                uint32_t* pairs_all, int32_t* n_pairs);

/* getMatches.m:51  matchFeatures(features1, features2, 'Method',..,'MatchThreshold',..,
 * 'MaxRatio',..,'Metric',..,'Unique',..) on Q x D / M x D double features (exact
 * search; 'Approximate' is answered exactly).  Only the matchFeatures fields of opts
 * are used.  pairs as above; metric (optional) receives matchMetric. */
int pcreg_match_features(const double* f1, int Q, int ld1, const double* f2, int M, int ld2, int D,
                         const pcreg_match_opts* opts, uint32_t* pairs, double* metric, int* P);

/* getMatches.m:1  matches = getMatches(descSurface, descModel, par): append the
 * constant column (:22-26), element-wise power (:35-37), then matchFeatures (:51-56). */
int pcreg_get_matches(const double* descSurface, int Q, int ldS, const double* descModel, int M,
                      int ldM, int D, const pcreg_match_opts* par, uint32_t* pairs, double* metric,
                      int* P);

/* One surface set against MANY row subsets of one model set -- the loop of completeExperimentFast.m:101-150
 *     descCur = descModel(mask, :);  matches = getMatches(descSurface, descCur, par);        (:121-149, hundreds of spheres)
 * with both sets uploaded ONCE.  pcreg_desc_set_create copies an n x D column-major double matrix (ld >= n) to the device;
 * pcreg_get_matches_on_sets(surface, model, rows, n_rows, ...) is pcreg_get_matches(descSurface, descModel(rows + 1, :), ...)
 * -- the same kernels on the same values, the same pairs bit for bit -- with rows = the 0-based ascending row numbers of the
 * subset (NULL: the whole model set).  A set belongs to the device that was current when it was created. */
typedef struct pcreg_desc_set pcreg_desc_set;
int pcreg_desc_set_create(const double* desc, int n, int ld, int D, pcreg_desc_set** set);
int pcreg_desc_set_destroy(pcreg_desc_set* set);
int pcreg_desc_set_size(const pcreg_desc_set* set, int* n, int* D);
int pcreg_get_matches_on_sets(const pcreg_desc_set* surface, const pcreg_desc_set* model, const int32_t* model_rows, int n_rows,
                              const pcreg_match_opts* par, uint32_t* pairs, double* metric, int* P);
/* pcreg_get_matches_segmented on uploaded sets: ALL spheres of the loop above in one call, nothing but the row lists going up and
 * the pairs coming down (the 470 MB of a 60 000 x 980 model set take longer to upload than the whole sweep takes to match).
 * Arguments and results as pcreg_get_matches_segmented.  From their first segmented call on the sets keep a row-major copy, and
 * the model set its powered rows for the options of the last call (so a set then holds up to three times its n x D doubles). */
int pcreg_get_matches_segmented_on_sets(const pcreg_desc_set* surface, const pcreg_desc_set* model, const int32_t* seg_rows,
                                        const int32_t* seg_off, int S, const pcreg_match_opts* par, uint32_t* pairs_all, int32_t* n_pairs);

/* The sphere sweep of completeExperimentFast.m:46-224 at the host tier, in two calls (the first fixes the sizes of the second).
 *
 * pcreg_sphere_counts: counts[i] = #{ rows of featModel with norm(row - centres(i, :)) < R }  (:52-64; featModel VM x 3, centres
 * S x 3, both column-major doubles).  The caller keeps the spheres with min_pts <= counts <= max_pts (:61-64).
 *
 * pcreg_sphere_sweep, for the S spheres kept (centres S x 3, num_desc[i] = their counts): per sphere
 *     mask = getDescriptorMask(featModel, c_i, R_desc);  matches = getMatches(descSurface, descModel(mask, :), par)      (:109-149)
 * on resident descriptor sets (pcreg_desc_set_create), then for every sphere with more than putative_thresh matches (:166-184)
 *     [T, ~, numSuccess, maxInliers] = ransac(featSurface(matches(:,1), :), featCur(matches(:,2), :), coef, ...)          (:201-216)
 * with the built-in sampler seeded coef->seed + t for the t-th such sphere -- one launch chain, two synchronisations.
 * Outputs: model_rows: the spheres' 0-based ascending row lists back to back (sum of num_desc entries); pairs_all [S][Q][2]
 * (Q = rows of the surface set) and n_pairs[S] as pcreg_get_matches_segmented; trial[t], t < *n_trials: the 0-based spheres
 * that were registered, in ascending order; T (16 per trial, column-major 4 x 4, zeros where failed[t]), num_success, max_inliers,
 * failed: capacity S each.  Metric SAD; coef->minPtNum = 3. */
int pcreg_sphere_counts(const double* featModel, int VM, int ldM, const double* centres, int S, int ldC, double R, int32_t* counts);
int pcreg_sphere_sweep(const pcreg_desc_set* surface, const pcreg_desc_set* model, const double* featSurface, int ldS, const double* featModel, int ldM,
                       const double* centres, int S, int ldC, const int32_t* num_desc, double R_desc, const pcreg_match_opts* par, int putative_thresh,
                       const pcreg_ransac_opts* coef, int32_t* model_rows, uint32_t* pairs_all, int32_t* n_pairs, int32_t* trial, int* n_trials,
                       double* T, int32_t* num_success, int32_t* max_inliers, int32_t* failed);

/* The same with ONE model and many surfaces (completeExperimentFast.m runs once per surface crop): what the sweep makes of the model
 * alone -- the spheres' row lists and gathered keypoints, the model set restricted to the union of those rows, its powered rows per
 * set of getMatches options -- lives in a handle.  pcreg_sphere_model_create takes pcreg_sphere_sweep's model-side arguments and
 * returns the row lists (model_rows: sum of num_desc entries, 0-based); pcreg_sphere_sweep_on_model takes the surface-side ones and
 * returns pcreg_sphere_sweep's other outputs (the same values).  The handle holds copies: the model set may be destroyed first. */
typedef struct pcreg_sphere_model pcreg_sphere_model;
int pcreg_sphere_model_create(const pcreg_desc_set* model, const double* featModel, int ldM, const double* centres, int S, int ldC,
                              const int32_t* num_desc, double R_desc, int32_t* model_rows, pcreg_sphere_model** out);
int pcreg_sphere_model_destroy(pcreg_sphere_model* m);
int pcreg_sphere_sweep_on_model(pcreg_sphere_model* m, const pcreg_desc_set* surface, const double* featSurface, int ldS, const pcreg_match_opts* par,
                                int putative_thresh, const pcreg_ransac_opts* coef, uint32_t* pairs_all, int32_t* n_pairs, int32_t* trial, int* n_trials,
                                double* T, int32_t* num_success, int32_t* max_inliers, int32_t* failed);

/* AlignPoints_KNN.m:1  [pts_aligned, coeff_unambig, c] = AlignPoints_KNN(pts, C1, C2).
 * aligned: n x 3 (ld n); coeff: column-major 3x3; c: 3. */
int pcreg_align_points_knn(const double* pts, int n, int ld, int C1, int C2,
                           double* aligned, double coeff[9], double c[3]);

/* B supports in one launch (the per-keypoint loop of
 * getSpacialHistogramDescriptors.m:64-145 calls the same LRF per support):
 * support b owns rows [offsets[b], offsets[b+1]) of pts / aligned; coeff 9*B, c 3*B;
 * status[b] = 0 ok, 1 = support too small (n < 2), 2 = the support is larger than the launch holds (never from this
 * entry, which sizes the launch itself: see pcreg_dev_align_points_knn_batched).  A support may hold at most 8192 points
 * (it is kept in the registers of one workgroup); larger -> PCREG_E_ARG.  The reference's supports hold 500 ... 6000
 * (completeExperimentFast.m:300-302). */
int pcreg_align_points_knn_batched(const double* pts, int total, int ld, const int32_t* offsets,
                                   int B, int C1, int C2, double* aligned, double* coeff,
                                   double* c, int32_t* status);

/* The same for a `single` cloud: the outputs keep the class (AlignPoints_KNN.m:17,59: everything derives from pts).  Inputs
 * are widened to double exactly, the double kernel runs, outputs are rounded once to float.  MATLAB's own single
 * arithmetic may decide a borderline K-th-nearest / sign vote differently: documented in INTEGRATION.md, not reproduced. */
int pcreg_align_points_knn_f32(const float* pts, int n, int ld, int C1, int C2,
                               float* aligned, float coeff[9], float c[3]);

/* `options` of getSpacialHistogramDescriptors.m:18-27 (completeExperimentFast.m:299-304). */
typedef struct pcreg_desc_opts {
    int32_t min_pts;       /* options.min_pts                                            */
    int32_t max_pts;       /* options.max_pts (INT32_MAX for inf)                        */
    double  R;             /* options.R: support radius                                  */
    double  thVar[2];      /* options.thVar: eigenvalue-ratio rejection thresholds       */
    double  k;             /* options.k: fraction of nearest points used for the LRF;
                              >= 1 means 'all'                                           */
    int32_t ALIGN_POINTS;  /* options.ALIGN_POINTS                                       */
} pcreg_desc_opts;
#define PCREG_DESC_LEN 980   /* NUM_R*NUM_THETA*NUM_PHI = 10*7*14, getSpacialHistogramDescriptors.m:38-40 */

/* getSpacialHistogramDescriptors.m:2  [feat, desc] = getSpacialHistogramDescriptors(pts,
 * sample_pts, options) (with getLocalPoints.m and histcn.m folded in).  pts: P x 3,
 * sample_pts: S x 3 (column-major).  Outputs are ROW-major with capacity S rows:
 * feat [V][3], desc [V][980] (counts, r fastest / then theta / then phi, i.e. MATLAB's
 * reshape(counts,[],1)); *V = number of surviving keypoints, in input order.
 * The O(S*P) brute-force radius search of the reference is replaced by a uniform grid.
 * Limits: a support of more than 8191 points (possible only with options.max_pts > 8190;
 * it lives in LDS) and a cloud of 2^28 points or more (the kernel addresses the sorted
 * cloud with 32-bit byte offsets) are refused with PCREG_E_ARG. */
int pcreg_spatial_histogram_descriptors(const double* pts, int P, int ld, const double* sample_pts, int S, int lds,
                                        const pcreg_desc_opts* options, double* feat, double* desc, int* V);

/* The same for `single` data (clouds from pcread are single: upsampleMesh.m:21, GetPointcloudFromModel.m:269, fed on by
 * completeExperimentFast.m:291,309).  feat / desc are DOUBLE whatever the input classes: the reference preallocates them
 * with nan(...) and assigns into them (getSpacialHistogramDescriptors.m:61-62).  When either input is single, MATLAB runs
 * getLocalPoints.m:8-31 in single; what is element-wise there is reproduced in fp32 exactly as written -- the open box test,
 * pts_cube - c, sqrt(x^2 + y^2 + z^2), dists < R -- i.e. WHICH keypoints survive and which points form a support, and the
 * support's coordinates are MATLAB's single pts_rel values.  mean / pca / the histogram run in double on those values
 * (INTEGRATION.md says what is not knowable).  _mixed takes each input in its own class: *_is_single != 0 -> const float*,
 * else const double*. */
int pcreg_spatial_histogram_descriptors_f32(const float* pts, int P, int ld, const float* sample_pts, int S, int lds,
                                            const pcreg_desc_opts* options, double* feat, double* desc, int* V);
int pcreg_spatial_histogram_descriptors_mixed(const void* pts, int pts_is_single, int P, int ld, const void* sample_pts,
                                              int sample_is_single, int S, int lds, const pcreg_desc_opts* options,
                                              double* feat, double* desc, int* V);

/* The final stage of completeExperimentFast.m:280-394 at the host tier, in two calls (the first fixes the keypoint draw of the
 * second, as pcreg_sphere_counts does for pcreg_sphere_sweep).  K clusters: locs K x 3 column-major (locCur of :283-288), T [K][16]:
 * the transforms that MOVE the surface, T_k = invertTF(transCur_k) (:291) computed by the caller in its own arithmetic, K
 * column-major 4 x 4 matrices back to back (MATLAB's 4 x 4 x K).
 *
 * pcreg_final_stage_limits: limits [K][6] = (xmin xmax ymin ymax zmin zmax) of pts_tform_k = quickTF(pts, T_k) as the library moves
 * the surface -- bit for bit the copies pcreg_final_stage describes.  pcRandomUniformSamples (:418-432) draws from MATLAB's rand
 * stream, so the keypoints stay the caller's; their count and box come from these limits.
 *
 * pcreg_final_stage: per cluster k (:291-353)
 *     pts_tform = quickTF(pts, T_k);  [feat, desc] = getSpacialHistogramDescriptors(pts_tform, keypoints_k, desc_opts with ALIGN_POINTS = 0)
 *     mask = getDescriptorMask(featModel_noLRF, locs(k,:), R_desc);  matches = getMatches(desc, descModel_noLRF(mask, :), par)
 * then (:357-394) the matches closer than maxDist, precision(k) = numel(close) / size(matches, 1) * 100 (NaN for 0 / 0), the best
 * cluster by MATLAB's max (first maximum, NaN skipped, the first cluster when all are NaN), T_refine = estimateTransform over its
 * close matches, pts_final = quickTF(pts_tform_best, invertTF(T_refine)) (pts_tform_best itself when T_refine is []).
 * model: the no-LRF model descriptors (pcreg_desc_set, D = 980); featModel VM x 3 column-major; pts N x 3 (ld >= N); keypoints
 * kp_off[K] x 3 column-major (ld = kp_off[K]), cluster k's rows [kp_off[k], kp_off[k+1]).
 * Outputs: num_keypoints (V_k, the surviving keypoints), num_desc (model keypoints in the sphere), num_matches, num_close,
 * precision: K each; *best 0-based; T_refine column-major 4 x 4 (zeros with *refine_empty = 1 for MATLAB's []); pts_final N x 3
 * (ld N); pairs (or NULL): capacity kp_off[K] rows of [surface, model] 1-based uint32 pairs, cluster k's num_matches[k] pairs at
 * row kp_off[k] (the model index counting inside the sphere, like matches of :344).  Metric SAD.
 * Enqueue order: upload, every moved copy in one launch, per cluster the descriptor chain, the spheres' counts, ONE read of the
 * sizes, the spheres' row lists, per cluster the row gather and getMatches, the close-match / refine kernel (one wave per cluster),
 * the pick / final-surface kernel, ONE read of the results.  (getMatches with Unique on more than ~4500 keypoints synchronises once
 * per cluster to size its back-search, as pcreg_dev_get_matches documents.)
 * Memory: a cluster's fp64 descriptors take 7.84 KB per keypoint drawn.  Up to 4 GB of them the clusters run as one batch; above,
 * they run in batches of consecutive clusters whose descriptors fit 4 GB together (a larger single cluster runs alone), reusing
 * the buffers: one more synchronisation (the batch's sizes) per batch, identical results.
 * Every size is checked before anything is enqueued: K >= 1, kp_off[0] = 0 and non-decreasing, N >= 1, ld >= N, the set's D = 980;
 * a support above the LDS capacity is refused with PCREG_E_ARG. */
int pcreg_final_stage_limits(const double* pts, int N, int ld, const double* T, int K, double* limits);
int pcreg_final_stage(const pcreg_desc_set* model_noLRF, const double* featModel_noLRF, int ldM, const double* pts, int N, int ld,
                      const double* locs, const double* T, int K, const double* keypoints, const int32_t* kp_off,
                      const pcreg_desc_opts* desc_opts, const pcreg_match_opts* par, double R_desc, double maxDist,
                      int32_t* num_keypoints, int32_t* num_desc, int32_t* num_matches, int32_t* num_close, double* precision,
                      int32_t* best, double T_refine[16], int32_t* refine_empty, double* pts_final, uint32_t* pairs);

/* ---- device tier ------------------------------------------------------------------
 * All pointers are device memory on the current device; `stream` is a hipStream_t.
 * Workspaces are caller-owned device buffers; query the size first. */

/* Two nearest model points per query for one model shard.  idx_base is added to the
 * reported indices (global row of the shard's first point).  idx [Q][2] int32, dist
 * [Q][2] float. */
size_t pcreg_dev_knn2_points_f32_workspace(int Q, int M);
int pcreg_dev_knn2_points_f32(const float* q, int Q, int ldq, const float* m, int M, int ldm,
                              int32_t idx_base, int32_t* idx, float* dist,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- a PREPARED MODEL: one model, many surfaces (completeExperimentFast.m:131-149 matches every candidate sphere,
 * :201-216 registers every promising one, against the same model; BASELINE cfg 5: 64 crops vs one CT model) ----------
 * Everything that depends on the model alone -- its bounding box, the tiles of matrix-core operands, the model-wide
 * seeding grid -- is computed once; a search against the handle is four launches, the match stage one.
 * pcreg_dev_model_create enqueues the preparation on `stream` and returns at once; the model's points (`m`, n x 3
 * column-major, ldm) are NOT copied and must stay valid and unchanged while the handle lives.  A handle may be used
 * from several streams at once as long as each call has its own workspace.  Reported rows are idx_base + local row. */
typedef struct pcreg_dev_model pcreg_dev_model;
int pcreg_dev_model_create(const float* m, int M, int ldm, void* stream, pcreg_dev_model** model);
int pcreg_dev_model_destroy(pcreg_dev_model* model);
/* Top-2 of every query over the prepared model (pcreg_dev_knn2_points_f32's contract and bits).  The workspace also
 * receives a uniform grid over the queries, which pcreg_dev_model_match_f32 / _match_table_f32 need for Unique: pass
 * the SAME workspace to them, with no other search on it in between. */
/* Test hooks: copy what a prepared model holds into device buffers of the caller, enqueued on `stream` (any pointer may be
 * NULL): perm [M] (perm[sorted row] = original row), the fp32 sorted copy [3][M] (ld = M), the tile boxes [n_tiles][6]
 * (lo x, y, z, hi x, y, z of every tile of 512 sorted rows) -- and the raw 24-word preparation record to the HOST (waits for
 * the stream; 20 words used, ints as their bit patterns; zeros for M = 0).  pcreg_debug_search_export copies the query order qperm [Q]
 * (slot -> query) and the seed distances dk [Q] of the last search on `workspace` (sized for Q, M). */
int pcreg_debug_dev_model_export(const pcreg_dev_model* model, int32_t* perm, float* sorted_soa, float* tile_box, float prep[24],
                                 void* stream);
int pcreg_debug_search_export(const void* workspace, size_t workspace_bytes, int Q, int M, int32_t* qperm, float* dk, void* stream);
size_t pcreg_dev_model_search_workspace(int Q, int M);
int pcreg_dev_model_search_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, int32_t idx_base,
                               int32_t* idx, float* dist, void* workspace, size_t workspace_bytes, void* stream);
/* knnsearch(model, q, 'K', k) on the device: pcreg_model_knn_f32's contract, reported rows idx_base + local row (-1 past
 * M).  Q <= 4 Mi per call; the workspace (O(Q) bytes, any k) is sized by pcreg_dev_model_knn_workspace.  Nothing is
 * certified and there is no fallback: every distance is the fp32 chain itself, tiles are skipped by DESIGN 4.1's rule
 * with the k-th-neighbour bound.  A handle may serve several streams at once, each call with its own workspace. */
size_t pcreg_dev_model_knn_workspace(int Q, int M, int k);
int pcreg_dev_model_knn_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, int k, int32_t idx_base, int32_t* idx,
                            float* dist, void* workspace, size_t workspace_bytes, void* stream);
/* rangesearch(model, q, r) on the device in two calls (count + scan, then fill + order): pcreg_model_range_f32's contract with
 * r2 = r^2.  Count: counts [Q] and seg_off [Q + 1], the exclusive running sums in 64 bits (seg_off[Q] = total rows).  Fill: idx
 * / dist [capacity], query i's rows at seg_off[i] .. seg_off[i + 1] in (distance, row) order, idx = idx_base + 0-based row.
 * The fill never writes outside [seg_off[i], seg_off[i + 1]) intersected with [0, capacity), whatever seg_off holds: a seg_off
 * made with a smaller radius, or a capacity below the total, truncates segments (which rows remain is then unspecified).
 * Each call forms its own query order, so the caller may read the total, allocate, and fill later, on any stream; nothing
 * synchronises.  Q <= 4 Mi per call.  One workspace size serves both calls: 147 712 + 3 * roundup(4 * max(Q, 1), 256) bytes,
 * i.e. 12 bytes per query, whatever M, r2 and the size of the result.  Tiles are skipped by DESIGN 4.1's rule with the
 * radius as the bound.  A handle may serve several streams at once, each call with its own workspace. */
size_t pcreg_dev_model_range_workspace(int Q, int M);
int pcreg_dev_model_range_count_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, float r2,
                                    int32_t* counts, int64_t* seg_off, void* workspace, size_t workspace_bytes, void* stream);
int pcreg_dev_model_range_fill_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, float r2, int32_t idx_base,
                                   const int64_t* seg_off, int64_t capacity, int32_t* idx, float* dist,
                                   void* workspace, size_t workspace_bytes, void* stream);
/* pcreg_model_score_f32's contract on the device: q, T_dev [B][16], n_close [B], sum_d2 [B] and idx / dist [B][Q]
 * (or NULL) are device pointers.  Nothing synchronises; no workgroup waits for another.  The B * Q transformed queries go
 * through the walk in batches of whole transforms of at most 4 Mi query slots, each batch in ONE spatial order; tiles are
 * skipped by DESIGN 4.1's rule with the radius as the bound.  No result depends on the batching.  Workspace, with
 * nb = max(1, min(B, floor(4 Mi / max(Q, 1)))), S = max(nb * Q, 1) and P = nb * max(ceil(Q / 2048), 1):
 * 131 328 + roundup(12 S, 256) + 2 roundup(4 S, 256) + roundup(8 P, 256) + roundup(4 P, 256) bytes, O(min(B Q, 4 Mi)) whatever
 * M, r2 and the result.  A workspace shorter than that is PCREG_E_ARG too.  A handle may serve several streams at once, each
 * call with its own workspace. */
size_t pcreg_dev_model_score_workspace(int Q, int B, int M);
int pcreg_dev_model_score_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq,
                              const double* T_dev /* [B][16] on the device */, int B, float r2,
                              int32_t* n_close /* [B] */, double* sum_d2 /* [B] */,
                              int32_t* idx /* [B][Q] or NULL */, float* dist /* [B][Q] or NULL */,
                              void* workspace, size_t workspace_bytes, void* stream);
/* ONE step of pcreg_model_refit_f32's contract on the device: q, T_dev [B][16], T_out [B][16], T_step [B][16] (or
 * NULL: not wanted), n_close [B], sum_d2 [B] and empty [B] are device pointers.  T_out may not alias T_dev (a caller that
 * repeats the step alternates two blocks).  Nothing synchronises; no workgroup waits for another.  The chain is
 * pcreg_dev_model_score_f32's -- the same batches of whole transforms, the same walk and culling rule, with the winning row's
 * coordinates kept per query slot -- followed per batch by the moments per (transform, chunk of 2048 queries) and the fit per
 * transform.  No result depends on the batching.  Workspace, with nb, S and P as for pcreg_dev_model_score_workspace: that
 * layout followed by the winning rows' coordinates and the chunk moments,
 * 131 328 + 2 roundup(12 S, 256) + 2 roundup(4 S, 256) + roundup(8 P, 256) + roundup(4 P, 256) + roundup(216 P, 256) bytes.  A
 * workspace shorter than that is PCREG_E_ARG too.  A handle may serve several streams at once, each call with its own workspace.
 * The debug keys "score_batch_slots" and "knn_nocull" act on this chain as on scoring's. */
size_t pcreg_dev_model_refit_workspace(int Q, int B, int M);
int pcreg_dev_model_refit_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq,
                              const double* T_dev /* [B][16] on the device */, int B, float r2,
                              double* T_out /* [B][16] */, double* T_step /* [B][16] or NULL */,
                              int32_t* n_close /* [B] */, double* sum_d2 /* [B] */, int32_t* empty /* [B] */,
                              void* workspace, size_t workspace_bytes, void* stream);
/* ONE step of pcreg_model_refit_plane_f32's contract on the device: q, T_dev [B][16], normals_dev [3 * ldn],
 * T_out [B][16], T_step [B][16] (or NULL: not wanted), n_close, sum_d2, n_plane, sum_res2 and empty [B] are device pointers.
 * normals_dev is what pcreg_dev_model_normals_f32 writes and may not be NULL; T_out may not alias T_dev.  Nothing synchronises;
 * no workgroup waits for another.  The chain is pcreg_dev_model_refit_f32's up to the walk, which also keeps the winning ORIGINAL
 * row per query slot; then per batch the 28 sums per (transform, chunk of 2048 queries), the normals gathered by that row, and
 * the fit per transform.  No result depends on the batching.  Workspace, with nb, S and P as for
 * pcreg_dev_model_score_workspace: the refit's layout followed by the winning row per slot and the chunk plane counts, with 28
 * instead of 27 chunk sums,
 * 131 328 + 2 roundup(12 S, 256) + 3 roundup(4 S, 256) + roundup(8 P, 256) + 2 roundup(4 P, 256) + roundup(224 P, 256) bytes.  A
 * workspace shorter than that is PCREG_E_ARG too, and so are ldn < M and normals_dev NULL.  A handle may serve several streams at
 * once, each call with its own workspace.  The debug keys "score_batch_slots" and "knn_nocull" act on this chain as on scoring's. */
size_t pcreg_dev_model_refit_plane_workspace(int Q, int B, int M);
int pcreg_dev_model_refit_plane_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq,
                                    const double* T_dev /* [B][16] on the device */, int B, float r2,
                                    const float* normals_dev /* [3][ldn] */, int ldn,
                                    double* T_out /* [B][16] */, double* T_step /* [B][16] or NULL */,
                                    int32_t* n_close /* [B] */, double* sum_d2 /* [B] */, int32_t* n_plane /* [B] */,
                                    double* sum_res2 /* [B] */, int32_t* empty /* [B] */,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* ONE step of pcreg_model_refit_gicp_f32's contract on the device: pcreg_dev_model_refit_plane_f32's arguments and
 * rules, with qnormals_dev [3 * ldnq] -- what pcreg_dev_model_normals_f32 writes for a model made of the queries -- and epsilon
 * added, and n_pairs in n_plane's place.  The chain is the plane refit's with the plane-to-plane sums in the point-to-plane ones'
 * place; the workspace has the plane refit's size and layout.  PCREG_E_ARG also for ldnq < Q, qnormals_dev NULL with Q > 0, and
 * epsilon NaN or outside (0, 1]. */
size_t pcreg_dev_model_refit_gicp_workspace(int Q, int B, int M);
int pcreg_dev_model_refit_gicp_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq,
                                   const double* T_dev /* [B][16] on the device */, int B, float r2,
                                   const float* normals_dev /* [3][ldn] */, int ldn,
                                   const float* qnormals_dev /* [3][ldnq] */, int ldnq, double epsilon,
                                   double* T_out /* [B][16] */, double* T_step /* [B][16] or NULL */,
                                   int32_t* n_close /* [B] */, double* sum_d2 /* [B] */, int32_t* n_pairs /* [B] */,
                                   double* sum_res2 /* [B] */, int32_t* empty /* [B] */,
                                   void* workspace, size_t workspace_bytes, void* stream);
/* ONE step of the trimmed contract (pcreg_model_score_trimmed_f32) on the device: each entry takes its untrimmed
 * twin's arguments and rules with keep_ratio after r2 and n_within / d2_cut [B] (device pointers, either may be NULL) at the end.
 * Between the walk and the sums a trim pass selects each transform's keep-th smallest d by four 8-bit histogram passes and
 * turns the other pairs into misses; no host read happens.  THE WORKSPACE IS THE UNTRIMMED TWIN'S, pcreg_dev_model_X_workspace(Q, B,
 * M) bytes and not one more: the pass keeps its counters in blocks of that layout that are dead between the walk and the sums.
 * PCREG_E_ARG also for keep_ratio NaN, <= 0 or > 1. */
int pcreg_dev_model_score_trimmed_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq,
                                      const double* T_dev /* [B][16] on the device */, int B, float r2, double keep_ratio,
                                      int32_t* n_close /* [B] */, double* sum_d2 /* [B] */, int32_t* idx /* [B][Q] or NULL */,
                                      float* dist /* [B][Q] or NULL */, void* workspace, size_t workspace_bytes, void* stream,
                                      int32_t* n_within /* [B] or NULL */, float* d2_cut /* [B] or NULL */);
int pcreg_dev_model_refit_trimmed_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq,
                                      const double* T_dev /* [B][16] on the device */, int B, float r2, double keep_ratio,
                                      double* T_out /* [B][16] */, double* T_step /* [B][16] or NULL */, int32_t* n_close /* [B] */,
                                      double* sum_d2 /* [B] */, int32_t* empty /* [B] */, void* workspace, size_t workspace_bytes,
                                      void* stream, int32_t* n_within /* [B] or NULL */, float* d2_cut /* [B] or NULL */);
int pcreg_dev_model_refit_plane_trimmed_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq,
                                            const double* T_dev /* [B][16] on the device */, int B, float r2, double keep_ratio,
                                            const float* normals_dev /* [3][ldn] */, int ldn, double* T_out /* [B][16] */,
                                            double* T_step /* [B][16] or NULL */, int32_t* n_close /* [B] */, double* sum_d2 /* [B] */,
                                            int32_t* n_plane /* [B] */, double* sum_res2 /* [B] */, int32_t* empty /* [B] */,
                                            void* workspace, size_t workspace_bytes, void* stream,
                                            int32_t* n_within /* [B] or NULL */, float* d2_cut /* [B] or NULL */);
int pcreg_dev_model_refit_gicp_trimmed_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq,
                                           const double* T_dev /* [B][16] on the device */, int B, float r2, double keep_ratio,
                                           const float* normals_dev /* [3][ldn] */, int ldn,
                                           const float* qnormals_dev /* [3][ldnq] */, int ldnq, double epsilon,
                                           double* T_out /* [B][16] */, double* T_step /* [B][16] or NULL */,
                                           int32_t* n_close /* [B] */, double* sum_d2 /* [B] */, int32_t* n_pairs /* [B] */,
                                           double* sum_res2 /* [B] */, int32_t* empty /* [B] */,
                                           void* workspace, size_t workspace_bytes, void* stream,
                                           int32_t* n_within /* [B] or NULL */, float* d2_cut /* [B] or NULL */);
/* ONE step of pcreg_model_refit_cpd_f32's contract on the device: everything is a device pointer, nothing
 * synchronises, T_step may be NULL, T_out may not alias T_dev (sigma2_out may alias sigma2_in).  The shift dmin comes from
 * pcreg_dev_model_score_f32's chain at r2 = +inf inside the call.  The workspace, with nb = max(1, min(B, floor(131072 / max(Q, 1))))
 * transforms a batch, S = max(nb Q, 1), P = nb max(ceil(Q / 2048), 1), L = max(the contract's number of slices, 1), and roundup(x)
 * to a multiple of 256:
 *   roundup(pcreg_dev_model_score_workspace(Q, B, M)) + roundup(4 max(B Q, 1)) + roundup(4 max(B, 1)) + 256 + roundup(12 S)
 *   + roundup(32 P) + roundup(4 P) + roundup(48 nb) + roundup(20 L S) + roundup(152 P) bytes
 * (0 for an argument out of range).  PCREG_E_ARG also for a workspace shorter than that. */
size_t pcreg_dev_model_refit_cpd_workspace(int Q, int B, int M);
int pcreg_dev_model_refit_cpd_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq,
                                  const double* T_dev /* [B][16] on the device */, int B, const double* sigma2_in /* [B] */,
                                  double outlier, double* T_out /* [B][16] */, double* T_step /* [B][16] or NULL */,
                                  double* sigma2_out /* [B] */, double* Np /* [B] */, double* sum_res2 /* [B] */,
                                  double* sum_d2 /* [B] */, int32_t* n_live /* [B] */, int32_t* empty /* [B] */,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* clusterPoints(model, r) on the device: the connected components of the graph "rows i != j with fp32 squared distance
 * fmaf(dz,dz,fmaf(dy,dy,dx*dx)) <= r2" over the model's own rows (pcreg_model_cluster_f32's contract), in one launch chain
 * (DESIGN 4.11).  label [M], indexed by ORIGINAL row: the 0-based number of the row's cluster, clusters numbered in ascending
 * order of their smallest row.  n_clusters: one int32 on the device.  first / sizes ([M] each, either may be NULL): first[c]
 * the smallest row of cluster c and sizes[c] its number of rows for c < n_clusters, ZERO at and past n_clusters.  The result
 * is a function of (model rows, r2) only.  Nothing synchronises; no workgroup waits for another.  r2 NaN or negative:
 * PCREG_E_ARG.  Workspace: 2 * roundup(4 * max(M, 1), 256) + roundup(4 * max(ceil(M / 2048), 1), 256) bytes, whatever r2 and
 * the result.  Tile pairs are skipped by DESIGN 4.1's rule with the radius as the bound.  A handle may serve several streams at
 * once, each call with its own workspace. */
size_t pcreg_dev_model_cluster_workspace(int M);
int pcreg_dev_model_cluster_f32(const pcreg_dev_model* model, float r2, int32_t* label, int32_t* n_clusters, int32_t* first,
                                int32_t* sizes, void* workspace, size_t workspace_bytes, void* stream);
/* pcreg_model_dbscan_f32's contract on the device, in one launch chain without a host read: the neighbour count of
 * every row by a full self-join, the union of the core rows by pcreg_dev_model_cluster_f32's walk with only core rows staged,
 * flatten and number with only core roots counted, a second full self-join that gives every border row the smallest root among
 * its core neighbours, and the labels.  label [M] int32 by ORIGINAL row, -1 for noise; n_clusters one int32 on the device; core
 * [M] uint8, count [M] int32, first [M] (first[c] the smallest CORE row of cluster c) and sizes [M] (sizes[c] the rows of cluster
 * c, border rows included): each of the four may be NULL; first and sizes are ZERO at and past n_clusters.  The result is a
 * function of (model rows, r2, minpts) only -- not of the order of atomics, the order inside a cell, culling or the stream.
 * Nothing synchronises; no workgroup waits for another.  PCREG_E_ARG: r2 NaN or negative, minpts < 1, a NULL model, label,
 * n_clusters or workspace.  PCREG_E_WORKSPACE for a short workspace.
 * Workspace: 4 * roundup(4 * max(M, 1), 256) + roundup(4 * max(ceil(M / 2048), 1), 256) bytes, whatever r2, minpts and the
 * result.  A handle may serve several streams at once, each call with its own workspace. */
size_t pcreg_dev_model_dbscan_workspace(int M);
int pcreg_dev_model_dbscan_f32(const pcreg_dev_model* model, float r2, int minpts, int32_t* label, int32_t* n_clusters, uint8_t* core,
                               int32_t* count, int32_t* first, int32_t* sizes, void* workspace, size_t workspace_bytes, void* stream);
/* pcreg_model_normals_f32's contract on the device: normals [3 * ldn] and variation [M] (or NULL) are device
 * pointers, the viewpoint stays on the host (it travels as kernel arguments).  Two launches: the seed bound of every sorted row,
 * then one walk in which a workgroup owns 64 rows of a tile, keeps their k-lists in registers and finishes each row's normal
 * itself; tiles are skipped by DESIGN 4.1's rule with the k-th-neighbour bound.  The queries are the model's own sorted copy, so
 * any M a model can hold is served in one call.  Nothing synchronises; no workgroup waits for another.  Workspace: the seed bounds,
 * roundup(4 * max(M, 1), 256) bytes, whatever k.  A handle may serve several streams at once, each call with its own workspace. */
size_t pcreg_dev_model_normals_workspace(int M, int k);
int pcreg_dev_model_normals_f32(const pcreg_dev_model* model, int k, const double* viewpoint /* host, 3 or NULL */, float* normals,
                                int ldn, float* variation /* or NULL */, void* workspace, size_t workspace_bytes, void* stream);
/* pcreg_model_denoise_f32's contract on the device: mean_dist [M], inliers [M], n_inliers (one int32) and stats [4]
 * are device pointers, each may be NULL as there.  Six launches: the seed bound of every sorted row with k + 1; the normals' walk
 * with a list of distances alone, each row's mean distance finished in registers; the chunk sums; mu and the chunk deviations; sd,
 * thr and the chunk inlier counts; the ascending scatter and the count (skipped without n_inliers).  Nothing synchronises; no
 * workgroup waits for another.  Workspace, with R = max(M, 1) and C = max(ceil(M / 2048), 1):
 * roundup(4 R, 256) + roundup(8 R, 256) + 2 roundup(8 C, 256) + 2 roundup(4 C, 256) + 256 bytes, whatever k; a workspace shorter
 * than that is PCREG_E_ARG too.  A handle may serve several streams at once, each call with its own workspace.  The debug keys
 * "knn_nocull" and "knn_stats" act on the walk as on the normals'. */
size_t pcreg_dev_model_denoise_workspace(int M, int k);
int pcreg_dev_model_denoise_f32(const pcreg_dev_model* model, int k, double threshold, double* mean_dist /* or NULL */,
                                int32_t* inliers /* or NULL */, int32_t* n_inliers /* or NULL */, double* stats /* [4] or NULL */,
                                void* workspace, size_t workspace_bytes, void* stream);
/* pcreg_model_fps_f32's contract on the device: idx [K], dist [K], n_out, cover_d2, min_dist [M], label [M] and info
 * (one int32) are device pointers, each may be NULL except n_out.  info = 0 after a run; a DEAD start row, which only the device can
 * see, gives info = 1 and *n_out = 0 with nothing else written.  Two launches: ONE workgroup of 1024 threads runs every step -- the
 * steps are strictly sequential, and no workgroup waits for another -- keeping per 512-row tile its (max D, original row, sorted row)
 * and box in LDS, 36 bytes a tile, which is what bounds M by PCREG_FPS_MAX_ROWS; a step visits only the tiles, and inside them the
 * 64-row units, whose box DESIGN 4.1's rule does not certify farther from the sample than their largest D.  The second launch
 * scatters min_dist and label to original-row order.  Nothing synchronises and nothing is read on the host.  Workspace, with
 * R = max(M, 1) and U = 8 max(ceil(M / 512), 1): 2 roundup(4 R, 256) + roundup(16 U, 256) + 256 bytes, whatever K; 0 for M < 0 or
 * M > PCREG_FPS_MAX_ROWS; a workspace shorter than that is PCREG_E_ARG too.  A handle may serve several streams at once, each call
 * with its own workspace.  The debug key "knn_nocull" visits every tile and unit (same bits); "knn_stats" counts for
 * pcreg_debug_fps_stats. */
size_t pcreg_dev_model_fps_workspace(int M, int K);
int pcreg_dev_model_fps_f32(const pcreg_dev_model* model, int K, int start, float stop_d2, int32_t* idx /* or NULL */,
                            float* dist /* or NULL */, int32_t* n_out, float* cover_d2 /* or NULL */, float* min_dist /* or NULL */,
                            int32_t* label /* or NULL */, int32_t* info /* or NULL */, void* workspace, size_t workspace_bytes, void* stream);
/* pcreg_model_fpfh_f32's contract on the device: normals_dev [3 * ldn] (what pcreg_dev_model_normals_f32 writes; may
 * not be NULL with M > 0), fpfh [M][33] double and spfh [M][33] uint8 (or NULL) are device pointers, both ROW-major by original row
 * -- fpfh is what pcreg_dev_get_matches takes as row-major descriptors with D = 33.  Three launches: the seed bound of every sorted
 * row; the normals' walk, whose epilogue stores each row's list to an [M][k] table, gathers the neighbours' coordinates and normals
 * and counts the pair features; one thread per (row, feature) that weights the neighbours' counts in list order.  Nothing
 * synchronises; no workgroup waits for another.  Workspace, with R = max(M, 1):
 * roundup(4 R, 256) + 2 roundup(4 R k, 256) + roundup(33 R, 256) bytes; a workspace shorter than that is PCREG_E_ARG too, and so is
 * ldn < M.  A handle may serve several streams at once, each call with its own workspace.  The debug keys "knn_nocull" and
 * "knn_stats" act on the walk as on the normals'. */
size_t pcreg_dev_model_fpfh_workspace(int M, int k);
int pcreg_dev_model_fpfh_f32(const pcreg_dev_model* model, int k, const float* normals_dev /* [3][ldn] */, int ldn,
                             double* fpfh /* [M][33] */, uint8_t* spfh /* [M][33] or NULL */, void* workspace, size_t workspace_bytes,
                             void* stream);
/* pcreg_model_fpfh_radius_f32's contract on the device, in TWO calls, because the size of the lists is data; neither
 * synchronises.  pcreg_dev_model_fpfh_radius_count_f32 is pcreg_dev_model_range_count_f32 with the model's own rows as the
 * queries: counts [M] int32 and seg_off [M + 1] int64 on the device; its workspace is pcreg_dev_model_fpfh_radius_workspace(M, 0)
 * bytes.  The caller reads seg_off[M], the total, takes a workspace of pcreg_dev_model_fpfh_radius_workspace(M, capacity) bytes with
 * capacity >= the total, and calls pcreg_dev_model_fpfh_radius_f32 with the same r2 and seg_off: the radius search's fill writes
 * the lists (0-based rows) into the workspace, one kernel counts the pairs of every row's counted window (a wave of 64 lanes a row, LDS
 * integer atomics), one thread per (row, bin) weights the neighbours' counts in list order.  normals_dev [3 * ldn] (may not be NULL
 * with M > 0), fpfh [M][33] double, spfh [M][33] uint32 (or NULL) and n_neighbors [M] int32 (or NULL) are device pointers, ROW-major
 * by original row -- fpfh is what pcreg_dev_get_matches takes as row-major descriptors with D = 33.  A capacity below the total
 * truncates segments as pcreg_dev_model_range_fill_f32 documents: the descriptors of the truncated rows, and of rows that have
 * them as neighbours, are then unspecified, and nothing is written outside the outputs and the workspace.  Workspace, with
 * R = max(M, 1) and C = capacity: pcreg_dev_model_range_workspace(M, M) + 2 roundup(4 C, 256) + roundup(4 R, 256) +
 * roundup(132 R, 256) bytes; a workspace shorter than that is PCREG_E_ARG too, and so are ldn < M, M > 4 Mi, a negative capacity or
 * max_neighbors, r2 NaN or negative.  A handle may serve several streams at once, each call with its own workspace.  The debug
 * keys "knn_nocull", "knn_stats" and "range_sort_cap" act on the radius search as there; "fpfh_radius_lanes" (4, 16) changes the
 * lanes per row of the counting kernel and no bit. */
size_t pcreg_dev_model_fpfh_radius_workspace(int M, int64_t capacity);
int pcreg_dev_model_fpfh_radius_count_f32(const pcreg_dev_model* model, float r2, int32_t* counts /* [M] */, int64_t* seg_off /* [M + 1] */,
                                          void* workspace, size_t workspace_bytes, void* stream);
int pcreg_dev_model_fpfh_radius_f32(const pcreg_dev_model* model, float r2, int max_neighbors, const float* normals_dev /* [3][ldn] */, int ldn,
                                    const int64_t* seg_off /* [M + 1] */, int64_t capacity, double* fpfh /* [M][33] */,
                                    uint32_t* spfh /* [M][33] or NULL */, int32_t* n_neighbors /* [M] or NULL */, void* workspace,
                                    size_t workspace_bytes, void* stream);
/* pcreg_model_iss_f32's contract on the device: n_neighbors [M], eig [M][3] (or NULL), saliency [M], keypoints [M] and
 * n_keypoints (one int32) are device pointers, NULL as there.  Four launches: the self-join walk over all tiles with the integer
 * scatter, whose epilogue finishes each row's eigenvalues and saliency itself; the same walk at r2_nonmax over the rows with a
 * saliency, a flag byte per row; the two launches of the chunk scan that list the flagged rows ascending (the last three skipped
 * without n_keypoints).  Tiles are skipped by DESIGN 4.1's rule with D = the squared radius and the box of the workgroup's tile.
 * Nothing synchronises; no workgroup waits for another.  Workspace, with R = max(M, 1) and C = max(ceil(M / 2048), 1):
 * roundup(R, 256) + roundup(4 C, 256) bytes; a workspace shorter than that is PCREG_E_ARG too.  A handle may serve several streams
 * at once, each call with its own workspace.  The debug keys "knn_nocull" and "knn_stats" act on both walks as on the normals'
 * (each walk counts as one search of n_tiles^2 nominal visits). */
size_t pcreg_dev_model_iss_workspace(int M);
int pcreg_dev_model_iss_f32(const pcreg_dev_model* model, float r2_salient, float r2_nonmax, double gamma21, double gamma32,
                            int min_neighbors, int32_t* n_neighbors, double* eig /* or NULL */, double* saliency,
                            int32_t* keypoints /* or NULL */, int32_t* n_keypoints /* or NULL */, void* workspace,
                            size_t workspace_bytes, void* stream);
/* pcreg_model_fit_planes_f32's contract on the device: samples [P][B][3] (or NULL), labels, planes, centres, counts,
 * rmse, n_planes (one int32) and the diagnostics are device pointers, NULL as there; ref_vec is three HOST doubles or NULL; a sample
 * s names original row s - idx_base.  The rows are read through the pointer the handle was created on.  Two launches (reset; alive
 * bytes, labels and the box of the finite rows), then nine per round: the two launches of the chunk scan that list the alive rows
 * with their coordinates, the hypotheses, the scoring (lane = trial over 2048 staged rows, one integer atomic pair per chunk and
 * trial), the selection, the refit scatter, its 128-bit epilogue, the classification and the round's totals.  A device word says
 * that extraction has ended; every later launch reads it and returns.  Nothing synchronises, nothing is cleared by a memset, no
 * workgroup waits for another.  Workspace, with R = max(M, 1), C = max(ceil(M / 2048), 1) and T = n_trials:
 * 6400 + roundup(R, 256) + roundup(4 C, 256) + 4 roundup(4 R, 256) + 2 roundup(12 T, 256) + roundup(T, 256) + roundup(8 T, 256) +
 * roundup(4 T, 256) bytes; a workspace shorter than that is PCREG_E_ARG too.  A handle may serve several streams at once, each call
 * with its own workspace. */
size_t pcreg_dev_model_fit_planes_workspace(int M, int n_trials);
int pcreg_dev_model_fit_planes_f32(const pcreg_dev_model* model, float max_distance, const double* ref_vec /* host [3] or NULL */,
                                   double max_angle, int max_planes, int n_trials, int min_inliers, uint64_t seed,
                                   const int32_t* samples /* or NULL */, int32_t idx_base, int32_t* labels, double* planes, double* centres,
                                   int32_t* counts, double* rmse, int32_t* n_planes, int32_t* best_trial /* or NULL */,
                                   int64_t* best_cost /* or NULL */, int32_t* best_count /* or NULL */, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* pcreg_model_fit_spheres_f32's contract on the device: samples [P][B][4] (or NULL), labels, spheres, counts, rmse,
 * refit_used, n_spheres (one int32) and the diagnostics are device pointers, NULL as there; a sample s names original row
 * s - idx_base.  The rows are read through the pointer the handle was created on.  Two launches (reset; alive bytes, labels and the
 * box of the finite rows), then nine per round: the two launches of the chunk scan that list the alive rows with their coordinates,
 * the hypotheses, the scoring (lane = trial over 2048 staged rows, one integer atomic pair per chunk and trial), the selection, the
 * refit's seventeen integer sums (one set of atomics a workgroup), its 128-bit epilogue with the solve, the classification and the
 * round's totals.  A device word says that extraction has ended; every later launch reads it and returns.  Nothing synchronises,
 * nothing is cleared by a memset, no floating-point atomic, no workgroup waits for another.  Workspace, with R = max(M, 1),
 * C = max(ceil(M / 2048), 1) and T = n_trials:
 * 9984 + roundup(R, 256) + roundup(4 C, 256) + 4 roundup(4 R, 256) + roundup(12 T, 256) + roundup(16 T, 256) + roundup(T, 256) +
 * roundup(8 T, 256) + roundup(4 T, 256) bytes; a workspace shorter than that is PCREG_E_ARG too.  A handle may serve several streams
 * at once, each call with its own workspace. */
size_t pcreg_dev_model_fit_spheres_workspace(int M, int n_trials);
int pcreg_dev_model_fit_spheres_f32(const pcreg_dev_model* model, float max_distance, float min_radius, float max_radius, int max_spheres,
                                    int n_trials, int min_inliers, uint64_t seed, const int32_t* samples /* or NULL */, int32_t idx_base,
                                    int32_t* labels, double* spheres, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_spheres,
                                    int32_t* best_trial /* or NULL */, int64_t* best_cost /* or NULL */, int32_t* best_count /* or NULL */,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* pcreg_model_fit_cylinders_f32's contract on the device: normals_dev [3][ldn] fp32 by original row, ldn >= M, as
 * pcreg_dev_model_normals_f32 writes it (never NULL with M > 0); samples [P][B][2] (or NULL), labels, cylinders, extents, counts,
 * rmse, refit_used, n_cylinders (one int32) and the diagnostics are device pointers, NULL as there; ref_vec is three HOST doubles
 * or NULL; a sample s names original row s - idx_base.  The rows are read through the pointer the handle was created on.  Two
 * launches (reset; alive bytes, usable-normal bytes, labels and the box of the finite rows), then eleven per round: the two
 * launches of the chunk scan that list the alive rows with their coordinates, the hypotheses, the scoring (lane = trial over 2048
 * staged rows, one integer atomic pair per chunk and trial), the selection, the axis pass' seven integer sums, the basis (Jacobi,
 * w, u, v), the circle pass' eleven integer sums (one set of atomics a workgroup each), the 128-bit epilogue with the solve, the
 * classification with the extent along the axis, and the round's totals.  A device word says that extraction has ended; every later
 * launch reads it and returns.  Nothing synchronises, nothing is cleared by a memset, no floating-point atomic, no workgroup waits
 * for another.  Workspace, with R = max(M, 1), C = max(ceil(M / 2048), 1) and T = n_trials:
 * 11008 + 2 roundup(R, 256) + roundup(4 C, 256) + 4 roundup(4 R, 256) + roundup(12 T, 256) + roundup(28 T, 256) + roundup(T, 256) +
 * roundup(8 T, 256) + roundup(4 T, 256) bytes; a workspace shorter than that is PCREG_E_ARG too.  A handle may serve several streams
 * at once, each call with its own workspace. */
size_t pcreg_dev_model_fit_cylinders_workspace(int M, int n_trials);
int pcreg_dev_model_fit_cylinders_f32(const pcreg_dev_model* model, float max_distance, float min_radius, float max_radius,
                                      const double* ref_vec /* 3 host doubles or NULL */, double max_angle, const float* normals_dev,
                                      int ldn, int max_cylinders, int n_trials, int min_inliers, uint64_t seed,
                                      const int32_t* samples /* or NULL */, int32_t idx_base, int32_t* labels, double* cylinders,
                                      double* extents, int32_t* counts, double* rmse, int32_t* refit_used, int32_t* n_cylinders,
                                      int32_t* best_trial /* or NULL */, int64_t* best_cost /* or NULL */,
                                      int32_t* best_count /* or NULL */, void* workspace, size_t workspace_bytes, void* stream);
/* matchFeatures' filter chain on that top-2 in ONE launch: threshold, ratio test, Unique back-check, ordered compaction
 * into 1-based pairs [k][2] and the matched coordinates pts1 / pts2 (n x 3 column-major doubles, ld = Q; both NULL to
 * skip) -- completeExperimentFast.m:205-206.  The handle holds the WHOLE model (one rank). */
int pcreg_dev_model_match_f32(const pcreg_dev_model* model, const float* q, int Q, int ldq, const int32_t* idx,
                              const float* dist, float thr_abs, float max_ratio, int unique, void* workspace,
                              size_t workspace_bytes, uint32_t* pairs, double* pts1, double* pts2, int32_t* n_pairs,
                              void* stream);
/* The same split around the multi-GPU exchange (idx / dist are the MERGED global top-2):
 * _match_table_f32: this rank's contribution to a [4][Q] table of 4-byte words, column = query: rows 0-2 the coordinate
 *   bits of the query's nearest model point, row 3 its Unique verdict (1 when Unique is off), written by the rank whose
 *   shard [m_lo, m_lo + M) holds that point and only for queries that pass the filters; zero elsewhere.  An integer
 *   all_reduce(SUM) over the ranks assembles the table exactly (one contributor per column).
 * pcreg_dev_match_from_table_f32: filters again (deterministic), verdicts and coordinates from the summed table, ordered
 *   compaction.  `workspace`: any search workspace of this Q (only its counters are used). */
int pcreg_dev_model_match_table_f32(const pcreg_dev_model* model, int32_t m_lo, int M_total, const float* q, int Q, int ldq,
                                    const int32_t* idx, const float* dist, float thr_abs, float max_ratio, int unique,
                                    void* workspace, size_t workspace_bytes, int32_t* table, void* stream);
int pcreg_dev_match_from_table_f32(const float* q, int Q, int ldq, int M_total, const int32_t* idx, const float* dist,
                                   float thr_abs, float max_ratio, const int32_t* table, void* workspace,
                                   size_t workspace_bytes, uint32_t* pairs, double* pts1, double* pts2, int32_t* n_pairs,
                                   void* stream);

/* Merge R candidate lists (e.g. the all-gathered per-shard results, laid out
 * [R][Q][2]) into one top-2 per query, ordering by (dist, idx). */
int pcreg_dev_merge_top2_f32(const int32_t* idx_in, const float* dist_in, int R, int Q,
                             int32_t* idx, float* dist, void* stream);
/* The same with list r starting r * rank_stride ELEMENTS into idx_in / dist_in (>= 2 Q): lets one all_gather
 * carry a rank's indices and distances in a single buffer. */
int pcreg_dev_merge_top2_strided_f32(const int32_t* idx_in, const float* dist_in, int R, int Q, size_t rank_stride,
                                     int32_t* idx, float* dist, void* stream);
/* The k analogue (knnsearch over a model split into shards): R lists of [Q][k] with list r starting r * rank_stride
 * ELEMENTS in (0: densely packed, Q * k; else >= Q * k) -> one [Q][k] per query by (dist, idx); -1 entries are empty and
 * an index repeated across lists is kept once. */
int pcreg_dev_merge_topk_f32(const int32_t* idx_in, const float* dist_in, int R, int Q, int k, size_t rank_stride,
                             int32_t* idx, float* dist, void* stream);

/* Device-resident ransac: n is read from device memory (*n_dev <= n_cap), so the
 * match stage can feed it without a host round trip.  Results land in `out`
 * (pcreg_dev_ransac_result) and inlier_idx (capacity n_cap). */
typedef struct pcreg_dev_ransac_result {
    double  T[16];
    int32_t n_inliers, num_success, max_inliers, failed, n, winner;
} pcreg_dev_ransac_result;
size_t pcreg_dev_ransac_workspace(int n_cap, int iterNum);
int pcreg_dev_ransac(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld,
                     const pcreg_ransac_opts* opts, const int32_t* sample_idx,
                     pcreg_dev_ransac_result* out, int32_t* inlier_idx,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Measurement aid: with timing enabled, the candidates kernel of every point search the CALLER asks for (any size) is
 * bracketed by two HIP events on its launch stream; pcreg_dev_search_kernel_ms returns the mean
 * duration over the launches since the previous call (it waits for them) and their number. */
int pcreg_dev_search_kernel_timing(int enable);
int pcreg_dev_search_kernel_ms(float* mean_ms, int* launches);

/* One registration's hypotheses split over ranks (optional mode): every rank runs the
 * hypotheses [hyp_begin, hyp_begin + hyp_count) of a job of opts->iterNum -- the built-in sampler and the
 * first-maximum tie-break (ransac.m:70-72) use the GLOBAL hypothesis index, so the union over ranks is
 * exactly the single-rank run -- and leaves its share's best in `part` (device).  Combine on the ranks:
 * key by MAX, num_success by SUM, has / T from the rank whose key equals the maximum; then
 * pcreg_dev_ransac_finish builds the result and the inlier list from the combined part.  sample_idx,
 * if given, holds the hyp_count rows of THIS share. */
typedef struct pcreg_dev_ransac_part {
    unsigned long long key;          /* (inlier count << 32) | ~global hypothesis index; 0 for an empty share */
    int32_t num_success, has;        /* hypotheses of the share with count >= thInlr; 1 if the winner holds a transform */
    double  T[12];                   /* the winner's transform, rows of [R t] (as stored internally) */
} pcreg_dev_ransac_part;
int pcreg_dev_ransac_partial(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld,
                             const pcreg_ransac_opts* opts, const int32_t* sample_idx, int hyp_begin, int hyp_count,
                             pcreg_dev_ransac_part* part, void* workspace, size_t workspace_bytes, void* stream);
int pcreg_dev_ransac_finish(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld,
                            const pcreg_ransac_opts* opts, const pcreg_dev_ransac_part* combined,
                            pcreg_dev_ransac_result* out, int32_t* inlier_idx, void* stream);
/* The same from the n_parts UNCOMBINED parts of all shares (e.g. one all_gather of the 112-byte structs): the
 * kernel takes the maximum key, sums num_success and uses the winner's transform itself. */
int pcreg_dev_ransac_finish_parts(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld,
                                  const pcreg_ransac_opts* opts, const pcreg_dev_ransac_part* parts, int n_parts,
                                  pcreg_dev_ransac_result* out, int32_t* inlier_idx, void* stream);

/* ---- descriptor stage, resident: speedyDescriptors.m:59 -> getMatches.m -> ransac.m --------
 * (completeExperimentFast.m:131-213 per sphere position) without a host copy in between. */

/* getSpacialHistogramDescriptors.m:25-258 on device buffers.  pts / sample_pts are n x 3
 * column-major (ld / lds); feat [S][3] and desc [S][980] are ROW-major with capacity S
 * (row v < V is the v-th surviving keypoint, in sample order); counters[0] = V,
 * counters[1] = 0 or the size of a support that exceeded the LDS capacity (then the
 * outputs are invalid: lower max_pts). */
size_t pcreg_dev_spatial_histogram_descriptors_workspace(int P, int S);
int pcreg_dev_spatial_histogram_descriptors(const double* pts, int P, int ld, const double* sample_pts, int S, int lds,
                                            const pcreg_desc_opts* options, double* feat, double* desc,
                                            int32_t* counters, void* workspace, size_t workspace_bytes, void* stream);
/* What a resident pipeline keeps: the 980 counts of a row as uint16 (integer counts <= the support size <= 8191: 1.96 KB
 * per keypoint instead of 7.84 KB), written ONCE, straight from the histogram in LDS: rows [S][980] in KEYPOINT order (row s is
 * meaningful only for a surviving keypoint s), row_index [S] = the ascending list of the V survivors, feat [V][3] compact.
 * pcreg_dev_get_matches_rows_u16 takes rows + index as they are.  single_mode: 0 double data; 1 `single` arithmetic for the
 * support (see pcreg_spatial_histogram_descriptors_f32; data widened exactly to double by the caller), keypoints single;
 * 2 the same with a single cloud and double keypoints.  Same workspace. */
int pcreg_dev_spatial_histogram_descriptors_rows_u16(const double* pts, int P, int ld, const double* sample_pts, int S, int lds,
                                                     const pcreg_desc_opts* options, int single_mode, double* feat, uint16_t* rows,
                                                     int32_t* row_index, int32_t* counters, void* workspace, size_t workspace_bytes,
                                                     void* stream);

/* getMatches.m:21-59 on device buffers.  layout: PCREG_LAYOUT_FEATURE_MAJOR = MATLAB's
 * column-major n x D (ld >= n); PCREG_LAYOUT_ROW_MAJOR = dense [n][D] (ld == D), what the
 * descriptor entry point above emits.  The inputs are not modified.  pairs [Q][2] uint32,
 * 1-based, ascending surface row; metric [Q] or NULL; *n_pairs device int32.  Q and M are
 * host integers (grid sizes); with Unique and Q*Q*D > 2e10 the call synchronises the stream ONCE (the
 * candidate count that sizes the back-search); otherwise it does not synchronise. */
#define PCREG_LAYOUT_FEATURE_MAJOR 0
#define PCREG_LAYOUT_ROW_MAJOR     1
size_t pcreg_dev_get_matches_workspace(int Q, int M, int D);
int pcreg_dev_get_matches(const double* descSurface, int Q, int ldS, const double* descModel, int M, int ldM, int D,
                          int layout, const pcreg_match_opts* par, uint32_t* pairs, double* metric,
                          int32_t* n_pairs, void* workspace, size_t workspace_bytes, void* stream);
/* The same on uint16 rows (pcreg_dev_spatial_histogram_descriptors_rows_u16's output): row i of a descriptor set is
 * rows[index[i]] (index NULL: rows[i]); the counts are widened to double, exactly, on the way into getMatches.m:24-37's
 * private copies -- pairs (numbered by i) and metric are those of the double entry.  Same workspace. */
int pcreg_dev_get_matches_rows_u16(const uint16_t* rowsSurface, const int32_t* indexSurface, int Q, const uint16_t* rowsModel,
                                   const int32_t* indexModel, int M, int D, const pcreg_match_opts* par, uint32_t* pairs,
                                   double* metric, int32_t* n_pairs, void* workspace, size_t workspace_bytes, void* stream);

/* completeExperimentFast.m:205-206: pts1 = featSurface(matches(:,1),:), pts2 =
 * featModel(matches(:,2),:) as n x 3 column-major with ld = cap -- the input of
 * pcreg_dev_ransac (n = *n_pairs stays on the device).  feat* are row-major [.][3]. */
int pcreg_dev_gather_matched_rows(const uint32_t* pairs, const int32_t* n_pairs, int cap, const double* featSurface,
                                  const double* featModel, double* pts1, double* pts2, void* stream);

/* ---- sphere-sweep driver pieces (completeExperimentFast.m:46-225) and its final stage ----
 * feat is row-major [V][3] (what the descriptor entry point emits). */

/* counts[s] = #{ i : vecnorm(feat(i,:) - centres(s,:)) < R }: the sphere validity test of
 * completeExperimentFast.m:57-64 (getLocalPoints.m:23-34 reduced to its count). centres [S][3]. */
int pcreg_dev_sphere_counts(const double* feat, int V, const double* centres, int S, double R,
                            int32_t* counts, void* stream);

/* getDescriptorMask (completeExperimentFast.m:435-439, margin folded into R) as the ascending
 * 0-based index list of the rows inside the sphere; *n_out = its length.  `centre` is HOST memory. */
size_t pcreg_dev_sphere_select_workspace(int V);
int pcreg_dev_sphere_select(const double* feat, int V, const double centre[3], double R, int32_t* idx,
                            int32_t* n_out, void* workspace, size_t workspace_bytes, void* stream);

/* getDescriptorMask for S spheres in one launch (completeExperimentFast.m:109-125 for every sphere of the sweep): the row
 * list of sphere s is written at idx[seg_off[s] ..], ascending and 0-based; seg_off [S + 1] (device) are the running sums of
 * pcreg_dev_sphere_counts' counts.  feat_out (or NULL): featCur of every sphere back to back ([seg_off[S]][3] row-major);
 * n_out (or NULL) [S]: the lengths found (== the counts).  centres [S][3] on the device. */
int pcreg_dev_sphere_select_batched(const double* feat, int V, const double* centres, int S, double R, const int32_t* seg_off,
                                    int32_t* idx, double* feat_out, int32_t* n_out, void* stream);

/* getMatches.m:21-59 for S segments in ONE chain of launches: getMatches(descSurface, descModel(rows_s, :), par) for every
 * segment s, rows_s = seg_rows[seg_off[s] .. seg_off[s+1]) (0-based, ascending) -- the per-sphere calls of the sweep,
 * completeExperimentFast.m:131-149, which the reference runs under parfor.  descSurface [Q][D], descModel [VM][D] dense
 * row-major doubles (what the descriptor entry point emits).  total_rows = seg_off[S] and max_rows = the longest segment
 * are known to the host from the counts.  pairs_all [S][Q][2]: segment s's pairs, 1-based, the model index counting WITHIN
 * the segment like the per-sphere call's; n_pairs [S]; metric_all [S][Q] or NULL.  The pairs are those of one
 * pcreg_dev_get_matches call per segment (same arithmetic on the same operands: the appended constant and the row norms
 * differ per segment, the powered columns do not and are computed once).  Metric SAD only.
 * Memory: the one-chain form takes  4 VM' Q'  (the shared score matrix, VM' / Q' = VM / Q rounded up to 128)  +  8 D (VM + Q)  (the
 * powered rows)  +  ~S Q (32 splits + 500) bytes (the per-segment lists and re-rank work items);  up to 4 GB of that it runs as ONE chain and nothing
 * synchronises.  Above, the call runs in batches of consecutive segments on gathered sub-models (the union of the rows a batch
 * names), inside a workspace of 4 GB + 12 VM + 4 total_rows + 4 S bytes: same pairs, one host synchronisation at entry and one or
 * two per batch.  A single segment that does not fit the bound is refused with PCREG_E_WORKSPACE. */
size_t pcreg_dev_get_matches_segmented_workspace(int Q, int VM, int D, int S, int total_rows, int max_rows);
int pcreg_dev_get_matches_segmented(const double* descSurface, int Q, const double* descModel, int VM, int D, const int32_t* seg_rows,
                                    const int32_t* seg_off, int S, int total_rows, int max_rows, const pcreg_match_opts* par,
                                    uint32_t* pairs_all, double* metric_all, int32_t* n_pairs, void* workspace, size_t workspace_bytes,
                                    void* stream);
/* One model, many surfaces: the part of the call above that depends on the model set and the options only -- its powered rows and
 * six scalars per row -- prepared once into a caller-owned buffer of pcreg_dev_segmented_model_bytes(VM, D) bytes, and the call that
 * uses it (prepared_change_metric / prepared_metric_factor: the options it was made with; a call whose par differs recomputes them
 * itself).  The caller must not change descModel while the preparation is in use.  Same pairs as pcreg_dev_get_matches_segmented. */
size_t pcreg_dev_segmented_model_bytes(int VM, int D);
int pcreg_dev_segmented_model_prepare(const double* descModel, int VM, int D, const pcreg_match_opts* par, void* prepared, size_t prepared_bytes,
                                      void* stream);
int pcreg_dev_get_matches_segmented_prepared(const double* descSurface, int Q, const double* descModel, int VM, int D, const void* prepared,
                                             int prepared_change_metric, double prepared_metric_factor, const int32_t* seg_rows,
                                             const int32_t* seg_off, int S, int total_rows, int max_rows, const pcreg_match_opts* par,
                                             uint32_t* pairs_all, double* metric_all, int32_t* n_pairs, void* workspace, size_t workspace_bytes,
                                             void* stream);

/* dst(k,:) = src(idx(k),:), k < min(*n, cap): featCur / descCur of completeExperimentFast.m:122-125
 * (row-major, D doubles per row). */
int pcreg_dev_gather_rows_f64(const double* src, int D, const int32_t* idx, const int32_t* n, int cap,
                              double* dst, void* stream);

/* The batched sphere sweep (completeExperimentFast.m:166-224 for ALL spheres in one enqueue chain, no host round trip
 * between the per-sphere getMatches calls and the per-trial ransac calls -- the reference runs both under parfor).
 * pcreg_dev_sweep_plan:   trial = find(num_putative > putative_thresh) (:175) in sphere order -> trial_idx [S] (-1 past
 *                         n_trials), offsets [S+1] of each trial's pairs in the packed arrays, *n_trials.
 * pcreg_dev_sweep_gather: pts1 = featSurface(matches(:,1),:), pts2 = featuresM(matches(:,2),:) (:205-206) for every trial,
 *                         packed at offsets[t] (n x 3 column-major, leading dimension ld).  pairs_all [S][VS][2] are the
 *                         1-based pairs of pcreg_dev_get_matches per sphere, featCur_all the spheres' gathered keypoints
 *                         ([rows][3]) back to back, sphere i starting at row row_off[i].
 * pcreg_dev_ransac_batched: pcreg_ransac_batched on device buffers: registration b owns rows [offsets[b], offsets[b+1])
 *                         (offsets on the DEVICE: sizes need not be known on the host), built-in sampler seeded seed + b;
 *                         empty registrations report failed = 1.  out [B], inlier_idx has the rows' layout. */
int pcreg_dev_sweep_plan(const int32_t* n_pairs, int S, int putative_thresh, int32_t* trial_idx, int32_t* offsets,
                         int32_t* n_trials, void* stream);
int pcreg_dev_sweep_gather(const uint32_t* pairs_all, int VS, const int32_t* n_pairs, const int32_t* trial_idx,
                           const int32_t* offsets, const int32_t* n_trials, int S, const double* featSurface,
                           const double* featCur_all, const int64_t* row_off, double* pts1, double* pts2, int ld,
                           void* stream);
size_t pcreg_dev_ransac_batched_workspace(int n_cap, int iterNum, int B);
int pcreg_dev_ransac_batched(const double* pts1, const double* pts2, int ld, const int32_t* offsets, int B, int n_cap,
                             const pcreg_ransac_opts* opts, pcreg_dev_ransac_result* out, int32_t* inlier_idx,
                             void* workspace, size_t workspace_bytes, void* stream);
/* pcreg_fgr_batched on device buffers (its contract, above): every pointer but opts is device memory, the offsets are not read on
 * the host; n_cap = the largest registration: it chooses the kernel form and the launch and is trusted for that only (a
 * registration of more rows reports failed = 1).  T0, tuple_idx and kept may be NULL.  out [B]; inlier_idx and kept have the rows'
 * layout.  Enqueued on `stream`, nothing synchronises; the workspace (0 for an argument out of range) may hold anything. */
size_t pcreg_dev_fgr_batched_workspace(int n_cap, int B, int iterations);
int pcreg_dev_fgr_batched(const double* pts1, const double* pts2, int ld, const int32_t* offsets, int B, int n_cap,
                          const pcreg_fgr_opts* opts, const double* T0, const int32_t* tuple_idx, pcreg_fgr_result* out,
                          int32_t* inlier_idx, uint8_t* kept, void* workspace, size_t workspace_bytes, void* stream);

/* AlignPoints_KNN.m:17-59 for B supports resident in HBM (the device-tier form of
 * pcreg_align_points_knn_batched; same layouts, every pointer is device memory): support b owns rows
 * [offsets[b], offsets[b+1]) of pts / aligned (n x 3 column-major, ld >= total); max_n = the largest support
 * (<= 8192, else PCREG_E_ARG): it chooses the launch and is trusted, the offsets are not read on the host;
 * coeff 9*B, c 3*B, status B: 0 ok, 1 = fewer than 2 points, 2 = the support holds more points than the launch chosen
 * for max_n does (max_n was too small).  With a status other than 0 nothing else is written for that support: its rows
 * of aligned, coeff and c keep what they held.  Enqueued on `stream`, nothing synchronises. */
int pcreg_dev_align_points_knn_batched(const double* pts, int total, int ld, const int32_t* offsets, int B, int max_n,
                                       int C1, int C2, double* aligned, double* coeff, double* c, int32_t* status,
                                       void* stream);

/* quickTF.m:5-7: out = [pts, 1] * T (first three columns).  pts/out n x 3 column-major on the
 * device, T 4x4 column-major in HOST memory (invertTF is a 16-number host operation). */
int pcreg_dev_quick_tf(const double* pts, int n, int ld, const double T[16], double* out, int ldo, void* stream);

/* completeExperimentFast.m:368-391: inliers = vecnorm(pts1 - pts2) < maxDist, T_refine =
 * estimateTransform over them.  n = *n_dev <= cap; T16 (device, column-major 4x4, zeros when
 * empty), info[0] = number of inliers, info[1] = 1 if the transform is empty. */
int pcreg_dev_refine_by_distance(const double* pts1, const double* pts2, const int32_t* n_dev, int cap, int ld,
                                 double maxDist, double* T16, int32_t* info, void* stream);

/* unique(A, 'rows') on the device (pcreg_unique_rows3's contract): A n x 3 doubles column-major with leading
 * dimension ld >= n_cap, n = *n_dev read on the device (clamped into [0, n_cap]; rows past n are never read), ia [n_cap]
 * (idx_base-based), n_unique one int32 on the device.  Every double is ordered by an order-preserving u64 image (sign flip, -0
 * as +0); a NaN is ordered by that image of its bit pattern -- positive NaNs behind +inf, negative ones before -inf, two NaNs equal
 * iff their bits are -- which is NOT MATLAB's rule; any input terminates and stays in bounds.  A tile sort of 2048 records in LDS,
 * ceil(log2(n_cap / 2048)) merge passes, head flags + scan + compaction; no workgroup waits for another, nothing synchronises.
 * Workspace: 2 * (3 * roundup(8 * max(n, 1), 256) + roundup(4 * max(n, 1), 256)) + roundup(4 * max(ceil(n / 2048), 1), 256) bytes
 * with n = n_cap; a shorter one is PCREG_E_ARG. */
size_t pcreg_dev_unique_rows3_workspace(int n_cap);
int pcreg_dev_unique_rows3_f64(const double* A, const int32_t* n_dev, int n_cap, int ld, int32_t idx_base, int32_t* ia,
                               int32_t* n_unique, void* workspace, size_t workspace_bytes, void* stream);
/* pcreg_aggregate_matches on the device as one launch chain: out1 / out2 n_cap x 3 (leading dimension ldo >= n_cap), ia [n_cap]
 * or NULL (idx_base-based composed index), n_out one int32 on the device.  Workspace:
 * 2 * roundup(4 * max(n, 1), 256) + 256 + roundup(24 * max(n, 1), 256) + pcreg_dev_unique_rows3_workspace(n) bytes, n = n_cap.
 * The chain leaves the count after the FIRST unique as one int32 at byte offset 2 * roundup(4 * max(n, 1), 256) of the workspace. */
size_t pcreg_dev_aggregate_matches_workspace(int n_cap);
int pcreg_dev_aggregate_matches(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld, double* out1,
                                double* out2, int ldo, int32_t idx_base, int32_t* ia, int32_t* n_out, void* workspace,
                                size_t workspace_bytes, void* stream);
/* pcreg_downsample_grid_f32's contract on the device: pts, out [3 * ldo], count [n] or NULL, label [n] or NULL are
 * device pointers; n_out and info one int32 each on the device.  The device cannot know of the 2^21-cell refusal without a read:
 * info = 0 when the cloud is fine, 1 when it is refused, then with n_out = 0 and nothing else written.  Nothing synchronises and
 * nothing is read on the host; the launch chain depends on n alone.  Limits per chunk of 2048 rows and one reducing workgroup,
 * (u64 key, u32 row) records, a stable least-significant-digit radix sort over ping-pong buffers (8-bit digits; only the passes
 * under the used key bits move data), head flags + chunk scan, one thread per voxel for the ordered means.
 * Workspace, with nn = max(n, 1) and chunks = ceil(nn / 2048):
 *   256 + roundup(24 * chunks, 256) + roundup(4 * chunks, 256) + 2 * (roundup(8 * nn, 256) + roundup(4 * nn, 256))
 *       + roundup(1024 * chunks, 256) + 1024 + roundup(4 * chunks, 256) + roundup(4 * nn, 256) bytes;
 * a shorter one is PCREG_E_ARG, and so are pcreg_downsample_grid_f32's argument cases and a NULL n_out, info or workspace.
 * pcreg_dev_downsample_grid_chunk: the records one workgroup of the sort handles (2048), for tests that straddle it. */
size_t pcreg_dev_downsample_grid_workspace(int n);
int pcreg_dev_downsample_grid_chunk(void);
int pcreg_dev_downsample_grid_f32(const float* pts, int n, int ld, double step, float* out, int ldo, int32_t* count, int32_t* label,
                                  int32_t* n_out, int32_t* info, void* workspace, size_t workspace_bytes, void* stream);
/* pcreg_ndt's contract on the device.  pcreg_dev_ndt_create: pts is a device pointer; the table is built on `stream`
 * by pcreg_dev_downsample_grid_f32's chain up to the voxel order, one thread per voxel for the Gaussians and a chunk scan that
 * compacts them; it is a one-off and synchronises the stream twice (the voxel count sizes the scratch, the Gaussian count is kept).
 * The handle owns its table and does not keep pts.  pcreg_dev_ndt_size / pcreg_dev_ndt_get are pcreg_ndt_size / pcreg_ndt_get (the
 * outputs are HOST pointers; get synchronises the device).
 * pcreg_dev_ndt_refit_f32 is ONE step: q, T_dev [B][16], T_out [B][16], T_step [B][16] (or NULL: not wanted), n_pairs, sum_e and
 * empty [B] are device pointers; T_out may not alias T_dev.  Nothing synchronises, nothing is read on the host, no workgroup
 * waits for another: one launch of a workgroup per (transform, chunk of 2048 queries) -- a thread moves its 8 consecutive queries,
 * finds their candidate voxels by a branch-free binary search of the table's sorted keys and adds the pairs' 28 sums -- and one of
 * a wave per transform for the fit.  There is no batching.  Workspace, with P = B * max(ceil(Q / 2048), 1):
 *   roundup(224 P, 256) + roundup(4 P, 256) bytes;
 * a shorter one is PCREG_E_ARG, and so is a NULL one unless that is 0 bytes.  A handle may serve several streams at once, each
 * call with its own workspace.  pcreg_dev_ndt_refit_workspace returns 0 for arguments the step refuses. */
typedef struct pcreg_dev_ndt pcreg_dev_ndt;
int pcreg_dev_ndt_create(const float* pts, int n, int ld, double step, int min_points, void* stream, pcreg_dev_ndt** ndt);
int pcreg_dev_ndt_destroy(pcreg_dev_ndt* ndt);
int pcreg_dev_ndt_size(const pcreg_dev_ndt* ndt, int* n_voxels, int* n_gaussians);
int pcreg_dev_ndt_get(const pcreg_dev_ndt* ndt, int32_t* cells, int32_t* counts, double* means, double* C, float* lo, float* origin);
size_t pcreg_dev_ndt_refit_workspace(int Q, int B);
int pcreg_dev_ndt_refit_f32(const pcreg_dev_ndt* ndt, const float* q, int Q, int ldq, const double* T_dev /* [B][16] on the device */,
                            int B, int neighbors, double outlier_ratio, double* T_out /* [B][16] */, double* T_step /* [B][16] or NULL */,
                            int32_t* n_pairs /* [B] */, double* sum_e /* [B] */, int32_t* empty /* [B] */, void* workspace,
                            size_t workspace_bytes, void* stream);
/* T = estimateTransform(pts1(idx, :), pts2(idx, :)) with the index list on the device (completeExperiment.m:458 on ransac's
 * inlier_idx): rows idx[0 .. *n_idx_dev) (idx_base-based; the count is clamped into [0, cap], every index into the cap rows) of
 * pts1 / pts2 (cap x 3 column-major, leading dimension ld >= cap).  The arithmetic of pcreg_dev_refine_by_distance with every
 * listed row counted: 3 rows by the three-point fit, fewer give an empty transform.  T16 and info ([0] rows used, [1] 1 if empty)
 * as there. */
int pcreg_dev_estimate_transform_indexed(const double* pts1, const double* pts2, int ld, const int32_t* idx, int32_t idx_base,
                                         const int32_t* n_idx_dev, int cap, double* T16, int32_t* info, void* stream);

/* The final stage's device pieces, batched over its K clusters (pcreg_final_stage runs on them).
 * pcreg_dev_quick_tf_batched: out copy k (n x 3 column-major, leading dimension ldo, starting at out + 3 k ldo) = [pts, 1] * T_k,
 *   T_dev [K][16] column-major 4 x 4 on the DEVICE; bit for bit K calls of pcreg_dev_quick_tf.  limits (or NULL) [K][6]: every
 *   copy's (xmin xmax ymin ymax zmin zmax) (+inf / -inf for n = 0).  One launch for the copies.
 * pcreg_dev_final_close_refine_batched: completeExperimentFast.m:357-391 for K clusters, one wave each.  Cluster k's pairs (1-based
 *   [.][2], as pcreg_dev_get_matches writes them) and its surviving keypoints (feat, row-major [.][3]) start at row kp_off[k] (capacity
 *   kp_off[k+1] - kp_off[k]); its model keypoints at row seg_off[k] of featCur_all ([.][3]); n_pairs[k] pairs.  Out: n_close[k],
 *   precision[k] = n_close / n * 100 (fp64, NaN for n = 0), T16 [K][16] and empty[k] -- bit for bit pcreg_dev_gather_matched_rows +
 *   pcreg_dev_refine_by_distance on the cluster (one device function serves both kernels).  kp_off / seg_off on the device.
 * pcreg_dev_final_pick_apply: best = MATLAB's max over precision (first maximum, NaN skipped, 0 if all are NaN) into *best (device
 *   int32), out (n x 3, ldo) = quickTF(copy best of pts_tform_all, invertTF(T16[best])) with invertTF.m's arithmetic, or copy best
 *   itself when empty[best]; pts_tform_all holds K copies of n x 3 (leading dimension ld) at 3 k ld.  Nothing is read on the host. */
int pcreg_dev_quick_tf_batched(const double* pts, int n, int ld, const double* T_dev, int K, double* out, int ldo, double* limits, void* stream);
int pcreg_dev_final_close_refine_batched(const uint32_t* pairs, const int32_t* n_pairs, const double* feat, const int32_t* kp_off,
                                         const double* featCur_all, const int32_t* seg_off, int K, double maxDist, int32_t* n_close,
                                         double* precision, double* T16, int32_t* empty, void* stream);
int pcreg_dev_final_pick_apply(const double* precision, const double* T16, const int32_t* empty, int K, const double* pts_tform_all, int n,
                               int ld, double* out, int ldo, int32_t* best, void* stream);

/* ---- multi-GPU behind the C ABI (RCCL over xGMI inside the library; comm.hip) -----------------------------
 * One process per GPU -- a MATLAB parfor / spmd worker each, the reference's own unit of parallelism
 * (completeExperimentFast.m:134,201).  Worker 0 calls pcreg_comm_get_unique_id; the 128 bytes reach the other
 * workers by the host language's own means (labBroadcast, a file); every worker calls pcreg_set_device and then
 * pcreg_comm_init(rank, world, id).  The sharded calls are collective: every rank must make them, in the same
 * order, and every rank gets the same result -- bit for bit the single-GPU one.  RCCL is dlopen'ed at
 * pcreg_comm_init (PCREG_E_HIP with a message if librccl.so.1 is missing). */
typedef struct pcreg_comm_id { char bytes[128]; } pcreg_comm_id;      /* an ncclUniqueId */
int pcreg_comm_get_unique_id(pcreg_comm_id* id);
int pcreg_comm_init(int rank, int world, const pcreg_comm_id* id);
/* The same communicator over HOST-STAGED exchanges instead of RCCL: the ranks meet in the POSIX shared-memory segment
 * `name` ("/something", unique per group; every rank passes the same).  For workers that share one GPU (RCCL refuses two
 * ranks on a device) and for boxes without RCCL; the messages of this path are latency-sized (<= 16 Q bytes). */
int pcreg_comm_init_host_staged(int rank, int world, const char* name);
int pcreg_comm_rank(int* rank, int* world);
int pcreg_comm_destroy(void);

/* pcreg_match_points_f32 with the MODEL rows split over the ranks: this rank passes rows
 * [m_lo, m_lo + M_local) of the M_total-row model and the whole (replicated) surface.  One all_gather of the
 * per-rank top-2 lists + merge, filters on every rank, Unique by the owner of the model row, one integer
 * all_reduce of the candidate table.  pairs: 1-based [surface row, GLOBAL model row], capacity Q. */
int pcreg_match_points_sharded_f32(const float* q, int Q, int ldq, const float* m_local, int M_local, int ldm,
                                   int m_lo, int M_total, float thr_abs, float max_ratio, int unique,
                                   uint32_t* pairs, int* P);

/* pcreg_ransac (built-in sampler, minPtNum 3) with the hypotheses of ONE registration split over the ranks:
 * every rank passes the same pts1 / pts2, scores iterNum / world hypotheses, one all_gather of the 112-byte
 * partial results agrees the first-maximum winner (ransac.m:70-72 on the GLOBAL hypothesis index). */
int pcreg_ransac_sharded(const double* pts1, const double* pts2, int n, int ld, const pcreg_ransac_opts* opts,
                         double T[16], int32_t* inlier_idx, int* n_inliers, int* num_success, int* max_inliers,
                         int* failed);

/* ---- on-disk formats of the drivers (host code, no device needed) --------------------------
 * .pcd clouds (pcread / pcwrite, completeExperimentFast.m:12-13,30,403): ascii, binary and
 * binary_compressed (LZF) files are read; x/y/z may be float or double, rgb/rgba is returned as
 * the packed 0x00RRGGBB word.  xyz is n x 3 column-major (ld >= n), like pointCloud.Location.
 * x/y/z may have any TYPE / SIZE of the format (I, U: 1, 2, 4, 8 bytes; F: 4, 8), each value converted
 * to float once, from its own type; fields this library does not know are skipped.
 * A file is untrusted input: a malformed one is refused with PCREG_E_ARG and a message that names
 * it, never read past its end, and no exception leaves these functions.  pcreg_pcd_info validates the
 * whole header (list lengths, types, sizes, COUNT >= 1, x / y / z present once, rgb / rgba one 4-byte
 * word, WIDTH * HEIGHT and POINTS within 0 .. INT_MAX) and reports a count only if the file is large
 * enough to hold that many points (binary: points * point size; ascii: two bytes a value;
 * binary_compressed: the two stored sizes against the header and the file), so a caller may allocate
 * from it.  Limits: a header line of at most 1 MiB, a COUNT of at most 16 Mi, a point of at most
 * 16 MiB.  pcreg_pcd_read refuses what only the payload shows: a corrupt LZF stream, an ascii token
 * that is no number (nan and inf are numbers), an ascii integer that its I / U field of that size
 * does not hold (a sign on a U value included). */
int pcreg_pcd_info(const char* path, int* n_points, int* has_rgb);
int pcreg_pcd_read(const char* path, float* xyz, int ld, uint32_t* rgb /* n or NULL */, int n);
int pcreg_pcd_write(const char* path, const float* xyz, int n, int ld, const uint32_t* rgb /* or NULL */,
                    int binary);

/* .mat descriptor caches (load, completeExperimentFast.m:21-24,312-313): one real numeric
 * variable of a Level-5 MAT-file (save -v6 / -v7, zlib-compressed elements included; v7.3 = HDF5
 * is not supported) as column-major doubles.  name NULL or "" = the first numeric array.  Call
 * with out == NULL for the shape (dimensions beyond the second are folded into cols).  The data
 * element may be of any numeric type (MATLAB stores whole-numbered doubles as the smallest integer
 * type that holds them); a 64-bit integer is rounded to double once.
 * Every tag is read inside the bytes that remain, and no exception leaves the function.  The file
 * as a whole is refused (PCREG_E_ARG, a message that names it) when it is no little-endian Level-5
 * file (version 4 and big-endian files included), when an element runs past its end, when a
 * compressed element does not inflate or does not begin with a matrix.  A variable is refused only
 * when it is the one asked for: a cell, struct, char, sparse, complex or object variable -- an
 * opaque string / table / datetime object included -- is passed over on the way to another, and so
 * is a numeric one that cannot be returned: fewer than two dimensions, a negative one, rows, cols
 * or rows * cols beyond INT_MAX, fewer data than the shape, data of no numeric type. */
int pcreg_mat_read_double(const char* path, const char* name, double* out, int* rows, int* cols);

#ifdef __cplusplus
}
#endif
#endif /* PCREG_H */
