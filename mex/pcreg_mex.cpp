// mex/pcreg_mex.cpp -- the MATLAB binding of libpcreg_hip.so (include/pcreg.h).
//
// One gateway, string-dispatched:   out = pcreg_mex('<command>', args...)
//   'estimateTransform', pts1, pts2                      -> T (4x4 or [])
//   'calcDists', T, pts1, pts2                           -> d (n x 1)
//   'ransac', pts1, pts2, coef, sample_idx|[], seed      -> T, inlierIdx, numSuccess, maxInliers, failed
//   'getMatches', descSurface, descModel, par            -> matches (P x 2 uint32)
//   'AlignPoints_KNN', pts, C1, C2                       -> pts_aligned, coeff_unambig, c
//   'getSpacialHistogramDescriptors', pts, sample_pts, options -> feat (V x 3), desc (V x 980)
//   'modelCreate', model (single M x 3) -> handle (uint64) | 'modelMatchPoints', handle, surface (single Q x 3), thrAbs, maxRatio, unique
//                                          -> pairs (P x 2 uint32) | 'modelDestroy', handle      (one model, many surfaces)
//   'modelKnn', handle, queries (single Q x 3), k        -> idx (Q x k int32, 1-based, 0 past M), D2 (Q x k single, squared)
//                                          (knnsearch(model, Y, 'K', k) against the handle; matlab/knnsearchModel.m)
//   'modelRange', handle, queries (single Q x 3), r      -> counts (Q x 1 int32), idx (total x 1 int32, 1-based), D2 (total x 1 single,
//                                          squared): query i's rows follow those of the queries before it, ordered by (distance, row)
//                                          (rangesearch(model, Y, r) against the handle; matlab/rangesearchModel.m)
//   'modelScore', handle, pts (single Q x 3), T (double 4 x 4 x B), maxDist -> nClose (B x 1 int32), sumD2 (B x 1 double), idx (Q x B
//                                          int32, 1-based, 0 for none), D2 (Q x B single, squared; Inf for none): per transform
//                                          the rows of pts with a model row within maxDist of [pts, 1] * T(:, :, b) and the sum of
//                                          their squared distances; an all-zero T(:, :, b) scores nothing; the last two outputs
//                                          are built only when asked for (matlab/scoreTransformsModel.m)
//   'modelRefit', handle, pts (single Q x 3), T (double 4 x 4 x B), maxDist, steps -> Tout (double 4 x 4 x B), nClose (B x 1 int32),
//                                          sumD2 (B x 1 double): every T(:, :, b) refitted `steps` times on the rows of pts with a
//                                          model row within maxDist of their moved place -- T <- T * estimateTransform(model rows,
//                                          moved points); a zero page where there is no fit (fewer than three pairs, an empty
//                                          estimateTransform, an all-zero T(:, :, b)); nClose / sumD2 are 'modelScore''s for the
//                                          transform that went into the last step (matlab/refitTransformsModel.m)
//   'modelRefitPlane', handle, pts (single Q x 3), T (double 4 x 4 x B), maxDist, steps, normals (single M x 3 | []), k -> Tout (double
//                                          4 x 4 x B), nClose (B x 1 int32), sumD2 (B x 1 double), nPlane (B x 1 int32), sumRes2 (B x 1
//                                          double): 'modelRefit' with the linearised point-to-plane step in estimateTransform's
//                                          place; normals by model row as 'modelNormals' returns them (a row with a NaN offers no
//                                          plane, the sign is immaterial), or [] to compute them once with k (3 .. 32); a zero
//                                          page where there is no fit (fewer than six planes, a direction the planes leave free, an
//                                          all-zero T(:, :, b)); the counts and sums are those of the transform that went into the
//                                          last step, sqrt(sumRes2 ./ double(nPlane)) its plane RMSE (matlab/refitPlaneModel.m)
//   'modelRefitGicp', handle, pts (single Q x 3), T (double 4 x 4 x B), maxDist, steps, normals (single M x 3 | []), ptsNormals (single
//                                          Q x 3 | []), k, epsilon -> Tout (double 4 x 4 x B), nClose (B x 1 int32), sumD2 (B x 1
//                                          double), nPairs (B x 1 int32), sumRes2 (B x 1 double): 'modelRefitPlane' with the
//                                          plane-to-plane (generalized ICP) step in its place; either set of normals may be [] to
//                                          compute it once with k (3 .. 32); epsilon in (0, 1] is the covariance along a normal; a
//                                          zero page where there is no fit (matlab/refitGicpModel.m)
//   'modelScoreTrimmed', 'modelRefitTrimmed', 'modelRefitPlaneTrimmed', 'modelRefitGicpTrimmed': the four commands above with keepRatio
//                                          (a double scalar in (0, 1]) after maxDist and two more outputs at the end, nWithin (B x 1
//                                          int32) and d2Cut (B x 1 single): of each transform's rows within maxDist only the closest
//                                          keepRatio share is kept (pcregistericp's InlierRatio; ties to the lower row of pts),
//                                          every other output is about the kept pairs, nWithin counts the pairs before the trim
//                                          and d2Cut is the largest kept squared distance, Inf where nothing is kept; 'modelScoreTrimmed'
//                                          has 0 / Inf at trimmed slots of idx / D2 (matlab/scoreTransformsTrimmedModel.m, refitTransformsTrimmedModel.m,
//                                          refitPlaneTrimmedModel.m, refitGicpTrimmedModel.m: the untrimmed wrappers' arguments and a trailing
//                                          'InlierRatio', rho)
//   'modelRefitCpd', handle, pts (single Q x 3), T (double 4 x 4 x B), sigma2 (double scalar | B x 1), outlier, steps -> Tout (double
//                                          4 x 4 x B), sigma2Out, Np, sumRes2, sumD2 (B x 1 double each), nLive (B x 1 int32): rigid
//                                          coherent-point-drift steps, every moved point softly against EVERY model row (B * Q * M
//                                          pairs a step: for downsampled clouds); sigma2 0 asks for the initial variance, outlier in
//                                          [0, 1); a zero page and sigma2Out 0 where there is no fit; sigma2Out is the variance AFTER
//                                          the last step, the sums and nLive are those of the transform that went into it
//                                          (matlab/refitCpdModel.m)
//   'modelCluster', handle, r | 'clusterPoints', pts (single M x 3), r -> label (M x 1 int32, the 1-based cluster of every row),
//                                          clOff (C + 1 int32 offsets), members (M x 1 int32, 1-based rows): cluster c is
//                                          members(clOff(c) + 1 : clOff(c + 1)), ascending; the connected components of the graph
//                                          "distance <= r", numbered by their smallest row (clusterPoints.m:16-45;
//                                          matlab/clusterPointsModel.m, matlab/clusterPointsFast.m)
//   'modelDbscan', handle, epsilon, minpts | 'dbscanPoints', pts (single M x 3), epsilon, minpts -> label (M x 1 int32, the 1-based
//                                          cluster of every row, -1 for noise), core (M x 1 uint8, 1 for a core row), clOff
//                                          (C + 1 int32 offsets), members (int32, 1-based rows, the clustered rows only): DBSCAN as
//                                          MATLAB's dbscan(X, epsilon, minpts) -- a row is core with at least minpts rows, itself
//                                          included, within epsilon; clusters numbered by their smallest core row; a border row
//                                          joins the smallest-numbered cluster among its core neighbours; always four outputs
//                                          (matlab/dbscanModel.m, matlab/dbscanFast.m)
//   'modelNormals', handle, k, viewpoint | 'pointNormals', pts (single M x 3), k, viewpoint -> normals (M x 3 single), variation
//                                          (M x 1 single): the normal of every row from its k nearest rows (3 <= k <= 32, the row
//                                          itself among them), the eigenvector of the smallest eigenvalue of their scatter in
//                                          double; viewpoint [] (the component of largest magnitude is made non-negative) or a
//                                          double 1 x 3 the normals point towards, always passed; variation = lambda_min / the
//                                          sum of the three eigenvalues, built only when asked for; NaN rows where there is no
//                                          normal (matlab/pcnormalsModel.m, matlab/pcnormalsFast.m)
//   'modelDenoise', handle, k, threshold | 'pointDenoise', pts (single M x 3), k, threshold -> inlierIndices (n x 1 uint32, 1-based,
//                                          ascending, as pcdenoise returns them), meanDist (M x 1 double), thr (double scalar):
//                                          pcdenoise(ptCloud, 'NumNeighbors', k, 'Threshold', threshold) -- meanDist the mean
//                                          distance of every row to its k nearest other rows (1 <= k <= 31), NaN for a row with a
//                                          NaN or Inf; thr = mean + threshold * std of the finite ones; a row is an inlier iff
//                                          meanDist <= thr; the last two outputs are built only when asked for
//                                          (matlab/pcdenoiseModel.m, matlab/pcdenoiseFast.m)
//   'modelFps', handle, K, start, stopD2 | 'pointFps', pts (single M x 3), K, start, stopD2 -> idx (n x 1 uint32, 1-based rows in
//                                          selection order), d2 (n x 1 single), label (M x 1 uint32), minD2 (M x 1 single), coverD2
//                                          (single scalar): farthest point sampling (pcreg_model_fps_f32) -- at most K rows (a
//                                          whole number >= 0), each the finite row farthest from all rows chosen before it; start a
//                                          1-based row, or 0 for the lowest finite row; stopD2 a single scalar >= 0 (Inf allowed), the
//                                          SQUARED distance at which the sampling stops early; d2 the squared distance of each
//                                          sample to the earlier ones (d2(1) = Inf); label the 1-based position in idx of the
//                                          nearest sample (0 for a row with a NaN or Inf) and minD2 the squared distance to it
//                                          (NaN there); single stays single; outputs past the first are built only when asked
//                                          for (matlab/farthestPointsModel.m, matlab/farthestPointsFast.m)
//   'modelFpfh', handle, k, normals (single M x 3 | []), kNormals, viewpoint | 'pointFpfh', pts (single M x 3), k, normals, kNormals,
//                                          viewpoint -> features (M x 33 double), spfh (M x 33 uint8):
//                                          extractFPFHFeatures(ptCloud, 'NumNeighbors', k) in this library's rule -- the FPFH
//                                          descriptor of every row from its k nearest rows (3 <= k <= 32, the row itself among
//                                          them) and a normal per row; normals by model row as 'modelNormals' returns them (THE
//                                          SIGN matters: orient them with a viewpoint), or [] to compute them in the call from the
//                                          kNormals nearest rows (3 .. 32, always passed) and the viewpoint ([] or double 1 x 3,
//                                          always passed); each of a row's three histograms adds up to 100 or is all zero, a row
//                                          with a NaN or Inf is NaN; spfh, the integer pair counts, is built only when asked for
//                                          (matlab/extractFPFHModel.m, matlab/extractFPFHFast.m)
//   'modelFpfhRadius', handle, r2, maxNeighbors, normals (single M x 3 | []), kNormals, viewpoint | 'pointFpfhRadius', pts (single
//                                          M x 3), r2, maxNeighbors, normals, kNormals, viewpoint -> features (M x 33 double), spfh
//                                          (M x 33 uint32), nNeighbors (M x 1 int32): extractFPFHFeatures(ptCloud, 'Radius', r) in
//                                          this library's rule (pcreg_model_fpfh_radius_f32) -- the FPFH descriptor of every row
//                                          from the rows within the radius and a normal per row; r2 a single scalar >= 0 (Inf
//                                          allowed), the SQUARED radius (the wrappers square the radius in double and round once:
//                                          single(r^2)); maxNeighbors a whole number >= 0, the n nearest rows within the radius
//                                          that count (0: all of them; 'NumNeighbors' beyond 32); normals, kNormals and viewpoint
//                                          as 'modelFpfh' takes them, always passed; at most 4 Mi rows; spfh, the integer pair
//                                          counts, and nNeighbors, the neighbours counted per row, are built only when asked for
//                                          (matlab/extractFPFHRadiusModel.m, matlab/extractFPFHRadiusFast.m)
//   'modelIss', handle, r2Salient, r2NonMax, threshold21, threshold32, minNeighbors | 'pointIss', pts (single M x 3), r2Salient, ... ->
//                                          keypoints (n x 1 uint32, 1-based, ascending), saliency (M x 1 double), eig (M x 3 double,
//                                          descending along a row), nNeighbors (M x 1 int32): detectISSFeatures(ptCloud, ...) in this
//                                          library's rule (pcreg_model_iss_f32) -- r2Salient and r2NonMax are single scalars, the
//                                          SQUARED radii (the wrappers square the radius in double and round once: single(r^2));
//                                          threshold21 / threshold32 finite doubles > 0; minNeighbors a whole number >= 1; all
//                                          always passed; the last three outputs are built only when asked for
//                                          (matlab/detectISSModel.m, matlab/detectISSFast.m)
//   'modelPlanes', handle, maxDistance, refVec, maxAngle, maxPlanes, nTrials, minInliers, seed, samples | 'pointPlanes', pts (single
//                                          M x 3), maxDistance, ... -> labels (M x 1 int32: plane p's rows carry p, 0 is no plane),
//                                          planes (n x 4 double: nx ny nz d), centres (n x 3 double), counts (n x 1 int32), rmse (n x 1
//                                          double), diag (maxPlanes x 3 double: every round's winning trial, 1-based and 0 for none, its
//                                          MSAC cost and its inlier count): pcfitplane and the fit / remove / fit-again loop in this
//                                          library's rule (pcreg_model_fit_planes_f32) -- maxDistance a single scalar (finite, normal,
//                                          > 0); refVec [] or a double 1 x 3; maxAngle a double scalar in RADIANS, in (0, pi/2] with a
//                                          refVec; maxPlanes 1 .. 64, nTrials 1 .. 2^20, minInliers >= 3 and seed >= 0 whole doubles;
//                                          samples [] or int32 3 x (nTrials * maxPlanes), 1-based rows, column p * nTrials + b the trial
//                                          b of round p; all always passed; outputs after the first are built only when asked for
//                                          (matlab/fitPlanesModel.m, matlab/fitPlanesFast.m, matlab/pcfitplaneFast.m)
//   'modelFitSpheres', handle, maxDistance, minRadius, maxRadius, maxSpheres, nTrials, minInliers, seed, samples | 'pointFitSpheres',
//                                          pts (single M x 3), maxDistance, ... -> labels (M x 1 int32: sphere p's rows carry p, 0 is no
//                                          sphere), spheres (n x 4 double: cx cy cz R), counts (n x 1 int32), rmse (n x 1 double),
//                                          refitUsed (n x 1 int32: 0 where the round kept its winning trial's own sphere), diag
//                                          (maxSpheres x 3 double: every round's winning trial, 1-based and 0 for none, its MSAC cost and
//                                          its inlier count): pcfitsphere and the fit / remove / fit-again loop in this library's rule
//                                          (pcreg_model_fit_spheres_f32) -- maxDistance a single scalar (finite, normal, > 0); minRadius
//                                          and maxRadius single scalars, 0 <= minRadius <= maxRadius, maxRadius may be Inf; maxSpheres
//                                          1 .. 64, nTrials 1 .. 2^20, minInliers >= 4 and seed >= 0 whole doubles; samples [] or int32
//                                          4 x (nTrials * maxSpheres), 1-based rows, column p * nTrials + b the trial b of round p; all
//                                          always passed; outputs after the first are built only when asked for
//                                          (matlab/fitSpheresModel.m, matlab/fitSpheresFast.m, matlab/pcfitsphereFast.m)
//   'modelFitCylinders', handle, maxDistance, minRadius, maxRadius, refVec, maxAngle, normals, kNormals, maxCylinders, nTrials,
//                                          minInliers, seed, samples | 'pointFitCylinders', pts (single M x 3), maxDistance, ... ->
//                                          labels (M x 1 int32: cylinder p's rows carry p, 0 is no cylinder), cylinders (n x 7 double:
//                                          cx cy cz wx wy wz R), extents (n x 2 double: h_lo h_hi along the axis from the centre),
//                                          counts (n x 1 int32), rmse (n x 1 double), refitUsed (n x 1 int32: 0 where the round kept its
//                                          winning trial's own cylinder), diag (maxCylinders x 3 double: every round's winning trial,
//                                          1-based and 0 for none, its MSAC cost and its inlier count): pcfitcylinder and the fit /
//                                          remove / fit-again loop in this library's rule (pcreg_model_fit_cylinders_f32) --
//                                          maxDistance, minRadius, maxRadius as in 'modelFitSpheres'; refVec [] or a double 1 x 3 (finite,
//                                          not all zero) and maxAngle a double scalar in RADIANS, in (0, pi / 2] when refVec is given:
//                                          they bound the axis; normals single M x 3 or [] (then computed in the call from the kNormals
//                                          nearest rows, a whole double 3 .. 32, always passed); maxCylinders 1 .. 64, nTrials 1 .. 2^20,
//                                          minInliers >= 4 and seed >= 0 whole doubles; samples [] or int32 2 x (nTrials * maxCylinders),
//                                          1-based rows, column p * nTrials + b the trial b of round p; all always passed; outputs after
//                                          the first are built only when asked for (matlab/fitCylindersModel.m,
//                                          matlab/fitCylindersFast.m, matlab/pcfitcylinderFast.m)
//   'uniqueRows3', A (double n x 3)                        -> ia (u x 1 double, 1-based): [C, ia] = unique(A, 'rows'), C = A(ia, :)
//                                          (rows ordered by column 1, 2, 3; first occurrences; NaN refused; matlab/uniqueRowsFast.m)
//   'aggregateMatches', pts1, pts2 (double n x 3 each)   -> pts1u, pts2u (u x 3), ia (u x 1 double, 1-based rows of the input):
//                                          completeExperiment.m:440-443, unique over pts1 then over pts2 (matlab/aggregateMatches.m)
//   'downsampleGrid', pts (single n x 3), gridStep          -> ptsOut (u x 3 single), counts (u x 1 int32), labels (n x 1 int32):
//                                          pcdownsample(pc, 'gridAverage', gridStep) -- the mean of the rows of every occupied
//                                          cell floor((x - min) / gridStep), cells and sums in double, the voxels in ascending
//                                          (c1, c2, c3) order; counts the rows of every voxel, labels the 1-based output row of
//                                          every input row, 0 for a row with a NaN or Inf; the last two are built only when asked
//                                          for; the input keeps its class, a double cloud is refused (matlab/pcdownsampleFast.m)
//   'ndtCreate', pts (single n x 3), step, minPoints        -> handle (uint64), nVoxels, nGaussians: the cloud summarised ONCE as one
//                                          Gaussian per voxel of gridStep `step` with at least minPoints (>= 3) rows -- the table NDT
//                                          steps refine against (pcreg_ndt_create; matlab/ndtModel.m) | 'ndtDestroy', handle
//   'ndtRefit', handle, pts (single Q x 3), T (double 4 x 4 x B), neighbors (1 | 7), outlierRatio (in [0, 1)), steps -> Tout (double
//                                          4 x 4 x B), nPairs (B x 1 int32), sumE (B x 1 double): B transforms refined by `steps`
//                                          Gauss-Newton NDT steps -- each moved point against the Gaussian of its voxel (and of its
//                                          six face neighbours), no nearest-row search; a zero page where there is no fit; the
//                                          counts and sums are those of the transform that went into the last step.  A step, not
//                                          pcregisterndt's policy (matlab/refitNdtModel.m, matlab/refitNdtFast.m)
//   'descCreate', desc (double n x D) -> handle (uint64) | 'getMatchesOnSet', hSurface, hModel, int32 rows | [], par -> matches
//                                          | 'descDestroy', handle        (one surface set, many row subsets of one model set)
//   'getMatchesSegmented', descSurface, descModel, int32 rows, int32 segOff, par | 'getMatchesSegmentedOnSet', hSurface, hModel, ...
//                                          -> pairs, nPairs                (every sphere of the sweep in one call)
//   'ransacBatched', pts1, pts2, int32 offsets, coef, sample_idx|[], seed -> T (4x4xB), inlierIdx, nInliers, numSuccess, maxInliers, failed
//   'fgrBatched', pts1, pts2, int32 offsets, opts, int32 tupleIdx|[], T0|[] -> T (4x4xB), inlierIdx, stats (B x 9), kept (uint8)   (fast global registration; matlab/fgrBatched.m, pcregisterfgrFast.m)
//   'sphereCounts', featModel, centres, R -> counts | 'sphereSweep', hSurface, hModel, featSurface, featModel, centres, int32 numDesc,
//       R_desc, par, putativeThresh, coef, seed -> modelRows, pairs, nPairs, trial, T, numSuccess, maxInliers, failed   (completeExperimentFast.m:52-224)
//   'sphereModelCreate', hModel, featModel, centres, int32 numDesc, R_desc -> handle, modelRows | 'sphereSweepOnModel', hSphereModel, hSurface,
//       featSurface, S, par, putativeThresh, coef, seed -> pairs, nPairs, trial, T, numSuccess, maxInliers, failed | 'sphereModelDestroy', handle
//   'finalStageLimits', pts, T (4x4xK, invertTF of each transCur) -> limits (K x 6) | 'finalStage', hModelNoLRF, featModel_noLRF, pts,
//       locs, T, keypoints, int32 kpOff, descOpt, par, R_desc, maxDist -> numKeypoints, numDesc, numMatches, numClose, precisions,
//       best (1-based), T_refine ([] if empty), ptsFinal, pairs         (completeExperimentFast.m:280-394 after clusterPoints)
//   'getLocalPoints', pts, R, c, min_points, max_points   -> pts_sphere, dists
//   'setDevice', ordinal | 'commId' -> id | 'commInit', rank, world, id | 'commDestroy'     (one worker per GPU)
//   'matchPointsSharded', surface, modelRows, m_lo, M_total, thrAbs, maxRatio, unique     -> pairs (P x 2 uint32, global model rows)
//   'ransacSharded', pts1, pts2, coef, seed                -> T, inlierIdx, numSuccess, maxInliers, failed
// The shim only unpacks mxArrays: MATLAB's column-major doubles go straight through
// (ld = number of rows).  It never throws with C++ objects alive:
// errors are collected as codes and raised by one mexErrMsgIdAndTxt at the very end.
//
// Build (on a machine with MATLAB; neither the build container nor the GPU box has one):
//   mex -I../include mex/pcreg_mex.cpp -L../pcreg_amd -lpcreg_hip -output matlab/pcreg_mex
// This file is compile-gated on mex.h and is NOT part of libpcreg_hip.so.
#if __has_include("mex.h")
#include "mex.h"
#include <cstdint>
#include <cstring>
#include <string>
#include <cmath>
#include <vector>
#include "../include/pcreg.h"

static double field(const mxArray* s, const char* name, double dflt, bool* missing = nullptr) {
    const mxArray* f = mxIsStruct(s) ? mxGetField(s, 0, name) : nullptr;
    if (!f) { if (missing) *missing = true; return dflt; }
    if (mxIsChar(f)) return dflt;
    return mxGetScalar(f);
}
static bool field_is(const mxArray* s, const char* name, const char* value) {
    const mxArray* f = mxIsStruct(s) ? mxGetField(s, 0, name) : nullptr;
    if (!f || !mxIsChar(f)) return false;
    char buf[64]; mxGetString(f, buf, sizeof buf);
    return strcmp(buf, value) == 0;
}

// r of the radius commands: a real double or single scalar >= 0 (NaN refused)
static bool radius_ok(const mxArray* a) {
    return (mxIsDouble(a) || mxIsSingle(a)) && mxGetM(a) * mxGetN(a) == 1 && mxGetScalar(a) >= 0.0;
}
// keepRatio of the trimmed commands: a real double scalar in (0, 1] (NaN refused)
static bool ratio_ok(const mxArray* a) {
    return mxIsDouble(a) && mxGetM(a) * mxGetN(a) == 1 && mxGetScalar(a) > 0.0 && mxGetScalar(a) <= 1.0;
}
// steps of the refit commands: a whole number 1 .. 1e6 as a double scalar
static bool steps_ok(const mxArray* a) {
    return mxIsDouble(a) && mxGetM(a) * mxGetN(a) == 1 && mxGetScalar(a) >= 1.0 && mxGetScalar(a) <= 1e6 && mxGetScalar(a) == (double)(int)mxGetScalar(a);
}
// pts (single Q x 3) and T (double 4 x 4 x B, or empty) of the scoring and refit commands
static bool pts_t_ok(const mxArray* pts, const mxArray* T) {
    return mxIsSingle(pts) && mxGetN(pts) == 3 && mxIsDouble(T) && (mxGetM(T) == 4 || mxIsEmpty(T)) && mxGetN(T) % 4 == 0;
}
// the three outputs of 'modelCluster' / 'clusterPoints': label (M x 1 int32, 1-based), clOff (C + 1 int32), members (M x 1 int32,
// 1-based); single(r) is squared once, in single.  Nothing is left allocated on an error.
static int cluster_on_handle(pcreg_model* h, float r, mxArray* out[3]) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    mxArray* ol = mxCreateNumericMatrix((size_t)M, 1, mxINT32_CLASS, mxREAL);
    mxArray* om = mxCreateNumericMatrix((size_t)M, 1, mxINT32_CLASS, mxREAL);
    mxArray* bo = mxCreateNumericMatrix((size_t)M + 1, 1, mxINT32_CLASS, mxREAL);
    int32_t *lab = (int32_t*)mxGetData(ol), *mem = (int32_t*)mxGetData(om), *off = (int32_t*)mxGetData(bo);
    int32_t nc = 0;
    rc = pcreg_model_cluster_f32(h, r * r, lab, &nc, off, mem);
    if (rc == PCREG_OK) {
        for (int i = 0; i < M; ++i) { lab[i] += 1; mem[i] += 1; }
        out[0] = ol; out[2] = om;
        out[1] = mxCreateNumericMatrix((size_t)nc + 1, 1, mxINT32_CLASS, mxREAL);
        memcpy(mxGetData(out[1]), off, ((size_t)nc + 1) * sizeof(int32_t));
    } else { mxDestroyArray(ol); mxDestroyArray(om); }
    mxDestroyArray(bo);
    return rc;
}

// the four outputs of 'modelDbscan' / 'dbscanPoints': label (M x 1 int32, 1-based, -1 for noise), core (M x 1 uint8, 0 / 1), clOff
// (C + 1 int32), members (int32, 1-based, the clustered rows only); single(epsilon) is squared once, in single.  Nothing is left
// allocated on an error.
static int dbscan_on_handle(pcreg_model* h, float eps, int minpts, mxArray* out[4]) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    mxArray* ol = mxCreateNumericMatrix((size_t)M, 1, mxINT32_CLASS, mxREAL);
    mxArray* oc = mxCreateNumericMatrix((size_t)M, 1, mxUINT8_CLASS, mxREAL);
    mxArray* bm = mxCreateNumericMatrix((size_t)M, 1, mxINT32_CLASS, mxREAL);
    mxArray* bo = mxCreateNumericMatrix((size_t)M + 1, 1, mxINT32_CLASS, mxREAL);
    int32_t *lab = (int32_t*)mxGetData(ol), *mem = (int32_t*)mxGetData(bm), *off = (int32_t*)mxGetData(bo);
    int32_t nc = 0;
    rc = pcreg_model_dbscan_f32(h, eps * eps, minpts, lab, &nc, (uint8_t*)mxGetData(oc), nullptr, off, mem);
    if (rc == PCREG_OK) {
        for (int i = 0; i < M; ++i) if (lab[i] >= 0) lab[i] += 1;
        out[0] = ol; out[1] = oc;
        out[2] = mxCreateNumericMatrix((size_t)nc + 1, 1, mxINT32_CLASS, mxREAL);
        memcpy(mxGetData(out[2]), off, ((size_t)nc + 1) * sizeof(int32_t));
        const int n = off[nc];
        out[3] = mxCreateNumericMatrix((size_t)n, 1, mxINT32_CLASS, mxREAL);
        int32_t* om = (int32_t*)mxGetData(out[3]);
        for (int i = 0; i < n; ++i) om[i] = mem[i] + 1;
    } else { mxDestroyArray(ol); mxDestroyArray(oc); }
    mxDestroyArray(bm); mxDestroyArray(bo);
    return rc;
}

// k and viewpoint of the normals commands: a real double scalar, whole, 3 .. PCREG_KNN_MAX_K; [] or three doubles
static bool normals_k_ok(const mxArray* a) {
    return mxIsDouble(a) && mxGetM(a) * mxGetN(a) == 1 && mxGetScalar(a) >= 3.0 && mxGetScalar(a) <= (double)PCREG_KNN_MAX_K &&
           mxGetScalar(a) == (double)(int)mxGetScalar(a);
}
// a real double scalar that is a whole number in [lo, hi] (NaN refused)
static bool whole_scalar_ok(const mxArray* a, double lo, double hi) {
    return mxIsDouble(a) && mxGetM(a) * mxGetN(a) == 1 && mxGetScalar(a) >= lo && mxGetScalar(a) <= hi && mxGetScalar(a) == (double)(int)mxGetScalar(a);
}
static bool viewpoint_ok(const mxArray* a) { return mxIsEmpty(a) || (mxIsDouble(a) && mxGetM(a) * mxGetN(a) == 3); }
// the outputs of 'modelNormals' / 'pointNormals': normals (M x 3 single) and, with want_var, variation (M x 1 single).  Nothing is
// left allocated on an error.
static int normals_on_handle(pcreg_model* h, int k, const mxArray* vp, bool want_var, mxArray* out[2]) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    mxArray* on = mxCreateNumericMatrix((size_t)M, 3, mxSINGLE_CLASS, mxREAL);
    mxArray* ov = want_var ? mxCreateNumericMatrix((size_t)M, 1, mxSINGLE_CLASS, mxREAL) : nullptr;
    rc = pcreg_model_normals_f32(h, k, mxIsEmpty(vp) ? nullptr : mxGetPr(vp), (float*)mxGetData(on), M > 0 ? M : 1,
                                 ov ? (float*)mxGetData(ov) : nullptr);
    if (rc == PCREG_OK) { out[0] = on; out[1] = ov; }
    else { mxDestroyArray(on); if (ov) mxDestroyArray(ov); }
    return rc;
}

// the outputs of 'modelFpfh' / 'pointFpfh': features (M x 33 double) and, with want_spfh, the counts (M x 33 uint8; the library's
// rows of 33 are turned into MATLAB's columns).  nrm: single M x 3 or [].  Nothing is left allocated on an error; *usage is set when
// the normals have another number of rows than the model.
static int fpfh_on_handle(pcreg_model* h, int k, const mxArray* nrm, int k_normals, const mxArray* vp, bool want_spfh, mxArray* out[2],
                          const char** usage) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    const bool given = !mxIsEmpty(nrm);
    if (given && (int)mxGetM(nrm) != M) { *usage = "Fpfh: normals must have one row per row of the cloud"; return PCREG_OK; }
    mxArray* of = mxCreateDoubleMatrix((size_t)M, 33, mxREAL);
    mxArray* tc = want_spfh ? mxCreateNumericMatrix(33, (size_t)(M > 0 ? M : 1), mxUINT8_CLASS, mxREAL) : nullptr;
    rc = pcreg_model_fpfh_f32(h, k, given ? (const float*)mxGetData(nrm) : nullptr, M > 0 ? M : 1, k_normals, mxIsEmpty(vp) ? nullptr : mxGetPr(vp),
                              mxGetPr(of), M > 0 ? M : 1, tc ? (uint8_t*)mxGetData(tc) : nullptr);
    if (rc == PCREG_OK) {
        out[0] = of;
        if (tc) {
            out[1] = mxCreateNumericMatrix((size_t)M, 33, mxUINT8_CLASS, mxREAL);
            const uint8_t* src = (const uint8_t*)mxGetData(tc);
            uint8_t* dst = (uint8_t*)mxGetData(out[1]);
            for (int i = 0; i < M; ++i)
                for (int b = 0; b < 33; ++b) dst[(size_t)i + (size_t)b * (size_t)M] = src[(size_t)i * 33 + b];
        }
    } else mxDestroyArray(of);
    if (tc) mxDestroyArray(tc);
    return rc;
}

// r2 and maxNeighbors of the radius FPFH commands: a real single scalar >= 0 (Inf allowed, NaN not); a real double scalar, whole,
// 0 .. 2^31 - 1
static bool fpfh_radius_args_ok(const mxArray* r2, const mxArray* n) {
    if (!mxIsSingle(r2) || mxGetM(r2) * mxGetN(r2) != 1 || !(*(const float*)mxGetData(r2) >= 0.0f)) return false;
    return mxIsDouble(n) && mxGetM(n) * mxGetN(n) == 1 && mxGetScalar(n) >= 0.0 && mxGetScalar(n) <= 2147483647.0 &&
           mxGetScalar(n) == (double)(int)mxGetScalar(n);
}
// the outputs of 'modelFpfhRadius' / 'pointFpfhRadius': features (M x 33 double), with nout > 1 the counts (M x 33 uint32; the
// library's rows of 33 are turned into MATLAB's columns), with nout > 2 nNeighbors (M x 1 int32).  nrm: single M x 3 or [].  Nothing is
// left allocated on an error; *usage is set when the normals have another number of rows than the model.
static int fpfh_radius_on_handle(pcreg_model* h, float r2, int max_neighbors, const mxArray* nrm, int k_normals, const mxArray* vp, int nout,
                                 mxArray* out[3], const char** usage) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    const bool given = !mxIsEmpty(nrm);
    if (given && (int)mxGetM(nrm) != M) { *usage = "FpfhRadius: normals must have one row per row of the cloud"; return PCREG_OK; }
    mxArray* of = mxCreateDoubleMatrix((size_t)M, 33, mxREAL);
    mxArray* tc = nout > 1 ? mxCreateNumericMatrix(33, (size_t)(M > 0 ? M : 1), mxUINT32_CLASS, mxREAL) : nullptr;
    mxArray* on = nout > 2 ? mxCreateNumericMatrix((size_t)M, 1, mxINT32_CLASS, mxREAL) : nullptr;
    rc = pcreg_model_fpfh_radius_f32(h, r2, max_neighbors, given ? (const float*)mxGetData(nrm) : nullptr, M > 0 ? M : 1, k_normals,
                                     mxIsEmpty(vp) ? nullptr : mxGetPr(vp), mxGetPr(of), M > 0 ? M : 1, tc ? (uint32_t*)mxGetData(tc) : nullptr,
                                     on ? (int32_t*)mxGetData(on) : nullptr);
    if (rc == PCREG_OK) {
        out[0] = of;
        if (tc) {
            out[1] = mxCreateNumericMatrix((size_t)M, 33, mxUINT32_CLASS, mxREAL);
            const uint32_t* src = (const uint32_t*)mxGetData(tc);
            uint32_t* dst = (uint32_t*)mxGetData(out[1]);
            for (int i = 0; i < M; ++i)
                for (int b = 0; b < 33; ++b) dst[(size_t)i + (size_t)b * (size_t)M] = src[(size_t)i * 33 + b];
        }
        out[2] = on;
    } else { mxDestroyArray(of); if (on) mxDestroyArray(on); }
    if (tc) mxDestroyArray(tc);
    return rc;
}

// k and threshold of the denoise commands: a real double scalar, whole, 1 .. PCREG_KNN_MAX_K - 1; a finite real double scalar >= 0
static bool denoise_k_ok(const mxArray* a) {
    return mxIsDouble(a) && mxGetM(a) * mxGetN(a) == 1 && mxGetScalar(a) >= 1.0 && mxGetScalar(a) <= (double)(PCREG_KNN_MAX_K - 1) &&
           mxGetScalar(a) == (double)(int)mxGetScalar(a);
}
static bool denoise_t_ok(const mxArray* a) {
    return mxIsDouble(a) && mxGetM(a) * mxGetN(a) == 1 && mxGetScalar(a) >= 0.0 && mxGetScalar(a) <= 1.7976931348623157e308;
}
// the outputs of 'modelDenoise' / 'pointDenoise': inlierIndices (n x 1 uint32, 1-based), and with nout > 1 meanDist (M x 1 double),
// with nout > 2 thr.  Nothing is left allocated on an error.
static int denoise_on_handle(pcreg_model* h, int k, double t, int nout, mxArray* out[3]) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    mxArray* ti = mxCreateNumericMatrix((size_t)(M > 0 ? M : 1), 1, mxINT32_CLASS, mxREAL);
    mxArray* om = nout > 1 ? mxCreateDoubleMatrix((size_t)M, 1, mxREAL) : nullptr;
    int32_t n = 0;
    double stats[4] = {0.0, 0.0, 0.0, 0.0};
    rc = pcreg_model_denoise_f32(h, k, t, om && M > 0 ? mxGetPr(om) : nullptr, (int32_t*)mxGetData(ti), &n, stats);
    if (rc == PCREG_OK) {
        out[0] = mxCreateNumericMatrix((size_t)n, 1, mxUINT32_CLASS, mxREAL);
        const int32_t* src = (const int32_t*)mxGetData(ti);
        uint32_t* dst = (uint32_t*)mxGetData(out[0]);
        for (int32_t i = 0; i < n; ++i) dst[i] = (uint32_t)src[i] + 1u;
        out[1] = om;
        if (nout > 2) out[2] = mxCreateDoubleScalar(stats[0]);
    } else if (om) mxDestroyArray(om);
    mxDestroyArray(ti);
    return rc;
}

// K, start and stopD2 of the sampling commands, a[0 .. 2]: two whole double scalars 0 .. 2^31 - 1 (start is 1-based, 0 = the lowest
// finite row), a single scalar >= 0 and not NaN
static bool fps_args_ok(const mxArray* const* a) {
    return whole_scalar_ok(a[0], 0.0, 2147483647.0) && whole_scalar_ok(a[1], 0.0, 2147483647.0) && mxIsSingle(a[2]) &&
           mxGetM(a[2]) * mxGetN(a[2]) == 1 && *(const float*)mxGetData(a[2]) >= 0.0f;
}
// the outputs of 'modelFps' / 'pointFps': idx (n x 1 uint32, 1-based) and, as far as nout asks, d2 (n x 1 single), label (M x 1
// uint32), minD2 (M x 1 single), coverD2 (single scalar).  Nothing is left allocated on an error.
static int fps_on_handle(pcreg_model* h, int K, int start1, float stop_d2, int nout, mxArray* out[5]) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    mxArray* ti = mxCreateNumericMatrix((size_t)(K > 0 ? K : 1), 1, mxINT32_CLASS, mxREAL);
    mxArray* td = nout > 1 ? mxCreateNumericMatrix((size_t)(K > 0 ? K : 1), 1, mxSINGLE_CLASS, mxREAL) : nullptr;
    mxArray* ol = nout > 2 ? mxCreateNumericMatrix((size_t)M, 1, mxUINT32_CLASS, mxREAL) : nullptr;      // (a label is never negative)
    mxArray* om = nout > 3 ? mxCreateNumericMatrix((size_t)M, 1, mxSINGLE_CLASS, mxREAL) : nullptr;
    int32_t n = 0;
    float cover = 0.0f;
    rc = pcreg_model_fps_f32(h, K, start1 - 1, stop_d2, (int32_t*)mxGetData(ti), td ? (float*)mxGetData(td) : nullptr, &n, &cover,
                             om && M > 0 ? (float*)mxGetData(om) : nullptr, ol && M > 0 ? (int32_t*)mxGetData(ol) : nullptr);
    if (rc == PCREG_OK) {
        out[0] = mxCreateNumericMatrix((size_t)n, 1, mxUINT32_CLASS, mxREAL);
        const int32_t* src = (const int32_t*)mxGetData(ti);
        uint32_t* dst = (uint32_t*)mxGetData(out[0]);
        for (int32_t i = 0; i < n; ++i) dst[i] = (uint32_t)src[i] + 1u;
        if (td) {
            out[1] = mxCreateNumericMatrix((size_t)n, 1, mxSINGLE_CLASS, mxREAL);
            if (n > 0) memcpy(mxGetData(out[1]), mxGetData(td), sizeof(float) * (size_t)n);
        }
        out[2] = ol; out[3] = om;
        if (nout > 4) { out[4] = mxCreateNumericMatrix(1, 1, mxSINGLE_CLASS, mxREAL); *(float*)mxGetData(out[4]) = cover; }
    } else { if (ol) mxDestroyArray(ol); if (om) mxDestroyArray(om); }
    mxDestroyArray(ti);
    if (td) mxDestroyArray(td);
    return rc;
}

// the parameters of the ISS commands, prhs[0 .. 4]: two single scalars (finite, normal, > 0), two double scalars (finite, > 0), a
// whole double >= 1
static bool iss_args_ok(const mxArray* const* a) {
    for (int i = 0; i < 2; ++i) {
        if (!mxIsSingle(a[i]) || mxGetM(a[i]) * mxGetN(a[i]) != 1) return false;
        const float v = *(const float*)mxGetData(a[i]);
        if (!(v >= 1.17549435e-38f && v <= 3.40282347e+38f)) return false;
    }
    for (int i = 2; i < 4; ++i)
        if (!mxIsDouble(a[i]) || mxGetM(a[i]) * mxGetN(a[i]) != 1 || !(mxGetScalar(a[i]) > 0.0 && mxGetScalar(a[i]) <= 1.7976931348623157e308)) return false;
    return mxIsDouble(a[4]) && mxGetM(a[4]) * mxGetN(a[4]) == 1 && mxGetScalar(a[4]) >= 1.0 && mxGetScalar(a[4]) <= 2147483647.0 &&
           mxGetScalar(a[4]) == (double)(int)mxGetScalar(a[4]);
}
// the outputs of 'modelIss' / 'pointIss': keypoints (n x 1 uint32, 1-based), and with nout > 1 saliency (M x 1 double), with nout > 2
// eig (M x 3 double: the library's rows transposed into MATLAB's columns), with nout > 3 nNeighbors (M x 1 int32).  Nothing is left
// allocated on an error.
static int iss_on_handle(pcreg_model* h, const mxArray* const* a, int nout, mxArray* out[4]) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    const size_t R = (size_t)(M > 0 ? M : 1);
    mxArray* tk = mxCreateNumericMatrix(R, 1, mxINT32_CLASS, mxREAL);
    mxArray* te = nout > 2 ? mxCreateDoubleMatrix(3, R, mxREAL) : nullptr;      // [M][3] row-major is 3 x M column-major
    mxArray* os = mxCreateDoubleMatrix((size_t)M, 1, mxREAL);
    mxArray* on = mxCreateNumericMatrix((size_t)M, 1, mxINT32_CLASS, mxREAL);
    int32_t n = 0;
    rc = pcreg_model_iss_f32(h, *(const float*)mxGetData(a[0]), *(const float*)mxGetData(a[1]), mxGetScalar(a[2]), mxGetScalar(a[3]),
                             (int)mxGetScalar(a[4]), M > 0 ? (int32_t*)mxGetData(on) : nullptr, te ? mxGetPr(te) : nullptr,
                             M > 0 ? mxGetPr(os) : nullptr, (int32_t*)mxGetData(tk), &n);
    if (rc == PCREG_OK) {
        out[0] = mxCreateNumericMatrix((size_t)n, 1, mxUINT32_CLASS, mxREAL);
        const int32_t* src = (const int32_t*)mxGetData(tk);
        uint32_t* dst = (uint32_t*)mxGetData(out[0]);
        for (int32_t i = 0; i < n; ++i) dst[i] = (uint32_t)src[i] + 1u;
        if (nout > 2) {
            out[2] = mxCreateDoubleMatrix((size_t)M, 3, mxREAL);
            const double* e = mxGetPr(te);
            double* d = mxGetPr(out[2]);
            for (int c = 0; c < 3; ++c)
                for (int i = 0; i < M; ++i) d[(size_t)i + (size_t)c * (size_t)M] = e[(size_t)i * 3 + c];
        }
    }
    if (rc == PCREG_OK && nout > 1) out[1] = os; else mxDestroyArray(os);
    if (rc == PCREG_OK && nout > 3) out[3] = on; else mxDestroyArray(on);
    if (te) mxDestroyArray(te);
    mxDestroyArray(tk);
    return rc;
}

// the parameters of the plane commands, prhs[0 .. 7]: maxDistance (single scalar, finite, normal, > 0), refVec ([] or double 1 x 3, finite, not zero),
// maxAngle (double scalar), maxPlanes, nTrials, minInliers, seed (whole doubles in range), samples ([] or int32 3 x nTrials * maxPlanes)
static bool whole_in(const mxArray* a, double lo, double hi) {
    if (!mxIsDouble(a) || mxGetM(a) * mxGetN(a) != 1) return false;
    const double v = mxGetScalar(a);
    return v >= lo && v <= hi && v == std::floor(v);
}
static bool planes_args_ok(const mxArray* const* a) {
    if (!mxIsSingle(a[0]) || mxGetM(a[0]) * mxGetN(a[0]) != 1) return false;
    const float t = *(const float*)mxGetData(a[0]);
    if (!(t >= 1.17549435e-38f && t <= 3.40282347e+38f)) return false;
    if (!(mxIsEmpty(a[1]) || (mxIsDouble(a[1]) && mxGetM(a[1]) * mxGetN(a[1]) == 3))) return false;
    if (!mxIsEmpty(a[1])) {                                       // finite and not all zero
        const double* r = mxGetPr(a[1]);
        for (int c = 0; c < 3; ++c) if (!(std::fabs(r[c]) <= 1.7976931348623157e308)) return false;
        if (r[0] == 0.0 && r[1] == 0.0 && r[2] == 0.0) return false;
    }
    if (!mxIsDouble(a[2]) || mxGetM(a[2]) * mxGetN(a[2]) != 1) return false;
    if (!mxIsEmpty(a[1]) && !(mxGetScalar(a[2]) > 0.0 && mxGetScalar(a[2]) <= 1.5707963267948966)) return false;
    if (!whole_in(a[3], 1.0, 64.0) || !whole_in(a[4], 1.0, 1048576.0) || !whole_in(a[5], 3.0, 2147483647.0) ||
        !whole_in(a[6], 0.0, 9007199254740992.0))
        return false;
    if (mxIsEmpty(a[7])) return true;
    return mxIsInt32(a[7]) && mxGetM(a[7]) == 3 && mxGetN(a[7]) == (size_t)mxGetScalar(a[3]) * (size_t)mxGetScalar(a[4]);
}
// the outputs of 'modelPlanes' / 'pointPlanes' (see the head of this file).  Nothing is left allocated on an error.
static int planes_on_handle(pcreg_model* h, const mxArray* const* a, int nout, mxArray* out[6]) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    const int P = (int)mxGetScalar(a[3]);
    mxArray* ol = mxCreateNumericMatrix((size_t)M, 1, mxINT32_CLASS, mxREAL);
    std::vector<double> planes(4 * (size_t)P), centres(3 * (size_t)P), rmse((size_t)P);
    std::vector<int32_t> counts((size_t)P), bt((size_t)P), bn((size_t)P);
    std::vector<int64_t> bc((size_t)P);
    int32_t n = 0;
    rc = pcreg_model_fit_planes_f32(h, *(const float*)mxGetData(a[0]), mxIsEmpty(a[1]) ? nullptr : mxGetPr(a[1]), mxGetScalar(a[2]), P,
                                    (int)mxGetScalar(a[4]), (int)mxGetScalar(a[5]), (uint64_t)mxGetScalar(a[6]),
                                    mxIsEmpty(a[7]) ? nullptr : (const int32_t*)mxGetData(a[7]), M > 0 ? (int32_t*)mxGetData(ol) : nullptr,
                                    planes.data(), centres.data(), counts.data(), rmse.data(), &n, bt.data(), bc.data(), bn.data());
    if (rc != PCREG_OK) { mxDestroyArray(ol); return rc; }
    out[0] = ol;
    if (nout > 1) {                                               // the library's rows transposed into MATLAB's columns
        out[1] = mxCreateDoubleMatrix((size_t)n, 4, mxREAL);
        for (int c = 0; c < 4; ++c) for (int i = 0; i < n; ++i) mxGetPr(out[1])[(size_t)i + (size_t)c * (size_t)n] = planes[(size_t)i * 4 + c];
    }
    if (nout > 2) {
        out[2] = mxCreateDoubleMatrix((size_t)n, 3, mxREAL);
        for (int c = 0; c < 3; ++c) for (int i = 0; i < n; ++i) mxGetPr(out[2])[(size_t)i + (size_t)c * (size_t)n] = centres[(size_t)i * 3 + c];
    }
    if (nout > 3) {
        out[3] = mxCreateNumericMatrix((size_t)n, 1, mxINT32_CLASS, mxREAL);
        for (int i = 0; i < n; ++i) ((int32_t*)mxGetData(out[3]))[i] = counts[(size_t)i];
    }
    if (nout > 4) {
        out[4] = mxCreateDoubleMatrix((size_t)n, 1, mxREAL);
        for (int i = 0; i < n; ++i) mxGetPr(out[4])[i] = rmse[(size_t)i];
    }
    if (nout > 5) {
        out[5] = mxCreateDoubleMatrix((size_t)P, 3, mxREAL);
        double* d = mxGetPr(out[5]);
        const bool ran_more = n < P;                              // round n ran too and ended the extraction: its diagnostics are real
        for (int i = 0; i < P; ++i) {
            const bool ran = i < n || (ran_more && i == n && M > 0);
            d[i] = ran ? (double)bt[(size_t)i] + 1.0 : 0.0;
            d[(size_t)i + (size_t)P] = (double)bc[(size_t)i];
            d[(size_t)i + 2 * (size_t)P] = (double)bn[(size_t)i];
        }
    }
    return rc;
}

// the parameters of the sphere commands, prhs[0 .. 7]: maxDistance (single scalar, finite, normal, > 0), minRadius and maxRadius (single
// scalars, 0 <= minRadius <= maxRadius), maxSpheres, nTrials, minInliers, seed (whole doubles in range), samples ([] or int32 4 x nTrials *
// maxSpheres)
static bool fit_spheres_args_ok(const mxArray* const* a) {
    for (int k = 0; k < 3; ++k)
        if (!mxIsSingle(a[k]) || mxGetM(a[k]) * mxGetN(a[k]) != 1) return false;
    const float t = *(const float*)mxGetData(a[0]), r0 = *(const float*)mxGetData(a[1]), r1 = *(const float*)mxGetData(a[2]);
    if (!(t >= 1.17549435e-38f && t <= 3.40282347e+38f)) return false;
    if (!(r0 >= 0.0f && r0 <= r1)) return false;                   // (a NaN fails)
    if (!whole_in(a[3], 1.0, 64.0) || !whole_in(a[4], 1.0, 1048576.0) || !whole_in(a[5], 4.0, 2147483647.0) ||
        !whole_in(a[6], 0.0, 9007199254740992.0))
        return false;
    if (mxIsEmpty(a[7])) return true;
    return mxIsInt32(a[7]) && mxGetM(a[7]) == 4 && mxGetN(a[7]) == (size_t)mxGetScalar(a[3]) * (size_t)mxGetScalar(a[4]);
}
// the outputs of 'modelFitSpheres' / 'pointFitSpheres' (see the head of this file).  Nothing is left allocated on an error.
static int fit_spheres_on_handle(pcreg_model* h, const mxArray* const* a, int nout, mxArray* out[6]) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    const int P = (int)mxGetScalar(a[3]);
    mxArray* ol = mxCreateNumericMatrix((size_t)M, 1, mxINT32_CLASS, mxREAL);
    std::vector<double> spheres(4 * (size_t)P), rmse((size_t)P);
    std::vector<int32_t> counts((size_t)P), used((size_t)P), bt((size_t)P), bn((size_t)P);
    std::vector<int64_t> bc((size_t)P);
    int32_t n = 0;
    rc = pcreg_model_fit_spheres_f32(h, *(const float*)mxGetData(a[0]), *(const float*)mxGetData(a[1]), *(const float*)mxGetData(a[2]), P,
                                     (int)mxGetScalar(a[4]), (int)mxGetScalar(a[5]), (uint64_t)mxGetScalar(a[6]),
                                     mxIsEmpty(a[7]) ? nullptr : (const int32_t*)mxGetData(a[7]), M > 0 ? (int32_t*)mxGetData(ol) : nullptr,
                                     spheres.data(), counts.data(), rmse.data(), used.data(), &n, bt.data(), bc.data(), bn.data());
    if (rc != PCREG_OK) { mxDestroyArray(ol); return rc; }
    out[0] = ol;
    if (nout > 1) {                                               // the library's rows transposed into MATLAB's columns
        out[1] = mxCreateDoubleMatrix((size_t)n, 4, mxREAL);
        for (int c = 0; c < 4; ++c) for (int i = 0; i < n; ++i) mxGetPr(out[1])[(size_t)i + (size_t)c * (size_t)n] = spheres[(size_t)i * 4 + c];
    }
    if (nout > 2) {
        out[2] = mxCreateNumericMatrix((size_t)n, 1, mxINT32_CLASS, mxREAL);
        for (int i = 0; i < n; ++i) ((int32_t*)mxGetData(out[2]))[i] = counts[(size_t)i];
    }
    if (nout > 3) {
        out[3] = mxCreateDoubleMatrix((size_t)n, 1, mxREAL);
        for (int i = 0; i < n; ++i) mxGetPr(out[3])[i] = rmse[(size_t)i];
    }
    if (nout > 4) {
        out[4] = mxCreateNumericMatrix((size_t)n, 1, mxINT32_CLASS, mxREAL);
        for (int i = 0; i < n; ++i) ((int32_t*)mxGetData(out[4]))[i] = used[(size_t)i];
    }
    if (nout > 5) {
        out[5] = mxCreateDoubleMatrix((size_t)P, 3, mxREAL);
        double* d = mxGetPr(out[5]);
        const bool ran_more = n < P;                              // round n ran too and ended the extraction: its diagnostics are real
        for (int i = 0; i < P; ++i) {
            const bool ran = i < n || (ran_more && i == n && M > 0);
            d[i] = ran ? (double)bt[(size_t)i] + 1.0 : 0.0;
            d[(size_t)i + (size_t)P] = (double)bc[(size_t)i];
            d[(size_t)i + 2 * (size_t)P] = (double)bn[(size_t)i];
        }
    }
    return rc;
}

// the parameters of the cylinder commands, prhs[0 .. 11]: maxDistance, minRadius, maxRadius (single scalars as for the spheres), refVec
// ([] or three finite doubles, not all zero), maxAngle (a double scalar, in (0, pi / 2] with refVec), normals ([] or single M x 3),
// kNormals (3 .. 32), maxCylinders, nTrials, minInliers, seed (whole doubles in range), samples ([] or int32 2 x nTrials * maxCylinders)
static bool fit_cylinders_args_ok(const mxArray* const* a, size_t M) {
    for (int k = 0; k < 3; ++k)
        if (!mxIsSingle(a[k]) || mxGetM(a[k]) * mxGetN(a[k]) != 1) return false;
    const float t = *(const float*)mxGetData(a[0]), r0 = *(const float*)mxGetData(a[1]), r1 = *(const float*)mxGetData(a[2]);
    if (!(t >= 1.17549435e-38f && t <= 3.40282347e+38f)) return false;
    if (!(r0 >= 0.0f && r0 <= r1)) return false;                   // (a NaN fails)
    if (!(mxIsEmpty(a[3]) || (mxIsDouble(a[3]) && mxGetM(a[3]) * mxGetN(a[3]) == 3))) return false;
    if (!mxIsEmpty(a[3])) {                                       // finite and not all zero
        const double* r = mxGetPr(a[3]);
        for (int c = 0; c < 3; ++c) if (!(std::fabs(r[c]) <= 1.7976931348623157e308)) return false;
        if (r[0] == 0.0 && r[1] == 0.0 && r[2] == 0.0) return false;
    }
    if (!mxIsDouble(a[4]) || mxGetM(a[4]) * mxGetN(a[4]) != 1) return false;
    if (!mxIsEmpty(a[3]) && !(mxGetScalar(a[4]) > 0.0 && mxGetScalar(a[4]) <= 1.5707963267948966)) return false;
    if (!(mxIsEmpty(a[5]) || (mxIsSingle(a[5]) && mxGetM(a[5]) == M && mxGetN(a[5]) == 3))) return false;
    if (!whole_in(a[6], 3.0, 32.0) || !whole_in(a[7], 1.0, 64.0) || !whole_in(a[8], 1.0, 1048576.0) ||
        !whole_in(a[9], 4.0, 2147483647.0) || !whole_in(a[10], 0.0, 9007199254740992.0))
        return false;
    if (mxIsEmpty(a[11])) return true;
    return mxIsInt32(a[11]) && mxGetM(a[11]) == 2 && mxGetN(a[11]) == (size_t)mxGetScalar(a[7]) * (size_t)mxGetScalar(a[8]);
}
// the outputs of 'modelFitCylinders' / 'pointFitCylinders' (see the head of this file).  Nothing is left allocated on an error.
static int fit_cylinders_on_handle(pcreg_model* h, const mxArray* const* a, int nout, mxArray* out[7]) {
    int M = 0;
    int rc = pcreg_model_size(h, &M);
    if (rc != PCREG_OK) return rc;
    if (!mxIsEmpty(a[5]) && mxGetM(a[5]) != (size_t)M) return PCREG_E_ARG;           // (a handle's rows are known only here)
    const int P = (int)mxGetScalar(a[7]);
    mxArray* ol = mxCreateNumericMatrix((size_t)M, 1, mxINT32_CLASS, mxREAL);
    std::vector<double> cyl(7 * (size_t)P), ext(2 * (size_t)P), rmse((size_t)P);
    std::vector<int32_t> counts((size_t)P), used((size_t)P), bt((size_t)P), bn((size_t)P);
    std::vector<int64_t> bc((size_t)P);
    int32_t n = 0;
    rc = pcreg_model_fit_cylinders_f32(h, *(const float*)mxGetData(a[0]), *(const float*)mxGetData(a[1]), *(const float*)mxGetData(a[2]),
                                       mxIsEmpty(a[3]) ? nullptr : mxGetPr(a[3]), mxGetScalar(a[4]),
                                       mxIsEmpty(a[5]) ? nullptr : (const float*)mxGetData(a[5]), M > 0 ? M : 1, (int)mxGetScalar(a[6]), P,
                                       (int)mxGetScalar(a[8]), (int)mxGetScalar(a[9]), (uint64_t)mxGetScalar(a[10]),
                                       mxIsEmpty(a[11]) ? nullptr : (const int32_t*)mxGetData(a[11]), M > 0 ? (int32_t*)mxGetData(ol) : nullptr,
                                       cyl.data(), ext.data(), counts.data(), rmse.data(), used.data(), &n, bt.data(), bc.data(), bn.data());
    if (rc != PCREG_OK) { mxDestroyArray(ol); return rc; }
    out[0] = ol;
    if (nout > 1) {                                               // the library's rows transposed into MATLAB's columns
        out[1] = mxCreateDoubleMatrix((size_t)n, 7, mxREAL);
        for (int c = 0; c < 7; ++c) for (int i = 0; i < n; ++i) mxGetPr(out[1])[(size_t)i + (size_t)c * (size_t)n] = cyl[(size_t)i * 7 + c];
    }
    if (nout > 2) {
        out[2] = mxCreateDoubleMatrix((size_t)n, 2, mxREAL);
        for (int c = 0; c < 2; ++c) for (int i = 0; i < n; ++i) mxGetPr(out[2])[(size_t)i + (size_t)c * (size_t)n] = ext[(size_t)i * 2 + c];
    }
    if (nout > 3) {
        out[3] = mxCreateNumericMatrix((size_t)n, 1, mxINT32_CLASS, mxREAL);
        for (int i = 0; i < n; ++i) ((int32_t*)mxGetData(out[3]))[i] = counts[(size_t)i];
    }
    if (nout > 4) {
        out[4] = mxCreateDoubleMatrix((size_t)n, 1, mxREAL);
        for (int i = 0; i < n; ++i) mxGetPr(out[4])[i] = rmse[(size_t)i];
    }
    if (nout > 5) {
        out[5] = mxCreateNumericMatrix((size_t)n, 1, mxINT32_CLASS, mxREAL);
        for (int i = 0; i < n; ++i) ((int32_t*)mxGetData(out[5]))[i] = used[(size_t)i];
    }
    if (nout > 6) {
        out[6] = mxCreateDoubleMatrix((size_t)P, 3, mxREAL);
        double* d = mxGetPr(out[6]);
        const bool ran_more = n < P;                              // round n ran too and ended the extraction: its diagnostics are real
        for (int i = 0; i < P; ++i) {
            const bool ran = i < n || (ran_more && i == n && M > 0);
            d[i] = ran ? (double)bt[(size_t)i] + 1.0 : 0.0;
            d[(size_t)i + (size_t)P] = (double)bc[(size_t)i];
            d[(size_t)i + 2 * (size_t)P] = (double)bn[(size_t)i];
        }
    }
    return rc;
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs < 1 || !mxIsChar(prhs[0])) { mexErrMsgIdAndTxt("pcreg:usage", "pcreg_mex('<command>', ...)"); return; }
    char cmd[64]; mxGetString(prhs[0], cmd, sizeof cmd);
    int rc = PCREG_OK;
    const char* usage = nullptr;

    if (!strcmp(cmd, "estimateTransform")) {
        if (nrhs != 3) usage = "estimateTransform: pts1, pts2";
        else {
            int n = (int)mxGetM(prhs[1]);
            double T[16]; int empty = 1;
            rc = pcreg_estimate_transform(mxGetPr(prhs[1]), mxGetPr(prhs[2]), n, n, T, &empty);
            if (rc == PCREG_OK) {
                plhs[0] = empty ? mxCreateDoubleMatrix(0, 0, mxREAL) : mxCreateDoubleMatrix(4, 4, mxREAL);
                if (!empty) memcpy(mxGetPr(plhs[0]), T, sizeof T);
            }
        }
    } else if (!strcmp(cmd, "calcDists")) {
        if (nrhs != 4) usage = "calcDists: T, pts1, pts2";
        else {
            int n = (int)mxGetM(prhs[2]);
            plhs[0] = mxCreateDoubleMatrix(n, 1, mxREAL);
            rc = pcreg_calc_dists(mxGetPr(prhs[1]), mxGetPr(prhs[2]), mxGetPr(prhs[3]), n, n, mxGetPr(plhs[0]));
        }
    } else if (!strcmp(cmd, "ransac")) {
        if (nrhs < 4) usage = "ransac: pts1, pts2, coef[, sample_idx, seed]";
        else {
            const mxArray* c = prhs[3];
            pcreg_ransac_opts o;
            o.minPtNum = (int)field(c, "minPtNum", 3); o.iterNum = (int)field(c, "iterNum", 1000);
            o.thDist = field(c, "thDist", 0.5); o.thInlrRatio = field(c, "thInlrRatio", 0.1);
            o.REFINE = (int)field(c, "REFINE", 1); o.VERBOSE = (int)field(c, "VERBOSE", 1);
            o.seed = nrhs > 5 ? (uint64_t)mxGetScalar(prhs[5]) : 0;
            int n = (int)mxGetM(prhs[1]);
            // sample_idx: int32 minPtNum x iterNum (each COLUMN one hypothesis) or []
            const int32_t* si = (nrhs > 4 && !mxIsEmpty(prhs[4]) && mxIsInt32(prhs[4])) ? (const int32_t*)mxGetData(prhs[4]) : nullptr;
            mxArray* inl = mxCreateNumericMatrix(n > 0 ? n : 1, 1, mxINT32_CLASS, mxREAL);
            double T[16]; int ni = 0, ns = 0, mi = 0, fl = 1;
            rc = pcreg_ransac(mxGetPr(prhs[1]), mxGetPr(prhs[2]), n, n, &o, si, T, (int32_t*)mxGetData(inl), &ni, &ns, &mi, &fl, nullptr, nullptr);
            if (rc == PCREG_OK) {
                plhs[0] = fl ? mxCreateDoubleMatrix(0, 0, mxREAL) : mxCreateDoubleMatrix(4, 4, mxREAL);
                if (!fl) memcpy(mxGetPr(plhs[0]), T, sizeof T);
                if (nlhs > 1) {                         // inlierIdx as a double column, like find()
                    plhs[1] = mxCreateDoubleMatrix(fl ? 0 : ni, fl ? 0 : 1, mxREAL);
                    const int32_t* src = (const int32_t*)mxGetData(inl);
                    for (int k = 0; k < (fl ? 0 : ni); ++k) mxGetPr(plhs[1])[k] = (double)src[k];
                }
                if (nlhs > 2) plhs[2] = mxCreateDoubleScalar(ns);
                if (nlhs > 3) plhs[3] = mxCreateDoubleScalar(mi);
                if (nlhs > 4) plhs[4] = mxCreateDoubleScalar(fl);
            }
            mxDestroyArray(inl);
        }
    } else if (!strcmp(cmd, "ransacBatched")) {                // [T, inlierIdx, nInliers, numSuccess, maxInliers, failed] =
        // pcreg_mex('ransacBatched', pts1, pts2, int32(offsets), coef[, sampleIdx, seed]): B registrations in one launch (the parfor of
        // completeExperimentFast.m:201-216).  pts1 / pts2: the registrations' rows back to back (total x 3); offsets: B + 1 running row
        // offsets (0-based); sampleIdx: int32 minPtNum x (iterNum B), registration after registration, or []; seed: registration b
        // samples with seed + b.  T: 4 x 4 x B (zeros where failed); inlierIdx: the lists back to back (1-based inside a registration),
        // nInliers / numSuccess / maxInliers / failed: B x 1.  matlab/ransacBatched.m
        if (nrhs < 5 || !mxIsInt32(prhs[3])) usage = "ransacBatched: pts1, pts2, int32 offsets, coef[, sample_idx, seed]";
        else {
            const mxArray* c = prhs[4];
            pcreg_ransac_opts o;
            o.minPtNum = (int)field(c, "minPtNum", 3); o.iterNum = (int)field(c, "iterNum", 1000);
            o.thDist = field(c, "thDist", 0.5); o.thInlrRatio = field(c, "thInlrRatio", 0.1);
            o.REFINE = (int)field(c, "REFINE", 1); o.VERBOSE = (int)field(c, "VERBOSE", 1);
            o.seed = nrhs > 6 ? (uint64_t)mxGetScalar(prhs[6]) : 0;
            const int total = (int)mxGetM(prhs[1]);
            const int B = (int)(mxGetM(prhs[3]) * mxGetN(prhs[3])) - 1;
            const int32_t* off = (const int32_t*)mxGetData(prhs[3]);
            const int32_t* si = (nrhs > 5 && !mxIsEmpty(prhs[5]) && mxIsInt32(prhs[5])) ? (const int32_t*)mxGetData(prhs[5]) : nullptr;
            if (B < 0 || off[0] != 0 || off[B] != total || (int)mxGetM(prhs[2]) != total) usage = "ransacBatched: offsets must run from 0 to size(pts1, 1) = size(pts2, 1)";
            else if (si && mxGetM(prhs[5]) * mxGetN(prhs[5]) != (size_t)o.minPtNum * (size_t)o.iterNum * (size_t)B) usage = "ransacBatched: sampleIdx must be minPtNum x (iterNum * B)";
            else {
                const size_t b1 = (size_t)(B > 0 ? B : 1);
                mxArray* inl = mxCreateNumericMatrix(total > 0 ? total : 1, 1, mxINT32_CLASS, mxREAL);
                mxArray* ni = mxCreateNumericMatrix(b1, 1, mxINT32_CLASS, mxREAL); mxArray* ns = mxCreateNumericMatrix(b1, 1, mxINT32_CLASS, mxREAL);
                mxArray* mi = mxCreateNumericMatrix(b1, 1, mxINT32_CLASS, mxREAL); mxArray* fl = mxCreateNumericMatrix(b1, 1, mxINT32_CLASS, mxREAL);
                mwSize dims[3] = {4, 4, (mwSize)B};
                plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
                rc = B == 0 ? PCREG_OK : pcreg_ransac_batched(mxGetPr(prhs[1]), mxGetPr(prhs[2]), total, total > 0 ? total : 1, off, B, &o, si, mxGetPr(plhs[0]),
                                                               (int32_t*)mxGetData(inl), (int32_t*)mxGetData(ni), (int32_t*)mxGetData(ns), (int32_t*)mxGetData(mi),
                                                               (int32_t*)mxGetData(fl));
                if (rc == PCREG_OK) {
                    const int32_t *n_ = (const int32_t*)mxGetData(ni), *f_ = (const int32_t*)mxGetData(fl), *src = (const int32_t*)mxGetData(inl);
                    size_t tot_inl = 0;
                    for (int b = 0; b < B; ++b) {
                        if (f_[b]) memset(mxGetPr(plhs[0]) + (size_t)b * 16, 0, 128);
                        else tot_inl += (size_t)n_[b];
                    }
                    if (nlhs > 1) {                     // the inlier lists back to back, as a double column like find()
                        plhs[1] = mxCreateDoubleMatrix(tot_inl, tot_inl ? 1 : 0, mxREAL);
                        size_t k = 0;
                        for (int b = 0; b < B; ++b) if (!f_[b]) for (int e = 0; e < n_[b]; ++e) mxGetPr(plhs[1])[k++] = (double)src[off[b] + e];
                    }
                    auto col = [&](const mxArray* a, bool zero_failed) {
                        mxArray* out = mxCreateDoubleMatrix(B, B ? 1 : 0, mxREAL);
                        const int32_t* v = (const int32_t*)mxGetData(a);
                        for (int b = 0; b < B; ++b) mxGetPr(out)[b] = (zero_failed && f_[b]) ? 0.0 : (double)v[b];
                        return out;
                    };
                    if (nlhs > 2) plhs[2] = col(ni, true);
                    if (nlhs > 3) plhs[3] = col(ns, false);
                    if (nlhs > 4) plhs[4] = col(mi, false);
                    if (nlhs > 5) plhs[5] = col(fl, false);
                }
                mxDestroyArray(inl); mxDestroyArray(ni); mxDestroyArray(ns); mxDestroyArray(mi); mxDestroyArray(fl);
            }
        }
    } else if (!strcmp(cmd, "fgrBatched")) {                   // [T, inlierIdx, stats, kept] =
        // pcreg_mex('fgrBatched', pts1, pts2, int32(offsets), opts[, tupleIdx, T0]): fast global registration of B sets of matched pairs
        // in one call (pcreg_fgr_batched's contract).  pts1 / pts2: the registrations' rows back to back (total x 3 doubles);
        // offsets: B + 1 running row offsets (0-based); opts: a struct with delta2 (required, compared with SQUARED distances) and any of
        // iterations (128), decrease_every (4), division_factor (1.4), mu0 (0: the default), n_tuples (0: no tuple test), tuple_scale
        // (0.95), seed (0); tupleIdx: int32 3 x (n_tuples B), one COLUMN per triple, registration after registration, or []; T0: 4 x 4 x B
        // doubles or [].  T: 4 x 4 x B (zeros where failed); inlierIdx: the lists back to back (1-based inside a registration); stats: B x 9
        // doubles, the columns failed, n_live, n_kept, n_inliers, mu0, mu_final, cost, sum_d2, n; kept: total x 1 uint8.  matlab/fgrBatched.m
        const mxArray* c = nrhs > 4 ? prhs[4] : nullptr;
        bool no_delta = false;
        if (c) (void)field(c, "delta2", 0.0, &no_delta);
        if (nrhs < 5 || nrhs > 7 || !mxIsDouble(prhs[1]) || !mxIsDouble(prhs[2]) || !mxIsInt32(prhs[3]) || !mxIsStruct(c))
            usage = "fgrBatched: pts1, pts2 (total x 3 doubles), int32 offsets, opts (a struct)[, int32 tupleIdx, T0]";
        else if (no_delta) usage = "fgrBatched: opts.delta2 is required";
        else {
            pcreg_fgr_opts o;
            o.delta2 = field(c, "delta2", 0.0); o.iterations = (int32_t)field(c, "iterations", 128);
            o.decrease_every = (int32_t)field(c, "decrease_every", 4); o.division_factor = field(c, "division_factor", 1.4);
            o.mu0 = field(c, "mu0", 0.0); o.n_tuples = (int32_t)field(c, "n_tuples", 0); o.reserved = 0;
            o.tuple_scale = field(c, "tuple_scale", 0.95); o.seed = (uint64_t)field(c, "seed", 0.0);
            const int total = (int)mxGetM(prhs[1]);
            const int B = (int)(mxGetM(prhs[3]) * mxGetN(prhs[3])) - 1;
            const int32_t* off = (const int32_t*)mxGetData(prhs[3]);
            const bool has_tab = nrhs > 5 && !mxIsEmpty(prhs[5]), has_T0 = nrhs > 6 && !mxIsEmpty(prhs[6]);
            if (B < 0 || off[0] != 0 || off[B] != total || (int)mxGetM(prhs[2]) != total || (total > 0 && (mxGetN(prhs[1]) != 3 || mxGetN(prhs[2]) != 3)))
                usage = "fgrBatched: offsets must run from 0 to size(pts1, 1) = size(pts2, 1), and the points have 3 columns";
            else if (has_tab && (!mxIsInt32(prhs[5]) || o.n_tuples < 0 || mxGetM(prhs[5]) * mxGetN(prhs[5]) != (size_t)3 * (size_t)o.n_tuples * (size_t)B))
                usage = "fgrBatched: tupleIdx must be int32, 3 x (n_tuples * B)";
            else if (has_T0 && (!mxIsDouble(prhs[6]) || mxGetM(prhs[6]) * mxGetN(prhs[6]) != (size_t)16 * (size_t)B))
                usage = "fgrBatched: T0 must be 4 x 4 x B doubles";
            else {
                const size_t b1 = (size_t)(B > 0 ? B : 1), t1 = (size_t)(total > 0 ? total : 1);
                mxArray* inl = mxCreateNumericMatrix(t1, 1, mxINT32_CLASS, mxREAL);
                mxArray* res = mxCreateNumericMatrix(sizeof(pcreg_fgr_result), b1, mxUINT8_CLASS, mxREAL);
                mxArray* kept = mxCreateNumericMatrix(t1, 1, mxUINT8_CLASS, mxREAL);
                pcreg_fgr_result* r = (pcreg_fgr_result*)mxGetData(res);
                rc = B == 0 ? PCREG_OK : pcreg_fgr_batched(mxGetPr(prhs[1]), mxGetPr(prhs[2]), total, (int)t1, off, B, &o, has_T0 ? mxGetPr(prhs[6]) : nullptr,
                                                            has_tab ? (const int32_t*)mxGetData(prhs[5]) : nullptr, r, (int32_t*)mxGetData(inl),
                                                            (uint8_t*)mxGetData(kept));
                if (rc == PCREG_OK) {
                    mwSize dims[3] = {4, 4, (mwSize)B};
                    plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
                    size_t tot_inl = 0;
                    for (int b = 0; b < B; ++b) {
                        memcpy(mxGetPr(plhs[0]) + (size_t)b * 16, r[b].T, 128);
                        tot_inl += (size_t)r[b].n_inliers;
                    }
                    if (nlhs > 1) {                     // the inlier lists back to back, as a double column like find()
                        plhs[1] = mxCreateDoubleMatrix(tot_inl, tot_inl ? 1 : 0, mxREAL);
                        const int32_t* src = (const int32_t*)mxGetData(inl);
                        size_t k = 0;
                        for (int b = 0; b < B; ++b) for (int e = 0; e < r[b].n_inliers; ++e) mxGetPr(plhs[1])[k++] = (double)src[off[b] + e];
                    }
                    if (nlhs > 2) {
                        plhs[2] = mxCreateDoubleMatrix(B, B ? 9 : 0, mxREAL);
                        double* s = mxGetPr(plhs[2]);
                        for (int b = 0; b < B; ++b) {
                            const double v[9] = {(double)r[b].failed, (double)r[b].n_live, (double)r[b].n_kept, (double)r[b].n_inliers, r[b].mu0, r[b].mu_final,
                                                 r[b].cost, r[b].sum_d2, (double)r[b].n};
                            for (int k = 0; k < 9; ++k) s[(size_t)k * B + b] = v[k];
                        }
                    }
                    if (nlhs > 3) {
                        plhs[3] = mxCreateNumericMatrix(total, total ? 1 : 0, mxUINT8_CLASS, mxREAL);
                        if (total > 0) memcpy(mxGetData(plhs[3]), mxGetData(kept), (size_t)total);
                    }
                }
                mxDestroyArray(inl); mxDestroyArray(res); mxDestroyArray(kept);
            }
        }
    } else if (!strcmp(cmd, "getMatches")) {
        if (nrhs != 4) usage = "getMatches: descSurface, descModel, par";
        else {
            const mxArray* p = prhs[3];
            pcreg_match_opts o;
            o.metric = field_is(p, "Metric", "SAD") ? PCREG_METRIC_SAD : PCREG_METRIC_SSD;
            o.matchThreshold = field(p, "MatchThreshold", 1.0); o.maxRatio = field(p, "MaxRatio", 0.6);
            o.unique = (int)field(p, "Unique", 0); o.prenormalized = 0;
            o.unnormalize = (int)field(p, "UNNORMALIZE", 0); o.norm_factor = field(p, "norm_factor", 0.0);
            o.change_metric = (int)field(p, "CHANGE_METRIC", 0); o.metric_factor = field(p, "metric_factor", 1.0);
            int Q = (int)mxGetM(prhs[1]), M = (int)mxGetM(prhs[2]), D = (int)mxGetN(prhs[1]);
            mxArray* buf = mxCreateNumericMatrix(2, Q > 0 ? Q : 1, mxUINT32_CLASS, mxREAL);   // row-major pairs = 2 x Q column-major
            int P = 0;
            rc = pcreg_get_matches(mxGetPr(prhs[1]), Q, Q, mxGetPr(prhs[2]), M, M, D, &o, (uint32_t*)mxGetData(buf), nullptr, &P);
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
                const uint32_t* src = (const uint32_t*)mxGetData(buf); uint32_t* dst = (uint32_t*)mxGetData(plhs[0]);
                for (int k = 0; k < P; ++k) { dst[k] = src[2 * k]; dst[k + P] = src[2 * k + 1]; }
            }
            mxDestroyArray(buf);
        }
    } else if (!strcmp(cmd, "getMatchesSegmented")) {         // [pairs, nPairs] = pcreg_mex('getMatchesSegmented', descSurface, descModel, int32(rows), int32(segOff), par)
        // rows: the model rows of all segments back to back (1-based, ascending inside a segment); segOff: S + 1 running offsets
        // (0-based); pairs: sum(nPairs) x 2 uint32, segment after segment; nPairs: S x 1 int32.  matlab/getMatchesSegmented.m
        if (nrhs != 6 || !mxIsInt32(prhs[3]) || !mxIsInt32(prhs[4])) usage = "getMatchesSegmented: descSurface, descModel, int32 rows, int32 segOff, par";
        else {
            const mxArray* p = prhs[5];
            pcreg_match_opts o;
            o.metric = field_is(p, "Metric", "SAD") ? PCREG_METRIC_SAD : PCREG_METRIC_SSD;
            o.matchThreshold = field(p, "MatchThreshold", 1.0); o.maxRatio = field(p, "MaxRatio", 0.6);
            o.unique = (int)field(p, "Unique", 0); o.prenormalized = 0;
            o.unnormalize = (int)field(p, "UNNORMALIZE", 0); o.norm_factor = field(p, "norm_factor", 0.0);
            o.change_metric = (int)field(p, "CHANGE_METRIC", 0); o.metric_factor = field(p, "metric_factor", 1.0);
            const int Q = (int)mxGetM(prhs[1]), VM = (int)mxGetM(prhs[2]), D = (int)mxGetN(prhs[1]);
            const int S = (int)(mxGetM(prhs[4]) * mxGetN(prhs[4])) - 1;
            const size_t tot = mxGetM(prhs[3]) * mxGetN(prhs[3]);
            const int32_t* off = (const int32_t*)mxGetData(prhs[4]);
            if (S < 0 || off[0] != 0 || (size_t)off[S] != tot) usage = "getMatchesSegmented: segOff must run from 0 to numel(rows)";
            else {
                mxArray* r0 = mxCreateNumericMatrix(tot > 0 ? tot : 1, 1, mxINT32_CLASS, mxREAL);
                mxArray* buf = mxCreateNumericMatrix(2, (size_t)(S > 0 ? S : 1) * (Q > 0 ? Q : 1), mxUINT32_CLASS, mxREAL);
                mxArray* np = mxCreateNumericMatrix(S > 0 ? S : 1, 1, mxINT32_CLASS, mxREAL);
                int32_t* rz = (int32_t*)mxGetData(r0); const int32_t* r1 = (const int32_t*)mxGetData(prhs[3]);
                for (size_t k = 0; k < tot; ++k) rz[k] = r1[k] - 1;
                rc = pcreg_get_matches_segmented(mxGetPr(prhs[1]), Q, Q, mxGetPr(prhs[2]), VM, VM, D, rz, off, S, &o, (uint32_t*)mxGetData(buf),
                                                 (int32_t*)mxGetData(np));
                if (rc == PCREG_OK) {
                    const int32_t* n = (const int32_t*)mxGetData(np);
                    size_t P = 0; for (int z = 0; z < S; ++z) P += (size_t)n[z];
                    plhs[0] = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
                    const uint32_t* src = (const uint32_t*)mxGetData(buf); uint32_t* dst = (uint32_t*)mxGetData(plhs[0]);
                    size_t k = 0;
                    for (int z = 0; z < S; ++z)
                        for (int e = 0; e < n[z]; ++e, ++k) { dst[k] = src[((size_t)z * Q + e) * 2]; dst[k + P] = src[((size_t)z * Q + e) * 2 + 1]; }
                    if (nlhs > 1) { plhs[1] = mxCreateNumericMatrix(S, 1, mxINT32_CLASS, mxREAL); memcpy(mxGetData(plhs[1]), n, (size_t)S * 4); }
                }
                mxDestroyArray(r0); mxDestroyArray(buf); mxDestroyArray(np);
            }
        }
    } else if (!strcmp(cmd, "AlignPoints_KNN")) {
        if (nrhs != 4) usage = "AlignPoints_KNN: pts, C1, C2";
        else {
            int n = (int)mxGetM(prhs[1]);
            const bool sgl = mxIsSingle(prhs[1]);                // single in -> single out, like MATLAB's own function
            const mxClassID cls = sgl ? mxSINGLE_CLASS : mxDOUBLE_CLASS;
            plhs[0] = mxCreateNumericMatrix(n, 3, cls, mxREAL);
            mxArray* co = mxCreateNumericMatrix(3, 3, cls, mxREAL); mxArray* c = mxCreateNumericMatrix(1, 3, cls, mxREAL);
            if (sgl) rc = pcreg_align_points_knn_f32((const float*)mxGetData(prhs[1]), n, n, (int)mxGetScalar(prhs[2]), (int)mxGetScalar(prhs[3]),
                                                     (float*)mxGetData(plhs[0]), (float*)mxGetData(co), (float*)mxGetData(c));
            else rc = pcreg_align_points_knn(mxGetPr(prhs[1]), n, n, (int)mxGetScalar(prhs[2]), (int)mxGetScalar(prhs[3]),
                                             mxGetPr(plhs[0]), mxGetPr(co), mxGetPr(c));
            if (nlhs > 1) plhs[1] = co; else mxDestroyArray(co);
            if (nlhs > 2) plhs[2] = c; else mxDestroyArray(c);
        }
    } else if (!strcmp(cmd, "getSpacialHistogramDescriptors")) {
        if (nrhs != 4) usage = "getSpacialHistogramDescriptors: pts, sample_pts, options";
        else {
            const mxArray* p = prhs[3];
            pcreg_desc_opts o;
            double mx = field(p, "max_pts", 6000);
            o.min_pts = (int)field(p, "min_pts", 500); o.max_pts = mx > 2147483647.0 ? 2147483647 : (int)mx;
            o.R = field(p, "R", 3.5); o.ALIGN_POINTS = (int)field(p, "ALIGN_POINTS", 1);
            const mxArray* tv = mxGetField(p, 0, "thVar");
            o.thVar[0] = tv ? mxGetPr(tv)[0] : 3.0; o.thVar[1] = tv ? mxGetPr(tv)[1] : 1.5;
            const mxArray* kk = mxGetField(p, 0, "k");
            o.k = (!kk || mxIsChar(kk)) ? 1.0 : mxGetScalar(kk);           // 'all' -> 1
            int P = (int)mxGetM(prhs[1]), S = (int)mxGetM(prhs[2]);
            // each input in its own class (single or double); feat / desc are DOUBLE whatever the inputs: the reference
            // preallocates them with nan(...) and assigns into them (getSpacialHistogramDescriptors.m:61-62)
            const int ps = mxIsSingle(prhs[1]) ? 1 : 0, ss = mxIsSingle(prhs[2]) ? 1 : 0;
            mxArray* f = mxCreateNumericMatrix(3, S > 0 ? S : 1, mxDOUBLE_CLASS, mxREAL);     // row-major V x 3 == 3 x V column-major
            mxArray* d = mxCreateNumericMatrix(PCREG_DESC_LEN, S > 0 ? S : 1, mxDOUBLE_CLASS, mxREAL);
            int V = 0;
            rc = pcreg_spatial_histogram_descriptors_mixed(mxGetData(prhs[1]), ps, P, P, mxGetData(prhs[2]), ss, S, S, &o, mxGetPr(f), mxGetPr(d), &V);
            if (rc == PCREG_OK) {      // transpose into MATLAB's V x 3 / V x 980
                plhs[0] = mxCreateNumericMatrix(V, 3, mxDOUBLE_CLASS, mxREAL);
                if (nlhs > 1) plhs[1] = mxCreateNumericMatrix(V, PCREG_DESC_LEN, mxDOUBLE_CLASS, mxREAL);
                for (int v = 0; v < V; ++v) for (int c = 0; c < 3; ++c) mxGetPr(plhs[0])[v + (size_t)c * V] = mxGetPr(f)[c + 3 * (size_t)v];
                if (nlhs > 1) for (int v = 0; v < V; ++v) for (int c = 0; c < PCREG_DESC_LEN; ++c) mxGetPr(plhs[1])[v + (size_t)c * V] = mxGetPr(d)[c + PCREG_DESC_LEN * (size_t)v];
            }
            mxDestroyArray(f); mxDestroyArray(d);
        }
    } else if (!strcmp(cmd, "finalStageLimits")) {            // limits = pcreg_mex('finalStageLimits', pts, T)
        // limits(k, :) = [xmin xmax ymin ymax zmin zmax] of quickTF(pts, T(:, :, k)) as the library moves the surface (the box of
        // pcRandomUniformSamples, :418-432); T(:, :, k) = invertTF(transCur_k).  matlab/finalStage.m
        if (nrhs != 3 || !mxIsDouble(prhs[1]) || !mxIsDouble(prhs[2]) || mxGetN(prhs[1]) != 3 || mxGetM(prhs[1]) == 0 || mxGetM(prhs[2]) != 4 ||
            mxGetN(prhs[2]) == 0 || mxGetN(prhs[2]) % 4 != 0)
            usage = "finalStageLimits: pts (N x 3 double, N >= 1), T (4 x 4 x K double)";
        else {
            const int N = (int)mxGetM(prhs[1]), K = (int)(mxGetN(prhs[2]) / 4);
            mxArray* lim = mxCreateDoubleMatrix(6, K, mxREAL);                      // [K][6] == 6 x K column-major
            rc = pcreg_final_stage_limits(mxGetPr(prhs[1]), N, N, mxGetPr(prhs[2]), K, mxGetPr(lim));
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateDoubleMatrix(K, 6, mxREAL);
                for (int k = 0; k < K; ++k) for (int c = 0; c < 6; ++c) mxGetPr(plhs[0])[k + (size_t)c * K] = mxGetPr(lim)[c + 6 * (size_t)k];
            }
            mxDestroyArray(lim);
        }
    } else if (!strcmp(cmd, "finalStage")) {
        // [numKeypoints, numDesc, numMatches, numClose, precisions, best, T_refine, ptsFinal, pairs] = pcreg_mex('finalStage', hModelNoLRF,
        //     featModel_noLRF, pts, locs, T, keypoints, int32(kpOff), descOpt, par, R_desc, maxDist)
        // completeExperimentFast.m:291-394 for K clusters in one call: locs K x 3 (locCur), T 4 x 4 x K (invertTF(transCur)), keypoints: every
        // cluster's draw back to back, kpOff: the K + 1 running row offsets (0-based).  best is 1-based; T_refine is [] when empty; pairs:
        // sum(numMatches) x 2 uint32, cluster after cluster (model index inside the cluster's sphere).  matlab/finalStage.m
        if (nrhs != 12 || !mxIsUint64(prhs[1]) || !mxIsDouble(prhs[2]) || !mxIsDouble(prhs[3]) || !mxIsDouble(prhs[4]) || !mxIsDouble(prhs[5]) ||
            !mxIsDouble(prhs[6]) || !mxIsInt32(prhs[7]))
            usage = "finalStage: hModelNoLRF (uint64), featModel_noLRF, pts, locs (double n x 3), T (4 x 4 x K double), keypoints (double S x 3), "
                    "int32 kpOff, descOpt, par, R_desc, maxDist";
        else {
            const mxArray* q = prhs[8];
            pcreg_desc_opts d;
            const double mx = field(q, "max_pts", 6000);
            d.min_pts = (int)field(q, "min_pts", 500); d.max_pts = mx > 2147483647.0 ? 2147483647 : (int)mx;
            d.R = field(q, "R", 3.5); d.ALIGN_POINTS = 0;                            // :300
            const mxArray* tv = mxIsStruct(q) ? mxGetField(q, 0, "thVar") : nullptr;
            d.thVar[0] = (tv && mxGetM(tv) * mxGetN(tv) >= 2) ? mxGetPr(tv)[0] : 3.0; d.thVar[1] = (tv && mxGetM(tv) * mxGetN(tv) >= 2) ? mxGetPr(tv)[1] : 1.5;
            const mxArray* kk = mxIsStruct(q) ? mxGetField(q, 0, "k") : nullptr;
            d.k = (!kk || mxIsChar(kk)) ? 1.0 : mxGetScalar(kk);
            const mxArray* p = prhs[9];
            pcreg_match_opts o;
            o.metric = field_is(p, "Metric", "SAD") ? PCREG_METRIC_SAD : PCREG_METRIC_SSD;
            o.matchThreshold = field(p, "MatchThreshold", 1.0); o.maxRatio = field(p, "MaxRatio", 0.6);
            o.unique = (int)field(p, "Unique", 0); o.prenormalized = 0;
            o.unnormalize = (int)field(p, "UNNORMALIZE", 0); o.norm_factor = field(p, "norm_factor", 0.0);
            o.change_metric = (int)field(p, "CHANGE_METRIC", 0); o.metric_factor = field(p, "metric_factor", 1.0);
            pcreg_desc_set* hM = (pcreg_desc_set*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            int VM = 0, D = 0;
            rc = pcreg_desc_set_size(hM, &VM, &D);
            // every size below is the gateway's own: rows of the arrays it was handed, checked against each other
            const int N = (int)mxGetM(prhs[3]), K = (int)mxGetM(prhs[4]), S = (int)mxGetM(prhs[6]);
            const int32_t* off = (const int32_t*)mxGetData(prhs[7]);
            const int n_off = (int)(mxGetM(prhs[7]) * mxGetN(prhs[7]));
            if (rc == PCREG_OK && ((int)mxGetM(prhs[2]) != VM || (VM > 0 && mxGetN(prhs[2]) != 3) || N == 0 || mxGetN(prhs[3]) != 3 || K == 0 ||
                                   mxGetN(prhs[4]) != 3 || mxGetM(prhs[5]) != 4 || mxGetN(prhs[5]) != 4 * (size_t)K || (S > 0 && mxGetN(prhs[6]) != 3) ||
                                   n_off != K + 1 || off[0] != 0 || off[K] != S))
                usage = "finalStage: featModel_noLRF must have the rows of the model set, pts N x 3 (N >= 1), locs K x 3 (K >= 1), T 4 x 4 x K, "
                        "keypoints S x 3, kpOff K + 1 offsets from 0 to S";
            else if (rc == PCREG_OK) {
                const size_t k1 = (size_t)K, s1 = (size_t)(S > 0 ? S : 1);
                mxArray* nk = mxCreateNumericMatrix(k1, 1, mxINT32_CLASS, mxREAL); mxArray* nd = mxCreateNumericMatrix(k1, 1, mxINT32_CLASS, mxREAL);
                mxArray* nm = mxCreateNumericMatrix(k1, 1, mxINT32_CLASS, mxREAL); mxArray* nc = mxCreateNumericMatrix(k1, 1, mxINT32_CLASS, mxREAL);
                mxArray* pr = mxCreateDoubleMatrix(k1, 1, mxREAL);
                mxArray* pf = mxCreateDoubleMatrix((size_t)N, 3, mxREAL);
                mxArray* buf = mxCreateNumericMatrix(2, s1, mxUINT32_CLASS, mxREAL);     // [S][2]: cluster k's pairs from row kpOff(k)
                double Tr[16]; int32_t best = 0, empty = 1;
                rc = pcreg_final_stage(hM, mxGetPr(prhs[2]), VM > 0 ? VM : 1, mxGetPr(prhs[3]), N, N, mxGetPr(prhs[4]), mxGetPr(prhs[5]), K, mxGetPr(prhs[6]), off,
                                       &d, &o, mxGetScalar(prhs[10]), mxGetScalar(prhs[11]), (int32_t*)mxGetData(nk), (int32_t*)mxGetData(nd),
                                       (int32_t*)mxGetData(nm), (int32_t*)mxGetData(nc), mxGetPr(pr), &best, Tr, &empty, mxGetPr(pf),
                                       (uint32_t*)mxGetData(buf));
                if (rc == PCREG_OK) {
                    auto out = [&](int k, mxArray* a) { if (nlhs > k) plhs[k] = a; else mxDestroyArray(a); };
                    auto col = [&](const mxArray* v) { mxArray* a = mxCreateDoubleMatrix(k1, 1, mxREAL); for (int i = 0; i < K; ++i) mxGetPr(a)[i] = (double)((const int32_t*)mxGetData(v))[i]; return a; };
                    plhs[0] = col(nk);
                    out(1, col(nd)); out(2, col(nm)); out(3, col(nc));
                    out(4, mxDuplicateArray(pr));
                    out(5, mxCreateDoubleScalar((double)best + 1.0));
                    { mxArray* Ta = empty ? mxCreateDoubleMatrix(0, 0, mxREAL) : mxCreateDoubleMatrix(4, 4, mxREAL); if (!empty) memcpy(mxGetPr(Ta), Tr, sizeof Tr); out(6, Ta); }
                    out(7, mxDuplicateArray(pf));
                    {
                        const int32_t* n = (const int32_t*)mxGetData(nm);
                        size_t P = 0; for (int k = 0; k < K; ++k) P += (size_t)n[k];
                        mxArray* pa = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
                        const uint32_t* src = (const uint32_t*)mxGetData(buf); uint32_t* dst = (uint32_t*)mxGetData(pa);
                        size_t j = 0;
                        for (int k = 0; k < K; ++k)
                            for (int e = 0; e < n[k]; ++e, ++j) { dst[j] = src[((size_t)off[k] + e) * 2]; dst[j + P] = src[((size_t)off[k] + e) * 2 + 1]; }
                        out(8, pa);
                    }
                }
                mxDestroyArray(nk); mxDestroyArray(nd); mxDestroyArray(nm); mxDestroyArray(nc); mxDestroyArray(pr); mxDestroyArray(pf); mxDestroyArray(buf);
            }
        }
    } else if (!strcmp(cmd, "getLocalPoints")) {              // [pts_sphere, dists] = pcreg_mex('getLocalPoints', pts, R, c, min_points, max_points)
        if (nrhs != 6 || mxGetN(prhs[1]) != 3) usage = "getLocalPoints: pts (N x 3), R, c (1 x 3), min_points, max_points";
        else {
            // a single cloud or centre: MATLAB's element-wise single arithmetic (getLocalPoints.m:8-25) and single results
            const bool ps = mxIsSingle(prhs[1]), cs = mxIsSingle(prhs[3]);
            const int mode = cs ? 1 : (ps ? 2 : 0);
            const int N = (int)mxGetM(prhs[1]);
            mxArray* wide = mxCreateNumericMatrix(N > 0 ? N : 1, 3, mxDOUBLE_CLASS, mxREAL);
            if (ps) { const float* f = (const float*)mxGetData(prhs[1]); for (size_t k = 0; k < (size_t)N * 3; ++k) mxGetPr(wide)[k] = (double)f[k]; }
            else if (N > 0) memcpy(mxGetPr(wide), mxGetPr(prhs[1]), sizeof(double) * 3 * (size_t)N);
            double c[3];
            for (int k = 0; k < 3; ++k) c[k] = cs ? (double)((const float*)mxGetData(prhs[3]))[k] : mxGetPr(prhs[3])[k];
            mxArray* out = mxCreateNumericMatrix(N > 0 ? N : 1, 3, mxDOUBLE_CLASS, mxREAL);
            mxArray* dd = mxCreateNumericMatrix(N > 0 ? N : 1, 1, mxDOUBLE_CLASS, mxREAL);
            int n = 0;
            rc = pcreg_get_local_points(mxGetPr(wide), N, N > 0 ? N : 1, mxGetScalar(prhs[2]), c, mxGetScalar(prhs[4]), mxGetScalar(prhs[5]), mode,
                                        mxGetPr(out), mxGetPr(dd), &n);
            if (rc == PCREG_OK) {
                const mxClassID cls = mode ? mxSINGLE_CLASS : mxDOUBLE_CLASS;
                plhs[0] = n ? mxCreateNumericMatrix(n, 3, cls, mxREAL) : mxCreateDoubleMatrix(0, 0, mxREAL);          // [] as in the reference
                if (nlhs > 1) plhs[1] = n ? mxCreateNumericMatrix(n, 1, cls, mxREAL) : mxCreateDoubleMatrix(0, 0, mxREAL);
                if (n && mode) {
                    float* o = (float*)mxGetData(plhs[0]); for (size_t k = 0; k < (size_t)n * 3; ++k) o[k] = (float)mxGetPr(out)[k];
                    if (nlhs > 1) { float* q = (float*)mxGetData(plhs[1]); for (int k = 0; k < n; ++k) q[k] = (float)mxGetPr(dd)[k]; }
                } else if (n) {
                    memcpy(mxGetPr(plhs[0]), mxGetPr(out), sizeof(double) * 3 * (size_t)n);
                    if (nlhs > 1) memcpy(mxGetPr(plhs[1]), mxGetPr(dd), sizeof(double) * (size_t)n);
                }
            }
            mxDestroyArray(wide); mxDestroyArray(out); mxDestroyArray(dd);
        }
    } else if (!strcmp(cmd, "modelCreate")) {                 // h = pcreg_mex('modelCreate', single(model)): uploaded and prepared ONCE
        if (nrhs != 2 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3) usage = "modelCreate: model (single M x 3)";
        else {
            int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            if (rc == PCREG_OK) { plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL); *(uint64_t*)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)h; }
        }
    } else if (!strcmp(cmd, "modelMatchPoints")) {            // pairs = pcreg_mex('modelMatchPoints', h, single(surface), thrAbs, maxRatio, unique)
        if (nrhs != 6 || !mxIsUint64(prhs[1]) || !mxIsSingle(prhs[2]) || mxGetN(prhs[2]) != 3) usage = "modelMatchPoints: handle (uint64), surface (single Q x 3), thrAbs, maxRatio, unique";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            int Q = (int)mxGetM(prhs[2]);
            mxArray* buf = mxCreateNumericMatrix(2, Q > 0 ? Q : 1, mxUINT32_CLASS, mxREAL);
            int P = 0;
            rc = pcreg_model_match_points_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, (float)mxGetScalar(prhs[3]), (float)mxGetScalar(prhs[4]),
                                              (int)mxGetScalar(prhs[5]), (uint32_t*)mxGetData(buf), &P);
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
                const uint32_t* src = (const uint32_t*)mxGetData(buf); uint32_t* dst = (uint32_t*)mxGetData(plhs[0]);
                for (int k = 0; k < P; ++k) { dst[k] = src[2 * k]; dst[k + P] = src[2 * k + 1]; }
            }
            mxDestroyArray(buf);
        }
    } else if (!strcmp(cmd, "modelKnn")) {                    // [idx, D2] = pcreg_mex('modelKnn', h, single(Y), k): knnsearch(model, Y, 'K', k)
        if (nrhs != 4 || !mxIsUint64(prhs[1]) || !mxIsSingle(prhs[2]) || mxGetN(prhs[2]) != 3 || mxGetM(prhs[3]) * mxGetN(prhs[3]) != 1 ||
            !(mxGetScalar(prhs[3]) >= 1.0 && mxGetScalar(prhs[3]) <= (double)PCREG_KNN_MAX_K) || mxGetScalar(prhs[3]) != (double)(int)mxGetScalar(prhs[3]))
            usage = "modelKnn: handle (uint64), queries (single Q x 3), k (an integer in 1..32)";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), k = (int)mxGetScalar(prhs[3]);
            mxArray* bi = mxCreateNumericMatrix((size_t)k, Q > 0 ? Q : 1, mxINT32_CLASS, mxREAL);      // [Q][k] row-major
            mxArray* bd = mxCreateNumericMatrix((size_t)k, Q > 0 ? Q : 1, mxSINGLE_CLASS, mxREAL);
            if (Q > 0) rc = pcreg_model_knn_f32(h, (const float*)mxGetData(prhs[2]), Q, Q, k, (int32_t*)mxGetData(bi), (float*)mxGetData(bd));
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateNumericMatrix((size_t)Q, (size_t)k, mxINT32_CLASS, mxREAL);
                plhs[1] = mxCreateNumericMatrix((size_t)Q, (size_t)k, mxSINGLE_CLASS, mxREAL);
                const int32_t* si = (const int32_t*)mxGetData(bi); const float* sd = (const float*)mxGetData(bd);
                int32_t* di = (int32_t*)mxGetData(plhs[0]); float* dd = (float*)mxGetData(plhs[1]);
                for (int i = 0; i < Q; ++i)
                    for (int j = 0; j < k; ++j) { di[i + (size_t)j * Q] = si[(size_t)i * k + j] + 1; dd[i + (size_t)j * Q] = sd[(size_t)i * k + j]; }
            }
            mxDestroyArray(bi); mxDestroyArray(bd);
        }
    } else if (!strcmp(cmd, "modelRange")) {                  // [counts, idx, D2] = pcreg_mex('modelRange', h, single(Y), r): rangesearch(model, Y, r)
        if (nrhs != 4 || !mxIsUint64(prhs[1]) || !mxIsSingle(prhs[2]) || mxGetN(prhs[2]) != 3 || !(mxIsDouble(prhs[3]) || mxIsSingle(prhs[3])) ||
            mxGetM(prhs[3]) * mxGetN(prhs[3]) != 1 || !(mxGetScalar(prhs[3]) >= 0.0))
            usage = "modelRange: handle (uint64), queries (single Q x 3), r (a real scalar >= 0)";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]);
            const float r = (float)mxGetScalar(prhs[3]), r2 = r * r;             // single(r) squared once, in single
            const float* q = (const float*)mxGetData(prhs[2]);
            mxArray* so = mxCreateNumericMatrix((size_t)Q + 1, 1, mxUINT64_CLASS, mxREAL);    // (8-byte elements: seg_off)
            int64_t* seg = (int64_t*)mxGetData(so);
            rc = pcreg_model_range_f32(h, q, Q, Q > 0 ? Q : 1, r2, 0, seg, nullptr, nullptr);       // capacity 0: sizes the result
            if (rc == PCREG_OK) {
                const int64_t total = seg[Q];
                mxArray* oi = mxCreateNumericMatrix((size_t)total, 1, mxINT32_CLASS, mxREAL);
                mxArray* od = mxCreateNumericMatrix((size_t)total, 1, mxSINGLE_CLASS, mxREAL);
                int32_t* di = (int32_t*)mxGetData(oi);
                if (total > 0) rc = pcreg_model_range_f32(h, q, Q, Q, r2, total, seg, di, (float*)mxGetData(od));
                if (rc == PCREG_OK && seg[Q] != total) rc = PCREG_E_ARG;           // (the model cannot change between the two calls)
                if (rc == PCREG_OK) {
                    for (int64_t k = 0; k < total; ++k) di[k] += 1;
                    plhs[0] = mxCreateNumericMatrix((size_t)Q, 1, mxINT32_CLASS, mxREAL);
                    int32_t* dc = (int32_t*)mxGetData(plhs[0]);
                    for (int i = 0; i < Q; ++i) dc[i] = (int32_t)(seg[i + 1] - seg[i]);
                    plhs[1] = oi; plhs[2] = od;
                } else { mxDestroyArray(oi); mxDestroyArray(od); }
            }
            mxDestroyArray(so);
        }
    } else if (!strcmp(cmd, "modelScore")) {                  // [nClose, sumD2, idx, D2] = pcreg_mex('modelScore', h, single(pts), T, maxDist)
        if (nrhs != 5 || !mxIsUint64(prhs[1]) || !mxIsSingle(prhs[2]) || mxGetN(prhs[2]) != 3 || !mxIsDouble(prhs[3]) ||
            (mxGetM(prhs[3]) != 4 && !mxIsEmpty(prhs[3])) || mxGetN(prhs[3]) % 4 != 0 || !radius_ok(prhs[4]))
            usage = "modelScore: handle (uint64), pts (single Q x 3), T (double 4 x 4 x B), maxDist (a real scalar >= 0)";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), B = mxIsEmpty(prhs[3]) ? 0 : (int)(mxGetN(prhs[3]) / 4);
            const float r = (float)mxGetScalar(prhs[4]), r2 = r * r;             // single(maxDist) squared once, in single
            const bool rows = nlhs > 2;
            mxArray* on = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);
            mxArray* os = mxCreateDoubleMatrix((size_t)B, 1, mxREAL);
            mxArray* oi = rows ? mxCreateNumericMatrix((size_t)Q, (size_t)B, mxINT32_CLASS, mxREAL) : nullptr;      // [B][Q] row-major = Q x B
            mxArray* od = rows ? mxCreateNumericMatrix((size_t)Q, (size_t)B, mxSINGLE_CLASS, mxREAL) : nullptr;
            int32_t* di = rows ? (int32_t*)mxGetData(oi) : nullptr;
            if (B > 0) rc = pcreg_model_score_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, mxGetPr(prhs[3]), B, r2, (int32_t*)mxGetData(on),
                                                  mxGetPr(os), di, rows ? (float*)mxGetData(od) : nullptr);
            if (rc == PCREG_OK) {
                for (size_t k = 0; rows && k < (size_t)Q * (size_t)B; ++k) di[k] += 1;
                plhs[0] = on; plhs[1] = os;
                if (rows) { plhs[2] = oi; plhs[3] = od; }
            } else { mxDestroyArray(on); mxDestroyArray(os); mxDestroyArray(oi); mxDestroyArray(od); }
        }
    } else if (!strcmp(cmd, "modelRefit")) {                  // [Tout, nClose, sumD2] = pcreg_mex('modelRefit', h, single(pts), T, maxDist, steps)
        if (nrhs != 6 || !mxIsUint64(prhs[1]) || !mxIsSingle(prhs[2]) || mxGetN(prhs[2]) != 3 || !mxIsDouble(prhs[3]) ||
            (mxGetM(prhs[3]) != 4 && !mxIsEmpty(prhs[3])) || mxGetN(prhs[3]) % 4 != 0 || !radius_ok(prhs[4]) || !mxIsDouble(prhs[5]) ||
            mxGetM(prhs[5]) * mxGetN(prhs[5]) != 1 || !(mxGetScalar(prhs[5]) >= 1.0) || !(mxGetScalar(prhs[5]) <= 1e6) ||
            mxGetScalar(prhs[5]) != (double)(int)mxGetScalar(prhs[5]))
            usage = "modelRefit: handle (uint64), pts (single Q x 3), T (double 4 x 4 x B), maxDist (a real scalar >= 0), steps (a whole number >= 1)";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), B = mxIsEmpty(prhs[3]) ? 0 : (int)(mxGetN(prhs[3]) / 4);
            const float r = (float)mxGetScalar(prhs[4]), r2 = r * r;             // single(maxDist) squared once, in single
            const mwSize dims[3] = {4, 4, (mwSize)B};
            mxArray* ot = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
            mxArray* on = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);
            mxArray* os = mxCreateDoubleMatrix((size_t)B, 1, mxREAL);
            mxArray* oe = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);   // (an empty fit is a zero page of Tout already)
            if (B > 0) rc = pcreg_model_refit_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, mxGetPr(prhs[3]), B, r2, (int)mxGetScalar(prhs[5]),
                                                  mxGetPr(ot), (int32_t*)mxGetData(on), mxGetPr(os), (int32_t*)mxGetData(oe));
            mxDestroyArray(oe);
            if (rc == PCREG_OK) {
                plhs[0] = ot;
                if (nlhs > 1) plhs[1] = on; else mxDestroyArray(on);
                if (nlhs > 2) plhs[2] = os; else mxDestroyArray(os);
            } else { mxDestroyArray(ot); mxDestroyArray(on); mxDestroyArray(os); }
        }
    } else if (!strcmp(cmd, "modelRefitPlane")) {             // [Tout, nClose, sumD2, nPlane, sumRes2] = pcreg_mex('modelRefitPlane', h, single(pts), T, maxDist, steps, normals, k)
        if (nrhs != 8 || !mxIsUint64(prhs[1]) || !mxIsSingle(prhs[2]) || mxGetN(prhs[2]) != 3 || !mxIsDouble(prhs[3]) ||
            (mxGetM(prhs[3]) != 4 && !mxIsEmpty(prhs[3])) || mxGetN(prhs[3]) % 4 != 0 || !radius_ok(prhs[4]) || !mxIsDouble(prhs[5]) ||
            mxGetM(prhs[5]) * mxGetN(prhs[5]) != 1 || !(mxGetScalar(prhs[5]) >= 1.0) || !(mxGetScalar(prhs[5]) <= 1e6) ||
            mxGetScalar(prhs[5]) != (double)(int)mxGetScalar(prhs[5]) || (!mxIsEmpty(prhs[6]) && (!mxIsSingle(prhs[6]) || mxGetN(prhs[6]) != 3)) ||
            !normals_k_ok(prhs[7]))
            usage = "modelRefitPlane: handle (uint64), pts (single Q x 3), T (double 4 x 4 x B), maxDist (a real scalar >= 0), steps (a whole number >= 1), "
                    "normals (single M x 3, or [] to compute them), k (a whole number 3 .. 32)";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), B = mxIsEmpty(prhs[3]) ? 0 : (int)(mxGetN(prhs[3]) / 4);
            const float r = (float)mxGetScalar(prhs[4]), r2 = r * r;             // single(maxDist) squared once, in single
            const bool given = !mxIsEmpty(prhs[6]);
            int M = 0;
            rc = pcreg_model_size(h, &M);
            if (rc == PCREG_OK && given && (int)mxGetM(prhs[6]) != M) usage = "modelRefitPlane: normals must have one row per model row";
            else if (rc == PCREG_OK) {
                const mwSize dims[3] = {4, 4, (mwSize)B};
                mxArray* ot = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
                mxArray* on = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);
                mxArray* os = mxCreateDoubleMatrix((size_t)B, 1, mxREAL);
                mxArray* op = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);
                mxArray* og = mxCreateDoubleMatrix((size_t)B, 1, mxREAL);
                mxArray* oe = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);   // (an empty fit is a zero page of Tout already)
                if (B > 0) rc = pcreg_model_refit_plane_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, mxGetPr(prhs[3]), B, r2,
                                                            (int)mxGetScalar(prhs[5]), given ? (const float*)mxGetData(prhs[6]) : nullptr, M > 0 ? M : 1,
                                                            (int)mxGetScalar(prhs[7]), mxGetPr(ot), (int32_t*)mxGetData(on), mxGetPr(os),
                                                            (int32_t*)mxGetData(op), mxGetPr(og), (int32_t*)mxGetData(oe));
                mxDestroyArray(oe);
                if (rc == PCREG_OK) {
                    plhs[0] = ot;
                    if (nlhs > 1) plhs[1] = on; else mxDestroyArray(on);
                    if (nlhs > 2) plhs[2] = os; else mxDestroyArray(os);
                    if (nlhs > 3) plhs[3] = op; else mxDestroyArray(op);
                    if (nlhs > 4) plhs[4] = og; else mxDestroyArray(og);
                } else { mxDestroyArray(ot); mxDestroyArray(on); mxDestroyArray(os); mxDestroyArray(op); mxDestroyArray(og); }
            }
        }
    } else if (!strcmp(cmd, "modelRefitGicp")) {              // [Tout, nClose, sumD2, nPairs, sumRes2] = pcreg_mex('modelRefitGicp', h, single(pts), T, maxDist, steps, normals, ptsNormals, k, epsilon)
        if (nrhs != 10 || !mxIsUint64(prhs[1]) || !mxIsSingle(prhs[2]) || mxGetN(prhs[2]) != 3 || !mxIsDouble(prhs[3]) ||
            (mxGetM(prhs[3]) != 4 && !mxIsEmpty(prhs[3])) || mxGetN(prhs[3]) % 4 != 0 || !radius_ok(prhs[4]) || !mxIsDouble(prhs[5]) ||
            mxGetM(prhs[5]) * mxGetN(prhs[5]) != 1 || !(mxGetScalar(prhs[5]) >= 1.0) || !(mxGetScalar(prhs[5]) <= 1e6) ||
            mxGetScalar(prhs[5]) != (double)(int)mxGetScalar(prhs[5]) || (!mxIsEmpty(prhs[6]) && (!mxIsSingle(prhs[6]) || mxGetN(prhs[6]) != 3)) ||
            (!mxIsEmpty(prhs[7]) && (!mxIsSingle(prhs[7]) || mxGetN(prhs[7]) != 3)) || !normals_k_ok(prhs[8]) || !mxIsDouble(prhs[9]) ||
            mxGetM(prhs[9]) * mxGetN(prhs[9]) != 1 || !(mxGetScalar(prhs[9]) > 0.0) || !(mxGetScalar(prhs[9]) <= 1.0))
            usage = "modelRefitGicp: handle (uint64), pts (single Q x 3), T (double 4 x 4 x B), maxDist (a real scalar >= 0), steps (a whole number >= 1), "
                    "normals (single M x 3, or [] to compute them), ptsNormals (single Q x 3, or [] to compute them), k (a whole number 3 .. 32), "
                    "epsilon (a double scalar in (0, 1])";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), B = mxIsEmpty(prhs[3]) ? 0 : (int)(mxGetN(prhs[3]) / 4);
            const float r = (float)mxGetScalar(prhs[4]), r2 = r * r;             // single(maxDist) squared once, in single
            const bool given = !mxIsEmpty(prhs[6]), given_q = !mxIsEmpty(prhs[7]);
            int M = 0;
            rc = pcreg_model_size(h, &M);
            if (rc == PCREG_OK && given && (int)mxGetM(prhs[6]) != M) usage = "modelRefitGicp: normals must have one row per model row";
            else if (rc == PCREG_OK && given_q && (int)mxGetM(prhs[7]) != Q) usage = "modelRefitGicp: ptsNormals must have one row per row of pts";
            else if (rc == PCREG_OK) {
                const mwSize dims[3] = {4, 4, (mwSize)B};
                mxArray* ot = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
                mxArray* on = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);
                mxArray* os = mxCreateDoubleMatrix((size_t)B, 1, mxREAL);
                mxArray* op = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);
                mxArray* og = mxCreateDoubleMatrix((size_t)B, 1, mxREAL);
                mxArray* oe = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);   // (an empty fit is a zero page of Tout already)
                if (B > 0) rc = pcreg_model_refit_gicp_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, mxGetPr(prhs[3]), B, r2,
                                                           (int)mxGetScalar(prhs[5]), given ? (const float*)mxGetData(prhs[6]) : nullptr, M > 0 ? M : 1,
                                                           given_q ? (const float*)mxGetData(prhs[7]) : nullptr, Q > 0 ? Q : 1,
                                                           (int)mxGetScalar(prhs[8]), mxGetScalar(prhs[9]), mxGetPr(ot), (int32_t*)mxGetData(on),
                                                           mxGetPr(os), (int32_t*)mxGetData(op), mxGetPr(og), (int32_t*)mxGetData(oe));
                mxDestroyArray(oe);
                if (rc == PCREG_OK) {
                    plhs[0] = ot;
                    if (nlhs > 1) plhs[1] = on; else mxDestroyArray(on);
                    if (nlhs > 2) plhs[2] = os; else mxDestroyArray(os);
                    if (nlhs > 3) plhs[3] = op; else mxDestroyArray(op);
                    if (nlhs > 4) plhs[4] = og; else mxDestroyArray(og);
                } else { mxDestroyArray(ot); mxDestroyArray(on); mxDestroyArray(os); mxDestroyArray(op); mxDestroyArray(og); }
            }
        }
    } else if (!strcmp(cmd, "modelScoreTrimmed")) {           // [nClose, sumD2, idx, D2, nWithin, d2Cut] = pcreg_mex('modelScoreTrimmed', h, single(pts), T, maxDist, keepRatio)
        if (nrhs != 6 || !mxIsUint64(prhs[1]) || !pts_t_ok(prhs[2], prhs[3]) || !radius_ok(prhs[4]) || !ratio_ok(prhs[5]))
            usage = "modelScoreTrimmed: handle (uint64), pts (single Q x 3), T (double 4 x 4 x B), maxDist (a real scalar >= 0), keepRatio (a double scalar in (0, 1])";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), B = mxIsEmpty(prhs[3]) ? 0 : (int)(mxGetN(prhs[3]) / 4);
            const float r = (float)mxGetScalar(prhs[4]), r2 = r * r;             // single(maxDist) squared once, in single
            const bool rows = nlhs > 2;
            mxArray* on = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);
            mxArray* os = mxCreateDoubleMatrix((size_t)B, 1, mxREAL);
            mxArray* oi = rows ? mxCreateNumericMatrix((size_t)Q, (size_t)B, mxINT32_CLASS, mxREAL) : nullptr;      // [B][Q] row-major = Q x B
            mxArray* od = rows ? mxCreateNumericMatrix((size_t)Q, (size_t)B, mxSINGLE_CLASS, mxREAL) : nullptr;
            mxArray* ow = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);
            mxArray* oc = mxCreateNumericMatrix((size_t)B, 1, mxSINGLE_CLASS, mxREAL);
            int32_t* di = rows ? (int32_t*)mxGetData(oi) : nullptr;
            if (B > 0) rc = pcreg_model_score_trimmed_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, mxGetPr(prhs[3]), B, r2, mxGetScalar(prhs[5]),
                                                          (int32_t*)mxGetData(on), mxGetPr(os), di, rows ? (float*)mxGetData(od) : nullptr,
                                                          (int32_t*)mxGetData(ow), (float*)mxGetData(oc));
            if (rc == PCREG_OK) {
                for (size_t k = 0; rows && k < (size_t)Q * (size_t)B; ++k) di[k] += 1;
                plhs[0] = on; plhs[1] = os;
                if (rows) { plhs[2] = oi; plhs[3] = od; }
                if (nlhs > 4) plhs[4] = ow; else mxDestroyArray(ow);
                if (nlhs > 5) plhs[5] = oc; else mxDestroyArray(oc);
            } else { mxDestroyArray(on); mxDestroyArray(os); mxDestroyArray(oi); mxDestroyArray(od); mxDestroyArray(ow); mxDestroyArray(oc); }
        }
    } else if (!strcmp(cmd, "modelRefitTrimmed")) {           // [Tout, nClose, sumD2, nWithin, d2Cut] = pcreg_mex('modelRefitTrimmed', h, single(pts), T, maxDist, keepRatio, steps)
        if (nrhs != 7 || !mxIsUint64(prhs[1]) || !pts_t_ok(prhs[2], prhs[3]) || !radius_ok(prhs[4]) || !ratio_ok(prhs[5]) || !steps_ok(prhs[6]))
            usage = "modelRefitTrimmed: handle (uint64), pts (single Q x 3), T (double 4 x 4 x B), maxDist (a real scalar >= 0), keepRatio (a double scalar in "
                    "(0, 1]), steps (a whole number >= 1)";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), B = mxIsEmpty(prhs[3]) ? 0 : (int)(mxGetN(prhs[3]) / 4);
            const float r = (float)mxGetScalar(prhs[4]), r2 = r * r;             // single(maxDist) squared once, in single
            const mwSize dims[3] = {4, 4, (mwSize)B};
            mxArray* o[5] = {mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL), mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL),
                             mxCreateDoubleMatrix((size_t)B, 1, mxREAL), mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL),
                             mxCreateNumericMatrix((size_t)B, 1, mxSINGLE_CLASS, mxREAL)};
            mxArray* oe = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);   // (an empty fit is a zero page of Tout already)
            if (B > 0) rc = pcreg_model_refit_trimmed_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, mxGetPr(prhs[3]), B, r2, mxGetScalar(prhs[5]),
                                                          (int)mxGetScalar(prhs[6]), mxGetPr(o[0]), (int32_t*)mxGetData(o[1]), mxGetPr(o[2]),
                                                          (int32_t*)mxGetData(oe), (int32_t*)mxGetData(o[3]), (float*)mxGetData(o[4]));
            mxDestroyArray(oe);
            if (rc == PCREG_OK) {
                plhs[0] = o[0];
                if (nlhs > 1) plhs[1] = o[1]; else mxDestroyArray(o[1]);
                if (nlhs > 2) plhs[2] = o[2]; else mxDestroyArray(o[2]);
                if (nlhs > 3) plhs[3] = o[3]; else mxDestroyArray(o[3]);
                if (nlhs > 4) plhs[4] = o[4]; else mxDestroyArray(o[4]);
            } else {
                for (mxArray* a : o) mxDestroyArray(a);
            }
        }
    } else if (!strcmp(cmd, "modelRefitPlaneTrimmed")) {      // [Tout, nClose, sumD2, nPlane, sumRes2, nWithin, d2Cut] = pcreg_mex('modelRefitPlaneTrimmed', h, single(pts), T, maxDist, keepRatio, steps, normals, k)
        if (nrhs != 9 || !mxIsUint64(prhs[1]) || !pts_t_ok(prhs[2], prhs[3]) || !radius_ok(prhs[4]) || !ratio_ok(prhs[5]) || !steps_ok(prhs[6]) ||
            (!mxIsEmpty(prhs[7]) && (!mxIsSingle(prhs[7]) || mxGetN(prhs[7]) != 3)) || !normals_k_ok(prhs[8]))
            usage = "modelRefitPlaneTrimmed: handle (uint64), pts (single Q x 3), T (double 4 x 4 x B), maxDist (a real scalar >= 0), keepRatio (a double scalar "
                    "in (0, 1]), steps (a whole number >= 1), normals (single M x 3, or [] to compute them), k (a whole number 3 .. 32)";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), B = mxIsEmpty(prhs[3]) ? 0 : (int)(mxGetN(prhs[3]) / 4);
            const float r = (float)mxGetScalar(prhs[4]), r2 = r * r;             // single(maxDist) squared once, in single
            const bool given = !mxIsEmpty(prhs[7]);
            int M = 0;
            rc = pcreg_model_size(h, &M);
            if (rc == PCREG_OK && given && (int)mxGetM(prhs[7]) != M) usage = "modelRefitPlaneTrimmed: normals must have one row per model row";
            else if (rc == PCREG_OK) {
                const mwSize dims[3] = {4, 4, (mwSize)B};
                mxArray* o[7] = {mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL), mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL),
                                 mxCreateDoubleMatrix((size_t)B, 1, mxREAL), mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL),
                                 mxCreateDoubleMatrix((size_t)B, 1, mxREAL), mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL),
                                 mxCreateNumericMatrix((size_t)B, 1, mxSINGLE_CLASS, mxREAL)};
                mxArray* oe = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);   // (an empty fit is a zero page of Tout already)
                if (B > 0) rc = pcreg_model_refit_plane_trimmed_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, mxGetPr(prhs[3]), B, r2,
                                                                    mxGetScalar(prhs[5]), (int)mxGetScalar(prhs[6]),
                                                                    given ? (const float*)mxGetData(prhs[7]) : nullptr, M > 0 ? M : 1, (int)mxGetScalar(prhs[8]),
                                                                    mxGetPr(o[0]), (int32_t*)mxGetData(o[1]), mxGetPr(o[2]), (int32_t*)mxGetData(o[3]),
                                                                    mxGetPr(o[4]), (int32_t*)mxGetData(oe), (int32_t*)mxGetData(o[5]), (float*)mxGetData(o[6]));
                mxDestroyArray(oe);
                if (rc == PCREG_OK) {
                    plhs[0] = o[0];
                    if (nlhs > 1) plhs[1] = o[1]; else mxDestroyArray(o[1]);
                    if (nlhs > 2) plhs[2] = o[2]; else mxDestroyArray(o[2]);
                    if (nlhs > 3) plhs[3] = o[3]; else mxDestroyArray(o[3]);
                    if (nlhs > 4) plhs[4] = o[4]; else mxDestroyArray(o[4]);
                    if (nlhs > 5) plhs[5] = o[5]; else mxDestroyArray(o[5]);
                    if (nlhs > 6) plhs[6] = o[6]; else mxDestroyArray(o[6]);
                } else {
                    for (mxArray* a : o) mxDestroyArray(a);
                }
            }
        }
    } else if (!strcmp(cmd, "modelRefitGicpTrimmed")) {       // [Tout, nClose, sumD2, nPairs, sumRes2, nWithin, d2Cut] = pcreg_mex('modelRefitGicpTrimmed', h, single(pts), T, maxDist, keepRatio, steps, normals, ptsNormals, k, epsilon)
        if (nrhs != 11 || !mxIsUint64(prhs[1]) || !pts_t_ok(prhs[2], prhs[3]) || !radius_ok(prhs[4]) || !ratio_ok(prhs[5]) || !steps_ok(prhs[6]) ||
            (!mxIsEmpty(prhs[7]) && (!mxIsSingle(prhs[7]) || mxGetN(prhs[7]) != 3)) || (!mxIsEmpty(prhs[8]) && (!mxIsSingle(prhs[8]) || mxGetN(prhs[8]) != 3)) ||
            !normals_k_ok(prhs[9]) || !mxIsDouble(prhs[10]) || mxGetM(prhs[10]) * mxGetN(prhs[10]) != 1 || !(mxGetScalar(prhs[10]) > 0.0) ||
            !(mxGetScalar(prhs[10]) <= 1.0))
            usage = "modelRefitGicpTrimmed: handle (uint64), pts (single Q x 3), T (double 4 x 4 x B), maxDist (a real scalar >= 0), keepRatio (a double scalar "
                    "in (0, 1]), steps (a whole number >= 1), normals (single M x 3, or [] to compute them), ptsNormals (single Q x 3, or [] to compute them), "
                    "k (a whole number 3 .. 32), epsilon (a double scalar in (0, 1])";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), B = mxIsEmpty(prhs[3]) ? 0 : (int)(mxGetN(prhs[3]) / 4);
            const float r = (float)mxGetScalar(prhs[4]), r2 = r * r;             // single(maxDist) squared once, in single
            const bool given = !mxIsEmpty(prhs[7]), given_q = !mxIsEmpty(prhs[8]);
            int M = 0;
            rc = pcreg_model_size(h, &M);
            if (rc == PCREG_OK && given && (int)mxGetM(prhs[7]) != M) usage = "modelRefitGicpTrimmed: normals must have one row per model row";
            else if (rc == PCREG_OK && given_q && (int)mxGetM(prhs[8]) != Q) usage = "modelRefitGicpTrimmed: ptsNormals must have one row per row of pts";
            else if (rc == PCREG_OK) {
                const mwSize dims[3] = {4, 4, (mwSize)B};
                mxArray* o[7] = {mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL), mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL),
                                 mxCreateDoubleMatrix((size_t)B, 1, mxREAL), mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL),
                                 mxCreateDoubleMatrix((size_t)B, 1, mxREAL), mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL),
                                 mxCreateNumericMatrix((size_t)B, 1, mxSINGLE_CLASS, mxREAL)};
                mxArray* oe = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);   // (an empty fit is a zero page of Tout already)
                if (B > 0) rc = pcreg_model_refit_gicp_trimmed_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, mxGetPr(prhs[3]), B, r2,
                                                                   mxGetScalar(prhs[5]), (int)mxGetScalar(prhs[6]),
                                                                   given ? (const float*)mxGetData(prhs[7]) : nullptr, M > 0 ? M : 1,
                                                                   given_q ? (const float*)mxGetData(prhs[8]) : nullptr, Q > 0 ? Q : 1,
                                                                   (int)mxGetScalar(prhs[9]), mxGetScalar(prhs[10]), mxGetPr(o[0]), (int32_t*)mxGetData(o[1]),
                                                                   mxGetPr(o[2]), (int32_t*)mxGetData(o[3]), mxGetPr(o[4]), (int32_t*)mxGetData(oe),
                                                                   (int32_t*)mxGetData(o[5]), (float*)mxGetData(o[6]));
                mxDestroyArray(oe);
                if (rc == PCREG_OK) {
                    plhs[0] = o[0];
                    if (nlhs > 1) plhs[1] = o[1]; else mxDestroyArray(o[1]);
                    if (nlhs > 2) plhs[2] = o[2]; else mxDestroyArray(o[2]);
                    if (nlhs > 3) plhs[3] = o[3]; else mxDestroyArray(o[3]);
                    if (nlhs > 4) plhs[4] = o[4]; else mxDestroyArray(o[4]);
                    if (nlhs > 5) plhs[5] = o[5]; else mxDestroyArray(o[5]);
                    if (nlhs > 6) plhs[6] = o[6]; else mxDestroyArray(o[6]);
                } else {
                    for (mxArray* a : o) mxDestroyArray(a);
                }
            }
        }
    } else if (!strcmp(cmd, "modelRefitCpd")) {               // [Tout, sigma2Out, Np, sumRes2, sumD2, nLive] = pcreg_mex('modelRefitCpd', h, single(pts), T, sigma2, outlier, steps)
        const int Bt = nrhs == 7 && mxIsDouble(prhs[3]) && !mxIsEmpty(prhs[3]) ? (int)(mxGetN(prhs[3]) / 4) : 0;
        if (nrhs != 7 || !mxIsUint64(prhs[1]) || !mxIsSingle(prhs[2]) || mxGetN(prhs[2]) != 3 || !mxIsDouble(prhs[3]) ||
            (mxGetM(prhs[3]) != 4 && !mxIsEmpty(prhs[3])) || mxGetN(prhs[3]) % 4 != 0 || !mxIsDouble(prhs[4]) ||
            (mxGetM(prhs[4]) * mxGetN(prhs[4]) != 1 && mxGetM(prhs[4]) * mxGetN(prhs[4]) != (size_t)Bt) || !mxIsDouble(prhs[5]) ||
            mxGetM(prhs[5]) * mxGetN(prhs[5]) != 1 || !(mxGetScalar(prhs[5]) >= 0.0) || !(mxGetScalar(prhs[5]) < 1.0) || !whole_scalar_ok(prhs[6], 1.0, 1e6))
            usage = "modelRefitCpd: handle (uint64), pts (single Q x 3), T (double 4 x 4 x B), sigma2 (a double scalar or one per page of T; 0 asks for "
                    "the initial variance), outlier (a double scalar in [0, 1)), steps (a whole number >= 1)";
        else {
            pcreg_model* h = (pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), B = Bt;
            std::vector<double> sig((size_t)(B > 0 ? B : 1), mxGetPr(prhs[4])[0]);
            if (mxGetM(prhs[4]) * mxGetN(prhs[4]) == (size_t)B) memcpy(sig.data(), mxGetPr(prhs[4]), sizeof(double) * (size_t)B);
            const mwSize dims[3] = {4, 4, (mwSize)B};
            mxArray* ot = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
            mxArray* od[4];
            for (mxArray*& a : od) a = mxCreateDoubleMatrix((size_t)B, 1, mxREAL);
            mxArray* on = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);
            mxArray* oe = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);       // (an empty fit is a zero page of Tout already)
            rc = pcreg_model_refit_cpd_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, mxGetPr(prhs[3]), B, sig.data(), mxGetScalar(prhs[5]),
                                           (int)mxGetScalar(prhs[6]), mxGetPr(ot), mxGetPr(od[0]), mxGetPr(od[1]), mxGetPr(od[2]), mxGetPr(od[3]),
                                           (int32_t*)mxGetData(on), (int32_t*)mxGetData(oe));
            mxDestroyArray(oe);
            if (rc == PCREG_OK) {
                plhs[0] = ot;
                for (int i = 0; i < 4; ++i) { if (nlhs > 1 + i) plhs[1 + i] = od[i]; else mxDestroyArray(od[i]); }
                if (nlhs > 5) plhs[5] = on; else mxDestroyArray(on);
            } else { mxDestroyArray(ot); for (mxArray* a : od) mxDestroyArray(a); mxDestroyArray(on); }
        }
    } else if (!strcmp(cmd, "ndtCreate")) {                   // [h, nVoxels, nGaussians] = pcreg_mex('ndtCreate', single(pts), step, minPoints)
        if (nrhs != 4 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !whole_scalar_ok(prhs[3], 3.0, 1e9) || !mxIsDouble(prhs[2]) ||
            mxGetM(prhs[2]) * mxGetN(prhs[2]) != 1 || !(mxGetScalar(prhs[2]) > 0.0) || !std::isfinite(mxGetScalar(prhs[2])))
            usage = "ndtCreate: pts (single n x 3), step (a finite double scalar > 0), minPoints (a whole number >= 3)";
        else {
            const int n = (int)mxGetM(prhs[1]);
            pcreg_ndt* h = nullptr;
            int nv = 0, ng = 0;
            rc = pcreg_ndt_create((const float*)mxGetData(prhs[1]), n, n > 0 ? n : 1, mxGetScalar(prhs[2]), (int)mxGetScalar(prhs[3]), &h);
            if (rc == PCREG_OK) rc = pcreg_ndt_size(h, &nv, &ng);
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL); *(uint64_t*)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)h;
                if (nlhs > 1) plhs[1] = mxCreateDoubleScalar((double)nv);
                if (nlhs > 2) plhs[2] = mxCreateDoubleScalar((double)ng);
            } else if (h) (void)pcreg_ndt_destroy(h);
        }
    } else if (!strcmp(cmd, "ndtRefit")) {                    // [Tout, nPairs, sumE] = pcreg_mex('ndtRefit', h, single(pts), T, neighbors, outlierRatio, steps)
        if (nrhs != 7 || !mxIsUint64(prhs[1]) || !mxIsSingle(prhs[2]) || mxGetN(prhs[2]) != 3 || !mxIsDouble(prhs[3]) ||
            (mxGetM(prhs[3]) != 4 && !mxIsEmpty(prhs[3])) || mxGetN(prhs[3]) % 4 != 0 || !whole_scalar_ok(prhs[4], 1.0, 7.0) ||
            (mxGetScalar(prhs[4]) != 1.0 && mxGetScalar(prhs[4]) != 7.0) || !mxIsDouble(prhs[5]) || mxGetM(prhs[5]) * mxGetN(prhs[5]) != 1 ||
            !(mxGetScalar(prhs[5]) >= 0.0) || !(mxGetScalar(prhs[5]) < 1.0) || !whole_scalar_ok(prhs[6], 1.0, 1e6))
            usage = "ndtRefit: handle (uint64), pts (single Q x 3), T (double 4 x 4 x B), neighbors (1 or 7), outlierRatio (a double scalar in [0, 1)), "
                    "steps (a whole number >= 1)";
        else {
            pcreg_ndt* h = (pcreg_ndt*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            const int Q = (int)mxGetM(prhs[2]), B = mxIsEmpty(prhs[3]) ? 0 : (int)(mxGetN(prhs[3]) / 4);
            const mwSize dims[3] = {4, 4, (mwSize)B};
            mxArray* ot = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
            mxArray* on = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);
            mxArray* os = mxCreateDoubleMatrix((size_t)B, 1, mxREAL);
            mxArray* oe = mxCreateNumericMatrix((size_t)B, 1, mxINT32_CLASS, mxREAL);   // (an empty fit is a zero page of Tout already)
            rc = pcreg_ndt_refit_f32(h, (const float*)mxGetData(prhs[2]), Q, Q > 0 ? Q : 1, mxGetPr(prhs[3]), B, (int)mxGetScalar(prhs[4]),
                                     mxGetScalar(prhs[5]), (int)mxGetScalar(prhs[6]), mxGetPr(ot), (int32_t*)mxGetData(on), mxGetPr(os),
                                     (int32_t*)mxGetData(oe));
            mxDestroyArray(oe);
            if (rc == PCREG_OK) {
                plhs[0] = ot;
                if (nlhs > 1) plhs[1] = on; else mxDestroyArray(on);
                if (nlhs > 2) plhs[2] = os; else mxDestroyArray(os);
            } else { mxDestroyArray(ot); mxDestroyArray(on); mxDestroyArray(os); }
        }
    } else if (!strcmp(cmd, "ndtDestroy")) {
        if (nrhs != 2 || !mxIsUint64(prhs[1])) usage = "ndtDestroy: handle (uint64)";
        else rc = pcreg_ndt_destroy((pcreg_ndt*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]));
    } else if (!strcmp(cmd, "modelCluster")) {                // [label, clOff, members] = pcreg_mex('modelCluster', h, r): clusterPoints(model, r)
        if (nrhs != 3 || !mxIsUint64(prhs[1]) || !radius_ok(prhs[2])) usage = "modelCluster: handle (uint64), r (a real scalar >= 0)";
        else {
            mxArray* out[3] = {nullptr, nullptr, nullptr};
            rc = cluster_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), (float)mxGetScalar(prhs[2]), out);
            if (rc == PCREG_OK) { plhs[0] = out[0]; plhs[1] = out[1]; plhs[2] = out[2]; }
        }
    } else if (!strcmp(cmd, "clusterPoints")) {               // [label, clOff, members] = pcreg_mex('clusterPoints', single(pts), r): clusterPoints(pts, r)
        if (nrhs != 3 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !radius_ok(prhs[2])) usage = "clusterPoints: pts (single M x 3), r (a real scalar >= 0)";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[3] = {nullptr, nullptr, nullptr};
            if (rc == PCREG_OK) rc = cluster_on_handle(h, (float)mxGetScalar(prhs[2]), out);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK) { plhs[0] = out[0]; plhs[1] = out[1]; plhs[2] = out[2]; }
        }
    } else if (!strcmp(cmd, "modelDbscan")) {                 // [label, core, clOff, members] = pcreg_mex('modelDbscan', h, epsilon, minpts)
        if (nrhs != 4 || !mxIsUint64(prhs[1]) || !radius_ok(prhs[2]) || !whole_scalar_ok(prhs[3], 1.0, 2147483647.0))
            usage = "modelDbscan: handle (uint64), epsilon (a real scalar >= 0), minpts (a whole number >= 1)";
        else {
            mxArray* out[4] = {nullptr, nullptr, nullptr, nullptr};
            rc = dbscan_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), (float)mxGetScalar(prhs[2]), (int)mxGetScalar(prhs[3]), out);
            if (rc == PCREG_OK) { plhs[0] = out[0]; plhs[1] = out[1]; plhs[2] = out[2]; plhs[3] = out[3]; }
        }
    } else if (!strcmp(cmd, "dbscanPoints")) {                // [label, core, clOff, members] = pcreg_mex('dbscanPoints', single(pts), epsilon, minpts)
        if (nrhs != 4 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !radius_ok(prhs[2]) || !whole_scalar_ok(prhs[3], 1.0, 2147483647.0))
            usage = "dbscanPoints: pts (single M x 3), epsilon (a real scalar >= 0), minpts (a whole number >= 1)";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[4] = {nullptr, nullptr, nullptr, nullptr};
            if (rc == PCREG_OK) rc = dbscan_on_handle(h, (float)mxGetScalar(prhs[2]), (int)mxGetScalar(prhs[3]), out);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK) { plhs[0] = out[0]; plhs[1] = out[1]; plhs[2] = out[2]; plhs[3] = out[3]; }
        }
    } else if (!strcmp(cmd, "modelNormals")) {                // [normals, variation] = pcreg_mex('modelNormals', h, k, viewpoint)
        if (nrhs != 4 || !mxIsUint64(prhs[1]) || !normals_k_ok(prhs[2]) || !viewpoint_ok(prhs[3]))
            usage = "modelNormals: handle (uint64), k (a whole number 3 .. 32), viewpoint ([] or double 1 x 3)";
        else {
            mxArray* out[2] = {nullptr, nullptr};
            rc = normals_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), (int)mxGetScalar(prhs[2]), prhs[3], nlhs > 1, out);
            if (rc == PCREG_OK) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; }
        }
    } else if (!strcmp(cmd, "pointNormals")) {                // [normals, variation] = pcreg_mex('pointNormals', single(pts), k, viewpoint)
        if (nrhs != 4 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !normals_k_ok(prhs[2]) || !viewpoint_ok(prhs[3]))
            usage = "pointNormals: pts (single M x 3), k (a whole number 3 .. 32), viewpoint ([] or double 1 x 3)";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[2] = {nullptr, nullptr};
            if (rc == PCREG_OK) rc = normals_on_handle(h, (int)mxGetScalar(prhs[2]), prhs[3], nlhs > 1, out);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; }
        }
    } else if (!strcmp(cmd, "modelFpfh")) {                   // [features, spfh] = pcreg_mex('modelFpfh', h, k, normals, kNormals, viewpoint)
        if (nrhs != 6 || !mxIsUint64(prhs[1]) || !normals_k_ok(prhs[2]) || (!mxIsEmpty(prhs[3]) && (!mxIsSingle(prhs[3]) || mxGetN(prhs[3]) != 3)) ||
            !normals_k_ok(prhs[4]) || !viewpoint_ok(prhs[5]))
            usage = "modelFpfh: handle (uint64), k (a whole number 3 .. 32), normals (single M x 3, or [] to compute them), kNormals (a whole number "
                    "3 .. 32), viewpoint ([] or double 1 x 3)";
        else {
            mxArray* out[2] = {nullptr, nullptr};
            rc = fpfh_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), (int)mxGetScalar(prhs[2]), prhs[3], (int)mxGetScalar(prhs[4]),
                                prhs[5], nlhs > 1, out, &usage);
            if (usage) usage = "modelFpfh: normals must have one row per model row";
            if (rc == PCREG_OK && !usage) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; }
        }
    } else if (!strcmp(cmd, "pointFpfh")) {                   // [features, spfh] = pcreg_mex('pointFpfh', single(pts), k, normals, kNormals, viewpoint)
        if (nrhs != 6 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !normals_k_ok(prhs[2]) ||
            (!mxIsEmpty(prhs[3]) && (!mxIsSingle(prhs[3]) || mxGetN(prhs[3]) != 3)) || !normals_k_ok(prhs[4]) || !viewpoint_ok(prhs[5]))
            usage = "pointFpfh: pts (single M x 3), k (a whole number 3 .. 32), normals (single M x 3, or [] to compute them), kNormals (a whole number "
                    "3 .. 32), viewpoint ([] or double 1 x 3)";
        else if (!mxIsEmpty(prhs[3]) && mxGetM(prhs[3]) != mxGetM(prhs[1])) usage = "pointFpfh: normals must have one row per row of pts";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[2] = {nullptr, nullptr};
            if (rc == PCREG_OK) rc = fpfh_on_handle(h, (int)mxGetScalar(prhs[2]), prhs[3], (int)mxGetScalar(prhs[4]), prhs[5], nlhs > 1, out, &usage);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK && !usage) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; }
        }
    } else if (!strcmp(cmd, "modelFpfhRadius")) {             // [features, spfh, nNeighbors] = pcreg_mex('modelFpfhRadius', h, r2, maxNeighbors, normals, kNormals, viewpoint)
        if (nrhs != 7 || !mxIsUint64(prhs[1]) || !fpfh_radius_args_ok(prhs[2], prhs[3]) ||
            (!mxIsEmpty(prhs[4]) && (!mxIsSingle(prhs[4]) || mxGetN(prhs[4]) != 3)) || !normals_k_ok(prhs[5]) || !viewpoint_ok(prhs[6]))
            usage = "modelFpfhRadius: handle (uint64), r2 (a single scalar >= 0, the squared radius), maxNeighbors (a whole number >= 0), normals "
                    "(single M x 3, or [] to compute them), kNormals (a whole number 3 .. 32), viewpoint ([] or double 1 x 3)";
        else {
            mxArray* out[3] = {nullptr, nullptr, nullptr};
            rc = fpfh_radius_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), *(const float*)mxGetData(prhs[2]),
                                       (int)mxGetScalar(prhs[3]), prhs[4], (int)mxGetScalar(prhs[5]), prhs[6], nlhs, out, &usage);
            if (usage) usage = "modelFpfhRadius: normals must have one row per model row";
            if (rc == PCREG_OK && !usage) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; if (out[2]) plhs[2] = out[2]; }
        }
    } else if (!strcmp(cmd, "pointFpfhRadius")) {             // [features, spfh, nNeighbors] = pcreg_mex('pointFpfhRadius', single(pts), r2, maxNeighbors, normals, kNormals, viewpoint)
        if (nrhs != 7 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !fpfh_radius_args_ok(prhs[2], prhs[3]) ||
            (!mxIsEmpty(prhs[4]) && (!mxIsSingle(prhs[4]) || mxGetN(prhs[4]) != 3)) || !normals_k_ok(prhs[5]) || !viewpoint_ok(prhs[6]))
            usage = "pointFpfhRadius: pts (single M x 3), r2 (a single scalar >= 0, the squared radius), maxNeighbors (a whole number >= 0), normals "
                    "(single M x 3, or [] to compute them), kNormals (a whole number 3 .. 32), viewpoint ([] or double 1 x 3)";
        else if (!mxIsEmpty(prhs[4]) && mxGetM(prhs[4]) != mxGetM(prhs[1])) usage = "pointFpfhRadius: normals must have one row per row of pts";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[3] = {nullptr, nullptr, nullptr};
            if (rc == PCREG_OK) rc = fpfh_radius_on_handle(h, *(const float*)mxGetData(prhs[2]), (int)mxGetScalar(prhs[3]), prhs[4], (int)mxGetScalar(prhs[5]),
                                                           prhs[6], nlhs, out, &usage);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK && !usage) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; if (out[2]) plhs[2] = out[2]; }
        }
    } else if (!strcmp(cmd, "modelDenoise")) {                // [inlierIndices, meanDist, thr] = pcreg_mex('modelDenoise', h, k, threshold)
        if (nrhs != 4 || !mxIsUint64(prhs[1]) || !denoise_k_ok(prhs[2]) || !denoise_t_ok(prhs[3]))
            usage = "modelDenoise: handle (uint64), k (a whole number 1 .. 31), threshold (a finite double scalar >= 0)";
        else {
            mxArray* out[3] = {nullptr, nullptr, nullptr};
            rc = denoise_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), (int)mxGetScalar(prhs[2]), mxGetScalar(prhs[3]), nlhs, out);
            if (rc == PCREG_OK) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; if (out[2]) plhs[2] = out[2]; }
        }
    } else if (!strcmp(cmd, "pointDenoise")) {                // [inlierIndices, meanDist, thr] = pcreg_mex('pointDenoise', single(pts), k, threshold)
        if (nrhs != 4 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !denoise_k_ok(prhs[2]) || !denoise_t_ok(prhs[3]))
            usage = "pointDenoise: pts (single M x 3), k (a whole number 1 .. 31), threshold (a finite double scalar >= 0)";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[3] = {nullptr, nullptr, nullptr};
            if (rc == PCREG_OK) rc = denoise_on_handle(h, (int)mxGetScalar(prhs[2]), mxGetScalar(prhs[3]), nlhs, out);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; if (out[2]) plhs[2] = out[2]; }
        }
    } else if (!strcmp(cmd, "modelFps")) {                    // [idx, d2, label, minD2, coverD2] = pcreg_mex('modelFps', h, K, start, stopD2)
        if (nrhs != 5 || !mxIsUint64(prhs[1]) || !fps_args_ok(prhs + 2))
            usage = "modelFps: handle (uint64), K (a whole number >= 0), start (a 1-based row, or 0 for the lowest finite row), stopD2 (a single "
                    "scalar >= 0, the squared stop distance)";
        else {
            mxArray* out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
            rc = fps_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), (int)mxGetScalar(prhs[2]), (int)mxGetScalar(prhs[3]),
                               *(const float*)mxGetData(prhs[4]), nlhs, out);
            if (rc == PCREG_OK) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; if (out[2]) plhs[2] = out[2]; if (out[3]) plhs[3] = out[3]; if (out[4]) plhs[4] = out[4]; }
        }
    } else if (!strcmp(cmd, "pointFps")) {                    // [idx, d2, label, minD2, coverD2] = pcreg_mex('pointFps', single(pts), K, start, stopD2)
        if (nrhs != 5 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !fps_args_ok(prhs + 2))
            usage = "pointFps: pts (single M x 3), K (a whole number >= 0), start (a 1-based row, or 0 for the lowest finite row), stopD2 (a single "
                    "scalar >= 0, the squared stop distance)";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
            if (rc == PCREG_OK) rc = fps_on_handle(h, (int)mxGetScalar(prhs[2]), (int)mxGetScalar(prhs[3]), *(const float*)mxGetData(prhs[4]), nlhs, out);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; if (out[2]) plhs[2] = out[2]; if (out[3]) plhs[3] = out[3]; if (out[4]) plhs[4] = out[4]; }
        }
    } else if (!strcmp(cmd, "modelIss")) {                   // [keypoints, saliency, eig, nNeighbors] = pcreg_mex('modelIss', h, r2s, r2n, t21, t32, minNb)
        if (nrhs != 7 || !mxIsUint64(prhs[1]) || !iss_args_ok(prhs + 2))
            usage = "modelIss: handle (uint64), r2Salient and r2NonMax (single scalars, the squared radii: finite, normal, > 0), threshold21 and "
                    "threshold32 (finite double scalars > 0), minNeighbors (a whole number >= 1)";
        else {
            mxArray* out[4] = {nullptr, nullptr, nullptr, nullptr};
            rc = iss_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), prhs + 2, nlhs, out);
            if (rc == PCREG_OK) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; if (out[2]) plhs[2] = out[2]; if (out[3]) plhs[3] = out[3]; }
        }
    } else if (!strcmp(cmd, "pointIss")) {                    // [keypoints, saliency, eig, nNeighbors] = pcreg_mex('pointIss', single(pts), r2s, r2n, t21, t32, minNb)
        if (nrhs != 7 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !iss_args_ok(prhs + 2))
            usage = "pointIss: pts (single M x 3), r2Salient and r2NonMax (single scalars, the squared radii: finite, normal, > 0), threshold21 and "
                    "threshold32 (finite double scalars > 0), minNeighbors (a whole number >= 1)";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[4] = {nullptr, nullptr, nullptr, nullptr};
            if (rc == PCREG_OK) rc = iss_on_handle(h, prhs + 2, nlhs, out);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK) { plhs[0] = out[0]; if (out[1]) plhs[1] = out[1]; if (out[2]) plhs[2] = out[2]; if (out[3]) plhs[3] = out[3]; }
        }
    } else if (!strcmp(cmd, "modelPlanes")) {                 // [labels, planes, centres, counts, rmse, diag] = pcreg_mex('modelPlanes', h, t, ref, ang, P, B, minInl, seed, samples)
        if (nrhs != 10 || !mxIsUint64(prhs[1]) || !planes_args_ok(prhs + 2))
            usage = "modelPlanes: handle (uint64), maxDistance (a single scalar: finite, normal, > 0), refVec ([] or a finite non-zero double 1 x 3), maxAngle (a double "
                    "scalar, radians, in (0, pi/2] with a refVec), maxPlanes (1 .. 64), nTrials (1 .. 2^20), minInliers (>= 3), seed (a whole number "
                    ">= 0), samples ([] or int32 3 x nTrials * maxPlanes)";
        else {
            mxArray* out[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            rc = planes_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), prhs + 2, nlhs, out);
            if (rc == PCREG_OK) {
                plhs[0] = out[0];
                if (out[1]) plhs[1] = out[1];
                if (out[2]) plhs[2] = out[2];
                if (out[3]) plhs[3] = out[3];
                if (out[4]) plhs[4] = out[4];
                if (out[5]) plhs[5] = out[5];
            }
        }
    } else if (!strcmp(cmd, "pointPlanes")) {                 // [labels, planes, centres, counts, rmse, diag] = pcreg_mex('pointPlanes', single(pts), t, ref, ang, P, B, minInl, seed, samples)
        if (nrhs != 10 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !planes_args_ok(prhs + 2))
            usage = "pointPlanes: pts (single M x 3), maxDistance (a single scalar: finite, normal, > 0), refVec ([] or a finite non-zero double 1 x 3), maxAngle (a double "
                    "scalar, radians, in (0, pi/2] with a refVec), maxPlanes (1 .. 64), nTrials (1 .. 2^20), minInliers (>= 3), seed (a whole number "
                    ">= 0), samples ([] or int32 3 x nTrials * maxPlanes)";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            if (rc == PCREG_OK) rc = planes_on_handle(h, prhs + 2, nlhs, out);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK) {
                plhs[0] = out[0];
                if (out[1]) plhs[1] = out[1];
                if (out[2]) plhs[2] = out[2];
                if (out[3]) plhs[3] = out[3];
                if (out[4]) plhs[4] = out[4];
                if (out[5]) plhs[5] = out[5];
            }
        }
    } else if (!strcmp(cmd, "modelFitSpheres")) {             // [labels, spheres, counts, rmse, refitUsed, diag] = pcreg_mex('modelFitSpheres', h, t, rmin, rmax, P, B, minInl, seed, samples)
        if (nrhs != 10 || !mxIsUint64(prhs[1]) || !fit_spheres_args_ok(prhs + 2))
            usage = "modelFitSpheres: handle (uint64), maxDistance (a single scalar: finite, normal, > 0), minRadius and maxRadius (single scalars, 0 <= minRadius <= maxRadius), "
                    "maxSpheres (1 .. 64), nTrials (1 .. 2^20), minInliers (>= 4), seed (a whole number >= 0), samples ([] or int32 4 x nTrials * "
                    "maxSpheres)";
        else {
            mxArray* out[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            rc = fit_spheres_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), prhs + 2, nlhs, out);
            if (rc == PCREG_OK) {
                plhs[0] = out[0];
                if (out[1]) plhs[1] = out[1];
                if (out[2]) plhs[2] = out[2];
                if (out[3]) plhs[3] = out[3];
                if (out[4]) plhs[4] = out[4];
                if (out[5]) plhs[5] = out[5];
            }
        }
    } else if (!strcmp(cmd, "pointFitSpheres")) {             // [labels, spheres, counts, rmse, refitUsed, diag] = pcreg_mex('pointFitSpheres', single(pts), t, rmin, rmax, P, B, minInl, seed, samples)
        if (nrhs != 10 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !fit_spheres_args_ok(prhs + 2))
            usage = "pointFitSpheres: pts (single M x 3), maxDistance (a single scalar: finite, normal, > 0), minRadius and maxRadius (single scalars, 0 <= minRadius <= maxRadius), "
                    "maxSpheres (1 .. 64), nTrials (1 .. 2^20), minInliers (>= 4), seed (a whole number >= 0), samples ([] or int32 4 x nTrials * "
                    "maxSpheres)";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            if (rc == PCREG_OK) rc = fit_spheres_on_handle(h, prhs + 2, nlhs, out);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK) {
                plhs[0] = out[0];
                if (out[1]) plhs[1] = out[1];
                if (out[2]) plhs[2] = out[2];
                if (out[3]) plhs[3] = out[3];
                if (out[4]) plhs[4] = out[4];
                if (out[5]) plhs[5] = out[5];
            }
        }
    } else if (!strcmp(cmd, "modelFitCylinders")) {           // [labels, cylinders, extents, counts, rmse, refitUsed, diag] = pcreg_mex('modelFitCylinders', h, t, rmin, rmax, refVec, maxAngle, normals, kNormals, P, B, minInl, seed, samples)
        if (nrhs != 14 || !mxIsUint64(prhs[1]) || !fit_cylinders_args_ok(prhs + 2, mxIsEmpty(prhs[7]) ? 0 : mxGetM(prhs[7])))
            usage = "modelFitCylinders: handle (uint64), maxDistance (a single scalar: finite, normal, > 0), minRadius and maxRadius (single scalars, 0 <= minRadius <= maxRadius), "
                    "refVec ([] or a double 1 x 3, finite, not all zero), maxAngle (a double scalar, radians, in (0, pi/2] with refVec), normals ([] or single M x 3), "
                    "kNormals (3 .. 32), maxCylinders (1 .. 64), nTrials (1 .. 2^20), minInliers (>= 4), seed (a whole number >= 0), samples ([] or int32 "
                    "2 x nTrials * maxCylinders)";
        else {
            mxArray* out[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            rc = fit_cylinders_on_handle((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]), prhs + 2, nlhs, out);
            if (rc == PCREG_OK) {
                plhs[0] = out[0];
                if (out[1]) plhs[1] = out[1];
                if (out[2]) plhs[2] = out[2];
                if (out[3]) plhs[3] = out[3];
                if (out[4]) plhs[4] = out[4];
                if (out[5]) plhs[5] = out[5];
                if (out[6]) plhs[6] = out[6];
            }
        }
    } else if (!strcmp(cmd, "pointFitCylinders")) {           // [labels, cylinders, extents, counts, rmse, refitUsed, diag] = pcreg_mex('pointFitCylinders', single(pts), t, rmin, rmax, refVec, maxAngle, normals, kNormals, P, B, minInl, seed, samples)
        if (nrhs != 14 || !mxIsSingle(prhs[1]) || mxGetN(prhs[1]) != 3 || !fit_cylinders_args_ok(prhs + 2, mxGetM(prhs[1])))
            usage = "pointFitCylinders: pts (single M x 3), maxDistance (a single scalar: finite, normal, > 0), minRadius and maxRadius (single scalars, 0 <= minRadius <= maxRadius), "
                    "refVec ([] or a double 1 x 3, finite, not all zero), maxAngle (a double scalar, radians, in (0, pi/2] with refVec), normals ([] or single M x 3), "
                    "kNormals (3 .. 32), maxCylinders (1 .. 64), nTrials (1 .. 2^20), minInliers (>= 4), seed (a whole number >= 0), samples ([] or int32 "
                    "2 x nTrials * maxCylinders)";
        else {
            const int M = (int)mxGetM(prhs[1]);
            pcreg_model* h = nullptr;
            rc = pcreg_model_create((const float*)mxGetData(prhs[1]), M, M > 0 ? M : 1, &h);
            mxArray* out[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            if (rc == PCREG_OK) rc = fit_cylinders_on_handle(h, prhs + 2, nlhs, out);
            if (h) (void)pcreg_model_destroy(h);
            if (rc == PCREG_OK) {
                plhs[0] = out[0];
                if (out[1]) plhs[1] = out[1];
                if (out[2]) plhs[2] = out[2];
                if (out[3]) plhs[3] = out[3];
                if (out[4]) plhs[4] = out[4];
                if (out[5]) plhs[5] = out[5];
                if (out[6]) plhs[6] = out[6];
            }
        }
    } else if (!strcmp(cmd, "uniqueRows3")) {                 // ia = pcreg_mex('uniqueRows3', A): [C, ia] = unique(A, 'rows') with C = A(ia, :)
        if (nrhs != 2 || !mxIsDouble(prhs[1]) || (mxGetN(prhs[1]) != 3 && !mxIsEmpty(prhs[1]))) usage = "uniqueRows3: A (double n x 3)";
        else {
            const int n = mxIsEmpty(prhs[1]) ? 0 : (int)mxGetM(prhs[1]);
            mxArray* tmp = mxCreateNumericMatrix(n > 0 ? n : 1, 1, mxINT32_CLASS, mxREAL);
            int nu = 0;
            rc = pcreg_unique_rows3(mxGetPr(prhs[1]), n, n > 0 ? n : 1, (int32_t*)mxGetData(tmp), &nu);
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateDoubleMatrix(nu, nu > 0 ? 1 : 0, mxREAL);
                const int32_t* src = (const int32_t*)mxGetData(tmp);
                for (int k = 0; k < nu; ++k) mxGetPr(plhs[0])[k] = (double)src[k];
            }
            mxDestroyArray(tmp);
        }
    } else if (!strcmp(cmd, "aggregateMatches")) {            // [pts1u, pts2u, ia] = pcreg_mex('aggregateMatches', pts1, pts2)
        if (nrhs != 3 || !mxIsDouble(prhs[1]) || !mxIsDouble(prhs[2]) || mxGetM(prhs[1]) != mxGetM(prhs[2]) ||
            (!mxIsEmpty(prhs[1]) && (mxGetN(prhs[1]) != 3 || mxGetN(prhs[2]) != 3)))
            usage = "aggregateMatches: pts1, pts2 (double n x 3 each, the same n)";
        else {
            const int n = mxIsEmpty(prhs[1]) ? 0 : (int)mxGetM(prhs[1]);
            const size_t ld = n > 0 ? n : 1;
            mxArray* t1 = mxCreateDoubleMatrix(ld, 3, mxREAL);
            mxArray* t2 = mxCreateDoubleMatrix(ld, 3, mxREAL);
            mxArray* ti = mxCreateNumericMatrix(ld, 1, mxINT32_CLASS, mxREAL);
            int nu = 0;
            rc = pcreg_aggregate_matches(mxGetPr(prhs[1]), mxGetPr(prhs[2]), n, (int)ld, mxGetPr(t1), mxGetPr(t2), (int)ld, (int32_t*)mxGetData(ti), &nu);
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateDoubleMatrix(nu, 3, mxREAL);
                if (nlhs > 1) plhs[1] = mxCreateDoubleMatrix(nu, 3, mxREAL);
                if (nlhs > 2) plhs[2] = mxCreateDoubleMatrix(nu, nu > 0 ? 1 : 0, mxREAL);
                for (int c = 0; c < 3; ++c)
                    for (int k = 0; k < nu; ++k) {
                        mxGetPr(plhs[0])[k + (size_t)c * nu] = mxGetPr(t1)[k + c * ld];
                        if (nlhs > 1) mxGetPr(plhs[1])[k + (size_t)c * nu] = mxGetPr(t2)[k + c * ld];
                    }
                if (nlhs > 2) for (int k = 0; k < nu; ++k) mxGetPr(plhs[2])[k] = (double)((const int32_t*)mxGetData(ti))[k];
            }
            mxDestroyArray(t1); mxDestroyArray(t2); mxDestroyArray(ti);
        }
    } else if (!strcmp(cmd, "downsampleGrid")) {              // [ptsOut, counts, labels] = pcreg_mex('downsampleGrid', single(pts), gridStep)
        if (nrhs == 3 && mxIsDouble(prhs[1]) && !mxIsEmpty(prhs[1]))
            usage = "downsampleGrid: the cloud must be single -- pass single(pts); the result keeps the class of the input";
        else if (nrhs != 3 || !(mxIsSingle(prhs[1]) || mxIsEmpty(prhs[1])) || (mxGetN(prhs[1]) != 3 && !mxIsEmpty(prhs[1])) || !mxIsDouble(prhs[2]) ||
                 mxGetM(prhs[2]) * mxGetN(prhs[2]) != 1 || !(mxGetScalar(prhs[2]) > 0.0) || !(mxGetScalar(prhs[2]) <= 1.7976931348623157e308))
            usage = "downsampleGrid: pts (single n x 3), gridStep (a finite double scalar > 0)";
        else {
            const int n = mxIsEmpty(prhs[1]) ? 0 : (int)mxGetM(prhs[1]);
            const size_t ld = n > 0 ? n : 1;
            mxArray* to = mxCreateNumericMatrix(ld, 3, mxSINGLE_CLASS, mxREAL);
            mxArray* tc = mxCreateNumericMatrix(ld, 1, mxINT32_CLASS, mxREAL);
            mxArray* tl = mxCreateNumericMatrix((size_t)n, n > 0 ? 1 : 0, mxINT32_CLASS, mxREAL);
            int u = 0;
            rc = pcreg_downsample_grid_f32(n > 0 ? (const float*)mxGetData(prhs[1]) : nullptr, n, (int)ld, mxGetScalar(prhs[2]), (float*)mxGetData(to),
                                           (int)ld, nlhs > 1 ? (int32_t*)mxGetData(tc) : nullptr, nlhs > 2 && n > 0 ? (int32_t*)mxGetData(tl) : nullptr, &u);
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateNumericMatrix((size_t)u, 3, mxSINGLE_CLASS, mxREAL);
                for (int c = 0; c < 3; ++c)
                    if (u > 0) memcpy((float*)mxGetData(plhs[0]) + (size_t)c * u, (const float*)mxGetData(to) + c * ld, (size_t)u * sizeof(float));
                if (nlhs > 1) {
                    plhs[1] = mxCreateNumericMatrix((size_t)u, u > 0 ? 1 : 0, mxINT32_CLASS, mxREAL);
                    if (u > 0) memcpy(mxGetData(plhs[1]), mxGetData(tc), (size_t)u * sizeof(int32_t));
                }
                if (nlhs > 2) { plhs[2] = tl; tl = nullptr; }             // (no live row: the library wrote nothing, the zeros stand)
            }
            mxDestroyArray(to); mxDestroyArray(tc);
            if (tl) mxDestroyArray(tl);
        }
    } else if (!strcmp(cmd, "descCreate")) {                  // h = pcreg_mex('descCreate', desc): an n x D double descriptor set, uploaded ONCE
        if (nrhs != 2 || !mxIsDouble(prhs[1])) usage = "descCreate: desc (double n x D)";
        else {
            const int n = (int)mxGetM(prhs[1]), D = (int)mxGetN(prhs[1]);
            pcreg_desc_set* h = nullptr;
            rc = pcreg_desc_set_create(mxGetPr(prhs[1]), n, n > 0 ? n : 1, D > 0 ? D : 1, &h);
            if (rc == PCREG_OK) { plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL); *(uint64_t*)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)h; }
        }
    } else if (!strcmp(cmd, "getMatchesOnSet")) {             // matches = pcreg_mex('getMatchesOnSet', hSurface, hModel, int32(rows) | [], par)
        // = getMatches(descSurface, descModel(rows, :), par) on the resident sets (rows 1-based, ascending; []: the whole model set)
        if (nrhs != 5 || !mxIsUint64(prhs[1]) || !mxIsUint64(prhs[2]) || !(mxIsInt32(prhs[3]) || mxGetM(prhs[3]) * mxGetN(prhs[3]) == 0))
            usage = "getMatchesOnSet: hSurface (uint64), hModel (uint64), int32 rows or [], par";
        else {
            const mxArray* p = prhs[4];
            pcreg_match_opts o;
            o.metric = field_is(p, "Metric", "SAD") ? PCREG_METRIC_SAD : PCREG_METRIC_SSD;
            o.matchThreshold = field(p, "MatchThreshold", 1.0); o.maxRatio = field(p, "MaxRatio", 0.6);
            o.unique = (int)field(p, "Unique", 0); o.prenormalized = 0;
            o.unnormalize = (int)field(p, "UNNORMALIZE", 0); o.norm_factor = field(p, "norm_factor", 0.0);
            o.change_metric = (int)field(p, "CHANGE_METRIC", 0); o.metric_factor = field(p, "metric_factor", 1.0);
            pcreg_desc_set* hS = (pcreg_desc_set*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            pcreg_desc_set* hM = (pcreg_desc_set*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[2]);
            int Q = 0, D = 0;
            rc = pcreg_desc_set_size(hS, &Q, &D);
            const size_t nr = mxGetM(prhs[3]) * mxGetN(prhs[3]);
            mxArray* r0 = mxCreateNumericMatrix(nr > 0 ? nr : 1, 1, mxINT32_CLASS, mxREAL);          // 0-based copy of the row list
            if (nr > 0) { const int32_t* r1 = (const int32_t*)mxGetData(prhs[3]); int32_t* z = (int32_t*)mxGetData(r0); for (size_t k = 0; k < nr; ++k) z[k] = r1[k] - 1; }
            mxArray* buf = mxCreateNumericMatrix(2, Q > 0 ? Q : 1, mxUINT32_CLASS, mxREAL);
            int P = 0;
            if (rc == PCREG_OK) rc = pcreg_get_matches_on_sets(hS, hM, nr > 0 ? (const int32_t*)mxGetData(r0) : nullptr, (int)nr, &o, (uint32_t*)mxGetData(buf), nullptr, &P);
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
                const uint32_t* src = (const uint32_t*)mxGetData(buf); uint32_t* dst = (uint32_t*)mxGetData(plhs[0]);
                for (int k = 0; k < P; ++k) { dst[k] = src[2 * k]; dst[k + P] = src[2 * k + 1]; }
            }
            mxDestroyArray(buf); mxDestroyArray(r0);
        }
    } else if (!strcmp(cmd, "getMatchesSegmentedOnSet")) {    // [pairs, nPairs] = pcreg_mex('getMatchesSegmentedOnSet', hSurface, hModel, int32(rows), int32(segOff), par)
        // getMatchesSegmented on the resident sets: rows / segOff / outputs as there.  matlab/getMatchesSegmentedOnSet.m
        if (nrhs != 6 || !mxIsUint64(prhs[1]) || !mxIsUint64(prhs[2]) || !mxIsInt32(prhs[3]) || !mxIsInt32(prhs[4]))
            usage = "getMatchesSegmentedOnSet: hSurface (uint64), hModel (uint64), int32 rows, int32 segOff, par";
        else {
            const mxArray* p = prhs[5];
            pcreg_match_opts o;
            o.metric = field_is(p, "Metric", "SAD") ? PCREG_METRIC_SAD : PCREG_METRIC_SSD;
            o.matchThreshold = field(p, "MatchThreshold", 1.0); o.maxRatio = field(p, "MaxRatio", 0.6);
            o.unique = (int)field(p, "Unique", 0); o.prenormalized = 0;
            o.unnormalize = (int)field(p, "UNNORMALIZE", 0); o.norm_factor = field(p, "norm_factor", 0.0);
            o.change_metric = (int)field(p, "CHANGE_METRIC", 0); o.metric_factor = field(p, "metric_factor", 1.0);
            pcreg_desc_set* hS = (pcreg_desc_set*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            pcreg_desc_set* hM = (pcreg_desc_set*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[2]);
            int Q = 0, D = 0;
            rc = pcreg_desc_set_size(hS, &Q, &D);
            const int S = (int)(mxGetM(prhs[4]) * mxGetN(prhs[4])) - 1;
            const size_t tot = mxGetM(prhs[3]) * mxGetN(prhs[3]);
            const int32_t* off = (const int32_t*)mxGetData(prhs[4]);
            if (S < 0 || off[0] != 0 || (size_t)off[S] != tot) usage = "getMatchesSegmentedOnSet: segOff must run from 0 to numel(rows)";
            else if (rc == PCREG_OK) {
                mxArray* r0 = mxCreateNumericMatrix(tot > 0 ? tot : 1, 1, mxINT32_CLASS, mxREAL);
                mxArray* buf = mxCreateNumericMatrix(2, (size_t)(S > 0 ? S : 1) * (Q > 0 ? Q : 1), mxUINT32_CLASS, mxREAL);
                mxArray* np = mxCreateNumericMatrix(S > 0 ? S : 1, 1, mxINT32_CLASS, mxREAL);
                int32_t* rz = (int32_t*)mxGetData(r0); const int32_t* r1 = (const int32_t*)mxGetData(prhs[3]);
                for (size_t k = 0; k < tot; ++k) rz[k] = r1[k] - 1;
                rc = pcreg_get_matches_segmented_on_sets(hS, hM, rz, off, S, &o, (uint32_t*)mxGetData(buf), (int32_t*)mxGetData(np));
                if (rc == PCREG_OK) {
                    const int32_t* n = (const int32_t*)mxGetData(np);
                    size_t P = 0; for (int z = 0; z < S; ++z) P += (size_t)n[z];
                    plhs[0] = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
                    const uint32_t* src = (const uint32_t*)mxGetData(buf); uint32_t* dst = (uint32_t*)mxGetData(plhs[0]);
                    size_t k = 0;
                    for (int z = 0; z < S; ++z)
                        for (int e = 0; e < n[z]; ++e, ++k) { dst[k] = src[((size_t)z * Q + e) * 2]; dst[k + P] = src[((size_t)z * Q + e) * 2 + 1]; }
                    if (nlhs > 1) { plhs[1] = mxCreateNumericMatrix(S, 1, mxINT32_CLASS, mxREAL); memcpy(mxGetData(plhs[1]), n, (size_t)S * 4); }
                }
                mxDestroyArray(r0); mxDestroyArray(buf); mxDestroyArray(np);
            }
        }
    } else if (!strcmp(cmd, "sphereCounts")) {                // counts = pcreg_mex('sphereCounts', featModel, centres, R): completeExperimentFast.m:52-64
        if (nrhs != 4 || !mxIsDouble(prhs[1]) || !mxIsDouble(prhs[2]) || mxGetN(prhs[1]) != 3 || mxGetN(prhs[2]) != 3) usage = "sphereCounts: featModel (n x 3 double), centres (S x 3 double), R";
        else {
            const int VM = (int)mxGetM(prhs[1]), S = (int)mxGetM(prhs[2]);
            mxArray* cnt = mxCreateNumericMatrix(S > 0 ? S : 1, 1, mxINT32_CLASS, mxREAL);
            rc = pcreg_sphere_counts(mxGetPr(prhs[1]), VM, VM > 0 ? VM : 1, mxGetPr(prhs[2]), S, S > 0 ? S : 1, mxGetScalar(prhs[3]), (int32_t*)mxGetData(cnt));
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateDoubleMatrix(S, S ? 1 : 0, mxREAL);
                const int32_t* c = (const int32_t*)mxGetData(cnt);
                for (int i = 0; i < S; ++i) mxGetPr(plhs[0])[i] = (double)c[i];
            }
            mxDestroyArray(cnt);
        }
    } else if (!strcmp(cmd, "sphereSweep")) {
        // [modelRows, pairs, nPairs, trial, T, numSuccess, maxInliers, failed] = pcreg_mex('sphereSweep', hSurface, hModel, featSurface, featModel,
        //     centres, int32(numDesc), R_desc, par, putativeThresh, ransacCoef, seed)
        // completeExperimentFast.m:101-224 for the spheres kept after sphereCounts.  modelRows: the spheres' row lists back to back (1-based);
        // pairs: sum(nPairs) x 2 uint32, sphere after sphere; trial: the registered spheres (1-based); T: 4 x 4 x numel(trial).  matlab/sphereSweep.m
        if (nrhs != 12 || !mxIsUint64(prhs[1]) || !mxIsUint64(prhs[2]) || !mxIsDouble(prhs[3]) || !mxIsDouble(prhs[4]) || !mxIsDouble(prhs[5]) || !mxIsInt32(prhs[6]))
            usage = "sphereSweep: hSurface, hModel (uint64), featSurface, featModel, centres (double n x 3), int32 numDesc, R_desc, par, putativeThresh, ransacCoef, seed";
        else {
            const mxArray* p = prhs[8];
            pcreg_match_opts o;
            o.metric = field_is(p, "Metric", "SAD") ? PCREG_METRIC_SAD : PCREG_METRIC_SSD;
            o.matchThreshold = field(p, "MatchThreshold", 1.0); o.maxRatio = field(p, "MaxRatio", 0.6);
            o.unique = (int)field(p, "Unique", 0); o.prenormalized = 0;
            o.unnormalize = (int)field(p, "UNNORMALIZE", 0); o.norm_factor = field(p, "norm_factor", 0.0);
            o.change_metric = (int)field(p, "CHANGE_METRIC", 0); o.metric_factor = field(p, "metric_factor", 1.0);
            const mxArray* c = prhs[10];
            pcreg_ransac_opts ro;
            ro.minPtNum = (int)field(c, "minPtNum", 3); ro.iterNum = (int)field(c, "iterNum", 1000);
            ro.thDist = field(c, "thDist", 0.5); ro.thInlrRatio = field(c, "thInlrRatio", 0.1);
            ro.REFINE = (int)field(c, "REFINE", 1); ro.VERBOSE = 0;
            ro.seed = (uint64_t)mxGetScalar(prhs[11]);
            pcreg_desc_set* hS = (pcreg_desc_set*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            pcreg_desc_set* hM = (pcreg_desc_set*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[2]);
            int Q = 0, VM = 0, D = 0, D2 = 0;
            rc = pcreg_desc_set_size(hS, &Q, &D);
            if (rc == PCREG_OK) rc = pcreg_desc_set_size(hM, &VM, &D2);
            const int S = (int)mxGetM(prhs[5]);
            const int32_t* nd = (const int32_t*)mxGetData(prhs[6]);
            if (rc == PCREG_OK && ((int)mxGetM(prhs[3]) != Q || (int)mxGetM(prhs[4]) != VM || mxGetN(prhs[3]) != 3 || mxGetN(prhs[4]) != 3 || (S > 0 && mxGetN(prhs[5]) != 3) ||
                                   (int)(mxGetM(prhs[6]) * mxGetN(prhs[6])) != S))
                usage = "sphereSweep: featSurface / featModel must have the rows of their descriptor sets, centres S x 3, numDesc S entries";
            else if (rc == PCREG_OK) {
                size_t tot = 0; for (int i = 0; i < S; ++i) tot += (size_t)(nd[i] > 0 ? nd[i] : 0);
                const size_t s1 = (size_t)(S > 0 ? S : 1);
                mxArray* rows = mxCreateNumericMatrix(tot > 0 ? tot : 1, 1, mxINT32_CLASS, mxREAL);
                mxArray* buf = mxCreateNumericMatrix(2, s1 * (Q > 0 ? Q : 1), mxUINT32_CLASS, mxREAL);
                mxArray* np = mxCreateNumericMatrix(s1, 1, mxINT32_CLASS, mxREAL); mxArray* tr = mxCreateNumericMatrix(s1, 1, mxINT32_CLASS, mxREAL);
                mxArray* Tb = mxCreateDoubleMatrix(16, s1, mxREAL);
                mxArray* ns = mxCreateNumericMatrix(s1, 1, mxINT32_CLASS, mxREAL); mxArray* mi = mxCreateNumericMatrix(s1, 1, mxINT32_CLASS, mxREAL);
                mxArray* fl = mxCreateNumericMatrix(s1, 1, mxINT32_CLASS, mxREAL);
                int nt = 0;
                rc = pcreg_sphere_sweep(hS, hM, mxGetPr(prhs[3]), Q > 0 ? Q : 1, mxGetPr(prhs[4]), VM > 0 ? VM : 1, mxGetPr(prhs[5]), S, S > 0 ? S : 1, nd, mxGetScalar(prhs[7]),
                                        &o, (int)mxGetScalar(prhs[9]), &ro, (int32_t*)mxGetData(rows), (uint32_t*)mxGetData(buf), (int32_t*)mxGetData(np), (int32_t*)mxGetData(tr),
                                        &nt, mxGetPr(Tb), (int32_t*)mxGetData(ns), (int32_t*)mxGetData(mi), (int32_t*)mxGetData(fl));
                if (rc == PCREG_OK) {
                    const int32_t* n = (const int32_t*)mxGetData(np);
                    size_t P = 0; for (int z = 0; z < S; ++z) P += (size_t)n[z];
                    plhs[0] = mxCreateDoubleMatrix(tot, tot ? 1 : 0, mxREAL);
                    { const int32_t* r = (const int32_t*)mxGetData(rows); for (size_t k = 0; k < tot; ++k) mxGetPr(plhs[0])[k] = (double)r[k] + 1.0; }
                    auto out = [&](int k, mxArray* a) { if (nlhs > k) plhs[k] = a; else mxDestroyArray(a); };
                    {
                        mxArray* pr = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
                        const uint32_t* src = (const uint32_t*)mxGetData(buf); uint32_t* dst = (uint32_t*)mxGetData(pr);
                        size_t k = 0;
                        for (int z = 0; z < S; ++z)
                            for (int e = 0; e < n[z]; ++e, ++k) { dst[k] = src[((size_t)z * Q + e) * 2]; dst[k + P] = src[((size_t)z * Q + e) * 2 + 1]; }
                        out(1, pr);
                    }
                    auto col = [&](const int32_t* v, int len, double add) { mxArray* a = mxCreateDoubleMatrix(len, len ? 1 : 0, mxREAL); for (int i = 0; i < len; ++i) mxGetPr(a)[i] = (double)v[i] + add; return a; };
                    out(2, col(n, S, 0.0));
                    out(3, col((const int32_t*)mxGetData(tr), nt, 1.0));
                    { mwSize dims[3] = {4, 4, (mwSize)nt}; mxArray* T3 = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL); if (nt) memcpy(mxGetPr(T3), mxGetPr(Tb), (size_t)nt * 128); out(4, T3); }
                    out(5, col((const int32_t*)mxGetData(ns), nt, 0.0));
                    out(6, col((const int32_t*)mxGetData(mi), nt, 0.0));
                    out(7, col((const int32_t*)mxGetData(fl), nt, 0.0));
                }
                mxDestroyArray(rows); mxDestroyArray(buf); mxDestroyArray(np); mxDestroyArray(tr); mxDestroyArray(Tb); mxDestroyArray(ns); mxDestroyArray(mi); mxDestroyArray(fl);
            }
        }
    } else if (!strcmp(cmd, "sphereModelCreate")) {           // [h, modelRows] = pcreg_mex('sphereModelCreate', hModel, featModel, centres, int32(numDesc), R_desc)
        // the model side of sphereSweep in a handle (one model, many surfaces); modelRows: the spheres' row lists back to back (1-based)
        if (nrhs != 6 || !mxIsUint64(prhs[1]) || !mxIsDouble(prhs[2]) || !mxIsDouble(prhs[3]) || !mxIsInt32(prhs[4]) || mxGetN(prhs[2]) != 3)
            usage = "sphereModelCreate: hModel (uint64), featModel (n x 3 double), centres (S x 3 double), int32 numDesc, R_desc";
        else {
            pcreg_desc_set* hM = (pcreg_desc_set*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            int VM = 0, D = 0;
            rc = pcreg_desc_set_size(hM, &VM, &D);
            const int S = (int)mxGetM(prhs[3]);
            const int32_t* nd = (const int32_t*)mxGetData(prhs[4]);
            if (rc == PCREG_OK && ((int)mxGetM(prhs[2]) != VM || (S > 0 && mxGetN(prhs[3]) != 3) || (int)(mxGetM(prhs[4]) * mxGetN(prhs[4])) != S))
                usage = "sphereModelCreate: featModel must have the rows of the model set, centres S x 3, numDesc S entries";
            else if (rc == PCREG_OK) {
                size_t tot = 0; for (int i = 0; i < S; ++i) tot += (size_t)(nd[i] > 0 ? nd[i] : 0);
                mxArray* rows = mxCreateNumericMatrix(tot > 0 ? tot : 1, 1, mxINT32_CLASS, mxREAL);
                pcreg_sphere_model* h = nullptr;
                rc = pcreg_sphere_model_create(hM, mxGetPr(prhs[2]), VM > 0 ? VM : 1, mxGetPr(prhs[3]), S, S > 0 ? S : 1, nd, mxGetScalar(prhs[5]), (int32_t*)mxGetData(rows), &h);
                if (rc == PCREG_OK) {
                    plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL); *(uint64_t*)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)h;
                    if (nlhs > 1) {
                        plhs[1] = mxCreateDoubleMatrix(tot, tot ? 1 : 0, mxREAL);
                        const int32_t* r = (const int32_t*)mxGetData(rows);
                        for (size_t k = 0; k < tot; ++k) mxGetPr(plhs[1])[k] = (double)r[k] + 1.0;
                    }
                }
                mxDestroyArray(rows);
            }
        }
    } else if (!strcmp(cmd, "sphereSweepOnModel")) {
        // [pairs, nPairs, trial, T, numSuccess, maxInliers, failed] = pcreg_mex('sphereSweepOnModel', hSphereModel, hSurface, featSurface, S, par,
        //     putativeThresh, ransacCoef, seed)            (S = the number of spheres of the model handle; outputs as 'sphereSweep' without the rows)
        if (nrhs != 9 || !mxIsUint64(prhs[1]) || !mxIsUint64(prhs[2]) || !mxIsDouble(prhs[3]) || mxGetN(prhs[3]) != 3)
            usage = "sphereSweepOnModel: hSphereModel, hSurface (uint64), featSurface (n x 3 double), S, par, putativeThresh, ransacCoef, seed";
        else {
            const mxArray* p = prhs[5];
            pcreg_match_opts o;
            o.metric = field_is(p, "Metric", "SAD") ? PCREG_METRIC_SAD : PCREG_METRIC_SSD;
            o.matchThreshold = field(p, "MatchThreshold", 1.0); o.maxRatio = field(p, "MaxRatio", 0.6);
            o.unique = (int)field(p, "Unique", 0); o.prenormalized = 0;
            o.unnormalize = (int)field(p, "UNNORMALIZE", 0); o.norm_factor = field(p, "norm_factor", 0.0);
            o.change_metric = (int)field(p, "CHANGE_METRIC", 0); o.metric_factor = field(p, "metric_factor", 1.0);
            const mxArray* c = prhs[7];
            pcreg_ransac_opts ro;
            ro.minPtNum = (int)field(c, "minPtNum", 3); ro.iterNum = (int)field(c, "iterNum", 1000);
            ro.thDist = field(c, "thDist", 0.5); ro.thInlrRatio = field(c, "thInlrRatio", 0.1);
            ro.REFINE = (int)field(c, "REFINE", 1); ro.VERBOSE = 0;
            ro.seed = (uint64_t)mxGetScalar(prhs[8]);
            pcreg_sphere_model* sm = (pcreg_sphere_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]);
            pcreg_desc_set* hS = (pcreg_desc_set*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[2]);
            int Q = 0, D = 0;
            rc = pcreg_desc_set_size(hS, &Q, &D);
            const int S = (int)mxGetScalar(prhs[4]);
            if (rc == PCREG_OK && ((int)mxGetM(prhs[3]) != Q || S < 0)) usage = "sphereSweepOnModel: featSurface must have the rows of the surface set";
            else if (rc == PCREG_OK) {
                const size_t s1 = (size_t)(S > 0 ? S : 1);
                mxArray* buf = mxCreateNumericMatrix(2, s1 * (Q > 0 ? Q : 1), mxUINT32_CLASS, mxREAL);
                mxArray* np = mxCreateNumericMatrix(s1, 1, mxINT32_CLASS, mxREAL); mxArray* tr = mxCreateNumericMatrix(s1, 1, mxINT32_CLASS, mxREAL);
                mxArray* Tb = mxCreateDoubleMatrix(16, s1, mxREAL);
                mxArray* ns = mxCreateNumericMatrix(s1, 1, mxINT32_CLASS, mxREAL); mxArray* mi = mxCreateNumericMatrix(s1, 1, mxINT32_CLASS, mxREAL);
                mxArray* fl = mxCreateNumericMatrix(s1, 1, mxINT32_CLASS, mxREAL);
                int nt = 0;
                rc = pcreg_sphere_sweep_on_model(sm, hS, mxGetPr(prhs[3]), Q > 0 ? Q : 1, &o, (int)mxGetScalar(prhs[6]), &ro, (uint32_t*)mxGetData(buf), (int32_t*)mxGetData(np),
                                                 (int32_t*)mxGetData(tr), &nt, mxGetPr(Tb), (int32_t*)mxGetData(ns), (int32_t*)mxGetData(mi), (int32_t*)mxGetData(fl));
                if (rc == PCREG_OK) {
                    const int32_t* n = (const int32_t*)mxGetData(np);
                    size_t P = 0; for (int z = 0; z < S; ++z) P += (size_t)n[z];
                    plhs[0] = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
                    {
                        const uint32_t* src = (const uint32_t*)mxGetData(buf); uint32_t* dst = (uint32_t*)mxGetData(plhs[0]);
                        size_t k = 0;
                        for (int z = 0; z < S; ++z)
                            for (int e = 0; e < n[z]; ++e, ++k) { dst[k] = src[((size_t)z * Q + e) * 2]; dst[k + P] = src[((size_t)z * Q + e) * 2 + 1]; }
                    }
                    auto out = [&](int k, mxArray* a) { if (nlhs > k) plhs[k] = a; else mxDestroyArray(a); };
                    auto col = [&](const int32_t* v, int len, double add) { mxArray* a = mxCreateDoubleMatrix(len, len ? 1 : 0, mxREAL); for (int i = 0; i < len; ++i) mxGetPr(a)[i] = (double)v[i] + add; return a; };
                    out(1, col(n, S, 0.0));
                    out(2, col((const int32_t*)mxGetData(tr), nt, 1.0));
                    { mwSize dims[3] = {4, 4, (mwSize)nt}; mxArray* T3 = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL); if (nt) memcpy(mxGetPr(T3), mxGetPr(Tb), (size_t)nt * 128); out(3, T3); }
                    out(4, col((const int32_t*)mxGetData(ns), nt, 0.0));
                    out(5, col((const int32_t*)mxGetData(mi), nt, 0.0));
                    out(6, col((const int32_t*)mxGetData(fl), nt, 0.0));
                }
                mxDestroyArray(buf); mxDestroyArray(np); mxDestroyArray(tr); mxDestroyArray(Tb); mxDestroyArray(ns); mxDestroyArray(mi); mxDestroyArray(fl);
            }
        }
    } else if (!strcmp(cmd, "sphereModelDestroy")) {
        if (nrhs != 2 || !mxIsUint64(prhs[1])) usage = "sphereModelDestroy: handle (uint64)";
        else rc = pcreg_sphere_model_destroy((pcreg_sphere_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]));
    } else if (!strcmp(cmd, "descDestroy")) {
        if (nrhs != 2 || !mxIsUint64(prhs[1])) usage = "descDestroy: handle (uint64)";
        else rc = pcreg_desc_set_destroy((pcreg_desc_set*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]));
    } else if (!strcmp(cmd, "modelDestroy")) {
        if (nrhs != 2 || !mxIsUint64(prhs[1])) usage = "modelDestroy: handle (uint64)";
        else rc = pcreg_model_destroy((pcreg_model*)(uintptr_t)*(const uint64_t*)mxGetData(prhs[1]));
    } else if (!strcmp(cmd, "setDevice")) {                   // one GPU per parfor / spmd worker: pcreg_mex('setDevice', labindex - 1)
        if (nrhs != 2) usage = "setDevice: ordinal";
        else rc = pcreg_set_device((int)mxGetScalar(prhs[1]));
    } else if (!strcmp(cmd, "commId")) {                      // id = pcreg_mex('commId') on worker 1; labBroadcast it
        if (nrhs != 1) usage = "commId: no arguments";
        else {
            pcreg_comm_id id;
            rc = pcreg_comm_get_unique_id(&id);
            if (rc == PCREG_OK) { plhs[0] = mxCreateNumericMatrix(1, sizeof id, mxUINT8_CLASS, mxREAL); memcpy(mxGetData(plhs[0]), &id, sizeof id); }
        }
    } else if (!strcmp(cmd, "commInit")) {                    // pcreg_mex('commInit', rank, world, id)
        if (nrhs != 4 || mxGetM(prhs[3]) * mxGetN(prhs[3]) != sizeof(pcreg_comm_id) || !mxIsUint8(prhs[3])) usage = "commInit: rank, world, id (1 x 128 uint8)";
        else { pcreg_comm_id id; memcpy(&id, mxGetData(prhs[3]), sizeof id); rc = pcreg_comm_init((int)mxGetScalar(prhs[1]), (int)mxGetScalar(prhs[2]), &id); }
    } else if (!strcmp(cmd, "commDestroy")) {
        rc = pcreg_comm_destroy();
    } else if (!strcmp(cmd, "matchPointsSharded")) {          // pairs = pcreg_mex('matchPointsSharded', surface, modelRows, m_lo, M_total, thrAbs, maxRatio, unique)
        if (nrhs != 8 || !mxIsSingle(prhs[1]) || !mxIsSingle(prhs[2])) usage = "matchPointsSharded: surface (single Q x 3), model rows (single M_local x 3), m_lo, M_total, thrAbs, maxRatio, unique";
        else {
            int Q = (int)mxGetM(prhs[1]), Ml = (int)mxGetM(prhs[2]);
            mxArray* buf = mxCreateNumericMatrix(2, Q > 0 ? Q : 1, mxUINT32_CLASS, mxREAL);
            int P = 0;
            rc = pcreg_match_points_sharded_f32((const float*)mxGetData(prhs[1]), Q, Q, (const float*)mxGetData(prhs[2]), Ml, Ml > 0 ? Ml : 1,
                                                (int)mxGetScalar(prhs[3]), (int)mxGetScalar(prhs[4]), (float)mxGetScalar(prhs[5]), (float)mxGetScalar(prhs[6]),
                                                (int)mxGetScalar(prhs[7]), (uint32_t*)mxGetData(buf), &P);
            if (rc == PCREG_OK) {
                plhs[0] = mxCreateNumericMatrix(P, 2, mxUINT32_CLASS, mxREAL);
                const uint32_t* src = (const uint32_t*)mxGetData(buf); uint32_t* dst = (uint32_t*)mxGetData(plhs[0]);
                for (int k = 0; k < P; ++k) { dst[k] = src[2 * k]; dst[k + P] = src[2 * k + 1]; }
            }
            mxDestroyArray(buf);
        }
    } else if (!strcmp(cmd, "ransacSharded")) {               // [T, inlierIdx, numSuccess, maxInliers, failed] = pcreg_mex('ransacSharded', pts1, pts2, coef, seed)
        if (nrhs != 5) usage = "ransacSharded: pts1, pts2, coef, seed";
        else {
            const mxArray* c = prhs[3];
            pcreg_ransac_opts o;
            o.minPtNum = (int)field(c, "minPtNum", 3); o.iterNum = (int)field(c, "iterNum", 1000);
            o.thDist = field(c, "thDist", 0.5); o.thInlrRatio = field(c, "thInlrRatio", 0.1);
            o.REFINE = (int)field(c, "REFINE", 1); o.VERBOSE = 0; o.seed = (uint64_t)mxGetScalar(prhs[4]);
            int n = (int)mxGetM(prhs[1]);
            mxArray* inl = mxCreateNumericMatrix(n > 0 ? n : 1, 1, mxINT32_CLASS, mxREAL);
            double T[16]; int ni = 0, ns = 0, mi = 0, fl = 1;
            rc = pcreg_ransac_sharded(mxGetPr(prhs[1]), mxGetPr(prhs[2]), n, n, &o, T, (int32_t*)mxGetData(inl), &ni, &ns, &mi, &fl);
            if (rc == PCREG_OK) {
                plhs[0] = fl ? mxCreateDoubleMatrix(0, 0, mxREAL) : mxCreateDoubleMatrix(4, 4, mxREAL);
                if (!fl) memcpy(mxGetPr(plhs[0]), T, sizeof T);
                if (nlhs > 1) {
                    plhs[1] = mxCreateDoubleMatrix(fl ? 0 : ni, fl ? 0 : 1, mxREAL);
                    const int32_t* src = (const int32_t*)mxGetData(inl);
                    for (int k = 0; k < (fl ? 0 : ni); ++k) mxGetPr(plhs[1])[k] = (double)src[k];
                }
                if (nlhs > 2) plhs[2] = mxCreateDoubleScalar(ns);
                if (nlhs > 3) plhs[3] = mxCreateDoubleScalar(mi);
                if (nlhs > 4) plhs[4] = mxCreateDoubleScalar(fl);
            }
            mxDestroyArray(inl);
        }
    } else {
        usage = "unknown command";
    }
    if (usage) mexErrMsgIdAndTxt("pcreg:usage", "%s", usage);
    if (rc != PCREG_OK) mexErrMsgIdAndTxt("pcreg:hip", "%s", pcreg_last_error());
}
#endif  // __has_include("mex.h")
