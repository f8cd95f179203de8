"""pcreg_amd -- MI355X (gfx950) implementation of PCReg's correspondence-search +
RANSAC rigid-alignment hot path, behind the reference's own function names.

The arithmetic lives in libpcreg_hip.so (hand-written HIP kernels, C ABI in
include/pcreg.h).  This package is the thin host-side mirror of the MATLAB interface;
it has no CPU fallback and raises if the library or a gfx950 device is missing.
"""
from .api import (EMPTY, GETINLIERS_COEFF, Model, NdtModel, AlignPoints_KNN, AlignPoints_KNN_batched, calcDists,  # noqa: F401
                  estimateTransform, getInliersRANSAC, getLocalPoints, getMatches, getMatchesOnSet, getMatchesSegmentedOnSet, sphereCounts, sphereSweep, SphereModel, sphereSweepOnModel, finalStageLimits, finalStage, DescSet, getMatchesSegmented, getSpacialHistogramDescriptors, speedyDescriptors, invertTF, knn2_points, knn_points, rangesearch_points, cluster_points, dbscan_points, point_normals, point_denoise, point_farthest_points, point_fpfh, point_fpfh_radius, point_iss, point_fit_planes, point_fit_spheres, point_fit_cylinders, unique_rows, aggregate_matches, pcdownsample, matchFeatures,
                  match_points, quickTF, ransac, ransac_batched, fgr, fgr_batched, register_fgr)

__all__ = ["EMPTY", "GETINLIERS_COEFF", "Model", "NdtModel", "AlignPoints_KNN", "AlignPoints_KNN_batched", "calcDists",
           "estimateTransform", "getInliersRANSAC", "getLocalPoints", "getMatches", "getMatchesOnSet", "getMatchesSegmentedOnSet", "sphereCounts", "sphereSweep", "SphereModel", "sphereSweepOnModel", "finalStageLimits", "finalStage", "DescSet", "getMatchesSegmented", "getSpacialHistogramDescriptors", "speedyDescriptors", "invertTF", "knn2_points", "knn_points", "rangesearch_points", "cluster_points", "dbscan_points", "point_normals", "point_denoise", "point_farthest_points", "point_fpfh", "point_fpfh_radius", "point_iss", "point_fit_planes", "point_fit_spheres", "point_fit_cylinders", "unique_rows", "aggregate_matches", "pcdownsample", "matchFeatures",
           "match_points", "quickTF", "ransac", "ransac_batched", "fgr", "fgr_batched", "register_fgr"]
