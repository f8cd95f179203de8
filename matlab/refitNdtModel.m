function [Tout, nPairs, sumE] = refitNdtModel(h, pts, T, neighbors, outlierRatio, steps)
%REFITNDTMODEL  Refine candidate transforms by NDT steps against the table of a handle of ndtModel(model, step).
%   The third refinement beside refitTransformsModel (point to point) and refitPlaneModel (point to plane), and the cheapest: no
%   nearest-row search.  T is 4 x 4 x B, every page used as quickTF uses it ([pts, 1] * T).  Per step and page, every moved row of
%   pts is paired with the Gaussian of the voxel it falls in (neighbors = 1, the default) or also with those of the voxel's six
%   face neighbours (neighbors = 7); the small rigid motion S that minimises the pairs' Mahalanobis distances, each weighted by its
%   current likelihood exp(-d2 / 2 * distance) (one Gauss-Newton step, applied as an exact rotation), makes the page T * S.
%   outlierRatio (default 0.55, in [0, 1)) sets d2 as pcregisterndt's OutlierRatio does; 0 means d2 = 1.  steps (default 1) repeats
%   the step on the device without a round trip.
%   THIS IS A STEP, not pcregisterndt: no convergence test, no line search, no multi-resolution schedule, and not its bits.
%   Tout(:, :, b) is a ZERO PAGE where there is no fit: fewer than six pairs, pairs that leave a direction free, or an all-zero
%   T(:, :, b).  nPairs(b) and sumE(b), the pairs and the sum of their weights, describe the transform that went INTO the last step.
if nargin < 4, neighbors = 1; end
if nargin < 5, outlierRatio = 0.55; end
if nargin < 6, steps = 1; end
[Tout, nPairs, sumE] = pcreg_mex('ndtRefit', h, single(pts), double(T), double(neighbors), double(outlierRatio), double(steps));
end
