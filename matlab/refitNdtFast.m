function [Tout, nPairs, sumE] = refitNdtFast(model, step, pts, T, neighbors, outlierRatio, steps, minPoints)
% [Tout, nPairs, sumE] = refitNdtFast(model, step, pts, T, neighbors, outlierRatio, steps, minPoints)   refitNdtModel's result for an
% M x 3 model cloud without a handle: the table is built for this call only (keep a handle of ndtModel and call refitNdtModel for
% repeated calls).
if nargin < 5, neighbors = 1; end
if nargin < 6, outlierRatio = 0.55; end
if nargin < 7, steps = 1; end
if nargin < 8, minPoints = 6; end
h = pcreg_mex('ndtCreate', single(model), double(step), double(minPoints));
release = onCleanup(@() pcreg_mex('ndtDestroy', h));
[Tout, nPairs, sumE] = pcreg_mex('ndtRefit', h, single(pts), double(T), double(neighbors), double(outlierRatio), double(steps));
end
