function [Tout, sigma2Out, Np, sumRes2, sumD2, nLive] = refitCpdModel(h, pts, T, sigma2, outlier, steps)
%REFITCPDMODEL  Refit candidate transforms by rigid coherent-point-drift steps against the model of a handle of pcreg_mex('modelCreate', single(model)).
%   What pcregistercpd(..., 'Transform', 'Rigid') iterates, as a STEP: T is 4 x 4 x B, every page used as quickTF uses it
%   ([pts, 1] * T).  Per step and page every moved row of pts is paired SOFTLY with EVERY model row: a Gaussian of their distance
%   with variance sigma2 against a uniform outlier term of weight outlier.  The rigid motion S that best carries the moved points
%   onto their weighted model points (with the determinant correction: never a reflection) makes the page T * S, and the variance
%   is re-estimated by coherent point drift's closed form.  steps (default 1) repeats that on the device without a round trip,
%   each step starting from the variance the one before it left.  No radius, no normals, no voxel size; the capture range is
%   wide, and with a small variance a step is the point-to-point step of refitTransformsModel.  The moved points are the data
%   and the model rows the centroids (the reverse of Myronenko's roles; the same objective for a rigid motion without scale), which
%   suits a surface that is a crop of its model.  A step, not pcregistercpd: no convergence test, no scale, no affine or
%   non-rigid variant.
%   THE COST is B * Q * M pairs a step: downsample both clouds first (pcdownsampleFast), 10^3 to 10^4 points a side.
%   sigma2 (default 0) is a scalar or one value per page; 0 asks for the initial variance, the mean squared distance over all
%   pairs divided by 3; a negative or NaN value makes the page empty.  outlier (default 0.1) lies in [0, 1).
%   Tout(:, :, b) is a ZERO PAGE and sigma2Out(b) is 0 where there is no fit: an all-zero or non-finite T(:, :, b), fewer than three
%   finite rows on either side, no weight left (every point an outlier), model points that do not determine a rotation.
%   sigma2Out is the variance AFTER the last step: pass it on to continue.  Np (the sum of the posterior weights), sumRes2 (the
%   weighted squared residual; sqrt(sumRes2 ./ Np) is the weighted RMSE), sumD2 (the sum of squared nearest-row distances, as
%   scoreTransformsModel gives with maxDist = inf) and nLive (the rows of pts whose moved place is finite) describe the transform
%   that went INTO the last step.
if nargin < 4, sigma2 = 0; end
if nargin < 5, outlier = 0.1; end
if nargin < 6, steps = 1; end
[Tout, sigma2Out, Np, sumRes2, sumD2, nLive] = pcreg_mex('modelRefitCpd', h, single(pts), double(T), double(sigma2), double(outlier), double(steps));
end
