function [Tout, nClose, sumD2] = refitTransformsModel(h, pts, T, maxDist, steps)
%REFITTRANSFORMSMODEL  Refit candidate transforms on their close dense pairs against the model of a handle of pcreg_mex('modelCreate', single(model)).
%   The T_refine of completeExperimentFast.m:383-394 with the whole cloud in the place of a cluster's re-matched keypoints, for
%   every candidate at once: T is 4 x 4 x B, every page used as quickTF uses it ([pts, 1] * T).  Per step and page, the rows of
%   pts with a model row within maxDist of their moved place give pairs (model row, moved point), S = estimateTransform(model
%   rows, moved points) maps the moved points onto the model, and the page becomes T * S; steps (default 1) repeats that on the
%   device without a round trip.
%   Tout(:, :, b) is a ZERO PAGE where there is no fit: fewer than three pairs, an empty estimateTransform, or an all-zero
%   T(:, :, b) -- the empty transform of a failed ransac stays empty.
%   nClose(b) and sumD2(b) are scoreTransformsModel's counts and sums for the transform that went INTO the last step (T itself
%   when steps = 1): sqrt(sumD2 ./ double(nClose)) is its inlier RMSE, not Tout's.
%   The distances are formed in single and compared with <= , as scoreTransformsModel forms them.
if nargin < 5, steps = 1; end
[Tout, nClose, sumD2] = pcreg_mex('modelRefit', h, single(pts), double(T), maxDist, double(steps));
end
