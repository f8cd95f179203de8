function [inlierIndices, meanDist, thr] = pcdenoiseModel(h, k, threshold)
% [inlierIndices, meanDist, thr] = pcdenoiseModel(h, k, threshold)   statistical outlier removal over the rows of a prepared model
% (h = pcreg_mex('modelCreate', single(model))), as pcdenoise(ptCloud, 'NumNeighbors', k, 'Threshold', threshold) does it:
% meanDist (M x 1 double) is the mean distance of every row to its k nearest other rows, 1 <= k <= 31 (default 4), NaN for a row
% with a NaN or Inf; thr = mean(meanDist) + threshold * std(meanDist) over the finite ones (default threshold 1.0); inlierIndices
% (uint32 column, ascending) are the rows with meanDist <= thr.  The neighbour rule and the order of the sums are this library's
% (pcreg_model_denoise_f32 in include/pcreg.h).
if nargin < 2, k = 4; end
if nargin < 3, threshold = 1.0; end
if nargout > 2
    [inlierIndices, meanDist, thr] = pcreg_mex('modelDenoise', h, double(k), double(threshold));
elseif nargout > 1
    [inlierIndices, meanDist] = pcreg_mex('modelDenoise', h, double(k), double(threshold));
else
    inlierIndices = pcreg_mex('modelDenoise', h, double(k), double(threshold));
end
end
