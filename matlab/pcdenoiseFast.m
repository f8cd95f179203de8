function [ptsOut, inlierIndices, outlierIndices, meanDist] = pcdenoiseFast(pts, k, threshold)
% [ptsOut, inlierIndices, outlierIndices, meanDist] = pcdenoiseFast(pts, k, threshold)   pcdenoise(ptCloud, 'NumNeighbors', k,
% 'Threshold', threshold) for an M x 3 cloud without a handle: the cloud is uploaded and prepared for this call only (keep a handle
% and call pcdenoiseModel for repeated calls).  ptsOut = pts(inlierIndices, :) keeps the class of pts; inlierIndices and
% outlierIndices are uint32 columns, ascending, each the complement of the other; meanDist (M x 1 double) is pcdenoiseModel's.
if nargin < 2, k = 4; end
if nargin < 3, threshold = 1.0; end
if nargout > 3
    [inlierIndices, meanDist] = pcreg_mex('pointDenoise', single(pts), double(k), double(threshold));
else
    inlierIndices = pcreg_mex('pointDenoise', single(pts), double(k), double(threshold));
end
ptsOut = pts(inlierIndices, :);
keep = false(size(pts, 1), 1);
keep(inlierIndices) = true;
outlierIndices = uint32(find(~keep));
end
