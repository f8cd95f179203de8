function [keypoints, keypointIndices, saliency, eigenvalues, numNeighbors] = detectISSFast(pts, varargin)
% [keypoints, keypointIndices, saliency, eigenvalues, numNeighbors] = detectISSFast(pts, 'SalientRadius', rs, 'NonMaxRadius', rn,
% 'Threshold21', g21, 'Threshold32', g32, 'MinNeighbors', n)   detectISSFeatures for an M x 3 cloud without a handle: the cloud is
% uploaded and prepared for this call only (keep a handle and call detectISSModel for repeated calls).
% keypoints = pts(keypointIndices, :) keeps the class of pts; the other outputs and the name-value pairs are detectISSModel's.  The
% radii are squared in double and the square is rounded once to single (pcreg_model_iss_f32 in include/pcreg.h).
p = inputParser;
addParameter(p, 'SalientRadius', []);
addParameter(p, 'NonMaxRadius', []);
addParameter(p, 'Threshold21', 0.975);
addParameter(p, 'Threshold32', 0.975);
addParameter(p, 'MinNeighbors', 5);
parse(p, varargin{:});
if isempty(p.Results.SalientRadius) || isempty(p.Results.NonMaxRadius)
    error('pcreg:usage', 'detectISSFast: SalientRadius and NonMaxRadius are required');
end
r2s = single(double(p.Results.SalientRadius) ^ 2);
r2n = single(double(p.Results.NonMaxRadius) ^ 2);
g21 = double(p.Results.Threshold21);
g32 = double(p.Results.Threshold32);
mn = double(p.Results.MinNeighbors);
if nargout > 4
    [keypointIndices, saliency, eigenvalues, numNeighbors] = pcreg_mex('pointIss', single(pts), r2s, r2n, g21, g32, mn);
elseif nargout > 3
    [keypointIndices, saliency, eigenvalues] = pcreg_mex('pointIss', single(pts), r2s, r2n, g21, g32, mn);
elseif nargout > 2
    [keypointIndices, saliency] = pcreg_mex('pointIss', single(pts), r2s, r2n, g21, g32, mn);
else
    keypointIndices = pcreg_mex('pointIss', single(pts), r2s, r2n, g21, g32, mn);
end
keypoints = pts(keypointIndices, :);
end
