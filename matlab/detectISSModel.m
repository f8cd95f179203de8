function [keypointIndices, saliency, eigenvalues, numNeighbors] = detectISSModel(h, varargin)
% [keypointIndices, saliency, eigenvalues, numNeighbors] = detectISSModel(h, 'SalientRadius', rs, 'NonMaxRadius', rn, 'Threshold21',
% g21, 'Threshold32', g32, 'MinNeighbors', n)   ISS keypoints (Intrinsic Shape Signatures) over the rows of a prepared model
% (h = pcreg_mex('modelCreate', single(model))), with detectISSFeatures' name-value pairs.  SalientRadius and NonMaxRadius are
% required (no default is guessed from the cloud's resolution); Threshold21 and Threshold32 default to 0.975, MinNeighbors to 5.
% keypointIndices (uint32 column, ascending) are the rows whose saliency no row within NonMaxRadius beats; saliency (M x 1 double)
% is the smallest eigenvalue of the covariance of the rows within SalientRadius for a row that passes both ratio tests and has
% MinNeighbors such rows (itself included), else 0; eigenvalues (M x 3 double) are that covariance's, descending; numNeighbors
% (M x 1 int32).  The radii are squared in double and the square is rounded once to single, as pcreg_model_iss_f32 in
% include/pcreg.h states; the neighbour rule, the exact sums and the tie rule are that contract's.
[r2s, r2n, g21, g32, mn] = issArgs(varargin{:});
if nargout > 3
    [keypointIndices, saliency, eigenvalues, numNeighbors] = pcreg_mex('modelIss', h, r2s, r2n, g21, g32, mn);
elseif nargout > 2
    [keypointIndices, saliency, eigenvalues] = pcreg_mex('modelIss', h, r2s, r2n, g21, g32, mn);
elseif nargout > 1
    [keypointIndices, saliency] = pcreg_mex('modelIss', h, r2s, r2n, g21, g32, mn);
else
    keypointIndices = pcreg_mex('modelIss', h, r2s, r2n, g21, g32, mn);
end
end

function [r2s, r2n, g21, g32, mn] = issArgs(varargin)
p = inputParser;
addParameter(p, 'SalientRadius', []);
addParameter(p, 'NonMaxRadius', []);
addParameter(p, 'Threshold21', 0.975);
addParameter(p, 'Threshold32', 0.975);
addParameter(p, 'MinNeighbors', 5);
parse(p, varargin{:});
if isempty(p.Results.SalientRadius) || isempty(p.Results.NonMaxRadius)
    error('pcreg:usage', 'detectISSModel: SalientRadius and NonMaxRadius are required');
end
r2s = single(double(p.Results.SalientRadius) ^ 2);
r2n = single(double(p.Results.NonMaxRadius) ^ 2);
g21 = double(p.Results.Threshold21);
g32 = double(p.Results.Threshold32);
mn = double(p.Results.MinNeighbors);
end
