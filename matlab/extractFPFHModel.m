function [features, spfh] = extractFPFHModel(h, k, normals, kNormals, viewpoint)
% [features, spfh] = extractFPFHModel(h, k, normals, kNormals, viewpoint)   FPFH descriptors of a prepared model (h =
% pcreg_mex('modelCreate', single(model))): extractFPFHFeatures(ptCloud, 'NumNeighbors', k) in this library's rule.  features:
% M x 33 double, three histograms of eleven bins a row, each adding up to 100 (or all zero where a row has no neighbour that
% counts); NaN for a row with a NaN or Inf.  k: 3 <= k <= 32, the row itself among its k nearest rows (default 32; MATLAB's own
% default of 50 is above this library's list).  normals: M x 3 single by model row, as pcnormalsModel returns them -- THEIR SIGN
% MATTERS, so orient them with a viewpoint -- or [] (the default) to compute them in the call from the kNormals nearest rows
% (default k) and the viewpoint (1 x 3, or [] for the sign rule of pcnormalsModel).  spfh: M x 33 uint8, the integer counts of
% the pair features of every row.  The weight of a neighbour is the inverse of the SQUARED distance.  The rule is stated once, at
% pcreg_model_fpfh_f32 in include/pcreg.h; it is not bit for bit that of MATLAB's own extractFPFHFeatures.
if nargin < 2, k = 32; end
if nargin < 3, normals = []; end
if nargin < 4 || isempty(kNormals), kNormals = k; end
if nargin < 5, viewpoint = []; end
if nargout > 1
    [features, spfh] = pcreg_mex('modelFpfh', h, double(k), single(normals), double(kNormals), double(viewpoint));
else
    features = pcreg_mex('modelFpfh', h, double(k), single(normals), double(kNormals), double(viewpoint));
end
end
