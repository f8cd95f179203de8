function [features, spfh, nNeighbors] = extractFPFHRadiusModel(h, radius, maxNeighbors, normals, kNormals, viewpoint)
% [features, spfh, nNeighbors] = extractFPFHRadiusModel(h, radius, maxNeighbors, normals, kNormals, viewpoint)   FPFH descriptors of
% a prepared model (h = pcreg_mex('modelCreate', single(model))) from radius neighbourhoods: extractFPFHFeatures(ptCloud, 'Radius',
% radius) in this library's rule.  features: M x 33 double, three histograms of eleven bins a row, each adding up to 100 (or all
% zero where a row has no neighbour that counts); NaN for a row with a NaN or Inf.  radius: a number >= 0 (Inf allowed); the
% neighbourhood of a row is every OTHER row within it (inclusive, single-precision distances; coincident rows are no neighbours).
% maxNeighbors (default 0): n > 0 counts only the n nearest rows within the radius, 0 counts all of them.  THIS IS HOW MATLAB'S
% DEFAULT OF 50 NEIGHBOURS IS REACHED, which extractFPFHModel's list of 32 cannot serve: maxNeighbors = 50 with a radius
% wide enough to hold 50 rows; a row with fewer rows inside the radius uses what is there.  normals: M x 3 single by model row, as
% pcnormalsModel returns them -- THEIR SIGN MATTERS, so orient them with a viewpoint -- or [] (the default) to compute them in the
% call from the kNormals nearest rows (3 .. 32, default 6) and the viewpoint (1 x 3, or [] for the sign rule of pcnormalsModel).
% spfh: M x 33 uint32, the integer counts of the pair features of every row; nNeighbors: M x 1 int32, the neighbours counted.
% The weight of a neighbour is the inverse of the SQUARED distance.  At most 4 Mi rows a call; the device holds 8 bytes per (row,
% neighbour) pair within the radius while the call runs.  The rule is stated once, at pcreg_model_fpfh_radius_f32 in
% include/pcreg.h; it is not bit for bit that of MATLAB's own extractFPFHFeatures.
if nargin < 3 || isempty(maxNeighbors), maxNeighbors = 0; end
if nargin < 4, normals = []; end
if nargin < 5 || isempty(kNormals), kNormals = 6; end
if nargin < 6, viewpoint = []; end
r2 = single(double(radius)^2);                        % squared in double, rounded once
if nargout > 2
    [features, spfh, nNeighbors] = pcreg_mex('modelFpfhRadius', h, r2, double(maxNeighbors), single(normals), double(kNormals), double(viewpoint));
elseif nargout > 1
    [features, spfh] = pcreg_mex('modelFpfhRadius', h, r2, double(maxNeighbors), single(normals), double(kNormals), double(viewpoint));
else
    features = pcreg_mex('modelFpfhRadius', h, r2, double(maxNeighbors), single(normals), double(kNormals), double(viewpoint));
end
end
