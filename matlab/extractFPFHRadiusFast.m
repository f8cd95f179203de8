function [features, spfh, nNeighbors] = extractFPFHRadiusFast(pts, varargin)
% features = extractFPFHRadiusFast(pts, 'Radius', radius, 'NumNeighbors', n, 'Normals', normals, 'NumNeighborsNormals', kNormals,
%                                  'Viewpoint', viewpoint)
% extractFPFHFeatures(ptCloud, 'Radius', radius) for an M x 3 cloud without a handle: the cloud is uploaded and prepared for this
% call only (keep a handle and call extractFPFHRadiusModel for repeated calls).  Radius is required.  The other name-value pairs are
% optional: NumNeighbors n (default 0: every row within the radius counts; n > 0: the n nearest of them -- MATLAB's default of 50
% neighbours is 'NumNeighbors', 50 with a radius wide enough to hold 50 rows, and a row with fewer rows inside the radius uses what
% is there), Normals M x 3 by row (default []: computed in the call from the NumNeighborsNormals nearest rows, 3 .. 32, default 6,
% oriented towards Viewpoint, 1 x 3 or []).  The sign of a normal matters.  features (M x 33 double), spfh (M x 33 uint32) and
% nNeighbors (M x 1 int32) are extractFPFHRadiusModel's.
radius = []; maxNeighbors = 0; normals = []; kNormals = 6; viewpoint = [];
if mod(numel(varargin), 2) ~= 0, error('pcreg:usage', 'extractFPFHRadiusFast: name-value arguments come in pairs'); end
for a = 1:2:numel(varargin)
    switch lower(char(varargin{a}))
        case 'radius', radius = varargin{a + 1};
        case 'numneighbors', maxNeighbors = varargin{a + 1};
        case 'normals', normals = varargin{a + 1};
        case 'numneighborsnormals', kNormals = varargin{a + 1};
        case 'viewpoint', viewpoint = varargin{a + 1};
        otherwise, error('pcreg:usage', 'extractFPFHRadiusFast: unknown name %s', char(varargin{a}));
    end
end
if isempty(radius), error('pcreg:usage', 'extractFPFHRadiusFast: ''Radius'' is required'); end
r2 = single(double(radius)^2);                        % squared in double, rounded once
if nargout > 2
    [features, spfh, nNeighbors] = pcreg_mex('pointFpfhRadius', single(pts), r2, double(maxNeighbors), single(normals), double(kNormals), double(viewpoint));
elseif nargout > 1
    [features, spfh] = pcreg_mex('pointFpfhRadius', single(pts), r2, double(maxNeighbors), single(normals), double(kNormals), double(viewpoint));
else
    features = pcreg_mex('pointFpfhRadius', single(pts), r2, double(maxNeighbors), single(normals), double(kNormals), double(viewpoint));
end
end
