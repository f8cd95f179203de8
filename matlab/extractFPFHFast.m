function [features, spfh] = extractFPFHFast(pts, varargin)
% features = extractFPFHFast(pts, 'NumNeighbors', k, 'Normals', normals, 'NumNeighborsNormals', kNormals, 'Viewpoint', viewpoint)
% extractFPFHFeatures(ptCloud, 'NumNeighbors', k) for an M x 3 cloud without a handle: the cloud is uploaded and prepared for this
% call only (keep a handle and call extractFPFHModel for repeated calls).  Every name-value pair is optional: NumNeighbors 3 .. 32
% (default 32; MATLAB's own default of 50 is above this library's list), Normals M x 3 by row (default []: computed in the call from
% the NumNeighborsNormals nearest rows, default NumNeighbors, oriented towards Viewpoint, 1 x 3 or []).  The sign of a normal
% matters.  features (M x 33 double) and spfh (M x 33 uint8) are extractFPFHModel's.
k = 32; normals = []; kNormals = []; viewpoint = [];
if mod(numel(varargin), 2) ~= 0, error('pcreg:usage', 'extractFPFHFast: name-value arguments come in pairs'); end
for a = 1:2:numel(varargin)
    switch lower(char(varargin{a}))
        case 'numneighbors', k = varargin{a + 1};
        case 'normals', normals = varargin{a + 1};
        case 'numneighborsnormals', kNormals = varargin{a + 1};
        case 'viewpoint', viewpoint = varargin{a + 1};
        otherwise, error('pcreg:usage', 'extractFPFHFast: unknown name %s', char(varargin{a}));
    end
end
if isempty(kNormals), kNormals = k; end
if nargout > 1
    [features, spfh] = pcreg_mex('pointFpfh', single(pts), double(k), single(normals), double(kNormals), double(viewpoint));
else
    features = pcreg_mex('pointFpfh', single(pts), double(k), single(normals), double(kNormals), double(viewpoint));
end
end
