function [normals, variation] = pcnormalsFast(pts, k, viewpoint)
% [normals, variation] = pcnormalsFast(pts, k, viewpoint)   pcnormalsModel's result for an M x 3 cloud without a handle: the cloud
% is uploaded and prepared for this call only (keep a handle and call pcnormalsModel for repeated calls).
if nargin < 2, k = 6; end
if nargin < 3, viewpoint = []; end
if nargout > 1
    [normals, variation] = pcreg_mex('pointNormals', single(pts), double(k), double(viewpoint));
else
    normals = pcreg_mex('pointNormals', single(pts), double(k), double(viewpoint));
end
end
