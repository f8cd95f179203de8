function [idx, d2, label, minD2] = farthestPointsFast(pts, K, varargin)
% [idx, d2, label, minD2] = farthestPointsFast(pts, K, 'Start', s, 'StopDistance', r)   farthest point sampling of an M x 3 cloud
% without a handle: the cloud is uploaded and prepared for this call only (keep a handle and call farthestPointsModel for repeated
% calls).  pts(idx, :) are at most K well-spread rows of pts; the options and the outputs are farthestPointsModel's: idx (n x 1
% uint32, selection order), d2 (n x 1 single, squared), label (M x 1 uint32, the position in idx of every row's nearest sample),
% minD2 (M x 1 single, squared).  'StopDistance' r is a distance, squared in single inside.
s = 0; r = 0;
if mod(numel(varargin), 2) ~= 0, error('pcreg:usage', 'farthestPointsFast: name-value arguments come in pairs'); end
for a = 1:2:numel(varargin)
    switch lower(char(varargin{a}))
        case 'start',        s = varargin{a + 1};
        case 'stopdistance', r = varargin{a + 1};
        otherwise, error('pcreg:usage', 'farthestPointsFast: unknown option %s', char(varargin{a}));
    end
end
r2 = single(r) * single(r);
if nargout > 3
    [idx, d2, label, minD2] = pcreg_mex('pointFps', single(pts), double(K), double(s), r2);
elseif nargout > 2
    [idx, d2, label] = pcreg_mex('pointFps', single(pts), double(K), double(s), r2);
elseif nargout > 1
    [idx, d2] = pcreg_mex('pointFps', single(pts), double(K), double(s), r2);
else
    idx = pcreg_mex('pointFps', single(pts), double(K), double(s), r2);
end
end
