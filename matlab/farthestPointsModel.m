function [idx, d2, label, minD2, coverD2] = farthestPointsModel(h, K, varargin)
% [idx, d2, label, minD2, coverD2] = farthestPointsModel(h, K, 'Start', s, 'StopDistance', r)   farthest point sampling over the rows
% of a prepared model (h = pcreg_mex('modelCreate', single(model))): at most K rows, each the row farthest from all rows chosen
% before it, so the first K rows of idx are K well-spread rows of the model whatever its density.  Rows with a NaN or Inf are never
% chosen and never measured.
%   'Start'         s  the first sample, a 1-based row (it must be finite); 0 (the default) takes the lowest finite row
%   'StopDistance'  r  a distance >= 0 (default 0): the sampling also stops once every finite row lies within r of a sample, so
%                      farthestPointsModel(h, size(model, 1), 'StopDistance', r) is "sample until the cloud is covered at r".
%                      r is squared in single inside, and the comparison is made on squared single distances.
% idx (n x 1 uint32) the chosen rows in selection order, n <= K; d2 (n x 1 single) the SQUARED distance of each sample to the
% samples before it (d2(1) = Inf, non-increasing after); label (M x 1 uint32) per row the position in idx of its nearest sample, ties
% to the earliest (0 for a row with a NaN or Inf); minD2 (M x 1 single) the squared distance to that sample (NaN there); coverD2
% (single) = max(minD2): every finite row lies within sqrt(coverD2) of a sample.  The rule is this library's
% (pcreg_model_fps_f32 in include/pcreg.h): single arithmetic, ties to the lowest row.
[s, r] = parseArgs(varargin{:});
r2 = single(r) * single(r);
if nargout > 4
    [idx, d2, label, minD2, coverD2] = pcreg_mex('modelFps', h, double(K), double(s), r2);
elseif nargout > 3
    [idx, d2, label, minD2] = pcreg_mex('modelFps', h, double(K), double(s), r2);
elseif nargout > 2
    [idx, d2, label] = pcreg_mex('modelFps', h, double(K), double(s), r2);
elseif nargout > 1
    [idx, d2] = pcreg_mex('modelFps', h, double(K), double(s), r2);
else
    idx = pcreg_mex('modelFps', h, double(K), double(s), r2);
end
end

function [s, r] = parseArgs(varargin)
s = 0; r = 0;
if mod(numel(varargin), 2) ~= 0, error('pcreg:usage', 'farthestPointsModel: name-value arguments come in pairs'); end
for a = 1:2:numel(varargin)
    switch lower(char(varargin{a}))
        case 'start',        s = varargin{a + 1};
        case 'stopdistance', r = varargin{a + 1};
        otherwise, error('pcreg:usage', 'farthestPointsModel: unknown option %s', char(varargin{a}));
    end
end
end
