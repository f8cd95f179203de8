function [fitness, rmse, nClose, idx, D2, nWithin, d2Cut] = scoreTransformsTrimmedModel(h, pts, T, maxDist, varargin)
%SCORETRANSFORMSTRIMMEDMODEL  scoreTransformsModel with pcregistericp's 'InlierRatio': each candidate is scored on its closest pairs.
%   [fitness, rmse, nClose, idx, D2, nWithin, d2Cut] = scoreTransformsTrimmedModel(h, pts, T, maxDist, invert, 'InlierRatio', rho)
%   takes scoreTransformsModel's arguments (invert may be left out) and a trailing 'InlierRatio', rho with rho in (0, 1].  Of the
%   rows of pts with a model row within maxDist of their transformed place, the closest min(n, max(1, floor(rho * n + 0.5))) are
%   kept -- ordered by squared distance (single), ties to the lower row of pts.  nClose, fitness and rmse are about the kept pairs;
%   idx / D2 hold 0 / Inf at trimmed rows, as at rows without a pair; nWithin(b) (int32) is the number of pairs before the trim and
%   d2Cut(b) (single) the largest kept squared distance, Inf where nothing is kept.  rho = 1 keeps everything.
%   Without 'InlierRatio' this IS scoreTransformsModel (the 'modelScore' command), and nWithin, d2Cut are [].
[rho, args] = pcregTrailingInlierRatio(varargin);
if isempty(rho)
    nWithin = []; d2Cut = [];
    if nargout > 3
        [fitness, rmse, nClose, idx, D2] = scoreTransformsModel(h, pts, T, maxDist, args{:});
    else
        [fitness, rmse, nClose] = scoreTransformsModel(h, pts, T, maxDist, args{:});
        idx = []; D2 = [];
    end
    return
end
invert = false;
if numel(args) >= 1, invert = args{1}; end
if iscell(T)
    A = zeros(4, 4, numel(T));
    for b = 1:numel(T)
        if ~isempty(T{b}), A(:, :, b) = T{b}; end
    end
else
    A = double(T);
end
if invert
    for b = 1:size(A, 3)
        if any(any(A(:, :, b))), A(:, :, b) = invertTF(A(:, :, b)); end
    end
end
[nClose, sumD2, idx, D2, nWithin, d2Cut] = pcreg_mex('modelScoreTrimmed', h, single(pts), A, maxDist, double(rho));
fitness = double(nClose) / size(pts, 1);
rmse = sqrt(sumD2 ./ double(nClose));
end

function [rho, args] = pcregTrailingInlierRatio(args)
% strips a trailing 'InlierRatio', rho from a cell of arguments; rho = [] without one
rho = [];
n = numel(args);
if n >= 2 && (ischar(args{n - 1}) || isstring(args{n - 1})) && strcmpi(args{n - 1}, 'InlierRatio')
    rho = args{n};
    args = args(1:n - 2);
end
end
