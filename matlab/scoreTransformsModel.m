function [fitness, rmse, nClose, idx, D2] = scoreTransformsModel(h, pts, T, maxDist, invert)
%SCORETRANSFORMSMODEL  How well do candidate transforms put a cloud on the model of a handle of pcreg_mex('modelCreate', single(model))?
%   T: a 4 x 4 x B array or a cell of 4 x 4 matrices, used as quickTF uses them ([pts, 1] * T); an empty cell entry (or an all-zero
%   matrix) is the empty transform of a failed ransac and scores nothing.  invert = true applies invertTF to every transform
%   first: ransac's transforms map the model onto the surface.
%   nClose(b): the rows of pts with a model row within maxDist of their transformed place; fitness = nClose / size(pts, 1);
%   rmse(b) = sqrt(sum of their squared distances / nClose(b)), NaN where nothing is close.  idx (Q x B, 1-based, 0 for none) and
%   D2 (Q x B single, squared, Inf for none) are the nearest such row and its distance, built only when asked for.
%   The distances are formed in single and compared with <= : a row whose distance is within rounding of maxDist may fall on the
%   other side of the bound than vecnorm(...) < maxDist in double.
if nargin < 5, invert = false; end
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
if nargout > 3
    [nClose, sumD2, idx, D2] = pcreg_mex('modelScore', h, single(pts), A, maxDist);
else
    [nClose, sumD2] = pcreg_mex('modelScore', h, single(pts), A, maxDist);
end
fitness = double(nClose) / size(pts, 1);
rmse = sqrt(sumD2 ./ double(nClose));
end
