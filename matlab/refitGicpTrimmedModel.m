function [Tout, nClose, sumD2, nPairs, sumRes2, nWithin, d2Cut] = refitGicpTrimmedModel(h, pts, T, maxDist, varargin)
%REFITGICPTRIMMEDMODEL  refitGicpModel with pcregistericp's 'InlierRatio': every step keeps each candidate's closest pairs.
%   [Tout, nClose, sumD2, nPairs, sumRes2, nWithin, d2Cut] = refitGicpTrimmedModel(h, pts, T, maxDist, steps, normals, ptsNormals,
%   k, epsilon, 'InlierRatio', rho) takes refitGicpModel's arguments (the optional ones may be left out) and a trailing
%   'InlierRatio', rho with rho in (0, 1].  The pairs are trimmed as refitTransformsTrimmedModel trims them -- by the squared
%   distance (single) between the moved point and its nearest model row -- and the plane-to-plane pairs, nPairs and sumRes2 are
%   taken among the kept pairs.  nWithin(b) (int32) is the number of pairs before the trim, d2Cut(b) (single) the largest kept
%   squared distance.
%   Without 'InlierRatio' this IS refitGicpModel (the 'modelRefitGicp' command), and nWithin, d2Cut are [].
[rho, args] = pcregTrailingInlierRatio(varargin);
if isempty(rho)
    [Tout, nClose, sumD2, nPairs, sumRes2] = refitGicpModel(h, pts, T, maxDist, args{:});
    nWithin = []; d2Cut = [];
    return
end
opt = {1, [], [], 6, 1e-3};                        % steps, normals, ptsNormals, k, epsilon
opt(1:numel(args)) = args;
[Tout, nClose, sumD2, nPairs, sumRes2, nWithin, d2Cut] = pcreg_mex('modelRefitGicpTrimmed', h, single(pts), double(T), maxDist, double(rho), double(opt{1}), single(opt{2}), single(opt{3}), double(opt{4}), double(opt{5}));
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
