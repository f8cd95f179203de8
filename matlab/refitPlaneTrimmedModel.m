function [Tout, nClose, sumD2, nPlane, sumRes2, nWithin, d2Cut] = refitPlaneTrimmedModel(h, pts, T, maxDist, varargin)
%REFITPLANETRIMMEDMODEL  refitPlaneModel with pcregistericp's 'InlierRatio': every step keeps each candidate's closest pairs.
%   [Tout, nClose, sumD2, nPlane, sumRes2, nWithin, d2Cut] = refitPlaneTrimmedModel(h, pts, T, maxDist, steps, normals, k,
%   'InlierRatio', rho) takes refitPlaneModel's arguments (the optional ones may be left out) and a trailing 'InlierRatio', rho
%   with rho in (0, 1].  The pairs are trimmed as refitTransformsTrimmedModel trims them -- by the squared distance (single) between
%   the moved point and its nearest model row, not by the plane residual -- and the plane pairs, nPlane and sumRes2 are taken among
%   the kept pairs.  nWithin(b) (int32) is the number of pairs before the trim, d2Cut(b) (single) the largest kept squared distance.
%   Without 'InlierRatio' this IS refitPlaneModel (the 'modelRefitPlane' command), and nWithin, d2Cut are [].
[rho, args] = pcregTrailingInlierRatio(varargin);
if isempty(rho)
    [Tout, nClose, sumD2, nPlane, sumRes2] = refitPlaneModel(h, pts, T, maxDist, args{:});
    nWithin = []; d2Cut = [];
    return
end
opt = {1, [], 6};                                  % steps, normals, k
opt(1:numel(args)) = args;
[Tout, nClose, sumD2, nPlane, sumRes2, nWithin, d2Cut] = pcreg_mex('modelRefitPlaneTrimmed', h, single(pts), double(T), maxDist, double(rho), double(opt{1}), single(opt{2}), double(opt{3}));
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
