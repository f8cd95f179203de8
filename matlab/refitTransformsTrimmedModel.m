function [Tout, nClose, sumD2, nWithin, d2Cut] = refitTransformsTrimmedModel(h, pts, T, maxDist, varargin)
%REFITTRANSFORMSTRIMMEDMODEL  refitTransformsModel with pcregistericp's 'InlierRatio': every step keeps each candidate's closest pairs.
%   [Tout, nClose, sumD2, nWithin, d2Cut] = refitTransformsTrimmedModel(h, pts, T, maxDist, steps, 'InlierRatio', rho) takes
%   refitTransformsModel's arguments (steps may be left out) and a trailing 'InlierRatio', rho with rho in (0, 1].  Of the rows of
%   pts with a model row within maxDist of their moved place, every step keeps the closest
%   min(n, max(1, floor(rho * n + 0.5))) -- ordered by squared distance (single), ties to the lower row of pts -- and fits those
%   alone.  maxDist = Inf is 'InlierRatio' with no distance at all.  On partly overlapping clouds this is what gets a candidate out
%   of where the radius alone stalls: the wrong partners sit in the far share of the pairs.
%   nClose(b) and sumD2(b) count and sum the KEPT pairs of the transform that went INTO the last step; nWithin(b) (int32) is the
%   number of its pairs before the trim and d2Cut(b) (single) the largest kept squared distance, Inf where nothing is kept.
%   rho = 1 keeps everything: the outputs are refitTransformsModel's, bit for bit.
%   Without 'InlierRatio' this IS refitTransformsModel (the 'modelRefit' command), and nWithin, d2Cut are [].
[rho, args] = pcregTrailingInlierRatio(varargin);
if isempty(rho)
    [Tout, nClose, sumD2] = refitTransformsModel(h, pts, T, maxDist, args{:});
    nWithin = []; d2Cut = [];
    return
end
steps = 1;
if numel(args) >= 1, steps = args{1}; end
[Tout, nClose, sumD2, nWithin, d2Cut] = pcreg_mex('modelRefitTrimmed', h, single(pts), double(T), maxDist, double(rho), double(steps));
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
