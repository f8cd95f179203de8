function [T, info] = pcregisterfgrFast(moving, fixed, gridStep, varargin)
%PCREGISTERFGRFAST  [T, info] = pcregisterfgrFast(moving, fixed, gridStep, 'MaxDistance', d, 'NumNeighbors', k, 'Options', opts, 'Match', par)
%   The composition a pcregisterfgr(moving, fixed, gridStep) user expects, over this library's own wrappers: pcdownsampleFast of
%   both clouds at gridStep, pcnormalsFast and extractFPFHFast (k neighbours, default 16) on both, getMatches of the moving
%   descriptors against the fixed ones (every nearest descriptor, kept when the choice is mutual: Unique), then fgrBatched on the
%   matched points with delta2 = d^2 (default d = gridStep):  [moving, ones] * T = [fixed, ones].  T is [] where the registration
%   failed.  'Options' adds fields to fgrBatched's opts (iterations, n_tuples, ...), 'Match' to getMatches' par.
%   info: matches (P x 2, rows of the two downsampled clouds), movingDown, fixedDown, inlierIdx (rows of matches) and fgrBatched's
%   stats.  The rule is this library's contract (include/pcreg.h: pcreg_fgr_batched), not MathWorks' implementation: pcregisterfgr
%   draws its tuples from MATLAB's random stream, this one is deterministic.
d = gridStep; k = 16; opts = struct(); par = struct();
if mod(numel(varargin), 2) ~= 0, error('pcreg:usage', 'pcregisterfgrFast: name-value arguments come in pairs'); end
for a = 1:2:numel(varargin)
    switch lower(char(varargin{a}))
        case 'maxdistance', d = varargin{a + 1};
        case 'numneighbors', k = varargin{a + 1};
        case 'options', opts = varargin{a + 1};
        case 'match', par = varargin{a + 1};
        otherwise, error('pcreg:usage', 'pcregisterfgrFast: unknown name %s', char(varargin{a}));
    end
end
match = struct('UNNORMALIZE', false, 'CHANGE_METRIC', false, 'Method', 'Exhaustive', 'MatchThreshold', 100, 'MaxRatio', 1, ...
               'Metric', 'SSD', 'Unique', true, 'VERBOSE', 0);
names = fieldnames(par);
for a = 1:numel(names), match.(names{a}) = par.(names{a}); end
opts.delta2 = double(d) * double(d);
movingDown = pcdownsampleFast(moving, gridStep);
fixedDown = pcdownsampleFast(fixed, gridStep);
descMoving = extractFPFHFast(movingDown, 'NumNeighbors', k, 'Normals', pcnormalsFast(movingDown, k));
descFixed = extractFPFHFast(fixedDown, 'NumNeighbors', k, 'Normals', pcnormalsFast(fixedDown, k));
matches = getMatches(descMoving, descFixed, match);
[TCells, inlierCells, stats] = fgrBatched({double(fixedDown(matches(:, 2), :))}, {double(movingDown(matches(:, 1), :))}, opts);
T = TCells{1};
info = struct('matches', matches, 'movingDown', movingDown, 'fixedDown', fixedDown, 'inlierIdx', inlierCells{1}, 'stats', stats);
end
