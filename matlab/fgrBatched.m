function [TCells, inlierCells, stats, keptCells] = fgrBatched(pts1Cells, pts2Cells, opts, tupleCells, T0Cells)
%FGRBATCHED  Fast global registration of the matched pairs (pts1Cells{i}, pts2Cells{i}) for every i in ONE library call.
%   The estimator of pcregisterfgr (Zhou, Park, Koltun 2016) in ransac's place: [pts2Cells{i}, ones] * TCells{i} = [pts1Cells{i}, ones].
%   No samples and no hypotheses: a Geman-McClure weight per pair is annealed down to opts.delta2 and a six-unknown rigid step is
%   solved at every stage, so the result depends on nothing but the inputs (pcreg_fgr_batched's contract in include/pcreg.h).
%       [TCells, inlierCells, stats] = fgrBatched(pts1Cells, pts2Cells, struct('delta2', thDist));
%   opts: delta2 (required; compared with SQUARED distances, as ransacCoef.thDist is) and any of iterations (128), decrease_every
%   (4), division_factor (1.4), mu0 (0: the squared extent of the kept pairs), n_tuples (0: no tuple test), tuple_scale (0.95),
%   seed (0: registration i draws its triples with seed + i - 1).
%   tupleCells (optional): tupleCells{i} an n_tuples x 3 table of 1-based pair indices, the triples of the tuple test of registration
%   i in place of the built-in ones.  T0Cells (optional): T0Cells{i} a 4 x 4 start, [] for the identity.
%   TCells{i} is [] where the registration failed (fewer than 3 kept pairs, collinear pairs), as ransacBatched returns it;
%   inlierCells{i} the kept pairs within sqrt(delta2) of the final transform, ascending; keptCells{i} a logical column, the pairs the
%   tuple test kept; stats a struct of column vectors: failed, n_live, n_kept, n_inliers, mu0, mu_final, cost, sum_d2.
    B = numel(pts1Cells);
    lens = cellfun(@(p) size(p, 1), pts1Cells(:));
    pts1 = double(vertcat(pts1Cells{:})); pts2 = double(vertcat(pts2Cells{:}));
    if isempty(pts1), pts1 = zeros(0, 3); pts2 = zeros(0, 3); end
    offsets = int32([0; cumsum(lens)]);
    tupleIdx = [];
    if nargin > 3 && ~isempty(tupleCells)
        tupleIdx = zeros(3, opts.n_tuples * B, 'int32');             % one COLUMN per triple, registration after registration
        for b = 1:B
            tupleIdx(:, (b - 1) * opts.n_tuples + (1:opts.n_tuples)) = int32(tupleCells{b}');
        end
    end
    T0 = [];
    if nargin > 4 && ~isempty(T0Cells)
        T0 = repmat(eye(4), 1, 1, B);
        for b = 1:B
            if ~isempty(T0Cells{b}), T0(:, :, b) = double(T0Cells{b}); end
        end
    end
    [T, inlierIdx, s, kept] = pcreg_mex('fgrBatched', pts1, pts2, offsets, opts, tupleIdx, T0);
    TCells = cell(size(pts1Cells)); inlierCells = cell(size(pts1Cells)); keptCells = cell(size(pts1Cells));
    k = 0;
    for b = 1:B
        if s(b, 1)
            TCells{b} = []; inlierCells{b} = [];
        else
            TCells{b} = T(:, :, b);
            inlierCells{b} = inlierIdx(k + 1:k + s(b, 4));
        end
        k = k + s(b, 4);
        keptCells{b} = logical(kept(double(offsets(b)) + 1:double(offsets(b + 1))));
    end
    stats = struct('failed', s(:, 1), 'n_live', s(:, 2), 'n_kept', s(:, 3), 'n_inliers', s(:, 4), 'mu0', s(:, 5), 'mu_final', s(:, 6), ...
                   'cost', s(:, 7), 'sum_d2', s(:, 8));
end
