function [Idx, D] = knnsearchModel(h, Y, K)
%KNNSEARCHMODEL  [Idx, D] = knnsearch(model, Y, 'K', K) against a model handle of pcreg_mex('modelCreate', single(model)).
%   Exact fp32 search on the GPU (1 <= K <= 32): Idx the 1-based model rows of the K nearest points of every row of Y
%   (Q x min(K, M) double, ties to the lowest row), D their Euclidean distances (square roots of the single squared
%   distances, as double).
[idx, D2] = pcreg_mex('modelKnn', h, single(Y), K);
keep = 1:size(idx, 2);
if ~isempty(idx)
    keep = find(idx(1, :) > 0);                 % columns past M are 0 in every row
end
Idx = double(idx(:, keep));
D = sqrt(double(D2(:, keep)));
end
