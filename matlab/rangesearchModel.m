function [Idx, D] = rangesearchModel(h, Y, r)
%RANGESEARCHMODEL  [Idx, D] = rangesearch(model, Y, r) against a model handle of pcreg_mex('modelCreate', single(model)).
%   Exact fp32 search on the GPU: Idx{i} the 1-based model rows within distance r of row i of Y (a double row vector, ascending
%   distance, ties to the lowest row; 1 x 0 when there is none), D{i} their Euclidean distances (square roots of the single
%   squared distances, as double).  The distances are formed in single: a row whose distance is within rounding of r may
%   fall on the other side of the bound than in MATLAB's double arithmetic.
[counts, idx, D2] = pcreg_mex('modelRange', h, single(Y), r);
counts = double(counts(:)).';
Idx = mat2cell(double(idx(:)).', 1, counts).';
D = mat2cell(sqrt(double(D2(:))).', 1, counts).';
end
