function [idx, corepts] = dbscanModel(h, epsilon, minpts)
%DBSCANMODEL  [idx, corepts] = dbscan(model, epsilon, minpts) over the rows of a model handle of pcreg_mex('modelCreate', single(model)).
%   DBSCAN on the GPU in one call, without the Statistics Toolbox.  A row is a core row when at least minpts rows, itself
%   included, lie within epsilon of it (inclusive); the clusters are the connected components of the core rows, numbered in
%   ascending order of their smallest core row; a row that is not core but within epsilon of a core row is a border row and
%   joins the smallest-numbered cluster among those core rows, as dbscan's sequential loop does.  idx is M x 1 double: the
%   1-based cluster of every row, -1 for noise.  corepts is M x 1 logical.  A row with a NaN or Inf coordinate is noise.  The
%   distances are formed in single: a pair whose distance is within rounding of epsilon may fall on the other side of the bound
%   than in MATLAB's double arithmetic.
[label, core, ~, ~] = pcreg_mex('modelDbscan', h, epsilon, minpts);
idx = double(label(:));
corepts = logical(core(:));
end
