function [idx, corepts] = dbscanFast(X, epsilon, minpts)
%DBSCANFAST  [idx, corepts] = dbscanFast(X, epsilon, minpts): dbscan(X, epsilon, minpts) on the GPU, without the Statistics Toolbox.
%   X is N x 3, single or double (a double cloud is converted to single, as clusterPointsFast does).  idx is N x 1 double: the
%   1-based cluster of every row, -1 for noise; corepts is N x 1 logical: the core rows -- what MATLAB's dbscan returns, with
%   the clusters numbered in ascending order of their smallest core row and a border row in the smallest-numbered cluster
%   among its core neighbours (see dbscanModel).  To run several (epsilon, minpts) on the same cloud, keep a handle:
%   h = pcreg_mex('modelCreate', single(X)); dbscanModel(h, epsilon, minpts).
[label, core, ~, ~] = pcreg_mex('dbscanPoints', single(X), epsilon, minpts);
idx = double(label(:));
corepts = logical(core(:));
end
