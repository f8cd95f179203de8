function clusters = clusterPointsModel(h, r)
%CLUSTERPOINTSMODEL  clusters = clusterPoints(model, r) over the rows of a model handle of pcreg_mex('modelCreate', single(model)).
%   The connected components of the graph in which two rows are adjacent when their distance is <= r, found on the GPU in
%   one call.  clusters is a 1 x C cell of double row vectors: the 1-based rows of every cluster, ascending; the clusters
%   are ordered by their smallest row.  A row with a NaN or Inf coordinate is a cluster of its own.  The distances are formed
%   in single: a pair whose distance is within rounding of r may fall on the other side of the bound than in MATLAB's double
%   arithmetic.
[~, clOff, members] = pcreg_mex('modelCluster', h, r);
clusters = mat2cell(double(members(:)).', 1, diff(double(clOff(:))).');
end
