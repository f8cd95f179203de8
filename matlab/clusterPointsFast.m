function clusters = clusterPointsFast(pts, r)
%CLUSTERPOINTSFAST  clusters = clusterPointsFast(pts, r): clusterPoints(pts, r) on the GPU, without the Statistics Toolbox.
%   pts is N x 3.  clusters is a 1 x C cell of double row vectors: the 1-based rows of every connected component of the
%   graph "distance <= r", ascending; the clusters are ordered by their smallest row, as the frontier loop of
%   clusterPoints finds them.  The distances are formed in single (see clusterPointsModel).  To cluster the same cloud
%   with several radii, keep a handle: h = pcreg_mex('modelCreate', single(pts)); clusterPointsModel(h, r).
[~, clOff, members] = pcreg_mex('clusterPoints', single(pts), r);
clusters = mat2cell(double(members(:)).', 1, diff(double(clOff(:))).');
end
