function [Tout, nClose, sumD2, nPairs, sumRes2] = refitGicpModel(h, pts, T, maxDist, steps, normals, ptsNormals, k, epsilon)
%REFITGICPMODEL  Refit candidate transforms by plane-to-plane (generalized ICP) steps against the model of a handle of pcreg_mex('modelCreate', single(model)).
%   refitPlaneModel with the plane-to-plane step in the point-to-plane step's place -- what pcregistericp calls Metric =
%   'planeToPlane': T is 4 x 4 x B, every page used as quickTF uses it ([pts, 1] * T).  Per step and page, the rows of pts with a
%   model row within maxDist of their moved place give pairs (model row, moved point).  Each side of a pair has the covariance
%   I - (1 - epsilon) * n * n' about its own normal (the query's normal turned by the page's rotation), and the pair is weighted by
%   the inverse of the two covariances' sum: fully across either surface, about half as much along them.  The small rigid motion S
%   that minimises the weighted squared distances (linearised, then applied as an exact rotation) makes the page T * S.  steps
%   (default 1) repeats that on the device without a round trip.  Unlike refitPlaneModel this holds a FLAT model too, because
%   every pair also pulls along the surface.  A step, not an ICP policy: no convergence test, no robust kernel.
%   normals is M x 3 by model row and ptsNormals Q x 3 by row of pts, as pcnormalsModel returns them for either cloud; either may
%   be [] (the default) to compute it once inside the call from the k nearest rows of its own cloud (default 6, pcnormals'
%   default).  THE NORMAL RULE IS THIS LIBRARY'S (pcnormalsModel), not pcnormals'.  Normals are used as they are; their signs are
%   immaterial; a pair with a NaN component on either side is dropped.  epsilon (default 1e-3) lies in (0, 1].
%   Tout(:, :, b) is a ZERO PAGE where there is no fit: fewer than six pairs, pairs that leave a direction free, or an all-zero
%   T(:, :, b).
%   nClose(b), sumD2(b) are scoreTransformsModel's for the transform that went INTO the last step; nPairs(b) counts its
%   plane-to-plane pairs and sumRes2(b) sums their weighted squared distances e' * W * e.
if nargin < 5, steps = 1; end
if nargin < 6, normals = []; end
if nargin < 7, ptsNormals = []; end
if nargin < 8, k = 6; end
if nargin < 9, epsilon = 1e-3; end
[Tout, nClose, sumD2, nPairs, sumRes2] = pcreg_mex('modelRefitGicp', h, single(pts), double(T), maxDist, double(steps), single(normals), single(ptsNormals), double(k), double(epsilon));
end
