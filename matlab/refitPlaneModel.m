function [Tout, nClose, sumD2, nPlane, sumRes2] = refitPlaneModel(h, pts, T, maxDist, steps, normals, k)
%REFITPLANEMODEL  Refit candidate transforms by point-to-plane steps against the model of a handle of pcreg_mex('modelCreate', single(model)).
%   refitTransformsModel with the linearised point-to-plane step in estimateTransform's place: T is 4 x 4 x B, every page used as
%   quickTF uses it ([pts, 1] * T).  Per step and page, the rows of pts with a model row within maxDist of their moved place give
%   pairs (model row, moved point); the residual of a pair is the distance of the moved point from the PLANE through the model row
%   with that row's normal; the small rigid motion S that minimises the squared residuals (linearised, then applied as an exact
%   rotation) makes the page T * S.  steps (default 1) repeats that on the device without a round trip.  On a surface this moves
%   a candidate much further per step than refitTransformsModel: a nearest row is nearly the right partner across the surface
%   even where it is the wrong one along it.
%   normals is M x 3 by model row, as pcnormalsModel(h, k) returns it, or [] (the default) to compute the normals once inside the
%   call from the k nearest rows (default 6, pcnormals' default).  THE NORMAL RULE IS THIS LIBRARY'S (pcnormalsModel), not
%   pcnormals'.  A normal is used as it is; its sign is immaterial; a row with a NaN component offers no plane, so set the rows
%   you distrust (a high variation, say) to NaN.
%   Tout(:, :, b) is a ZERO PAGE where there is no fit: fewer than six planes, planes that leave a direction free (a flat model),
%   or an all-zero T(:, :, b).
%   nClose(b), sumD2(b) are scoreTransformsModel's for the transform that went INTO the last step; nPlane(b) counts its pairs
%   with a plane and sumRes2(b) sums their squared plane distances: sqrt(sumRes2 ./ double(nPlane)) is its plane RMSE, not Tout's.
if nargin < 5, steps = 1; end
if nargin < 6, normals = []; end
if nargin < 7, k = 6; end
[Tout, nClose, sumD2, nPlane, sumRes2] = pcreg_mex('modelRefitPlane', h, single(pts), double(T), maxDist, double(steps), single(normals), double(k));
end
