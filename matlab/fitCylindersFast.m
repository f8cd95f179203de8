function [labels, cylinders, extents, counts, rmse, refitUsed, diag] = fitCylindersFast(pts, maxDistance, varargin)
% [labels, cylinders, extents, counts, rmse, refitUsed, diag] = fitCylindersFast(pts, maxDistance, 'Normals', N, 'NumNeighborsNormals', k,
% 'ReferenceVector', v, 'MaxAngularDistance', deg, 'MaxNumCylinders', P, 'MaxNumTrials', B, 'MinInliers', n, 'MinRadius', r0,
% 'MaxRadius', r1, 'Seed', s, 'Samples', S)   fitCylindersModel for an M x 3 cloud without a handle: the cloud is uploaded and prepared
% for this call only (keep a handle and call fitCylindersModel for repeated calls).  The outputs and the name-value pairs are
% fitCylindersModel's; the rule is the contract at pcreg_model_fit_cylinders_f32 in include/pcreg.h.
p = inputParser;
addParameter(p, 'Normals', []);
addParameter(p, 'NumNeighborsNormals', 12);
addParameter(p, 'ReferenceVector', []);
addParameter(p, 'MaxAngularDistance', 5);
addParameter(p, 'MaxNumCylinders', 1);
addParameter(p, 'MaxNumTrials', 1000);
addParameter(p, 'MinInliers', 4);
addParameter(p, 'MinRadius', 0);
addParameter(p, 'MaxRadius', Inf);
addParameter(p, 'Seed', 0);
addParameter(p, 'Samples', []);
parse(p, varargin{:});
t = single(maxDistance);
rmin = single(p.Results.MinRadius);
rmax = single(p.Results.MaxRadius);
rv = double(p.Results.ReferenceVector(:)');
ang = double(p.Results.MaxAngularDistance) * pi / 180;
nrm = single(p.Results.Normals);
kn = double(p.Results.NumNeighborsNormals);
P = double(p.Results.MaxNumCylinders);
B = double(p.Results.MaxNumTrials);
mn = double(p.Results.MinInliers);
sd = double(p.Results.Seed);
smp = int32(p.Results.Samples);
if nargout > 6
    [labels, cylinders, extents, counts, rmse, refitUsed, diag] = pcreg_mex('pointFitCylinders', single(pts), t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
elseif nargout > 5
    [labels, cylinders, extents, counts, rmse, refitUsed] = pcreg_mex('pointFitCylinders', single(pts), t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
elseif nargout > 4
    [labels, cylinders, extents, counts, rmse] = pcreg_mex('pointFitCylinders', single(pts), t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
elseif nargout > 3
    [labels, cylinders, extents, counts] = pcreg_mex('pointFitCylinders', single(pts), t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
elseif nargout > 2
    [labels, cylinders, extents] = pcreg_mex('pointFitCylinders', single(pts), t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
elseif nargout > 1
    [labels, cylinders] = pcreg_mex('pointFitCylinders', single(pts), t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
else
    labels = pcreg_mex('pointFitCylinders', single(pts), t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
end
end
