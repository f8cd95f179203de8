function [labels, spheres, counts, rmse, refitUsed, diag] = fitSpheresFast(pts, maxDistance, varargin)
% [labels, spheres, counts, rmse, refitUsed, diag] = fitSpheresFast(pts, maxDistance, 'MaxNumSpheres', P, 'MaxNumTrials', B, 'MinInliers', n,
% 'MinRadius', r0, 'MaxRadius', r1, 'Seed', s, 'Samples', S)   fitSpheresModel for an M x 3 cloud without a handle: the cloud is
% uploaded and prepared for this call only (keep a handle and call fitSpheresModel for repeated calls).  The outputs and the
% name-value pairs are fitSpheresModel's; the rule is the contract at pcreg_model_fit_spheres_f32 in include/pcreg.h.
p = inputParser;
addParameter(p, 'MaxNumSpheres', 1);
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
P = double(p.Results.MaxNumSpheres);
B = double(p.Results.MaxNumTrials);
mn = double(p.Results.MinInliers);
sd = double(p.Results.Seed);
smp = int32(p.Results.Samples);
if nargout > 5
    [labels, spheres, counts, rmse, refitUsed, diag] = pcreg_mex('pointFitSpheres', single(pts), t, rmin, rmax, P, B, mn, sd, smp);
elseif nargout > 4
    [labels, spheres, counts, rmse, refitUsed] = pcreg_mex('pointFitSpheres', single(pts), t, rmin, rmax, P, B, mn, sd, smp);
elseif nargout > 3
    [labels, spheres, counts, rmse] = pcreg_mex('pointFitSpheres', single(pts), t, rmin, rmax, P, B, mn, sd, smp);
elseif nargout > 2
    [labels, spheres, counts] = pcreg_mex('pointFitSpheres', single(pts), t, rmin, rmax, P, B, mn, sd, smp);
elseif nargout > 1
    [labels, spheres] = pcreg_mex('pointFitSpheres', single(pts), t, rmin, rmax, P, B, mn, sd, smp);
else
    labels = pcreg_mex('pointFitSpheres', single(pts), t, rmin, rmax, P, B, mn, sd, smp);
end
end
