function [labels, spheres, counts, rmse, refitUsed, diag] = fitSpheresModel(h, maxDistance, varargin)
% [labels, spheres, counts, rmse, refitUsed, diag] = fitSpheresModel(h, maxDistance, 'MaxNumSpheres', P, 'MaxNumTrials', B, 'MinInliers', n,
% 'MinRadius', r0, 'MaxRadius', r1, 'Seed', s, 'Samples', S)   MSAC sphere fitting and sphere extraction over the rows of a prepared
% model (h = pcreg_mex('modelCreate', single(model))): pcfitsphere(ptCloud, maxDistance) and the loop over it -- fit, take the inliers
% out, fit again -- up to MaxNumSpheres times in ONE call: every marker sphere or ball tip of a scan.
% MaxNumSpheres defaults to 1, MaxNumTrials to 1000 (pcfitsphere's default), MinInliers to 4, MinRadius to 0, MaxRadius to Inf (only
% trial spheres with MinRadius <= R <= MaxRadius count, compared in single), Seed to 0; Samples, int32 4 x (MaxNumTrials *
% MaxNumSpheres) of 1-based rows, replaces the sampler.  labels (M x 1 int32) is p for the rows of sphere p and 0 for the rest;
% spheres (n x 4 double) holds [cx cy cz R] per sphere as sphereModel.Parameters does; counts (n x 1 int32) and rmse (n x 1) describe
% each sphere's inliers; refitUsed (n x 1 int32) is 0 where a round kept its winning trial's own sphere; diag (MaxNumSpheres x 3) is
% every round's winning trial (1-based), its MSAC cost and its inlier count.  The rule is the contract at pcreg_model_fit_spheres_f32
% in include/pcreg.h.
[t, rmin, rmax, P, B, mn, sd, smp] = fitSpheresArgs(maxDistance, varargin{:});
if nargout > 5
    [labels, spheres, counts, rmse, refitUsed, diag] = pcreg_mex('modelFitSpheres', h, t, rmin, rmax, P, B, mn, sd, smp);
elseif nargout > 4
    [labels, spheres, counts, rmse, refitUsed] = pcreg_mex('modelFitSpheres', h, t, rmin, rmax, P, B, mn, sd, smp);
elseif nargout > 3
    [labels, spheres, counts, rmse] = pcreg_mex('modelFitSpheres', h, t, rmin, rmax, P, B, mn, sd, smp);
elseif nargout > 2
    [labels, spheres, counts] = pcreg_mex('modelFitSpheres', h, t, rmin, rmax, P, B, mn, sd, smp);
elseif nargout > 1
    [labels, spheres] = pcreg_mex('modelFitSpheres', h, t, rmin, rmax, P, B, mn, sd, smp);
else
    labels = pcreg_mex('modelFitSpheres', h, t, rmin, rmax, P, B, mn, sd, smp);
end
end

function [t, rmin, rmax, P, B, mn, sd, smp] = fitSpheresArgs(maxDistance, varargin)
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
end
