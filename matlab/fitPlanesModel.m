function [labels, planes, centres, counts, rmse, diag] = fitPlanesModel(h, maxDistance, varargin)
% [labels, planes, centres, counts, rmse, diag] = fitPlanesModel(h, maxDistance, 'MaxNumPlanes', P, 'MaxNumTrials', B, 'MinInliers', n,
% 'ReferenceVector', v, 'MaxAngularDistance', deg, 'Seed', s, 'Samples', S)   MSAC plane fitting and plane extraction over the rows of
% a prepared model (h = pcreg_mex('modelCreate', single(model))): pcfitplane(ptCloud, maxDistance[, referenceVector,
% maxAngularDistance]) and the loop that follows it -- fit, take the inliers out, fit again -- up to MaxNumPlanes times in ONE call.
% MaxNumPlanes defaults to 1, MaxNumTrials to 1000 (pcfitplane's default), MinInliers to 3, MaxAngularDistance to 5 DEGREES (as
% pcfitplane; used only with a ReferenceVector), Seed to 0; Samples, int32 3 x (MaxNumTrials * MaxNumPlanes) of 1-based rows,
% replaces the sampler.  labels (M x 1 int32) is p for the rows of plane p and 0 for the rest; planes (n x 4 double) holds
% [nx ny nz d] per plane as planeModel.Parameters does; centres (n x 3), counts (n x 1 int32) and rmse (n x 1) describe each plane's
% inliers; diag (MaxNumPlanes x 3) is every round's winning trial (1-based), its MSAC cost and its inlier count.  The rule is the
% contract at pcreg_model_fit_planes_f32 in include/pcreg.h.
[t, ref, ang, P, B, mn, sd, smp] = planesArgs(maxDistance, varargin{:});
if nargout > 5
    [labels, planes, centres, counts, rmse, diag] = pcreg_mex('modelPlanes', h, t, ref, ang, P, B, mn, sd, smp);
elseif nargout > 4
    [labels, planes, centres, counts, rmse] = pcreg_mex('modelPlanes', h, t, ref, ang, P, B, mn, sd, smp);
elseif nargout > 3
    [labels, planes, centres, counts] = pcreg_mex('modelPlanes', h, t, ref, ang, P, B, mn, sd, smp);
elseif nargout > 2
    [labels, planes, centres] = pcreg_mex('modelPlanes', h, t, ref, ang, P, B, mn, sd, smp);
elseif nargout > 1
    [labels, planes] = pcreg_mex('modelPlanes', h, t, ref, ang, P, B, mn, sd, smp);
else
    labels = pcreg_mex('modelPlanes', h, t, ref, ang, P, B, mn, sd, smp);
end
end

function [t, ref, ang, P, B, mn, sd, smp] = planesArgs(maxDistance, varargin)
p = inputParser;
addParameter(p, 'MaxNumPlanes', 1);
addParameter(p, 'MaxNumTrials', 1000);
addParameter(p, 'MinInliers', 3);
addParameter(p, 'ReferenceVector', []);
addParameter(p, 'MaxAngularDistance', 5);
addParameter(p, 'Seed', 0);
addParameter(p, 'Samples', []);
parse(p, varargin{:});
t = single(maxDistance);
ref = double(p.Results.ReferenceVector(:)');
ang = double(p.Results.MaxAngularDistance) * pi / 180;
P = double(p.Results.MaxNumPlanes);
B = double(p.Results.MaxNumTrials);
mn = double(p.Results.MinInliers);
sd = double(p.Results.Seed);
smp = int32(p.Results.Samples);
end
