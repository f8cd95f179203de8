function [labels, planes, centres, counts, rmse, diag] = fitPlanesFast(pts, maxDistance, varargin)
% [labels, planes, centres, counts, rmse, diag] = fitPlanesFast(pts, maxDistance, 'MaxNumPlanes', P, 'MaxNumTrials', B, 'MinInliers', n,
% 'ReferenceVector', v, 'MaxAngularDistance', deg, 'Seed', s, 'Samples', S)   fitPlanesModel for an M x 3 cloud without a handle: the
% cloud is uploaded and prepared for this call only (keep a handle and call fitPlanesModel for repeated calls).  The outputs and the
% name-value pairs are fitPlanesModel's; the rule is the contract at pcreg_model_fit_planes_f32 in include/pcreg.h.
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
if nargout > 5
    [labels, planes, centres, counts, rmse, diag] = pcreg_mex('pointPlanes', single(pts), t, ref, ang, P, B, mn, sd, smp);
elseif nargout > 4
    [labels, planes, centres, counts, rmse] = pcreg_mex('pointPlanes', single(pts), t, ref, ang, P, B, mn, sd, smp);
elseif nargout > 3
    [labels, planes, centres, counts] = pcreg_mex('pointPlanes', single(pts), t, ref, ang, P, B, mn, sd, smp);
elseif nargout > 2
    [labels, planes, centres] = pcreg_mex('pointPlanes', single(pts), t, ref, ang, P, B, mn, sd, smp);
elseif nargout > 1
    [labels, planes] = pcreg_mex('pointPlanes', single(pts), t, ref, ang, P, B, mn, sd, smp);
else
    labels = pcreg_mex('pointPlanes', single(pts), t, ref, ang, P, B, mn, sd, smp);
end
end
