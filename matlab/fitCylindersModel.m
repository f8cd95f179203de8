function [labels, cylinders, extents, counts, rmse, refitUsed, diag] = fitCylindersModel(h, maxDistance, varargin)
% [labels, cylinders, extents, counts, rmse, refitUsed, diag] = fitCylindersModel(h, maxDistance, 'Normals', N, 'NumNeighborsNormals', k,
% 'ReferenceVector', v, 'MaxAngularDistance', deg, 'MaxNumCylinders', P, 'MaxNumTrials', B, 'MinInliers', n, 'MinRadius', r0,
% 'MaxRadius', r1, 'Seed', s, 'Samples', S)   MSAC cylinder fitting and cylinder extraction over the rows of a prepared model
% (h = pcreg_mex('modelCreate', single(model))): pcfitcylinder(ptCloud, maxDistance, referenceVector, maxAngularDistance) and the loop
% over it -- fit, take the inliers out, fit again -- up to MaxNumCylinders times in ONE call: every shaft, sleeve, trocar or rod of a
% scan.  Normals (M x 3, as pcnormalsModel returns them; their sign does not matter) default to [], which computes them in the call
% from the NumNeighborsNormals nearest rows (default 12).  ReferenceVector (1 x 3) with MaxAngularDistance in DEGREES (default 5, as
% pcfitcylinder's) bounds the axis.  MaxNumCylinders defaults to 1, MaxNumTrials to 1000, MinInliers to 4, MinRadius to 0, MaxRadius
% to Inf (only trial cylinders with MinRadius <= R <= MaxRadius count, compared in single), Seed to 0; Samples, int32 2 x
% (MaxNumTrials * MaxNumCylinders) of 1-based rows, replaces the sampler.  labels (M x 1 int32) is p for the rows of cylinder p and
% 0 for the rest; cylinders (n x 7 double) holds [cx cy cz wx wy wz R] per cylinder: a point of the axis, its unit direction, the
% radius; extents (n x 2) holds [hLo hHi], so that the axis runs from c + hLo w to c + hHi w; counts (n x 1 int32) and rmse (n x 1)
% describe each cylinder's inliers; refitUsed (n x 1 int32) is 0 where a round kept its winning trial's own cylinder; diag
% (MaxNumCylinders x 3) is every round's winning trial (1-based), its MSAC cost and its inlier count.  The rule is the contract at
% pcreg_model_fit_cylinders_f32 in include/pcreg.h.
[t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp] = fitCylindersArgs(maxDistance, varargin{:});
if nargout > 6
    [labels, cylinders, extents, counts, rmse, refitUsed, diag] = pcreg_mex('modelFitCylinders', h, t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
elseif nargout > 5
    [labels, cylinders, extents, counts, rmse, refitUsed] = pcreg_mex('modelFitCylinders', h, t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
elseif nargout > 4
    [labels, cylinders, extents, counts, rmse] = pcreg_mex('modelFitCylinders', h, t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
elseif nargout > 3
    [labels, cylinders, extents, counts] = pcreg_mex('modelFitCylinders', h, t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
elseif nargout > 2
    [labels, cylinders, extents] = pcreg_mex('modelFitCylinders', h, t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
elseif nargout > 1
    [labels, cylinders] = pcreg_mex('modelFitCylinders', h, t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
else
    labels = pcreg_mex('modelFitCylinders', h, t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp);
end
end

function [t, rmin, rmax, rv, ang, nrm, kn, P, B, mn, sd, smp] = fitCylindersArgs(maxDistance, varargin)
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
end
