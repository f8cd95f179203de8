function [model, inlierIndices, outlierIndices, rmse] = pcfitcylinderFast(pts, maxDistance, varargin)
% [model, inlierIndices, outlierIndices, rmse] = pcfitcylinderFast(pts, maxDistance, referenceVector, maxAngularDistance, 'Normals', N,
% 'NumNeighborsNormals', k, 'MaxNumTrials', B, 'MinRadius', r0, 'MaxRadius', r1, 'Seed', s)   pcfitcylinder for an M x 3 cloud: ONE
% cylinder by MSAC in one library call (fitCylindersFast with MaxNumCylinders = 1).  referenceVector (1 x 3) and maxAngularDistance
% (degrees, default 5) are optional and positional, as pcfitcylinder's; pcfitcylinder requires ptCloud.Normal, here 'Normals' may be
% left out and is then computed in the call.  model is the 1 x 7 double [x1 y1 z1 x2 y2 z2 r] that cylinderModel takes: the two end
% points of the axis, c + hLo w and c + hHi w over the inliers, and the radius ([] when no cylinder was found); inlierIndices and
% outlierIndices are uint32 columns taken from the labels (the rows with a NaN or Inf are outliers), rmse the root mean square
% radial distance of the inliers.  The rule is the contract at pcreg_model_fit_cylinders_f32 in include/pcreg.h, not
% pcfitcylinder's bits (INTEGRATION.md).
args = varargin;
if ~isempty(args) && isnumeric(args{1})
    ref = {'ReferenceVector', args{1}};
    args(1) = [];
    if ~isempty(args) && isnumeric(args{1})
        ref = [ref, {'MaxAngularDistance', args{1}}];
        args(1) = [];
    end
    args = [ref, args];
end
[labels, cylinders, extents, ~, rmse] = fitCylindersFast(pts, maxDistance, 'MaxNumCylinders', 1, args{:});
if isempty(cylinders)
    model = [];
else
    c = cylinders(1, 1:3);
    w = cylinders(1, 4:6);
    model = [c + extents(1, 1) * w, c + extents(1, 2) * w, cylinders(1, 7)];
end
inlierIndices = uint32(find(labels == 1));
outlierIndices = uint32(find(labels ~= 1));
end
