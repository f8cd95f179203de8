function [model, inlierIndices, outlierIndices, rmse] = pcfitplaneFast(pts, maxDistance, referenceVector, maxAngularDistance, varargin)
% [model, inlierIndices, outlierIndices, rmse] = pcfitplaneFast(pts, maxDistance[, referenceVector[, maxAngularDistance]], 'MaxNumTrials',
% B, 'Seed', s)   pcfitplane for an M x 3 cloud: ONE plane by MSAC in one library call (fitPlanesFast with MaxNumPlanes = 1).
% model is the 1 x 4 double [nx ny nz d] of planeModel.Parameters ([] when no plane was found), inlierIndices and outlierIndices are
% uint32 columns taken from the labels (the rows with a NaN or Inf are outliers), rmse the root mean square distance of the
% inliers.  maxAngularDistance is in DEGREES and defaults to 5, as pcfitplane's.  The rule is the contract at
% pcreg_model_fit_planes_f32 in include/pcreg.h, not pcfitplane's bits (INTEGRATION.md).
if nargin < 3
    referenceVector = [];
end
if nargin < 4 || isempty(maxAngularDistance)
    maxAngularDistance = 5;
end
[labels, planes, ~, ~, rmse] = fitPlanesFast(pts, maxDistance, 'MaxNumPlanes', 1, 'ReferenceVector', referenceVector, ...
    'MaxAngularDistance', maxAngularDistance, varargin{:});
model = planes;
inlierIndices = uint32(find(labels == 1));
outlierIndices = uint32(find(labels ~= 1));
end
