function [model, inlierIndices, outlierIndices, rmse] = pcfitsphereFast(pts, maxDistance, varargin)
% [model, inlierIndices, outlierIndices, rmse] = pcfitsphereFast(pts, maxDistance, 'MaxNumTrials', B, 'MinRadius', r0, 'MaxRadius', r1,
% 'Seed', s)   pcfitsphere for an M x 3 cloud: ONE sphere by MSAC in one library call (fitSpheresFast with MaxNumSpheres = 1).
% model is the 1 x 4 double [cx cy cz R] of sphereModel.Parameters ([] when no sphere was found), inlierIndices and outlierIndices
% are uint32 columns taken from the labels (the rows with a NaN or Inf are outliers), rmse the root mean square radial distance of
% the inliers.  The rule is the contract at pcreg_model_fit_spheres_f32 in include/pcreg.h, not pcfitsphere's bits (INTEGRATION.md).
[labels, spheres, ~, rmse] = fitSpheresFast(pts, maxDistance, 'MaxNumSpheres', 1, varargin{:});
model = spheres;
inlierIndices = uint32(find(labels == 1));
outlierIndices = uint32(find(labels ~= 1));
end
