function [h, nVoxels, nGaussians] = ndtModel(pts, step, minPoints)
%NDTMODEL  Summarise a cloud once as one Gaussian per voxel: the table that NDT steps refine candidate transforms against.
%   h = ndtModel(pts, step) puts the n x 3 cloud on a grid of voxel size step (pcdownsample's 'gridAverage' grid: cells
%   floor((x - min) / step), rows with a NaN or Inf ignored) and keeps, for every voxel with at least minPoints rows (default 6, at
%   least 3), the mean and the inverse covariance of its rows.  An eigenvalue of the covariance below 1 % of the largest one is
%   raised to it, so a flat voxel still has an inverse; a voxel whose rows are all equal holds no Gaussian.  nVoxels counts the
%   occupied voxels, nGaussians those that hold a Gaussian.  A cloud that spans 2^21 or more cells along an axis is refused.
%   Release the handle with pcreg_mex('ndtDestroy', h).  See refitNdtModel.
if nargin < 3, minPoints = 6; end
[h, nVoxels, nGaussians] = pcreg_mex('ndtCreate', single(pts), double(step), double(minPoints));
end
