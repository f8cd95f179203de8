function [ptsOut, counts, labels] = pcdownsampleFast(pts, gridStep)
%PCDOWNSAMPLEFAST  [ptsOut, counts, labels] = pcdownsampleFast(pts, gridStep): pcdownsample(pc, 'gridAverage', gridStep) for an
%   n x 3 cloud on the GPU.  The grid starts at the minimum of the finite rows; a voxel is a distinct cell
%   floor((x - min) / gridStep), taken in double; ptsOut (single) holds the mean of the rows of every voxel, summed in double in
%   row order, the voxels in ascending order of (cell 1, cell 2, cell 3) -- MATLAB documents no order for pcdownsample's.
%   counts (int32): the rows of every voxel.  labels (int32, n x 1): the row of ptsOut every row of pts went into, 0 for a
%   row with a NaN or Inf; average colours or normals alongside with accumarray(labels(labels > 0), ...) ./ double(counts).
%   The gateway refuses a double cloud: the conversion is made here, once, and the result is single.
if nargout > 2
    [ptsOut, counts, labels] = pcreg_mex('downsampleGrid', single(pts), double(gridStep));
elseif nargout > 1
    [ptsOut, counts] = pcreg_mex('downsampleGrid', single(pts), double(gridStep));
else
    ptsOut = pcreg_mex('downsampleGrid', single(pts), double(gridStep));
end
end
