function [normals, variation] = pcnormalsModel(h, k, viewpoint)
% [normals, variation] = pcnormalsModel(h, k, viewpoint)   surface normals of a prepared model (h = pcreg_mex('modelCreate',
% single(model))) from the k nearest rows of every row, 3 <= k <= 32, the row itself among them (default k = 6, as pcnormals).
% normals: M x 3 single, the eigenvector of the smallest eigenvalue of the neighbourhood's scatter, taken in double; viewpoint
% (1 x 3, optional): the normals point towards it; without one the component of largest magnitude is non-negative.  variation:
% M x 1 single, lambda_min / (lambda_1 + lambda_2 + lambda_3), the surface variation by which a normal is judged.  NaN rows
% where there is no normal (a non-finite row, fewer than three finite rows, coincident neighbours).  The neighbour rule and the
% sign are this library's (pcreg_model_normals_f32 in include/pcreg.h), not bit for bit those of MATLAB's own pcnormals.
if nargin < 2, k = 6; end
if nargin < 3, viewpoint = []; end
if nargout > 1
    [normals, variation] = pcreg_mex('modelNormals', h, double(k), double(viewpoint));
else
    normals = pcreg_mex('modelNormals', h, double(k), double(viewpoint));
end
end
