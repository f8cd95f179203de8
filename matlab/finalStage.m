function out = finalStage(hModelNoLRF, featModel_noLRF, ptsSurface, locs, transforms, d, margin, descOpt, par, R_desc, maxDist)
%FINALSTAGE  The post-RANSAC stage of completeExperimentFast.m:280-394 (after clusterPoints) as two library calls.
%   locs (K x 3) and transforms (4 x 4 x K) are locCur / transCur of every cluster, chosen by the caller as at :283-288.
%   hModelNoLRF: pcreg_mex('descCreate', descModel_noLRF); featModel_noLRF: its keypoints.  Replaces, per cluster,
%       :291      pts_Surface_tform = quickTF(ptsSurface, invertTF(transCur))
%       :297      sample_ptsSurface = pcRandomUniformSamples(pointCloud(pts_Surface_tform), d, margin)
%       :300-353  descriptors with ALIGN_POINTS = false, the model's no-LRF descriptors inside the cluster's sphere, getMatches
%       :357-378  the share of matches closer than maxDist
%   and then :381-394 (the best cluster, T_refine, pts_Surface_final).
%   The keypoints are drawn HERE, cluster after cluster as the reference loop draws them, with MATLAB's rand on the box of the
%   surface as the library moves it (pcreg_mex('finalStageLimits', ...)): the count and the box come from the bits the
%   descriptors will see.
%   out.precisions (K x 1, NaN where a cluster has no match), out.bestCluster (1-based), out.T_refine ([] when fewer than three
%   close matches), out.ptsSurfaceFinal (N x 3), out.matches{i} (P_i x 2 uint32), out.numKeypoints / numDesc / numMatches / numClose.
    if nargin < 11, maxDist = 1.5; end
    K = size(locs, 1);
    T = zeros(4, 4, K);
    for i = 1:K
        T(:, :, i) = moveTF(transforms(:, :, i));
    end
    lim = pcreg_mex('finalStageLimits', double(ptsSurface), T);
    kp = cell(K, 1);
    for i = 1:K
        kp{i} = drawInBox(lim(i, :), d, margin);
    end
    kpOff = int32([0; cumsum(cellfun(@(c) size(c, 1), kp(:)))]);
    [numKeypoints, numDesc, numMatches, numClose, precisions, best, T_refine, ptsFinal, pairs] = pcreg_mex('finalStage', hModelNoLRF, ...
        double(featModel_noLRF), double(ptsSurface), double(locs), T, vertcat(kp{:}, zeros(0, 3)), kpOff, descOpt, par, R_desc, maxDist);
    out.precisions = precisions; out.bestCluster = best; out.T_refine = T_refine; out.ptsSurfaceFinal = ptsFinal;
    out.matches = mat2cell(pairs, numMatches, 2);
    out.numKeypoints = numKeypoints; out.numDesc = numDesc; out.numMatches = numMatches; out.numClose = numClose;
end

function Ti = moveTF(TF)
% invertTF of completeExperimentFast.m: the inverse of a rigid transform in the row-vector convention
    Ti = eye(4);
    Ti(1:3, 1:3) = TF(1:3, 1:3)';
    Ti(4, 1:3) = -TF(4, 1:3) * TF(1:3, 1:3)';
end

function s = drawInBox(lim, d, margin)
% pcRandomUniformSamples (:418-432) on the limits [xmin xmax ymin ymax zmin zmax]: the same operations in the same order
    rx = lim(2) - lim(1) + 2*margin;
    ry = lim(4) - lim(3) + 2*margin;
    rz = lim(6) - lim(5) + 2*margin;
    n = round((rx * ry * rz) / (d^3));
    s = rand(n, 3);
    s = s .* [rx, ry, rz];
    s = s + [lim(1), lim(3), lim(5)] - margin;
end
