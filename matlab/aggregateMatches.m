function [pts1, pts2, ia] = aggregateMatches(pts1_agg, pts2_agg)
%AGGREGATEMATCHES  [pts1, pts2, ia] = aggregateMatches(pts1_agg, pts2_agg): the stacked putative matches of a cluster of
%   spheres made unique, completeExperiment.m:440-443 in one call:
%       [pts1_agg, ia] = unique(pts1_agg, 'rows');  pts2_agg = pts2_agg(ia, :);
%       [pts2_agg, ia] = unique(pts2_agg, 'rows');  pts1_agg = pts1_agg(ia, :);
%   pts1 / pts2 are the surviving pairs, sorted by the model point (pts2); ia their rows in the input (a double column).
%   Then, as the script does: [T, inl] = ransac(pts1, pts2, options, @estimateTransform, @calcDists) and
%   T_final = estimateTransform(pts1(inl, :), pts2(inl, :)).
[pts1, pts2, ia] = pcreg_mex('aggregateMatches', double(pts1_agg), double(pts2_agg));
end
