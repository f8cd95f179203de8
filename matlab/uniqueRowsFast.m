function [C, ia] = uniqueRowsFast(A)
%UNIQUEROWSFAST  [C, ia] = uniqueRowsFast(A): [C, ia] = unique(A, 'rows') for an n x 3 double matrix on the GPU.
%   The rows of C are in lexicographic order by column 1, 2, 3 (-0 equals +0); ia holds the FIRST occurrence of every
%   row of C in A, a double column, so that C = A(ia, :) carries that occurrence's bits.  A row that holds a NaN is
%   refused: unique keeps every NaN row apart, which this ordering does not do.
ia = pcreg_mex('uniqueRows3', double(A));
C = A(ia, :);
end
