/* tests/cluster_ref.c -- TEST REFERENCE: clusterPoints as connected components in fp32, the library's contract restated in
 * plain C.  Rows i != j are adjacent iff d = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) <= r2 with dx = m_i.x - m_j.x in float
 * (compiled with -ffp-contract=off, so nothing else fuses), as a float comparison (inclusive; NaN never passes; +inf <= +inf
 * does).  A row with a non-finite coordinate has no neighbour.  Clusters are numbered in ascending order of their smallest row.
 *
 * The neighbour scan goes over a uniform grid in double.  A computed d <= r2 bounds the true coordinate differences by
 * sqrt(r2) (1 + 4u) + 2^-73 (rounding of the chain, and the absolute error of a product that underflows), so with cells of
 * sqrt(r2) (1 + 1e-3) + 1e-21 or larger every adjacent pair lies in the same or in neighbouring cells.  At most 256 cells per
 * axis (larger cells are still valid).  r2 = +inf: every pair of finite rows is adjacent (their d is a number or +inf, never
 * NaN), so all finite rows are one cluster and no scan is needed.  Serial union-find, the larger root hooked under the smaller.
 * Points are column-major (x = p[i], y = p[i + ld], z = p[i + 2 ld]). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int find(int32_t* parent, int a) {
    while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; }
    return a;
}
static void unite(int32_t* parent, int a, int b) {
    const int ra = find(parent, a), rb = find(parent, b);
    if (ra < rb) parent[rb] = ra; else if (rb < ra) parent[ra] = rb;
}

/* label [M], *n_clusters, cl_off [M + 1], members [M]; returns 0, or 3 when out of memory */
int cluster_ref(const float* m, int M, int ld, float r2, int32_t* label, int32_t* n_clusters, int32_t* cl_off, int32_t* members) {
    *n_clusters = 0;
    cl_off[0] = 0;
    if (M <= 0) return M < 0 ? 1 : 0;
    const float *X = m, *Y = m + (size_t)ld, *Z = m + 2 * (size_t)ld;
    int32_t* parent = (int32_t*)malloc(sizeof(int32_t) * (size_t)M);
    int32_t* cell = (int32_t*)malloc(sizeof(int32_t) * (size_t)M);
    int32_t* rows = (int32_t*)malloc(sizeof(int32_t) * (size_t)M);
    if (!parent || !cell || !rows) { free(parent); free(cell); free(rows); return 3; }
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int n_fin = 0, first_fin = -1;
    for (int i = 0; i < M; ++i) {
        parent[i] = i;
        cell[i] = -1;
        if (!(isfinite(X[i]) && isfinite(Y[i]) && isfinite(Z[i]))) continue;
        const double p[3] = {X[i], Y[i], Z[i]};
        for (int c = 0; c < 3; ++c) { if (p[c] < lo[c]) lo[c] = p[c]; if (p[c] > hi[c]) hi[c] = p[c]; }
        if (first_fin < 0) first_fin = i;
        ++n_fin;
    }
    if (n_fin > 1 && r2 == INFINITY) {
        for (int i = 0; i < M; ++i) if (isfinite(X[i]) && isfinite(Y[i]) && isfinite(Z[i])) parent[i] = first_fin;
    } else if (n_fin > 1) {
        const double want = sqrt((double)r2) * (1.0 + 1e-3) + 1e-21;
        int n[3]; double cs[3];
        for (int c = 0; c < 3; ++c) {
            const double ext = hi[c] - lo[c], cnt = floor(ext / want) + 1.0;
            if (cnt > 256.0) { n[c] = 256; cs[c] = ext / 256.0; } else { n[c] = (int)cnt; cs[c] = want; }
        }
        const size_t ncell = (size_t)n[0] * n[1] * n[2];
        int32_t* start = (int32_t*)calloc(ncell + 1, sizeof(int32_t));
        if (!start) { free(parent); free(cell); free(rows); return 3; }
        for (int i = 0; i < M; ++i) {
            if (!(isfinite(X[i]) && isfinite(Y[i]) && isfinite(Z[i]))) continue;
            const double p[3] = {X[i], Y[i], Z[i]};
            int k[3];
            for (int c = 0; c < 3; ++c) {
                double f = floor((p[c] - lo[c]) / cs[c]);
                if (!(f >= 0.0)) f = 0.0;
                if (f > n[c] - 1) f = n[c] - 1;
                k[c] = (int)f;
            }
            cell[i] = (int32_t)(((size_t)k[2] * n[1] + k[1]) * n[0] + k[0]);
            ++start[cell[i] + 1];
        }
        for (size_t c = 0; c < ncell; ++c) start[c + 1] += start[c];
        for (int i = M - 1; i >= 0; --i) if (cell[i] >= 0) rows[--start[cell[i] + 1]] = i;      /* ascending rows per cell; start[c + 1] becomes the begin of c */
        /* after the pass above the begin of cell c is start[c + 1] and its end is the begin of c + 1, start[c + 2] (n_fin for the last) */
        for (int i = 0; i < M; ++i) {
            if (cell[i] < 0) continue;
            const int kx = cell[i] % n[0], ky = (cell[i] / n[0]) % n[1], kz = cell[i] / (n[0] * n[1]);
            for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
                const int x = kx + dx, y = ky + dy, z = kz + dz;
                if (x < 0 || y < 0 || z < 0 || x >= n[0] || y >= n[1] || z >= n[2]) continue;
                const size_t c = ((size_t)z * n[1] + y) * n[0] + x;
                const int32_t b = start[c + 1], e = c + 1 < ncell ? start[c + 2] : n_fin;
                for (int32_t s = b; s < e; ++s) {
                    const int j = rows[s];
                    if (j <= i) continue;
                    const float ex = X[i] - X[j], ey = Y[i] - Y[j], ez = Z[i] - Z[j];
                    const float d = fmaf(ez, ez, fmaf(ey, ey, ex * ex));
                    if (d <= r2) unite(parent, i, j);
                }
            }
        }
        free(start);
    }
    /* numbering: a root is its set's smallest row */
    int32_t nc = 0;
    for (int i = 0; i < M; ++i) if (parent[i] == i) cell[i] = nc++;
    for (int i = 0; i < M; ++i) label[i] = cell[find(parent, i)];
    for (int c = 0; c <= nc; ++c) cl_off[c] = 0;
    for (int i = 0; i < M; ++i) ++cl_off[label[i] + 1];
    for (int c = 0; c < nc; ++c) cl_off[c + 1] += cl_off[c];
    for (int c = 0; c < nc; ++c) rows[c] = cl_off[c];
    for (int i = 0; i < M; ++i) members[rows[label[i]]++] = i;
    *n_clusters = nc;
    free(parent); free(cell); free(rows);
    return 0;
}
