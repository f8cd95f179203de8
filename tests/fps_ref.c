/* tests/fps_ref.c -- TEST INFRASTRUCTURE: the farthest point sampling contract of include/pcreg.h (pcreg_model_fps_f32) restated by
 * brute force, O(M K), in original row order: no culling, no ordering, no tiles.  Compiled with -ffp-contract=off; the one fused
 * operation is the fmaf the contract names, so the bits are the contract's.
 *
 * fps_ref returns 0 and writes what the device tier writes: idx / dist [K], *n_out, *cover_d2, min_dist / label [M], *info (each may
 * be NULL except n_out).  A dead start row: *info = 1, *n_out = 0, nothing else.  -1 for an argument the contract refuses. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

static int finite3(float x, float y, float z) { return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; }
static float point_d2(float qx, float qy, float qz, float mx, float my, float mz) {
    const float dx = qx - mx, dy = qy - my, dz = qz - mz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

int fps_ref(const float* m, int M, int ldm, int K, int start, float stop_d2, int32_t* idx, float* dist, int32_t* n_out, float* cover_d2,
            float* min_dist, int32_t* label, int32_t* info) {
    if (!n_out || K < 0 || M < 0 || ldm < M || (M > 0 && (!m || start < -1 || start >= M)) || !(stop_d2 >= 0.0f)) return -1;
    const float* x = m; const float* y = m + ldm; const float* z = m + 2 * (size_t)ldm;
    int s = -1, i, j = 0;
    if (K > 0 && M > 0) {
        if (start >= 0) {
            if (!finite3(x[start], y[start], z[start])) { *n_out = 0; if (info) *info = 1; return 0; }
            s = start;
        } else {
            for (i = 0; i < M && s < 0; ++i) if (finite3(x[i], y[i], z[i])) s = i;
        }
    }
    if (info) *info = 0;
    if (s < 0) {                                                  /* K = 0, M = 0 or no live row */
        *n_out = 0;
        if (cover_d2) *cover_d2 = NAN;
        for (i = 0; i < M; ++i) { if (min_dist) min_dist[i] = NAN; if (label) label[i] = 0; }
        return 0;
    }
    float* D = (float*)malloc(sizeof(float) * (size_t)M);
    int32_t* L = (int32_t*)malloc(sizeof(int32_t) * (size_t)M);
    char* live = (char*)malloc((size_t)M);
    if (!D || !L || !live) { free(D); free(L); free(live); return -2; }
    for (i = 0; i < M; ++i) { live[i] = (char)finite3(x[i], y[i], z[i]); D[i] = live[i] ? INFINITY : NAN; L[i] = 0; }
    float mx = INFINITY;
    for (;;) {
        if (idx) idx[j] = s;
        if (dist) dist[j] = mx;                                   /* the D[s] it was chosen with; +inf for the first */
        int r = -1;
        mx = -1.0f;
        for (i = 0; i < M; ++i) {
            if (!live[i]) continue;
            const float d = point_d2(x[i], y[i], z[i], x[s], y[s], z[s]);
            if (d < D[i]) { D[i] = d; L[i] = j + 1; }
            if (D[i] > mx) { mx = D[i]; r = i; }                  /* strict: ties stay with the lowest row */
        }
        ++j;
        if (j == K || !(mx > stop_d2)) break;
        s = r;
    }
    *n_out = j;
    if (cover_d2) *cover_d2 = mx;
    for (i = 0; i < M; ++i) { if (min_dist) min_dist[i] = D[i]; if (label) label[i] = L[i]; }
    free(D); free(L); free(live);
    return 0;
}
