/* tests/trimabi/check_trim_header.c -- TEST INFRASTRUCTURE for tests/test_trim_abi.py.  Includes include/pcreg.h from plain C (and,
 * compiled again as C++, from C++) and takes the trimmed scoring and refits' eight entry points through function pointers of the
 * types a caller would write from the header's text: a drift between a declaration and that text (argument order, widths) fails to
 * compile under -Werror.  Then calls each with an argument the contract refuses before anything runs, so no device is needed.
 * Exit codes: 0 = every call answered as the header says; anything else = failure. */
#include "pcreg.h"
#include <stdio.h>

typedef size_t (*ws_fn)(int, int, int);
typedef int (*dev_score_fn)(const pcreg_dev_model*, const float*, int, int, const double*, int, float, double, int32_t*, double*, int32_t*, float*,
                            void*, size_t, void*, int32_t*, float*);
typedef int (*dev_refit_fn)(const pcreg_dev_model*, const float*, int, int, const double*, int, float, double, double*, double*, int32_t*, double*,
                            int32_t*, void*, size_t, void*, int32_t*, float*);
typedef int (*dev_plane_fn)(const pcreg_dev_model*, const float*, int, int, const double*, int, float, double, const float*, int, double*, double*,
                            int32_t*, double*, int32_t*, double*, int32_t*, void*, size_t, void*, int32_t*, float*);
typedef int (*dev_gicp_fn)(const pcreg_dev_model*, const float*, int, int, const double*, int, float, double, const float*, int, const float*, int,
                           double, double*, double*, int32_t*, double*, int32_t*, double*, int32_t*, void*, size_t, void*, int32_t*, float*);
typedef int (*host_score_fn)(pcreg_model*, const float*, int, int, const double*, int, float, double, int32_t*, double*, int32_t*, float*, int32_t*,
                             float*);
typedef int (*host_refit_fn)(pcreg_model*, const float*, int, int, const double*, int, float, double, int, double*, int32_t*, double*, int32_t*,
                             int32_t*, float*);
typedef int (*host_plane_fn)(pcreg_model*, const float*, int, int, const double*, int, float, double, int, const float*, int, int, double*, int32_t*,
                             double*, int32_t*, double*, int32_t*, int32_t*, float*);
typedef int (*host_gicp_fn)(pcreg_model*, const float*, int, int, const double*, int, float, double, int, const float*, int, const float*, int, int,
                            double, double*, int32_t*, double*, int32_t*, double*, int32_t*, int32_t*, float*);

int main(void) {
    ws_fn old[4] = {pcreg_dev_model_score_workspace, pcreg_dev_model_refit_workspace, pcreg_dev_model_refit_plane_workspace,
                    pcreg_dev_model_refit_gicp_workspace};
    dev_score_fn dev_score = pcreg_dev_model_score_trimmed_f32;
    dev_refit_fn dev_refit = pcreg_dev_model_refit_trimmed_f32;
    dev_plane_fn dev_plane = pcreg_dev_model_refit_plane_trimmed_f32;
    dev_gicp_fn dev_gicp = pcreg_dev_model_refit_gicp_trimmed_f32;
    host_score_fn host_score = pcreg_model_score_trimmed_f32;
    host_refit_fn host_refit = pcreg_model_refit_trimmed_f32;
    host_plane_fn host_plane = pcreg_model_refit_plane_trimmed_f32;
    host_gicp_fn host_gicp = pcreg_model_refit_gicp_trimmed_f32;
    float q[12] = {0}, n[12] = {0}, cut[1];
    double T[16] = {0}, To[16], s[1], r[1];
    int32_t c[1], p[1], e[1], w[1];
    int rc[8], i;
    for (i = 0; i < 4; ++i) {
        /* the trimmed entries take the untrimmed workspace: q below is far smaller than it, which PCREG_E_ARG must say too */
        if (old[i](4, 1, 0) <= sizeof q || old[i](-1, 1, 0) != 0) { printf("workspace %d\n", i); return 1; }
    }
    rc[0] = dev_score(NULL, q, 4, 4, T, 1, 1.0f, 0.5, c, s, NULL, NULL, q, sizeof q, NULL, w, cut);
    rc[1] = dev_refit(NULL, q, 4, 4, T, 1, 1.0f, 0.5, To, NULL, c, s, e, q, sizeof q, NULL, w, cut);
    rc[2] = dev_plane(NULL, q, 4, 4, T, 1, 1.0f, 0.5, n, 4, To, NULL, c, s, p, r, e, q, sizeof q, NULL, w, cut);
    rc[3] = dev_gicp(NULL, q, 4, 4, T, 1, 1.0f, 0.5, n, 4, n, 4, 1e-3, To, NULL, c, s, p, r, e, q, sizeof q, NULL, w, cut);
    rc[4] = host_score(NULL, q, 4, 4, T, 1, 1.0f, 0.5, c, s, NULL, NULL, w, cut);
    rc[5] = host_refit(NULL, q, 4, 4, T, 1, 1.0f, 0.5, 1, To, c, s, e, w, cut);
    rc[6] = host_plane(NULL, q, 4, 4, T, 1, 1.0f, 0.5, 1, n, 4, 6, To, c, s, p, r, e, w, cut);
    rc[7] = host_gicp(NULL, q, 4, 4, T, 1, 1.0f, 0.5, 1, n, 4, n, 4, 6, 1e-3, To, c, s, p, r, e, NULL, NULL);
    for (i = 0; i < 8; ++i)
        if (rc[i] != PCREG_E_ARG) { printf("entry %d, null handle: rc %d\n", i, rc[i]); return 1; }
    printf("ok (%s)\n", pcreg_last_error());
    return 0;
}
