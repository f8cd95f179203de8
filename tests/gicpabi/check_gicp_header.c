/* tests/gicpabi/check_gicp_header.c -- TEST INFRASTRUCTURE for tests/test_refit_gicp_abi.py.  Includes include/pcreg.h from plain C
 * (and, compiled again as C++, from C++) and takes the plane-to-plane refit's three entry points through function pointers of the
 * types a caller would write from the header's text: a drift between a declaration and that text (argument order, widths) fails to
 * compile under -Werror.  Then calls each with an argument the contract refuses before anything runs, so no device is needed.
 * Exit codes: 0 = every call answered as the header says; anything else = failure. */
#include "pcreg.h"
#include <stdio.h>

typedef size_t (*ws_fn)(int, int, int);
typedef int (*dev_fn)(const pcreg_dev_model*, const float*, int, int, const double*, int, float, const float*, int, const float*, int, double,
                      double*, double*, int32_t*, double*, int32_t*, double*, int32_t*, void*, size_t, void*);
typedef int (*host_fn)(pcreg_model*, const float*, int, int, const double*, int, float, int, const float*, int, const float*, int, int, double,
                       double*, int32_t*, double*, int32_t*, double*, int32_t*);

int main(void) {
    ws_fn ws = pcreg_dev_model_refit_gicp_workspace;
    dev_fn dev = pcreg_dev_model_refit_gicp_f32;
    host_fn host = pcreg_model_refit_gicp_f32;
    float q[12] = {0}, n[12] = {0};
    double T[16] = {0}, To[16], s[1], r[1];
    int32_t c[1], p[1], e[1];
    int rc;
    if (ws(4, 1, 0) != pcreg_dev_model_refit_plane_workspace(4, 1, 0) || ws(-1, 1, 0) != 0) { printf("workspace\n"); return 1; }
    rc = dev(NULL, q, 4, 4, T, 1, 1.0f, n, 4, n, 4, 1e-3, To, NULL, c, s, p, r, e, q, sizeof q, NULL);
    if (rc != PCREG_E_ARG) { printf("device tier, null handle: rc %d\n", rc); return 1; }
    rc = host(NULL, q, 4, 4, T, 1, 1.0f, 1, n, 4, n, 4, 6, 1e-3, To, c, s, p, r, e);
    if (rc != PCREG_E_ARG) { printf("host tier, null handle: rc %d\n", rc); return 1; }
    printf("ok (%s)\n", pcreg_last_error());
    return 0;
}
