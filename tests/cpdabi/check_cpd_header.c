/* tests/cpdabi/check_cpd_header.c -- TEST INFRASTRUCTURE for tests/test_cpd_abi.py.  Includes include/pcreg.h from plain C (and,
 * compiled again as C++, from C++) and takes the coherent-point-drift refit's three entry points through function pointers of the
 * types a caller would write from the header's text: a drift between a declaration and that text (argument order, widths) fails to
 * compile under -Werror.  Then calls each with an argument the contract refuses before anything runs, so no device is needed.
 * Exit codes: 0 = every call answered as the header says; anything else = failure. */
#include "pcreg.h"
#include <stdio.h>

typedef size_t (*ws_fn)(int, int, int);
typedef int (*dev_fn)(const pcreg_dev_model*, const float*, int, int, const double*, int, const double*, double, double*, double*, double*, double*,
                      double*, double*, int32_t*, int32_t*, void*, size_t, void*);
typedef int (*host_fn)(pcreg_model*, const float*, int, int, const double*, int, const double*, double, int, double*, double*, double*, double*,
                       double*, int32_t*, int32_t*);

int main(void) {
    ws_fn ws = pcreg_dev_model_refit_cpd_workspace;
    dev_fn dev = pcreg_dev_model_refit_cpd_f32;
    host_fn host = pcreg_model_refit_cpd_f32;
    float q[12] = {0};
    double T[16] = {0}, To[16], sg[1] = {0}, so[1], np[1], r[1], s[1];
    int32_t n[1], e[1];
    int rc;
    if (ws(4, 1, 3) == 0 || ws(-1, 1, 3) != 0 || ws(4, 1, 3) < pcreg_dev_model_score_workspace(4, 1, 3)) { printf("workspace\n"); return 1; }
    rc = dev(NULL, q, 4, 4, T, 1, sg, 0.1, To, NULL, so, np, r, s, n, e, q, sizeof q, NULL);
    if (rc != PCREG_E_ARG) { printf("device tier, null handle: rc %d\n", rc); return 1; }
    rc = host(NULL, q, 4, 4, T, 1, sg, 0.1, 1, To, so, np, r, s, n, e);
    if (rc != PCREG_E_ARG) { printf("host tier, null handle: rc %d\n", rc); return 1; }
    printf("ok (%s)\n", pcreg_last_error());
    return 0;
}
