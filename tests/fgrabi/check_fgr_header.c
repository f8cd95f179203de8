/* tests/fgrabi/check_fgr_header.c -- TEST INFRASTRUCTURE for tests/test_fgr_abi.py.  Includes include/pcreg.h from plain C (and,
 * compiled again as C++, from C++) and takes fast global registration's four entry points through function pointers of the types
 * a caller would write from the header's text: a drift between a declaration and that text (argument order, widths) fails to
 * compile under -Werror.  Then calls each tier with an argument the contract refuses before anything runs, so no device is needed.
 * Exit codes: 0 = every call answered as the header says; anything else = failure. */
#include "pcreg.h"
#include <stdio.h>

typedef int (*cap_fn)(void);
typedef size_t (*ws_fn)(int, int, int);
typedef int (*dev_fn)(const double*, const double*, int, const int32_t*, int, int, const pcreg_fgr_opts*, const double*, const int32_t*,
                      pcreg_fgr_result*, int32_t*, uint8_t*, void*, size_t, void*);
typedef int (*host_fn)(const double*, const double*, int, int, const int32_t*, int, const pcreg_fgr_opts*, const double*, const int32_t*,
                       pcreg_fgr_result*, int32_t*, uint8_t*);

int main(void) {
    cap_fn cap = pcreg_fgr_resident_capacity;
    ws_fn ws = pcreg_dev_fgr_batched_workspace;
    dev_fn dev = pcreg_dev_fgr_batched;
    host_fn host = pcreg_fgr_batched;
    double p[12] = {0};
    int32_t off[2] = {0, 4}, inl[4];
    pcreg_fgr_opts o = {1.0, 128, 4, 1.4, 0.0, 0, 0, 0.95, 0};
    pcreg_fgr_result r[1];
    int rc;
    if (sizeof(pcreg_fgr_opts) != 56 || sizeof(pcreg_fgr_result) != 184) { printf("struct sizes\n"); return 1; }
    if (cap() < 2049 || cap() * 48 > 160 * 1024) { printf("capacity\n"); return 1; }
    if (ws(4, 1, 128) == 0 || ws(-1, 1, 128) != 0 || ws(4, 0, 128) != 0 || ws(4, 1, 0) != 0) { printf("workspace\n"); return 1; }
    o.division_factor = 1.0;
    rc = dev(p, p, 4, off, 1, 4, &o, NULL, NULL, r, inl, NULL, p, sizeof p, NULL);
    if (rc != PCREG_E_ARG) { printf("device tier, division_factor 1: rc %d\n", rc); return 1; }
    rc = host(p, p, 4, 4, off, 1, &o, NULL, NULL, r, inl, NULL);
    if (rc != PCREG_E_ARG) { printf("host tier, division_factor 1: rc %d\n", rc); return 1; }
    printf("ok (%s)\n", pcreg_last_error());
    return 0;
}
