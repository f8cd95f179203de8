/* tests/fpsabi/check_fps_header.c -- TEST INFRASTRUCTURE for tests/test_fps_abi.py.  Includes include/pcreg.h from plain C (and,
 * compiled again as C++, from C++) and takes the farthest point sampling's four entry points through function pointers of the types
 * a caller would write from the header's text: a drift between a declaration and that text (argument order, widths) fails to
 * compile under -Werror.  Then calls each with an argument the contract refuses before anything runs, so no device is needed.
 * Exit codes: 0 = every call answered as the header says; anything else = failure. */
#include "pcreg.h"
#include <stdio.h>

typedef size_t (*ws_fn)(int, int);
typedef int (*dev_fn)(const pcreg_dev_model*, int, int, float, int32_t*, float*, int32_t*, float*, float*, int32_t*, int32_t*, void*, size_t, void*);
typedef int (*host_fn)(pcreg_model*, int, int, float, int32_t*, float*, int32_t*, float*, float*, int32_t*);
typedef int (*point_fn)(const float*, int, int, int, int, float, int32_t*, float*, int32_t*, float*, float*, int32_t*);

int main(void) {
    ws_fn ws = pcreg_dev_model_fps_workspace;
    dev_fn dev = pcreg_dev_model_fps_f32;
    host_fn host = pcreg_model_fps_f32;
    point_fn point = pcreg_point_fps_f32;
    float m[12] = {0}, dist[2], cover, md[4];
    int32_t idx[2], n, lab[4], info;
    int rc;
    if (ws(4, 2) != 3 * 256 + 256 || ws(-1, 2) != 0 || ws(PCREG_FPS_MAX_ROWS, 2) == 0 || ws(PCREG_FPS_MAX_ROWS + 1, 2) != 0) { printf("workspace\n"); return 1; }
    rc = dev(NULL, 2, -1, 0.0f, idx, dist, &n, &cover, md, lab, &info, m, sizeof m, NULL);
    if (rc != PCREG_E_ARG) { printf("device tier, null handle: rc %d\n", rc); return 1; }
    rc = host(NULL, 2, -1, 0.0f, idx, dist, &n, &cover, md, lab);
    if (rc != PCREG_E_ARG) { printf("host tier, null handle: rc %d\n", rc); return 1; }
    rc = point(m, 4, 4, 2, 4, 0.0f, idx, dist, &n, &cover, md, lab);
    if (rc != PCREG_E_ARG) { printf("point tier, start = M: rc %d\n", rc); return 1; }
    rc = point(m, 4, 4, 2, -1, -1.0f, idx, dist, &n, &cover, md, lab);
    if (rc != PCREG_E_ARG) { printf("point tier, stop_d2 < 0: rc %d\n", rc); return 1; }
    printf("ok (%s)\n", pcreg_last_error());
    return 0;
}
