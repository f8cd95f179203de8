// tests/mexdownsample/downsample_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'downsampleGrid' command of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as matlab/pcdownsampleFast.m drives it; the outputs
// are handed back through a plain C interface for tests/test_mex_downsample.py.  Returns 0, or 1 with the raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0 && p) memcpy(mxGetData(a), p, m * n * 4);
    return a;
}

static int call(int nlhs, mxArray** plhs, std::vector<mxArray*>& rhs, char* err, int errlen) {
    int rc = 0;
    try { mexFunction(nlhs, plhs, (int)rhs.size(), const_cast<const mxArray**>(rhs.data())); }
    catch (const MexError& e) { snprintf(err, errlen, "%s: %s", e.id.c_str(), e.msg.c_str()); rc = 1; }
    for (mxArray* a : rhs) mxDestroyArray(a);
    return rc;
}

extern "C" {

int dd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('downsampleGrid', ...) with nargs arguments after the command.  The cloud: a 4 x 3 single (first_kind 0), a 4 x 3 double
// (1) or a 4 x 2 single (2); the step: a double scalar `step`, an int32 scalar (step_kind 1) or a double 1 x 2 (2)
int dd_usage(int nargs, int first_kind, int step_kind, double step, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    const float q[12] = {0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mxArray* first = first_kind == 1 ? mxCreateDoubleMatrix(4, 3, mxREAL) : first_kind == 2 ? smat(q, 4, 2) : smat(q, 4, 3);
    mxArray* sa;
    if (step_kind == 1) { sa = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(sa) = (int32_t)step; }
    else if (step_kind == 2) sa = mxCreateDoubleMatrix(1, 2, mxREAL);
    else sa = mxCreateDoubleScalar(step);
    std::vector<mxArray*> rhs{mxCreateString("downsampleGrid"), first, sa, mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(3, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// [ptsOut (, counts (, labels))] = downsampleGrid(single(pts), step) with nlhs outputs (1 .. 3).  out: room for 3 n floats, written
// as u x 3 column-major; counts: n; labels: n; *u_out = u
int dd_round_trip(const float* pts, int n, double step, int nlhs, float* out, int32_t* counts, int32_t* labels, int* u_out, int* n_lhs,
                  char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    std::vector<mxArray*> rhs{mxCreateString("downsampleGrid"), smat(pts, n, 3), mxCreateDoubleScalar(step)};
    int rc = call(nlhs, lhs, rhs, err, errlen);
    if (!rc) {
        *n_lhs = 0;
        for (mxArray* a : lhs) *n_lhs += a != nullptr;
        const size_t u = lhs[0] ? mxGetM(lhs[0]) : 0;
        bool ok = lhs[0] && mxIsSingle(lhs[0]) && mxGetN(lhs[0]) == 3 && u <= (size_t)n && *n_lhs == nlhs;
        if (ok && nlhs > 1) ok = mxIsInt32(lhs[1]) && mxGetM(lhs[1]) == u;
        if (ok && nlhs > 2) ok = mxIsInt32(lhs[2]) && mxGetM(lhs[2]) == (size_t)n;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else {
            *u_out = (int)u;
            if (u > 0) memcpy(out, mxGetData(lhs[0]), u * 3 * 4);
            if (nlhs > 1 && u > 0) memcpy(counts, mxGetData(lhs[1]), u * 4);
            if (nlhs > 2 && n > 0) memcpy(labels, mxGetData(lhs[2]), (size_t)n * 4);
        }
    }
    for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    return rc;
}

}  // extern "C"
