// tests/mexdenoise/denoise_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelDenoise' and 'pointDenoise' commands of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as matlab/pcdenoiseModel.m and matlab/pcdenoiseFast.m
// drive them; the outputs are handed back through a plain C interface for tests/test_mex_denoise.py.  Returns 0, or 1 with the
// raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0) memcpy(mxGetData(a), p, m * n * 4);
    return a;
}
// a scalar argument: a double (kind 0), an int32 (1), a single (2) or a double 1 x 2 (3)
static mxArray* scalar(int kind, double v) {
    if (kind == 1) { mxArray* a = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(a) = (int32_t)v; return a; }
    if (kind == 2) { mxArray* a = mxCreateNumericMatrix(1, 1, mxSINGLE_CLASS, mxREAL); *(float*)mxGetData(a) = (float)v; return a; }
    if (kind == 3) { mxArray* a = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetPr(a)[0] = mxGetPr(a)[1] = v; return a; }
    return mxCreateDoubleScalar(v);
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

// pcreg_mex('modelDenoise' | 'pointDenoise' (via_handle 0), ...) with nargs arguments after the command.  First argument: a bogus
// (null) handle, or a 4 x 3 cloud, single or double (first_kind 1) or a 4 x 2 single (first_kind 2); k and threshold: scalar()'s kinds
int dd_usage(int via_handle, int nargs, int first_kind, int k_kind, double k, int t_kind, double t, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    const float q[12] = {0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mxArray* first;
    if (via_handle) first = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    else first = first_kind == 1 ? mxCreateDoubleMatrix(4, 3, mxREAL) : first_kind == 2 ? smat(q, 4, 2) : smat(q, 4, 3);
    std::vector<mxArray*> rhs{mxCreateString(via_handle ? "modelDenoise" : "pointDenoise"), first, scalar(k_kind, k), scalar(t_kind, t),
                              mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(3, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// via_handle: h = modelCreate(model); [inlierIndices (, meanDist (, thr))] = modelDenoise(h, k, threshold); modelDestroy(h) -- otherwise
// pointDenoise(model, k, threshold) -- with nlhs outputs (1 .. 3).  inliers: capacity M uint32, *n_inliers of them; mean_dist: M doubles.
int dd_round_trip(int via_handle, const float* model, int M, int k, double t, int nlhs, uint32_t* inliers, int* n_inliers, double* mean_dist,
                  double* thr, int* n_out, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    mxArray* h = nullptr;
    int rc;
    if (via_handle) {
        { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
        h = lhs[0]; lhs[0] = nullptr;
        std::vector<mxArray*> rhs{mxCreateString("modelDenoise"), mxDuplicateArray(h), mxCreateDoubleScalar((double)k), mxCreateDoubleScalar(t)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    } else {
        std::vector<mxArray*> rhs{mxCreateString("pointDenoise"), smat(model, M, 3), mxCreateDoubleScalar((double)k), mxCreateDoubleScalar(t)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && lhs[0]->cls == mxUINT32_CLASS && mxGetM(lhs[0]) <= (size_t)M && mxGetN(lhs[0]) == 1 && *n_out == nlhs;
        if (ok && nlhs > 1) ok = mxIsDouble(lhs[1]) && mxGetM(lhs[1]) == (size_t)M && mxGetN(lhs[1]) == 1;
        if (ok && nlhs > 2) ok = mxIsDouble(lhs[2]) && mxGetM(lhs[2]) == 1 && mxGetN(lhs[2]) == 1;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else {
            *n_inliers = (int)mxGetM(lhs[0]);
            if (*n_inliers > 0) memcpy(inliers, mxGetData(lhs[0]), (size_t)*n_inliers * 4);
            if (nlhs > 1 && M > 0) memcpy(mean_dist, mxGetPr(lhs[1]), (size_t)M * 8);
            if (nlhs > 2) *thr = mxGetScalar(lhs[2]);
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    if (h) { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
