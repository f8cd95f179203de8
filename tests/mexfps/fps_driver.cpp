// tests/mexfps/fps_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelFps' and 'pointFps' commands of mex/pcreg_mex.cpp
// (built with tests/mexstub/mex.h into a library of its own), as matlab/farthestPointsModel.m and matlab/farthestPointsFast.m drive
// them; the outputs are handed back through a plain C interface for tests/test_mex_fps.py.  Returns 0, or 1 with the raised
// id:message.
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

int fd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelFps' | 'pointFps' (via_handle 0), ...) with nargs arguments after the command.  First argument: a bogus (null)
// handle, or a 4 x 3 cloud, single or double (first_kind 1) or a 4 x 2 single (first_kind 2); K, start and stopD2: scalar()'s kinds
int fd_usage(int via_handle, int nargs, int first_kind, int k_kind, double K, int s_kind, double start, int r_kind, double stop, char* err,
             int errlen) {
    mxArray* lhs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const float q[12] = {0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mxArray* first;
    if (via_handle) first = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    else first = first_kind == 1 ? mxCreateDoubleMatrix(4, 3, mxREAL) : first_kind == 2 ? smat(q, 4, 2) : smat(q, 4, 3);
    std::vector<mxArray*> rhs{mxCreateString(via_handle ? "modelFps" : "pointFps"), first, scalar(k_kind, K), scalar(s_kind, start),
                              scalar(r_kind, stop), mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(5, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// via_handle: h = modelCreate(model); [idx (, d2 (, label (, minD2 (, coverD2))))] = modelFps(h, K, start, stopD2); modelDestroy(h) --
// otherwise pointFps(model, K, start, stopD2) -- with nlhs outputs (1 .. 5); start is 1-based (0: the lowest finite row).  idx / d2:
// capacity K, *n of them; label / min_d2: M entries.
int fd_round_trip(int via_handle, const float* model, int M, int K, int start, float stop_d2, int nlhs, uint32_t* idx, float* d2, int* n,
                  uint32_t* label, float* min_d2, float* cover, int* n_out, char* err, int errlen) {
    mxArray* lhs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    mxArray* h = nullptr;
    int rc;
    if (via_handle) {
        { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
        h = lhs[0]; lhs[0] = nullptr;
        std::vector<mxArray*> rhs{mxCreateString("modelFps"), mxDuplicateArray(h), mxCreateDoubleScalar((double)K), mxCreateDoubleScalar((double)start),
                                  scalar(2, (double)stop_d2)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    } else {
        std::vector<mxArray*> rhs{mxCreateString("pointFps"), smat(model, M, 3), mxCreateDoubleScalar((double)K), mxCreateDoubleScalar((double)start),
                                  scalar(2, (double)stop_d2)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && lhs[0]->cls == mxUINT32_CLASS && mxGetM(lhs[0]) <= (size_t)K && mxGetN(lhs[0]) == 1 && *n_out == nlhs;
        if (ok && nlhs > 1) ok = mxIsSingle(lhs[1]) && mxGetM(lhs[1]) == mxGetM(lhs[0]) && mxGetN(lhs[1]) == 1;
        if (ok && nlhs > 2) ok = lhs[2]->cls == mxUINT32_CLASS && mxGetM(lhs[2]) == (size_t)M && mxGetN(lhs[2]) == 1;
        if (ok && nlhs > 3) ok = mxIsSingle(lhs[3]) && mxGetM(lhs[3]) == (size_t)M && mxGetN(lhs[3]) == 1;
        if (ok && nlhs > 4) ok = mxIsSingle(lhs[4]) && mxGetM(lhs[4]) == 1 && mxGetN(lhs[4]) == 1;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else {
            *n = (int)mxGetM(lhs[0]);
            if (*n > 0) memcpy(idx, mxGetData(lhs[0]), (size_t)*n * 4);
            if (nlhs > 1 && *n > 0) memcpy(d2, mxGetData(lhs[1]), (size_t)*n * 4);
            if (nlhs > 2 && M > 0) memcpy(label, mxGetData(lhs[2]), (size_t)M * 4);
            if (nlhs > 3 && M > 0) memcpy(min_d2, mxGetData(lhs[3]), (size_t)M * 4);
            if (nlhs > 4) *cover = *(const float*)mxGetData(lhs[4]);
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    if (h) { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
