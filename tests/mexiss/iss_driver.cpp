// tests/mexiss/iss_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelIss' and 'pointIss' commands of mex/pcreg_mex.cpp
// (built with tests/mexstub/mex.h into a library of its own), as matlab/detectISSModel.m and matlab/detectISSFast.m drive them; the
// outputs are handed back through a plain C interface for tests/test_mex_iss.py.  Returns 0, or 1 with the raised id:message.
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

int di_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelIss' | 'pointIss' (via_handle 0), ...) with nargs arguments after the command.  First argument: a bogus (null)
// handle, or a 4 x 3 cloud, single or double (first_kind 1) or a 4 x 2 single (first_kind 2); the five parameters: scalar()'s kinds
// and values
int di_usage(int via_handle, int nargs, int first_kind, const int* kinds, const double* vals, char* err, int errlen) {
    mxArray* lhs[4] = {nullptr, nullptr, nullptr, nullptr};
    const float q[12] = {0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mxArray* first;
    if (via_handle) first = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    else first = first_kind == 1 ? mxCreateDoubleMatrix(4, 3, mxREAL) : first_kind == 2 ? smat(q, 4, 2) : smat(q, 4, 3);
    std::vector<mxArray*> rhs{mxCreateString(via_handle ? "modelIss" : "pointIss"), first};
    for (int i = 0; i < 5; ++i) rhs.push_back(scalar(kinds[i], vals[i]));
    rhs.push_back(mxCreateDoubleScalar(1.0));
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(4, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// via_handle: h = modelCreate(model); [keypoints (, saliency (, eig (, nNeighbors)))] = modelIss(h, r2s, r2n, g21, g32, mn);
// modelDestroy(h) -- otherwise pointIss(model, ...) -- with nlhs outputs (1 .. 4).  keypoints: capacity M uint32, *n_keypoints of
// them; saliency: M doubles; eig: M x 3 doubles column-major; n_neighbors: M int32.
int di_round_trip(int via_handle, const float* model, int M, float r2s, float r2n, double g21, double g32, int mn, int nlhs, uint32_t* keypoints,
                  int* n_keypoints, double* saliency, double* eig, int32_t* n_neighbors, int* n_out, char* err, int errlen) {
    mxArray* lhs[4] = {nullptr, nullptr, nullptr, nullptr};
    mxArray* h = nullptr;
    int rc;
    auto params = [&](std::vector<mxArray*>& rhs) {
        rhs.push_back(scalar(2, r2s)); rhs.push_back(scalar(2, r2n)); rhs.push_back(mxCreateDoubleScalar(g21));
        rhs.push_back(mxCreateDoubleScalar(g32)); rhs.push_back(mxCreateDoubleScalar((double)mn));
    };
    if (via_handle) {
        { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
        h = lhs[0]; lhs[0] = nullptr;
        std::vector<mxArray*> rhs{mxCreateString("modelIss"), mxDuplicateArray(h)};
        params(rhs);
        rc = call(nlhs, lhs, rhs, err, errlen);
    } else {
        std::vector<mxArray*> rhs{mxCreateString("pointIss"), smat(model, M, 3)};
        params(rhs);
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && lhs[0]->cls == mxUINT32_CLASS && mxGetM(lhs[0]) <= (size_t)M && mxGetN(lhs[0]) == 1 && *n_out == nlhs;
        if (ok && nlhs > 1) ok = mxIsDouble(lhs[1]) && mxGetM(lhs[1]) == (size_t)M && mxGetN(lhs[1]) == 1;
        if (ok && nlhs > 2) ok = mxIsDouble(lhs[2]) && mxGetM(lhs[2]) == (size_t)M && mxGetN(lhs[2]) == 3;
        if (ok && nlhs > 3) ok = lhs[3]->cls == mxINT32_CLASS && mxGetM(lhs[3]) == (size_t)M && mxGetN(lhs[3]) == 1;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else {
            *n_keypoints = (int)mxGetM(lhs[0]);
            if (*n_keypoints > 0) memcpy(keypoints, mxGetData(lhs[0]), (size_t)*n_keypoints * 4);
            if (nlhs > 1 && M > 0) memcpy(saliency, mxGetPr(lhs[1]), (size_t)M * 8);
            if (nlhs > 2 && M > 0) memcpy(eig, mxGetPr(lhs[2]), (size_t)M * 24);
            if (nlhs > 3 && M > 0) memcpy(n_neighbors, mxGetData(lhs[3]), (size_t)M * 4);
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    if (h) { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
