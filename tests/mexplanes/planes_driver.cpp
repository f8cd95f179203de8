// tests/mexplanes/planes_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelPlanes' and 'pointPlanes' commands of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as matlab/fitPlanesModel.m and matlab/fitPlanesFast.m
// drive them; the outputs are handed back through a plain C interface for tests/test_mex_planes.py.  Returns 0, or 1 with the raised
// id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0) memcpy(mxGetData(a), p, m * n * 4);
    return a;
}
// a scalar argument: a double (kind 0), an int32 (1), a single (2), a double 1 x 2 (3) or an empty double (4)
static mxArray* scalar(int kind, double v) {
    if (kind == 1) { mxArray* a = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(a) = (int32_t)v; return a; }
    if (kind == 2) { mxArray* a = mxCreateNumericMatrix(1, 1, mxSINGLE_CLASS, mxREAL); *(float*)mxGetData(a) = (float)v; return a; }
    if (kind == 3) { mxArray* a = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetPr(a)[0] = mxGetPr(a)[1] = v; return a; }
    if (kind == 4) return mxCreateDoubleMatrix(0, 0, mxREAL);
    return mxCreateDoubleScalar(v);
}
static mxArray* ref_arg(const double* ref) {
    if (!ref) return mxCreateDoubleMatrix(0, 0, mxREAL);
    mxArray* a = mxCreateDoubleMatrix(1, 3, mxREAL);
    memcpy(mxGetPr(a), ref, 24);
    return a;
}
static mxArray* samples_arg(const int32_t* s, size_t rows, size_t cols) {
    if (!s) return mxCreateDoubleMatrix(0, 0, mxREAL);
    mxArray* a = mxCreateNumericMatrix(rows, cols, mxINT32_CLASS, mxREAL);
    if (rows * cols > 0) memcpy(mxGetData(a), s, rows * cols * 4);
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

int dp_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelPlanes' | 'pointPlanes' (via_handle 0), ...) with nargs arguments after the command.  First argument: a bogus
// (null) handle, or a 4 x 3 cloud, single or double (first_kind 1) or a 4 x 2 single (first_kind 2).  The parameters: maxDistance,
// maxAngle, maxPlanes, nTrials, minInliers, seed by scalar()'s kinds and values (six of each); ref_kind 0: [], 1: double 1 x 3 of
// ref, 2: double 1 x 2; samples_kind 0: [], 1: int32 3 x samples_cols zeros, 2: double 3 x samples_cols
int dp_usage(int via_handle, int nargs, int first_kind, const int* kinds, const double* vals, int ref_kind, const double* ref, int samples_kind,
             int samples_cols, char* err, int errlen) {
    mxArray* lhs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const float q[12] = {0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mxArray* first;
    if (via_handle) first = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    else first = first_kind == 1 ? mxCreateDoubleMatrix(4, 3, mxREAL) : first_kind == 2 ? smat(q, 4, 2) : smat(q, 4, 3);
    std::vector<mxArray*> rhs{mxCreateString(via_handle ? "modelPlanes" : "pointPlanes"), first};
    rhs.push_back(scalar(kinds[0], vals[0]));
    rhs.push_back(ref_kind == 1 ? ref_arg(ref) : ref_kind == 2 ? scalar(3, 1.0) : ref_arg(nullptr));
    for (int i = 1; i < 6; ++i) rhs.push_back(scalar(kinds[i], vals[i]));
    rhs.push_back(samples_kind == 1 ? mxCreateNumericMatrix(3, (size_t)samples_cols, mxINT32_CLASS, mxREAL)
                                    : samples_kind == 2 ? mxCreateDoubleMatrix(3, (size_t)samples_cols, mxREAL) : mxCreateDoubleMatrix(0, 0, mxREAL));
    rhs.push_back(mxCreateDoubleScalar(1.0));
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(6, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// via_handle: h = modelCreate(model); [labels (, planes (, centres (, counts (, rmse (, diag)))))] = modelPlanes(h, t, ref, ang, P, B,
// minInl, seed, samples); modelDestroy(h) -- otherwise pointPlanes(model, ...) -- with nlhs outputs (1 .. 6).  ref: three doubles or
// null; samples: int32 3 x (B * P), 1-based, or null.  labels: M int32; planes: capacity P x 4 doubles, handed back ROW-major, *n_planes
// rows; centres: P x 3 likewise; counts: P int32; rmse: P doubles; diag: P x 3 doubles row-major.
int dp_round_trip(int via_handle, const float* model, int M, float t, const double* ref, double ang, int P, int B, int min_inliers, double seed,
                  const int32_t* samples, int nlhs, int32_t* labels, double* planes, double* centres, int32_t* counts, double* rmse, double* diag,
                  int* n_planes, int* n_out, char* err, int errlen) {
    mxArray* lhs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    mxArray* h = nullptr;
    int rc;
    auto params = [&](std::vector<mxArray*>& rhs) {
        rhs.push_back(scalar(2, t)); rhs.push_back(ref_arg(ref)); rhs.push_back(mxCreateDoubleScalar(ang));
        rhs.push_back(mxCreateDoubleScalar((double)P)); rhs.push_back(mxCreateDoubleScalar((double)B));
        rhs.push_back(mxCreateDoubleScalar((double)min_inliers)); rhs.push_back(mxCreateDoubleScalar(seed));
        rhs.push_back(samples_arg(samples, 3, (size_t)P * (size_t)B));
    };
    if (via_handle) {
        { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
        h = lhs[0]; lhs[0] = nullptr;
        std::vector<mxArray*> rhs{mxCreateString("modelPlanes"), mxDuplicateArray(h)};
        params(rhs);
        rc = call(nlhs, lhs, rhs, err, errlen);
    } else {
        std::vector<mxArray*> rhs{mxCreateString("pointPlanes"), smat(model, M, 3)};
        params(rhs);
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && lhs[0]->cls == mxINT32_CLASS && mxGetM(lhs[0]) == (size_t)M && mxGetN(lhs[0]) == 1 && *n_out == nlhs;
        const size_t n = nlhs > 1 && lhs[1] ? mxGetM(lhs[1]) : 0;
        if (ok && nlhs > 1) ok = mxIsDouble(lhs[1]) && n <= (size_t)P && mxGetN(lhs[1]) == 4;
        if (ok && nlhs > 2) ok = mxIsDouble(lhs[2]) && mxGetM(lhs[2]) == n && mxGetN(lhs[2]) == 3;
        if (ok && nlhs > 3) ok = lhs[3]->cls == mxINT32_CLASS && mxGetM(lhs[3]) == n && mxGetN(lhs[3]) == 1;
        if (ok && nlhs > 4) ok = mxIsDouble(lhs[4]) && mxGetM(lhs[4]) == n && mxGetN(lhs[4]) == 1;
        if (ok && nlhs > 5) ok = mxIsDouble(lhs[5]) && mxGetM(lhs[5]) == (size_t)P && mxGetN(lhs[5]) == 3;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else {
            *n_planes = (int)n;
            if (M > 0) memcpy(labels, mxGetData(lhs[0]), (size_t)M * 4);
            for (size_t i = 0; i < n; ++i) {
                if (nlhs > 1) for (int c = 0; c < 4; ++c) planes[i * 4 + c] = mxGetPr(lhs[1])[i + (size_t)c * n];
                if (nlhs > 2) for (int c = 0; c < 3; ++c) centres[i * 3 + c] = mxGetPr(lhs[2])[i + (size_t)c * n];
                if (nlhs > 3) counts[i] = ((const int32_t*)mxGetData(lhs[3]))[i];
                if (nlhs > 4) rmse[i] = mxGetPr(lhs[4])[i];
            }
            if (nlhs > 5) for (int i = 0; i < P; ++i) for (int c = 0; c < 3; ++c) diag[i * 3 + c] = mxGetPr(lhs[5])[(size_t)i + (size_t)c * (size_t)P];
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    if (h) { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
