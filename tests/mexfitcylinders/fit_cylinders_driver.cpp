// tests/mexfitcylinders/fit_cylinders_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelFitCylinders' and
// 'pointFitCylinders' commands of mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as
// matlab/fitCylindersModel.m and matlab/fitCylindersFast.m drive them; the outputs are handed back through a plain C interface for
// tests/test_mex_fit_cylinders.py.  Returns 0, or 1 with the raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0 && p) memcpy(mxGetData(a), p, m * n * 4);
    return a;
}
// an argument: a double (kind 0), an int32 (1), a single (2), a double 1 x 2 (3), an empty double (4), a single 1 x 2 (5), a double
// 1 x 3 (6), a single 4 x 3 (7), a single 3 x 3 (8) or a double 4 x 3 (9), every entry v
static mxArray* scalar(int kind, double v) {
    if (kind == 1) { mxArray* a = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(a) = (int32_t)v; return a; }
    if (kind == 2) { mxArray* a = mxCreateNumericMatrix(1, 1, mxSINGLE_CLASS, mxREAL); *(float*)mxGetData(a) = (float)v; return a; }
    if (kind == 3) { mxArray* a = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetPr(a)[0] = mxGetPr(a)[1] = v; return a; }
    if (kind == 4) return mxCreateDoubleMatrix(0, 0, mxREAL);
    if (kind == 5) { mxArray* a = mxCreateNumericMatrix(1, 2, mxSINGLE_CLASS, mxREAL); ((float*)mxGetData(a))[0] = ((float*)mxGetData(a))[1] = (float)v; return a; }
    if (kind == 6) { mxArray* a = mxCreateDoubleMatrix(1, 3, mxREAL); for (int i = 0; i < 3; ++i) mxGetPr(a)[i] = v; return a; }
    if (kind == 7 || kind == 8) {
        const size_t m = kind == 7 ? 4 : 3;
        mxArray* a = mxCreateNumericMatrix(m, 3, mxSINGLE_CLASS, mxREAL);
        for (size_t i = 0; i < m * 3; ++i) ((float*)mxGetData(a))[i] = (float)v;
        return a;
    }
    if (kind == 9) { mxArray* a = mxCreateDoubleMatrix(4, 3, mxREAL); for (int i = 0; i < 12; ++i) mxGetPr(a)[i] = v; return a; }
    return mxCreateDoubleScalar(v);
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

int ds_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelFitCylinders' | 'pointFitCylinders' (via_handle 0), ...) with nargs arguments after the command.  First argument: a
// bogus (null) handle, or a 4 x 3 cloud, single or double (first_kind 1) or a 4 x 2 single (first_kind 2).  The parameters:
// maxDistance, minRadius, maxRadius, refVec, maxAngle, normals, kNormals, maxCylinders, nTrials, minInliers, seed by scalar()'s kinds
// and values (eleven of each); samples_kind 0: [], 1: int32 2 x samples_cols zeros, 2: double 2 x samples_cols, 3: int32 3 x samples_cols
int ds_usage(int via_handle, int nargs, int first_kind, const int* kinds, const double* vals, int samples_kind, int samples_cols, char* err,
             int errlen) {
    mxArray* lhs[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const float q[12] = {0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mxArray* first;
    if (via_handle) first = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    else first = first_kind == 1 ? mxCreateDoubleMatrix(4, 3, mxREAL) : first_kind == 2 ? smat(q, 4, 2) : smat(q, 4, 3);
    std::vector<mxArray*> rhs{mxCreateString(via_handle ? "modelFitCylinders" : "pointFitCylinders"), first};
    for (int i = 0; i < 11; ++i) rhs.push_back(scalar(kinds[i], vals[i]));
    rhs.push_back(samples_kind == 1   ? mxCreateNumericMatrix(2, (size_t)samples_cols, mxINT32_CLASS, mxREAL)
                  : samples_kind == 2 ? mxCreateDoubleMatrix(2, (size_t)samples_cols, mxREAL)
                  : samples_kind == 3 ? mxCreateNumericMatrix(3, (size_t)samples_cols, mxINT32_CLASS, mxREAL)
                                      : mxCreateDoubleMatrix(0, 0, mxREAL));
    rhs.push_back(mxCreateDoubleScalar(1.0));
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(7, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// via_handle: h = modelCreate(model); [labels (, cylinders (, extents (, counts (, rmse (, refitUsed (, diag))))))] =
// modelFitCylinders(h, t, rmin, rmax, refVec, maxAngle, normals, kNormals, P, B, minInl, seed, samples); modelDestroy(h) -- otherwise
// pointFitCylinders(model, ...) -- with nlhs outputs (1 .. 7).  ref_vec: three doubles or null; normals: M x 3 column-major floats or
// null; samples: int32 2 x (B * P), 1-based, or null.  labels: M int32; cylinders: capacity P x 7 doubles, handed back ROW-major,
// *n_cylinders rows; extents: P x 2 row-major; counts: P int32; rmse: P doubles; used: P int32; diag: P x 3 doubles row-major.
int ds_round_trip(int via_handle, const float* model, int M, float t, float rmin, float rmax, const double* ref_vec, double max_angle,
                  const float* normals, int k_normals, int P, int B, int min_inliers, double seed, const int32_t* samples, int nlhs,
                  int32_t* labels, double* cylinders, double* extents, int32_t* counts, double* rmse, int32_t* used, double* diag,
                  int* n_cylinders, int* n_out, char* err, int errlen) {
    mxArray* lhs[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    mxArray* h = nullptr;
    int rc;
    auto params = [&](std::vector<mxArray*>& rhs) {
        rhs.push_back(scalar(2, t)); rhs.push_back(scalar(2, rmin)); rhs.push_back(scalar(2, rmax));
        if (ref_vec) { mxArray* a = mxCreateDoubleMatrix(1, 3, mxREAL); for (int i = 0; i < 3; ++i) mxGetPr(a)[i] = ref_vec[i]; rhs.push_back(a); }
        else rhs.push_back(mxCreateDoubleMatrix(0, 0, mxREAL));
        rhs.push_back(mxCreateDoubleScalar(max_angle));
        rhs.push_back(normals ? smat(normals, (size_t)M, 3) : mxCreateDoubleMatrix(0, 0, mxREAL));
        rhs.push_back(mxCreateDoubleScalar((double)k_normals));
        rhs.push_back(mxCreateDoubleScalar((double)P)); rhs.push_back(mxCreateDoubleScalar((double)B));
        rhs.push_back(mxCreateDoubleScalar((double)min_inliers)); rhs.push_back(mxCreateDoubleScalar(seed));
        rhs.push_back(samples_arg(samples, 2, (size_t)P * (size_t)B));
    };
    if (via_handle) {
        { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
        h = lhs[0]; lhs[0] = nullptr;
        std::vector<mxArray*> rhs{mxCreateString("modelFitCylinders"), mxDuplicateArray(h)};
        params(rhs);
        rc = call(nlhs, lhs, rhs, err, errlen);
    } else {
        std::vector<mxArray*> rhs{mxCreateString("pointFitCylinders"), smat(model, M, 3)};
        params(rhs);
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && lhs[0]->cls == mxINT32_CLASS && mxGetM(lhs[0]) == (size_t)M && mxGetN(lhs[0]) == 1 && *n_out == nlhs;
        const size_t n = nlhs > 1 && lhs[1] ? mxGetM(lhs[1]) : 0;
        if (ok && nlhs > 1) ok = mxIsDouble(lhs[1]) && n <= (size_t)P && mxGetN(lhs[1]) == 7;
        if (ok && nlhs > 2) ok = mxIsDouble(lhs[2]) && mxGetM(lhs[2]) == n && mxGetN(lhs[2]) == 2;
        if (ok && nlhs > 3) ok = lhs[3]->cls == mxINT32_CLASS && mxGetM(lhs[3]) == n && mxGetN(lhs[3]) == 1;
        if (ok && nlhs > 4) ok = mxIsDouble(lhs[4]) && mxGetM(lhs[4]) == n && mxGetN(lhs[4]) == 1;
        if (ok && nlhs > 5) ok = lhs[5]->cls == mxINT32_CLASS && mxGetM(lhs[5]) == n && mxGetN(lhs[5]) == 1;
        if (ok && nlhs > 6) ok = mxIsDouble(lhs[6]) && mxGetM(lhs[6]) == (size_t)P && mxGetN(lhs[6]) == 3;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else {
            *n_cylinders = (int)n;
            if (M > 0) memcpy(labels, mxGetData(lhs[0]), (size_t)M * 4);
            for (size_t i = 0; i < n; ++i) {
                if (nlhs > 1) for (int c = 0; c < 7; ++c) cylinders[i * 7 + c] = mxGetPr(lhs[1])[i + (size_t)c * n];
                if (nlhs > 2) for (int c = 0; c < 2; ++c) extents[i * 2 + c] = mxGetPr(lhs[2])[i + (size_t)c * n];
                if (nlhs > 3) counts[i] = ((const int32_t*)mxGetData(lhs[3]))[i];
                if (nlhs > 4) rmse[i] = mxGetPr(lhs[4])[i];
                if (nlhs > 5) used[i] = ((const int32_t*)mxGetData(lhs[5]))[i];
            }
            if (nlhs > 6) for (int i = 0; i < P; ++i) for (int c = 0; c < 3; ++c) diag[i * 3 + c] = mxGetPr(lhs[6])[(size_t)i + (size_t)c * (size_t)P];
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    if (h) { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
