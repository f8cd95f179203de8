// tests/mexndt/ndt_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'ndtCreate', 'ndtRefit' and 'ndtDestroy' commands of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as matlab/ndtModel.m and matlab/refitNdtModel.m drive
// them, the outputs handed back through a plain C interface for tests/test_mex_ndt.py.  Returns 0, or 1 with the raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0) memcpy(mxGetData(a), p, m * n * 4);
    return a;
}
// B transforms, 16 doubles each, as MATLAB's 4 x 4 x B
static mxArray* tmat(const double* T, int B) {
    const mwSize dims[3] = {4, 4, (mwSize)B};
    mxArray* a = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    if (B > 0) memcpy(mxGetData(a), T, (size_t)B * 16 * 8);
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

int nd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('ndtCreate', ...) with nargs arguments after the command: a 2 x 3 single or double cloud (pts_double), step, minPoints
int nd_create_usage(int nargs, int pts_double, double step, double min_points, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    const float q[6] = {0, 0, 0, 1, 1, 1};
    std::vector<mxArray*> rhs{mxCreateString("ndtCreate"), pts_double ? mxCreateDoubleMatrix(2, 3, mxREAL) : smat(q, 2, 3), mxCreateDoubleScalar(step),
                              mxCreateDoubleScalar(min_points), mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(3, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// pcreg_mex('ndtRefit', ...) with nargs arguments after the command: a bogus (null) handle, a 2 x 3 single or double cloud, T: 4 x 4 x 2
// double or 3 x 4 double (t_kind 1), neighbors, outlierRatio, steps; and pcreg_mex('ndtDestroy') without a handle (nargs < 0)
int nd_refit_usage(int nargs, int pts_double, int t_kind, double neighbors, double ratio, double steps, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    if (nargs < 0) {
        std::vector<mxArray*> rhs{mxCreateString("ndtDestroy")};
        return call(0, lhs, rhs, err, errlen);
    }
    mxArray* h = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    const float q[6] = {0, 0, 0, 1, 1, 1};
    const double T[32] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<mxArray*> rhs{mxCreateString("ndtRefit"), h, pts_double ? mxCreateDoubleMatrix(2, 3, mxREAL) : smat(q, 2, 3),
                              t_kind == 1 ? mxCreateDoubleMatrix(3, 4, mxREAL) : tmat(T, 2), mxCreateDoubleScalar(neighbors), mxCreateDoubleScalar(ratio),
                              mxCreateDoubleScalar(steps), mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(3, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// [h, nVoxels, nGaussians] = ndtCreate(model, step, minPoints); [Tout (, nPairs, sumE)] = ndtRefit(h, pts, T, neighbors, ratio, steps)
// with nlhs outputs (1 or 3); ndtDestroy(h).  T_out: B x 16 doubles, page b the column-major 4 x 4 x B layout.  sizes: nVoxels,
// nGaussians.  *n_out: the outputs of ndtRefit that were set.
int nd_round_trip(const float* model, int M, double step, int min_points, const float* pts, int Q, const double* T, int B, int neighbors, double ratio,
                  int steps, int nlhs, int* sizes, double* T_out, int32_t* n_pairs, double* sum_e, int* n_out, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    {
        std::vector<mxArray*> rhs{mxCreateString("ndtCreate"), smat(model, M, 3), mxCreateDoubleScalar(step), mxCreateDoubleScalar((double)min_points)};
        if (call(3, lhs, rhs, err, errlen)) return 1;
    }
    mxArray* h = lhs[0]; lhs[0] = nullptr;
    sizes[0] = (int)mxGetScalar(lhs[1]); sizes[1] = (int)mxGetScalar(lhs[2]);
    mxDestroyArray(lhs[1]); mxDestroyArray(lhs[2]); lhs[1] = lhs[2] = nullptr;
    int rc;
    {
        std::vector<mxArray*> rhs{mxCreateString("ndtRefit"), mxDuplicateArray(h), smat(pts, Q, 3), tmat(T, B), mxCreateDoubleScalar((double)neighbors),
                                  mxCreateDoubleScalar(ratio), mxCreateDoubleScalar((double)steps)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && mxIsDouble(lhs[0]) && (B == 0 || mxGetM(lhs[0]) == 4) && mxGetN(lhs[0]) == (size_t)4 * B && *n_out == nlhs;
        if (ok && nlhs == 3) ok = mxIsInt32(lhs[1]) && mxIsDouble(lhs[2]) && mxGetM(lhs[1]) == (size_t)B && mxGetN(lhs[1]) == 1 && mxGetM(lhs[2]) == (size_t)B &&
                                  mxGetN(lhs[2]) == 1;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else if (B > 0) {
            memcpy(T_out, mxGetData(lhs[0]), (size_t)B * 16 * 8);
            if (nlhs == 3) { memcpy(n_pairs, mxGetData(lhs[1]), (size_t)B * 4); memcpy(sum_e, mxGetData(lhs[2]), (size_t)B * 8); }
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    { std::vector<mxArray*> rhs{mxCreateString("ndtDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
