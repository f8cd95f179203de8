// tests/mexscore/score_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelScore' command of mex/pcreg_mex.cpp (built
// with tests/mexstub/mex.h into a library of its own): modelCreate, modelScore, modelDestroy as matlab/scoreTransformsModel.m drives
// them, the outputs handed back through a plain C interface for tests/test_mex_score.py.  Returns 0, or 1 with the raised id:message.
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

int sd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelScore', ...) with nargs arguments after the command: a bogus (null) handle, a 2 x 3 single or double cloud
// (pts_double), T: 4 x 4 x 2 double, 3 x 4 double (t_kind 1) or 4 x 4 x 2 single (t_kind 2), and maxDist: a double scalar or an
// int32 scalar (r_kind 1)
int sd_usage(int nargs, int pts_double, int t_kind, int r_kind, double r, char* err, int errlen) {
    mxArray* lhs[4] = {nullptr, nullptr, nullptr, nullptr};
    mxArray* h = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    const float q[6] = {0, 0, 0, 1, 1, 1};
    const double T[32] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mxArray* ta = t_kind == 1 ? mxCreateDoubleMatrix(3, 4, mxREAL) : t_kind == 2 ? mxCreateNumericMatrix(4, 8, mxSINGLE_CLASS, mxREAL) : tmat(T, 2);
    mxArray* ra;
    if (r_kind == 1) { ra = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(ra) = (int32_t)r; }
    else ra = mxCreateDoubleScalar(r);
    std::vector<mxArray*> rhs{mxCreateString("modelScore"), h, pts_double ? mxCreateDoubleMatrix(2, 3, mxREAL) : smat(q, 2, 3), ta, ra,
                              mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(4, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// h = modelCreate(model); [nClose, sumD2 (, idx, D2)] = modelScore(h, pts, T, maxDist) with nlhs outputs (2 or 4); modelDestroy(h).
// n_close: B int32; sum_d2: B doubles; idx / d2: Q x B column-major (nlhs 4 only).  *n_out: the outputs the gateway set.
int sd_round_trip(const float* model, int M, const float* pts, int Q, const double* T, int B, double max_dist, int nlhs, int32_t* n_close,
                  double* sum_d2, int32_t* idx, float* d2, int* n_out, char* err, int errlen) {
    mxArray* lhs[4] = {nullptr, nullptr, nullptr, nullptr};
    { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
    mxArray* h = lhs[0]; lhs[0] = nullptr;
    int rc;
    {
        std::vector<mxArray*> rhs{mxCreateString("modelScore"), mxDuplicateArray(h), smat(pts, Q, 3), tmat(T, B), mxCreateDoubleScalar(max_dist)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && lhs[1] && mxIsInt32(lhs[0]) && mxIsDouble(lhs[1]) && mxGetM(lhs[0]) == (size_t)B && mxGetN(lhs[0]) == 1 &&
                  mxGetM(lhs[1]) == (size_t)B && mxGetN(lhs[1]) == 1 && *n_out == nlhs;
        if (ok && nlhs == 4)
            ok = mxIsInt32(lhs[2]) && mxIsSingle(lhs[3]) && mxGetM(lhs[2]) == (size_t)Q && mxGetN(lhs[2]) == (size_t)B && mxGetM(lhs[3]) == (size_t)Q &&
                 mxGetN(lhs[3]) == (size_t)B;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else {
            if (B > 0) { memcpy(n_close, mxGetData(lhs[0]), (size_t)B * 4); memcpy(sum_d2, mxGetData(lhs[1]), (size_t)B * 8); }
            if (nlhs == 4 && (size_t)Q * B > 0) { memcpy(idx, mxGetData(lhs[2]), (size_t)Q * B * 4); memcpy(d2, mxGetData(lhs[3]), (size_t)Q * B * 4); }
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
