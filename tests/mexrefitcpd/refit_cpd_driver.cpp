// tests/mexrefitcpd/refit_cpd_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelRefitCpd' command of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own): modelCreate, modelRefitCpd, modelDestroy as
// matlab/refitCpdModel.m drives them, the outputs handed back through a plain C interface for tests/test_mex_cpd.py.
// Returns 0, or 1 with the raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0) memcpy(mxGetData(a), p, m * n * 4);
    return a;
}
static mxArray* dcol(const double* p, size_t n) {
    mxArray* a = mxCreateDoubleMatrix(n, 1, mxREAL);
    if (n > 0) memcpy(mxGetData(a), p, n * 8);
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

int cd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelRefitCpd', ...) with nargs arguments after the command: a bogus (null) handle, a 2 x 3 single or double cloud
// (pts_double), T: 4 x 4 x 2 double or 3 x 4 double (t_kind 1), sigma2 with n_sigma entries (1, 2 or anything else; single when
// sigma_single), outlier, steps
int cd_usage(int nargs, int pts_double, int t_kind, int n_sigma, int sigma_single, double sigma2, double outlier, double steps, char* err, int errlen) {
    mxArray* lhs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    mxArray* h = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    const float q[6] = {0, 0, 0, 1, 1, 1};
    const double T[32] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double sg[4] = {sigma2, sigma2, sigma2, sigma2};
    mxArray* ta = t_kind == 1 ? mxCreateDoubleMatrix(3, 4, mxREAL) : tmat(T, 2);
    mxArray* sa = sigma_single ? smat(q, 1, 1) : dcol(sg, (size_t)n_sigma);
    std::vector<mxArray*> rhs{mxCreateString("modelRefitCpd"), h, pts_double ? mxCreateDoubleMatrix(2, 3, mxREAL) : smat(q, 2, 3), ta, sa,
                              mxCreateDoubleScalar(outlier), mxCreateDoubleScalar(steps), mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(6, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// h = modelCreate(model); [Tout (, sigma2Out, Np, sumRes2, sumD2, nLive)] = modelRefitCpd(h, pts, T, sigma2, outlier, steps) with nlhs
// outputs (1 or 6); modelDestroy(h).  sigma2: n_sigma doubles (1 or B).  T_out: B x 16 doubles, page b the column-major 4 x 4 x B
// layout; dbl: 4 B doubles (sigma2Out, Np, sumRes2, sumD2).  *n_out: the outputs set.
int cd_round_trip(const float* model, int M, const float* pts, int Q, const double* T, int B, const double* sigma2, int n_sigma, double outlier,
                  int steps, int nlhs, double* T_out, double* dbl, int32_t* n_live, int* n_out, char* err, int errlen) {
    mxArray* lhs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
    mxArray* h = lhs[0]; lhs[0] = nullptr;
    int rc;
    {
        std::vector<mxArray*> rhs{mxCreateString("modelRefitCpd"), mxDuplicateArray(h), smat(pts, Q, 3), tmat(T, B), dcol(sigma2, (size_t)n_sigma),
                                  mxCreateDoubleScalar(outlier), mxCreateDoubleScalar((double)steps)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && mxIsDouble(lhs[0]) && (B == 0 || mxGetM(lhs[0]) == 4) && mxGetN(lhs[0]) == (size_t)4 * B && *n_out == nlhs;
        if (ok && nlhs == 6) {
            ok = mxIsInt32(lhs[5]);
            for (int i = 1; ok && i < 5; ++i) ok = mxIsDouble(lhs[i]);
            for (int i = 1; ok && i < 6; ++i) ok = mxGetM(lhs[i]) == (size_t)B && mxGetN(lhs[i]) == 1;
        }
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else if (B > 0) {
            memcpy(T_out, mxGetData(lhs[0]), (size_t)B * 16 * 8);
            if (nlhs == 6) {
                for (int i = 0; i < 4; ++i) memcpy(dbl + (size_t)i * B, mxGetData(lhs[1 + i]), (size_t)B * 8);
                memcpy(n_live, mxGetData(lhs[5]), (size_t)B * 4);
            }
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
