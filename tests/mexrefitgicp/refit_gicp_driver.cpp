// tests/mexrefitgicp/refit_gicp_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelRefitGicp' command of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own): modelCreate, modelRefitGicp, modelDestroy as
// matlab/refitGicpModel.m drives them, the outputs handed back through a plain C interface for tests/test_mex_refit_gicp.py.
// Returns 0, or 1 with the raised id:message.
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

// normals of kind 0: [], 1: 2 x 3 double, 2: 2 x 2 single, 3: 2 x 3 single
static mxArray* nmat(int kind) {
    const float q[6] = {0, 0, 1, 1, 0, 0};
    return kind == 1 ? mxCreateDoubleMatrix(2, 3, mxREAL) : kind == 2 ? smat(q, 2, 2) : kind == 3 ? smat(q, 2, 3) : smat(q, 0, 0);
}

extern "C" {

int gd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelRefitGicp', ...) with nargs arguments after the command: a bogus (null) handle, a 2 x 3 single or double cloud
// (pts_double), T: 4 x 4 x 2 double or 3 x 4 double (t_kind 1), maxDist r, steps, normals and ptsNormals of kinds n_kind and q_kind
// (nmat), k and epsilon
int gd_usage(int nargs, int pts_double, int t_kind, int n_kind, int q_kind, double r, double steps, double k, double epsilon, char* err, int errlen) {
    mxArray* lhs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    mxArray* h = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    const float q[6] = {0, 0, 0, 1, 1, 1};
    const double T[32] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mxArray* ta = t_kind == 1 ? mxCreateDoubleMatrix(3, 4, mxREAL) : tmat(T, 2);
    std::vector<mxArray*> rhs{mxCreateString("modelRefitGicp"), h, pts_double ? mxCreateDoubleMatrix(2, 3, mxREAL) : smat(q, 2, 3), ta,
                              mxCreateDoubleScalar(r), mxCreateDoubleScalar(steps), nmat(n_kind), nmat(q_kind), mxCreateDoubleScalar(k),
                              mxCreateDoubleScalar(epsilon), mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(5, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// h = modelCreate(model); [Tout (, nClose, sumD2, nPairs, sumRes2)] = modelRefitGicp(h, pts, T, maxDist, steps, normals | [], ptsNormals |
// [], k, epsilon) with nlhs outputs (1 or 5); modelDestroy(h).  normals: n_rows x 3 column-major, or null for []; qnormals: q_rows x 3,
// or null for [].  T_out: B x 16 doubles, page b the column-major 4 x 4 x B layout.  *n_out: the outputs set.
int gd_round_trip(const float* model, int M, const float* pts, int Q, const double* T, int B, double max_dist, int steps, const float* normals,
                  int n_rows, const float* qnormals, int q_rows, int k, double epsilon, int nlhs, double* T_out, int32_t* n_close, double* sum_d2,
                  int32_t* n_pairs, double* sum_res2, int* n_out, char* err, int errlen) {
    mxArray* lhs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
    mxArray* h = lhs[0]; lhs[0] = nullptr;
    int rc;
    {
        std::vector<mxArray*> rhs{mxCreateString("modelRefitGicp"), mxDuplicateArray(h), smat(pts, Q, 3), tmat(T, B), mxCreateDoubleScalar(max_dist),
                                  mxCreateDoubleScalar((double)steps), normals ? smat(normals, n_rows, 3) : smat(nullptr, 0, 0),
                                  qnormals ? smat(qnormals, q_rows, 3) : smat(nullptr, 0, 0), mxCreateDoubleScalar((double)k),
                                  mxCreateDoubleScalar(epsilon)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && mxIsDouble(lhs[0]) && (B == 0 || mxGetM(lhs[0]) == 4) && mxGetN(lhs[0]) == (size_t)4 * B && *n_out == nlhs;
        if (ok && nlhs == 5) {
            ok = mxIsInt32(lhs[1]) && mxIsDouble(lhs[2]) && mxIsInt32(lhs[3]) && mxIsDouble(lhs[4]);
            for (int i = 1; ok && i < 5; ++i) ok = mxGetM(lhs[i]) == (size_t)B && mxGetN(lhs[i]) == 1;
        }
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else if (B > 0) {
            memcpy(T_out, mxGetData(lhs[0]), (size_t)B * 16 * 8);
            if (nlhs == 5) {
                memcpy(n_close, mxGetData(lhs[1]), (size_t)B * 4); memcpy(sum_d2, mxGetData(lhs[2]), (size_t)B * 8);
                memcpy(n_pairs, mxGetData(lhs[3]), (size_t)B * 4); memcpy(sum_res2, mxGetData(lhs[4]), (size_t)B * 8);
            }
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
