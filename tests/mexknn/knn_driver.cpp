// tests/mexknn/knn_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelKnn' command of mex/pcreg_mex.cpp (built with
// tests/mexstub/mex.h into a library of its own): modelCreate, modelKnn, modelDestroy as matlab/knnsearchModel.m drives them, the
// outputs handed back through a plain C interface for tests/test_knn_k_abi.py.  Returns 0, or 1 with the raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0) memcpy(mxGetData(a), p, m * n * 4);
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

int kd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelKnn', ...) with nargs arguments after the command: a bogus handle, a Q x 3 single (Q = 2) or double query
// (as_double), and k
int kd_usage(int nargs, int as_double, double k, char* err, int errlen) {
    mxArray* lhs[2] = {nullptr, nullptr};
    mxArray* h = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    const float q[6] = {0, 0, 0, 1, 1, 1};
    std::vector<mxArray*> rhs{mxCreateString("modelKnn"), h, as_double ? mxCreateDoubleMatrix(2, 3, mxREAL) : smat(q, 2, 3),
                              mxCreateDoubleScalar(k)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(2, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// h = modelCreate(model); [idx, D2] = modelKnn(h, Y, k); modelDestroy(h).  idx: Q x k int32 column-major, D2: Q x k single
int kd_round_trip(const float* model, int M, const float* Y, int Q, int k, int32_t* idx, float* d2, char* err, int errlen) {
    mxArray* lhs[2] = {nullptr, nullptr};
    { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
    mxArray* h = lhs[0]; lhs[0] = nullptr;
    int rc;
    {
        std::vector<mxArray*> rhs{mxCreateString("modelKnn"), mxDuplicateArray(h), smat(Y, Q, 3), mxCreateDoubleScalar(k)};
        rc = call(2, lhs, rhs, err, errlen);
    }
    if (!rc) {
        if (mxGetM(lhs[0]) != (size_t)Q || mxGetN(lhs[0]) != (size_t)k || mxGetM(lhs[1]) != (size_t)Q || mxGetN(lhs[1]) != (size_t)k ||
            !mxIsInt32(lhs[0]) || !mxIsSingle(lhs[1])) {
            snprintf(err, errlen, "driver: unexpected output shapes or classes");
            rc = 1;
        } else if (Q > 0) {
            memcpy(idx, mxGetData(lhs[0]), (size_t)Q * k * 4);
            memcpy(d2, mxGetData(lhs[1]), (size_t)Q * k * 4);
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
