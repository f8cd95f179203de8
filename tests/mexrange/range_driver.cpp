// tests/mexrange/range_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelRange' command of mex/pcreg_mex.cpp (built
// with tests/mexstub/mex.h into a library of its own): modelCreate, modelRange, modelDestroy as matlab/rangesearchModel.m drives
// them, the outputs handed back through a plain C interface for tests/test_range_abi.py.  Returns 0, or 1 with the raised id:message.
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

int rd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelRange', ...) with nargs arguments after the command: a bogus (null) handle, a Q x 3 single (Q = 2) or double
// query (q_double), and r: a double scalar, an int32 scalar (r_kind 1) or a 1 x 2 double (r_kind 2)
int rd_usage(int nargs, int q_double, int r_kind, double r, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    mxArray* h = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    const float q[6] = {0, 0, 0, 1, 1, 1};
    mxArray* ra;
    if (r_kind == 1) { ra = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(ra) = (int32_t)r; }
    else if (r_kind == 2) { ra = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetPr(ra)[0] = mxGetPr(ra)[1] = r; }
    else ra = mxCreateDoubleScalar(r);
    std::vector<mxArray*> rhs{mxCreateString("modelRange"), h, q_double ? mxCreateDoubleMatrix(2, 3, mxREAL) : smat(q, 2, 3), ra, mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(3, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// h = modelCreate(model); [counts, idx, D2] = modelRange(h, Y, r); modelDestroy(h).  counts: Q int32; *total: the rows returned;
// idx / d2: the first min(total, cap) of them
int rd_round_trip(const float* model, int M, const float* Y, int Q, double r, int32_t* counts, long long* total, long long cap, int32_t* idx,
                  float* d2, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
    mxArray* h = lhs[0]; lhs[0] = nullptr;
    int rc;
    {
        std::vector<mxArray*> rhs{mxCreateString("modelRange"), mxDuplicateArray(h), smat(Y, Q, 3), mxCreateDoubleScalar(r)};
        rc = call(3, lhs, rhs, err, errlen);
    }
    if (!rc) {
        const size_t n = mxGetM(lhs[1]);
        if (mxGetM(lhs[0]) != (size_t)Q || mxGetN(lhs[0]) != 1 || mxGetN(lhs[1]) != 1 || mxGetM(lhs[2]) != n || mxGetN(lhs[2]) != 1 ||
            !mxIsInt32(lhs[0]) || !mxIsInt32(lhs[1]) || !mxIsSingle(lhs[2])) {
            snprintf(err, errlen, "driver: unexpected output shapes or classes");
            rc = 1;
        } else {
            *total = (long long)n;
            const size_t keep = n < (size_t)cap ? n : (size_t)cap;
            if (Q > 0) memcpy(counts, mxGetData(lhs[0]), (size_t)Q * 4);
            if (keep > 0) { memcpy(idx, mxGetData(lhs[1]), keep * 4); memcpy(d2, mxGetData(lhs[2]), keep * 4); }
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
