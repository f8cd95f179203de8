// tests/mexunique/unique_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'uniqueRows3' and 'aggregateMatches' commands of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as matlab/uniqueRowsFast.m and
// matlab/aggregateMatches.m drive them; the outputs are handed back through a plain C interface.  Returns 0, or 1 with the raised
// id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* dmat(const double* p, size_t m, size_t n) {
    mxArray* a = mxCreateDoubleMatrix(m, n, mxREAL);
    if (m * n > 0 && p) memcpy(mxGetData(a), p, m * n * 8);
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

int ud_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('uniqueRows3' | 'aggregateMatches', ...) with nargs arguments after the command: n x cols matrices (first_single: the
// first one a single; rows2: the rows of the second one), filled with `fill`
int ud_usage(int aggregate, int nargs, int first_single, int n, int cols, int rows2, double fill, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    mxArray* a = first_single ? mxCreateNumericMatrix(n, cols, mxSINGLE_CLASS, mxREAL) : mxCreateDoubleMatrix(n, cols, mxREAL);
    if (!first_single) for (size_t k = 0; k < (size_t)n * cols; ++k) mxGetPr(a)[k] = fill;
    mxArray* b = mxCreateDoubleMatrix(rows2, cols, mxREAL);
    std::vector<mxArray*> rhs{mxCreateString(aggregate ? "aggregateMatches" : "uniqueRows3"), a, b, mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(aggregate ? 3 : 1, lhs, rhs, err, errlen);
    for (mxArray* x : lhs) mxDestroyArray(x);
    return rc;
}

// aggregate == 0: ia = uniqueRows3(A); else [o1, o2, ia] = aggregateMatches(A, B).  ia: room for n doubles, o1 / o2 for 3 n
int ud_round_trip(int aggregate, const double* A, const double* B, int n, double* ia, int* n_out, double* o1, double* o2, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    int rc;
    if (aggregate) { std::vector<mxArray*> rhs{mxCreateString("aggregateMatches"), dmat(A, n, 3), dmat(B, n, 3)}; rc = call(3, lhs, rhs, err, errlen); }
    else { std::vector<mxArray*> rhs{mxCreateString("uniqueRows3"), dmat(A, n, 3)}; rc = call(1, lhs, rhs, err, errlen); }
    if (!rc) {
        const mxArray* li = lhs[aggregate ? 2 : 0];
        const size_t u = mxGetM(li);
        if (!mxIsDouble(li) || u > (size_t)n || (aggregate && (mxGetM(lhs[0]) != u || mxGetN(lhs[0]) != 3 || mxGetM(lhs[1]) != u || mxGetN(lhs[1]) != 3))) {
            snprintf(err, errlen, "driver: unexpected output shapes or classes");
            rc = 1;
        } else {
            *n_out = (int)u;
            if (u > 0) memcpy(ia, mxGetPr(li), u * 8);
            if (aggregate && u > 0) { memcpy(o1, mxGetPr(lhs[0]), 3 * u * 8); memcpy(o2, mxGetPr(lhs[1]), 3 * u * 8); }
        }
    }
    for (mxArray*& x : lhs) { mxDestroyArray(x); x = nullptr; }
    return rc;
}

}  // extern "C"
