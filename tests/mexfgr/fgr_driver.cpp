// tests/mexfgr/fgr_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'fgrBatched' command of mex/pcreg_mex.cpp (built with
// tests/mexstub/mex.h into a library of its own), as matlab/fgrBatched.m drives it; the outputs are handed back through a plain C
// interface.  Returns 0, or 1 with the raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* dmat(const double* p, size_t m, size_t n) {
    mxArray* a = mxCreateDoubleMatrix(m, n, mxREAL);
    if (m * n > 0 && p) memcpy(mxGetData(a), p, m * n * 8);
    return a;
}
static mxArray* imat(const int32_t* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxINT32_CLASS, mxREAL);
    if (m * n > 0 && p) memcpy(mxGetData(a), p, m * n * 4);
    return a;
}
// opts: delta2, iterations, decrease_every, division_factor, mu0, n_tuples, tuple_scale, seed; a NaN leaves the field out
static mxArray* opts_struct(const double* o) {
    static const char* names[8] = {"delta2", "iterations", "decrease_every", "division_factor", "mu0", "n_tuples", "tuple_scale", "seed"};
    mxArray* s = mxCreateStructMatrix(1, 1, 0, nullptr);
    for (int k = 0; k < 8; ++k) if (o[k] == o[k]) mxSetField(s, 0, names[k], mxCreateDoubleScalar(o[k]));
    return s;
}

static int call(int nlhs, mxArray** plhs, std::vector<mxArray*>& rhs, char* err, int errlen) {
    int rc = 0;
    try { mexFunction(nlhs, plhs, (int)rhs.size(), const_cast<const mxArray**>(rhs.data())); }
    catch (const MexError& e) { snprintf(err, errlen, "%s: %s", e.id.c_str(), e.msg.c_str()); rc = 1; }
    for (mxArray* a : rhs) mxDestroyArray(a);
    return rc;
}

extern "C" {

int fd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('fgrBatched', ...) with nargs arguments after the command, built to be refused.  kind: 0 well-formed (total = 8 rows, B = 2),
// 1 single points, 2 double offsets, 3 opts no struct, 4 offsets that end short of the rows, 5 a two-column cloud, 6 a tupleIdx of
// the wrong size, 7 a double tupleIdx, 8 a T0 of the wrong size, 9 pts2 with fewer rows
int fd_usage(int nargs, int kind, const double* o, char* err, int errlen) {
    mxArray* lhs[4] = {nullptr, nullptr, nullptr, nullptr};
    const int32_t off[3] = {0, 3, kind == 4 ? 7 : 8};
    const double offd[3] = {0, 3, 8};
    const size_t nt = o[5] == o[5] && o[5] > 0 ? (size_t)o[5] : 0;
    std::vector<mxArray*> rhs{mxCreateString("fgrBatched"),
                              kind == 1 ? mxCreateNumericMatrix(8, 3, mxSINGLE_CLASS, mxREAL) : mxCreateDoubleMatrix(8, kind == 5 ? 2 : 3, mxREAL),
                              mxCreateDoubleMatrix(kind == 9 ? 7 : 8, 3, mxREAL), kind == 2 ? dmat(offd, 3, 1) : imat(off, 3, 1),
                              kind == 3 ? mxCreateDoubleScalar(1.0) : opts_struct(o),
                              kind == 7 ? mxCreateDoubleMatrix(3, nt * 2, mxREAL) : imat(nullptr, 3, kind == 6 ? nt * 2 + 1 : nt * 2),
                              mxCreateDoubleMatrix(4, kind == 8 ? 4 : 8, mxREAL), mxCreateDoubleScalar(0.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(4, lhs, rhs, err, errlen);
    for (mxArray* x : lhs) mxDestroyArray(x);
    return rc;
}

// [T, inlierIdx, stats, kept] = pcreg_mex('fgrBatched', pts1, pts2, offsets, opts[, tupleIdx, T0]) with nlhs outputs.  pts1 / pts2: total
// x 3 column-major; tab (3 x n_tuples B) and T0 (16 B) may be null.  T: room for 16 B doubles, inl for total, stats for 9 B, kept for total
int fd_round_trip(const double* p1, const double* p2, int total, const int32_t* off, int B, const double* o, const int32_t* tab, const double* T0,
                  int nlhs, double* T, double* inl, int* n_inl, double* stats, uint8_t* kept, char* err, int errlen) {
    mxArray* lhs[4] = {nullptr, nullptr, nullptr, nullptr};
    const size_t nt = o[5] == o[5] && o[5] > 0 ? (size_t)o[5] : 0;
    std::vector<mxArray*> rhs{mxCreateString("fgrBatched"), dmat(p1, total, 3), dmat(p2, total, 3), imat(off, B + 1, 1), opts_struct(o)};
    if (tab || T0) rhs.push_back(tab ? imat(tab, 3, nt * B) : mxCreateDoubleMatrix(0, 0, mxREAL));
    if (T0) rhs.push_back(dmat(T0, 4, 4 * (size_t)B));
    int rc = call(nlhs, lhs, rhs, err, errlen);
    if (!rc) {
        bool ok = mxIsDouble(lhs[0]) && mxGetM(lhs[0]) == 4 && mxGetN(lhs[0]) == 4 * (size_t)B;
        if (ok && nlhs > 1) ok = mxIsDouble(lhs[1]) && mxGetM(lhs[1]) <= (size_t)total;
        if (ok && nlhs > 2) ok = mxIsDouble(lhs[2]) && mxGetM(lhs[2]) == (size_t)B && mxGetN(lhs[2]) == (B ? 9u : 0u);
        if (ok && nlhs > 3) ok = mxIsUint8(lhs[3]) && mxGetM(lhs[3]) == (size_t)total;
        if (!ok) { snprintf(err, errlen, "driver: unexpected output shapes or classes"); rc = 1; }
        else {
            if (B > 0) memcpy(T, mxGetPr(lhs[0]), 128 * (size_t)B);
            *n_inl = nlhs > 1 ? (int)mxGetM(lhs[1]) : -1;
            if (nlhs > 1 && *n_inl > 0) memcpy(inl, mxGetPr(lhs[1]), 8 * (size_t)*n_inl);
            if (nlhs > 2 && B > 0) memcpy(stats, mxGetPr(lhs[2]), 72 * (size_t)B);
            if (nlhs > 3 && total > 0) memcpy(kept, mxGetData(lhs[3]), (size_t)total);
        }
    }
    for (mxArray*& x : lhs) { mxDestroyArray(x); x = nullptr; }
    return rc;
}

}  // extern "C"
