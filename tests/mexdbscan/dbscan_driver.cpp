// tests/mexdbscan/dbscan_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelDbscan' and 'dbscanPoints' commands of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as matlab/dbscanModel.m and matlab/dbscanFast.m
// drive them; the outputs are handed back through a plain C interface.  Returns 0, or 1 with the raised id:message.
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

// a scalar argument: a double (kind 0), an int32 (kind 1) or a 1 x 2 double (kind 2)
static mxArray* scalar(int kind, double v) {
    mxArray* a;
    if (kind == 1) { a = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(a) = (int32_t)v; }
    else if (kind == 2) { a = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetPr(a)[0] = mxGetPr(a)[1] = v; }
    else a = mxCreateDoubleScalar(v);
    return a;
}

extern "C" {

int dd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelDbscan' | 'dbscanPoints', ...) with nargs arguments after the command: a bogus (null) handle or a 2 x 3 single
// (first_double: a double) cloud, epsilon and minpts each of the kind given (see scalar)
int dd_usage(int via_handle, int nargs, int first_double, int r_kind, double r, int k_kind, double minpts, char* err, int errlen) {
    mxArray* lhs[4] = {nullptr, nullptr, nullptr, nullptr};
    const float q[6] = {0, 0, 0, 1, 1, 1};
    mxArray* first = first_double ? mxCreateDoubleMatrix(2, 3, mxREAL) : via_handle ? mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL) : smat(q, 2, 3);
    std::vector<mxArray*> rhs{mxCreateString(via_handle ? "modelDbscan" : "dbscanPoints"), first, scalar(r_kind, r), scalar(k_kind, minpts),
                              mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(4, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// via_handle: h = modelCreate(pts); [label, core, clOff, members] = modelDbscan(h, r, minpts); modelDestroy(h); else
// dbscanPoints(pts, r, minpts).  label: M int32; core: M bytes; cl_off: *n_clusters + 1 int32 (room for M + 1); members: *n_members
// int32 (room for M)
int dd_round_trip(int via_handle, const float* pts, int M, double r, double minpts, int32_t* label, uint8_t* core, int32_t* cl_off,
                  int* n_clusters, int32_t* members, int* n_members, char* err, int errlen) {
    mxArray* lhs[4] = {nullptr, nullptr, nullptr, nullptr};
    mxArray* h = nullptr;
    int rc;
    if (via_handle) {
        { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(pts, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
        h = lhs[0]; lhs[0] = nullptr;
        std::vector<mxArray*> rhs{mxCreateString("modelDbscan"), mxDuplicateArray(h), mxCreateDoubleScalar(r), mxCreateDoubleScalar(minpts)};
        rc = call(4, lhs, rhs, err, errlen);
    } else {
        std::vector<mxArray*> rhs{mxCreateString("dbscanPoints"), smat(pts, M, 3), mxCreateDoubleScalar(r), mxCreateDoubleScalar(minpts)};
        rc = call(4, lhs, rhs, err, errlen);
    }
    if (!rc) {
        const size_t n = mxGetM(lhs[2]), nm = mxGetM(lhs[3]);
        if (mxGetM(lhs[0]) != (size_t)M || mxGetN(lhs[0]) != 1 || mxGetM(lhs[1]) != (size_t)M || mxGetN(lhs[1]) != 1 || n < 1 || n > (size_t)M + 1 ||
            mxGetN(lhs[2]) != 1 || nm > (size_t)M || mxGetN(lhs[3]) != 1 || !mxIsInt32(lhs[0]) || !mxIsUint8(lhs[1]) || !mxIsInt32(lhs[2]) ||
            !mxIsInt32(lhs[3])) {
            snprintf(err, errlen, "driver: unexpected output shapes or classes");
            rc = 1;
        } else {
            *n_clusters = (int)n - 1;
            *n_members = (int)nm;
            if (M > 0) { memcpy(label, mxGetData(lhs[0]), (size_t)M * 4); memcpy(core, mxGetData(lhs[1]), (size_t)M); }
            if (nm > 0) memcpy(members, mxGetData(lhs[3]), nm * 4);
            memcpy(cl_off, mxGetData(lhs[2]), n * 4);
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    if (h) { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
