// tests/mexcluster/cluster_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelCluster' and 'clusterPoints' commands of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as matlab/clusterPointsModel.m and
// matlab/clusterPointsFast.m drive them; the outputs are handed back through a plain C interface.  Returns 0, or 1 with the
// raised id:message.
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

int cd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelCluster' | 'clusterPoints', ...) with nargs arguments after the command: a bogus (null) handle or a 2 x 3 single
// (first_double: a double) cloud, and r: a double scalar, an int32 scalar (r_kind 1) or a 1 x 2 double (r_kind 2)
int cd_usage(int via_handle, int nargs, int first_double, int r_kind, double r, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    const float q[6] = {0, 0, 0, 1, 1, 1};
    mxArray* first = first_double ? mxCreateDoubleMatrix(2, 3, mxREAL) : via_handle ? mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL) : smat(q, 2, 3);
    mxArray* ra;
    if (r_kind == 1) { ra = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(ra) = (int32_t)r; }
    else if (r_kind == 2) { ra = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetPr(ra)[0] = mxGetPr(ra)[1] = r; }
    else ra = mxCreateDoubleScalar(r);
    std::vector<mxArray*> rhs{mxCreateString(via_handle ? "modelCluster" : "clusterPoints"), first, ra, mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(3, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// via_handle: h = modelCreate(pts); [label, clOff, members] = modelCluster(h, r); modelDestroy(h); else clusterPoints(pts, r).
// label / members: M int32 each; cl_off: *n_clusters + 1 int32 (room for M + 1)
int cd_round_trip(int via_handle, const float* pts, int M, double r, int32_t* label, int32_t* cl_off, int* n_clusters, int32_t* members,
                  char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    mxArray* h = nullptr;
    int rc;
    if (via_handle) {
        { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(pts, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
        h = lhs[0]; lhs[0] = nullptr;
        std::vector<mxArray*> rhs{mxCreateString("modelCluster"), mxDuplicateArray(h), mxCreateDoubleScalar(r)};
        rc = call(3, lhs, rhs, err, errlen);
    } else {
        std::vector<mxArray*> rhs{mxCreateString("clusterPoints"), smat(pts, M, 3), mxCreateDoubleScalar(r)};
        rc = call(3, lhs, rhs, err, errlen);
    }
    if (!rc) {
        const size_t n = mxGetM(lhs[1]);
        if (mxGetM(lhs[0]) != (size_t)M || mxGetN(lhs[0]) != 1 || mxGetM(lhs[2]) != (size_t)M || mxGetN(lhs[2]) != 1 || n < 1 || n > (size_t)M + 1 ||
            mxGetN(lhs[1]) != 1 || !mxIsInt32(lhs[0]) || !mxIsInt32(lhs[1]) || !mxIsInt32(lhs[2])) {
            snprintf(err, errlen, "driver: unexpected output shapes or classes");
            rc = 1;
        } else {
            *n_clusters = (int)n - 1;
            if (M > 0) { memcpy(label, mxGetData(lhs[0]), (size_t)M * 4); memcpy(members, mxGetData(lhs[2]), (size_t)M * 4); }
            memcpy(cl_off, mxGetData(lhs[1]), n * 4);
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    if (h) { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
