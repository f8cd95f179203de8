// tests/mexnormals/normals_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelNormals' and 'pointNormals' commands of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as matlab/pcnormalsModel.m and matlab/pcnormalsFast.m
// drive them; the outputs are handed back through a plain C interface for tests/test_mex_normals.py.  Returns 0, or 1 with the
// raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0) memcpy(mxGetData(a), p, m * n * 4);
    return a;
}
// the viewpoint argument: [] (vp null) or a double 1 x 3
static mxArray* vmat(const double* vp) {
    mxArray* a = mxCreateDoubleMatrix(vp ? 1 : 0, vp ? 3 : 0, mxREAL);
    if (vp) memcpy(mxGetPr(a), vp, 3 * 8);
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

// pcreg_mex('modelNormals' | 'pointNormals' (via_handle 0), ...) with nargs arguments after the command.  First argument: a bogus
// (null) handle, or a 4 x 3 cloud, single or double (first_kind 1) or a 4 x 2 single (first_kind 2); k: a double scalar or an int32
// scalar (k_kind 1); viewpoint: [] (v_kind 0), a double 1 x 3 (1), a double 1 x 2 (2) or a single 1 x 3 (3)
int nd_usage(int via_handle, int nargs, int first_kind, int k_kind, double k, int v_kind, char* err, int errlen) {
    mxArray* lhs[2] = {nullptr, nullptr};
    const float q[12] = {0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    mxArray* first;
    if (via_handle) first = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    else first = first_kind == 1 ? mxCreateDoubleMatrix(4, 3, mxREAL) : first_kind == 2 ? smat(q, 4, 2) : smat(q, 4, 3);
    mxArray* ka;
    if (k_kind == 1) { ka = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(ka) = (int32_t)k; }
    else ka = mxCreateDoubleScalar(k);
    const double v3[3] = {0, 0, 10};
    mxArray* va = v_kind == 0 ? vmat(nullptr) : v_kind == 1 ? vmat(v3) : v_kind == 2 ? mxCreateDoubleMatrix(1, 2, mxREAL)
                                                                                    : mxCreateNumericMatrix(1, 3, mxSINGLE_CLASS, mxREAL);
    std::vector<mxArray*> rhs{mxCreateString(via_handle ? "modelNormals" : "pointNormals"), first, ka, va, mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(2, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// via_handle: h = modelCreate(model); [normals (, variation)] = modelNormals(h, k, viewpoint); modelDestroy(h) -- otherwise
// pointNormals(model, k, viewpoint) -- with nlhs outputs (1 or 2).  normals: M x 3 column-major floats; variation: M floats.
int nd_round_trip(int via_handle, const float* model, int M, int k, const double* vp, int nlhs, float* normals, float* variation, int* n_out,
                  char* err, int errlen) {
    mxArray* lhs[2] = {nullptr, nullptr};
    mxArray* h = nullptr;
    int rc;
    if (via_handle) {
        { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
        h = lhs[0]; lhs[0] = nullptr;
        std::vector<mxArray*> rhs{mxCreateString("modelNormals"), mxDuplicateArray(h), mxCreateDoubleScalar((double)k), vmat(vp)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    } else {
        std::vector<mxArray*> rhs{mxCreateString("pointNormals"), smat(model, M, 3), mxCreateDoubleScalar((double)k), vmat(vp)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && mxIsSingle(lhs[0]) && mxGetM(lhs[0]) == (size_t)M && mxGetN(lhs[0]) == 3 && *n_out == nlhs;
        if (ok && nlhs == 2) ok = mxIsSingle(lhs[1]) && mxGetM(lhs[1]) == (size_t)M && mxGetN(lhs[1]) == 1;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else if (M > 0) {
            memcpy(normals, mxGetData(lhs[0]), (size_t)M * 3 * 4);
            if (nlhs == 2) memcpy(variation, mxGetData(lhs[1]), (size_t)M * 4);
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    if (h) { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
