// tests/mexfpfh/fpfh_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelFpfh' and 'pointFpfh' commands of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as matlab/extractFPFHModel.m and
// matlab/extractFPFHFast.m drive them; the outputs are handed back through a plain C interface for tests/test_mex_fpfh.py.
// Returns 0, or 1 with the raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0 && p) memcpy(mxGetData(a), p, m * n * 4);
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

int fd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelFpfh' | 'pointFpfh' (via_handle 0), ...) with nargs arguments after the command.  First argument: a bogus (null)
// handle, or a 4 x 3 cloud, single or double (first_kind 1) or a 4 x 2 single (first_kind 2); k and kNormals: double scalars, k an
// int32 scalar with k_kind 1; normals: [] (n_kind 0), single 4 x 3 (1), double 4 x 3 (2), single 4 x 2 (3), single 5 x 3 (4);
// viewpoint: [] (v_kind 0), a double 1 x 3 (1), a double 1 x 2 (2) or a single 1 x 3 (3)
int fd_usage(int via_handle, int nargs, int first_kind, int k_kind, double k, int n_kind, double kn, int v_kind, char* err, int errlen) {
    mxArray* lhs[2] = {nullptr, nullptr};
    const float q[15] = {0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0};
    mxArray* first;
    if (via_handle) first = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    else first = first_kind == 1 ? mxCreateDoubleMatrix(4, 3, mxREAL) : first_kind == 2 ? smat(q, 4, 2) : smat(q, 4, 3);
    mxArray* ka;
    if (k_kind == 1) { ka = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(ka) = (int32_t)k; }
    else ka = mxCreateDoubleScalar(k);
    mxArray* na = n_kind == 0 ? smat(nullptr, 0, 0) : n_kind == 1 ? smat(q, 4, 3) : n_kind == 2 ? mxCreateDoubleMatrix(4, 3, mxREAL)
                : n_kind == 3 ? smat(q, 4, 2) : smat(q, 5, 3);
    const double v3[3] = {0, 0, 10};
    mxArray* va = v_kind == 0 ? vmat(nullptr) : v_kind == 1 ? vmat(v3) : v_kind == 2 ? mxCreateDoubleMatrix(1, 2, mxREAL)
                                                                                    : mxCreateNumericMatrix(1, 3, mxSINGLE_CLASS, mxREAL);
    std::vector<mxArray*> rhs{mxCreateString(via_handle ? "modelFpfh" : "pointFpfh"), first, ka, na, mxCreateDoubleScalar(kn), va, mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(2, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// via_handle: h = modelCreate(model); [features (, spfh)] = modelFpfh(h, k, normals, kNormals, viewpoint); modelDestroy(h) --
// otherwise pointFpfh(model, k, normals, kNormals, viewpoint) -- with nlhs outputs (1 or 2).  normals: M x 3 column-major floats, or
// null for [].  features: M x 33 column-major doubles; spfh: M x 33 column-major bytes.
int fd_round_trip(int via_handle, const float* model, int M, int k, const float* normals, int kn, const double* vp, int nlhs, double* features,
                  uint8_t* spfh, int* n_out, char* err, int errlen) {
    mxArray* lhs[2] = {nullptr, nullptr};
    mxArray* h = nullptr;
    int rc;
    mxArray* na = normals ? smat(normals, M, 3) : smat(nullptr, 0, 0);
    if (via_handle) {
        { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) { mxDestroyArray(na); return 1; } }
        h = lhs[0]; lhs[0] = nullptr;
        std::vector<mxArray*> rhs{mxCreateString("modelFpfh"), mxDuplicateArray(h), mxCreateDoubleScalar((double)k), na, mxCreateDoubleScalar((double)kn), vmat(vp)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    } else {
        std::vector<mxArray*> rhs{mxCreateString("pointFpfh"), smat(model, M, 3), mxCreateDoubleScalar((double)k), na, mxCreateDoubleScalar((double)kn), vmat(vp)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && mxIsDouble(lhs[0]) && mxGetM(lhs[0]) == (size_t)M && mxGetN(lhs[0]) == 33 && *n_out == nlhs;
        if (ok && nlhs == 2) ok = mxIsUint8(lhs[1]) && mxGetM(lhs[1]) == (size_t)M && mxGetN(lhs[1]) == 33;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else if (M > 0) {
            memcpy(features, mxGetData(lhs[0]), (size_t)M * 33 * 8);
            if (nlhs == 2) memcpy(spfh, mxGetData(lhs[1]), (size_t)M * 33);
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    if (h) { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
