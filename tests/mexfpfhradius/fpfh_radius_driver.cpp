// tests/mexfpfhradius/fpfh_radius_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'modelFpfhRadius' and 'pointFpfhRadius'
// commands of mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own), as matlab/extractFPFHRadiusModel.m and
// matlab/extractFPFHRadiusFast.m drive them; the outputs are handed back through a plain C interface for
// tests/test_mex_fpfh_radius.py.  Returns 0, or 1 with the raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0 && p) memcpy(mxGetData(a), p, m * n * 4);
    return a;
}
static mxArray* sscalar(float v) { return smat(&v, 1, 1); }
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

int frd_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('modelFpfhRadius' | 'pointFpfhRadius' (via_handle 0), ...) with nargs arguments after the command.  First argument: a
// bogus (null) handle, or a 4 x 3 cloud, single or double (first_kind 1) or a 4 x 2 single (first_kind 2); r2: a single scalar, a
// double scalar with r_kind 1; maxNeighbors and kNormals: double scalars, maxNeighbors an int32 scalar with n_kind 1; normals: []
// (nrm_kind 0), single 4 x 3 (1), double 4 x 3 (2), single 4 x 2 (3), single 5 x 3 (4); viewpoint: [] (v_kind 0), a double 1 x 3
// (1), a double 1 x 2 (2) or a single 1 x 3 (3)
int frd_usage(int via_handle, int nargs, int first_kind, int r_kind, double r2, int n_kind, double n, int nrm_kind, double kn, int v_kind,
              char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    const float q[15] = {0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0};
    mxArray* first;
    if (via_handle) first = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    else first = first_kind == 1 ? mxCreateDoubleMatrix(4, 3, mxREAL) : first_kind == 2 ? smat(q, 4, 2) : smat(q, 4, 3);
    mxArray* ra = r_kind == 1 ? mxCreateDoubleScalar(r2) : sscalar((float)r2);
    mxArray* na;
    if (n_kind == 1) { na = mxCreateNumericMatrix(1, 1, mxINT32_CLASS, mxREAL); *(int32_t*)mxGetData(na) = (int32_t)n; }
    else na = mxCreateDoubleScalar(n);
    mxArray* nrm = nrm_kind == 0 ? smat(nullptr, 0, 0) : nrm_kind == 1 ? smat(q, 4, 3) : nrm_kind == 2 ? mxCreateDoubleMatrix(4, 3, mxREAL)
                 : nrm_kind == 3 ? smat(q, 4, 2) : smat(q, 5, 3);
    const double v3[3] = {0, 0, 10};
    mxArray* va = v_kind == 0 ? vmat(nullptr) : v_kind == 1 ? vmat(v3) : v_kind == 2 ? mxCreateDoubleMatrix(1, 2, mxREAL)
                                                                                    : mxCreateNumericMatrix(1, 3, mxSINGLE_CLASS, mxREAL);
    std::vector<mxArray*> rhs{mxCreateString(via_handle ? "modelFpfhRadius" : "pointFpfhRadius"), first, ra, na, nrm, mxCreateDoubleScalar(kn), va,
                              mxCreateDoubleScalar(1.0)};
    while ((int)rhs.size() > nargs + 1) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    int rc = call(3, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// via_handle: h = modelCreate(model); [features (, spfh (, nNeighbors))] = modelFpfhRadius(h, r2, maxNeighbors, normals, kNormals,
// viewpoint); modelDestroy(h) -- otherwise pointFpfhRadius(model, ...) -- with nlhs outputs (1 .. 3).  normals: M x 3 column-major
// floats, or null for [].  features: M x 33 column-major doubles; spfh: M x 33 column-major uint32; n_neighbors: M int32.
int frd_round_trip(int via_handle, const float* model, int M, float r2, int max_neighbors, const float* normals, int kn, const double* vp, int nlhs,
                   double* features, uint32_t* spfh, int32_t* n_neighbors, int* n_out, char* err, int errlen) {
    mxArray* lhs[3] = {nullptr, nullptr, nullptr};
    mxArray* h = nullptr;
    int rc;
    mxArray* na = normals ? smat(normals, M, 3) : smat(nullptr, 0, 0);
    if (via_handle) {
        { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) { mxDestroyArray(na); return 1; } }
        h = lhs[0]; lhs[0] = nullptr;
        std::vector<mxArray*> rhs{mxCreateString("modelFpfhRadius"), mxDuplicateArray(h), sscalar(r2), mxCreateDoubleScalar((double)max_neighbors), na,
                                  mxCreateDoubleScalar((double)kn), vmat(vp)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    } else {
        std::vector<mxArray*> rhs{mxCreateString("pointFpfhRadius"), smat(model, M, 3), sscalar(r2), mxCreateDoubleScalar((double)max_neighbors), na,
                                  mxCreateDoubleScalar((double)kn), vmat(vp)};
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (mxArray* a : lhs) *n_out += a != nullptr;
        bool ok = lhs[0] && mxIsDouble(lhs[0]) && mxGetM(lhs[0]) == (size_t)M && mxGetN(lhs[0]) == 33 && *n_out == nlhs;
        if (ok && nlhs >= 2) ok = lhs[1]->cls == mxUINT32_CLASS && mxGetM(lhs[1]) == (size_t)M && mxGetN(lhs[1]) == 33;
        if (ok && nlhs >= 3) ok = mxIsInt32(lhs[2]) && mxGetM(lhs[2]) == (size_t)M && mxGetN(lhs[2]) == 1;
        if (!ok) { snprintf(err, errlen, "driver: unexpected outputs, shapes or classes"); rc = 1; }
        else if (M > 0) {
            memcpy(features, mxGetData(lhs[0]), (size_t)M * 33 * 8);
            if (nlhs >= 2) memcpy(spfh, mxGetData(lhs[1]), (size_t)M * 33 * 4);
            if (nlhs >= 3) memcpy(n_neighbors, mxGetData(lhs[2]), (size_t)M * 4);
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    if (h) { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
