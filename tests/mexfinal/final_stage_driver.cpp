// tests/mexfinal/final_stage_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the 'finalStageLimits' / 'finalStage' commands of
// mex/pcreg_mex.cpp (built with tests/mexstub/mex.h into a library of its own): builds the mxArrays matlab/finalStage.m passes and
// hands the outputs back through a plain C interface for tests/test_mex_final_stage.py.  Returns 0, or 1 with the raised id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* dmat(const double* p, size_t m, size_t n) { mxArray* a = mxCreateDoubleMatrix(m, n, mxREAL); if (m * n > 0) memcpy(mxGetPr(a), p, m * n * 8); return a; }
static void put(mxArray* s, const char* k, double v) { mxSetField(s, 0, k, mxCreateDoubleScalar(v)); }

static int call(int nlhs, mxArray** plhs, std::vector<mxArray*>& rhs, char* err, int errlen) {
    int rc = 0;
    try { mexFunction(nlhs, plhs, (int)rhs.size(), const_cast<const mxArray**>(rhs.data())); }
    catch (const MexError& e) { snprintf(err, errlen, "%s: %s", e.id.c_str(), e.msg.c_str()); rc = 1; }
    for (mxArray* a : rhs) mxDestroyArray(a);
    return rc;
}

extern "C" {

int fs_live_arrays() { return g_mex_live_arrays; }

// pcreg_mex('finalStage') with too few arguments
int fs_usage(char* err, int errlen) {
    mxArray* lhs[1] = {nullptr};
    std::vector<mxArray*> rhs{mxCreateString("finalStage"), mxCreateDoubleScalar(1.0)};
    return call(1, lhs, rhs, err, errlen);
}

// limits = pcreg_mex('finalStageLimits', pts, T)   (T16: K column-major 4 x 4 back to back; limits: K x 6 column-major)
int fs_limits(const double* pts, int N, const double* T16, int K, double* limits, char* err, int errlen) {
    mxArray* lhs[1] = {nullptr};
    std::vector<mxArray*> rhs{mxCreateString("finalStageLimits"), dmat(pts, N, 3), dmat(T16, 4, 4 * (size_t)K)};
    if (call(1, lhs, rhs, err, errlen)) return 1;
    memcpy(limits, mxGetPr(lhs[0]), (size_t)K * 6 * 8);
    mxDestroyArray(lhs[0]);
    return 0;
}

// descCreate, ONE finalStage, descDestroy.  desc6: min_pts, max_pts, R, thVar(1), thVar(2), k; par7 as the shim's other drivers
// (Metric SAD).  Outputs as the command returns them: counts as doubles, best 1-based, T_refine (*t_empty = 1 for []), pts_final
// N x 3, pairs P x 2 column-major (capacity kp_off[K] rows), *P.
int fs_round_trip(const double* descM, int VM, int D, const double* featM, const double* pts, int N, const double* locs, int K, const double* T16,
                  const double* kp, const int32_t* kp_off, const double* desc6, const double* par7, double R_desc, double maxDist, double* nk,
                  double* nd, double* nm, double* nc, double* prec, double* best, double* T_refine, int* t_empty, double* pts_final,
                  uint32_t* pairs_colmajor, int* P, char* err, int errlen) {
    mxArray* lhs[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    { std::vector<mxArray*> rhs{mxCreateString("descCreate"), dmat(descM, VM, D)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
    mxArray* hM = lhs[0]; lhs[0] = nullptr;
    mxArray* o = mxCreateStructMatrix(1, 1, 0, nullptr);
    put(o, "min_pts", desc6[0]); put(o, "max_pts", desc6[1]); put(o, "R", desc6[2]); put(o, "k", desc6[5]); put(o, "ALIGN_POINTS", 1);
    mxSetField(o, 0, "thVar", dmat(desc6 + 3, 1, 2));
    mxArray* p = mxCreateStructMatrix(1, 1, 0, nullptr);
    mxSetField(p, 0, "Metric", mxCreateString("SAD")); mxSetField(p, 0, "Method", mxCreateString("Approximate"));
    put(p, "MatchThreshold", par7[0]); put(p, "MaxRatio", par7[1]); put(p, "Unique", par7[2]); put(p, "UNNORMALIZE", par7[3]);
    put(p, "norm_factor", par7[4]); put(p, "CHANGE_METRIC", par7[5]); put(p, "metric_factor", par7[6]); put(p, "VERBOSE", 0);
    const int S = kp_off[K];
    mxArray* off = mxCreateNumericMatrix((size_t)K + 1, 1, mxINT32_CLASS, mxREAL);
    memcpy(mxGetData(off), kp_off, ((size_t)K + 1) * 4);
    int rc = 0;
    {
        std::vector<mxArray*> rhs{mxCreateString("finalStage"), mxDuplicateArray(hM), dmat(featM, VM, 3), dmat(pts, N, 3), dmat(locs, K, 3),
                                  dmat(T16, 4, 4 * (size_t)K), dmat(kp, S, 3), off, o, p, mxCreateDoubleScalar(R_desc), mxCreateDoubleScalar(maxDist)};
        rc = call(9, lhs, rhs, err, errlen);
    }
    if (!rc) {
        memcpy(nk, mxGetPr(lhs[0]), (size_t)K * 8); memcpy(nd, mxGetPr(lhs[1]), (size_t)K * 8);
        memcpy(nm, mxGetPr(lhs[2]), (size_t)K * 8); memcpy(nc, mxGetPr(lhs[3]), (size_t)K * 8);
        memcpy(prec, mxGetPr(lhs[4]), (size_t)K * 8);
        *best = mxGetScalar(lhs[5]);
        *t_empty = mxIsEmpty(lhs[6]) ? 1 : 0;
        if (!*t_empty) memcpy(T_refine, mxGetPr(lhs[6]), 128);
        memcpy(pts_final, mxGetPr(lhs[7]), (size_t)N * 3 * 8);
        *P = (int)mxGetM(lhs[8]);
        if (*P) memcpy(pairs_colmajor, mxGetData(lhs[8]), (size_t)*P * 2 * 4);
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    { std::vector<mxArray*> rhs{mxCreateString("descDestroy"), hM}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
