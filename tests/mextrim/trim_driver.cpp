// tests/mextrim/trim_driver.cpp -- TEST INFRASTRUCTURE.  Plays MATLAB for the four trimmed commands of mex/pcreg_mex.cpp (built with
// tests/mexstub/mex.h into a library of its own): modelCreate, 'modelScoreTrimmed' / 'modelRefitTrimmed' / 'modelRefitPlaneTrimmed' /
// 'modelRefitGicpTrimmed' (or, with ratio == 0, their untrimmed commands as the wrappers call them without 'InlierRatio'),
// modelDestroy; the outputs handed back through a plain C interface for tests/test_mex_trim.py.  Returns 0, or 1 with the raised
// id:message.
#include "mex.h"

int g_mex_live_arrays = 0;

static mxArray* smat(const float* p, size_t m, size_t n) {
    mxArray* a = mxCreateNumericMatrix(m, n, mxSINGLE_CLASS, mxREAL);
    if (m * n > 0) memcpy(mxGetData(a), p, m * n * 4);
    return a;
}
// B transforms, 16 doubles each, as MATLAB's 4 x 4 x B
static mxArray* tmat(const double* T, int B) {
    const mwSize dims[3] = {4, 4, (mwSize)B};
    mxArray* a = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    if (B > 0) memcpy(mxGetData(a), T, (size_t)B * 16 * 8);
    return a;
}

static int call(int nlhs, mxArray** plhs, std::vector<mxArray*>& rhs, char* err, int errlen) {
    int rc = 0;
    try { mexFunction(nlhs, plhs, (int)rhs.size(), const_cast<const mxArray**>(rhs.data())); }
    catch (const MexError& e) { snprintf(err, errlen, "%s: %s", e.id.c_str(), e.msg.c_str()); rc = 1; }
    for (mxArray* a : rhs) mxDestroyArray(a);
    return rc;
}

static const char* kTrimmed[4] = {"modelScoreTrimmed", "modelRefitTrimmed", "modelRefitPlaneTrimmed", "modelRefitGicpTrimmed"};
static const char* kPlain[4] = {"modelScore", "modelRefit", "modelRefitPlane", "modelRefitGicp"};

// the arguments behind the command: h, pts, T, maxDist (, keepRatio of the trimmed command) and the command's own tail
static std::vector<mxArray*> args(int which, bool trimmed, mxArray* h, mxArray* pts, mxArray* T, double r, double ratio, double steps, mxArray* normals,
                                  mxArray* qnormals, double k, double epsilon) {
    std::vector<mxArray*> rhs{mxCreateString(trimmed ? kTrimmed[which] : kPlain[which]), h, pts, T, mxCreateDoubleScalar(r)};
    if (trimmed) rhs.push_back(mxCreateDoubleScalar(ratio));
    if (which >= 1) rhs.push_back(mxCreateDoubleScalar(steps));
    if (which >= 2) rhs.push_back(normals); else mxDestroyArray(normals);
    if (which == 3) rhs.push_back(qnormals); else mxDestroyArray(qnormals);
    if (which >= 2) rhs.push_back(mxCreateDoubleScalar(k));
    if (which == 3) rhs.push_back(mxCreateDoubleScalar(epsilon));
    return rhs;
}

extern "C" {

int td_live_arrays() { return g_mex_live_arrays; }

// the trimmed command `which` with a bogus (null) handle, a 2 x 3 cloud, T 4 x 4 x 2, [] normals; drop: arguments left off the end;
// extra: one more argument appended; bad_ratio_class: keepRatio as a single
int td_usage(int which, double r, double ratio, double steps, int drop, int extra, int bad_ratio_class, char* err, int errlen) {
    mxArray* lhs[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const float q[6] = {0, 0, 0, 1, 1, 1};
    const double T[32] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<mxArray*> rhs = args(which, true, mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL), smat(q, 2, 3), tmat(T, 2), r, ratio, steps,
                                     smat(q, 0, 0), smat(q, 0, 0), 6.0, 1e-3);
    if (bad_ratio_class) { mxDestroyArray(rhs[5]); const float half = 0.5f; rhs[5] = smat(&half, 1, 1); }
    for (int i = 0; i < drop; ++i) { mxDestroyArray(rhs.back()); rhs.pop_back(); }
    if (extra) rhs.push_back(mxCreateDoubleScalar(1.0));
    int rc = call(7, lhs, rhs, err, errlen);
    for (mxArray* a : lhs) mxDestroyArray(a);
    return rc;
}

// h = modelCreate(model); [out{1:nlhs}] = command(h, pts, T, maxDist (, keepRatio), ...); modelDestroy(h).  ratio == 0: the untrimmed
// command.  Output j comes back as raw bytes in out[j] (room for cap bytes each) with its class in cls[j] and its size in rows[j],
// cols[j]; *n_out: the outputs set.
int td_round_trip(int which, const float* model, int M, const float* pts, int Q, const double* T, int B, double max_dist, double ratio, int steps,
                  const float* normals, int n_rows, const float* qnormals, int q_rows, int k, double epsilon, int nlhs, void** out, size_t cap,
                  int* cls, int* rows, int* cols, int* n_out, char* err, int errlen) {
    mxArray* lhs[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    { std::vector<mxArray*> rhs{mxCreateString("modelCreate"), smat(model, M, 3)}; if (call(1, lhs, rhs, err, errlen)) return 1; }
    mxArray* h = lhs[0]; lhs[0] = nullptr;
    int rc;
    {
        std::vector<mxArray*> rhs = args(which, ratio != 0.0, mxDuplicateArray(h), smat(pts, Q, 3), tmat(T, B), max_dist, ratio, (double)steps,
                                         normals ? smat(normals, n_rows, 3) : smat(nullptr, 0, 0), qnormals ? smat(qnormals, q_rows, 3) : smat(nullptr, 0, 0),
                                         (double)k, epsilon);
        rc = call(nlhs, lhs, rhs, err, errlen);
    }
    if (!rc) {
        *n_out = 0;
        for (int j = 0; j < 7; ++j) {
            mxArray* a = lhs[j];
            if (!a) continue;
            ++*n_out;
            const size_t el = mxIsDouble(a) ? 8 : 4, bytes = mxGetM(a) * mxGetN(a) * el;
            cls[j] = mxIsDouble(a) ? 0 : mxIsSingle(a) ? 1 : mxIsInt32(a) ? 2 : -1;
            rows[j] = (int)mxGetM(a); cols[j] = (int)mxGetN(a);
            if (cls[j] < 0 || bytes > cap) { snprintf(err, errlen, "driver: output %d of an unexpected class or size", j); rc = 1; }
            else if (bytes) memcpy(out[j], mxGetData(a), bytes);
        }
        for (mxArray*& a : lhs) { mxDestroyArray(a); a = nullptr; }
    }
    { std::vector<mxArray*> rhs{mxCreateString("modelDestroy"), h}; if (call(0, lhs, rhs, err, errlen)) return 1; }
    return rc;
}

}  // extern "C"
