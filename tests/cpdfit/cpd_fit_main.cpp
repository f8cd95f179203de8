// tests/cpdfit/cpd_fit_main.cpp -- pcreg_amd/csrc/cpd_fit.hpp on the host, for tests/test_cpd_ref.py.
// usage: cpd_fit_main IN OUT.  IN holds records of 22 doubles: the 19 sums of a transform and the origin o they were taken about.
// OUT gets a record of 18 doubles per input record: 1 or 0 (a fit or empty), T_step's 16 doubles in the library's layout and
// sigma2_out, all 0.0 when empty.
#include <cstdio>
#include <vector>

#include "cpd_fit.hpp"

int main(int argc, char** argv) {
    constexpr int kRec = pcreg::kCpdSums + 3;
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<double> rec;
    double buf[kRec];
    while (std::fread(buf, sizeof(double), kRec, in) == (std::size_t)kRec) rec.insert(rec.end(), buf, buf + kRec);
    std::fclose(in);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (std::size_t r = 0; r < rec.size() / kRec; ++r) {
        const double* p = rec.data() + r * kRec;
        double sums[pcreg::kCpdSums], T[16], sig = 0.0, res[18];
        for (int k = 0; k < pcreg::kCpdSums; ++k) sums[k] = p[k];
        for (int e = 0; e < 16; ++e) T[e] = 0.0;
        const double o[3] = {p[19], p[20], p[21]};
        const bool ok = pcreg::cpd_fit(sums, o, T, sig);
        res[0] = ok ? 1.0 : 0.0;
        for (int e = 0; e < 16; ++e) res[1 + e] = ok ? T[e] : 0.0;
        res[17] = ok ? sig : 0.0;
        if (std::fwrite(res, sizeof(double), 18, out) != 18) { std::fclose(out); return 3; }
    }
    return std::fclose(out) == 0 ? 0 : 3;
}
