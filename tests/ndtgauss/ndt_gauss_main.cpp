// tests/ndtgauss/ndt_gauss_main.cpp -- pcreg_amd/csrc/ndt_gauss.hpp on the host, for tests/test_ndt_gauss_host.py.
// usage: ndt_gauss_main IN OUT.  IN holds records of 1 + 3 * 64 floats: the member count (a whole number, 2 .. 64), then the members'
// x y z in ascending row order (the rest of the record is ignored).  OUT gets a record of 10 doubles per input record: 1 or 0 (a
// Gaussian or void), the mean's three coordinates, then C's six entries, which are 0.0 when void.
#include <cstdio>
#include <vector>

#include "ndt_gauss.hpp"

int main(int argc, char** argv) {
    constexpr int kMax = 64, kRec = 1 + 3 * kMax;
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<float> rec;
    float buf[kRec];
    while (std::fread(buf, sizeof(float), kRec, in) == (std::size_t)kRec) rec.insert(rec.end(), buf, buf + kRec);
    std::fclose(in);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (std::size_t r = 0; r < rec.size() / kRec; ++r) {
        const float* p = rec.data() + r * kRec;
        const int count = (int)p[0];
        if (count < 2 || count > kMax) { std::fprintf(stderr, "record %zu: count %d\n", r, count); std::fclose(out); return 2; }
        double mean[3] = {0.0, 0.0, 0.0}, C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, res[10];
        const bool ok = pcreg::ndt_gauss(count, [p](int i, float& x, float& y, float& z) { x = p[1 + 3 * i]; y = p[2 + 3 * i]; z = p[3 + 3 * i]; },
                                         mean, C);
        res[0] = ok ? 1.0 : 0.0;
        for (int e = 0; e < 3; ++e) res[1 + e] = mean[e];
        for (int e = 0; e < 6; ++e) res[4 + e] = ok ? C[e] : 0.0;
        if (std::fwrite(res, sizeof(double), 10, out) != 10) { std::fclose(out); return 3; }
    }
    return std::fclose(out) == 0 ? 0 : 3;
}
