// tests/gicppair/gicp_pair_main.cpp -- pcreg_amd/csrc/gicp_pair.hpp on the host, for tests/test_gicp_pair_host.py.
// usage: gicp_pair_main IN OUT.  IN holds records of 23 doubles: the model row's normal and the query's normal (three fp32 values
// each, stored as doubles), the transform's 16 doubles, and a = 1 - epsilon.  OUT gets a record of 7 doubles per input record: 1 or
// 0 (a plane-to-plane pair or not), then W's six entries (xx xy xz yy yz zz), which are 0.0 when it is not a pair.
#include <cstdio>
#include <vector>

#include "gicp_pair.hpp"

int main(int argc, char** argv) {
    constexpr int kRec = 23;
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
        const float n[3] = {(float)p[0], (float)p[1], (float)p[2]}, nq[3] = {(float)p[3], (float)p[4], (float)p[5]};
        double W[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, res[7];
        const bool ok = pcreg::gicp_pair(n, nq, p + 6, p[22], W);
        res[0] = ok ? 1.0 : 0.0;
        for (int e = 0; e < 6; ++e) res[1 + e] = ok ? W[e] : 0.0;
        if (std::fwrite(res, sizeof(double), 7, out) != 7) { std::fclose(out); return 3; }
    }
    return std::fclose(out) == 0 ? 0 : 3;
}
