// tests/infopair/info_pair_main.cpp -- pcreg_amd/csrc/info_pair.hpp on the host, for tests/test_info_pair_host.py.
// usage: info_pair_main IN OUT.  IN holds records of 40 doubles: C (xx xy xz yy yz zz), x, u, e and the 27 sums before the pair.
// OUT gets a record of 62 doubles per input record: the weighted instantiation's 27 sums, y and qq, then the unweighted one's.
#include <cstdio>
#include <vector>

#include "info_pair.hpp"

template <bool kWeighted>
static void run(const double* p, double* res) {
    const double C[6] = {p[0], p[1], p[2], p[3], p[4], p[5]}, x[3] = {p[6], p[7], p[8]}, u[3] = {p[9], p[10], p[11]};
    double acc[27], y[3], qq;
    for (int k = 0; k < 27; ++k) acc[k] = p[13 + k];
    pcreg::info_pair<kWeighted>(C, x, u, p[12], acc, y, qq);
    for (int k = 0; k < 27; ++k) res[k] = acc[k];
    for (int k = 0; k < 3; ++k) res[27 + k] = y[k];
    res[30] = qq;
}

int main(int argc, char** argv) {
    constexpr int kRec = 40, kOut = 62;
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
        double res[kOut];
        run<true>(rec.data() + r * kRec, res);
        run<false>(rec.data() + r * kRec, res + 31);
        if (std::fwrite(res, sizeof(double), kOut, out) != (std::size_t)kOut) { std::fclose(out); return 3; }
    }
    return std::fclose(out) == 0 ? 0 : 3;
}
