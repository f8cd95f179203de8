// tests/planefit/plane_fit_main.cpp -- pcreg_amd/csrc/plane_fit.hpp on the host, for tests/test_plane_fit_host.py.
// usage: plane_fit_main IN OUT.  IN holds records of 32 doubles: the 28 sums, n_plane (a whole number), the origin's three
// coordinates.  OUT gets a record of 17 doubles per input record: 1 or 0 (a fit or empty), then the 16 numbers of T_step, which
// are 0.0 when empty -- the form the library reports.
#include <cstdio>
#include <vector>

#include "plane_fit.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<double> rec;
    double buf[32];
    while (std::fread(buf, sizeof(double), 32, in) == 32) rec.insert(rec.end(), buf, buf + 32);
    std::fclose(in);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (std::size_t r = 0; r < rec.size() / 32; ++r) {
        double sums[pcreg::kPlaneSums], T[16], res[17];
        for (int k = 0; k < pcreg::kPlaneSums; ++k) sums[k] = rec[r * 32 + k];
        const double o[3] = {rec[r * 32 + 29], rec[r * 32 + 30], rec[r * 32 + 31]};
        for (int e = 0; e < 16; ++e) T[e] = 0.0;
        const bool ok = pcreg::plane_fit(sums, (int)rec[r * 32 + 28], o, T);
        res[0] = ok ? 1.0 : 0.0;
        for (int e = 0; e < 16; ++e) res[1 + e] = ok ? T[e] : 0.0;
        if (std::fwrite(res, sizeof(double), 17, out) != 17) { std::fclose(out); return 3; }
    }
    return std::fclose(out) == 0 ? 0 : 3;
}
