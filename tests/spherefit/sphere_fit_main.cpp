// tests/spherefit/sphere_fit_main.cpp -- pcreg_amd/csrc/sphere_fit.hpp on the host, for tests/test_sphere_fit_host.py.
// usage: sphere_fit_main IN OUT.  IN holds records of 20 doubles: N6 (xx xy xz yy yz zz), h (3), S1 (3), sum w, n, p0 (3), back,
// min_radius, max_radius (the last two exactly representable floats).  OUT gets a record of 5 doubles per input record: 1 or 0 (the
// refit used or not), then the centre and R, which are 0.0 when it is not used.
#include <cstdio>
#include <vector>

#include "sphere_fit.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<double> rec;
    double buf[20];
    while (std::fread(buf, sizeof(double), 20, in) == 20) rec.insert(rec.end(), buf, buf + 20);
    std::fclose(in);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (std::size_t r = 0; r < rec.size() / 20; ++r) {
        const double* v = &rec[r * 20];
        const double N6[6] = {v[0], v[1], v[2], v[3], v[4], v[5]}, h[3] = {v[6], v[7], v[8]}, S1[3] = {v[9], v[10], v[11]};
        const double p0[3] = {v[14], v[15], v[16]};
        double centre[3] = {0.0, 0.0, 0.0}, R = 0.0, res[5];
        const bool ok = pcreg::fit_spheres_solve(N6, h, S1, v[12], v[13], p0, v[17], (float)v[18], (float)v[19], centre, R);
        res[0] = ok ? 1.0 : 0.0;
        for (int e = 0; e < 3; ++e) res[1 + e] = ok ? centre[e] : 0.0;
        res[4] = ok ? R : 0.0;
        if (std::fwrite(res, sizeof(double), 5, out) != 5) { std::fclose(out); return 3; }
    }
    return std::fclose(out) == 0 ? 0 : 3;
}
