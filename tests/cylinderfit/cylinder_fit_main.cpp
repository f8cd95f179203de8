// tests/cylinderfit/cylinder_fit_main.cpp -- pcreg_amd/csrc/cylinder_fit.hpp on the host, for tests/test_cylinder_fit_host.py.
// usage: cylinder_fit_main IN OUT.  IN holds records of 26 doubles: A6 (xx xy xz yy yz zz), n_n, use_ref (0 or 1), ref (3),
// N3 (xx xy yy), h (2), S1 (2), sum w2, n, p0 (3), back, min_radius, max_radius (the last two exactly representable floats).
// OUT gets a record of 15 doubles per input record: 1 or 0 (the basis found or not), w, u, v (0.0 when it is not), 1 or 0 (the
// refit used or not), then the centre and R, which are 0.0 when it is not used.  The circle step runs only with a basis, on the
// record's N3 .. n as they are.
#include <cstdio>
#include <vector>

#include "cylinder_fit.hpp"

int main(int argc, char** argv) {
    constexpr int kIn = 26, kOut = 15;
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<double> rec;
    double buf[kIn];
    while (std::fread(buf, sizeof(double), kIn, in) == kIn) rec.insert(rec.end(), buf, buf + kIn);
    std::fclose(in);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (std::size_t r = 0; r < rec.size() / kIn; ++r) {
        const double* x = &rec[r * kIn];
        const double A6[6] = {x[0], x[1], x[2], x[3], x[4], x[5]};
        const double N3[3] = {x[11], x[12], x[13]}, h[2] = {x[14], x[15]}, S1[2] = {x[16], x[17]}, p0[3] = {x[20], x[21], x[22]};
        double w[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0}, centre[3] = {0.0, 0.0, 0.0}, R = 0.0, res[kOut];
        const bool basis = pcreg::fit_cylinders_basis(A6, (long long)x[6], x[7] != 0.0, x[8], x[9], x[10], w, u, v);
        const bool used = basis && pcreg::fit_cylinders_circle(N3, h, S1, x[18], x[19], p0, u, v, x[23], (float)x[24], (float)x[25], centre, R);
        res[0] = basis ? 1.0 : 0.0;
        for (int e = 0; e < 3; ++e) { res[1 + e] = w[e]; res[4 + e] = u[e]; res[7 + e] = v[e]; }
        res[10] = used ? 1.0 : 0.0;
        for (int e = 0; e < 3; ++e) res[11 + e] = used ? centre[e] : 0.0;
        res[14] = used ? R : 0.0;
        if (std::fwrite(res, sizeof(double), kOut, out) != kOut) { std::fclose(out); return 3; }
    }
    return std::fclose(out) == 0 ? 0 : 3;
}
