// tests/fgrpair/fgr_pair_main.cpp -- pcreg_amd/csrc/fgr_pair.hpp and plane_fit.hpp on the host, for tests/test_fgr_ref.py.
// usage: fgr_pair_main IN OUT.  IN holds 21 doubles (T in the library's layout, o, mu, the number of pairs n) and n records of 6
// doubles (pts1 row, pts2 row).  OUT gets the 28 sums of the pairs added one after the other, 1 or 0 (a fit or empty), T_step and
// T * T_step (16 doubles each, zeros when empty), then per pair its liveness, rr and weight, and last the verdicts of fgr_triple_ok
// on the pairs (0, 1, 2), (1, 2, 3), ... at tuple_scale = 0.95, and fgr_mu_next(mu, 1.4, 1.0).
#include <cstdio>
#include <vector>

#include "fgr_pair.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    double head[21];
    if (std::fread(head, sizeof(double), 21, in) != 21) { std::fclose(in); return 2; }
    const int n = (int)head[20];
    std::vector<double> rows((std::size_t)n * 6);
    if (std::fread(rows.data(), sizeof(double), rows.size(), in) != rows.size()) { std::fclose(in); return 2; }
    std::fclose(in);
    double T[16], o[3] = {head[16], head[17], head[18]}, acc[27], last = 0.0;
    const double mu = head[19];
    for (int e = 0; e < 16; ++e) T[e] = head[e];
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    std::vector<double> out;
    std::vector<double> per;
    for (int i = 0; i < n; ++i) {
        double p[6], q[3], r[3];
        for (int e = 0; e < 6; ++e) p[e] = rows[(std::size_t)i * 6 + e];
        const bool live = pcreg::fgr_live(p);
        const double rr = pcreg::fgr_rr(T, p, q, r);
        per.push_back(live ? 1.0 : 0.0); per.push_back(rr); per.push_back(pcreg::fgr_weight(mu, rr));
        if (live) pcreg::fgr_pair_add(T, p, o, mu, acc, last);
    }
    double sums[pcreg::kPlaneSums], S[16], Tn[16];
    for (int k = 0; k < 27; ++k) sums[k] = acc[k];
    sums[27] = last;
    for (int e = 0; e < 16; ++e) { S[e] = 0.0; Tn[e] = 0.0; }
    const bool ok = pcreg::plane_fit(sums, 3 * n, o, S);
    if (ok) pcreg::fgr_compose(T, S, Tn);
    out.insert(out.end(), sums, sums + pcreg::kPlaneSums);
    out.push_back(ok ? 1.0 : 0.0);
    out.insert(out.end(), S, S + 16);
    out.insert(out.end(), Tn, Tn + 16);
    out.insert(out.end(), per.begin(), per.end());
    for (int i = 0; i + 2 < n; ++i) {
        double a[6], b[6], c[6];
        for (int e = 0; e < 6; ++e) { a[e] = rows[(std::size_t)i * 6 + e]; b[e] = rows[(std::size_t)(i + 1) * 6 + e]; c[e] = rows[(std::size_t)(i + 2) * 6 + e]; }
        out.push_back(pcreg::fgr_triple_ok(a, b, c, 0.95 * 0.95) ? 1.0 : 0.0);
    }
    out.push_back(pcreg::fgr_mu_next(mu, 1.4, 1.0));
    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { std::fclose(f); return 3; }
    return std::fclose(f) == 0 ? 0 : 3;
}
