// pcreg_amd/csrc/compose.hpp -- one entry of T * S for two 4 x 4 transforms in the library's layout (MATLAB's column-major storage,
// entry (r, c) at r + 4 c), its one definition: ((T(r,0) S(0,c) + T(r,1) S(1,c)) + T(r,2) S(2,c)) + T(r,3) S(3,c), nothing fused.
// refit_step.hpp's step_compose forms T_out = T_in * T_step from it, and so does fgr_pair.hpp's fgr_compose.  Plain C++ on the host,
// device code under hipcc; no HIP header, no project header.  Compile with -ffp-contract=off, as the library is.
#pragma once

#if !defined(PCREG_HD)
#if defined(__HIPCC__)
#define PCREG_HD __host__ __device__
#else
#define PCREG_HD
#endif
#endif

namespace pcreg {

PCREG_HD inline double compose_entry(const double* T, const double* S, int r, int c) {
    return ((T[r] * S[4 * c] + T[r + 4] * S[1 + 4 * c]) + T[r + 8] * S[2 + 4 * c]) + T[r + 12] * S[3 + 4 * c];
}

}  // namespace pcreg
