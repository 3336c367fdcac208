// pnx_grid_rician_args.hpp -- the host half of pnx_curvefit_grid_posterior_rician_f64 and pnx_log_i0e_f64 that needs no device:
// the checks of their arguments in front of any device work.  The Rician call takes the known-noise grid posterior's arguments
// without project_amplitude, so its checks are grid_posterior_check_args' with three more refusals: a noise sd that is not a
// finite positive number (a marginalised scale has no closed form under this likelihood), per-b-value weights (opts->sigma:
// the Rice density has one sd), and -- through project_amplitude = 0 -- nothing projected.  Free of HIP types, like
// pnx_grid_posterior_args.hpp: pnx_api.hip and pnx_grid_rician.hip use it, tests/host_stub/bessel_stub.cpp builds the same
// code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_posterior_args.hpp"

namespace pnx {

inline int grid_rician_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                  const double *atoms, const double *fixed, const double *lo, const double *hi, const double *log_prior,
                                  double noise_sd, const double *mean, int mem, GridPosteriorHost *H) {
    if (!(noise_sd > 0.0) || std::isinf(noise_sd))
        return set_error(PNX_ERR_INVALID, "grid posterior (rician): noise_sd=%g must be finite and > 0 (the Rician likelihood is built for a "
                                          "known noise sd: a marginalised scale has no closed form)", noise_sd);
    if (o->sigma)
        return set_error(PNX_ERR_UNSUPPORTED, "grid posterior (rician): sigma is not built (per-b-value weights: the Rice density has one "
                                              "noise sd, noise_sd)");
    return grid_posterior_check_args(o, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, 0, log_prior, noise_sd, mean, mem, H);
}

// The Rician kernel's LDS image: the posterior kernel's slab ([kpad][stride] doubles of the dictionary, then per atom ||s||^2, a spare
// row, log_prior and the n_free centred parameter values, each `width` wide), then per wave the 16 signal rows of its strip,
// [16][ypitch] doubles.  ypitch = kpad + 2: the four rows one read of the correction loop touches (kq, pitch apart) then fall
// into different banks.  waves: 4 up to 32 b-values, 2 beyond -- the signal rows of four waves at 128 b-values alone would fill
// the 64 KB.  The slab is narrower than the Gaussian kernel's; the correction loop, not the slab traffic, is what the call costs.
struct GridRicianSlab {
    GridSlab slab;  // lds_doubles: the dictionary part only
    int waves, ypitch, lds_doubles;
};
inline GridRicianSlab grid_rician_slab(int n_b, int n_free) {
    GridRicianSlab r;
    GridSlab &s = r.slab;
    s.kpad = (n_b + 3) & ~3;
    r.waves = s.kpad <= 32 ? 4 : 2;
    r.ypitch = s.kpad + 2;
    const int ydoubles = r.waves * 16 * r.ypitch;
    s.width = 16;
    for (int w = 16; w <= 256; w += 16) {
        const int stride = (w & 16) ? w : w + 16;
        if (s.kpad * stride + (3 + n_free) * w + ydoubles <= 8192) s.width = w;
    }
    s.stride = (s.width & 16) ? s.width : s.width + 16;
    s.lds_doubles = s.kpad * s.stride + (3 + n_free) * s.width;
    r.lds_doubles = s.lds_doubles + ydoubles;
    return r;
}

inline int log_i0e_check_args(int64_t n, const double *z, const double *out, int mem) {
    if (n < 0) return set_error(PNX_ERR_INVALID, "log_i0e: n < 0");
    if (n && (!z || !out)) return set_error(PNX_ERR_INVALID, "log_i0e: NULL data pointer");
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "log_i0e: mem=%d", mem);
    return PNX_OK;
}
}  // namespace pnx
