// pnx_varpro_prior_args.hpp -- the host half of pnx_curvefit_varpro_prior_em_f64 that needs no device: the checks of its arguments
// in front of any device work (the four of an EM by the grid EM's rule, then the variable-projection posterior's, shared) and the
// sizing of the EM kernels' LDS slab.  The normalised start (grid_prior_start), the stopping rule (grid_prior_converged) and the
// report of a call (grid_prior_report) are pnx_grid_prior_args.hpp's, called as they stand.  Free of HIP types, like
// pnx_varpro_posterior_args.hpp: pnx_api.hip and pnx_varpro_prior.hip use it, tests/host_stub/varpro_prior_args_stub.cpp builds the
// same code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_prior_args.hpp"
#include "pnx_varpro_posterior_args.hpp"

namespace pnx {

constexpr int kVarproPriorWaves = 4;  // waves of a block of the EM kernels: one wave-private row of weight sums each

// The four arguments of the EM first (prior_em_check_args, each refusal names its argument), then varpro_posterior_check_args with
// log_prior_out in the place of `mean`: the posterior's refusals (through it varpro_check_args's), atom and prior rules hold
// unchanged.  H->log_prior_norm normalises the start.
inline int varpro_prior_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                   const double *nl_atoms, const double *fixed, const double *lo, const double *hi, const double *log_prior,
                                   double noise_sd, int marginal_amplitudes, int n_iter, double pseudo_count, double rel_tol,
                                   const double *log_prior_out, int mem, VarproLayout *L, VarproPosteriorHost *H) {
    if (int rc = prior_em_check_args("varpro prior", n_iter, pseudo_count, rel_tol, log_prior_out)) return rc;
    return varpro_posterior_check_args(o, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, log_prior_out,
                                       mem, L, H);
}

// rows of a slab behind the variable projection's constants: the per-atom log-weight and the wave-private rows of the accumulate
// pass, which take the place of the posterior's k + 1 centred non-linear rows
inline int varpro_prior_extra_rows() { return 1 + kVarproPriorWaves; }

// The LDS image of a slab in both passes of the EM: the variable projection's (k blocks of [kpad][stride], varpro_const_rows(k)
// rows of constants), then varpro_prior_extra_rows() rows, each `width` wide.  width and stride follow grid_slab's rule.  Five extra
// rows against the posterior's k + 2: the same slab at three compartments, one row more at two and two rows more at one -- where
// that crosses a step of the rule the slab is 16 atoms narrower (two compartments at 32 b-values: 80 against 96).
inline GridSlab varpro_prior_slab(int n_b, int k) {
    GridSlab s;
    const int rows = varpro_const_rows(k) + varpro_prior_extra_rows();
    s.kpad = (n_b + 3) & ~3;
    s.width = 16;
    for (int w = 16; w <= 256; w += 16) {
        const int stride = (w & 16) ? w : w + 16;
        if (k * s.kpad * stride + rows * w <= 8192) s.width = w;
    }
    s.stride = (s.width & 16) ? s.width : s.width + 16;
    s.lds_doubles = k * s.kpad * s.stride + rows * s.width;
    return s;
}
}  // namespace pnx
