// pnx_varpro_posterior_args.hpp -- the host half of pnx_curvefit_varpro_posterior_f64 that needs no device: the checks of its
// arguments in front of any device work (the variable projection's, then log_prior, noise_sd and marginal_amplitudes), the
// normaliser of the prior, the per-row centres of the moment accumulation, the amplitude bound A of the cancellation floor and the
// sizing of the kernel's LDS slab.  Free of HIP types, like pnx_varpro_args.hpp: pnx_api.hip and pnx_varpro_posterior.hip use it,
// tests/host_stub/varpro_posterior_args_stub.cpp builds the same code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_posterior_args.hpp"
#include "pnx_varpro_args.hpp"

namespace pnx {

// What the host derives from the arguments once per call, beside the VarproLayout.
struct VarproPosteriorHost {
    double log_prior_norm = 0.0;         // log sum_g exp(log_prior_g): log(n_atoms) for the uniform prior
    double centre[PNX_MAX_PARAMS] = {};  // per free parameter: mid-range of the admissible atoms; 0 for a linear row
    double amp_l1 = 0.0;                 // A: the largest ||a'||_1 the class's clip rule can return for the call's box
};

// A per class (include/pnx.h), with F = sum_{j<K} max(|lo_fj|, |hi_fj|) + max(|1 - sum_{j<K} lo_fj|, |1 - sum_{j<K} hi_fj|):
//   free (mono, full)  sum_j max(|lo_j|, |hi_j|);   reduced  F;   S0  hi_S0 F   (lo_S0 >= 0 is checked, so |S| <= hi_S0)
inline double varpro_amp_l1(const VarproLayout &L) {
    auto big = [](double a, double b) { return std::fabs(a) > std::fabs(b) ? std::fabs(a) : std::fabs(b); };
    if (L.cls == kVarproFree) {
        double s = 0.0;
        for (int j = 0; j < L.k; ++j) s += big(L.lin_lo[j], L.lin_hi[j]);
        return s;
    }
    double f = 0.0, slo = 0.0, shi = 0.0;
    for (int j = 0; j < L.k - 1; ++j) {
        f += big(L.lin_lo[j], L.lin_hi[j]);
        slo += L.lin_lo[j];
        shi += L.lin_hi[j];
    }
    f += big(1.0 - slo, 1.0 - shi);
    return L.cls == kVarproS0 ? L.lin_hi[L.k - 1] * f : f;
}

// varpro_check_args (the refusals and the atom / bounds checks of the variable projection, unchanged; there is no fallback, so lo
// stands in for it), then the three new inputs.  Every refusal names its argument.  `mean` takes the place of p_out.
inline int varpro_posterior_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                       const double *nl_atoms, const double *fixed, const double *lo, const double *hi, const double *log_prior,
                                       double noise_sd, int marginal_amplitudes, const double *mean, int mem, VarproLayout *L,
                                       VarproPosteriorHost *H) {
    if (!mean) return set_error(PNX_ERR_INVALID, "varpro posterior: mean is NULL (the one output that is not optional)");
    if (!(noise_sd >= 0.0) || std::isinf(noise_sd))
        return set_error(PNX_ERR_INVALID, "varpro posterior: noise_sd=%g must be finite and > 0 (known noise) or 0 (marginalised)", noise_sd);
    if (marginal_amplitudes != 0 && marginal_amplitudes != 1)
        return set_error(PNX_ERR_INVALID, "varpro posterior: marginal_amplitudes=%d (0: profile weight, 1: the amplitudes are marginalised)",
                         marginal_amplitudes);
    if (lo && hi)
        for (int r = 0; r < o->n_free; ++r)
            if (!(lo[r] <= hi[r])) return set_error(PNX_ERR_INVALID, "varpro posterior: free parameter %d has lo=%g > hi=%g", r, lo[r], hi[r]);
    if (int rc = varpro_check_args(o, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, lo, mean, mem, L)) return rc;
    if (int rc = posterior_check_log_prior("varpro posterior", n_atoms, log_prior, &H->log_prior_norm)) return rc;
    // centres of the non-linear rows: min + (max - min) / 2 over the admissible atoms, exact when they all hold one value
    for (int r = 0; r < o->n_free; ++r) {
        H->centre[r] = 0.0;
        if (L->row_src[r] < 0) continue;
        double mn = HUGE_VAL, mx = -HUGE_VAL;
        for (int g = 0; g < n_atoms; ++g) {
            if (log_prior && log_prior[g] == -HUGE_VAL) continue;
            const double a = nl_atoms[(size_t)L->row_src[r] * n_atoms + g];
            mn = a < mn ? a : mn;
            mx = a > mx ? a : mx;
        }
        H->centre[r] = mn + 0.5 * (mx - mn);
    }
    H->amp_l1 = varpro_amp_l1(*L);
    return PNX_OK;
}

// rows of a slab behind the variable projection's constants: the per-atom log-weight and the k + 1 centred non-linear values a
// layout can have free (k rates and T1)
inline int varpro_posterior_extra_rows(int k) { return 1 + k + 1; }

// The posterior kernel's LDS image of a slab: the variable projection's (k blocks of [kpad][stride], varpro_const_rows(k) rows of
// constants), then varpro_posterior_extra_rows(k) rows, each `width` wide.  width and stride follow grid_slab's rule.
inline GridSlab varpro_posterior_slab(int n_b, int k) {
    GridSlab s;
    const int rows = varpro_const_rows(k) + varpro_posterior_extra_rows(k);
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
