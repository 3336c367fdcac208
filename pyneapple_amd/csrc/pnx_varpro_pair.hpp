// pnx_varpro_pair.hpp -- what the units over the variable-projection dictionary compute for ONE voxel-atom pair on the device: the
// amplitude solve with its clip rule (vp_solve) and the log-weight l_g of the pair (vp_log_weight).  One copy for
// pnx_varpro_posterior.hip (moments) and pnx_varpro_marginal.hip (marginals): the two kernels weigh a pair by the same expressions
// in the same order.
#pragma once
#include <hip/hip_runtime.h>

#include "pnx_varpro_args.hpp"

namespace pnx {

// packed index of the symmetric (i, j), as pnx_varpro.hip stores M
__host__ __device__ constexpr int vpk(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// The variable projection's amplitude solve and clip rule for one voxel-atom pair (pnx_varpro.hip varpro_match_kernel, the same
// arithmetic in the same order): c = Phi^T y, M packed, I what the solve reads.  ap: the clipped amplitudes a'; q: the reported
// linear parameters of the pair (f_j = a'_j / S kept inside the box for the S0 class); returns cost - 0.5 ||y||^2.
// OPEN: this, and sym_logdet with the prep kernel's difference system in pnx_varpro_posterior.hip, are hand copies
// of expressions inside varpro_match_kernel, spd_inverse and varpro_finish_kernel, made because the posterior was not to touch
// pnx_varpro.hip.  That the a_hat = 0 atoms of the variable projection are exactly the lw = -inf atoms here rests on the copies
// staying equal: whoever edits either side edits both, until this helper serves pnx_varpro.hip too.
template <int K, int CLS>
__device__ inline double vp_solve(const double *c, const double *M, const double *I, const double *lo, const double *hi, double *q, bool *clipped) {
    double ap[K];
    bool clip = false;
    if constexpr (CLS == kVarproReduced) {
        constexpr int NN = (K - 1) * K / 2;
        double tt[K], rest = 1.0;
#pragma unroll
        for (int i = 0; i < K - 1; ++i) tt[i] = (c[i] - c[K - 1]) - I[NN + i];
#pragma unroll
        for (int i = 0; i < K - 1; ++i) {
            double ah = 0.0;
#pragma unroll
            for (int j = 0; j < K - 1; ++j) ah = fma(I[vpk(i, j)], tt[j], ah);
            ap[i] = fmin(fmax(ah, lo[i]), hi[i]);
            clip |= ap[i] != ah;
            q[i] = ap[i];
            rest -= ap[i];
        }
        ap[K - 1] = rest;
        q[K - 1] = 0.0;
    } else {
        double ah[K], sum = 0.0;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            ah[i] = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) ah[i] = fma(I[vpk(i, j)], c[j], ah[i]);
            sum += ah[i];
        }
        if constexpr (CLS == kVarproFree) {
#pragma unroll
            for (int i = 0; i < K; ++i) {
                ap[i] = fmin(fmax(ah[i], lo[i]), hi[i]);
                clip |= ap[i] != ah[i];
                q[i] = ap[i];
            }
        } else {  // S0 class: the amplitude sum first, the fraction bounds scale with it
            const double S = fmin(fmax(sum, lo[K - 1]), hi[K - 1]);
            clip |= S != sum;
            double rest = S;
#pragma unroll
            for (int i = 0; i < K - 1; ++i) {
                ap[i] = fmin(fmax(ah[i], lo[i] * S), hi[i] * S);
                clip |= ap[i] != ah[i];
                // f_j = a'_j / S; the quotient of a'_j = hi_fj S may round one ulp past hi_fj: kept inside the box
                q[i] = S > 0.0 ? fmin(fmax(ap[i] / S, lo[i]), hi[i]) : lo[i];
                rest -= ap[i];
            }
            ap[K - 1] = rest;
            q[K - 1] = S;
        }
    }
    double cc = 0.0;  // 0.5 a'^T M a' - c . a'
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double ma = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) ma = fma(M[vpk(i, j)], ap[j], ma);
        cc = fma(ap[i], fma(0.5, ma, -c[i]), cc);
    }
    *clipped = clip;
    return cc;
}

// l_g of one voxel-atom pair, the posterior's expressions term for term: solve, clip, cost = 0.5 ||y||^2 + cc, then
//   noise marginalised:  lw - gain log(max(cost, tol)),  gain = nu / 2;     known noise:  lw - cost gain,  gain = 1 / noise_sd^2.
// lw holds the log prior (and the Occam term); the caller does not call this for lw = -inf, which weighs exactly 0.
template <int K, int CLS>
__device__ inline double vp_log_weight(const double *c, const double *M, const double *I, const double *lo, const double *hi, double yy,
                                       double tol, double lw, double gain, int noise_marginal) {
    double q[K];
    bool clip;
    const double cc = vp_solve<K, CLS>(c, M, I, lo, hi, q, &clip);
    const double cost = fma(0.5, yy, cc);
    return noise_marginal ? fma(-gain, log(fmax(cost, tol)), lw) : fma(-cost, gain, lw);
}
}  // namespace pnx
