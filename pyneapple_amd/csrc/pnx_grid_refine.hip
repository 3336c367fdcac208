// pnx_grid_refine.hip -- a second, fine grid per voxel, centred on that voxel's coarse posterior, and the posterior fold on it
// (pnx_curvefit_grid_refine_f64).  The grid differs from voxel to voxel, so the shared-dictionary product of
// pnx_grid_posterior.hip cannot serve it; the models are separable instead: a voxel needs exp(-b_i x) only at the values of its up
// to three rate axes, sum_k m_k n_b exponentials (at most 3 * 9 * 128), not one per atom and b-value.
//
//   grid_refine_kernel<MODEL>   one wave per voxel.  The wave keeps, for itself alone, in LDS: the signal row, the axis values of
//                               every model parameter (a fixed one is an axis of one value) and E[c][j][i] = exp(-b_i x_cj) of the
//                               rate axes.  Lanes stride over the atoms (the Cartesian product, the first row slowest: a mixed-radix
//                               counter that advances by 64 with carries, no division in the loop); per atom the DIRECT cost
//                               1/2 sum_i (y_i - s_i)^2, i ascending -- no cancellation term --, then grid_posterior_kernel's running
//                               log-sum-exp and Welford moments, and its merge over 64 lanes instead of 16.  No block barrier: nothing
//                               in LDS is shared between waves.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "pnx_curvefit_kernel.hpp"
#include "pnx_grid_refine.hpp"
#include "pnx_internal.hpp"

namespace pnx {

#define GRF_HIP(call)                                                                                \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) return set_error(PNX_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

struct RefArgs {
    const double *y;                // (n_vox, n_b)
    const double *centre, *hw;      // (n_free, n_vox)
    double *mean, *sd, *map_p;      // (n_free, n_vox); sd and map_p may be null
    double *ess, *log_norm;         // (n_vox) or null
    double *edge;                   // (n_free, n_vox) or null
    long long n_vox;
    int n_b, pitch, mmax, per_wave, marginal;
    int s0_pos;                     // model position of the projected S0, -1 without projection
    double gain;                    // 1 / noise_sd^2 (known noise), nu / 2 (marginalised)
    double tol_scale;               // 4 n_b 2^-52
    // per MODEL POSITION (not per free row), so that every index below is a compile-time one
    int is_free[kMaxP], row[kMaxP], npts[kMaxP];
    double lo[kMaxP], hi[kMaxP], fixeds[kMaxP];
    double b[kMaxB];
};

static_assert(kMaxP == PNX_MAX_PARAMS && kMaxB == PNX_MAX_BVALUES, "grid_refine_block sizes the LDS the kernel lays out");

template <int MODEL>
__global__ void __launch_bounds__(256) grid_refine_kernel(const RefArgs a) {
    using M = Model<MODEL>;
    constexpr int NALL = M::NALL, NC = M::NC, NP = kRefineMaxPoints;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), n_waves = blockDim.x >> 6;
    const int n_b = a.n_b, pitch = a.pitch, mmax = a.mmax;
    double *ys = lds + (size_t)wave * a.per_wave;  // [n_b]
    double *axv = ys + n_b;                        // [kMaxP][NP]: the values of every parameter's axis
    double *tab = axv + kMaxP * NP;                // [3][mmax][pitch]
    const double inf = __builtin_huge_val(), qnan = __builtin_nan("");
    const bool proj = a.s0_pos >= 0;
    for (long long v = (long long)blockIdx.x * n_waves + wave; v < a.n_vox; v += (long long)gridDim.x * n_waves) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the previous voxel's reads are behind us; LDS keeps a wave's order
        // ---- the voxel's axes (wave-uniform) and its signal row
        RefineAxis ax[NALL];
        double cc[NALL];  // the centre of the moment accumulation: the clipped centre, 0 for a projected S0 and a fixed parameter
        int bad = 0;
#pragma unroll
        for (int p = 0; p < NALL; ++p) {
            if (a.is_free[p] && p != a.s0_pos) {
                const double c = a.centre[(size_t)a.row[p] * a.n_vox + v], h = a.hw[(size_t)a.row[p] * a.n_vox + v];
                bad |= !(fabs(c) < inf) || !(h >= 0.0 && h < inf);
                ax[p] = grid_refine_axis(a.lo[p], a.hi[p], c, h, a.npts[p]);
                cc[p] = fmin(fmax(c, a.lo[p]), a.hi[p]);
            } else {
                const double f = p == a.s0_pos ? 1.0 : a.fixeds[p];  // the projected model is evaluated at S0 = 1
                ax[p].a = ax[p].b = f;
                ax[p].step = 0.0;
                ax[p].m = 1;
                cc[p] = 0.0;
            }
            if (lane < ax[p].m) axv[p * NP + lane] = grid_refine_value(ax[p], lane);
        }
        for (int i = lane; i < n_b; i += 64) {
            const double val = a.y[(size_t)v * n_b + i];
            bad |= !(fabs(val) < inf);
            ys[i] = val;
        }
        bad = __ballot(bad) != 0;
        int n_atoms = 1;
#pragma unroll
        for (int p = 0; p < NALL; ++p) n_atoms *= ax[p].m;
        double m = -inf, sw = 0.0, sw2 = 0.0, am = 0.0;
        double mu[NALL], m2[NALL], em[NALL];
        int bg = INT_MAX, cnt = 0;
#pragma unroll
        for (int p = 0; p < NALL; ++p) mu[p] = m2[p] = em[p] = 0.0;
        if (!bad) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            // ---- E[c][j][i] = exp(-b_i x_cj), the fit's own exp and argument
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int p = M::dpos(c);
                const int n_el = ax[p].m * n_b;
                for (int e = lane; e < n_el; e += 64) {
                    const int j = e / n_b, i = e - j * n_b;
                    const double nb = -a.b[i];
                    tab[(c * mmax + j) * pitch + i] = exp_fast(nb * axv[p * NP + j]);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            double tol = 0.0;
            if (a.marginal) {  // ||y||^2, i ascending, the same chain in every lane
                double yy = 0.0;
                for (int i = 0; i < n_b; ++i) yy = fma(ys[i], ys[i], yy);
                tol = fmax(a.tol_scale * yy, 2.2250738585072014e-308);
            }
            // ---- this lane's first atom and the digits of 64: index = ((j_0 m_1 + j_1) m_2 + ...), the last parameter fastest
            int jd[NALL], step[NALL];
            {
                int g = lane, s = 64;
#pragma unroll
                for (int p = NALL - 1; p >= 0; --p) {
                    const int mp = ax[p].m;
                    jd[p] = g % mp;
                    g /= mp;
                    step[p] = s % mp;
                    s /= mp;
                }
            }
            for (int g = lane; g < n_atoms; g += 64) {
                double prm[NALL];
#pragma unroll
                for (int p = 0; p < NALL; ++p) prm[p] = axv[p * NP + jd[p]];
                if (grid_refine_admissible(MODEL, prm)) {
                    const double *tc[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) tc[c] = tab + (c * mmax + jd[M::dpos(c)]) * pitch;
                    double amp = 1.0, acc = 0.0;
                    if (proj) {  // the closed-form clipped amplitude first: a = clip(y . s / s . s), lo_S0 for an all-zero row
                        double dot = 0.0, nrm = 0.0;
                        for (int i = 0; i < n_b; ++i) {
                            double E[NC];
#pragma unroll
                            for (int c = 0; c < NC; ++c) E[c] = tc[c][i];
                            const double s = M::signal(prm, E);
                            dot = fma(ys[i], s, dot);
                            nrm = fma(s, s, nrm);
                        }
                        double lo_s0 = 0.0, hi_s0 = 0.0;
#pragma unroll
                        for (int p = 0; p < NALL; ++p)
                            if (p == a.s0_pos) {
                                lo_s0 = a.lo[p];
                                hi_s0 = a.hi[p];
                            }
                        amp = nrm > 0.0 ? dot / nrm : lo_s0;
                        amp = fmin(fmax(amp, lo_s0), hi_s0);
                    }
                    for (int i = 0; i < n_b; ++i) {
                        double E[NC];
#pragma unroll
                        for (int c = 0; c < NC; ++c) E[c] = tc[c][i];
                        const double s = M::signal(prm, E);
                        const double d = proj ? fma(-amp, s, ys[i]) : ys[i] - s;
                        acc = fma(d, d, acc);
                    }
                    const double cost = 0.5 * acc;
                    const double ell = a.marginal ? -a.gain * log(fmax(cost, tol)) : -cost * a.gain;
                    // fold: grid_posterior_kernel's, and the share of the weight on the two ends of every axis
                    const double d = ell == m ? 0.0 : ell - m;  // +inf for the lane's first atom; (-inf) - (-inf), a cost that overflowed, is 0
                    const bool up = d > 0.0 || cnt == 0;  // the lane's first atom is its MAP so far, whatever its l
                    const double e = exp(-fabs(d));
                    const double alpha = up ? e : 1.0, w = up ? 1.0 : e;
                    m = up ? ell : m;
                    bg = up ? g : bg;
                    am = up ? amp : am;
                    const double wn = fma(alpha, sw, w);
                    const double q = w / wn;  // wn >= 1 once an atom has been seen
                    sw = wn;
                    sw2 = fma(alpha * alpha, sw2, w * w);
                    ++cnt;
#pragma unroll
                    for (int p = 0; p < NALL; ++p) {
                        if (!a.is_free[p]) continue;
                        const double x = (p == a.s0_pos ? amp : prm[p]) - cc[p];
                        const double dl = x - mu[p];
                        mu[p] = fma(q, dl, mu[p]);
                        m2[p] = fma(w, dl * (x - mu[p]), alpha * m2[p]);
                        const bool end = ax[p].m > 1 && (jd[p] == 0 || jd[p] == ax[p].m - 1);
                        em[p] = fma(alpha, em[p], end ? w : 0.0);
                    }
                }
                // the next atom of this lane: + 64 in the mixed radix, one carry per digit (j + step + carry < 2 m)
                int carry = 0;
#pragma unroll
                for (int p = NALL - 1; p >= 0; --p) {
                    const int t = jd[p] + step[p] + carry, mp = ax[p].m;
                    carry = t >= mp;
                    jd[p] = carry ? t - mp : t;
                }
            }
            // ---- the merge over the 64 lanes: log-sum-exp of the weights, Chan's update of the moments, (higher l, then lower
            // index) for the MAP atom.  A lane that saw no admitted atom holds m = -inf, W = 0.
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double om = __shfl_xor(m, off), ow = __shfl_xor(sw, off), ow2 = __shfl_xor(sw2, off), oa = __shfl_xor(am, off);
                const int og = __shfl_xor(bg, off), oc = __shfl_xor(cnt, off);
                const double mn = fmax(m, om);
                const double fa = m == mn ? 1.0 : exp(m - mn);  // (-inf) - (-inf) never reaches exp
                const double fb = om == mn ? 1.0 : exp(om - mn);
                const double wa = fa * sw, wb = fb * ow, wn = wa + wb;
                const double q = wn > 0.0 ? wb / wn : 0.0;
                const bool take = om > m || (om == m && og < bg);
                bg = take ? og : bg;
                am = take ? oa : am;
                cnt += oc;
#pragma unroll
                for (int p = 0; p < NALL; ++p) {
                    if (!a.is_free[p]) continue;
                    const double omu = __shfl_xor(mu[p], off), om2 = __shfl_xor(m2[p], off), oe = __shfl_xor(em[p], off);
                    const double dl = omu - mu[p];
                    mu[p] = fma(q, dl, mu[p]);
                    m2[p] = fma(dl * dl, wa * q, fma(fa, m2[p], fb * om2));
                    em[p] = fma(fa, em[p], fb * oe);
                }
                sw2 = fma(fa * fa, sw2, fb * fb * ow2);
                sw = wn;
                m = mn;
            }
        }
        // ---- outputs: lane p writes the row of model position p, lanes 8 and 9 the two per-voxel numbers
        const bool none = bad || cnt == 0;  // non-finite input, or no admitted atom: NaN everywhere
        int jm[NALL];
        {
            int g = none ? 0 : bg;
#pragma unroll
            for (int p = NALL - 1; p >= 0; --p) {
                jm[p] = g % ax[p].m;
                g /= ax[p].m;
            }
        }
#pragma unroll
        for (int p = 0; p < NALL; ++p) {
            if (lane == p && a.is_free[p]) {
                const size_t o = (size_t)a.row[p] * a.n_vox + v;
                a.mean[o] = none ? qnan : cc[p] + mu[p];
                if (a.sd) a.sd[o] = none ? qnan : sqrt(fmax(m2[p] / sw, 0.0));
                if (a.map_p) a.map_p[o] = none ? qnan : (p == a.s0_pos ? am : axv[p * NP + jm[p]]);
                if (a.edge) a.edge[o] = none ? qnan : em[p] / sw;
            }
        }
        if (lane == 8 && a.ess) a.ess[v] = none ? qnan : sw * sw / sw2;
        if (lane == 9 && a.log_norm) a.log_norm[v] = none ? qnan : m + log(sw) - log((double)cnt);
    }
}

template <int MODEL> static int launch_refine(const RefArgs &a, int waves, size_t lds, long long blocks, hipStream_t st) {
    hipLaunchKernelGGL((grid_refine_kernel<MODEL>), dim3((unsigned)blocks), dim3(waves * 64), lds, st, a);
    GRF_HIP(hipGetLastError());
    return PNX_OK;
}

int grid_refine_device(const pnx_curvefit_opts *o, const GridRefineHost &H, int64_t n_vox, const double *b, const double *y_d,
                       const double *fixed, const double *lo, const double *hi, double noise_sd, const int32_t *n_points,
                       const double *centre_d, const double *half_width_d, double *mean_d, double *sd_d, double *map_p_d, double *ess_d,
                       double *log_norm_d, double *edge_mass_d, int cus, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const GridRefineBlock B = grid_refine_block(o->n_b, H.mmax);
    RefArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.centre = centre_d;
    a.hw = half_width_d;
    a.mean = mean_d;
    a.sd = sd_d;
    a.map_p = map_p_d;
    a.ess = ess_d;
    a.log_norm = log_norm_d;
    a.edge = edge_mass_d;
    a.n_vox = n_vox;
    a.n_b = o->n_b;
    a.pitch = B.pitch;
    a.mmax = H.mmax;
    a.per_wave = B.per_wave;
    a.marginal = !(noise_sd > 0.0);
    a.s0_pos = H.s0_row >= 0 ? o->free_idx[H.s0_row] : -1;
    const int nu = o->n_b - (H.s0_row >= 0 ? 1 : 0);
    a.gain = a.marginal ? 0.5 * nu : 1.0 / (noise_sd * noise_sd);
    a.tol_scale = 4.0 * o->n_b * 0x1p-52;
    for (int p = 0; p < kMaxP; ++p) a.npts[p] = 1;
    for (int k = 0; k < o->n_free; ++k) {
        const int p = o->free_idx[k];
        a.is_free[p] = 1;
        a.row[p] = k;
        a.npts[p] = n_points[k];
        a.lo[p] = lo[k];
        a.hi[p] = hi[k];
    }
    for (int k = 0; k < o->n_fixed; ++k) a.fixeds[o->fixed_idx[k]] = fixed[k];
    for (int i = 0; i < o->n_b; ++i) a.b[i] = b[i];
    const size_t lds = (size_t)B.waves * B.per_wave * sizeof(double);  // <= 64 KB
    long long blocks = (n_vox + B.waves - 1) / B.waves;
    const long long cap = (long long)(cus > 0 ? cus : 256) * 8;
    if (blocks > cap) blocks = cap;
    switch (o->model) {
    case 0: return launch_refine<0>(a, B.waves, lds, blocks, stream);
    case 1: return launch_refine<1>(a, B.waves, lds, blocks, stream);
    case 2: return launch_refine<2>(a, B.waves, lds, blocks, stream);
    case 3: return launch_refine<3>(a, B.waves, lds, blocks, stream);
    case 4: return launch_refine<4>(a, B.waves, lds, blocks, stream);
    case 5: return launch_refine<5>(a, B.waves, lds, blocks, stream);
    case 6: return launch_refine<6>(a, B.waves, lds, blocks, stream);
    }
    return set_error(PNX_ERR_INVALID, "unknown model %d", o->model);
}

}  // namespace pnx
