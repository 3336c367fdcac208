// pnx_grid_mrf_kernel.hpp -- the field posterior's kernel and its launch, shared by the two translation units that instantiate it:
// pnx_grid_mrf.hip (WREAL = false: the Gaussian prior, the half-count n_v / 2 of a voxel held in a float, from field_n) and
// pnx_grid_tmrf.hip (WREAL = true: the Student-t prior, the half-weight W_v / 2 held in a double, from field_w).
// Everything else is one text, so the WREAL = false instantiations are the kernels of DESIGN.md 4.1p unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "pnx_grid_mrf.hpp"
#include "pnx_internal.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

#define GM_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) return set_error(PNX_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

// ---- posterior with the field -----------------------------------------------------------------------------------------------
// The posterior's block: four waves, one per SIMD, a strip of 16 voxels per wave and pass.  The slab (pnx_grid_mrf_args.hpp
// grid_mrf_slab): [kpad][stride] | nrm | inv | log_prior | r | theta[n_free], each `width` wide, then one double per wave for the
// reduction of delta.  NS: k-steps of y . s the register file is sized for (n_b <= 4 NS); NF: parameter rows (n_free <= NF); the
// field product takes (NF + 3) / 4 k-steps.
constexpr int kMrfWaves = 4;

struct MrfArgs {
    const double *y;      // (n_vox, n_b)
    const double *st;     // (kpad, gp)
    const double *nrm, *inv, *lp, *r;  // (gp)
    const double *theta;  // (n_free, gp)
    const double *wd;     // (kpad)
    const double *atoms;  // (n_free, n_atoms)
    const double *max_nrm;
    const double *fq;     // (n_free, n_vox)
    const int32_t *fn;    // (n_vox): the present neighbours, WREAL = false
    const double *fw;     // (n_vox): the sum of the neighbours' weights, WREAL = true
    double *mean, *sd, *map_p;  // (n_free, n_vox); sd and map_p may be null
    int32_t *map_atom;          // (n_vox) or null
    double *logev, *ess;        // (n_vox) or null
    double *block;              // (gridDim.x) partial maxima of delta, or null
    long long n_vox, first, count;
    int n_b, kpad, n_atoms, gp, n_free, width, stride, s0_row, marginal, use_field;
    double lo_s0, hi_s0;
    double tol_scale;  // 4 n_b 2^-52
    double gain;       // known noise: 1 / noise_sd^2;  marginalised: nu / 2
    double lp_norm;
    double centre[PNX_MAX_PARAMS];
    double scale[PNX_MAX_PARAMS];  // what delta of a row is divided by, 0: the row takes no part
};

template <int NS, int NF, bool PROJ, bool WREAL>
__global__ void __launch_bounds__(kMrfWaves * 64) grid_mrf_posterior_kernel(const MrfArgs a) {
    extern __shared__ double lds[];
    constexpr int NQ = (NF + 3) / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_b = a.n_b, kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lnrm = lds + kpad * stride, *linv = lnrm + W, *llp = linv + W, *lr = llp + W, *lth = lr + W, *lred = lth + a.n_free * W;
    const long long end = a.first + a.count;
    const long long n_strips = (a.count + 15) / 16;
    const long long n_groups = (n_strips + kMrfWaves - 1) / kMrfWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double max_nrm = *a.max_nrm;
    bool resident = false;
    double dmax = 0.0;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        // A fragment of this wave's strip, as the posterior loads it: rows past the end repeat the range's last voxel, never stored
        const long long v0 = a.first + (grp * kMrfWaves + wave) * 16;
        double yf[NS], yy, qf[NQ];
        int nf, nloc = 0;
        double wloc = 0.0;
        {
            const long long v = v0 + r16;
            const long long vv = v < end ? v : end - 1;
            const double *row = a.y + (size_t)vv * n_b;
            double ss = 0.0;
            int bad = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int k = 4 * s + kq;
                const double val = (s < ksteps && k < n_b) ? row[k] * a.wd[k] : 0.0;
                bad |= !(fabs(val) < inf);
                ss = fma(val, val, ss);
                yf[s] = val;
            }
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            bad |= __shfl_xor(bad, 16);
            bad |= __shfl_xor(bad, 32);
            yy = ss;
            nf = bad;
            // A fragment of the field product: q[4 s + kq] of voxel r16; rows past n_free and a projected S0 row hold 0
#pragma unroll
            for (int s = 0; s < NQ; ++s) {
                const int k = 4 * s + kq;
                qf[s] = (a.use_field && k < a.n_free && !(PROJ && k == a.s0_row)) ? a.fq[(size_t)k * a.n_vox + vv] : 0.0;
            }
            if constexpr (WREAL)
                wloc = a.use_field ? a.fw[vv] : 0.0;
            else
                nloc = a.use_field ? a.fn[vv] : 0;
        }
        // the accumulator rows of this lane are the voxels kq + 4 r of the strip: their ||y||^2, the floor of their cost, n_v / 2 (W_v / 2)
        double yyr[4], tol[4];
        typename std::conditional<WREAL, double, float>::type hn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            yyr[r] = __shfl(yy, kq + 4 * r);
            tol[r] = a.tol_scale * (yyr[r] + max_nrm);
            if constexpr (WREAL)
                hn[r] = 0.5 * __shfl(wloc, kq + 4 * r);
            else
                hn[r] = 0.5f * (float)__shfl(nloc, kq + 4 * r);
        }
        double m[4], sw[4], sw2[4], am[4], mu[4][NF], m2[4][NF];
        int bg[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            m[r] = -inf;
            sw[r] = sw2[r] = am[r] = 0.0;
            bg[r] = INT_MAX;
#pragma unroll
            for (int k = 0; k < NF; ++k) mu[r][k] = m2[r][k] = 0.0;
        }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                for (int k = wave; k < kpad; k += kMrfWaves)
                    for (int j = lane; j < wc; j += 64) lds[k * stride + j] = a.st[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < a.n_free; k += kMrfWaves)
                    for (int j = lane; j < wc; j += 64) lth[k * W + j] = a.theta[(size_t)k * a.gp + g0 + j];
                for (int j = threadIdx.x; j < wc; j += kMrfWaves * 64) {
                    lnrm[j] = a.nrm[g0 + j];
                    linv[j] = a.inv[g0 + j];
                    llp[j] = a.lp[g0 + j];
                    lr[j] = a.r[g0 + j];
                }
                __syncthreads();
                resident = n_slabs == 1;
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
                const double *bp = lds + kq * stride + t * 16 + r16;  // B fragment: S[g0 + 16 t + r16][4 s + kq]
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (s < ksteps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(yf[s], bp[4 * s * stride], acc, 0, 0, 0);
                }
                const int j = t * 16 + r16, g = g0 + j;
                // the field product q_v . thetac_g of the tile, an accumulator of its own: B[4 s + kq][r16] = thetac[4 s + kq][g]
                f64x4 fld = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < NQ; ++s) {
                    const int k = 4 * s + kq;
                    const double tb = (k < a.n_free && !(PROJ && k == a.s0_row)) ? lth[k * W + j] : 0.0;
                    fld = __builtin_amdgcn_mfma_f64_16x16x4f64(qf[s], tb, fld, 0, 0, 0);
                }
                // fold: this lane's atom against its four voxels.  A padded or excluded atom holds log_prior = -inf and contributes
                // exactly nothing; atoms arrive in ascending order, so a strict comparison keeps the lowest index among equal l.
                const double lpg = llp[j];
                if (lpg > -inf) {
                    const double nr = lnrm[j];
                    const double iv = PROJ ? linv[j] : 0.0;
                    const double rg = lr[j];
                    double th[NF];
#pragma unroll
                    for (int k = 0; k < NF; ++k) th[k] = k < a.n_free ? lth[k * W + j] : 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double dot = acc[r];
                        double amp = 1.0, c;  // c = cost - 0.5 ||y||^2, grid start's
                        if constexpr (PROJ) {
                            amp = fmin(fmax(dot * iv, a.lo_s0), a.hi_s0);
                            c = amp * fma(0.5 * amp, nr, -dot);
                        } else {
                            c = fma(0.5, nr, -dot);
                        }
                        const double cost = fma(0.5, yyr[r], c);
                        const double ell0 = a.marginal ? fma(-a.gain, log(fmax(cost, tol[r])), lpg) : fma(-cost, a.gain, lpg);
                        const double ell = ell0 + fma(-(double)hn[r], rg, fld[r]);  // a zero field: -0 * r + 0 = +0.0, ell0 unchanged
                        // weights relative to the running maximum: one exp serves the new weight or the rescale of the old sums
                        const double d = ell - m[r];  // +inf for the first atom of the row
                        const bool up = d > 0.0;
                        const double e = exp(-fabs(d));
                        const double alpha = up ? e : 1.0, w = up ? 1.0 : e;
                        m[r] = up ? ell : m[r];
                        bg[r] = up ? g : bg[r];
                        am[r] = up ? amp : am[r];
                        const double wn = fma(alpha, sw[r], w);
                        const double q = w / wn;  // wn >= 1 once an atom has been seen
                        sw[r] = wn;
                        sw2[r] = fma(alpha * alpha, sw2[r], w * w);
#pragma unroll
                        for (int k = 0; k < NF; ++k) {
                            const double x = (PROJ && k == a.s0_row) ? amp : th[k];
                            const double dl = x - mu[r][k];
                            mu[r][k] = fma(q, dl, mu[r][k]);
                            m2[r][k] = fma(w, dl * (x - mu[r][k]), alpha * m2[r][k]);
                        }
                    }
                }
            }
        }
        // one merge over the 16 lanes (atoms modulo 16) that share a voxel: log-sum-exp of the weights, Chan's update of the
        // moments, (higher l, then lower index) for the MAP atom.  A lane that saw no admissible atom holds m = -inf, W = 0.
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) {
                const double om = __shfl_xor(m[r], off, 16), ow = __shfl_xor(sw[r], off, 16), ow2 = __shfl_xor(sw2[r], off, 16);
                const double oa = __shfl_xor(am[r], off, 16);
                const int og = __shfl_xor(bg[r], off, 16);
                const double mn = fmax(m[r], om);
                const double fa = m[r] == mn ? 1.0 : exp(m[r] - mn);  // (-inf) - (-inf) never reaches exp
                const double fb = om == mn ? 1.0 : exp(om - mn);
                const double wa = fa * sw[r], wb = fb * ow, wn = wa + wb;
                const double q = wn > 0.0 ? wb / wn : 0.0;
                const bool take = om > m[r] || (om == m[r] && og < bg[r]);
                bg[r] = take ? og : bg[r];
                am[r] = take ? oa : am[r];
#pragma unroll
                for (int k = 0; k < NF; ++k) {
                    const double omu = __shfl_xor(mu[r][k], off, 16), om2 = __shfl_xor(m2[r][k], off, 16);
                    const double dl = omu - mu[r][k];
                    mu[r][k] = fma(q, dl, mu[r][k]);
                    m2[r][k] = fma(dl * dl, wa * q, fma(fa, m2[r][k], fb * om2));
                }
                sw2[r] = fma(fa * fa, sw2[r], fb * fb * ow2);
                sw[r] = wn;
                m[r] = mn;
            }
            const int src = kq + 4 * r;  // this voxel's row of the strip: its finite flag lives in lane `src`
            const int badv = __shfl(nf, src);
            const long long v = v0 + src;
            if (v < end) {
                const double qnan = __builtin_nan("");
                if (r16 < a.n_free) {
                    double mean = 0.0, var = 0.0, sc = 0.0;
#pragma unroll
                    for (int k = 0; k < NF; ++k)
                        if (r16 == k) {
                            mean = a.centre[k] + mu[r][k];
                            var = m2[r][k] / sw[r];
                            sc = a.scale[k];
                        }
                    const size_t o = (size_t)r16 * a.n_vox + v;
                    if (a.block && sc > 0.0 && !badv) dmax = fmax(dmax, fabs(mean - a.mean[o]) / sc);  // the old mean, before it is overwritten
                    a.mean[o] = badv ? qnan : mean;
                    if (a.sd) a.sd[o] = badv ? qnan : sqrt(fmax(var, 0.0));
                    if (a.map_p) {
                        double val = qnan;
                        if (!badv && bg[r] != INT_MAX) val = (PROJ && r16 == a.s0_row) ? am[r] : a.atoms[(size_t)r16 * a.n_atoms + bg[r]];
                        a.map_p[o] = val;
                    }
                } else if (r16 == 8) {
                    if (a.map_atom) a.map_atom[v] = (badv || bg[r] == INT_MAX) ? -1 : bg[r];
                } else if (r16 == 9) {
                    if (a.logev) a.logev[v] = badv ? qnan : m[r] + log(sw[r]) - a.lp_norm;
                } else if (r16 == 10) {
                    if (a.ess) a.ess[v] = badv ? qnan : sw[r] * sw[r] / sw2[r];
                }
            }
        }
    }
    if (a.block) {  // uniform: the block's maximum of delta, one value per wave through the slab's tail
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, off));
        if (lane == 0) lred[wave] = dmax;
        __syncthreads();
        if (threadIdx.x == 0) a.block[blockIdx.x] = fmax(fmax(lred[0], lred[1]), fmax(lred[2], lred[3]));
    }
}

template <int NS, int NF, bool WREAL> static int launch_mrf(const MrfArgs &a, size_t lds, long long blocks, hipStream_t st) {
    if (a.s0_row >= 0)
        hipLaunchKernelGGL((grid_mrf_posterior_kernel<NS, NF, true, WREAL>), dim3((unsigned)blocks), dim3(kMrfWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((grid_mrf_posterior_kernel<NS, NF, false, WREAL>), dim3((unsigned)blocks), dim3(kMrfWaves * 64), lds, st, a);
    GM_HIP(hipGetLastError());
    return PNX_OK;
}

template <int NS, bool WREAL> static int launch_mrf_nf(const MrfArgs &a, size_t lds, long long blocks, hipStream_t st) {
    if (a.n_free <= 3) return launch_mrf<NS, 3, WREAL>(a, lds, blocks, st);
    if (a.n_free <= 6) return launch_mrf<NS, 6, WREAL>(a, lds, blocks, st);
    return launch_mrf<NS, 8, WREAL>(a, lds, blocks, st);
}

// grid_mrf_posterior_device (pnx_grid_mrf.hpp) with the weight of the voxel's r_g term from field_n_d (WREAL = false) or field_w_d
// (WREAL = true); the other of the two is not read.
template <bool WREAL>
static int grid_mrf_posterior_run(const GridDict &D, const GridPosterior &P, const GridMrf &F, int64_t n_vox, int64_t first, int64_t count,
                                  const double *y_d, const double *field_q_d, const int32_t *field_n_d, const double *field_w_d, double *mean_d,
                                  double *sd_d, int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, double *delta_d,
                                  bool accumulate, int cus, hipStream_t stream) {
    if (count <= 0) {
        if (delta_d && !accumulate) GM_HIP(hipMemsetAsync(delta_d, 0, sizeof(double), stream));
        return PNX_OK;
    }
    const GridSlab S = grid_mrf_slab(D.n_b, D.n_free);
    MrfArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.nrm = D.nrm;
    a.inv = D.inv;
    a.lp = P.lp;
    a.r = F.r;
    a.theta = P.theta;
    a.wd = D.w;
    a.atoms = D.atoms;
    a.max_nrm = P.max_nrm;
    a.fq = field_q_d;
    a.fn = field_n_d;
    a.fw = field_w_d;
    a.mean = mean_d;
    a.sd = sd_d;
    a.map_p = map_p_d;
    a.map_atom = map_atom_d;
    a.logev = log_evidence_d;
    a.ess = ess_d;
    a.block = delta_d ? F.block : nullptr;
    a.n_vox = n_vox;
    a.first = first;
    a.count = count;
    a.n_b = D.n_b;
    a.kpad = S.kpad;
    a.n_atoms = D.n_atoms;
    a.gp = D.gp;
    a.n_free = D.n_free;
    a.width = S.width < D.gp ? S.width : D.gp;
    a.stride = S.stride;
    a.s0_row = D.s0_row;
    a.marginal = P.noise_sd == 0.0;
    a.use_field = F.any ? 1 : 0;
    a.lo_s0 = D.lo_s0;
    a.hi_s0 = D.hi_s0;
    a.tol_scale = 4.0 * D.n_b * 0x1p-52;
    a.gain = a.marginal ? 0.5 * (D.n_b - (D.s0_row >= 0 ? 1 : 0)) : 1.0 / (P.noise_sd * P.noise_sd);
    a.lp_norm = P.log_prior_norm;
    for (int k = 0; k < PNX_MAX_PARAMS; ++k) {
        a.centre[k] = P.centre[k];
        a.scale[k] = F.scale[k];
    }
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    const long long n_strips = (count + 15) / 16;
    long long blocks = (n_strips + kMrfWaves - 1) / kMrfWaves;
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;  // F.blocks
    if (blocks > cap) blocks = cap;
    int rc = S.kpad <= 32 ? launch_mrf_nf<8, WREAL>(a, lds, blocks, stream) : launch_mrf_nf<32, WREAL>(a, lds, blocks, stream);
    if (rc) return rc;
    if (delta_d) return grid_mrf_delta_device(F.block, (int)blocks, delta_d, accumulate, stream);
    return PNX_OK;
}

}  // namespace pnx
