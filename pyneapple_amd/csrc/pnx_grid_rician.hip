// pnx_grid_rician.hip -- the grid posterior under a Rician likelihood with a known noise sd (pnx_curvefit_grid_posterior_rician_f64,
// DESIGN.md 4.1t) and log I0e per element (pnx_log_i0e_f64).  Magnitude signals follow a Rice distribution; its log-density is the
// Gaussian one plus, per voxel and atom, C_g(v) = sum_i h(y_vi s_gi / sigma^2), h = log I0e (pnx_bessel.hpp), and constants of the voxel.
//
//   grid_rician_posterior_kernel   grid_posterior_kernel's strip, slab, lane map and fold (pnx_grid_posterior.hip), known noise, no
//                                  projected amplitude.  Between the MFMA product of a 16 x 16 tile and its fold every accumulator
//                                  element (voxel row kq + 4 r, atom column r16 of the lane) gains C: a loop over the b-values, i
//                                  ascending, one chain of additions per element.  s_gi is the slab's dictionary row in LDS (the B
//                                  operand, one read per (i, atom)), y_ri comes from the wave's 16 signal rows, which it keeps in
//                                  LDS beside the slab (the A fragments in registers serve the MFMA: a loop over i that is not
//                                  unrolled cannot index them, and the unrolled one does not fit the register file).  C is not a matrix product: it is
//                                  fp64 VALU work, 4 n_b evaluations of h per lane and tile.
//   log_i0e_kernel                 one lane per element.
//
// Lane maps of the MFMA as in pnx_grid.hip: A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom), row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "pnx_bessel.hpp"
#include "pnx_grid_rician.hpp"
#include "pnx_internal.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

#define GRC_HIP(call)                                                                                \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) return set_error(PNX_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

// ---- log I0e per element ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) log_i0e_kernel(const double *z, double *out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = log_i0e(z[i]);
}

int log_i0e_device(int64_t n, const double *z_d, double *out_d, hipStream_t stream) {
    if (n <= 0) return PNX_OK;
    const long long blocks = ((long long)n + 255) / 256;
    if (blocks > INT_MAX) return set_error(PNX_ERR_INVALID, "log_i0e: n=%lld is more than one launch holds", (long long)n);
    hipLaunchKernelGGL(log_i0e_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, z_d, out_d, (long long)n);
    GRC_HIP(hipGetLastError());
    return PNX_OK;
}

// ---- posterior --------------------------------------------------------------------------------------------------------------
// A block is NW waves (grid_rician_slab: 4 up to 32 b-values, 2 beyond), a wave owns one strip of 16 voxels per pass, the dictionary
// comes through LDS in slabs as in grid_posterior_kernel.  NS: k-steps the register file is sized for (n_b <= 4 NS); NF: parameter
// rows (n_free <= NF).

struct RicArgs {
    const double *y;               // (n_vox, n_b)
    const double *st;              // (kpad, gp)
    const double *nrm, *lp;        // (gp)
    const double *theta;           // (n_free, gp)
    const double *atoms;           // (n_free, n_atoms)
    double *mean, *sd, *map_p;     // (n_free, n_vox); sd and map_p may be null
    int32_t *map_atom;             // (n_vox) or null
    double *logev, *ess;           // (n_vox) or null
    long long n_vox;
    int n_b, kpad, n_atoms, gp, n_free, width, stride, ypitch, yoff;  // yoff: doubles in front of the signal rows
    double gain;  // 1 / noise_sd^2
    double lp_norm;
    double centre[PNX_MAX_PARAMS];
};

template <int NS, int NF, int NW>
__global__ void __launch_bounds__(NW * 64) grid_rician_posterior_kernel(const RicArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_b = a.n_b, kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lnrm = lds + kpad * stride, *linv = lnrm + W, *llp = linv + W, *lth = llp + W;
    double *ys = lds + a.yoff + wave * 16 * a.ypitch;  // this wave's signal rows, [16][ypitch]
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + NW - 1) / NW;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double gain = a.gain;
    constexpr bool YREG = NS <= 8;  // the A fragments stay in registers; the wide form reads them back from its signal rows in LDS
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        // A fragment of this wave's strip: rows past the end repeat the last voxel, never stored.  A negative entry is no
        // magnitude: the voxel is reported as a non-finite one.  ly: sum_i log(y_i / sigma^2), the voxel's constant of the evidence.
        const long long v0 = (grp * NW + wave) * 16;
        double yf[YREG ? NS : 1], yy, ly;
        int nf;
        {
            const long long v = v0 + r16;
            const double *row = a.y + (size_t)(v < a.n_vox ? v : a.n_vox - 1) * n_b;
            double ss = 0.0, sl = 0.0;
            int bad = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int k = 4 * s + kq;
                const bool in = s < ksteps && k < n_b;
                const double val = in ? row[k] : 0.0;
                bad |= !(fabs(val) < inf) || val < 0.0;
                ss = fma(val, val, ss);
                if (in) sl += log(val * gain);
                if constexpr (YREG) yf[s] = val;
                if (s < ksteps) ys[r16 * a.ypitch + k] = val;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the rows are wave-private: no block barrier; LDS keeps a wave's order
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            sl += __shfl_xor(sl, 16);
            sl += __shfl_xor(sl, 32);
            bad |= __shfl_xor(bad, 16);
            bad |= __shfl_xor(bad, 32);
            yy = ss;
            ly = sl;
            nf = bad;
        }
        double yyr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) yyr[r] = __shfl(yy, kq + 4 * r);
        double m[4], sw[4], sw2[4], mu[4][NF], m2[4][NF];
        int bg[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            m[r] = -inf;
            sw[r] = sw2[r] = 0.0;
            bg[r] = INT_MAX;
#pragma unroll
            for (int k = 0; k < NF; ++k) mu[r][k] = m2[r][k] = 0.0;
        }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                for (int k = wave; k < kpad; k += NW)
                    for (int j = lane; j < wc; j += 64) lds[k * stride + j] = a.st[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < a.n_free; k += NW)
                    for (int j = lane; j < wc; j += 64) lth[k * W + j] = a.theta[(size_t)k * a.gp + g0 + j];
                for (int j = threadIdx.x; j < wc; j += NW * 64) {
                    lnrm[j] = a.nrm[g0 + j];
                    llp[j] = a.lp[g0 + j];
                }
                __syncthreads();
                resident = n_slabs == 1;
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
                const double *bp = lds + kq * stride + t * 16 + r16;  // B fragment: S[g0 + 16 t + r16][4 s + kq]
                if constexpr (YREG) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        if (s < ksteps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(yf[s], bp[4 * s * stride], acc, 0, 0, 0);
                    }
                } else {  // the A fragments out of the wave's signal rows in LDS, in the same order of k
                    const double *ap = ys + r16 * a.ypitch + kq;
#pragma unroll 4
                    for (int s = 0; s < ksteps; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * s], bp[4 * s * stride], acc, 0, 0, 0);
                }
                // the Rician correction of the tile: C[r] = sum_i h(|(y[kq + 4 r][i] s[g][i]) / sigma^2|), i ascending
                const double *sp = lds + t * 16 + r16;  // s[g][i] = sp[i * stride]
                const double *yr = ys + kq * a.ypitch;  // y[kq + 4 r][i] = yr[4 r ypitch + i]
                double C[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
                for (int i = 0; i < n_b; ++i) {
                    const double sv = sp[i * stride];
#pragma unroll
                    for (int r = 0; r < 4; ++r) C[r] += log_i0e(fabs(yr[4 * r * a.ypitch + i] * sv * gain));
                }
                // fold: grid_posterior_kernel's, known noise, with l = (log_prior - cost / sigma^2) + C
                const int j = t * 16 + r16, g = g0 + j;
                const double lpg = llp[j];
                if (lpg > -inf) {
                    const double nr = lnrm[j];
                    double th[NF];
#pragma unroll
                    for (int k = 0; k < NF; ++k) th[k] = k < a.n_free ? lth[k * W + j] : 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double c = fma(0.5, nr, -acc[r]);
                        const double cost = fma(0.5, yyr[r], c);
                        const double lg = fma(-cost, gain, lpg);
                        const double ell = lg + C[r];
                        const double d = ell - m[r];  // +inf for the first atom of the row
                        const bool up = d > 0.0;
                        const double e = exp(-fabs(d));
                        const double alpha = up ? e : 1.0, w = up ? 1.0 : e;
                        m[r] = up ? ell : m[r];
                        bg[r] = up ? g : bg[r];
                        const double wn = fma(alpha, sw[r], w);
                        const double q = w / wn;  // wn >= 1 once an atom has been seen
                        sw[r] = wn;
                        sw2[r] = fma(alpha * alpha, sw2[r], w * w);
#pragma unroll
                        for (int k = 0; k < NF; ++k) {
                            const double x = th[k];
                            const double dl = x - mu[r][k];
                            mu[r][k] = fma(q, dl, mu[r][k]);
                            m2[r][k] = fma(w, dl * (x - mu[r][k]), alpha * m2[r][k]);
                        }
                    }
                }
            }
        }
        // the merge over the 16 lanes that share a voxel and the outputs: grid_posterior_kernel's
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) {
                const double om = __shfl_xor(m[r], off, 16), ow = __shfl_xor(sw[r], off, 16), ow2 = __shfl_xor(sw2[r], off, 16);
                const int og = __shfl_xor(bg[r], off, 16);
                const double mn = fmax(m[r], om);
                const double fa = m[r] == mn ? 1.0 : exp(m[r] - mn);  // (-inf) - (-inf) never reaches exp
                const double fb = om == mn ? 1.0 : exp(om - mn);
                const double wa = fa * sw[r], wb = fb * ow, wn = wa + wb;
                const double q = wn > 0.0 ? wb / wn : 0.0;
                const bool take = om > m[r] || (om == m[r] && og < bg[r]);
                bg[r] = take ? og : bg[r];
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
            const int src = kq + 4 * r;  // this voxel's row of the strip: its flag and its constant live in lane `src`
            const int badv = __shfl(nf, src);
            const double lyv = __shfl(ly, src);
            const long long v = v0 + src;
            if (v < a.n_vox) {
                const double qnan = __builtin_nan("");
                if (r16 < a.n_free) {
                    double mean = 0.0, var = 0.0;
#pragma unroll
                    for (int k = 0; k < NF; ++k)
                        if (r16 == k) {
                            mean = a.centre[k] + mu[r][k];
                            var = m2[r][k] / sw[r];
                        }
                    const size_t o = (size_t)r16 * a.n_vox + v;
                    a.mean[o] = badv ? qnan : mean;
                    if (a.sd) a.sd[o] = badv ? qnan : sqrt(fmax(var, 0.0));
                    if (a.map_p) {
                        double val = qnan;
                        if (!badv && bg[r] != INT_MAX) val = a.atoms[(size_t)r16 * a.n_atoms + bg[r]];
                        a.map_p[o] = val;
                    }
                } else if (r16 == 8) {
                    if (a.map_atom) a.map_atom[v] = (badv || bg[r] == INT_MAX) ? -1 : bg[r];
                } else if (r16 == 9) {
                    if (a.logev) {
                        const double le = m[r] + log(sw[r]) - a.lp_norm;
                        a.logev[v] = badv ? qnan : le + lyv;
                    }
                } else if (r16 == 10) {
                    if (a.ess) a.ess[v] = badv ? qnan : sw[r] * sw[r] / sw2[r];
                }
            }
        }
    }
}

template <int NS, int NF, int NW> static int launch_ric(const RicArgs &a, size_t lds, long long blocks, hipStream_t st) {
    hipLaunchKernelGGL((grid_rician_posterior_kernel<NS, NF, NW>), dim3((unsigned)blocks), dim3(NW * 64), lds, st, a);
    GRC_HIP(hipGetLastError());
    return PNX_OK;
}

template <int NS, int NW> static int launch_ric_nf(const RicArgs &a, size_t lds, long long blocks, hipStream_t st) {
    if (a.n_free <= 3) return launch_ric<NS, 3, NW>(a, lds, blocks, st);
    if (a.n_free <= 6) return launch_ric<NS, 6, NW>(a, lds, blocks, st);
    return launch_ric<NS, 8, NW>(a, lds, blocks, st);
}

int grid_rician_posterior_device(const GridDict &D, const GridPosterior &P, int64_t n_vox, const double *y_d, double *mean_d, double *sd_d,
                                 int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, int cus, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const GridRicianSlab RS = grid_rician_slab(D.n_b, D.n_free);
    const GridSlab &S = RS.slab;
    RicArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.nrm = D.nrm;
    a.lp = P.lp;
    a.theta = P.theta;
    a.atoms = D.atoms;
    a.mean = mean_d;
    a.sd = sd_d;
    a.map_p = map_p_d;
    a.map_atom = map_atom_d;
    a.logev = log_evidence_d;
    a.ess = ess_d;
    a.n_vox = n_vox;
    a.n_b = D.n_b;
    a.kpad = S.kpad;
    a.n_atoms = D.n_atoms;
    a.gp = D.gp;
    a.n_free = D.n_free;
    a.width = S.width < D.gp ? S.width : D.gp;
    a.stride = S.stride;
    a.ypitch = RS.ypitch;
    a.yoff = S.lds_doubles;
    a.gain = 1.0 / (P.noise_sd * P.noise_sd);
    a.lp_norm = P.log_prior_norm;
    for (int k = 0; k < PNX_MAX_PARAMS; ++k) a.centre[k] = P.centre[k];
    const size_t lds = (size_t)RS.lds_doubles * sizeof(double);  // <= 64 KB
    const long long n_strips = (n_vox + 15) / 16;
    long long blocks = (n_strips + RS.waves - 1) / RS.waves;
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;
    if (blocks > cap) blocks = cap;
    if (S.kpad <= 32) return launch_ric_nf<8, 4>(a, lds, blocks, stream);
    return launch_ric_nf<32, 2>(a, lds, blocks, stream);
}

}  // namespace pnx
