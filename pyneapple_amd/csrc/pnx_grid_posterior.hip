// pnx_grid_posterior.hip -- posterior mean / sd / MAP / evidence / effective sample size of every voxel over a dictionary of
// parameter vectors (pnx_curvefit_grid_posterior_f64).  Attention with Q = signals, K = dictionary, V = parameter
// values: the product y_v . s_g is grid start's (pnx_grid.hip: same dictionary, same slab and lane layout, same cost), the fold of
// an accumulator tile into (min, argmin) is replaced by a running log-sum-exp with weighted moments.
//
//   grid_posterior_prep_kernel   per atom what the fold reads besides the dictionary row: the parameter values minus their row's
//                                centre, log_prior padded with -inf, and max_g ||s_g||^2 (the cancellation floor)
//   grid_posterior_kernel        one strip of 16 voxels per wave.  In the 16x16x4 accumulator layout a lane owns one atom column
//                                and four voxel rows of a tile: per row it keeps (m, W, sum w^2, argmax, mean_k, M2_k) with
//                                weights relative to the running maximum m, merged by the weighted Welford / Chan update -- every
//                                M2 contribution is non-negative, so a posterior that sits on one atom reports a small sd instead
//                                of the cancellation of E[theta^2] - mean^2.  One log-sum-exp merge over the 16 lanes of a voxel.
//
// Lane maps of the MFMA as in pnx_grid.hip: A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom), row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "pnx_grid_posterior.hpp"
#include "pnx_internal.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

#define GP_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) return set_error(PNX_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- per-atom inputs --------------------------------------------------------------------------------------------------------
struct PrepArgs {
    const double *atoms;  // (n_free, n_atoms)
    const double *lp_in;  // (n_atoms) or null
    const double *nrm;    // (gp)
    double *theta;        // (n_free, gp)
    double *lp;           // (gp)
    double *max_nrm;      // (1)
    int n_free, n_atoms, gp;
    double centre[PNX_MAX_PARAMS];
};

__global__ void __launch_bounds__(256) grid_posterior_prep_kernel(const PrepArgs a) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    for (int i = blockIdx.x * 256 + tid; i < a.n_free * a.gp; i += gridDim.x * 256) {
        const int k = i / a.gp, g = i - k * a.gp;
        a.theta[i] = g < a.n_atoms ? a.atoms[(size_t)k * a.n_atoms + g] - a.centre[k] : 0.0;
    }
    for (int g = blockIdx.x * 256 + tid; g < a.gp; g += gridDim.x * 256)
        a.lp[g] = g < a.n_atoms ? (a.lp_in ? a.lp_in[g] : 0.0) : -__builtin_huge_val();
    if (blockIdx.x) return;
    double mx = 0.0;  // squared norms: never negative, padded atoms hold 0
    for (int g = tid; g < a.gp; g += 256) mx = fmax(mx, a.nrm[g]);
    red[tid] = mx;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) *a.max_nrm = red[0];
}

size_t grid_posterior_bytes(int n_free, int n_atoms) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15;
    return up256((size_t)n_free * gp * 8) + up256(gp * 8) + up256((size_t)n_atoms * 8) + up256(8);
}

int grid_posterior_prepare(const GridDict &D, const GridPosteriorHost &H, const double *log_prior_host, double noise_sd, void *buffer_d,
                           GridPosterior *P, hipStream_t st) {
    char *p = (char *)buffer_d;
    auto take = [&](size_t bytes) {
        void *q = p;
        p += up256(bytes);
        return (double *)q;
    };
    double *theta = take((size_t)D.n_free * D.gp * 8), *lp = take((size_t)D.gp * 8), *lp_in = take((size_t)D.n_atoms * 8), *mx = take(8);
    if (log_prior_host) GP_HIP(hipMemcpyAsync(lp_in, log_prior_host, (size_t)D.n_atoms * 8, hipMemcpyHostToDevice, st));  // staged as the atoms
    PrepArgs a;
    memset(&a, 0, sizeof(a));
    a.atoms = D.atoms;
    a.lp_in = log_prior_host ? lp_in : nullptr;
    a.nrm = D.nrm;
    a.theta = theta;
    a.lp = lp;
    a.max_nrm = mx;
    a.n_free = D.n_free;
    a.n_atoms = D.n_atoms;
    a.gp = D.gp;
    for (int k = 0; k < D.n_free; ++k) a.centre[k] = H.centre[k];
    const int blocks = (D.n_free * D.gp + 255) / 256;
    hipLaunchKernelGGL(grid_posterior_prep_kernel, dim3(blocks), dim3(256), 0, st, a);
    GP_HIP(hipGetLastError());
    P->theta = theta;
    P->lp = lp;
    P->max_nrm = mx;
    for (int k = 0; k < PNX_MAX_PARAMS; ++k) P->centre[k] = H.centre[k];
    P->log_prior_norm = H.log_prior_norm;
    P->noise_sd = noise_sd;
    return PNX_OK;
}

// ---- posterior --------------------------------------------------------------------------------------------------------------
// A block is four waves, one per SIMD, and a wave owns one strip of 16 voxels per pass: the accumulators of four voxel rows
// (4 (5 + 2 NF) doubles) and the y fragments (NS doubles) take 150 to 230 of the 512 registers a lane has at one wave per SIMD,
// the four independent exp / log chains of a fold the rest; at eight waves (256 registers) every instantiation but the smallest
// spilled.  The dictionary comes through LDS in slabs of `width` atoms (pnx_grid_posterior_args.hpp
// grid_posterior_slab): [kpad][stride] | nrm | inv | log_prior | theta[n_free], each `width` wide.  NS: k-steps the register file
// is sized for (n_b <= 4 NS); NF: parameter rows it is sized for (n_free <= NF).
constexpr int kPostWaves = 4;

struct PostArgs {
    const double *y;      // (n_vox, n_b)
    const double *st;     // (kpad, gp)
    const double *nrm, *inv, *lp;  // (gp)
    const double *theta;  // (n_free, gp)
    const double *wd;     // (kpad)
    const double *atoms;  // (n_free, n_atoms)
    const double *max_nrm;
    double *mean, *sd, *map_p;  // (n_free, n_vox); sd and map_p may be null
    int32_t *map_atom;          // (n_vox) or null
    double *logev, *ess;        // (n_vox) or null
    long long n_vox;
    int n_b, kpad, n_atoms, gp, n_free, width, stride, s0_row, marginal;
    double lo_s0, hi_s0;
    double tol_scale;  // 4 n_b 2^-52
    double gain;       // known noise: 1 / noise_sd^2;  marginalised: nu / 2
    double lp_norm;
    double centre[PNX_MAX_PARAMS];
};

template <int NS, int NF, bool PROJ>
__global__ void __launch_bounds__(kPostWaves * 64) grid_posterior_kernel(const PostArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_b = a.n_b, kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lnrm = lds + kpad * stride, *linv = lnrm + W, *llp = linv + W, *lth = llp + W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kPostWaves - 1) / kPostWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double max_nrm = *a.max_nrm;
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        // A fragment of this wave's strip, as grid start loads it: rows past the end repeat the last voxel, never stored
        const long long v0 = (grp * kPostWaves + wave) * 16;
        double yf[NS], yy;
        int nf;
        {
            const long long v = v0 + r16;
            const double *row = a.y + (size_t)(v < a.n_vox ? v : a.n_vox - 1) * n_b;
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
        }
        // the accumulator rows of this lane are the voxels kq + 4 r of the strip: their ||y||^2 and the floor of their cost
        double yyr[4], tol[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            yyr[r] = __shfl(yy, kq + 4 * r);
            tol[r] = a.tol_scale * (yyr[r] + max_nrm);
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
                for (int k = wave; k < kpad; k += kPostWaves)
                    for (int j = lane; j < wc; j += 64) lds[k * stride + j] = a.st[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < a.n_free; k += kPostWaves)
                    for (int j = lane; j < wc; j += 64) lth[k * W + j] = a.theta[(size_t)k * a.gp + g0 + j];
                for (int j = threadIdx.x; j < wc; j += kPostWaves * 64) {
                    lnrm[j] = a.nrm[g0 + j];
                    linv[j] = a.inv[g0 + j];
                    llp[j] = a.lp[g0 + j];
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
                // fold: this lane's atom against its four voxels.  A padded or excluded atom holds log_prior = -inf and contributes
                // exactly nothing; atoms arrive in ascending order, so a strict comparison keeps the lowest index among equal l.
                const int j = t * 16 + r16, g = g0 + j;
                const double lpg = llp[j];
                if (lpg > -inf) {
                    const double nr = lnrm[j];
                    const double iv = PROJ ? linv[j] : 0.0;
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
                        const double ell = a.marginal ? fma(-a.gain, log(fmax(cost, tol[r])), lpg) : fma(-cost, a.gain, lpg);
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
}

template <int NS, int NF> static int launch_post(const PostArgs &a, size_t lds, long long blocks, hipStream_t st) {
    if (a.s0_row >= 0)
        hipLaunchKernelGGL((grid_posterior_kernel<NS, NF, true>), dim3((unsigned)blocks), dim3(kPostWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((grid_posterior_kernel<NS, NF, false>), dim3((unsigned)blocks), dim3(kPostWaves * 64), lds, st, a);
    GP_HIP(hipGetLastError());
    return PNX_OK;
}

template <int NS> static int launch_post_nf(const PostArgs &a, size_t lds, long long blocks, hipStream_t st) {
    if (a.n_free <= 3) return launch_post<NS, 3>(a, lds, blocks, st);
    if (a.n_free <= 6) return launch_post<NS, 6>(a, lds, blocks, st);
    return launch_post<NS, 8>(a, lds, blocks, st);
}

int grid_posterior_device(const GridDict &D, const GridPosterior &P, int64_t n_vox, const double *y_d, double *mean_d, double *sd_d,
                          int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, int cus, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const GridSlab S = grid_posterior_slab(D.n_b, D.n_free);
    PostArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.nrm = D.nrm;
    a.inv = D.inv;
    a.lp = P.lp;
    a.theta = P.theta;
    a.wd = D.w;
    a.atoms = D.atoms;
    a.max_nrm = P.max_nrm;
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
    a.s0_row = D.s0_row;
    a.marginal = P.noise_sd == 0.0;
    a.lo_s0 = D.lo_s0;
    a.hi_s0 = D.hi_s0;
    a.tol_scale = 4.0 * D.n_b * 0x1p-52;
    a.gain = a.marginal ? 0.5 * (D.n_b - (D.s0_row >= 0 ? 1 : 0)) : 1.0 / (P.noise_sd * P.noise_sd);
    a.lp_norm = P.log_prior_norm;
    for (int k = 0; k < PNX_MAX_PARAMS; ++k) a.centre[k] = P.centre[k];
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    const long long n_strips = (n_vox + 15) / 16;
    long long blocks = (n_strips + kPostWaves - 1) / kPostWaves;
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;
    if (blocks > cap) blocks = cap;
    if (S.kpad <= 32) return launch_post_nf<8>(a, lds, blocks, stream);
    return launch_post_nf<32>(a, lds, blocks, stream);
}

}  // namespace pnx
