// pnx_varpro_logmrf.hip -- the neighbourhood (MRF) prior of the posterior over the variable projection's dictionary with a per-row
// choice of the coupled quantity (pnx_curvefit_varpro_posterior_logfield_f64,
// pnx_curvefit_varpro_posterior_logmrf_f64).  Every free non-linear row k couples f_k = nl_atoms[row_k] or f_k = log nl_atoms[row_k];
// with its neighbours' means of f held fixed a voxel's l_g gains
//     sum_{k non-linear} fc_kg q_vk - 0.5 n_v r_g,   fc = f - fcentre,  q_vk = precision_k sum_u (field_mean[k, u] - fcentre_k),
// and the fold reports, from one set of weights, the moments over the linear theta (mean, sd: what every other call of the
// posterior reports) and the mean of f (field_mean: what the next gather reads).
//
//   varpro_logmrf_posterior_kernel   varpro_mrf_posterior_kernel (pnx_varpro_mrf.hip), expression for expression, with two changes:
//                                    the slab carries the centred field rows fc beside the centred moment rows theta -- fc is the
//                                    B operand of the one-k-step field product, theta serves the moments only -- and a voxel row
//                                    keeps one more running weighted mean per non-linear row, of fc, through the same Welford step
//                                    and the same 16-lane Chan merge as mu.  With every coupling 0, fc holds theta's bytes and
//                                    the call returns the bytes of the linear field call; a zero field adds exactly +0.0.
//                                    Where the added means do not fit the register file without scratch, a lane folds fewer of
//                                    its four rows per sweep over the dictionary (NH > 1, the NS = 32 forms' remedy).
//
// The gather, the colour check and the reduction of delta over the blocks are pnx_grid_mrf.hip's.  Lane maps of the MFMA as in
// pnx_grid.hip: A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom), row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pnx_internal.hpp"
#include "pnx_varpro_logmrf.hpp"
#include "pnx_varpro_pair.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

#define VM_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) return set_error(PNX_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// the maximum of the blocks' partial maxima of delta: pnx_grid_mrf.hip's kernel, launched from here
__global__ void grid_mrf_delta_kernel(const double *block, int n, double *out, int accumulate);

// ---- per-call inputs --------------------------------------------------------------------------------------------------------
size_t varpro_logmrf_bytes(int n_nl, int n_atoms, int cus) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15;
    return up256(gp * 8) + up256((size_t)n_nl * gp * 8) + up256((size_t)(cus > 0 ? cus : 256) * 2 * 8) + up256(2 * sizeof(int32_t));
}

__global__ void varpro_logmrf_flags_kernel(int32_t *flags) {
    if (threadIdx.x < 2) flags[threadIdx.x] = INT_MAX;
}

int varpro_logmrf_prepare(const VarproDict &D, const VarproLogMrfHost &G, const double *nl_atoms_host, const double *precision,
                          const int32_t *coupling, int cus, void *buffer_d, VarproLogMrf *F, hipStream_t st) {
    char *p = (char *)buffer_d;
    F->r = (double *)p;
    p += up256((size_t)D.gp * 8);
    F->fc = (double *)p;
    p += up256((size_t)D.L.n_nl * D.gp * 8);
    F->blocks = (cus > 0 ? cus : 256) * 2;
    F->block = (double *)p;
    p += up256((size_t)F->blocks * 8);
    F->flags = (int32_t *)p;
    F->any = grid_mrf_any_precision(D.n_free, precision);
    varpro_logmrf_delta_scale(D.n_free, precision, G, F->scale);
    for (int k = 0; k < PNX_MAX_PARAMS; ++k) F->fcentre[k] = G.fcentre[k];
    std::vector<double> r((size_t)D.gp), fc((size_t)D.L.n_nl * D.gp);
    varpro_logmrf_rows(D.n_free, D.L, D.n_atoms, D.gp, nl_atoms_host, G.fcentre, precision, coupling, fc.data(), r.data());
    VM_HIP(hipMemcpyAsync(F->r, r.data(), (size_t)D.gp * 8, hipMemcpyHostToDevice, st));  // pageable: staged before the call returns, as the atoms
    VM_HIP(hipMemcpyAsync(F->fc, fc.data(), fc.size() * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(varpro_logmrf_flags_kernel, dim3(1), dim3(64), 0, st, F->flags);
    VM_HIP(hipGetLastError());
    return PNX_OK;
}

// ---- posterior with the field -----------------------------------------------------------------------------------------------
// The posterior's block: four waves, one per SIMD, a strip of 16 voxels per wave and pass.  The slab (pnx_varpro_logmrf_args.hpp
// varpro_logmrf_slab): [K kpad][stride] | constants [2 NM][W] | lw [W] | r [W] | theta [K + 1][W] | fc [K + 1][W], then one double
// per wave for the reduction of delta at the slab's tail.  NS: k-steps the register file is sized for (n_b <= 4 NS); T1: the layout
// has K + 1 free non-linear rows (every rate and T1), otherwise at most K.
constexpr int kVpLogMrfWaves = 4;

// Sweeps over the dictionary per strip: a lane folds 4 / NH of its four voxel rows per sweep (the products of the other rows are
// formed again).  The linear field kernel's rule, and one step further where the added means of fc would not fit the register file
// without scratch (DESIGN.md 4.1r has the compiler's resource table).
template <int NS, int K, int CLS, bool T1> constexpr int vp_logmrf_nh() {
    if (NS > 8) return K == 3 ? 4 : 2;
    return (K == 3 && T1) ? 2 : 1;
}
// At NS = 32 and K = 3 a lane already folds one row per sweep; with a free T1 or the S0 class the means of fc still do not fit.
template <int NS, int K, int CLS, bool T1> constexpr int vp_logmrf_np() { return (NS > 8 && K == 3 && (T1 || CLS == kVarproS0)) ? 2 : 1; }

struct VpLogMrfArgs {
    const double *y;      // (n_vox, n_b)
    const double *st;     // (K kpad, gp)
    const double *cst;    // (crow, gp)
    const double *wd;     // (kpad)
    const double *nl;     // (n_nl, n_atoms)
    const double *lw;     // (gp)
    const double *r;      // (gp)
    const double *theta;  // (n_nl, gp) the moment rows
    const double *fc;     // (n_nl, gp) the field rows
    const double *max_nrm;
    const double *fq;     // (n_free, n_vox)
    const int32_t *fn;    // (n_vox)
    double *mean, *sd, *map_p;     // (n_free, n_vox); sd and map_p may be null
    double *fmean;                 // (n_free, n_vox) the mean of f; read (the old value, for delta) and written
    int32_t *map_atom;             // (n_vox) or null
    double *logev, *ess, *cmass;   // (n_vox) or null
    double *block;                 // (gridDim.x) partial maxima of delta, or null
    long long n_vox, first, count;
    int n_b, kpad, n_atoms, gp, n_free, n_nl, width, stride, red_off, use_field;
    int noise_marginal;  // the noise is marginalised (noise_sd == 0); marginal_amplitudes is already inside lw
    int row_src[PNX_MAX_PARAMS];
    int nl_free[4];                 // per row of nl_atoms its free row (the row of field_q)
    double centre[PNX_MAX_PARAMS];  // per free row
    double fcentre[PNX_MAX_PARAMS]; // per free row, of f
    double scale[PNX_MAX_PARAMS];   // what delta of a row is divided by (the range of f), 0: the row takes no part
    double lo[3], hi[3];            // bounds of the linear slots (S0 class: slot K - 1 is S0)
    double tol_scale;               // 4 n_b 2^-52
    double amp2;                    // A^2
    double gain;                    // known noise: 1 / noise_sd^2;  marginalised: nu / 2
    double lp_norm;
};

template <int NS, int K, int CLS, bool T1>
__global__ void __launch_bounds__(kVpLogMrfWaves * 64) varpro_logmrf_posterior_kernel(const VpLogMrfArgs a) {
    constexpr int NM = K * (K + 1) / 2;
    constexpr int NLIN = CLS == kVarproReduced ? K - 1 : K;  // linear slots that are parameters
    constexpr int NNL = T1 ? K + 1 : K;                      // non-linear rows the layout can have free
    constexpr int NMOM = NLIN + NNL;                         // moments: the linear slots, then the non-linear rows
    constexpr int NH = vp_logmrf_nh<NS, K, CLS, T1>(), RH = 4 / NH;  // sweeps over the dictionary per strip, rows of a lane per sweep
    constexpr int NP = vp_logmrf_np<NS, K, CLS, T1>();               // passes of those sweeps: 2 splits the means of fc from the rest
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_b = a.n_b, kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lc = lds + K * kpad * stride, *llw = lc + 2 * NM * W, *lr = llw + W, *lth = lr + W, *lfc = lth + (K + 1) * W;
    double *lred = lds + a.red_off;
    const long long end = a.first + a.count;
    const long long n_strips = (a.count + 15) / 16;
    const long long n_groups = (n_strips + kVpLogMrfWaves - 1) / kVpLogMrfWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double floor_nrm = a.amp2 * *a.max_nrm;
    bool resident = false;
    if (lane == 0) lred[wave] = 0.0;  // this wave's maximum of delta: the slot is the wave's own until the barrier at the end
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        // A fragment of this wave's strip, as the posterior loads it: rows past the end repeat the range's last voxel, never stored
        const long long v0 = a.first + (grp * kVpLogMrfWaves + wave) * 16;
        double yf[NS], yy, qf;
        int nf, nloc;
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
                bad |= !(fabs(val) < inf);  // NaN or Inf, of the signal or through a zero sigma
                ss = fma(val, val, ss);
                yf[s] = val;
            }
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            bad |= __shfl_xor(bad, 16);
            bad |= __shfl_xor(bad, 32);
            yy = ss;
            nf = bad;
            // A fragment of the field product: q of non-linear row kq of voxel r16; rows past n_nl hold 0
            int fr = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (kq == k) fr = a.nl_free[k];
            qf = (a.use_field && kq < a.n_nl) ? a.fq[(size_t)fr * a.n_vox + vv] : 0.0;
            nloc = a.use_field ? a.fn[vv] : 0;
        }
        // the accumulator rows of this lane are the voxels kq + 4 r of the strip.  NH sweeps over the dictionary, each with the fold
        // state of RH of the lane's four rows (the products of the other rows are formed again: the price of no scratch).
        // Where even one row per sweep does not fit (NP == 2), the rows' sweeps run twice: first for every output of the linear
        // field kernel, then, with the same l, maximum and weight sums in the same order -- the same bits -- for the means of fc alone.
      auto sweep = [&](const int h, auto with_moments, auto with_field_means) __attribute__((always_inline)) {
        constexpr bool doM = decltype(with_moments)::value, doF = decltype(with_field_means)::value;
        // of this sweep's rows: their ||y||^2, the floor of their cost, n_v / 2
        double yyr[RH], tol[RH];
        float hn[RH];
#pragma unroll
        for (int r = 0; r < RH; ++r) {
            yyr[r] = __shfl(yy, kq + 4 * (h * RH + r));
            tol[r] = a.tol_scale * (yyr[r] + floor_nrm);
            hn[r] = 0.5f * (float)__shfl(nloc, kq + 4 * (h * RH + r));
        }
        double m[RH], sw[RH], sw2[RH], cm[RH], bq[RH][K], mu[RH][NMOM], m2[RH][NMOM], mf[RH][NNL];
        int bg[RH];
#pragma unroll
        for (int r = 0; r < RH; ++r) {
            m[r] = -inf;
            sw[r] = sw2[r] = cm[r] = 0.0;
            bg[r] = INT_MAX;
#pragma unroll
            for (int i = 0; i < K; ++i) bq[r][i] = 0.0;
#pragma unroll
            for (int k = 0; k < NMOM; ++k) mu[r][k] = m2[r][k] = 0.0;
#pragma unroll
            for (int k = 0; k < NNL; ++k) mf[r][k] = 0.0;
        }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                for (int k = wave; k < K * kpad; k += kVpLogMrfWaves)
                    for (int j = lane; j < wc; j += 64) lds[k * stride + j] = a.st[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < 2 * NM; k += kVpLogMrfWaves)
                    for (int j = lane; j < wc; j += 64) lc[k * W + j] = a.cst[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < a.n_nl; k += kVpLogMrfWaves)
                    for (int j = lane; j < wc; j += 64) {
                        lth[k * W + j] = a.theta[(size_t)k * a.gp + g0 + j];
                        lfc[k * W + j] = a.fc[(size_t)k * a.gp + g0 + j];
                    }
                for (int j = threadIdx.x; j < wc; j += kVpLogMrfWaves * 64) {
                    llw[j] = a.lw[g0 + j];
                    lr[j] = a.r[g0 + j];
                }
                __syncthreads();
                resident = n_slabs == 1;
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc[K];
#pragma unroll
                for (int i = 0; i < K; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
                const double *bp = lds + kq * stride + t * 16 + r16;  // B fragment: phi_i[g0 + 16 t + r16][4 s + kq]
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (s < ksteps) {
#pragma unroll
                        for (int i = 0; i < K; ++i)
                            acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(yf[s], bp[(i * kpad + 4 * s) * stride], acc[i], 0, 0, 0);
                    }
                }
                const int j16 = t * 16 + r16, g = g0 + j16;
                // the field product q_v . fc_g of the tile, an accumulator of its own: B[kq][r16] = fc[kq][g]
                const double tb = kq < a.n_nl ? lfc[kq * W + j16] : 0.0;
                const f64x4 fld = __builtin_amdgcn_mfma_f64_16x16x4f64(qf, tb, f64x4{0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
                // fold: this lane's atom against its rows.  A padded or excluded atom holds lw = -inf and contributes exactly
                // nothing; atoms arrive in ascending order, so a strict comparison keeps the lowest index among equal l.
                const double lwg = llw[j16];
                if (lwg > -inf) {
                    const double rg = lr[j16];
                    double M[NM], I[NM], th[NNL], fv[NNL];
#pragma unroll
                    for (int q = 0; q < NM; ++q) {
                        M[q] = lc[q * W + j16];
                        I[q] = lc[(NM + q) * W + j16];
                    }
#pragma unroll
                    for (int k = 0; k < NNL; ++k) {
                        th[k] = k < a.n_nl ? lth[k * W + j16] : 0.0;
                        fv[k] = k < a.n_nl ? lfc[k * W + j16] : 0.0;
                    }
#pragma unroll
                    for (int r = 0; r < RH; ++r) {
                        double c[K], q[K];
#pragma unroll
                        for (int i = 0; i < K; ++i) c[i] = acc[i][h * RH + r];
                        bool clip;
                        const double cc = vp_solve<K, CLS>(c, M, I, a.lo, a.hi, q, &clip);
                        const double cost = fma(0.5, yyr[r], cc);
                        const double ell0 = a.noise_marginal ? fma(-a.gain, log(fmax(cost, tol[r])), lwg) : fma(-cost, a.gain, lwg);
                        const double ell = ell0 + fma(-(double)hn[r], rg, fld[h * RH + r]);  // a zero field: -0 * r + 0 = +0.0, ell0 unchanged
                        // weights relative to the running maximum: one exp serves the new weight or the rescale of the old sums
                        const double d = ell - m[r];  // +inf for the first atom of the row
                        const bool up = d > 0.0;
                        const double e = exp(-fabs(d));
                        const double alpha = up ? e : 1.0, w = up ? 1.0 : e;
                        m[r] = up ? ell : m[r];
                        bg[r] = up ? g : bg[r];
                        const double wn = fma(alpha, sw[r], w);
                        const double qq = w / wn;  // wn >= 1 once an atom has been seen
                        sw[r] = wn;
                        if (doM) {
#pragma unroll
                            for (int i = 0; i < K; ++i) bq[r][i] = up ? q[i] : bq[r][i];
                            sw2[r] = fma(alpha * alpha, sw2[r], w * w);
                            cm[r] = fma(alpha, cm[r], clip ? w : 0.0);
#pragma unroll
                            for (int k = 0; k < NMOM; ++k) {
                                const double x = k < NLIN ? q[k < K ? k : 0] : th[k - NLIN < 0 ? 0 : k - NLIN];
                                const double dl = x - mu[r][k];
                                mu[r][k] = fma(qq, dl, mu[r][k]);
                                m2[r][k] = fma(w, dl * (x - mu[r][k]), alpha * m2[r][k]);
                            }
                        }
                        if (doF) {
#pragma unroll
                            for (int k = 0; k < NNL; ++k) mf[r][k] = fma(qq, fv[k] - mf[r][k], mf[r][k]);  // the mean of fc: mu's step, no second moment
                        }
                    }
                }
            }
        }
        // one merge over the 16 lanes (atoms modulo 16) that share a voxel: log-sum-exp of the weights, Chan's update of the
        // moments, (higher l, then lower index) for the MAP atom.  A lane that saw no admissible atom holds m = -inf, W = 0.
        double dmax = 0.0;
#pragma unroll
        for (int r = 0; r < RH; ++r) {
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) {
                const double om = __shfl_xor(m[r], off, 16), ow = __shfl_xor(sw[r], off, 16);
                const int og = __shfl_xor(bg[r], off, 16);
                const double mn = fmax(m[r], om);
                const double fa = m[r] == mn ? 1.0 : exp(m[r] - mn);  // (-inf) - (-inf) never reaches exp
                const double fb = om == mn ? 1.0 : exp(om - mn);
                const double wa = fa * sw[r], wb = fb * ow, wn = wa + wb;
                const double qq = wn > 0.0 ? wb / wn : 0.0;
                const bool take = om > m[r] || (om == m[r] && og < bg[r]);
                bg[r] = take ? og : bg[r];
                if (doM) {
                    const double ow2 = __shfl_xor(sw2[r], off, 16), ocm = __shfl_xor(cm[r], off, 16);
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const double oq = __shfl_xor(bq[r][i], off, 16);
                        bq[r][i] = take ? oq : bq[r][i];
                    }
#pragma unroll
                    for (int k = 0; k < NMOM; ++k) {
                        const double omu = __shfl_xor(mu[r][k], off, 16), om2 = __shfl_xor(m2[r][k], off, 16);
                        const double dl = omu - mu[r][k];
                        mu[r][k] = fma(qq, dl, mu[r][k]);
                        m2[r][k] = fma(dl * dl, wa * qq, fma(fa, m2[r][k], fb * om2));
                    }
                    sw2[r] = fma(fa * fa, sw2[r], fb * fb * ow2);
                    cm[r] = fma(fa, cm[r], fb * ocm);
                }
                if (doF) {
#pragma unroll
                    for (int k = 0; k < NNL; ++k) {
                        const double omf = __shfl_xor(mf[r][k], off, 16);
                        mf[r][k] = fma(qq, omf - mf[r][k], mf[r][k]);
                    }
                }
                sw[r] = wn;
                m[r] = mn;
            }
            const int src = kq + 4 * (h * RH + r);  // this voxel's row of the strip: its finite flag lives in lane `src`
            const int badv = __shfl(nf, src) | (bg[r] == INT_MAX);  // a non-finite signal, or no atom with a finite l
            const long long v = v0 + src;
            if (v < end) {
                const double qnan = __builtin_nan("");
                const int gi = badv ? 0 : bg[r];
                if (r16 < a.n_free) {
                    int rs = 0;
                    double ctr = 0.0, fctr = 0.0, sc = 0.0;
#pragma unroll
                    for (int k = 0; k < PNX_MAX_PARAMS; ++k)
                        if (r16 == k) {
                            rs = a.row_src[k];
                            ctr = a.centre[k];
                            fctr = a.fcentre[k];
                            sc = a.scale[k];
                        }
                    const int mom = rs >= 0 ? NLIN + rs : -1 - rs;  // this row's moment
                    double mean = 0.0, var = 0.0, mapv = 0.0;
#pragma unroll
                    for (int k = 0; k < NMOM; ++k)
                        if (mom == k) {
                            mean = ctr + mu[r][k];
                            var = m2[r][k] / sw[r];
                        }
                    if (rs >= 0) {
                        mapv = a.nl[(size_t)rs * a.n_atoms + gi];
                    } else {
#pragma unroll
                        for (int i = 0; i < K; ++i)
                            if (-1 - rs == i) mapv = bq[r][i];
                    }
                    const size_t o = (size_t)r16 * a.n_vox + v;
                    if (doM) {
                        a.mean[o] = badv ? qnan : mean;
                        if (a.sd) a.sd[o] = badv ? qnan : sqrt(fmax(var, 0.0));
                        if (a.map_p) a.map_p[o] = badv ? qnan : mapv;
                    }
                    if (doF) {
                        double fm = NP == 1 ? mean : a.mean[o];  // a fraction / S0 row: the bytes of mean (NP == 2: as this lane stored them)
#pragma unroll
                        for (int k = 0; k < NNL; ++k)
                            if (rs == k) fm = fctr + mf[r][k];
                        if (a.block && sc > 0.0 && !badv) dmax = fmax(dmax, fabs(fm - a.fmean[o]) / sc);  // the old mean of f, before it is overwritten
                        a.fmean[o] = badv ? qnan : fm;
                    }
                } else if (!doM) {
                    // the second pass writes field_mean alone
                } else if (r16 == 8) {
                    if (a.map_atom) a.map_atom[v] = badv ? -1 : gi;
                } else if (r16 == 9) {
                    if (a.logev) a.logev[v] = badv ? qnan : m[r] + log(sw[r]) - a.lp_norm;
                } else if (r16 == 10) {
                    if (a.ess) a.ess[v] = badv ? qnan : sw[r] * sw[r] / sw2[r];
                } else if (r16 == 11) {
                    if (a.cmass) a.cmass[v] = badv ? qnan : fmin(cm[r] / sw[r], 1.0);
                }
            }
        }
        if (a.block) {  // uniform: fold this sweep's maximum of delta into the wave's slot at the slab's tail
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, off));
            if (lane == 0) lred[wave] = fmax(lred[wave], dmax);
        }
      };
        if constexpr (NP == 1) {
#pragma unroll
            for (int h = 0; h < NH; ++h) sweep(h, std::true_type{}, std::true_type{});
        } else {
#pragma unroll
            for (int h = 0; h < NH; ++h) sweep(h, std::true_type{}, std::false_type{});
#pragma unroll
            for (int h = 0; h < NH; ++h) sweep(h, std::false_type{}, std::true_type{});
        }
        if (a.block && grp + gridDim.x >= n_groups) {  // uniform: the block's last group, its maximum
            __syncthreads();
            if (threadIdx.x == 0) a.block[blockIdx.x] = fmax(fmax(lred[0], lred[1]), fmax(lred[2], lred[3]));
        }
    }
}

template <int K, int CLS, bool T1> static int launch_vp_logmrf_t1(const VpLogMrfArgs &a, size_t lds, long long blocks, hipStream_t st) {
    if (a.kpad <= 32)
        hipLaunchKernelGGL((varpro_logmrf_posterior_kernel<8, K, CLS, T1>), dim3((unsigned)blocks), dim3(kVpLogMrfWaves * 64), lds, st, a);
    else if constexpr (K == 3 && CLS == kVarproS0 && T1)  // varpro_logmrf_check_layout refuses it on the host: not instantiated
        return set_error(PNX_ERR_UNSUPPORTED, "varpro posterior logfield: no kernel for three compartments with S0 and a free T1 above 32 b-values");
    else
        hipLaunchKernelGGL((varpro_logmrf_posterior_kernel<32, K, CLS, T1>), dim3((unsigned)blocks), dim3(kVpLogMrfWaves * 64), lds, st, a);
    VM_HIP(hipGetLastError());
    return PNX_OK;
}

template <int K, int CLS> static int launch_vp_logmrf(const VpLogMrfArgs &a, size_t lds, long long blocks, hipStream_t st) {
    return a.n_nl > K ? launch_vp_logmrf_t1<K, CLS, true>(a, lds, blocks, st) : launch_vp_logmrf_t1<K, CLS, false>(a, lds, blocks, st);
}

int varpro_logmrf_posterior_device(const VarproDict &D, const VarproPosterior &P, const VarproLogMrf &F, bool use_field, int64_t n_vox,
                                   int64_t first, int64_t count, const double *y_d, const double *field_q_d, const int32_t *field_n_d,
                                   double *mean_d, double *sd_d, int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d,
                                   double *clipped_mass_d, double *field_mean_d, double *delta_d, bool accumulate, int cus, hipStream_t stream) {
    if (count <= 0) {
        if (delta_d && !accumulate) VM_HIP(hipMemsetAsync(delta_d, 0, sizeof(double), stream));
        return PNX_OK;
    }
    const VarproLayout &L = D.L;
    if (L.n_nl > L.k + 1 || L.n_nl > 4) return set_error(PNX_ERR_INVALID, "varpro posterior logfield: %d non-linear rows for %d compartments", L.n_nl, L.k);
    const GridSlab S = varpro_logmrf_slab(D.n_b, L.k);
    VpLogMrfArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.cst = D.cst;
    a.wd = D.w;
    a.nl = D.nl;
    a.lw = P.lw;
    a.r = F.r;
    a.theta = P.theta;
    a.fc = F.fc;
    a.max_nrm = P.max_nrm;
    a.fq = field_q_d;
    a.fn = field_n_d;
    a.mean = mean_d;
    a.fmean = field_mean_d;
    a.sd = sd_d;
    a.map_p = map_p_d;
    a.map_atom = map_atom_d;
    a.logev = log_evidence_d;
    a.ess = ess_d;
    a.cmass = clipped_mass_d;
    a.block = delta_d ? F.block : nullptr;
    a.n_vox = n_vox;
    a.first = first;
    a.count = count;
    a.n_b = D.n_b;
    a.kpad = S.kpad;
    a.n_atoms = D.n_atoms;
    a.gp = D.gp;
    a.n_free = D.n_free;
    a.n_nl = L.n_nl;
    a.width = S.width < D.gp ? S.width : D.gp;
    a.stride = S.stride;
    a.red_off = S.lds_doubles - kGridMrfReduceDoubles;
    a.use_field = (use_field && F.any) ? 1 : 0;
    a.noise_marginal = P.noise_sd == 0.0;
    for (int r = 0; r < PNX_MAX_PARAMS; ++r) {
        a.row_src[r] = L.row_src[r];
        a.centre[r] = P.centre[r];
        a.fcentre[r] = F.fcentre[r];
        a.scale[r] = F.scale[r];
        if (r < D.n_free && L.row_src[r] >= 0) a.nl_free[L.row_src[r]] = r;
    }
    for (int j = 0; j < 3; ++j) {
        a.lo[j] = L.lin_lo[j];
        a.hi[j] = L.lin_hi[j];
    }
    a.tol_scale = 4.0 * D.n_b * 0x1p-52;
    a.amp2 = P.amp_l1 * P.amp_l1;
    a.gain = a.noise_marginal ? 0.5 * (D.n_b - L.n_lin) : 1.0 / (P.noise_sd * P.noise_sd);
    a.lp_norm = P.log_prior_norm;
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    const long long n_strips = (count + 15) / 16;
    long long blocks = (n_strips + kVpLogMrfWaves - 1) / kVpLogMrfWaves;
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;  // F.blocks
    if (blocks > cap) blocks = cap;
    int rc = PNX_ERR_INVALID;
    switch (L.k * 4 + L.cls) {
    case 1 * 4 + kVarproFree: rc = launch_vp_logmrf<1, kVarproFree>(a, lds, blocks, stream); break;
    case 2 * 4 + kVarproFree: rc = launch_vp_logmrf<2, kVarproFree>(a, lds, blocks, stream); break;
    case 2 * 4 + kVarproReduced: rc = launch_vp_logmrf<2, kVarproReduced>(a, lds, blocks, stream); break;
    case 2 * 4 + kVarproS0: rc = launch_vp_logmrf<2, kVarproS0>(a, lds, blocks, stream); break;
    case 3 * 4 + kVarproFree: rc = launch_vp_logmrf<3, kVarproFree>(a, lds, blocks, stream); break;
    case 3 * 4 + kVarproReduced: rc = launch_vp_logmrf<3, kVarproReduced>(a, lds, blocks, stream); break;
    case 3 * 4 + kVarproS0: rc = launch_vp_logmrf<3, kVarproS0>(a, lds, blocks, stream); break;
    default: return set_error(PNX_ERR_INVALID, "varpro posterior logfield: no kernel for %d compartments, class %d", L.k, L.cls);
    }
    if (rc) return rc;
    if (delta_d) {
        hipLaunchKernelGGL(grid_mrf_delta_kernel, dim3(1), dim3(256), 0, stream, (const double *)F.block, (int)blocks, delta_d, accumulate ? 1 : 0);
        VM_HIP(hipGetLastError());
    }
    return PNX_OK;
}

}  // namespace pnx
