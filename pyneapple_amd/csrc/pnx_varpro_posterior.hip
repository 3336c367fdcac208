// pnx_varpro_posterior.hip -- posterior mean / sd / MAP / evidence / effective sample size / clipped mass of every voxel over the
// variable projection's dictionary (pnx_curvefit_varpro_posterior_f64): only the rates (and a free T1) are on the
// grid, the amplitudes of every voxel-atom pair are eliminated in closed form (Bretthorst's treatment of sums of exponentials).
// The product c = Phi^T y, the amplitude solve, the clip rule and the cost are the variable projection's (pnx_varpro.hip: same
// dictionary, same lane maps, K MFMA chains per atom tile); the fold of a tile into (min, argmin) is replaced by the grid
// posterior's (pnx_grid_posterior.hip): a running log-sum-exp with weighted Welford / Chan moments.
//
//   varpro_posterior_prep_kernel   per atom what the fold reads besides the dictionary: the log-weight lw = log_prior (- 0.5 log
//                                  det N, N = M or the difference system, when the amplitudes are marginalised; -inf for a padded
//                                  atom and for one whose N is not positive definite), the non-linear values minus their row's
//                                  centre, and max_{g,j} ||phi_j||^2 (the cancellation floor)
//   varpro_posterior_kernel        one strip of 16 voxels per wave.  A lane owns one atom column and four voxel rows of a tile:
//                                  per row it keeps (m, W, sum w^2, clipped W, argmax and its amplitudes, mean_k, M2_k) with
//                                  weights relative to the running maximum m.  One log-sum-exp merge over the 16 lanes of a voxel.
//
// Lane maps of the MFMA as in pnx_grid.hip: A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom), row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "pnx_internal.hpp"
#include "pnx_varpro_pair.hpp"
#include "pnx_varpro_posterior.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

#define VPP_HIP(call)                                                                                \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) return set_error(PNX_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- per-atom inputs --------------------------------------------------------------------------------------------------------
struct VpPrepArgs {
    const double *nl;     // (n_nl, n_atoms)
    const double *lp_in;  // (n_atoms) or null
    const double *st;     // (K, kpad, gp)
    const double *cst;    // (crow, gp): M packed in its first rows
    double *theta;        // (n_nl, gp)
    double *lw;           // (gp)
    double *max_nrm;      // (1)
    int n_nl, n_atoms, gp, kpad, k, cls, marginal_amplitudes;
    double centre[PNX_MAX_PARAMS];  // per row of nl
};

// log det of the symmetric n x n (n <= 3) matrix packed in m[6] by the cofactors of its embedding [[N, 0], [0, I]]; *pd: positive
// definite by the test the variable projection's stored inverse applies (pnx_varpro.hip spd_inverse), so that exactly its
// a_hat = 0 atoms are the ones without a weight
__device__ inline double sym_logdet(int n, const double *m, bool *pd) {
    const double a00 = m[0], a10 = n > 1 ? m[1] : 0.0, a11 = n > 1 ? m[2] : 1.0;
    const double a20 = n > 2 ? m[3] : 0.0, a21 = n > 2 ? m[4] : 0.0, a22 = n > 2 ? m[5] : 1.0;
    const double c00 = a11 * a22 - a21 * a21, c10 = a21 * a20 - a10 * a22, c20 = a10 * a21 - a11 * a20;
    const double c22 = a00 * a11 - a10 * a10;
    const double det = a00 * c00 + a10 * c10 + a20 * c20;
    *pd = det > 0.0 && a00 > 0.0 && c22 > 0.0;
    return log(det);
}

template <int K> __global__ void __launch_bounds__(256) varpro_posterior_prep_kernel(const VpPrepArgs a) {
    __shared__ double red[256];
    constexpr int NM = K * (K + 1) / 2;
    const int tid = threadIdx.x;
    const double ninf = -__builtin_huge_val();
    for (int i = blockIdx.x * 256 + tid; i < a.n_nl * a.gp; i += gridDim.x * 256) {
        const int r = i / a.gp, g = i - r * a.gp;
        double c = 0.0;
#pragma unroll
        for (int q = 0; q < PNX_MAX_PARAMS; ++q)
            if (q == r) c = a.centre[q];
        a.theta[i] = g < a.n_atoms ? a.nl[(size_t)r * a.n_atoms + g] - c : 0.0;
    }
    for (int g = blockIdx.x * 256 + tid; g < a.gp; g += gridDim.x * 256) {
        double lw = ninf;
        if (g < a.n_atoms) {
            lw = a.lp_in ? a.lp_in[g] : 0.0;
            if (a.marginal_amplitudes) {
                double n[6] = {0, 0, 0, 0, 0, 0};
                int dim = K;
                if (a.cls == kVarproReduced) {  // the difference system, summed as varpro_finish_kernel sums it
                    dim = K - 1;
                    for (int k = 0; k < a.kpad; ++k) {
                        double v[K];
#pragma unroll
                        for (int j = 0; j < K; ++j) v[j] = a.st[((size_t)j * a.kpad + k) * a.gp + g];
#pragma unroll
                        for (int i = 0; i < K - 1; ++i) {
                            const double di = v[i] - v[K - 1];
#pragma unroll
                            for (int j = 0; j <= i; ++j) n[vpk(i, j)] = fma(di, v[j] - v[K - 1], n[vpk(i, j)]);
                        }
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < NM; ++q) n[q] = a.cst[(size_t)q * a.gp + g];
                }
                bool pd;
                const double ld = sym_logdet(dim, n, &pd);
                lw = pd ? fma(-0.5, ld, lw) : ninf;
            }
        }
        a.lw[g] = lw;
    }
    if (blockIdx.x) return;
    double mx = 0.0;  // squared norms, the diagonal of M: never negative, padded atoms hold 0
    for (int g = tid; g < a.gp; g += 256)
#pragma unroll
        for (int j = 0; j < K; ++j) mx = fmax(mx, a.cst[(size_t)vpk(j, j) * a.gp + g]);
    red[tid] = mx;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) *a.max_nrm = red[0];
}

size_t varpro_posterior_bytes(int n_nl, int n_atoms) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15;
    return up256((size_t)(n_nl > 0 ? n_nl : 1) * gp * 8) + up256(gp * 8) + up256((size_t)n_atoms * 8) + up256(8);
}

int varpro_posterior_prepare(const VarproDict &D, const VarproPosteriorHost &H, const double *log_prior_host, double noise_sd,
                             int marginal_amplitudes, void *buffer_d, VarproPosterior *P, hipStream_t st) {
    const VarproLayout &L = D.L;
    char *p = (char *)buffer_d;
    auto take = [&](size_t bytes) {
        void *q = p;
        p += up256(bytes);
        return (double *)q;
    };
    double *theta = take((size_t)(L.n_nl > 0 ? L.n_nl : 1) * D.gp * 8), *lw = take((size_t)D.gp * 8), *lp_in = take((size_t)D.n_atoms * 8);
    double *mx = take(8);
    if (log_prior_host) VPP_HIP(hipMemcpyAsync(lp_in, log_prior_host, (size_t)D.n_atoms * 8, hipMemcpyHostToDevice, st));  // staged as the atoms
    VpPrepArgs a;
    memset(&a, 0, sizeof(a));
    a.nl = D.nl;
    a.lp_in = log_prior_host ? lp_in : nullptr;
    a.st = D.st;
    a.cst = D.cst;
    a.theta = theta;
    a.lw = lw;
    a.max_nrm = mx;
    a.n_nl = L.n_nl;
    a.n_atoms = D.n_atoms;
    a.gp = D.gp;
    a.kpad = (D.n_b + 3) & ~3;
    a.k = L.k;
    a.cls = L.cls;
    a.marginal_amplitudes = marginal_amplitudes;
    for (int r = 0; r < D.n_free; ++r) {
        if (L.row_src[r] >= 0) a.centre[L.row_src[r]] = H.centre[r];
        P->centre[r] = H.centre[r];
    }
    const int work = (L.n_nl > 1 ? L.n_nl : 1) * D.gp;
    const dim3 grid((work + 255) / 256), block(256);
    if (L.k == 1)
        hipLaunchKernelGGL(varpro_posterior_prep_kernel<1>, grid, block, 0, st, a);
    else if (L.k == 2)
        hipLaunchKernelGGL(varpro_posterior_prep_kernel<2>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(varpro_posterior_prep_kernel<3>, grid, block, 0, st, a);
    VPP_HIP(hipGetLastError());
    P->theta = theta;
    P->lw = lw;
    P->max_nrm = mx;
    P->log_prior_norm = H.log_prior_norm;
    P->noise_sd = noise_sd;
    P->amp_l1 = H.amp_l1;
    P->marginal_amplitudes = marginal_amplitudes;
    return PNX_OK;
}

// ---- posterior --------------------------------------------------------------------------------------------------------------
// A block is four waves, one per SIMD, and a wave owns one strip of 16 voxels per pass (a block 64 voxels): the state of four
// voxel rows (4 (4 + K + 2 NMOM) doubles), the K accumulator tiles, the y fragments and the constants of the atom need the 512
// registers a lane has at one wave per SIMD (resource summary per instantiation: DESIGN.md 4.1i).  The dictionary comes through
// LDS in slabs of `width` atoms (pnx_varpro_posterior_args.hpp varpro_posterior_slab): the variable projection's image, then lw
// and the centred non-linear rows.  NS: k-steps the register file is sized for (n_b <= 4 NS).
constexpr int kVpPostWaves = 4;

struct VpPostArgs {
    const double *y;      // (n_vox, n_b)
    const double *st;     // (K kpad, gp)
    const double *cst;    // (crow, gp)
    const double *wd;     // (kpad)
    const double *nl;     // (n_nl, n_atoms)
    const double *lw;     // (gp)
    const double *theta;  // (n_nl, gp)
    const double *max_nrm;
    double *mean, *sd, *map_p;     // (n_free, n_vox); sd and map_p may be null
    int32_t *map_atom;             // (n_vox) or null
    double *logev, *ess, *cmass;   // (n_vox) or null
    long long n_vox;
    int n_b, kpad, n_atoms, gp, n_free, n_nl, width, stride;
    int noise_marginal;  // the noise is marginalised (noise_sd == 0); marginal_amplitudes is already inside lw
    int row_src[PNX_MAX_PARAMS];
    double centre[PNX_MAX_PARAMS];  // per free row
    double lo[3], hi[3];            // bounds of the linear slots (S0 class: slot K - 1 is S0)
    double tol_scale;               // 4 n_b 2^-52
    double amp2;                    // A^2
    double gain;                    // known noise: 1 / noise_sd^2;  marginalised: nu / 2
    double lp_norm;
};

// The amplitude solve and clip rule of one voxel-atom pair, vp_solve, is pnx_varpro_pair.hpp's: the marginals' kernel
// (pnx_varpro_marginal.hip) weighs a pair by the same function.
template <int NS, int K, int CLS>
__global__ void __launch_bounds__(kVpPostWaves * 64) varpro_posterior_kernel(const VpPostArgs a) {
    constexpr int NM = K * (K + 1) / 2;
    constexpr int NLIN = CLS == kVarproReduced ? K - 1 : K;  // linear slots that are parameters
    constexpr int NNL = K + 1;                               // non-linear rows a layout can have free
    constexpr int NMOM = NLIN + NNL;                         // moments: the linear slots, then the non-linear rows
    extern __shared__ double lds[];  // [K kpad][stride] | constants [2 NM][width] | lw [width] | theta [n_nl][width]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_b = a.n_b, kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lc = lds + K * kpad * stride, *llw = lc + 2 * NM * W, *lth = llw + W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kVpPostWaves - 1) / kVpPostWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double floor_nrm = a.amp2 * *a.max_nrm;
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        // A fragment of this wave's strip, as grid start loads it: rows past the end repeat the last voxel, never stored
        const long long v0 = (grp * kVpPostWaves + wave) * 16;
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
        }
        // the accumulator rows of this lane are the voxels kq + 4 r of the strip: their ||y||^2 and the floor of their cost
        double yyr[4], tol[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            yyr[r] = __shfl(yy, kq + 4 * r);
            tol[r] = a.tol_scale * (yyr[r] + floor_nrm);
        }
        double m[4], sw[4], sw2[4], cm[4], bq[4][K], mu[4][NMOM], m2[4][NMOM];
        int bg[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            m[r] = -inf;
            sw[r] = sw2[r] = cm[r] = 0.0;
            bg[r] = INT_MAX;
#pragma unroll
            for (int i = 0; i < K; ++i) bq[r][i] = 0.0;
#pragma unroll
            for (int k = 0; k < NMOM; ++k) mu[r][k] = m2[r][k] = 0.0;
        }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                for (int k = wave; k < K * kpad; k += kVpPostWaves)
                    for (int j = lane; j < wc; j += 64) lds[k * stride + j] = a.st[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < 2 * NM; k += kVpPostWaves)
                    for (int j = lane; j < wc; j += 64) lc[k * W + j] = a.cst[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < a.n_nl; k += kVpPostWaves)
                    for (int j = lane; j < wc; j += 64) lth[k * W + j] = a.theta[(size_t)k * a.gp + g0 + j];
                for (int j = threadIdx.x; j < wc; j += kVpPostWaves * 64) llw[j] = a.lw[g0 + j];
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
                // fold: this lane's atom against its four voxels.  A padded or excluded atom holds lw = -inf and contributes
                // exactly nothing; atoms arrive in ascending order, so a strict comparison keeps the lowest index among equal l.
                const int j16 = t * 16 + r16, g = g0 + j16;
                const double lwg = llw[j16];
                if (lwg > -inf) {
                    double M[NM], I[NM], th[NNL];
#pragma unroll
                    for (int q = 0; q < NM; ++q) {
                        M[q] = lc[q * W + j16];
                        I[q] = lc[(NM + q) * W + j16];
                    }
#pragma unroll
                    for (int k = 0; k < NNL; ++k) th[k] = k < a.n_nl ? lth[k * W + j16] : 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double c[K], q[K];
#pragma unroll
                        for (int i = 0; i < K; ++i) c[i] = acc[i][r];
                        bool clip;
                        const double cc = vp_solve<K, CLS>(c, M, I, a.lo, a.hi, q, &clip);
                        const double cost = fma(0.5, yyr[r], cc);
                        const double ell = a.noise_marginal ? fma(-a.gain, log(fmax(cost, tol[r])), lwg) : fma(-cost, a.gain, lwg);
                        // weights relative to the running maximum: one exp serves the new weight or the rescale of the old sums
                        const double d = ell - m[r];  // +inf for the first atom of the row
                        const bool up = d > 0.0;
                        const double e = exp(-fabs(d));
                        const double alpha = up ? e : 1.0, w = up ? 1.0 : e;
                        m[r] = up ? ell : m[r];
                        bg[r] = up ? g : bg[r];
#pragma unroll
                        for (int i = 0; i < K; ++i) bq[r][i] = up ? q[i] : bq[r][i];
                        const double wn = fma(alpha, sw[r], w);
                        const double qq = w / wn;  // wn >= 1 once an atom has been seen
                        sw[r] = wn;
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
                const double ocm = __shfl_xor(cm[r], off, 16);
                const int og = __shfl_xor(bg[r], off, 16);
                const double mn = fmax(m[r], om);
                const double fa = m[r] == mn ? 1.0 : exp(m[r] - mn);  // (-inf) - (-inf) never reaches exp
                const double fb = om == mn ? 1.0 : exp(om - mn);
                const double wa = fa * sw[r], wb = fb * ow, wn = wa + wb;
                const double qq = wn > 0.0 ? wb / wn : 0.0;
                const bool take = om > m[r] || (om == m[r] && og < bg[r]);
                bg[r] = take ? og : bg[r];
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
                sw[r] = wn;
                m[r] = mn;
            }
            const int src = kq + 4 * r;  // this voxel's row of the strip: its finite flag lives in lane `src`
            const int badv = __shfl(nf, src) | (bg[r] == INT_MAX);  // a non-finite signal, or no atom with a finite l
            const long long v = v0 + src;
            if (v < a.n_vox) {
                const double qnan = __builtin_nan("");
                const int gi = badv ? 0 : bg[r];
                if (r16 < a.n_free) {
                    int rs = 0;
                    double ctr = 0.0;
#pragma unroll
                    for (int k = 0; k < PNX_MAX_PARAMS; ++k)
                        if (r16 == k) {
                            rs = a.row_src[k];
                            ctr = a.centre[k];
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
                    a.mean[o] = badv ? qnan : mean;
                    if (a.sd) a.sd[o] = badv ? qnan : sqrt(fmax(var, 0.0));
                    if (a.map_p) a.map_p[o] = badv ? qnan : mapv;
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
    }
}

template <int K, int CLS> static int launch_post(const VpPostArgs &a, size_t lds, long long blocks, hipStream_t st) {
    if (a.kpad <= 32)
        hipLaunchKernelGGL((varpro_posterior_kernel<8, K, CLS>), dim3((unsigned)blocks), dim3(kVpPostWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((varpro_posterior_kernel<32, K, CLS>), dim3((unsigned)blocks), dim3(kVpPostWaves * 64), lds, st, a);
    VPP_HIP(hipGetLastError());
    return PNX_OK;
}

int varpro_posterior_device(const VarproDict &D, const VarproPosterior &P, int64_t n_vox, const double *y_d, double *mean_d, double *sd_d,
                            int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, double *clipped_mass_d, int cus,
                            hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const VarproLayout &L = D.L;
    const GridSlab S = varpro_posterior_slab(D.n_b, L.k);
    VpPostArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.cst = D.cst;
    a.wd = D.w;
    a.nl = D.nl;
    a.lw = P.lw;
    a.theta = P.theta;
    a.max_nrm = P.max_nrm;
    a.mean = mean_d;
    a.sd = sd_d;
    a.map_p = map_p_d;
    a.map_atom = map_atom_d;
    a.logev = log_evidence_d;
    a.ess = ess_d;
    a.cmass = clipped_mass_d;
    a.n_vox = n_vox;
    a.n_b = D.n_b;
    a.kpad = S.kpad;
    a.n_atoms = D.n_atoms;
    a.gp = D.gp;
    a.n_free = D.n_free;
    a.n_nl = L.n_nl;
    a.width = S.width < D.gp ? S.width : D.gp;
    a.stride = S.stride;
    a.noise_marginal = P.noise_sd == 0.0;
    for (int r = 0; r < PNX_MAX_PARAMS; ++r) {
        a.row_src[r] = L.row_src[r];
        a.centre[r] = P.centre[r];
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
    const long long n_strips = (n_vox + 15) / 16;
    long long blocks = (n_strips + kVpPostWaves - 1) / kVpPostWaves;
    // The variable projection's cap.  At one wave per SIMD a CU holds ONE of these blocks, so the second half of the grid starts as
    // the first half retires; the groups are spread over the blocks evenly and a slab is loaded per group whichever block takes it (a
    // one-slab dictionary: once per block),
    // so this costs no work, only a block start per CU.  Not separated by measurement from a cap of one block per CU.
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;
    if (blocks > cap) blocks = cap;
    switch (L.k * 4 + L.cls) {
    case 1 * 4 + kVarproFree: return launch_post<1, kVarproFree>(a, lds, blocks, stream);
    case 2 * 4 + kVarproFree: return launch_post<2, kVarproFree>(a, lds, blocks, stream);
    case 2 * 4 + kVarproReduced: return launch_post<2, kVarproReduced>(a, lds, blocks, stream);
    case 2 * 4 + kVarproS0: return launch_post<2, kVarproS0>(a, lds, blocks, stream);
    case 3 * 4 + kVarproFree: return launch_post<3, kVarproFree>(a, lds, blocks, stream);
    case 3 * 4 + kVarproReduced: return launch_post<3, kVarproReduced>(a, lds, blocks, stream);
    case 3 * 4 + kVarproS0: return launch_post<3, kVarproS0>(a, lds, blocks, stream);
    }
    return set_error(PNX_ERR_INVALID, "varpro posterior: no kernel for %d compartments, class %d", L.k, L.cls);
}

}  // namespace pnx
