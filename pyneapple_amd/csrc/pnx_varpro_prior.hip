// pnx_varpro_prior.hip -- the prior over the variable projection's dictionary learned from the volume itself
// (pnx_curvefit_varpro_prior_em_f64): the non-parametric maximum-likelihood mixture over the rate atoms,
// pi_g <- (1 / N) sum_v W_vg, by EM.  W_vg is the normalised weight the posterior (pnx_varpro_posterior.hip) forms per voxel-atom
// pair; an iteration needs its sum over the voxels per atom, the transposed reduction, of a matrix that never reaches memory.
// The Occam term -0.5 log det N_g belongs to the likelihood, not to the learned table: occ comes once per call from the
// posterior's prep kernel (prepared without a prior), the table lp and lw = lp + occ live in two more rows.  Two passes over the
// products c = Phi^T y, both on v_mfma_f64_16x16x4 with the posterior's lane maps, slabs, floor and vp_log_weight:
//
//   varpro_prior_init_kernel    lp = the normalised start, -inf where occ is not finite; lw = lp + occ; the admissible atoms counted
//   varpro_prior_norm_kernel    voxel-stationary, the posterior kernel without its moments, MAP state and clipped mass: per voxel
//                               row the running (m, sum w) only, L_v = m + log(sum w) to memory (NaN for a non-finite voxel, -inf
//                               for one without a finite l); per block the sum of its finite L_v and their number
//   varpro_prior_stats_kernel   the blocks' sums in block order: the log-likelihood of the volume and the voxels that take part
//   varpro_prior_acc_kernel     slab-stationary: the slab loop is the outer loop, so a block loads a dictionary slab (columns,
//                               constants, lw) once and streams its voxel groups past it.  Per tile a lane forms
//                               w = exp(l_g - L_v) for its four voxel rows, the four sums of a column meet over kq (lanes + 16,
//                               + 32) and go into a wave-private LDS row by a plain read-modify-write; at the end of a slab the
//                               block adds its four rows in wave order into partial[block][g]
//   varpro_prior_finish_kernel  per atom the blocks' sums in block order, then log pi_g and lw = log pi_g + occ in place
//
// No atomics: every sum has one order for a given grid size, so a call is reproducible bit for bit.
// Lane maps of the MFMA as in pnx_grid.hip: A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom), row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "pnx_launch.hpp"
#include "pnx_varpro_pair.hpp"
#include "pnx_varpro_prior.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kVpPriorWaves = kVarproPriorWaves;  // a block: one wave per SIMD, each with a strip of 16 voxels per group

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

static int vp_prior_blocks(int64_t n_vox, int cus) {
    const long long n_strips = (n_vox + 15) / 16;
    long long blocks = (n_strips + kVpPriorWaves - 1) / kVpPriorWaves;
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;
    if (blocks > cap) blocks = cap;
    return (int)(blocks > 1 ? blocks : 1);
}

size_t varpro_prior_bytes(int64_t n_vox, int n_atoms, int cus) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15, blocks = (size_t)vp_prior_blocks(n_vox, cus);
    return 2 * up256(gp * 8) + up256((size_t)n_atoms * 8) + up256((size_t)n_vox * 8) + up256(blocks * gp * 8) + 2 * up256(blocks * 8) +
           up256(sizeof(VarproPriorStats)) + up256(sizeof(int));
}

void varpro_prior_carve(int64_t n_vox, int n_atoms, int cus, void *buffer_d, VarproPriorWork *W) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15, blocks = (size_t)vp_prior_blocks(n_vox, cus);
    char *p = (char *)buffer_d;
    auto take = [&](size_t bytes) {
        void *q = p;
        p += up256(bytes);
        return q;
    };
    W->lp = (double *)take(gp * 8);
    W->lw = (double *)take(gp * 8);
    W->start = (double *)take((size_t)n_atoms * 8);
    W->lv = (double *)take((size_t)n_vox * 8);
    W->partial = (double *)take(blocks * gp * 8);
    W->block_l = (double *)take(blocks * 8);
    W->block_n = (long long *)take(blocks * 8);
    W->stats = (VarproPriorStats *)take(sizeof(VarproPriorStats));
    W->n_adm = (int *)take(sizeof(int));
    W->blocks = (int)blocks;
}

struct VpPriorArgs {
    const double *y;        // (n_vox, n_b)
    const double *st;       // (K kpad, gp)
    const double *cst;      // (crow, gp)
    const double *wd;       // (kpad)
    const double *occ;      // (gp) the Occam term, 0 with the profile weight; -inf for a padded atom and one whose N is not positive definite
    const double *start;    // (n_atoms)
    const double *max_nrm;
    double *lp;             // (gp) rewritten by the finish kernel
    double *lw;             // (gp) lp + occ: read by both passes, rewritten by the finish kernel
    double *lv;             // (n_vox)
    double *partial;        // (blocks, gp)
    double *block_l;        // (blocks)
    long long *block_n;     // (blocks)
    VarproPriorStats *stats;
    int *n_adm;
    long long n_vox;
    int n_b, kpad, n_atoms, gp, width, stride, noise_marginal, blocks;
    double lo[3], hi[3];  // bounds of the linear slots (S0 class: slot K - 1 is S0)
    double tol_scale;     // 4 n_b 2^-52
    double amp2;          // A^2
    double gain;          // known noise: 1 / noise_sd^2;  marginalised: nu / 2
    double alpha;         // pseudo_count
};

// ---- the table before the first pass --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) varpro_prior_init_kernel(const VpPriorArgs a) {
    __shared__ int red[256];
    const double inf = __builtin_huge_val();
    int cnt = 0;
    for (int g = threadIdx.x; g < a.gp; g += 256) {
        const double oc = a.occ[g];  // -inf for g >= n_atoms
        const double s = g < a.n_atoms ? a.start[g] : -inf;
        const bool adm = s > -inf && fabs(oc) < inf;
        a.lp[g] = adm ? s : -inf;
        a.lw[g] = adm ? s + oc : -inf;
        cnt += adm;
    }
    red[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *a.n_adm = red[0];
}

// The A fragment of a strip of 16 voxels from v0 on, as the posterior kernel loads it: weighted, rows past the end repeat the last
// voxel (never stored, never summed).  yy: ||y||^2 of voxel v0 + r16, bad: that voxel holds a non-finite value.
template <int NS> __device__ __forceinline__ void vp_prior_load_strip(const VpPriorArgs &a, long long v0, int r16, int kq, int ksteps,
                                                                     double (&yf)[NS], double &yy, int &bad) {
    const double inf = __builtin_huge_val();
    const long long v = v0 + r16;
    const double *row = a.y + (size_t)(v < a.n_vox ? v : a.n_vox - 1) * a.n_b;
    double ss = 0.0;
    int nf = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int k = 4 * s + kq;
        const double val = (s < ksteps && k < a.n_b) ? row[k] * a.wd[k] : 0.0;
        nf |= !(fabs(val) < inf);  // NaN or Inf, of the signal or through a zero sigma
        ss = fma(val, val, ss);
        yf[s] = val;
    }
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    nf |= __shfl_xor(nf, 16);
    nf |= __shfl_xor(nf, 32);
    yy = ss;
    bad = nf;
}

// One slab of the dictionary into LDS: [K kpad][stride] | constants [2 NM][W] | lw [W]; the caller holds the barriers.
template <int K> __device__ __forceinline__ void vp_prior_load_slab(const VpPriorArgs &a, double *lds, int g0, int wc, int lane, int wave) {
    constexpr int NM = K * (K + 1) / 2;
    const int W = a.width;
    double *lc = lds + K * a.kpad * a.stride, *llw = lc + 2 * NM * W;
    for (int k = wave; k < K * a.kpad; k += kVpPriorWaves)
        for (int j = lane; j < wc; j += 64) lds[k * a.stride + j] = a.st[(size_t)k * a.gp + g0 + j];
    for (int k = wave; k < 2 * NM; k += kVpPriorWaves)
        for (int j = lane; j < wc; j += 64) lc[k * W + j] = a.cst[(size_t)k * a.gp + g0 + j];
    for (int j = threadIdx.x; j < wc; j += kVpPriorWaves * 64) llw[j] = a.lw[g0 + j];
}

// The K chains of one tile: acc[i][r] = phi_i[atom 16 t + r16] . y[voxel kq + 4 r]
template <int NS, int K> __device__ __forceinline__ void vp_prior_products(const double *bp, const double (&yf)[NS], int ksteps, int kpad,
                                                                          int stride, f64x4 (&acc)[K]) {
#pragma unroll
    for (int i = 0; i < K; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s < ksteps) {
#pragma unroll
            for (int i = 0; i < K; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(yf[s], bp[(i * kpad + 4 * s) * stride], acc[i], 0, 0, 0);
        }
    }
}

// ---- normaliser pass ----------------------------------------------------------------------------------------------------------
template <int NS, int K, int CLS> __global__ void __launch_bounds__(kVpPriorWaves * 64, NS <= 8 ? 2 : 1) varpro_prior_norm_kernel(const VpPriorArgs a) {
    constexpr int NM = K * (K + 1) / 2;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    const double *lc = lds + K * kpad * stride, *llw = lc + 2 * NM * W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kVpPriorWaves - 1) / kVpPriorWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double floor_nrm = a.amp2 * *a.max_nrm;
    bool resident = false;
    double sum_l = 0.0;  // lanes with r16 == 0: the finite L_v they wrote, in the order they wrote them
    long long cnt = 0;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        const long long v0 = (grp * kVpPriorWaves + wave) * 16;
        double yf[NS], yy;
        int nf;
        vp_prior_load_strip<NS>(a, v0, r16, kq, ksteps, yf, yy, nf);
        // the accumulator rows of this lane are the voxels kq + 4 r of the strip: their ||y||^2 and the floor of their cost
        double yyr[4], tol[4], m[4], sw[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            yyr[r] = __shfl(yy, kq + 4 * r);
            tol[r] = a.tol_scale * (yyr[r] + floor_nrm);
            m[r] = -inf;
            sw[r] = 0.0;
        }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                vp_prior_load_slab<K>(a, lds, g0, wc, lane, wave);
                __syncthreads();
                resident = n_slabs == 1;
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc[K];
                vp_prior_products<NS, K>(lds + kq * stride + t * 16 + r16, yf, ksteps, kpad, stride, acc);
                // a padded or inadmissible atom holds lw = -inf and contributes exactly nothing
                const int j16 = t * 16 + r16;
                const double lwg = llw[j16];
                if (lwg > -inf) {
                    double M[NM], I[NM];
#pragma unroll
                    for (int q = 0; q < NM; ++q) {
                        M[q] = lc[q * W + j16];
                        I[q] = lc[(NM + q) * W + j16];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double c[K];
#pragma unroll
                        for (int i = 0; i < K; ++i) c[i] = acc[i][r];
                        const double ell = vp_log_weight<K, CLS>(c, M, I, a.lo, a.hi, yyr[r], tol[r], lwg, a.gain, a.noise_marginal);
                        // the posterior's running log-sum-exp: one exp serves the new weight or the rescale of the old sum
                        const double d = ell - m[r];  // +inf for the first atom of the row
                        const bool up = d > 0.0;
                        const double e = exp(-fabs(d));
                        sw[r] = fma(up ? e : 1.0, sw[r], up ? 1.0 : e);
                        m[r] = up ? ell : m[r];
                    }
                }
            }
        }
        // one log-sum-exp merge over the 16 lanes (atoms modulo 16) that share a voxel; a lane that saw no admissible atom holds
        // m = -inf, sum = 0
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) {
                const double om = __shfl_xor(m[r], off, 16), ow = __shfl_xor(sw[r], off, 16);
                const double mn = fmax(m[r], om);
                const double fa = m[r] == mn ? 1.0 : exp(m[r] - mn);  // (-inf) - (-inf) never reaches exp
                const double fb = om == mn ? 1.0 : exp(om - mn);
                sw[r] = fa * sw[r] + fb * ow;
                m[r] = mn;
            }
            const int src = kq + 4 * r;  // this voxel's row of the strip: its finite flag lives in lane `src`
            const int badv = __shfl(nf, src);
            const long long v = v0 + src;
            if (r16 == 0 && v < a.n_vox) {
                const double L = badv ? __builtin_nan("") : m[r] + log(sw[r]);  // -inf without an atom of finite l
                a.lv[v] = L;
                if (fabs(L) < inf) {
                    sum_l += L;
                    cnt += 1;
                }
            }
        }
    }
    // the block's share of the log-likelihood: its 16 writing lanes in (wave, kq) order
    __syncthreads();  // the slab is dead
    long long *lcnt = reinterpret_cast<long long *>(lds + kVpPriorWaves * 4);
    if (r16 == 0) {
        lds[wave * 4 + kq] = sum_l;
        lcnt[wave * 4 + kq] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        long long n = 0;
        for (int i = 0; i < kVpPriorWaves * 4; ++i) {
            s += lds[i];
            n += lcnt[i];
        }
        a.block_l[blockIdx.x] = s;
        a.block_n[blockIdx.x] = n;
    }
}

__global__ void __launch_bounds__(64) varpro_prior_stats_kernel(const VpPriorArgs a) {
    if (threadIdx.x) return;
    double s = 0.0;
    long long n = 0;
    for (int b = 0; b < a.blocks; ++b) {
        s += a.block_l[b];
        n += a.block_n[b];
    }
    a.stats->loglik = s;
    a.stats->n_finite = n;
}

// ---- accumulate pass ----------------------------------------------------------------------------------------------------------
// LDS: the slab as above, then acc[kVpPriorWaves][W] in the place of the posterior's centred non-linear rows.  A wave adds into its
// own row only, in program order; the rows meet at the end of the slab behind a barrier.
template <int NS, int K, int CLS> __global__ void __launch_bounds__(kVpPriorWaves * 64, NS <= 8 ? 2 : 1) varpro_prior_acc_kernel(const VpPriorArgs a) {
    constexpr int NM = K * (K + 1) / 2;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    const double *lc = lds + K * kpad * stride, *llw = lc + 2 * NM * W;
    double *lacc = lds + K * kpad * stride + (2 * NM + 1) * W, *mine = lacc + wave * W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kVpPriorWaves - 1) / kVpPriorWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double floor_nrm = a.amp2 * *a.max_nrm;
    for (int slab = 0; slab < n_slabs; ++slab) {
        const int g0 = slab * W;
        const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
        __syncthreads();  // the previous slab's rows have been written out
        vp_prior_load_slab<K>(a, lds, g0, wc, lane, wave);
        for (int j = lane; j < wc; j += 64) mine[j] = 0.0;
        __syncthreads();
        for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
            const long long v0 = (grp * kVpPriorWaves + wave) * 16;
            double yf[NS], yy;
            int nf;
            vp_prior_load_strip<NS>(a, v0, r16, kq, ksteps, yf, yy, nf);
            double yyr[4], tol[4], lv[4];
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                yyr[r] = __shfl(yy, kq + 4 * r);
                tol[r] = a.tol_scale * (yyr[r] + floor_nrm);
                const long long v = v0 + kq + 4 * r;
                lv[r] = v < a.n_vox ? a.lv[v] : __builtin_nan("");
                ok[r] = fabs(lv[r]) < inf;  // a voxel past the end or one that takes no part weighs nothing
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc[K];
                vp_prior_products<NS, K>(lds + kq * stride + t * 16 + r16, yf, ksteps, kpad, stride, acc);
                const int j16 = t * 16 + r16;
                const double lwg = llw[j16];
                double sum = 0.0;  // this atom's weights over the lane's four voxels; exactly 0 for a padded or inadmissible atom
                if (lwg > -inf) {
                    double M[NM], I[NM];
#pragma unroll
                    for (int q = 0; q < NM; ++q) {
                        M[q] = lc[q * W + j16];
                        I[q] = lc[(NM + q) * W + j16];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double c[K];
#pragma unroll
                        for (int i = 0; i < K; ++i) c[i] = acc[i][r];
                        const double ell = vp_log_weight<K, CLS>(c, M, I, a.lo, a.hi, yyr[r], tol[r], lwg, a.gain, a.noise_marginal);
                        sum += ok[r] ? exp(ell - lv[r]) : 0.0;
                    }
                }
                sum += __shfl_xor(sum, 16);
                sum += __shfl_xor(sum, 32);
                if (kq == 0) mine[j16] += sum;
            }
        }
        __syncthreads();
        double *dst = a.partial + (size_t)blockIdx.x * a.gp + g0;
        for (int j = threadIdx.x; j < wc; j += kVpPriorWaves * 64)
            dst[j] = ((lacc[j] + lacc[W + j]) + lacc[2 * W + j]) + lacc[3 * W + j];
    }
}

__global__ void __launch_bounds__(256) varpro_prior_finish_kernel(const VpPriorArgs a) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= a.gp) return;
    double s = 0.0;
    for (int b = 0; b < a.blocks; ++b) s += a.partial[(size_t)b * a.gp + g];
    const double inf = __builtin_huge_val();
    const double pi = (s + a.alpha) / ((double)a.stats->n_finite + a.alpha * (double)*a.n_adm);
    const double lp = (a.lp[g] > -inf && pi > 0.0) ? log(pi) : -inf;  // an inadmissible atom stays at -inf (padded atoms too)
    a.lp[g] = lp;
    a.lw[g] = lp > -inf ? lp + a.occ[g] : -inf;  // the determinant is not recomputed: occ is the call's
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static VpPriorArgs vp_prior_args(const VarproDict &D, const VarproPosterior &P, int64_t n_vox, const double *y_d, const VarproPriorWork &W) {
    const VarproLayout &L = D.L;
    const GridSlab S = varpro_prior_slab(D.n_b, L.k);
    VpPriorArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.cst = D.cst;
    a.wd = D.w;
    a.occ = P.lw;  // prepared without a prior
    a.start = W.start;
    a.max_nrm = P.max_nrm;
    a.lp = W.lp;
    a.lw = W.lw;
    a.lv = W.lv;
    a.partial = W.partial;
    a.block_l = W.block_l;
    a.block_n = W.block_n;
    a.stats = W.stats;
    a.n_adm = W.n_adm;
    a.n_vox = n_vox;
    a.n_b = D.n_b;
    a.kpad = S.kpad;
    a.n_atoms = D.n_atoms;
    a.gp = D.gp;
    a.width = S.width < D.gp ? S.width : D.gp;
    a.stride = S.stride;
    a.noise_marginal = P.noise_sd == 0.0;
    a.blocks = W.blocks;
    for (int j = 0; j < 3; ++j) {
        a.lo[j] = L.lin_lo[j];
        a.hi[j] = L.lin_hi[j];
    }
    a.tol_scale = 4.0 * D.n_b * 0x1p-52;
    a.amp2 = P.amp_l1 * P.amp_l1;
    a.gain = a.noise_marginal ? 0.5 * (D.n_b - L.n_lin) : 1.0 / (P.noise_sd * P.noise_sd);
    return a;
}

template <int K, int CLS> static void launch_vp_norm(const VpPriorArgs &a, size_t lds, hipStream_t st) {
    if (a.kpad <= 32)
        hipLaunchKernelGGL((varpro_prior_norm_kernel<8, K, CLS>), dim3((unsigned)a.blocks), dim3(kVpPriorWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((varpro_prior_norm_kernel<32, K, CLS>), dim3((unsigned)a.blocks), dim3(kVpPriorWaves * 64), lds, st, a);
}

template <int K, int CLS> static void launch_vp_acc(const VpPriorArgs &a, size_t lds, hipStream_t st) {
    if (a.kpad <= 32)
        hipLaunchKernelGGL((varpro_prior_acc_kernel<8, K, CLS>), dim3((unsigned)a.blocks), dim3(kVpPriorWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((varpro_prior_acc_kernel<32, K, CLS>), dim3((unsigned)a.blocks), dim3(kVpPriorWaves * 64), lds, st, a);
}

int varpro_prior_begin(const VarproDict &D, const VarproPosterior &P, const double *start_host, const VarproPriorWork &W, hipStream_t stream) {
    // the copy from pageable memory is staged before the call returns (as the atoms of the dictionary)
    PNX_HIP(hipMemcpyAsync(W.start, start_host, (size_t)D.n_atoms * sizeof(double), hipMemcpyHostToDevice, stream));
    const VpPriorArgs a = vp_prior_args(D, P, 0, nullptr, W);
    hipLaunchKernelGGL(varpro_prior_init_kernel, dim3(1), dim3(256), 0, stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

int varpro_prior_normalise(const VarproDict &D, const VarproPosterior &P, int64_t n_vox, const double *y_d, const VarproPriorWork &W,
                           hipStream_t stream) {
    const VarproLayout &L = D.L;
    const VpPriorArgs a = vp_prior_args(D, P, n_vox, y_d, W);
    const size_t lds = (size_t)varpro_prior_slab(D.n_b, L.k).lds_doubles * sizeof(double);  // <= 64 KB
    switch (L.k * 4 + L.cls) {
    case 1 * 4 + kVarproFree: launch_vp_norm<1, kVarproFree>(a, lds, stream); break;
    case 2 * 4 + kVarproFree: launch_vp_norm<2, kVarproFree>(a, lds, stream); break;
    case 2 * 4 + kVarproReduced: launch_vp_norm<2, kVarproReduced>(a, lds, stream); break;
    case 2 * 4 + kVarproS0: launch_vp_norm<2, kVarproS0>(a, lds, stream); break;
    case 3 * 4 + kVarproFree: launch_vp_norm<3, kVarproFree>(a, lds, stream); break;
    case 3 * 4 + kVarproReduced: launch_vp_norm<3, kVarproReduced>(a, lds, stream); break;
    case 3 * 4 + kVarproS0: launch_vp_norm<3, kVarproS0>(a, lds, stream); break;
    default: return set_error(PNX_ERR_INVALID, "varpro prior: no kernel for %d compartments, class %d", L.k, L.cls);
    }
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(varpro_prior_stats_kernel, dim3(1), dim3(64), 0, stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

int varpro_prior_update(const VarproDict &D, const VarproPosterior &P, int64_t n_vox, const double *y_d, const VarproPriorWork &W,
                        double pseudo_count, hipStream_t stream) {
    const VarproLayout &L = D.L;
    VpPriorArgs a = vp_prior_args(D, P, n_vox, y_d, W);
    a.alpha = pseudo_count;
    const size_t lds = (size_t)varpro_prior_slab(D.n_b, L.k).lds_doubles * sizeof(double);
    switch (L.k * 4 + L.cls) {
    case 1 * 4 + kVarproFree: launch_vp_acc<1, kVarproFree>(a, lds, stream); break;
    case 2 * 4 + kVarproFree: launch_vp_acc<2, kVarproFree>(a, lds, stream); break;
    case 2 * 4 + kVarproReduced: launch_vp_acc<2, kVarproReduced>(a, lds, stream); break;
    case 2 * 4 + kVarproS0: launch_vp_acc<2, kVarproS0>(a, lds, stream); break;
    case 3 * 4 + kVarproFree: launch_vp_acc<3, kVarproFree>(a, lds, stream); break;
    case 3 * 4 + kVarproReduced: launch_vp_acc<3, kVarproReduced>(a, lds, stream); break;
    case 3 * 4 + kVarproS0: launch_vp_acc<3, kVarproS0>(a, lds, stream); break;
    default: return set_error(PNX_ERR_INVALID, "varpro prior: no kernel for %d compartments, class %d", L.k, L.cls);
    }
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(varpro_prior_finish_kernel, dim3((unsigned)((D.gp + 255) / 256)), dim3(256), 0, stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

}  // namespace pnx
