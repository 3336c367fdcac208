// pnx_varpro_class.hip -- one prior row per segmentation label over the variable projection's dictionary
// (pnx_curvefit_varpro_posterior_classes_f64 and pnx_curvefit_varpro_prior_em_classes_f64).  The log-weight of a
// voxel-atom pair is lw[labels[v], g] = log_prior[labels[v], g] + occ_g: no longer a property of the atom column alone.  The
// kernels are the posterior's and the EM's (pnx_varpro_posterior.hip, pnx_varpro_prior.hip: the same K chains on
// v_mfma_f64_16x16x4, lane maps, dictionary slabs, vp_solve / vp_log_weight, floor and fold, expression for expression, so a
// voxel's sums are the bytes the unlabelled kernels give under its row); in LDS the slab carries n_classes rows of lw, and a lane
// looks its four voxel rows up under their own classes.  The Occam term occ_g = -0.5 log det N_g is shared by all classes: it is the
// posterior's prep kernel's lw under a null prior, built once per call.
//
//   varpro_class_table_kernel      per class the row lp (the host table or 0, -inf where occ is not finite and for padded atoms),
//                                  lw = lp + occ and the number of admissible atoms
//   varpro_class_posterior_kernel  varpro_posterior_kernel with the row of each voxel; a label outside [0, n_classes) makes the
//                                  voxel a non-finite one
//   varpro_class_norm_kernel       voxel-stationary: L_v under the voxel's row to memory, NaN for a voxel that takes no part
//   varpro_class_sums_kernel       per block and class the sum of the finite L_v of the block's voxels, each lane slot of the
//   varpro_class_stats_kernel      normaliser's grid in its own order, then the blocks in block order, then the classes in class order
//   varpro_class_acc_kernel        slab-stationary: per tile a lane forms its four weights; a wave-uniform loop over the classes
//                                  present in the strip selects the rows of one class, the four sums of a column meet over kq and go
//                                  into the wave's private LDS row OF THAT CLASS by a plain read-modify-write; at the end of a slab
//                                  the block adds its four rows per class in wave order
//   varpro_class_finish_kernel     per class and atom the blocks' sums in block order, then log pi_cg and lw in place
//
// No atomics: every sum has one order for a given grid size, so a call is reproducible bit for bit; W never reaches memory.  A
// pair at -inf is skipped before any arithmetic, so (-inf) - (-inf) is never formed.
// Lane maps of the MFMA as in pnx_grid.hip: A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom), row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "pnx_launch.hpp"
#include "pnx_varpro_class.hpp"
#include "pnx_varpro_pair.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kVpClassWaves = kVarproPriorWaves;  // a block: one wave per SIMD, each with a strip of 16 voxels per group

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

static int vp_class_blocks(int64_t n_vox, int cus) {
    const long long n_strips = (n_vox + 15) / 16;
    long long blocks = (n_strips + kVpClassWaves - 1) / kVpClassWaves;
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;
    if (blocks > cap) blocks = cap;
    return (int)(blocks > 1 ? blocks : 1);
}

// ---- the tables -----------------------------------------------------------------------------------------------------------------
// One block per class.  occ: the posterior's lw under a null prior, -inf for a padded atom and one whose N is not positive definite.
__global__ void __launch_bounds__(256) varpro_class_table_kernel(const double *lp_in, const double *occ, double *lp, double *lw, int *n_adm,
                                                                 int n_atoms, int gp) {
    __shared__ int red[256];
    const double inf = __builtin_huge_val();
    const int c = blockIdx.x;
    int cnt = 0;
    for (int g = threadIdx.x; g < gp; g += 256) {
        const double oc = occ[g];  // -inf for g >= n_atoms
        const double s = g < n_atoms ? (lp_in ? lp_in[(size_t)c * n_atoms + g] : 0.0) : -inf;
        const bool adm = s > -inf && fabs(oc) < inf;
        lp[(size_t)c * gp + g] = adm ? s : -inf;
        lw[(size_t)c * gp + g] = adm ? s + oc : -inf;
        cnt += adm;
    }
    red[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) n_adm[c] = red[0];
}

size_t varpro_class_table_bytes(int n_classes, int n_atoms) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15;
    return 2 * up256((size_t)n_classes * gp * 8) + up256((size_t)n_classes * n_atoms * 8) + up256(kGridMaxClasses * sizeof(int));
}

int varpro_class_table_prepare(const VarproDict &D, const VarproPosterior &P, const GridClassHost &K, int n_classes,
                               const double *log_prior_host, void *buffer_d, VarproClassTable *T, hipStream_t st) {
    char *p = (char *)buffer_d;
    auto take = [&](size_t bytes) {
        void *q = p;
        p += up256(bytes);
        return q;
    };
    T->lp = (double *)take((size_t)n_classes * D.gp * 8);
    T->lw = (double *)take((size_t)n_classes * D.gp * 8);
    T->lp_in = (double *)take((size_t)n_classes * D.n_atoms * 8);
    T->n_adm = (int *)take(kGridMaxClasses * sizeof(int));
    T->n_classes = n_classes;
    for (int c = 0; c < n_classes; ++c) T->norm[c] = K.norm[c];
    if (log_prior_host)
        PNX_HIP(hipMemcpyAsync(T->lp_in, log_prior_host, (size_t)n_classes * D.n_atoms * 8, hipMemcpyHostToDevice, st));  // staged as the atoms
    hipLaunchKernelGGL(varpro_class_table_kernel, dim3((unsigned)n_classes), dim3(256), 0, st, log_prior_host ? T->lp_in : nullptr, P.lw, T->lp,
                       T->lw, T->n_adm, D.n_atoms, D.gp);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

// ---- shared pieces ------------------------------------------------------------------------------------------------------------
struct VpClassArgs {
    const double *y;               // (n_vox, n_b)
    const int32_t *labels;         // (n_vox)
    const double *st;              // (K kpad, gp)
    const double *cst;             // (crow, gp)
    const double *wd;              // (kpad)
    const double *nl;              // (n_nl, n_atoms), the posterior only
    const double *theta;           // (n_nl, gp), the posterior only
    const double *occ;             // (gp) the Occam term, 0 with the profile weight
    const double *max_nrm;
    double *lp;                    // (n_classes, gp) rewritten by the finish kernel
    double *lw;                    // (n_classes, gp) lp + occ: read by every pass, rewritten by the finish kernel
    const int *n_adm;              // (n_classes)
    double *mean, *sd, *map_p;     // (n_free, n_vox); sd and map_p may be null
    int32_t *map_atom;             // (n_vox) or null
    double *logev, *ess, *cmass;   // (n_vox) or null
    double *lv;                    // (n_vox)
    double *partial;               // (blocks, n_classes, gp)
    double *block_l;               // (blocks, n_classes)
    long long *block_n;            // (blocks, n_classes)
    VarproClassStats *stats;
    long long n_vox;
    int n_b, kpad, n_atoms, gp, n_free, n_nl, width, stride, noise_marginal, blocks, n_classes;
    int row_src[PNX_MAX_PARAMS];
    double centre[PNX_MAX_PARAMS];  // per free row
    double lo[3], hi[3];            // bounds of the linear slots (S0 class: slot K - 1 is S0)
    double tol_scale;               // 4 n_b 2^-52
    double amp2;                    // A^2
    double gain;                    // known noise: 1 / noise_sd^2;  marginalised: nu / 2
    double alpha;                   // pseudo_count
    double lp_norm[kGridMaxClasses];
};

// The A fragment of a strip of 16 voxels from v0 on, as the posterior kernel loads it: weighted, rows past the end repeat the last
// voxel (never stored, never summed).  yy: ||y||^2 of voxel v0 + r16; bad: that voxel holds a non-finite value or a label outside
// [0, n_classes); cls: its class, 0 when bad.
template <int NS> __device__ __forceinline__ void vp_class_load_strip(const VpClassArgs &a, long long v0, int r16, int kq, int ksteps,
                                                                     double (&yf)[NS], double &yy, int &bad, int &cls) {
    const double inf = __builtin_huge_val();
    const long long v = v0 + r16;
    const size_t vi = (size_t)(v < a.n_vox ? v : a.n_vox - 1);
    const double *row = a.y + vi * a.n_b;
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
    const int lab = a.labels[vi];
    const int out = lab < 0 || lab >= a.n_classes;
    yy = ss;
    bad = nf | out;
    cls = out ? 0 : lab;
}

// One slab of the dictionary into LDS: [K kpad][stride] | constants [2 NM][W] | lw [n_classes][W]; the caller holds the barriers.
template <int K> __device__ __forceinline__ void vp_class_load_slab(const VpClassArgs &a, double *lds, int g0, int wc, int lane, int wave) {
    constexpr int NM = K * (K + 1) / 2;
    const int W = a.width;
    double *lc = lds + K * a.kpad * a.stride, *llw = lc + 2 * NM * W;
    for (int k = wave; k < K * a.kpad; k += kVpClassWaves)
        for (int j = lane; j < wc; j += 64) lds[k * a.stride + j] = a.st[(size_t)k * a.gp + g0 + j];
    for (int k = wave; k < 2 * NM; k += kVpClassWaves)
        for (int j = lane; j < wc; j += 64) lc[k * W + j] = a.cst[(size_t)k * a.gp + g0 + j];
    for (int c = wave; c < a.n_classes; c += kVpClassWaves)
        for (int j = lane; j < wc; j += 64) llw[c * W + j] = a.lw[(size_t)c * a.gp + g0 + j];
}

// The K chains of one tile: acc[i][r] = phi_i[atom 16 t + r16] . y[voxel kq + 4 r]
template <int NS, int K> __device__ __forceinline__ void vp_class_products(const double *bp, const double (&yf)[NS], int ksteps, int kpad,
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

// ---- posterior ----------------------------------------------------------------------------------------------------------------
// LDS: the slab as above, then theta [n_nl][W].  NS, K, CLS as in varpro_posterior_kernel; its register budget (one wave per SIMD)
// gains the class offset of each of the lane's four voxel rows and nothing else.
template <int NS, int K, int CLS>
__global__ void __launch_bounds__(kVpClassWaves * 64) varpro_class_posterior_kernel(const VpClassArgs a) {
    constexpr int NM = K * (K + 1) / 2;
    constexpr int NLIN = CLS == kVarproReduced ? K - 1 : K;  // linear slots that are parameters
    constexpr int NNL = K + 1;                               // non-linear rows a layout can have free
    constexpr int NMOM = NLIN + NNL;                         // moments: the linear slots, then the non-linear rows
    constexpr int NH = NS > 8 ? (K == 3 ? 4 : 2) : 1, RH = 4 / NH;  // sweeps over the dictionary per strip, rows of a lane per sweep
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lc = lds + K * kpad * stride, *llw = lc + 2 * NM * W, *lth = llw + a.n_classes * W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kVpClassWaves - 1) / kVpClassWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double floor_nrm = a.amp2 * *a.max_nrm;
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        const long long v0 = (grp * kVpClassWaves + wave) * 16;
        double yf[NS], yy;
        int nf, lab;
        vp_class_load_strip<NS>(a, v0, r16, kq, ksteps, yf, yy, nf, lab);
        // the accumulator rows of this lane are the voxels kq + 4 r of the strip.  NH sweeps over the dictionary, each with the fold
        // state of RH of the lane's four rows: one sweep at NS = 8; two (four at K = 3) at NS = 32, where the 32 y fragments leave
        // no room for the state of four rows (the products of the other rows are formed again: the price of no scratch).
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        // of this sweep's rows: their ||y||^2, the floor of their cost, their class
        double yyr[RH], tol[RH];
        int cls[RH];
#pragma unroll
        for (int r = 0; r < RH; ++r) {
            yyr[r] = __shfl(yy, kq + 4 * (h * RH + r));
            tol[r] = a.tol_scale * (yyr[r] + floor_nrm);
            cls[r] = __shfl(lab, kq + 4 * (h * RH + r)) * W;  // the offset of the class's row in llw
        }
        double m[RH], sw[RH], sw2[RH], cm[RH], bq[RH][K], mu[RH][NMOM], m2[RH][NMOM];
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
        }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                vp_class_load_slab<K>(a, lds, g0, wc, lane, wave);
                for (int k = wave; k < a.n_nl; k += kVpClassWaves)
                    for (int j = lane; j < wc; j += 64) lth[k * W + j] = a.theta[(size_t)k * a.gp + g0 + j];
                __syncthreads();
                resident = n_slabs == 1;
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc[K];
                vp_class_products<NS, K>(lds + kq * stride + t * 16 + r16, yf, ksteps, kpad, stride, acc);
                // fold: this lane's atom against its four voxels, each under its own row.  A padded atom holds -inf in every row,
                // an excluded pair in its own: either contributes exactly nothing.  Atoms arrive in ascending order, so a strict
                // comparison keeps the lowest index among equal l.
                const int j16 = t * 16 + r16, g = g0 + j16;
                double M[NM], I[NM], th[NNL];
#pragma unroll
                for (int q = 0; q < NM; ++q) {
                    M[q] = lc[q * W + j16];
                    I[q] = lc[(NM + q) * W + j16];
                }
#pragma unroll
                for (int k = 0; k < NNL; ++k) th[k] = k < a.n_nl ? lth[k * W + j16] : 0.0;
#pragma unroll
                for (int r = 0; r < RH; ++r) {
                    const double lwg = llw[cls[r] + j16];
                    if (lwg > -inf) {
                        double c[K], q[K];
#pragma unroll
                        for (int i = 0; i < K; ++i) c[i] = acc[i][h * RH + r];
                        bool clip;
                        const double cc = vp_solve<K, CLS>(c, M, I, a.lo, a.hi, q, &clip);
                        const double cost = fma(0.5, yyr[r], cc);
                        const double ell = a.noise_marginal ? fma(-a.gain, log(fmax(cost, tol[r])), lwg) : fma(-cost, a.gain, lwg);
                        // weights relative to the running maximum: one exp serves the new weight or the rescale of the old sums
                        const double d = ell - m[r];  // +inf for the first admissible atom of the row, however late it comes
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
        for (int r = 0; r < RH; ++r) {
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
            const int src = kq + 4 * (h * RH + r);  // this voxel's row of the strip: its flag and class live in lane `src`
            const int badv = __shfl(nf, src) | (bg[r] == INT_MAX);  // a non-finite signal, a label out of range, or no atom with a finite l
            const int cv = __shfl(lab, src);
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
                    if (a.logev) a.logev[v] = badv ? qnan : m[r] + log(sw[r]) - a.lp_norm[cv];
                } else if (r16 == 10) {
                    if (a.ess) a.ess[v] = badv ? qnan : sw[r] * sw[r] / sw2[r];
                } else if (r16 == 11) {
                    if (a.cmass) a.cmass[v] = badv ? qnan : fmin(cm[r] / sw[r], 1.0);
                }
            }
        }
      }
    }
}

// ---- normaliser pass ----------------------------------------------------------------------------------------------------------
template <int NS, int K, int CLS>
__global__ void __launch_bounds__(kVpClassWaves * 64, NS <= 8 ? 2 : 1) varpro_class_norm_kernel(const VpClassArgs a) {
    constexpr int NM = K * (K + 1) / 2;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    const double *lc = lds + K * kpad * stride, *llw = lc + 2 * NM * W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kVpClassWaves - 1) / kVpClassWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double floor_nrm = a.amp2 * *a.max_nrm;
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        const long long v0 = (grp * kVpClassWaves + wave) * 16;
        double yf[NS], yy;
        int nf, lab;
        vp_class_load_strip<NS>(a, v0, r16, kq, ksteps, yf, yy, nf, lab);
        double yyr[4], tol[4], m[4], sw[4];
        int cls[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            yyr[r] = __shfl(yy, kq + 4 * r);
            tol[r] = a.tol_scale * (yyr[r] + floor_nrm);
            cls[r] = __shfl(lab, kq + 4 * r) * W;
            m[r] = -inf;
            sw[r] = 0.0;
        }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                vp_class_load_slab<K>(a, lds, g0, wc, lane, wave);
                __syncthreads();
                resident = n_slabs == 1;
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc[K];
                vp_class_products<NS, K>(lds + kq * stride + t * 16 + r16, yf, ksteps, kpad, stride, acc);
                const int j16 = t * 16 + r16;
                double M[NM], I[NM];
#pragma unroll
                for (int q = 0; q < NM; ++q) {
                    M[q] = lc[q * W + j16];
                    I[q] = lc[(NM + q) * W + j16];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double lwg = llw[cls[r] + j16];
                    if (lwg > -inf) {  // a padded atom or an excluded pair contributes exactly nothing
                        double c[K];
#pragma unroll
                        for (int i = 0; i < K; ++i) c[i] = acc[i][r];
                        const double ell = vp_log_weight<K, CLS>(c, M, I, a.lo, a.hi, yyr[r], tol[r], lwg, a.gain, a.noise_marginal);
                        // the posterior's running log-sum-exp: one exp serves the new weight or the rescale of the old sum
                        const double d = ell - m[r];  // +inf for the first admissible atom of the row
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
            const int src = kq + 4 * r;
            const int badv = __shfl(nf, src);
            const long long v = v0 + src;
            if (r16 == 0 && v < a.n_vox) a.lv[v] = badv ? __builtin_nan("") : m[r] + log(sw[r]);  // -inf without an atom of finite l
        }
    }
}

// The log-likelihood per class, in the order the unlabelled normaliser sums it: thread (c, slot) walks the voxels that lane
// slot = 4 wave + kq of block blockIdx.x wrote above -- groups ascending, the four rows ascending -- and keeps those of class c;
// then per class the 16 slots in slot order.
__global__ void __launch_bounds__(256) varpro_class_sums_kernel(const VpClassArgs a) {
    __shared__ double ls[256];
    __shared__ long long ln[256];
    const int slot = threadIdx.x & 15, c = threadIdx.x >> 4;
    const int wave = slot >> 2, kq = slot & 3;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kVpClassWaves - 1) / kVpClassWaves;
    const double inf = __builtin_huge_val();
    double s = 0.0;
    long long n = 0;
    if (c < a.n_classes) {
        for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
            const long long v0 = (grp * kVpClassWaves + wave) * 16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long v = v0 + kq + 4 * r;
                if (v < a.n_vox && a.labels[v] == c) {
                    const double L = a.lv[v];
                    if (fabs(L) < inf) {
                        s += L;
                        n += 1;
                    }
                }
            }
        }
    }
    ls[threadIdx.x] = s;
    ln[threadIdx.x] = n;
    __syncthreads();
    if ((int)threadIdx.x < a.n_classes) {
        double bs = 0.0;
        long long bn = 0;
        for (int i = 0; i < 16; ++i) {
            bs += ls[threadIdx.x * 16 + i];
            bn += ln[threadIdx.x * 16 + i];
        }
        a.block_l[(size_t)blockIdx.x * a.n_classes + threadIdx.x] = bs;
        a.block_n[(size_t)blockIdx.x * a.n_classes + threadIdx.x] = bn;
    }
}

__global__ void __launch_bounds__(64) varpro_class_stats_kernel(const VpClassArgs a) {
    __shared__ double ls[kGridMaxClasses];
    const int c = threadIdx.x;
    if (c < a.n_classes) {
        double s = 0.0;
        long long n = 0;
        for (int b = 0; b < a.blocks; ++b) {
            s += a.block_l[(size_t)b * a.n_classes + c];
            n += a.block_n[(size_t)b * a.n_classes + c];
        }
        a.stats->loglik_class[c] = s;
        a.stats->n_finite[c] = n;
        ls[c] = s;
    }
    __syncthreads();
    if (c == 0) {
        double tot = ls[0];
        for (int i = 1; i < a.n_classes; ++i) tot += ls[i];
        a.stats->loglik = tot;
    }
}

// ---- accumulate pass ----------------------------------------------------------------------------------------------------------
// LDS: the slab as above, then acc[kVpClassWaves][n_classes][W].  A wave adds into its own rows only, in program order; the rows
// meet at the end of the slab behind a barrier.
template <int NS, int K, int CLS>
__global__ void __launch_bounds__(kVpClassWaves * 64, NS <= 8 ? 2 : 1) varpro_class_acc_kernel(const VpClassArgs a) {
    constexpr int NM = K * (K + 1) / 2;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width, C = a.n_classes;
    const double *lc = lds + K * kpad * stride, *llw = lc + 2 * NM * W;
    double *lacc = lds + K * kpad * stride + (2 * NM + C) * W, *mine = lacc + wave * C * W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kVpClassWaves - 1) / kVpClassWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double floor_nrm = a.amp2 * *a.max_nrm;
    for (int slab = 0; slab < n_slabs; ++slab) {
        const int g0 = slab * W;
        const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
        __syncthreads();  // the previous slab's rows have been written out
        vp_class_load_slab<K>(a, lds, g0, wc, lane, wave);
        for (int c = 0; c < C; ++c)
            for (int j = lane; j < wc; j += 64) mine[c * W + j] = 0.0;
        __syncthreads();
        for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
            const long long v0 = (grp * kVpClassWaves + wave) * 16;
            double yf[NS], yy;
            int nf, lab;
            vp_class_load_strip<NS>(a, v0, r16, kq, ksteps, yf, yy, nf, lab);
            // the classes present in the strip, as a wave-uniform bit mask: voxels past the end and bad ones aside
            unsigned present = (v0 + r16 < a.n_vox && !nf) ? 1u << lab : 0u;
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) present |= __shfl_xor(present, off, 16);
            present = __builtin_amdgcn_readfirstlane(present);
            double yyr[4], tol[4], lv[4];
            int cls[4];
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                yyr[r] = __shfl(yy, kq + 4 * r);
                tol[r] = a.tol_scale * (yyr[r] + floor_nrm);
                cls[r] = __shfl(lab, kq + 4 * r);
                const long long v = v0 + kq + 4 * r;
                lv[r] = v < a.n_vox ? a.lv[v] : __builtin_nan("");
                ok[r] = fabs(lv[r]) < inf;  // a voxel past the end or without a finite L_v weighs nothing
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc[K];
                vp_class_products<NS, K>(lds + kq * stride + t * 16 + r16, yf, ksteps, kpad, stride, acc);
                const int j16 = t * 16 + r16;
                double M[NM], I[NM];
#pragma unroll
                for (int q = 0; q < NM; ++q) {
                    M[q] = lc[q * W + j16];
                    I[q] = lc[(NM + q) * W + j16];
                }
                double w[4];  // this atom's weight on the lane's four voxels; exactly 0 for a padded atom or an excluded pair
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double lwg = llw[cls[r] * W + j16];
                    w[r] = 0.0;
                    if (ok[r] && lwg > -inf) {
                        double c[K];
#pragma unroll
                        for (int i = 0; i < K; ++i) c[i] = acc[i][r];
                        w[r] = exp(vp_log_weight<K, CLS>(c, M, I, a.lo, a.hi, yyr[r], tol[r], lwg, a.gain, a.noise_marginal) - lv[r]);
                    }
                }
                for (unsigned rest = present; rest; rest &= rest - 1) {  // wave-uniform: the rows of one class at a time
                    const int c = __builtin_ctz(rest);
                    double sum = 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) sum += cls[r] == c ? w[r] : 0.0;
                    sum += __shfl_xor(sum, 16);
                    sum += __shfl_xor(sum, 32);
                    if (kq == 0) mine[c * W + j16] += sum;
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < C * wc; i += kVpClassWaves * 64) {
            const int c = i / wc, j = i - c * wc;
            const double *l = lacc + c * W + j;
            a.partial[((size_t)blockIdx.x * C + c) * a.gp + g0 + j] = ((l[0] + l[C * W]) + l[2 * C * W]) + l[3 * C * W];
        }
    }
}

__global__ void __launch_bounds__(256) varpro_class_finish_kernel(const VpClassArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_classes * a.gp) return;
    const int c = i / a.gp, g = i - c * a.gp;
    const long long n = a.stats->n_finite[c];
    if (n == 0) return;  // a class without a voxel that takes part keeps its row
    double s = 0.0;
    for (int b = 0; b < a.blocks; ++b) s += a.partial[((size_t)b * a.n_classes + c) * a.gp + g];
    const double inf = __builtin_huge_val();
    const double pi = (s + a.alpha) / ((double)n + a.alpha * (double)a.n_adm[c]);
    const double lp = (a.lp[i] > -inf && pi > 0.0) ? log(pi) : -inf;  // an inadmissible atom stays at -inf (padded atoms too)
    a.lp[i] = lp;
    a.lw[i] = lp > -inf ? lp + a.occ[g] : -inf;  // the determinant is not recomputed: occ is the call's
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static VpClassArgs vp_class_args(const VarproDict &D, const VarproPosterior &P, const VarproClassTable &T, int64_t n_vox, const double *y_d,
                                 const int32_t *labels_d, const GridSlab &S) {
    const VarproLayout &L = D.L;
    VpClassArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.labels = labels_d;
    a.st = D.st;
    a.cst = D.cst;
    a.wd = D.w;
    a.nl = D.nl;
    a.theta = P.theta;
    a.occ = P.lw;  // prepared without a prior
    a.max_nrm = P.max_nrm;
    a.lp = T.lp;
    a.lw = T.lw;
    a.n_adm = T.n_adm;
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
    a.n_classes = T.n_classes;
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
    for (int c = 0; c < T.n_classes; ++c) a.lp_norm[c] = T.norm[c];
    return a;
}

template <int K, int CLS> static int launch_vp_class_post(const VpClassArgs &a, size_t lds, int blocks, hipStream_t st) {
    if (a.kpad <= 32)
        hipLaunchKernelGGL((varpro_class_posterior_kernel<8, K, CLS>), dim3((unsigned)blocks), dim3(kVpClassWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((varpro_class_posterior_kernel<32, K, CLS>), dim3((unsigned)blocks), dim3(kVpClassWaves * 64), lds, st, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

int varpro_class_posterior_device(const VarproDict &D, const VarproPosterior &P, const VarproClassTable &T, int64_t n_vox, const double *y_d,
                                  const int32_t *labels_d, double *mean_d, double *sd_d, int32_t *map_atom_d, double *map_p_d,
                                  double *log_evidence_d, double *ess_d, double *clipped_mass_d, int cus, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const VarproLayout &L = D.L;
    const GridSlab S = varpro_class_posterior_slab(D.n_b, L.k, T.n_classes);
    VpClassArgs a = vp_class_args(D, P, T, n_vox, y_d, labels_d, S);
    a.mean = mean_d;
    a.sd = sd_d;
    a.map_p = map_p_d;
    a.map_atom = map_atom_d;
    a.logev = log_evidence_d;
    a.ess = ess_d;
    a.cmass = clipped_mass_d;
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    const int blocks = vp_class_blocks(n_vox, cus);              // the unlabelled posterior's grid
    switch (L.k * 4 + L.cls) {
    case 1 * 4 + kVarproFree: return launch_vp_class_post<1, kVarproFree>(a, lds, blocks, stream);
    case 2 * 4 + kVarproFree: return launch_vp_class_post<2, kVarproFree>(a, lds, blocks, stream);
    case 2 * 4 + kVarproReduced: return launch_vp_class_post<2, kVarproReduced>(a, lds, blocks, stream);
    case 2 * 4 + kVarproS0: return launch_vp_class_post<2, kVarproS0>(a, lds, blocks, stream);
    case 3 * 4 + kVarproFree: return launch_vp_class_post<3, kVarproFree>(a, lds, blocks, stream);
    case 3 * 4 + kVarproReduced: return launch_vp_class_post<3, kVarproReduced>(a, lds, blocks, stream);
    case 3 * 4 + kVarproS0: return launch_vp_class_post<3, kVarproS0>(a, lds, blocks, stream);
    }
    return set_error(PNX_ERR_INVALID, "varpro posterior: no kernel for %d compartments, class %d", L.k, L.cls);
}

size_t varpro_class_prior_bytes(int64_t n_vox, int n_atoms, int n_classes, int cus) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15, blocks = (size_t)vp_class_blocks(n_vox, cus), C = (size_t)n_classes;
    return up256((size_t)n_vox * 8) + up256(blocks * C * gp * 8) + 2 * up256(blocks * C * 8) + up256(sizeof(VarproClassStats));
}

void varpro_class_prior_carve(int64_t n_vox, int n_atoms, int n_classes, int cus, void *buffer_d, VarproClassWork *W) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15, blocks = (size_t)vp_class_blocks(n_vox, cus), C = (size_t)n_classes;
    char *p = (char *)buffer_d;
    auto take = [&](size_t bytes) {
        void *q = p;
        p += up256(bytes);
        return q;
    };
    W->lv = (double *)take((size_t)n_vox * 8);
    W->partial = (double *)take(blocks * C * gp * 8);
    W->block_l = (double *)take(blocks * C * 8);
    W->block_n = (long long *)take(blocks * C * 8);
    W->stats = (VarproClassStats *)take(sizeof(VarproClassStats));
    W->blocks = (int)blocks;
}

static VpClassArgs vp_class_em_args(const VarproDict &D, const VarproPosterior &P, const VarproClassTable &T, int64_t n_vox, const double *y_d,
                                    const int32_t *labels_d, const VarproClassWork &W, const GridSlab &S) {
    VpClassArgs a = vp_class_args(D, P, T, n_vox, y_d, labels_d, S);
    a.lv = W.lv;
    a.partial = W.partial;
    a.block_l = W.block_l;
    a.block_n = W.block_n;
    a.stats = W.stats;
    a.blocks = W.blocks;
    return a;
}

template <int K, int CLS> static void launch_vp_class_norm(const VpClassArgs &a, size_t lds, hipStream_t st) {
    if (a.kpad <= 32)
        hipLaunchKernelGGL((varpro_class_norm_kernel<8, K, CLS>), dim3((unsigned)a.blocks), dim3(kVpClassWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((varpro_class_norm_kernel<32, K, CLS>), dim3((unsigned)a.blocks), dim3(kVpClassWaves * 64), lds, st, a);
}

template <int K, int CLS> static void launch_vp_class_acc(const VpClassArgs &a, size_t lds, hipStream_t st) {
    if (a.kpad <= 32)
        hipLaunchKernelGGL((varpro_class_acc_kernel<8, K, CLS>), dim3((unsigned)a.blocks), dim3(kVpClassWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((varpro_class_acc_kernel<32, K, CLS>), dim3((unsigned)a.blocks), dim3(kVpClassWaves * 64), lds, st, a);
}

int varpro_class_prior_normalise(const VarproDict &D, const VarproPosterior &P, const VarproClassTable &T, int64_t n_vox, const double *y_d,
                                 const int32_t *labels_d, const VarproClassWork &W, hipStream_t stream) {
    const VarproLayout &L = D.L;
    const GridSlab S = varpro_class_prior_slab(D.n_b, L.k, T.n_classes);
    const VpClassArgs a = vp_class_em_args(D, P, T, n_vox, y_d, labels_d, W, S);
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    switch (L.k * 4 + L.cls) {
    case 1 * 4 + kVarproFree: launch_vp_class_norm<1, kVarproFree>(a, lds, stream); break;
    case 2 * 4 + kVarproFree: launch_vp_class_norm<2, kVarproFree>(a, lds, stream); break;
    case 2 * 4 + kVarproReduced: launch_vp_class_norm<2, kVarproReduced>(a, lds, stream); break;
    case 2 * 4 + kVarproS0: launch_vp_class_norm<2, kVarproS0>(a, lds, stream); break;
    case 3 * 4 + kVarproFree: launch_vp_class_norm<3, kVarproFree>(a, lds, stream); break;
    case 3 * 4 + kVarproReduced: launch_vp_class_norm<3, kVarproReduced>(a, lds, stream); break;
    case 3 * 4 + kVarproS0: launch_vp_class_norm<3, kVarproS0>(a, lds, stream); break;
    default: return set_error(PNX_ERR_INVALID, "varpro prior: no kernel for %d compartments, class %d", L.k, L.cls);
    }
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(varpro_class_sums_kernel, dim3((unsigned)a.blocks), dim3(256), 0, stream, a);
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(varpro_class_stats_kernel, dim3(1), dim3(64), 0, stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

int varpro_class_prior_update(const VarproDict &D, const VarproPosterior &P, const VarproClassTable &T, int64_t n_vox, const double *y_d,
                              const int32_t *labels_d, const VarproClassWork &W, double pseudo_count, hipStream_t stream) {
    const VarproLayout &L = D.L;
    const GridSlab S = varpro_class_prior_slab(D.n_b, L.k, T.n_classes);
    VpClassArgs a = vp_class_em_args(D, P, T, n_vox, y_d, labels_d, W, S);
    a.alpha = pseudo_count;
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);
    switch (L.k * 4 + L.cls) {
    case 1 * 4 + kVarproFree: launch_vp_class_acc<1, kVarproFree>(a, lds, stream); break;
    case 2 * 4 + kVarproFree: launch_vp_class_acc<2, kVarproFree>(a, lds, stream); break;
    case 2 * 4 + kVarproReduced: launch_vp_class_acc<2, kVarproReduced>(a, lds, stream); break;
    case 2 * 4 + kVarproS0: launch_vp_class_acc<2, kVarproS0>(a, lds, stream); break;
    case 3 * 4 + kVarproFree: launch_vp_class_acc<3, kVarproFree>(a, lds, stream); break;
    case 3 * 4 + kVarproReduced: launch_vp_class_acc<3, kVarproReduced>(a, lds, stream); break;
    case 3 * 4 + kVarproS0: launch_vp_class_acc<3, kVarproS0>(a, lds, stream); break;
    default: return set_error(PNX_ERR_INVALID, "varpro prior: no kernel for %d compartments, class %d", L.k, L.cls);
    }
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(varpro_class_finish_kernel, dim3((unsigned)((T.n_classes * D.gp + 255) / 256)), dim3(256), 0, stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

}  // namespace pnx
