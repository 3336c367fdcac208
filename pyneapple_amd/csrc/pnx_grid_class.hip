// pnx_grid_class.hip -- one prior row per segmentation label (pnx_curvefit_grid_posterior_classes_f64 and
// pnx_curvefit_grid_prior_em_classes_f64).  The log prior of a voxel-atom pair is log_prior[labels[v], g]: no
// longer a property of the atom column alone.  The kernels are the posterior's and the EM's (pnx_grid_posterior.hip,
// pnx_grid_prior.hip: same v_mfma_f64_16x16x4 product, lane maps, dictionary slabs, cost, projection, floor and l_g, expression for
// expression, so a voxel's sums are the bytes the unlabelled kernels give under its row); in LDS the slab carries n_classes prior
// rows, and a lane looks its four voxel rows up under their own classes.
//
//   grid_class_table_kernel      the (n_classes, n_atoms) table padded to (n_classes, gp) with -inf
//   grid_class_posterior_kernel  grid_posterior_kernel with the row of each voxel; a label outside [0, n_classes) makes the voxel
//                                a non-finite one
//   grid_class_norm_kernel       voxel-stationary: L_v under the voxel's row to memory, NaN for a voxel that takes no part
//   grid_class_sums_kernel       per block and class the sum of the finite L_v of the block's voxels, each lane slot of the
//   grid_class_stats_kernel      normaliser's grid in its own order, then the blocks in block order, then the classes in class order
//   grid_class_acc_kernel        slab-stationary: per tile a lane forms its four weights; a wave-uniform loop over the classes
//                                present in the strip selects the rows of one class, the four sums of a column meet over kq and go
//                                into the wave's private LDS row OF THAT CLASS by a plain read-modify-write.  A strip of one class
//                                (a sorted label map) pays for one round; at the end of a slab the block adds its four rows per
//                                class in wave order
//   grid_class_finish_kernel     per class and atom the blocks' sums in block order, then log pi_cg in place
//
// No floating-point atomics: every sum has one order for a given grid size, so a call is reproducible bit for bit; W never reaches
// memory.  A pair at -inf is skipped before any exponential, so (-inf) - (-inf) is never formed.
// Lane maps of the MFMA as in pnx_grid.hip: A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom), row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "pnx_grid_class.hpp"
#include "pnx_launch.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kClassWaves = 4;  // a block: one wave per SIMD, each with a strip of 16 voxels per group

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

static int class_blocks(int64_t n_vox, int cus) {
    const long long n_strips = (n_vox + 15) / 16;
    long long blocks = (n_strips + kClassWaves - 1) / kClassWaves;
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;
    if (blocks > cap) blocks = cap;
    return (int)(blocks > 1 ? blocks : 1);
}

// ---- the table ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) grid_class_table_kernel(const double *lp_in, double *lp, int n_classes, int n_atoms, int gp) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_classes * gp; i += gridDim.x * 256) {
        const int c = i / gp, g = i - c * gp;
        lp[i] = g < n_atoms ? (lp_in ? lp_in[(size_t)c * n_atoms + g] : 0.0) : -__builtin_huge_val();
    }
}

size_t grid_class_table_bytes(int n_classes, int n_atoms) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15;
    return up256((size_t)n_classes * gp * 8) + up256((size_t)n_classes * n_atoms * 8);
}

int grid_class_table_prepare(const GridDict &D, const GridClassHost &K, int n_classes, const double *log_prior_host, void *buffer_d,
                             GridClassTable *T, hipStream_t st) {
    char *p = (char *)buffer_d;
    T->lp = (double *)p;
    T->lp_in = (double *)(p + up256((size_t)n_classes * D.gp * 8));
    T->n_classes = n_classes;
    for (int c = 0; c < n_classes; ++c) T->norm[c] = K.norm[c];
    if (log_prior_host)
        PNX_HIP(hipMemcpyAsync(T->lp_in, log_prior_host, (size_t)n_classes * D.n_atoms * 8, hipMemcpyHostToDevice, st));  // staged as the atoms
    const int blocks = (n_classes * D.gp + 255) / 256;
    hipLaunchKernelGGL(grid_class_table_kernel, dim3(blocks), dim3(256), 0, st, log_prior_host ? T->lp_in : nullptr, T->lp, n_classes,
                       D.n_atoms, D.gp);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

// ---- shared pieces ------------------------------------------------------------------------------------------------------------
struct ClassArgs {
    const double *y;               // (n_vox, n_b)
    const int32_t *labels;         // (n_vox)
    const double *st;              // (kpad, gp)
    const double *nrm, *inv;       // (gp)
    const double *theta;           // (n_free, gp), the posterior only
    const double *wd;              // (kpad)
    const double *atoms;           // (n_free, n_atoms), the posterior only
    const double *max_nrm;
    double *lp;                    // (n_classes, gp) read by every pass, rewritten by the finish kernel
    double *mean, *sd, *map_p;     // (n_free, n_vox); sd and map_p may be null
    int32_t *map_atom;             // (n_vox) or null
    double *logev, *ess;           // (n_vox) or null
    double *lv;                    // (n_vox)
    double *partial;               // (blocks, n_classes, gp)
    double *block_l;               // (blocks, n_classes)
    long long *block_n;            // (blocks, n_classes)
    GridClassStats *stats;
    long long n_vox;
    int n_b, kpad, n_atoms, gp, n_free, width, stride, s0_row, marginal, blocks, n_classes;
    int n_adm[kGridMaxClasses];
    double lo_s0, hi_s0;
    double tol_scale;  // 4 n_b 2^-52
    double gain;       // known noise: 1 / noise_sd^2;  marginalised: nu / 2
    double alpha;      // pseudo_count
    double lp_norm[kGridMaxClasses];
    double centre[PNX_MAX_PARAMS];
};

// The A fragment of a strip of 16 voxels from v0 on, as the posterior kernel loads it: weighted, rows past the end repeat the last
// voxel (never stored, never summed).  yy: ||y||^2 of voxel v0 + r16; bad: that voxel holds a non-finite value or a label outside
// [0, n_classes); cls: its class, 0 when bad.
template <int NS> __device__ __forceinline__ void class_load_strip(const ClassArgs &a, long long v0, int r16, int kq, int ksteps,
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
        nf |= !(fabs(val) < inf);
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

// l_g of one voxel-atom pair from the product y . s_g, the posterior kernel's expressions term for term.
template <bool PROJ> __device__ __forceinline__ double class_log_weight(const ClassArgs &a, double dot, double nr, double iv, double yy,
                                                                       double tol, double lpg) {
    double c;  // cost - 0.5 ||y||^2, grid start's
    if constexpr (PROJ) {
        const double amp = fmin(fmax(dot * iv, a.lo_s0), a.hi_s0);
        c = amp * fma(0.5 * amp, nr, -dot);
    } else {
        c = fma(0.5, nr, -dot);
    }
    const double cost = fma(0.5, yy, c);
    return a.marginal ? fma(-a.gain, log(fmax(cost, tol)), lpg) : fma(-cost, a.gain, lpg);
}

// One slab of the dictionary into LDS: [kpad][stride] | nrm | inv | log_prior[n_classes], each `W` wide; the caller holds the barriers.
__device__ __forceinline__ void class_load_slab(const ClassArgs &a, double *lds, int g0, int wc, int lane, int wave) {
    const int W = a.width;
    double *lnrm = lds + a.kpad * a.stride, *linv = lnrm + W, *llp = linv + W;
    for (int k = wave; k < a.kpad; k += kClassWaves)
        for (int j = lane; j < wc; j += 64) lds[k * a.stride + j] = a.st[(size_t)k * a.gp + g0 + j];
    for (int c = wave; c < a.n_classes; c += kClassWaves)
        for (int j = lane; j < wc; j += 64) llp[c * W + j] = a.lp[(size_t)c * a.gp + g0 + j];
    for (int j = threadIdx.x; j < wc; j += kClassWaves * 64) {
        lnrm[j] = a.nrm[g0 + j];
        linv[j] = a.inv[g0 + j];
    }
}

// ---- posterior ----------------------------------------------------------------------------------------------------------------
// LDS: the slab as above, then theta[n_free], each `W` wide.  NS, NF as in grid_posterior_kernel.
template <int NS, int NF, bool PROJ>
__global__ void __launch_bounds__(kClassWaves * 64) grid_class_posterior_kernel(const ClassArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lnrm = lds + kpad * stride, *linv = lnrm + W, *llp = linv + W, *lth = llp + a.n_classes * W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kClassWaves - 1) / kClassWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double max_nrm = *a.max_nrm;
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        const long long v0 = (grp * kClassWaves + wave) * 16;
        double yf[NS], yy;
        int nf, lab;
        class_load_strip<NS>(a, v0, r16, kq, ksteps, yf, yy, nf, lab);
        // the accumulator rows of this lane are the voxels kq + 4 r of the strip: their ||y||^2, the floor of their cost, their class
        double yyr[4], tol[4];
        int cls[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            yyr[r] = __shfl(yy, kq + 4 * r);
            tol[r] = a.tol_scale * (yyr[r] + max_nrm);
            cls[r] = __shfl(lab, kq + 4 * r) * W;  // the offset of the class's row in llp
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
                class_load_slab(a, lds, g0, wc, lane, wave);
                for (int k = wave; k < a.n_free; k += kClassWaves)
                    for (int j = lane; j < wc; j += 64) lth[k * W + j] = a.theta[(size_t)k * a.gp + g0 + j];
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
                // fold: this lane's atom against its four voxels, each under its own row.  A padded atom holds -inf in every row,
                // an excluded pair in its own: either contributes exactly nothing.  Atoms arrive in ascending order, so a strict
                // comparison keeps the lowest index among equal l.
                const int j = t * 16 + r16, g = g0 + j;
                const double nr = lnrm[j];
                const double iv = PROJ ? linv[j] : 0.0;
                double th[NF];
#pragma unroll
                for (int k = 0; k < NF; ++k) th[k] = k < a.n_free ? lth[k * W + j] : 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double lpg = llp[cls[r] + j];
                    if (lpg > -inf) {
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
                        const double d = ell - m[r];  // +inf for the first admissible atom of the row, however late it comes
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
            const int src = kq + 4 * r;  // this voxel's row of the strip: its flag and class live in lane `src`
            const int badv = __shfl(nf, src);
            const int cv = __shfl(lab, src);
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
                    if (a.logev) a.logev[v] = badv ? qnan : m[r] + log(sw[r]) - a.lp_norm[cv];
                } else if (r16 == 10) {
                    if (a.ess) a.ess[v] = badv ? qnan : sw[r] * sw[r] / sw2[r];
                }
            }
        }
    }
}

// ---- normaliser pass ----------------------------------------------------------------------------------------------------------
template <int NS, bool PROJ> __global__ void __launch_bounds__(kClassWaves * 64) grid_class_norm_kernel(const ClassArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    const double *lnrm = lds + kpad * stride, *linv = lnrm + W, *llp = linv + W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kClassWaves - 1) / kClassWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double max_nrm = *a.max_nrm;
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        const long long v0 = (grp * kClassWaves + wave) * 16;
        double yf[NS], yy;
        int nf, lab;
        class_load_strip<NS>(a, v0, r16, kq, ksteps, yf, yy, nf, lab);
        double yyr[4], tol[4], m[4], sw[4];
        int cls[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            yyr[r] = __shfl(yy, kq + 4 * r);
            tol[r] = a.tol_scale * (yyr[r] + max_nrm);
            cls[r] = __shfl(lab, kq + 4 * r) * W;
            m[r] = -inf;
            sw[r] = 0.0;
        }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                class_load_slab(a, lds, g0, wc, lane, wave);
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
                const int j = t * 16 + r16;
                const double nr = lnrm[j];
                const double iv = PROJ ? linv[j] : 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double lpg = llp[cls[r] + j];
                    if (lpg > -inf) {  // a padded atom or an excluded pair contributes exactly nothing
                        const double ell = class_log_weight<PROJ>(a, acc[r], nr, iv, yyr[r], tol[r], lpg);
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
            if (r16 == 0 && v < a.n_vox) a.lv[v] = badv ? __builtin_nan("") : m[r] + log(sw[r]);
        }
    }
}

// The log-likelihood per class, in the order the unlabelled normaliser sums it: thread (c, slot) walks the voxels that lane
// slot = 4 wave + kq of block blockIdx.x wrote above -- groups ascending, the four rows ascending -- and keeps those of class c;
// then per class the 16 slots in slot order.
__global__ void __launch_bounds__(256) grid_class_sums_kernel(const ClassArgs a) {
    __shared__ double ls[256];
    __shared__ long long ln[256];
    const int slot = threadIdx.x & 15, c = threadIdx.x >> 4;
    const int wave = slot >> 2, kq = slot & 3;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kClassWaves - 1) / kClassWaves;
    const double inf = __builtin_huge_val();
    double s = 0.0;
    long long n = 0;
    if (c < a.n_classes) {
        for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
            const long long v0 = (grp * kClassWaves + wave) * 16;
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

__global__ void __launch_bounds__(64) grid_class_stats_kernel(const ClassArgs a) {
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
// LDS: the slab as above, then acc[kClassWaves][n_classes][W].  A wave adds into its own rows only, in program order; the rows meet
// at the end of the slab behind a barrier.
template <int NS, bool PROJ> __global__ void __launch_bounds__(kClassWaves * 64) grid_class_acc_kernel(const ClassArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width, C = a.n_classes;
    const double *lnrm = lds + kpad * stride, *linv = lnrm + W, *llp = linv + W;
    double *lacc = lds + kpad * stride + (2 + C) * W, *mine = lacc + wave * C * W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kClassWaves - 1) / kClassWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double max_nrm = *a.max_nrm;
    for (int slab = 0; slab < n_slabs; ++slab) {
        const int g0 = slab * W;
        const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
        __syncthreads();  // the previous slab's rows have been written out
        class_load_slab(a, lds, g0, wc, lane, wave);
        for (int c = 0; c < C; ++c)
            for (int j = lane; j < wc; j += 64) mine[c * W + j] = 0.0;
        __syncthreads();
        for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
            const long long v0 = (grp * kClassWaves + wave) * 16;
            double yf[NS], yy;
            int nf, lab;
            class_load_strip<NS>(a, v0, r16, kq, ksteps, yf, yy, nf, lab);
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
                tol[r] = a.tol_scale * (yyr[r] + max_nrm);
                cls[r] = __shfl(lab, kq + 4 * r);
                const long long v = v0 + kq + 4 * r;
                lv[r] = v < a.n_vox ? a.lv[v] : __builtin_nan("");
                ok[r] = fabs(lv[r]) < inf;  // a voxel past the end or without a finite L_v weighs nothing
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
                const double *bp = lds + kq * stride + t * 16 + r16;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (s < ksteps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(yf[s], bp[4 * s * stride], acc, 0, 0, 0);
                }
                const int j = t * 16 + r16;
                const double nr = lnrm[j];
                const double iv = PROJ ? linv[j] : 0.0;
                double w[4];  // this atom's weight on the lane's four voxels; exactly 0 for a padded atom or an excluded pair
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double lpg = llp[cls[r] * W + j];
                    w[r] = 0.0;
                    if (ok[r] && lpg > -inf) w[r] = exp(class_log_weight<PROJ>(a, acc[r], nr, iv, yyr[r], tol[r], lpg) - lv[r]);
                }
                for (unsigned rest = present; rest; rest &= rest - 1) {  // wave-uniform: the rows of one class at a time
                    const int c = __builtin_ctz(rest);
                    double sum = 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) sum += cls[r] == c ? w[r] : 0.0;
                    sum += __shfl_xor(sum, 16);
                    sum += __shfl_xor(sum, 32);
                    if (kq == 0) mine[c * W + j] += sum;
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < C * wc; i += kClassWaves * 64) {
            const int c = i / wc, j = i - c * wc;
            const double *l = lacc + c * W + j;
            a.partial[((size_t)blockIdx.x * C + c) * a.gp + g0 + j] = ((l[0] + l[C * W]) + l[2 * C * W]) + l[3 * C * W];
        }
    }
}

__global__ void __launch_bounds__(256) grid_class_finish_kernel(const ClassArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_classes * a.gp) return;
    const int c = i / a.gp, g = i - c * a.gp;
    const long long n = a.stats->n_finite[c];
    if (n == 0) return;  // a class without a voxel that takes part keeps its row
    double s = 0.0;
    for (int b = 0; b < a.blocks; ++b) s += a.partial[((size_t)b * a.n_classes + c) * a.gp + g];
    const double inf = __builtin_huge_val();
    const double pi = (s + a.alpha) / ((double)n + a.alpha * a.n_adm[c]);
    a.lp[i] = (a.lp[i] > -inf && pi > 0.0) ? log(pi) : -inf;  // an atom that started at -inf stays there (padded atoms too)
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static ClassArgs class_args(const GridDict &D, const GridPosterior &P, const GridClassTable &T, int64_t n_vox, const double *y_d,
                            const int32_t *labels_d, const GridSlab &S) {
    ClassArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.labels = labels_d;
    a.st = D.st;
    a.nrm = D.nrm;
    a.inv = D.inv;
    a.theta = P.theta;
    a.wd = D.w;
    a.atoms = D.atoms;
    a.max_nrm = P.max_nrm;
    a.lp = T.lp;
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
    a.n_classes = T.n_classes;
    a.lo_s0 = D.lo_s0;
    a.hi_s0 = D.hi_s0;
    a.tol_scale = 4.0 * D.n_b * 0x1p-52;
    a.gain = a.marginal ? 0.5 * (D.n_b - (D.s0_row >= 0 ? 1 : 0)) : 1.0 / (P.noise_sd * P.noise_sd);
    for (int c = 0; c < T.n_classes; ++c) a.lp_norm[c] = T.norm[c];
    for (int k = 0; k < PNX_MAX_PARAMS; ++k) a.centre[k] = P.centre[k];
    return a;
}

template <int NS, int NF> static int launch_class_post(const ClassArgs &a, size_t lds, int blocks, hipStream_t st) {
    if (a.s0_row >= 0)
        hipLaunchKernelGGL((grid_class_posterior_kernel<NS, NF, true>), dim3((unsigned)blocks), dim3(kClassWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((grid_class_posterior_kernel<NS, NF, false>), dim3((unsigned)blocks), dim3(kClassWaves * 64), lds, st, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

template <int NS> static int launch_class_post_nf(const ClassArgs &a, size_t lds, int blocks, hipStream_t st) {
    if (a.n_free <= 3) return launch_class_post<NS, 3>(a, lds, blocks, st);
    if (a.n_free <= 6) return launch_class_post<NS, 6>(a, lds, blocks, st);
    return launch_class_post<NS, 8>(a, lds, blocks, st);
}

int grid_class_posterior_device(const GridDict &D, const GridPosterior &P, const GridClassTable &T, int64_t n_vox, const double *y_d,
                                const int32_t *labels_d, double *mean_d, double *sd_d, int32_t *map_atom_d, double *map_p_d,
                                double *log_evidence_d, double *ess_d, int cus, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const GridSlab S = grid_class_posterior_slab(D.n_b, D.n_free, T.n_classes);
    ClassArgs a = class_args(D, P, T, n_vox, y_d, labels_d, S);
    a.mean = mean_d;
    a.sd = sd_d;
    a.map_p = map_p_d;
    a.map_atom = map_atom_d;
    a.logev = log_evidence_d;
    a.ess = ess_d;
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    const int blocks = class_blocks(n_vox, cus);
    if (S.kpad <= 32) return launch_class_post_nf<8>(a, lds, blocks, stream);
    return launch_class_post_nf<32>(a, lds, blocks, stream);
}

size_t grid_class_prior_bytes(int64_t n_vox, int n_atoms, int n_classes, int cus) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15, blocks = (size_t)class_blocks(n_vox, cus), C = (size_t)n_classes;
    return up256((size_t)n_vox * 8) + up256(blocks * C * gp * 8) + 2 * up256(blocks * C * 8) + up256(sizeof(GridClassStats));
}

void grid_class_prior_carve(int64_t n_vox, int n_atoms, int n_classes, int cus, void *buffer_d, GridClassWork *W) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15, blocks = (size_t)class_blocks(n_vox, cus), C = (size_t)n_classes;
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
    W->stats = (GridClassStats *)take(sizeof(GridClassStats));
    W->blocks = (int)blocks;
}

static ClassArgs class_em_args(const GridDict &D, const GridPosterior &P, const GridClassTable &T, int64_t n_vox, const double *y_d,
                               const int32_t *labels_d, const GridClassWork &W, const GridSlab &S) {
    ClassArgs a = class_args(D, P, T, n_vox, y_d, labels_d, S);
    a.lv = W.lv;
    a.partial = W.partial;
    a.block_l = W.block_l;
    a.block_n = W.block_n;
    a.stats = W.stats;
    a.blocks = W.blocks;
    return a;
}

template <int NS> static void launch_class_norm(const ClassArgs &a, bool proj, size_t lds, hipStream_t st) {
    if (proj)
        hipLaunchKernelGGL((grid_class_norm_kernel<NS, true>), dim3((unsigned)a.blocks), dim3(kClassWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((grid_class_norm_kernel<NS, false>), dim3((unsigned)a.blocks), dim3(kClassWaves * 64), lds, st, a);
}

template <int NS> static void launch_class_acc(const ClassArgs &a, bool proj, size_t lds, hipStream_t st) {
    if (proj)
        hipLaunchKernelGGL((grid_class_acc_kernel<NS, true>), dim3((unsigned)a.blocks), dim3(kClassWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((grid_class_acc_kernel<NS, false>), dim3((unsigned)a.blocks), dim3(kClassWaves * 64), lds, st, a);
}

int grid_class_prior_normalise(const GridDict &D, const GridPosterior &P, const GridClassTable &T, int64_t n_vox, const double *y_d,
                               const int32_t *labels_d, const GridClassWork &W, hipStream_t stream) {
    const GridSlab S = grid_class_prior_slab(D.n_b, T.n_classes);
    const ClassArgs a = class_em_args(D, P, T, n_vox, y_d, labels_d, W, S);
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    if (S.kpad <= 32)
        launch_class_norm<8>(a, D.s0_row >= 0, lds, stream);
    else
        launch_class_norm<32>(a, D.s0_row >= 0, lds, stream);
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(grid_class_sums_kernel, dim3((unsigned)a.blocks), dim3(256), 0, stream, a);
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(grid_class_stats_kernel, dim3(1), dim3(64), 0, stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

int grid_class_prior_update(const GridDict &D, const GridPosterior &P, const GridClassTable &T, int64_t n_vox, const double *y_d,
                            const int32_t *labels_d, const GridClassWork &W, double pseudo_count, const int *n_adm, hipStream_t stream) {
    const GridSlab S = grid_class_prior_slab(D.n_b, T.n_classes);
    ClassArgs a = class_em_args(D, P, T, n_vox, y_d, labels_d, W, S);
    a.alpha = pseudo_count;
    for (int c = 0; c < T.n_classes; ++c) a.n_adm[c] = n_adm[c];
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);
    if (S.kpad <= 32)
        launch_class_acc<8>(a, D.s0_row >= 0, lds, stream);
    else
        launch_class_acc<32>(a, D.s0_row >= 0, lds, stream);
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(grid_class_finish_kernel, dim3((unsigned)((T.n_classes * D.gp + 255) / 256)), dim3(256), 0, stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

}  // namespace pnx
