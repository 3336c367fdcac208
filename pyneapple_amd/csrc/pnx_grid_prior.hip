// pnx_grid_prior.hip -- the prior over a dictionary learned from the volume itself (pnx_curvefit_grid_prior_em_f64, DESIGN.md
// 4.1j): the non-parametric maximum-likelihood mixture on a fixed grid, pi_g <- (1 / N) sum_v W_vg, by EM.  W_vg is the normalised
// weight the posterior kernel (pnx_grid_posterior.hip) forms per voxel-atom pair; an iteration needs its sum over the voxels per
// atom, the transposed reduction, of a matrix that never reaches memory.  Two passes over the product y_v . s_g, both on
// v_mfma_f64_16x16x4 with the posterior's lane maps, dictionary slabs, cost c_g(v), amplitude projection, floor tol_v and l_g:
//
//   grid_prior_norm_kernel    voxel-stationary, the posterior kernel without its moments: per voxel the running (m, sum w) only,
//                             L_v = m + log(sum w) to memory, NaN for a non-finite voxel; per block the sum of its finite L_v
//   grid_prior_stats_kernel   the blocks' sums in block order: the log-likelihood of the volume and its number of finite voxels
//   grid_prior_acc_kernel     slab-stationary: the slab loop is the outer loop, so a block loads a dictionary slab once and
//                             streams its voxel groups past it.  Per tile a lane forms w = exp(l_g - L_v) for its four voxel rows,
//                             the four sums of a column meet over kq (lanes + 16, + 32) and go into a wave-private LDS row by a
//                             plain read-modify-write; at the end of a slab the block adds its four rows in wave order
//   grid_prior_finish_kernel  per atom the blocks' sums in block order, then log pi_g in place
//
// No floating-point atomics: every sum has one order for a given grid size, so a call is reproducible bit for bit.
// Lane maps of the MFMA as in pnx_grid.hip: A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom), row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "pnx_grid_prior.hpp"
#include "pnx_launch.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kPriorWaves = 4;  // a block: one wave per SIMD, each with a strip of 16 voxels per group

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

static int prior_blocks(int64_t n_vox, int cus) {
    const long long n_strips = (n_vox + 15) / 16;
    long long blocks = (n_strips + kPriorWaves - 1) / kPriorWaves;
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;
    if (blocks > cap) blocks = cap;
    return (int)(blocks > 1 ? blocks : 1);
}

size_t grid_prior_bytes(int64_t n_vox, int n_atoms, int cus) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15, blocks = (size_t)prior_blocks(n_vox, cus);
    return up256((size_t)n_vox * 8) + up256(blocks * gp * 8) + 2 * up256(blocks * 8) + up256(sizeof(GridPriorStats));
}

void grid_prior_carve(int64_t n_vox, int n_atoms, int cus, void *buffer_d, GridPriorWork *W) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15, blocks = (size_t)prior_blocks(n_vox, cus);
    char *p = (char *)buffer_d;
    auto take = [&](size_t bytes) {
        void *q = p;
        p += up256(bytes);
        return q;
    };
    W->lv = (double *)take((size_t)n_vox * 8);
    W->partial = (double *)take(blocks * gp * 8);
    W->block_l = (double *)take(blocks * 8);
    W->block_n = (long long *)take(blocks * 8);
    W->stats = (GridPriorStats *)take(sizeof(GridPriorStats));
    W->blocks = (int)blocks;
}

struct PriorArgs {
    const double *y;               // (n_vox, n_b)
    const double *st;              // (kpad, gp)
    const double *nrm, *inv;       // (gp)
    const double *wd;              // (kpad)
    const double *max_nrm;
    double *lp;                    // (gp) read by both passes, rewritten by the finish kernel
    double *lv;                    // (n_vox)
    double *partial;               // (blocks, gp)
    double *block_l;               // (blocks)
    long long *block_n;            // (blocks)
    GridPriorStats *stats;
    long long n_vox;
    int n_b, kpad, gp, width, stride, marginal, blocks, n_adm;
    double lo_s0, hi_s0;
    double tol_scale;  // 4 n_b 2^-52
    double gain;       // known noise: 1 / noise_sd^2;  marginalised: nu / 2
    double alpha;      // pseudo_count
};

// The A fragment of a strip of 16 voxels from v0 on, as the posterior kernel loads it: weighted, rows past the end repeat the last
// voxel (never stored, never summed).  yy: ||y||^2 of voxel v0 + r16, bad: that voxel holds a non-finite value.
template <int NS> __device__ __forceinline__ void prior_load_strip(const PriorArgs &a, long long v0, int r16, int kq, int ksteps,
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
        nf |= !(fabs(val) < inf);
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

// l_g of one voxel-atom pair from the product y . s_g, the posterior kernel's expressions term for term.
template <bool PROJ> __device__ __forceinline__ double prior_log_weight(const PriorArgs &a, double dot, double nr, double iv, double yy,
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

// One slab of the dictionary into LDS: [kpad][stride] | nrm | inv | log_prior, each `W` wide; the caller holds the barriers.
__device__ __forceinline__ void prior_load_slab(const PriorArgs &a, double *lds, int g0, int wc, int lane, int wave) {
    const int W = a.width;
    double *lnrm = lds + a.kpad * a.stride, *linv = lnrm + W, *llp = linv + W;
    for (int k = wave; k < a.kpad; k += kPriorWaves)
        for (int j = lane; j < wc; j += 64) lds[k * a.stride + j] = a.st[(size_t)k * a.gp + g0 + j];
    for (int j = threadIdx.x; j < wc; j += kPriorWaves * 64) {
        lnrm[j] = a.nrm[g0 + j];
        linv[j] = a.inv[g0 + j];
        llp[j] = a.lp[g0 + j];
    }
}

// ---- normaliser pass ----------------------------------------------------------------------------------------------------------
template <int NS, bool PROJ> __global__ void __launch_bounds__(kPriorWaves * 64) grid_prior_norm_kernel(const PriorArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    const double *lnrm = lds + kpad * stride, *linv = lnrm + W, *llp = linv + W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kPriorWaves - 1) / kPriorWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double max_nrm = *a.max_nrm;
    bool resident = false;
    double sum_l = 0.0;  // lanes with r16 == 0: the finite L_v they wrote, in the order they wrote them
    long long cnt = 0;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        const long long v0 = (grp * kPriorWaves + wave) * 16;
        double yf[NS], yy;
        int nf;
        prior_load_strip<NS>(a, v0, r16, kq, ksteps, yf, yy, nf);
        // the accumulator rows of this lane are the voxels kq + 4 r of the strip: their ||y||^2 and the floor of their cost
        double yyr[4], tol[4], m[4], sw[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            yyr[r] = __shfl(yy, kq + 4 * r);
            tol[r] = a.tol_scale * (yyr[r] + max_nrm);
            m[r] = -inf;
            sw[r] = 0.0;
        }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                prior_load_slab(a, lds, g0, wc, lane, wave);
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
                // a padded or excluded atom holds log_prior = -inf and contributes exactly nothing
                const int j = t * 16 + r16;
                const double lpg = llp[j];
                if (lpg > -inf) {
                    const double nr = lnrm[j];
                    const double iv = PROJ ? linv[j] : 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double ell = prior_log_weight<PROJ>(a, acc[r], nr, iv, yyr[r], tol[r], lpg);
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
                const double L = badv ? __builtin_nan("") : m[r] + log(sw[r]);
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
    long long *lcnt = reinterpret_cast<long long *>(lds + kPriorWaves * 4);
    if (r16 == 0) {
        lds[wave * 4 + kq] = sum_l;
        lcnt[wave * 4 + kq] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        long long n = 0;
        for (int i = 0; i < kPriorWaves * 4; ++i) {
            s += lds[i];
            n += lcnt[i];
        }
        a.block_l[blockIdx.x] = s;
        a.block_n[blockIdx.x] = n;
    }
}

__global__ void __launch_bounds__(64) grid_prior_stats_kernel(const PriorArgs a) {
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
// LDS: the slab as above, then acc[kPriorWaves][W].  A wave adds into its own row only, in program order; the rows meet at the
// end of the slab behind a barrier.
template <int NS, bool PROJ> __global__ void __launch_bounds__(kPriorWaves * 64) grid_prior_acc_kernel(const PriorArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    const double *lnrm = lds + kpad * stride, *linv = lnrm + W, *llp = linv + W;
    double *lacc = lds + kpad * stride + 3 * W, *mine = lacc + wave * W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kPriorWaves - 1) / kPriorWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double max_nrm = *a.max_nrm;
    for (int slab = 0; slab < n_slabs; ++slab) {
        const int g0 = slab * W;
        const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
        __syncthreads();  // the previous slab's rows have been written out
        prior_load_slab(a, lds, g0, wc, lane, wave);
        for (int j = lane; j < wc; j += 64) mine[j] = 0.0;
        __syncthreads();
        for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
            const long long v0 = (grp * kPriorWaves + wave) * 16;
            double yf[NS], yy;
            int nf;
            prior_load_strip<NS>(a, v0, r16, kq, ksteps, yf, yy, nf);
            double yyr[4], tol[4], lv[4];
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                yyr[r] = __shfl(yy, kq + 4 * r);
                tol[r] = a.tol_scale * (yyr[r] + max_nrm);
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
                const double lpg = llp[j];
                double sum = 0.0;  // this atom's weights over the lane's four voxels; exactly 0 for a padded or excluded atom
                if (lpg > -inf) {
                    const double nr = lnrm[j];
                    const double iv = PROJ ? linv[j] : 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double ell = prior_log_weight<PROJ>(a, acc[r], nr, iv, yyr[r], tol[r], lpg);
                        sum += ok[r] ? exp(ell - lv[r]) : 0.0;
                    }
                }
                sum += __shfl_xor(sum, 16);
                sum += __shfl_xor(sum, 32);
                if (kq == 0) mine[j] += sum;
            }
        }
        __syncthreads();
        double *dst = a.partial + (size_t)blockIdx.x * a.gp + g0;
        for (int j = threadIdx.x; j < wc; j += kPriorWaves * 64)
            dst[j] = ((lacc[j] + lacc[W + j]) + lacc[2 * W + j]) + lacc[3 * W + j];
    }
}

__global__ void __launch_bounds__(256) grid_prior_finish_kernel(const PriorArgs a) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= a.gp) return;
    double s = 0.0;
    for (int b = 0; b < a.blocks; ++b) s += a.partial[(size_t)b * a.gp + g];
    const double inf = __builtin_huge_val();
    const double pi = (s + a.alpha) / ((double)a.stats->n_finite + a.alpha * a.n_adm);
    a.lp[g] = (a.lp[g] > -inf && pi > 0.0) ? log(pi) : -inf;  // an atom that started at -inf stays there (padded atoms too)
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static PriorArgs prior_args(const GridDict &D, const GridPosterior &P, int64_t n_vox, const double *y_d, const GridPriorWork &W,
                            const GridSlab &S) {
    PriorArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.nrm = D.nrm;
    a.inv = D.inv;
    a.wd = D.w;
    a.max_nrm = P.max_nrm;
    a.lp = const_cast<double *>(P.lp);  // carved from the call's own buffer
    a.lv = W.lv;
    a.partial = W.partial;
    a.block_l = W.block_l;
    a.block_n = W.block_n;
    a.stats = W.stats;
    a.n_vox = n_vox;
    a.n_b = D.n_b;
    a.kpad = S.kpad;
    a.gp = D.gp;
    a.width = S.width < D.gp ? S.width : D.gp;
    a.stride = S.stride;
    a.marginal = P.noise_sd == 0.0;
    a.blocks = W.blocks;
    a.lo_s0 = D.lo_s0;
    a.hi_s0 = D.hi_s0;
    a.tol_scale = 4.0 * D.n_b * 0x1p-52;
    a.gain = a.marginal ? 0.5 * (D.n_b - (D.s0_row >= 0 ? 1 : 0)) : 1.0 / (P.noise_sd * P.noise_sd);
    return a;
}

template <int NS> static void launch_norm(const PriorArgs &a, bool proj, size_t lds, hipStream_t st) {
    if (proj)
        hipLaunchKernelGGL((grid_prior_norm_kernel<NS, true>), dim3((unsigned)a.blocks), dim3(kPriorWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((grid_prior_norm_kernel<NS, false>), dim3((unsigned)a.blocks), dim3(kPriorWaves * 64), lds, st, a);
}

template <int NS> static void launch_acc(const PriorArgs &a, bool proj, size_t lds, hipStream_t st) {
    if (proj)
        hipLaunchKernelGGL((grid_prior_acc_kernel<NS, true>), dim3((unsigned)a.blocks), dim3(kPriorWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((grid_prior_acc_kernel<NS, false>), dim3((unsigned)a.blocks), dim3(kPriorWaves * 64), lds, st, a);
}

int grid_prior_normalise(const GridDict &D, const GridPosterior &P, int64_t n_vox, const double *y_d, const GridPriorWork &W, hipStream_t stream) {
    const GridSlab S = grid_prior_slab(D.n_b);
    const PriorArgs a = prior_args(D, P, n_vox, y_d, W, S);
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    if (S.kpad <= 32)
        launch_norm<8>(a, D.s0_row >= 0, lds, stream);
    else
        launch_norm<32>(a, D.s0_row >= 0, lds, stream);
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(grid_prior_stats_kernel, dim3(1), dim3(64), 0, stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

int grid_prior_update(const GridDict &D, const GridPosterior &P, int64_t n_vox, const double *y_d, const GridPriorWork &W, double pseudo_count,
                      int n_admissible, hipStream_t stream) {
    const GridSlab S = grid_prior_slab(D.n_b);
    PriorArgs a = prior_args(D, P, n_vox, y_d, W, S);
    a.alpha = pseudo_count;
    a.n_adm = n_admissible;
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);
    if (S.kpad <= 32)
        launch_acc<8>(a, D.s0_row >= 0, lds, stream);
    else
        launch_acc<32>(a, D.s0_row >= 0, lds, stream);
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(grid_prior_finish_kernel, dim3((unsigned)((D.gp + 255) / 256)), dim3(256), 0, stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

}  // namespace pnx
