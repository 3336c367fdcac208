// pnx_varpro.hip -- variable-projection dictionary fit (pnx_curvefit_varpro_f64).  Only the non-linear parameters
// of a layout (the rates, a free T1) are on the grid: an atom g is K unit columns phi_j = model(b; one-hot fractions, S0 = 1) / sigma,
// and the amplitudes of every voxel-atom pair come in closed form from c = Phi^T y (K dot products) and per-atom constants.
//
//   varpro_params_kernel   the K one-hot parameter vectors of every atom, which model_predict_kernel turns into the columns (the
//                          fit's own arithmetic, as grid start's dictionary)
//   varpro_finish_kernel   one lane per atom: columns weighted by 1 / sigma, transposed to k-major per compartment, padded with
//                          zero rows and zero atoms; M = Phi^T Phi, its inverse -- or, for the sum-to-one layouts, the inverse of
//                          the difference system (phi_j - phi_K) and its offsets (phi_j - phi_K) . phi_K, summed directly
//   varpro_match_kernel    grid start's product (pnx_grid.hip: same lane maps, y fragments in registers, LDS slab), K MFMA
//                          chains per atom tile so that a lane holds c_1 .. c_K of one voxel-atom pair; the fold solves, clips,
//                          evaluates cost = 0.5 ||y||^2 - c.a' + 0.5 a'^T M a' and keeps (min, argmin, a').  One cross-lane
//                          reduction at the end.  The (n_vox, G) product never reaches HBM.
//
// Lane maps of the MFMA as in pnx_grid.hip: A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom), row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "pnx_internal.hpp"
#include "pnx_predict.hpp"
#include "pnx_varpro.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

#define VP_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) return set_error(PNX_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// packed index of the symmetric (i, j), j <= i
__host__ __device__ constexpr int pk(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// ---- dictionary -------------------------------------------------------------------------------------------------------------
struct ParamsArgs {
    const double *nl;  // (n_nl, n_atoms)
    double *params;    // (n_free, K n_atoms): column j n_atoms + g is compartment j of atom g
    int n_free, n_atoms, k, cls;
    int row_src[PNX_MAX_PARAMS];
};

__global__ void __launch_bounds__(256) varpro_params_kernel(const ParamsArgs a) {
    const int cols = a.k * a.n_atoms;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_free * cols) return;
    const int r = i / cols, col = i - r * cols, j = col / a.n_atoms, g = col - j * a.n_atoms;
    int src = 0;
#pragma unroll
    for (int q = 0; q < PNX_MAX_PARAMS; ++q)
        if (q == r) src = a.row_src[q];
    double v;
    if (src >= 0) {
        v = a.nl[(size_t)src * a.n_atoms + g];
    } else {
        const int slot = -1 - src;
        v = (a.cls == kVarproS0 && slot == a.k - 1) ? 1.0 : (slot == j ? 1.0 : 0.0);  // S0 = 1; a one-hot fraction (mono: S0 = 1)
    }
    a.params[i] = v;
}

struct FinishArgs {
    const double *raw;  // (K n_atoms, n_b) model(b; column)
    double *st;         // (K, kpad, gp)
    double *cst;        // (crow, gp)
    double *wd;         // (kpad)
    int n_atoms, n_b, kpad, gp, k, cls;
    double w[PNX_MAX_BVALUES];  // 1 / sigma_i
};

// inverse of the symmetric positive definite n x n (n <= 3) matrix packed in m[6], by cofactors of its embedding
// [[M, 0], [0, I]]; a matrix that is not positive definite in this arithmetic gets the zero matrix (every amplitude 0, clipped)
__device__ inline void spd_inverse(int n, const double *m, double *inv) {
    const double a00 = m[0], a10 = n > 1 ? m[1] : 0.0, a11 = n > 1 ? m[2] : 1.0;
    const double a20 = n > 2 ? m[3] : 0.0, a21 = n > 2 ? m[4] : 0.0, a22 = n > 2 ? m[5] : 1.0;
    const double c00 = a11 * a22 - a21 * a21, c10 = a21 * a20 - a10 * a22, c20 = a10 * a21 - a11 * a20;
    const double c11 = a00 * a22 - a20 * a20, c21 = a10 * a20 - a00 * a21, c22 = a00 * a11 - a10 * a10;
    const double det = a00 * c00 + a10 * c10 + a20 * c20;
    const double s = (det > 0.0 && a00 > 0.0 && c22 > 0.0) ? 1.0 / det : 0.0;
    inv[0] = c00 * s;
    inv[1] = c10 * s;
    inv[2] = c11 * s;
    inv[3] = c20 * s;
    inv[4] = c21 * s;
    inv[5] = c22 * s;
}

// one lane per atom (padded atoms included: their rows and constants are zero); reads strided, writes coalesced, once per call
template <int K> __global__ void __launch_bounds__(256) varpro_finish_kernel(const FinishArgs a) {
    constexpr int NM = K * (K + 1) / 2;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < a.kpad) a.wd[g] = g < a.n_b ? a.w[g] : 0.0;
    if (g >= a.gp) return;
    const bool red = a.cls == kVarproReduced;
    double m[6] = {0, 0, 0, 0, 0, 0}, n[6] = {0, 0, 0, 0, 0, 0}, off[3] = {0, 0, 0};
    for (int k = 0; k < a.kpad; ++k) {
        double v[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            v[j] = (g < a.n_atoms && k < a.n_b) ? a.raw[((size_t)j * a.n_atoms + g) * a.n_b + k] * a.w[k] : 0.0;
            a.st[((size_t)j * a.kpad + k) * a.gp + g] = v[j];
        }
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) m[pk(i, j)] = fma(v[i], v[j], m[pk(i, j)]);
        if (K > 1) {  // the difference system of the sum-to-one layouts, summed directly: no cancellation between entries of M
#pragma unroll
            for (int i = 0; i < K - 1; ++i) {
                const double di = v[i] - v[K - 1];
                off[i] = fma(di, v[K - 1], off[i]);
#pragma unroll
                for (int j = 0; j <= i; ++j) n[pk(i, j)] = fma(di, v[j] - v[K - 1], n[pk(i, j)]);
            }
        }
    }
    constexpr int NN = (K - 1) * K / 2;  // entries of the difference system's inverse; its K - 1 offsets lie behind them
    double inv[6];
    spd_inverse(red ? K - 1 : K, red ? n : m, inv);
#pragma unroll
    for (int q = 0; q < NM; ++q) {
        a.cst[(size_t)q * a.gp + g] = m[q];
        double s = inv[q];
        if (red && q >= NN) s = q - NN < K - 1 ? off[q - NN] : 0.0;
        a.cst[(size_t)(NM + q) * a.gp + g] = s;
    }
}

size_t varpro_dict_bytes(int n_free, int n_nl, int k, int n_atoms, int n_b) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15, kpad = ((size_t)n_b + 3) & ~(size_t)3;
    return up256((size_t)n_nl * n_atoms * 8) + up256((size_t)n_free * k * n_atoms * 8) + up256((size_t)k * n_atoms * n_b * 8) +
           up256((size_t)k * kpad * gp * 8) + up256((size_t)varpro_const_rows(k) * gp * 8) + up256(kpad * 8);
}

int varpro_dict_build(const pnx_curvefit_opts *o, const VarproLayout &L, const double *b, int n_atoms, const double *nl_atoms_host,
                      const double *fixed_host, const double *fallback, void *buffer_d, VarproDict *D, hipStream_t st) {
    const int n = o->n_free, n_b = o->n_b, K = L.k;
    const int gp = (n_atoms + 15) & ~15, kpad = (n_b + 3) & ~3, cols = K * n_atoms;
    char *p = (char *)buffer_d;
    auto take = [&](size_t bytes) {
        void *q = p;
        p += up256(bytes);
        return (double *)q;
    };
    double *nl_d = take((size_t)L.n_nl * n_atoms * 8), *params = take((size_t)n * cols * 8), *raw = take((size_t)cols * n_b * 8);
    double *stt = take((size_t)K * kpad * gp * 8), *cst = take((size_t)varpro_const_rows(K) * gp * 8), *wd = take((size_t)kpad * 8);
    // the copy from pageable memory is staged before the call returns (as grid start's atoms)
    if (L.n_nl) VP_HIP(hipMemcpyAsync(nl_d, nl_atoms_host, (size_t)L.n_nl * n_atoms * 8, hipMemcpyHostToDevice, st));
    ParamsArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.nl = nl_d;
    pa.params = params;
    pa.n_free = n;
    pa.n_atoms = n_atoms;
    pa.k = K;
    pa.cls = L.cls;
    for (int r = 0; r < PNX_MAX_PARAMS; ++r) pa.row_src[r] = L.row_src[r];
    hipLaunchKernelGGL(varpro_params_kernel, dim3((n * cols + 255) / 256), dim3(256), 0, st, pa);
    VP_HIP(hipGetLastError());
    pnx_curvefit_opts c = *o;
    c.fixed_per_voxel = 0;
    if (int rc = model_predict_device(&c, cols, n_b, b, params, fixed_host, nullptr, raw, nullptr, st)) return rc;
    FinishArgs a;
    memset(&a, 0, sizeof(a));
    a.raw = raw;
    a.st = stt;
    a.cst = cst;
    a.wd = wd;
    a.n_atoms = n_atoms;
    a.n_b = n_b;
    a.kpad = kpad;
    a.gp = gp;
    a.k = K;
    a.cls = L.cls;
    for (int i = 0; i < n_b; ++i) a.w[i] = o->sigma ? 1.0 / o->sigma[i] : 1.0;  // transform = 1.0 / sigma, as the fit
    const int lanes = gp > kpad ? gp : kpad;
    const dim3 grid((lanes + 255) / 256), block(256);
    if (K == 1)
        hipLaunchKernelGGL(varpro_finish_kernel<1>, grid, block, 0, st, a);
    else if (K == 2)
        hipLaunchKernelGGL(varpro_finish_kernel<2>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(varpro_finish_kernel<3>, grid, block, 0, st, a);
    VP_HIP(hipGetLastError());
    D->nl = nl_d;
    D->st = stt;
    D->cst = cst;
    D->w = wd;
    D->n_b = n_b;
    D->n_free = n;
    D->n_atoms = n_atoms;
    D->gp = gp;
    D->L = L;
    for (int r = 0; r < PNX_MAX_PARAMS; ++r) D->fallback[r] = r < n ? fallback[r] : 0.0;
    return PNX_OK;
}

// ---- match ------------------------------------------------------------------------------------------------------------------
// A block is four waves, one per SIMD; a wave owns MS strips of 16 voxels per pass, a block 64 MS voxels.  Per accumulator row a
// lane keeps (min, packed argmin, a'): with K = 3 and MS = 2 that, the 3 x 2 accumulator tiles, the y fragments and the twelve
// constants of the atom take more than the 256 registers a lane has at two waves per SIMD, so the block is half of grid start's
// (the posterior's choice, pnx_grid_posterior.hip).  The dictionary comes through LDS in slabs of `width` atoms
// (pnx_varpro_args.hpp varpro_slab): K blocks of [kpad][stride], then the constant rows, each `width` wide.  NS: k-steps the
// register file is sized for (n_b <= 4 NS).
constexpr int kVarproWaves = 4;

struct VarproArgs {
    const double *y;    // (n_vox, n_b)
    const double *st;   // (K kpad, gp)
    const double *cst;  // (crow, gp)
    const double *wd;   // (kpad)
    const double *nl;   // (n_nl, n_atoms)
    double *p_out;      // (n_free, n_vox)
    int32_t *best;      // (n_vox) or null
    double *cost;       // (n_vox) or null
    int8_t *clipped;    // (n_vox) or null
    long long n_vox;
    int n_b, kpad, n_atoms, gp, n_free, width, stride;
    int row_src[PNX_MAX_PARAMS];
    double fallback[PNX_MAX_PARAMS];
    double lo[3], hi[3];  // bounds of the linear slots (S0 class: slot K - 1 is S0)
};

template <int NS, int MS, int K, int CLS>
__global__ void __launch_bounds__(kVarproWaves * 64) varpro_match_kernel(const VarproArgs a) {
    constexpr int NM = K * (K + 1) / 2;
    extern __shared__ double lds[];  // [K kpad][stride] | constants [2 NM][width]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_b = a.n_b, kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lc = lds + K * kpad * stride;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kVarproWaves * MS - 1) / (kVarproWaves * MS);
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        // A fragments of this wave's strips, as grid start loads them: rows past the end repeat the last voxel, never stored
        double yf[MS][NS], yy[MS];
        int nf[MS];
        long long v0[MS];
#pragma unroll
        for (int m = 0; m < MS; ++m) {
            v0[m] = ((grp * kVarproWaves + wave) * MS + m) * 16;
            const long long v = v0[m] + r16;
            const double *row = a.y + (size_t)(v < a.n_vox ? v : a.n_vox - 1) * n_b;
            double ss = 0.0;
            int bad = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int k = 4 * s + kq;
                const double val = (s < ksteps && k < n_b) ? row[k] * a.wd[k] : 0.0;
                bad |= !(fabs(val) < inf);  // NaN or Inf, of the signal or through a zero sigma
                ss = fma(val, val, ss);
                yf[m][s] = val;
            }
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            bad |= __shfl_xor(bad, 16);
            bad |= __shfl_xor(bad, 32);
            yy[m] = ss;  // ||y||^2 of row r16, the same in its four lanes
            nf[m] = bad;
        }
        double bm[MS][4], bq[MS][4][K];
        int bg[MS][4];  // 2 g + clipped: ordered as g
#pragma unroll
        for (int m = 0; m < MS; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bm[m][r] = inf;
                bg[m][r] = INT_MAX;
#pragma unroll
                for (int i = 0; i < K; ++i) bq[m][r][i] = 0.0;
            }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                for (int k = wave; k < K * kpad; k += kVarproWaves)
                    for (int j = lane; j < wc; j += 64) lds[k * stride + j] = a.st[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < 2 * NM; k += kVarproWaves)
                    for (int j = lane; j < wc; j += 64) lc[k * W + j] = a.cst[(size_t)k * a.gp + g0 + j];
                __syncthreads();
                resident = n_slabs == 1;
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc[K][MS];
#pragma unroll
                for (int i = 0; i < K; ++i)
#pragma unroll
                    for (int m = 0; m < MS; ++m) acc[i][m] = f64x4{0.0, 0.0, 0.0, 0.0};
                const double *bp = lds + kq * stride + t * 16 + r16;  // B fragment: phi_i[g0 + 16 t + r16][4 s + kq]
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (s < ksteps) {
#pragma unroll
                        for (int i = 0; i < K; ++i) {
                            const double bf = bp[(i * kpad + 4 * s) * stride];
#pragma unroll
                            for (int m = 0; m < MS; ++m) acc[i][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(yf[m][s], bf, acc[i][m], 0, 0, 0);
                        }
                    }
                }
                // fold: this lane's atom against its four voxels of each strip; atoms arrive in ascending order, so a strict
                // comparison keeps the lowest index among equal costs; a padded atom costs +inf and never wins
                const int j16 = t * 16 + r16, g = g0 + j16;
                const bool live = g < a.n_atoms;
                double M[NM], I[NM];
#pragma unroll
                for (int q = 0; q < NM; ++q) {
                    M[q] = lc[q * W + j16];
                    I[q] = lc[(NM + q) * W + j16];
                }
#pragma unroll
                for (int m = 0; m < MS; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double c[K], ap[K], q[K];
#pragma unroll
                        for (int i = 0; i < K; ++i) c[i] = acc[i][m][r];
                        bool clip = false;
                        if constexpr (CLS == kVarproReduced) {
                            // a_hat of the K - 1 free amplitudes: N^-1 ((c_i - c_K) - off_i); I = N^-1 packed, then the offsets
                            constexpr int NN = (K - 1) * K / 2;
                            double tt[K], rest = 1.0;
#pragma unroll
                            for (int i = 0; i < K - 1; ++i) tt[i] = (c[i] - c[K - 1]) - I[NN + i];
#pragma unroll
                            for (int i = 0; i < K - 1; ++i) {
                                double ah = 0.0;
#pragma unroll
                                for (int j = 0; j < K - 1; ++j) ah = fma(I[pk(i, j)], tt[j], ah);
                                ap[i] = fmin(fmax(ah, a.lo[i]), a.hi[i]);
                                clip |= ap[i] != ah;
                                q[i] = ap[i];
                                rest -= ap[i];
                            }
                            ap[K - 1] = rest;
                            q[K - 1] = 0.0;
                        } else {
                            double ah[K], sum = 0.0;
#pragma unroll
                            for (int i = 0; i < K; ++i) {
                                ah[i] = 0.0;
#pragma unroll
                                for (int j = 0; j < K; ++j) ah[i] = fma(I[pk(i, j)], c[j], ah[i]);
                                sum += ah[i];
                            }
                            if constexpr (CLS == kVarproFree) {
#pragma unroll
                                for (int i = 0; i < K; ++i) {
                                    ap[i] = fmin(fmax(ah[i], a.lo[i]), a.hi[i]);
                                    clip |= ap[i] != ah[i];
                                    q[i] = ap[i];
                                }
                            } else {  // S0 class: the amplitude sum first, the fraction bounds scale with it
                                const double S = fmin(fmax(sum, a.lo[K - 1]), a.hi[K - 1]);
                                clip |= S != sum;
                                double rest = S;
#pragma unroll
                                for (int i = 0; i < K - 1; ++i) {
                                    ap[i] = fmin(fmax(ah[i], a.lo[i] * S), a.hi[i] * S);
                                    clip |= ap[i] != ah[i];
                                    q[i] = ap[i];
                                    rest -= ap[i];
                                }
                                ap[K - 1] = rest;
                                q[K - 1] = S;
                            }
                        }
                        // cc = cost - 0.5 ||y||^2 = 0.5 a'^T M a' - c . a'
                        double cc = 0.0;
#pragma unroll
                        for (int i = 0; i < K; ++i) {
                            double ma = 0.0;
#pragma unroll
                            for (int j = 0; j < K; ++j) ma = fma(M[pk(i, j)], ap[j], ma);
                            cc = fma(ap[i], fma(0.5, ma, -c[i]), cc);
                        }
                        cc = live ? cc : inf;
                        if (cc < bm[m][r]) {
                            bm[m][r] = cc;
                            bg[m][r] = 2 * g + (clip ? 1 : 0);
#pragma unroll
                            for (int i = 0; i < K; ++i) bq[m][r][i] = q[i];
                        }
                    }
            }
        }
        // one reduction over the 16 lanes (atoms modulo 16) that share a voxel: lower cost, then lower index -- symmetric, so
        // every lane of the group ends with the same answer and lane r16 writes output row r16
#pragma unroll
        for (int m = 0; m < MS; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double c = bm[m][r], q[K];
                int g = bg[m][r];
#pragma unroll
                for (int i = 0; i < K; ++i) q[i] = bq[m][r][i];
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) {
                    const double oc = __shfl_xor(c, off, 16);
                    const int og = __shfl_xor(g, off, 16);
                    const bool take = oc < c || (oc == c && og < g);
#pragma unroll
                    for (int i = 0; i < K; ++i) {
                        const double oq = __shfl_xor(q[i], off, 16);
                        q[i] = take ? oq : q[i];
                    }
                    c = take ? oc : c;
                    g = take ? og : g;
                }
                const int src = kq + 4 * r;  // this voxel's row of the strip: its ||y||^2 and finite flag live in lane `src`
                const double yyv = __shfl(yy[m], src);
                const int badv = __shfl(nf[m], src) | (g == INT_MAX);
                const long long v = v0[m] + src;
                if (v < a.n_vox) {
                    const int gi = badv ? 0 : g >> 1;
                    if (r16 < a.n_free) {
                        int rs = 0;
                        double fb = 0.0;
#pragma unroll
                        for (int k = 0; k < PNX_MAX_PARAMS; ++k)
                            if (r16 == k) {
                                rs = a.row_src[k];
                                fb = a.fallback[k];
                            }
                        double val;
                        if (rs >= 0) {
                            val = a.nl[(size_t)rs * a.n_atoms + gi];
                        } else {
                            const int slot = -1 - rs;
                            double qs = q[0], ls = a.lo[0], hs = a.hi[0];
#pragma unroll
                            for (int i = 1; i < K; ++i)
                                if (slot == i) {
                                    qs = q[i];
                                    ls = a.lo[i];
                                    hs = a.hi[i];
                                }
                            val = qs;
                            // f_j = a'_j / S; the quotient of a'_j = hi_fj S may round one ulp past hi_fj: kept inside the box
                            if (CLS == kVarproS0 && slot != K - 1) val = q[K - 1] > 0.0 ? fmin(fmax(qs / q[K - 1], ls), hs) : ls;
                        }
                        a.p_out[(size_t)r16 * a.n_vox + v] = badv ? fb : val;
                    } else if (r16 == 8) {
                        if (a.best) a.best[v] = badv ? -1 : gi;
                    } else if (r16 == 9) {
                        if (a.cost) a.cost[v] = badv ? __builtin_nan("") : fma(0.5, yyv, c);
                    } else if (r16 == 10) {
                        if (a.clipped) a.clipped[v] = badv ? 0 : (int8_t)(g & 1);
                    }
                }
            }
    }
}

template <int NS, int MS, int K, int CLS> static int launch_one(const VarproArgs &a, size_t lds, long long n_strips, int cus, hipStream_t st) {
    long long blocks = (n_strips + kVarproWaves * MS - 1) / (kVarproWaves * MS);
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((varpro_match_kernel<NS, MS, K, CLS>), dim3((unsigned)blocks), dim3(kVarproWaves * 64), lds, st, a);
    VP_HIP(hipGetLastError());
    return PNX_OK;
}

template <int K, int CLS> static int launch_ns(const VarproArgs &a, size_t lds, long long n_strips, int cus, hipStream_t st) {
    if (a.kpad <= 32) return launch_one<8, 2, K, CLS>(a, lds, n_strips, cus, st);
    if (a.kpad <= 64) return launch_one<16, 2, K, CLS>(a, lds, n_strips, cus, st);
    return launch_one<32, 1, K, CLS>(a, lds, n_strips, cus, st);
}

int varpro_match_device(const VarproDict &D, int64_t n_vox, const double *y_d, double *p_out_d, int32_t *best_d, double *cost_d,
                        int8_t *clipped_d, int cus, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const VarproLayout &L = D.L;
    const GridSlab S = varpro_slab(D.n_b, L.k);
    VarproArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.cst = D.cst;
    a.wd = D.w;
    a.nl = D.nl;
    a.p_out = p_out_d;
    a.best = best_d;
    a.cost = cost_d;
    a.clipped = clipped_d;
    a.n_vox = n_vox;
    a.n_b = D.n_b;
    a.kpad = S.kpad;
    a.n_atoms = D.n_atoms;
    a.gp = D.gp;
    a.n_free = D.n_free;
    a.width = S.width < D.gp ? S.width : D.gp;
    a.stride = S.stride;
    for (int r = 0; r < PNX_MAX_PARAMS; ++r) {
        a.row_src[r] = L.row_src[r];
        a.fallback[r] = D.fallback[r];
    }
    for (int j = 0; j < 3; ++j) {
        a.lo[j] = L.lin_lo[j];
        a.hi[j] = L.lin_hi[j];
    }
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    const long long n_strips = (n_vox + 15) / 16;
    switch (L.k * 4 + L.cls) {
    case 1 * 4 + kVarproFree: return launch_ns<1, kVarproFree>(a, lds, n_strips, cus, stream);
    case 2 * 4 + kVarproFree: return launch_ns<2, kVarproFree>(a, lds, n_strips, cus, stream);
    case 2 * 4 + kVarproReduced: return launch_ns<2, kVarproReduced>(a, lds, n_strips, cus, stream);
    case 2 * 4 + kVarproS0: return launch_ns<2, kVarproS0>(a, lds, n_strips, cus, stream);
    case 3 * 4 + kVarproFree: return launch_ns<3, kVarproFree>(a, lds, n_strips, cus, stream);
    case 3 * 4 + kVarproReduced: return launch_ns<3, kVarproReduced>(a, lds, n_strips, cus, stream);
    case 3 * 4 + kVarproS0: return launch_ns<3, kVarproS0>(a, lds, n_strips, cus, stream);
    }
    return set_error(PNX_ERR_INVALID, "varpro: no kernel for %d compartments, class %d", L.k, L.cls);
}

}  // namespace pnx
