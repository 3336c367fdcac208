// pnx_predict.hip -- what a user does after a fit, on the device: the forward model and the data-term residual of both
// solver families as HBM-streaming kernels.
//
//   nnls_fit_stats_kernel   pred = B x and ss_res = ||y - B x||^2 per voxel from the spectra of an NNLS fit.  rnorm cannot
//                           serve: it contains the regulariser rows.  16 flop per byte at 250 x 32, so the product runs on
//                           v_mfma_f64_16x16x4_f64 like the Gram step (pnx_nnls.hip nnls_aty_mfma_kernel is the transposed product).
//   model_predict_kernel    pred = model(x; params) of the seven parametric layouts at any <= 128 x-values, optionally
//                           ss_res against a signal (the residual of failed voxels, which return p0, without a host loop).
#include <hip/hip_runtime.h>

#include <cstring>

#include "pnx_curvefit_kernel.hpp"
#include "pnx_launch.hpp"
#include "pnx_nnls.hpp"
#include "pnx_predict.hpp"
#include "pnx_tile.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;
using f64x2 = __attribute__((ext_vector_type(2))) double;

// ---- NNLS: pred = X B^T on the matrix cores ---------------------------------------------------------------------------------
// One wave owns a strip of 16 voxels; the block's LDS holds B^T for a group of G = 16 NT measurements, [k][G], K = n_bins
// padded to a multiple of 8 with zero rows, measurements beyond n_meas zero columns: partial tiles need no branch in the
// product.  The MFMA's k index is free as long as both operands agree, so a lane reads its voxel's coefficients as 16-byte
// pairs -- pair (8 t + 2 kq, + 1) feeds steps 2 t and 2 t + 1 -- and the LDS copy is stored in that order: row
// r = 8 t + 4 h + kq holds k = 8 t + 2 kq + h.  Four lanes cover 64 contiguous bytes of a row per load.  Lanes l and l + 16
// (kq and kq + 1) read adjacent LDS rows: 128 bytes apart at G = 16, and at G = 32 odd rows are stored with their two
// 16-column halves swapped, so the two always hit opposite halves of the 256-byte bank row (ds_read_b64 banks per 32 lanes).
// 64 KB of LDS hold 32 measurements up to 256 bins and 16 beyond; more measurements take further passes over the
// spectra, each adding its part of ss_res to what the same lane stored in the pass before.
constexpr int kStatsWaves = 8;
constexpr int kStatsLdsDoubles = 8192;

template <int NT, bool VEC>
__global__ void __launch_bounds__(kStatsWaves * 64) nnls_fit_stats_kernel(const double *__restrict__ X, const double *__restrict__ Y,
                                                                          const double *__restrict__ Bp, double *SS, double *PRED,
                                                                          long long n_vox, int n_bins, int n_meas, int bstride) {
    extern __shared__ double bsm[];  // [kpad][G]
    constexpr int G = NT * 16;
    const int kpad = (n_bins + 7) & ~7;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const long long n_strips = (n_vox + 15) / 16;
    for (int jg = 0; jg < n_meas; jg += G) {
        if (jg) __syncthreads();  // every wave has left the previous group's copy behind
        for (int e = threadIdx.x; e < G * kpad; e += blockDim.x) {
            const int c = e / kpad, k = e - c * kpad, j = jg + c;
            const int r = (k & ~7) | ((k & 1) << 2) | ((k >> 1) & 3);
            const int col = NT == 2 ? c ^ ((r & 1) << 4) : c;
            bsm[r * G + col] = (k < n_bins && j < n_meas) ? Bp[(size_t)j * bstride + k] : 0.0;
        }
        __syncthreads();
        // this lane's B fragment of tile t sits at column boff[t] of its row
        int boff[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) boff[t] = (NT == 2 ? (t ^ (kq & 1)) : t) * 16 + r16;
        for (long long st = (long long)blockIdx.x * kStatsWaves + wave; st < n_strips; st += (long long)gridDim.x * kStatsWaves) {
            const long long v0 = st * 16;
            const long long va = (v0 + r16) < n_vox ? (v0 + r16) : (n_vox - 1);  // rows past the end repeat the last voxel, never stored
            const double *xrow = X + (size_t)va * n_bins;
            f64x4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
            for (int k8 = 0; k8 < kpad; k8 += 8) {
                const int p = k8 + 2 * kq;
                double x0, x1;
                if constexpr (VEC) {  // n_bins even: a pair lies inside the row or wholly in the zero padding (read at 0 then)
                    const f64x2 xv = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(xrow + (p < n_bins ? p : 0)));
                    x0 = xv.x;
                    x1 = xv.y;
                } else {
                    x0 = __builtin_nontemporal_load(xrow + (p < n_bins ? p : 0));
                    x1 = __builtin_nontemporal_load(xrow + (p + 1 < n_bins ? p + 1 : 0));
                }
                const double *b0 = bsm + (k8 + kq) * G, *b1 = bsm + (k8 + 4 + kq) * G;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, b0[boff[t]], acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, b1[boff[t]], acc[t], 0, 0, 0);
                }
            }
            // D: column (measurement) = lane & 15, row (voxel of the strip) = kq + 4 * reg
            double part[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int j = jg + t * 16 + r16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long vrow = v0 + kq + 4 * r;
                    const bool ok = j < n_meas && vrow < n_vox;
                    const size_t at = ok ? (size_t)vrow * n_meas + j : 0;
                    const double pr = acc[t][r];
                    if (PRED && ok) PRED[at] = pr;
                    if (SS) {
                        const double d = ok ? Y[at] - pr : 0.0;
                        part[r] = fma(d, d, part[r]);
                    }
                }
            }
            if (SS) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#pragma unroll
                    for (int m = 8; m >= 1; m >>= 1) part[r] += __shfl_xor(part[r], m, 16);
                    const long long vrow = v0 + kq + 4 * r;
                    if (r16 == 0 && vrow < n_vox) SS[vrow] = jg ? SS[vrow] + part[r] : part[r];
                }
            }
        }
    }
}

template <int NT, bool VEC>
static int launch_stats(const NnlsPlanData *P, int64_t n_vox, const double *y, const double *x, double *ss, double *pred, hipStream_t st) {
    const int kpad = (P->n_bins + 7) & ~7;
    const size_t lds = (size_t)kpad * NT * 16 * sizeof(double);
    const long long n_strips = (n_vox + 15) / 16;
    long long blocks = (n_strips + kStatsWaves - 1) / kStatsWaves;
    const long long cap = (long long)(P->cus > 0 ? P->cus : 256) * 2;  // two 64 KB copies of the basis per CU
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((nnls_fit_stats_kernel<NT, VEC>), dim3((unsigned)blocks), dim3(kStatsWaves * 64), lds, st, x, y, P->Bp, ss, pred,
                       (long long)n_vox, P->n_bins, P->n_meas, P->bstride);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

int nnls_fit_stats_device(const NnlsPlanData *P, int64_t n_vox, const double *y_d, const double *coeff_d, double *ss_res_d,
                          double *pred_d, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const int kpad = (P->n_bins + 7) & ~7;
    // two tiles (32 measurements per pass) where their copy of the basis fits the 64 KB
    const bool two = P->n_meas > 16 && kpad * 32 <= kStatsLdsDoubles;
    if (kpad * 16 > kStatsLdsDoubles) return set_error(PNX_ERR_UNSUPPORTED, "fit_stats: n_bins=%d > %d", P->n_bins, kStatsLdsDoubles / 16);
    const bool vec = (P->n_bins & 1) == 0 && ((uintptr_t)coeff_d & 15) == 0;
    if (two) return vec ? launch_stats<2, true>(P, n_vox, y_d, coeff_d, ss_res_d, pred_d, stream) : launch_stats<2, false>(P, n_vox, y_d, coeff_d, ss_res_d, pred_d, stream);
    return vec ? launch_stats<1, true>(P, n_vox, y_d, coeff_d, ss_res_d, pred_d, stream) : launch_stats<1, false>(P, n_vox, y_d, coeff_d, ss_res_d, pred_d, stream);
}

// ---- parametric models: one lane per voxel ----------------------------------------------------------------------------------
// A block is one wave and 64 voxels.  The (64, n_x) tile of the output goes through LDS and leaves as 16-byte lines, lane after
// lane (pnx_tile.hpp: store_tile, [voxel][n_x | 1] doubles); a signal tile comes in the same way (load_tile).  The x-values are
// kernel arguments, read with scalar loads (one table for the whole grid, as the fit's b-values).
struct PredictArgs {
    const double *params;  // (n_free, n_vox)
    const double *fixed;   // (n_fixed, n_vox) when fixed_pv
    const double *y;       // (n_vox, n_x) or null
    double *pred;          // (n_vox, n_x) or null
    double *ss;            // (n_vox) or null
    long long n_vox;
    int n_x;
    int steam;
    int fixed_pv;
    double tr, tm;
    int is_free[kMaxP];  // per model parameter: free (row of params) or fixed (row of fixed / entry of fixeds)
    int row[kMaxP];
    double fixeds[kMaxP];
    double x[kMaxB];
};

static_assert(kWave == kTileRows, "a block of model_predict_kernel is the tile helpers' one wave");
template <int MODEL, bool T1>
__global__ void __launch_bounds__(kWave) model_predict_kernel(const PredictArgs a) {
    using M = Model<MODEL>;
    constexpr int NALL = M::NALL, NC = M::NC, NP = NALL + (T1 ? 1 : 0);
    extern __shared__ double tile[];  // [64][S]
    const int lane = threadIdx.x, n_x = a.n_x, S = n_x | 1;
    const long long v0 = (long long)blockIdx.x * kWave;
    const int c = (a.n_vox - v0) < kWave ? (int)(a.n_vox - v0) : kWave;
    const int n_el = c * n_x;
    if (a.y) {
        load_tile(tile, a.y, v0, n_el, n_x, lane);
        __syncthreads();
    }
    const size_t v = (size_t)v0 + (lane < c ? lane : c - 1);  // lanes past the end repeat the last voxel, never stored
    double p[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int r = a.row[j];
        p[j] = a.is_free[j] ? a.params[(size_t)r * a.n_vox + v] : (a.fixed_pv ? a.fixed[(size_t)r * a.n_vox + v] : a.fixeds[r]);
    }
    double A1 = 1.0, eTM = 1.0;
    if constexpr (T1) {  // S = base * A1 [* eTM], as the fit's row pass (pnx_curvefit_kernel.hpp)
        const double T1v = p[NALL];
        A1 = 1 - exp(-a.tr / T1v);
        eTM = a.steam ? exp(-a.tm / T1v) : 1.0;
    }
    double ss = 0.0;
    double *mine = tile + lane * S;
    for (int i = 0; i < n_x; ++i) {
        const double nb = -a.x[i];
        double E[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) E[k] = exp_fast(nb * p[M::dpos(k)]);
        const double base = M::signal(p, E);
        const double s = T1 ? base * A1 * eTM : base;
        if (a.y) {
            const double d = s - mine[i];
            ss = fma(d, d, ss);
        }
        if (a.pred) mine[i] = s;
    }
    if (a.ss && lane < c) a.ss[v] = ss;
    if (a.pred) {
        __syncthreads();
        store_tile(a.pred, v0, tile, n_el, n_x, lane);
    }
}

template <int MODEL, bool T1> static int launch_predict(const PredictArgs &a, hipStream_t st) {
    PNX_ALLOW_BIG_LDS(model_predict_kernel<MODEL, T1>);
    const size_t lds = tile_lds_bytes(1, a.n_x);  // 66 KB at 128 x-values
    const long long blocks = (a.n_vox + kWave - 1) / kWave;
    if (blocks > 0x7fffffffLL) return set_error(PNX_ERR_UNSUPPORTED, "predict: n_vox=%lld in one launch", a.n_vox);
    hipLaunchKernelGGL((model_predict_kernel<MODEL, T1>), dim3((unsigned)blocks), dim3(kWave), lds, st, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

int model_predict_device(const pnx_curvefit_opts *o, int64_t n_vox, int n_x, const double *x, const double *params_d,
                         const double *fixed, const double *y_d, double *pred_d, double *ss_res_d, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    PredictArgs a;
    memset(&a, 0, sizeof(a));
    a.params = params_d;
    a.y = y_d;
    a.pred = pred_d;
    a.ss = ss_res_d;
    a.n_vox = n_vox;
    a.n_x = n_x;
    a.steam = o->t1_mode == 2;
    a.fixed_pv = o->n_fixed && o->fixed_per_voxel;
    a.tr = o->tr;
    a.tm = o->tm;
    for (int k = 0; k < o->n_free; ++k) {
        a.is_free[o->free_idx[k]] = 1;
        a.row[o->free_idx[k]] = k;
    }
    for (int k = 0; k < o->n_fixed; ++k) {
        a.row[o->fixed_idx[k]] = k;
        if (!a.fixed_pv) a.fixeds[k] = fixed[k];
    }
    if (a.fixed_pv) a.fixed = fixed;
    for (int i = 0; i < n_x; ++i) a.x[i] = x[i];
#define PNX_PREDICT_CASE(m) \
    case m: return o->t1_mode ? launch_predict<m, true>(a, stream) : launch_predict<m, false>(a, stream);
    switch (o->model) {
        PNX_PREDICT_CASE(0)
        PNX_PREDICT_CASE(1)
        PNX_PREDICT_CASE(2)
        PNX_PREDICT_CASE(3)
        PNX_PREDICT_CASE(4)
        PNX_PREDICT_CASE(5)
        PNX_PREDICT_CASE(6)
    }
#undef PNX_PREDICT_CASE
    return set_error(PNX_ERR_INVALID, "unknown model %d", o->model);
}

}  // namespace pnx
