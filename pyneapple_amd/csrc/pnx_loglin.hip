// pnx_loglin.hip -- the log-linear mono-exponential fit ln S = ln S0 - b D per voxel (pnx_loglinear_f64 / _f32):
// a closed form over one pass of the data, so a voxel costs its signal row in and its results out.
//
//   loglinear_kernel<T>   one lane per voxel, one wave and 64 voxels per block.  The block's (64, n_b) signal tile comes into LDS
//                         through the shared loader (pnx_tile.hpp: load_tile, [voxel][n_b | 1] doubles).  A second tile of the
//                         same shape keeps log y: every later pass -- the centred sums (the line fit that every stage of
//                         peel_kernel repeats), the re-weighting passes, both residuals -- reads LDS and evaluates no logarithm
//                         again.  b-values, mask and bounds are kernel arguments, read with scalar loads.
//                         T is the storage type (double / float); the tile and the arithmetic are fp64 for both.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pnx_launch.hpp"
#include "pnx_loglin.hpp"
#include "pnx_tile.hpp"

namespace pnx {

template <typename T> struct LogLinArgs {
    LogLinOpts o;
    const T *y;       // (n_vox, n_b)
    T *params;        // (2, n_vox)
    T *pcov;          // (n_vox, 2, 2) or null
    int8_t *status;   // or null
    int32_t *n_used;  // or null
    T *ss;            // (n_vox) or null
    long long n_vox;
};

// weight of a usable sample: 1, y^2, or exp(a - b D)^2 at the previous estimate (mode 2)
__device__ __forceinline__ double ll_weight(int mode, double y, double b, double a, double D) {
    if (mode == 0) return 1.0;
    if (mode == 1) return y * y;
    const double e = exp(a - b * D);
    return e * e;
}

template <typename T> __global__ void __launch_bounds__(kTileRows) loglinear_kernel(const LogLinArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) double ll_tile[];  // y [64][S], then log y [64][S]
    const int lane = threadIdx.x, n_b = a.o.n_b, S = n_b | 1;
    double *ty = ll_tile, *tl = ll_tile + kTileRows * S;
    const long long v0 = (long long)blockIdx.x * kTileRows;
    const int c = (a.n_vox - v0) < kTileRows ? (int)(a.n_vox - v0) : kTileRows;
    const int n_el = c * n_b;
    load_tile(ty, a.y, v0, n_el, n_b, lane);
    __syncthreads();
    const int rl = lane < c ? lane : c - 1;  // lanes past the end repeat the last voxel, never stored
    const double *my = ty + rl * S;
    double *ml = tl + lane * S;  // every lane keeps the logarithms in a row of its own
    auto used = [&](int i) { return (a.o.use[i >> 6] >> (i & 63)) & 1ull; };  // the same in every lane: a scalar branch

    // the logarithms, once; what makes the voxel unusable
    bool nonfinite = false;
    int nu = 0;
    for (int i = 0; i < n_b; ++i) {
        if (!used(i)) continue;
        const double yi = my[i];
        nonfinite |= !(fabs(yi) <= 1.7976931348623157e308);  // NaN or +-inf
        const bool pos = yi > 0.0;
        ml[i] = pos ? log(yi) : 0.0;
        nu += pos;
    }

    // the centred closed form, then n_reweight passes with the weights of the estimate before
    double la = 0.0, D = 0.0, wa = 0.0, wD = 0.0, sw = 0.0, bm = 0.0, sbb = 0.0;
    int mode = a.o.weighting;
    bool ok = nu >= 2;
    for (int p = 0; p <= a.o.n_reweight; ++p) {
        mode = p ? 2 : a.o.weighting;
        wa = la;
        wD = D;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = 0; i < n_b; ++i) {
            if (!used(i)) continue;
            const double yi = my[i], bi = a.o.b[i];
            const double w = yi > 0.0 ? ll_weight(mode, yi, bi, wa, wD) : 0.0;
            s0 += w;
            s1 = fma(w, bi, s1);
            s2 = fma(w, ml[i], s2);
        }
        sw = s0;
        bm = s1 / s0;
        const double lm = s2 / s0;
        double sbl = 0.0;
        sbb = 0.0;
        for (int i = 0; i < n_b; ++i) {
            if (!used(i)) continue;
            const double yi = my[i], bi = a.o.b[i];
            const double w = yi > 0.0 ? ll_weight(mode, yi, bi, wa, wD) : 0.0;
            const double db = bi - bm, wdb = w * db;
            sbb = fma(wdb, db, sbb);
            sbl = fma(wdb, ml[i] - lm, sbl);
        }
        ok = ok && sbb != 0.0;
        D = -sbl / sbb;
        la = lm + D * bm;
    }
    const double kNaN = __builtin_nan("");
    const double kMax = 1.7976931348623157e308;
    ok = ok && fabs(la) <= kMax && fabs(D) <= kMax;
    int st = nonfinite ? -2 : (ok ? 1 : 0);
    double S0 = kNaN, S0c = kNaN, Dc = kNaN;
    if (st == 1) {
        S0 = exp(la);
        S0c = S0;
        Dc = D;
        if (a.o.clip) {  // comparisons, not fmin / fmax: they keep a NaN
            S0c = S0 < a.o.lo[0] ? a.o.lo[0] : (S0 > a.o.hi[0] ? a.o.hi[0] : S0);
            Dc = D < a.o.lo[1] ? a.o.lo[1] : (D > a.o.hi[1] ? a.o.hi[1] : D);
            if (S0c != S0 || Dc != D) st = 2;
        }
    }

    // log-domain residual at the estimate (the last pass's weights) and signal-domain residual at the returned point
    double swr = 0.0, ss = 0.0;
    const bool want_cov = a.pcov != nullptr, want_ss = a.ss != nullptr;
    if (want_cov || want_ss)
        for (int i = 0; i < n_b; ++i) {
            if (!used(i)) continue;
            const double yi = my[i], bi = a.o.b[i];
            if (want_cov) {
                const double w = yi > 0.0 ? ll_weight(mode, yi, bi, wa, wD) : 0.0;
                const double r = ml[i] - (la - bi * D);
                swr = fma(w * r, r, swr);
            }
            if (want_ss) {
                const double d = S0c * exp(-bi * Dc) - yi;
                ss = fma(d, d, ss);
            }
        }
    if (lane >= c) return;
    const size_t v = (size_t)v0 + lane;
    a.params[v] = (T)S0c;
    a.params[(size_t)a.n_vox + v] = (T)Dc;
    if (a.status) a.status[v] = (int8_t)st;
    if (a.n_used) a.n_used[v] = st == -2 ? 0 : nu;
    if (want_ss) a.ss[v] = (T)(st >= 1 ? ss : kNaN);
    if (want_cov) {
        double c00 = kNaN, c01 = kNaN, c11 = kNaN;
        if (st >= 1 && nu >= 3) {
            const double s2 = swr / (double)(nu - 2);
            const double va = s2 * (1.0 / sw + bm * bm / sbb), cad = s2 * bm / sbb;
            c00 = S0 * S0 * va;
            c01 = S0 * cad;
            c11 = s2 / sbb;
        }
        T *pc = a.pcov + 4 * v;
        pc[0] = (T)c00;
        pc[1] = (T)c01;
        pc[2] = (T)c01;
        pc[3] = (T)c11;
    }
}

template <typename T>
int loglinear_device(const LogLinOpts &o, int64_t n_vox, const T *y_d, T *params_d, T *pcov_d, int8_t *status_d, int32_t *n_used_d,
                     T *ss_res_d, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    PNX_ALLOW_BIG_LDS(loglinear_kernel<T>);
    const long long blocks = (n_vox + kTileRows - 1) / kTileRows;
    if (blocks > 0x7fffffffLL) return set_error(PNX_ERR_UNSUPPORTED, "loglinear: n_vox=%lld in one launch", (long long)n_vox);
    LogLinArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.o = o;
    a.y = y_d;
    a.params = params_d;
    a.pcov = pcov_d;
    a.status = status_d;
    a.n_used = n_used_d;
    a.ss = ss_res_d;
    a.n_vox = n_vox;
    hipLaunchKernelGGL((loglinear_kernel<T>), dim3((unsigned)blocks), dim3(kTileRows), loglin_lds_bytes(o.n_b), stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

template int loglinear_device<double>(const LogLinOpts &, int64_t, const double *, double *, double *, int8_t *, int32_t *, double *, hipStream_t);
template int loglinear_device<float>(const LogLinOpts &, int64_t, const float *, float *, float *, int8_t *, int32_t *, float *, hipStream_t);

}  // namespace pnx
