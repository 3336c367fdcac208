// pnx_peel.hip -- exponential peeling ("curve stripping") of the mono-, bi- and tri-exponential layouts per voxel (pnx_peel_f64 /
// _f32): K log-linear stages, the slowest compartment first, each on its own b-values and on what the stages
// before left of the signal.  A closed form: a voxel costs its signal row in and its results out.
//
//   peel_kernel<T>   one lane per voxel, one wave and 64 voxels per block.  The block's (64, n_b) signal tile comes into LDS
//                    through the shared loader (pnx_tile.hpp: load_tile, [voxel][n_b | 1] doubles).  A second tile of the same
//                    shape holds the running residual r, one row per lane: a stage reads it twice (the weighted means, then
//                    the centred sums: loglinear_kernel's line fit, operation for operation) and rewrites it once.  y itself
//                    stays for ss_res.  Two tiles are 132 KB at 128 b-values and a third does not fit, so no logarithm is kept at
//                    any n_b: both passes of a stage evaluate log r (the same instruction sequence on the same value, hence the
//                    same bits).  Per stage only A_k, D_k and n_used stay in registers.  b-values, the K masks, bounds and
//                    fallback are kernel arguments, read with scalar loads.
//                    T is the storage type (double / float); the tiles and the arithmetic are fp64 for both.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pnx_launch.hpp"
#include "pnx_peel.hpp"
#include "pnx_tile.hpp"

namespace pnx {

template <typename T> struct PeelArgs {
    PeelOpts o;
    const T *y;       // (n_vox, n_b)
    T *params;        // (n_params, n_vox)
    int8_t *status;   // or null
    int32_t *n_used;  // (n_stage, n_vox) or null
    T *ss;            // (n_vox) or null
    long long n_vox;
};

template <typename T> __global__ void __launch_bounds__(kTileRows) peel_kernel(const PeelArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) double peel_tile[];  // y [64][S], then r [64][S]
    const int lane = threadIdx.x, n_b = a.o.n_b, S = n_b | 1, K = a.o.n_stage;
    double *ty = peel_tile, *tr = peel_tile + kTileRows * S;
    const long long v0 = (long long)blockIdx.x * kTileRows;
    const int c = (a.n_vox - v0) < kTileRows ? (int)(a.n_vox - v0) : kTileRows;
    const int n_el = c * n_b;
    load_tile(ty, a.y, v0, n_el, n_b, lane);
    __syncthreads();
    const int rl = lane < c ? lane : c - 1;  // lanes past the end repeat the last voxel, never stored
    const double *my = ty + rl * S;
    double *mr = tr + lane * S;  // every lane keeps its residual in a row of its own
    const double kNaN = __builtin_nan("");
    const double kMax = 1.7976931348623157e308;
    auto bit = [](unsigned long long w0, unsigned long long w1, int i) { return ((i < 64 ? w0 : w1) >> (i & 63)) & 1ull; };

    // r = y; a non-finite sample of any stage's b-values makes the voxel unusable
    const unsigned long long m0 = a.o.use[0][0] | a.o.use[1][0] | a.o.use[2][0], m1 = a.o.use[0][1] | a.o.use[1][1] | a.o.use[2][1];
    bool nonfinite = false;
    for (int i = 0; i < n_b; ++i) {
        const double yi = my[i];
        mr[i] = yi;
        if (bit(m0, m1, i)) nonfinite |= !(fabs(yi) <= kMax);  // NaN or +-inf; the same branch in every lane
    }

    double A[kPeelMaxStages] = {0.0, 0.0, 0.0}, D[kPeelMaxStages] = {0.0, 0.0, 0.0};
    int nu[kPeelMaxStages] = {0, 0, 0};
    bool alive = true;
    const bool w2 = a.o.weighting == 1;
#pragma unroll
    for (int k = 0; k < kPeelMaxStages; ++k) {
        if (k >= K) continue;  // the same in every lane
        const unsigned long long u0 = a.o.use[k][0], u1 = a.o.use[k][1];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        int n = 0;
        for (int i = 0; i < n_b; ++i) {
            if (!bit(u0, u1, i)) continue;
            const double ri = mr[i], bi = a.o.b[i];
            const bool pos = ri > 0.0;  // a non-positive residual is left out, not clamped
            const double w = pos ? (w2 ? ri * ri : 1.0) : 0.0;
            const double l = pos ? log(ri) : 0.0;
            n += pos;
            s0 += w;
            s1 = fma(w, bi, s1);
            s2 = fma(w, l, s2);
        }
        const double bm = s1 / s0, lm = s2 / s0;
        double sbb = 0.0, sbl = 0.0;
        for (int i = 0; i < n_b; ++i) {
            if (!bit(u0, u1, i)) continue;
            const double ri = mr[i], bi = a.o.b[i];
            const bool pos = ri > 0.0;
            const double w = pos ? (w2 ? ri * ri : 1.0) : 0.0;
            const double l = pos ? log(ri) : 0.0;
            const double db = bi - bm, wdb = w * db;
            sbb = fma(wdb, db, sbb);
            sbl = fma(wdb, l - lm, sbl);
        }
        const double Dk = -sbl / sbb, ak = lm + Dk * bm, Ak = exp(ak);
        const bool ok = n >= 2 && sbb != 0.0 && fabs(ak) <= kMax && fabs(Dk) <= kMax && fabs(Ak) <= kMax;
        nu[k] = alive ? n : 0;  // a stage that was not reached used nothing
        alive = alive && ok;
        A[k] = Ak;
        D[k] = Dk;
        if (k + 1 < K)
            for (int i = 0; i < n_b; ++i) mr[i] -= Ak * exp(-a.o.b[i] * Dk);  // every sample, inside the stage's mask or not
    }

    // stage k is component K - k of the layout (component 1 is the fastest)
    int st = nonfinite ? -2 : (alive ? 1 : 0);
    const double Sum = A[0] + A[1] + A[2];  // the stages that do not exist add an exact 0
    double p[kPeelMaxParams] = {kNaN, kNaN, kNaN, kNaN, kNaN, kNaN};
    const int model = a.o.model, np = a.o.n_params;
    if (model == PNX_MODEL_MONO) {
        p[0] = A[0], p[1] = D[0];
    } else if (model == PNX_MODEL_BI_REDUCED || model == PNX_MODEL_BI_S0) {
        p[0] = A[1] / Sum, p[1] = D[1], p[2] = D[0], p[3] = Sum;
    } else if (model == PNX_MODEL_BI_FULL) {
        p[0] = A[1], p[1] = D[1], p[2] = A[0], p[3] = D[0];
    } else if (model == PNX_MODEL_TRI_REDUCED || model == PNX_MODEL_TRI_S0) {
        p[0] = A[2] / Sum, p[1] = D[2], p[2] = A[1] / Sum, p[3] = D[1], p[4] = D[0], p[5] = Sum;
    } else {
        p[0] = A[2], p[1] = D[2], p[2] = A[1], p[3] = D[1], p[4] = A[0], p[5] = D[0];
    }
    if (a.o.clip && st == 1) {  // comparisons, not fmin / fmax: they keep a NaN
        bool moved = false;
#pragma unroll
        for (int j = 0; j < kPeelMaxParams; ++j) {
            if (j >= np) continue;
            const bool below = p[j] < a.o.lo[j], above = p[j] > a.o.hi[j];
            p[j] = below ? a.o.lo[j] : (above ? a.o.hi[j] : p[j]);
            moved |= below | above;
        }
        if (moved) st = 2;
    }

    // signal-domain residual at the returned point over every sample of any stage: scale * (c1 e1 + c2 e2 + c3 e3)
    const bool want_ss = a.ss != nullptr;
    double ss = 0.0;
    if (want_ss) {
        double scale = 1.0, c1 = p[0], d1 = p[1], c2 = 0.0, d2 = 0.0, c3 = 0.0, d3 = 0.0;
        if (model == PNX_MODEL_BI_REDUCED || model == PNX_MODEL_BI_S0) {
            c2 = 1.0 - p[0], d2 = p[2];
            if (model == PNX_MODEL_BI_S0) scale = p[3];
        } else if (model == PNX_MODEL_BI_FULL) {
            c2 = p[2], d2 = p[3];
        } else if (model == PNX_MODEL_TRI_REDUCED || model == PNX_MODEL_TRI_S0) {
            c2 = p[2], d2 = p[3], c3 = 1.0 - p[0] - p[2], d3 = p[4];
            if (model == PNX_MODEL_TRI_S0) scale = p[5];
        } else if (model == PNX_MODEL_TRI_FULL) {
            c2 = p[2], d2 = p[3], c3 = p[4], d3 = p[5];
        }
        for (int i = 0; i < n_b; ++i) {
            if (!bit(m0, m1, i)) continue;
            const double bi = a.o.b[i];
            double m = c1 * exp(-bi * d1);
            if (K >= 2) m += c2 * exp(-bi * d2);
            if (K >= 3) m += c3 * exp(-bi * d3);
            const double d = scale * m - my[i];
            ss = fma(d, d, ss);
        }
    }
    if (lane >= c) return;
    const size_t v = (size_t)v0 + lane, nv = (size_t)a.n_vox;
    const bool failed = st <= 0;
#pragma unroll
    for (int j = 0; j < kPeelMaxParams; ++j) {
        if (j >= np) continue;
        a.params[j * nv + v] = (T)(failed ? (a.o.has_fallback ? a.o.fallback[j] : kNaN) : p[j]);
    }
    if (a.status) a.status[v] = (int8_t)st;
    if (a.n_used) {
#pragma unroll
        for (int k = 0; k < kPeelMaxStages; ++k)
            if (k < K) a.n_used[k * nv + v] = st == -2 ? 0 : nu[k];
    }
    if (want_ss) a.ss[v] = (T)(failed ? kNaN : ss);
}

template <typename T>
int peel_device(const PeelOpts &o, int64_t n_vox, const T *y_d, T *params_d, int8_t *status_d, int32_t *n_used_d, T *ss_res_d,
                hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    PNX_ALLOW_BIG_LDS(peel_kernel<T>);
    const long long blocks = (n_vox + kTileRows - 1) / kTileRows;
    if (blocks > 0x7fffffffLL) return set_error(PNX_ERR_UNSUPPORTED, "peel: n_vox=%lld in one launch", (long long)n_vox);
    PeelArgs<T> a;
    memset(&a, 0, sizeof(a));
    a.o = o;
    a.y = y_d;
    a.params = params_d;
    a.status = status_d;
    a.n_used = n_used_d;
    a.ss = ss_res_d;
    a.n_vox = n_vox;
    hipLaunchKernelGGL((peel_kernel<T>), dim3((unsigned)blocks), dim3(kTileRows), peel_lds_bytes(o.n_b), stream, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

template int peel_device<double>(const PeelOpts &, int64_t, const double *, double *, int8_t *, int32_t *, double *, hipStream_t);
template int peel_device<float>(const PeelOpts &, int64_t, const float *, float *, int8_t *, int32_t *, float *, hipStream_t);

}  // namespace pnx
