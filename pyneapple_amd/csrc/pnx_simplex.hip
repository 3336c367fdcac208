// pnx_simplex.hip -- the streaming kernels around the constrained curve fit (pnx_curvefit_simplex_f64):
// minimise 0.5 ||model(p) - y||^2 subject to lo <= p <= hi and f1 + f2 <= 1 for the reduced tri-exponential layouts
// [f1, D1, f2, D2, D3 (, S0)].  The fits themselves are the unchanged bounded TRF kernel (pnx_curvefit_kernel.hpp), run twice:
// on every voxel (phase 1), and as the bi-exponential model -- the face f1 + f2 = 1, where f3 = 0 and D3 drops out -- on the
// voxels whose box-only minimum is infeasible (phase 2).  What is new is here:
//
//   simplex_classify_kernel   flags status > 0 && f1 + f2 > 1 per voxel, clears lambda / face, and reduces the smallest phase-1
//                             evaluation count of the violators; hipcub::DeviceSelect::If (the select of pnx_mask_select_f64)
//                             compacts the flagged indices in ascending order
//   simplex_gather_kernel     one wave per 64 violators: their signal rows through an LDS tile into a dense (m, n_b) array
//                             (reads coalesced along each row, 16-byte stores), and one lane per violator for the
//                             parameter-major start values and intersected bounds of the face problem
//   simplex_merge_kernel      one lane per face voxel: the face result in the tri-exponential layout, one row pass with the
//                             fit's own Model<> code for the cost and the gradient entries g_f1, g_f2 of the FULL model, the
//                             multiplier lambda = -(g_f1 + g_f2) / 2 and the certificate face = 1 (lambda >= 0) / 2
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include <hipcub/hipcub.hpp>

#include "pnx_curvefit_kernel.hpp"
#include "pnx_launch.hpp"
#include "pnx_simplex.hpp"

namespace pnx {

using f64x2 = __attribute__((ext_vector_type(2))) double;

struct StreamBuf {  // stream-ordered scratch, freed behind the work that uses it
    void *p = nullptr;
    hipStream_t st = nullptr;
    int alloc(size_t bytes, hipStream_t s) {
        st = s;
        hipError_t e = hipMallocAsync(&p, bytes ? bytes : 8, s);
        if (e != hipSuccess) return set_error(PNX_ERR_NOMEM, "hipMallocAsync(%zu): %s", bytes, hipGetErrorString(e));
        return PNX_OK;
    }
    ~StreamBuf() {
        if (p) (void)hipFreeAsync(p, st);
    }
};

// ---- classify -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) simplex_classify_kernel(const double *__restrict__ f1, const double *__restrict__ f2,
                                                               const int8_t *__restrict__ status, const int32_t *__restrict__ nfev,
                                                               long long n_vox, unsigned char *__restrict__ flags,
                                                               double *__restrict__ lambda, int8_t *__restrict__ face,
                                                               unsigned int *min_nfev) {
    unsigned int mn = UINT_MAX;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_vox; v += (long long)gridDim.x * blockDim.x) {
        const bool viol = status[v] > 0 && (f1[v] + f2[v] > 1.0);
        flags[v] = viol ? 1 : 0;
        if (lambda) lambda[v] = 0.0;  // an interior voxel is a KKT point of the constrained problem with multiplier 0
        if (face) face[v] = 0;
        if (viol) {
            const unsigned int n = (unsigned int)nfev[v];
            mn = n < mn ? n : mn;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned int o = __shfl_xor(mn, m);
        mn = o < mn ? o : mn;
    }
    if ((threadIdx.x & 63) == 0 && mn != UINT_MAX) atomicMin(min_nfev, mn);  // a minimum does not depend on the order
}

struct FlagSet {  // idx -> flags[idx] != 0
    const unsigned char *flags;
    __host__ __device__ bool operator()(const long long &i) const { return flags[i] != 0; }
};

int simplex_select(const double *popt_d, int64_t n_vox, const int8_t *status_d, const int32_t *nfev_d, unsigned char *flags_d,
                   int64_t *idx_d, double *lambda_d, int8_t *face_d, int64_t *n_viol, int *min_nfev, hipStream_t st) {
    *n_viol = 0;
    *min_nfev = 0;
    if (n_vox <= 0) return PNX_OK;
    struct Head {
        long long count;
        unsigned int min_nfev, pad;
    };
    StreamBuf head, tmp;
    if (int rc = head.alloc(sizeof(Head), st)) return rc;
    Head *hd = (Head *)head.p;
    PNX_HIP(hipMemsetAsync(hd, 0xff, sizeof(Head), st));  // min_nfev = UINT_MAX
    size_t blocks = ((size_t)n_vox + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(simplex_classify_kernel, dim3((unsigned)blocks), dim3(256), 0, st, popt_d, popt_d + 2 * (size_t)n_vox, status_d,
                       nfev_d, (long long)n_vox, flags_d, lambda_d, face_d, &hd->min_nfev);
    PNX_HIP(hipGetLastError());
    // hipCUB takes an int count: calls beyond 2^30 voxels are cut into pieces (as pnx_mask_select_f64 does)
    const FlagSet pred{flags_d};
    long long total = 0;
    size_t bytes = 0;
    const int64_t piece = (int64_t)1 << 30;
    Head h{0, 0, 0};
    for (int64_t off = 0; off < n_vox; off += piece) {
        const int m = (int)((n_vox - off) < piece ? (n_vox - off) : piece);
        hipcub::CountingInputIterator<long long> it(off);
        size_t need = 0;
        PNX_HIP(hipcub::DeviceSelect::If(nullptr, need, it, (long long *)idx_d + total, &hd->count, m, pred, st));
        if (!tmp.p || need > bytes) {
            if (tmp.p) (void)hipFreeAsync(tmp.p, st);
            tmp.p = nullptr;
            if (int rc = tmp.alloc(need, st)) return rc;
            bytes = need;
        }
        PNX_HIP(hipcub::DeviceSelect::If(tmp.p, need, it, (long long *)idx_d + total, &hd->count, m, pred, st));
        PNX_HIP(hipMemcpyAsync(&h, hd, sizeof(Head), hipMemcpyDeviceToHost, st));
        PNX_HIP(hipStreamSynchronize(st));
        total += h.count;
    }
    *n_viol = total;
    *min_nfev = total ? (int)h.min_nfev : 0;
    return PNX_OK;
}

// ---- gather ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int row_of(int e, int n_b, float inv) {  // e / n_b for 0 <= e < 64 * 128
    int q = (int)((float)e * inv);
    q -= (q * n_b > e);
    q += ((q + 1) * n_b <= e);
    return q;
}

struct GatherArgs {
    const double *y;     // (n_vox, n_b)
    const double *popt;  // (NT, n_vox) phase-1 result
    const double *lo;    // (NT, n_vox) when per_voxel
    const double *hi;
    const long long *idx;  // (m) ascending
    double *y2;            // (m, n_b)
    double *p0_2, *lo2, *hi2;  // (N2, m)
    long long n_vox, m;
    int n_b;
    int per_voxel;
    double los[kMaxP], his[kMaxP];
};

template <bool S0>
__global__ void __launch_bounds__(kWave) simplex_gather_kernel(const GatherArgs a) {
    extern __shared__ __attribute__((aligned(16))) double tile[];  // [c][n_b], the dense image of the destination
    constexpr int N2 = S0 ? 4 : 3;
    const int lane = threadIdx.x, n_b = a.n_b;
    const long long j0 = (long long)blockIdx.x * kWave;
    const int c = (a.m - j0) < kWave ? (int)(a.m - j0) : kWave;
    const int n_el = c * n_b;
    const float inv = 1.0f / (float)n_b;
    const long long v = a.idx[j0 + (lane < c ? lane : c - 1)];  // lanes past the end repeat the last violator, never stored
    // rows in: consecutive lanes read consecutive elements of a row (a row is n_b contiguous doubles, rows lie anywhere)
    // (every lane takes part in every shuffle: the loop count is the wave's, the last piece is masked at the load)
    for (int e0 = 0; e0 < n_el; e0 += kWave) {
        const int e = e0 + lane, ec = e < n_el ? e : n_el - 1;
        const int r = row_of(ec, n_b, inv);
        const long long vr = __shfl(v, r);  // row r's voxel index lives in lane r
        if (e < n_el) tile[e] = a.y[(size_t)vr * n_b + (e - r * n_b)];
    }
    __syncthreads();
    // tile out: contiguous, 16-byte lines (j0 is a multiple of 64: the tile starts at an even element of the scratch array)
    double *dst = a.y2 + (size_t)j0 * n_b;
    if (((uintptr_t)a.y2 & 15) == 0) {
        for (int e = 2 * lane; e < n_el; e += 2 * kWave) {
            if (e + 1 < n_el) {
                f64x2 o;
                o.x = tile[e];
                o.y = tile[e + 1];
                *reinterpret_cast<f64x2 *>(dst + e) = o;
            } else {
                dst[e] = tile[e];
            }
        }
    } else {
        for (int e = lane; e < n_el; e += kWave) dst[e] = tile[e];
    }
    if (lane >= c) return;
    // the face problem of this lane's violator: [f1, D1, D2 (, S0)] from rows [0, 1, 3 (, 5)] of the tri-exponential layout
    constexpr int src[4] = {0, 1, 3, 5};
    const size_t j = (size_t)(j0 + lane);
    double lo3[6], hi3[6];
#pragma unroll
    for (int k = 0; k < (S0 ? 6 : 5); ++k) {
        lo3[k] = a.per_voxel ? a.lo[(size_t)k * a.n_vox + v] : a.los[k];
        hi3[k] = a.per_voxel ? a.hi[(size_t)k * a.n_vox + v] : a.his[k];
    }
    const double f1 = a.popt[v], f2 = a.popt[2 * (size_t)a.n_vox + v];
    // f2 = 1 - f1 on the face: lo_f2 <= 1 - f1 <= hi_f2.  An empty intersection (lo >= hi) is the fit's own status -1.
    const double l0 = fmax(lo3[0], 1.0 - hi3[2]), h0 = fmin(hi3[0], 1.0 - lo3[2]);
    double s0 = f1 / (f1 + f2);
    if (l0 < h0) s0 = fmin(fmax(s0, l0), h0);  // bounds of f1 or f2 above 0 can leave the projected start outside them
#pragma unroll
    for (int k = 0; k < N2; ++k) {
        a.p0_2[(size_t)k * a.m + j] = k == 0 ? s0 : a.popt[(size_t)src[k] * a.n_vox + v];
        a.lo2[(size_t)k * a.m + j] = k == 0 ? l0 : lo3[src[k]];
        a.hi2[(size_t)k * a.m + j] = k == 0 ? h0 : hi3[src[k]];
    }
}

template <auto kern> static int allow_big_lds_of() {
    PNX_ALLOW_BIG_LDS(kern);
    return PNX_OK;
}

template <bool S0> static int launch_gather(const GatherArgs &a, hipStream_t st) {
    if (int rc = allow_big_lds_of<simplex_gather_kernel<S0>>()) return rc;
    const size_t lds = (size_t)kWave * a.n_b * sizeof(double);  // 64 KB at 128 b-values
    const long long blocks = (a.m + kWave - 1) / kWave;
    hipLaunchKernelGGL((simplex_gather_kernel<S0>), dim3((unsigned)blocks), dim3(kWave), lds, st, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

int simplex_gather(int model, int n_b, const double *y_d, const double *popt_d, int64_t n_vox, const int64_t *idx_d, int64_t m,
                   int per_voxel, const double *lo, const double *hi, double *y2_d, double *p0_2_d, double *lo2_d, double *hi2_d,
                   hipStream_t st) {
    if (m <= 0) return PNX_OK;
    if (model != PNX_MODEL_TRI_REDUCED && model != PNX_MODEL_TRI_S0) return set_error(PNX_ERR_INVALID, "simplex gather: model %d", model);
    if (n_b < 1 || n_b > kMaxB) return set_error(PNX_ERR_INVALID, "simplex gather: n_b=%d", n_b);
    GatherArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.popt = popt_d;
    a.idx = (const long long *)idx_d;
    a.y2 = y2_d;
    a.p0_2 = p0_2_d;
    a.lo2 = lo2_d;
    a.hi2 = hi2_d;
    a.n_vox = n_vox;
    a.m = m;
    a.n_b = n_b;
    a.per_voxel = per_voxel;
    if (per_voxel) {
        a.lo = lo;
        a.hi = hi;
    } else {
        for (int k = 0; k < (model == PNX_MODEL_TRI_S0 ? 6 : 5); ++k) {
            a.los[k] = lo[k];
            a.his[k] = hi[k];
        }
    }
    return model == PNX_MODEL_TRI_S0 ? launch_gather<true>(a, st) : launch_gather<false>(a, st);
}

// ---- merge and certify ----------------------------------------------------------------------------------------------------
struct MergeArgs {
    const long long *idx;  // (m)
    const double *y2;      // (m, n_b)
    const double *popt2;   // (N2, m)
    const int8_t *status2;
    const int32_t *nfev2;
    const double *cost2;
    const double *p0;  // (NT, n_vox) when per_voxel
    double *popt;      // (NT, n_vox)
    double *pcov;      // (n_vox, NT, NT) or null
    int8_t *status;
    int32_t *nfev;
    double *cost;
    double *lambda;  // or null
    int8_t *face;    // or null
    long long n_vox, m;
    int n_b;
    int per_voxel;
    double p0s[kMaxP];
    double b[kMaxB];
};

template <int MODEL>
__global__ void __launch_bounds__(kWave) simplex_merge_kernel(const MergeArgs a) {
    using M = Model<MODEL>;
    constexpr int NT = M::NALL, NC = M::NC;
    constexpr bool S0 = MODEL == PNX_MODEL_TRI_S0;
    static_assert(MODEL == PNX_MODEL_TRI_REDUCED || MODEL == PNX_MODEL_TRI_S0, "the constraint is defined for the reduced tri-exponential layouts");
    extern __shared__ __attribute__((aligned(16))) double tile[];  // [64][S]: the odd row stride spreads the lanes' reads over the banks
    const int lane = threadIdx.x, n_b = a.n_b, S = n_b | 1;
    const long long j0 = (long long)blockIdx.x * kWave;
    const int c = (a.m - j0) < kWave ? (int)(a.m - j0) : kWave;
    const int n_el = c * n_b;
    const float inv = 1.0f / (float)n_b;
    const double *src = a.y2 + (size_t)j0 * n_b;
    for (int e = lane; e < n_el; e += kWave) {  // the block's rows are one contiguous piece of the gathered signal
        const int r = row_of(e, n_b, inv);
        tile[r * S + (e - r * n_b)] = src[e];
    }
    __syncthreads();
    if (lane >= c) return;
    const size_t j = (size_t)(j0 + lane);
    const size_t v = (size_t)a.idx[j];
    const size_t nv = (size_t)a.n_vox;
    const int st2 = a.status2[j];
    a.status[v] = (int8_t)st2;
    a.nfev[v] += a.nfev2[j];  // both phases
    if (a.pcov) {  // J^T J is singular on the face (D3 has no column): the reference's covariance estimate is NaN there
        double *pc = a.pcov + v * NT * NT;
        for (int t = 0; t < NT * NT; ++t) pc[t] = NAN;
    }
    if (st2 <= 0) {  // the usual sentinel: popt = p0, NaN covariance, phase 2's status and cost
#pragma unroll
        for (int k = 0; k < NT; ++k) a.popt[(size_t)k * nv + v] = a.per_voxel ? a.p0[(size_t)k * nv + v] : a.p0s[k];
        if (a.cost) a.cost[v] = a.cost2[j];
        if (a.lambda) a.lambda[v] = NAN;
        if (a.face) a.face[v] = 2;  // a face voxel without a certificate
        return;
    }
    double p[NT];
    p[0] = a.popt2[j];
    p[1] = a.popt2[a.m + j];
    p[2] = 1.0 - p[0];
    p[3] = a.popt2[2 * a.m + j];
    p[4] = a.popt[4 * nv + v];  // D3 is unidentifiable on the face: kept as phase 1 found it, inside its bounds
    if (S0) p[NT - 1] = a.popt2[3 * a.m + j];
    a.popt[v] = p[0];
    a.popt[nv + v] = p[1];
    a.popt[2 * nv + v] = p[2];
    a.popt[3 * nv + v] = p[3];
    if (S0) a.popt[5 * nv + v] = p[NT - 1];
    // one row pass of the FULL model at the face point: cost and the gradient entries of f1 and f2
    const double *mine = tile + lane * S;
    double ss = 0.0, g1 = 0.0, g2 = 0.0;
    for (int i = 0; i < n_b; ++i) {
        const double x = a.b[i];
        double E[NC], J[NT];
#pragma unroll
        for (int k = 0; k < NC; ++k) E[k] = exp_fast(-x * p[M::dpos(k)]);
        const double r = M::signal(p, E) - mine[i];
        M::jac(p, E, x, J);
        ss = fma(r, r, ss);
        g1 = fma(J[0], r, g1);
        g2 = fma(J[2], r, g2);
    }
    // stationarity of 0.5 ||r||^2 + lambda (f1 + f2 - 1): g_f1 = g_f2 = -lambda
    const double lam = -0.5 * (g1 + g2);
    if (a.cost) a.cost[v] = 0.5 * ss;
    if (a.lambda) a.lambda[v] = lam;
    if (a.face) a.face[v] = lam >= 0.0 ? 1 : 2;  // 2: the box-only minimum was infeasible, yet the face point wants to move inwards
}

template <int MODEL> static int launch_merge(const MergeArgs &a, hipStream_t st) {
    if (int rc = allow_big_lds_of<simplex_merge_kernel<MODEL>>()) return rc;
    const size_t lds = (size_t)kWave * (a.n_b | 1) * sizeof(double);  // 66 KB at 128 b-values
    const long long blocks = (a.m + kWave - 1) / kWave;
    hipLaunchKernelGGL((simplex_merge_kernel<MODEL>), dim3((unsigned)blocks), dim3(kWave), lds, st, a);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

int simplex_merge(int model, int n_b, const double *b_host, int64_t m, const int64_t *idx_d, const double *y2_d,
                  const double *popt2_d, const int8_t *status2_d, const int32_t *nfev2_d, const double *cost2_d, int per_voxel,
                  const double *p0, int64_t n_vox, double *popt_d, double *pcov_d, int8_t *status_d, int32_t *nfev_d, double *cost_d,
                  double *lambda_d, int8_t *face_d, hipStream_t st) {
    if (m <= 0) return PNX_OK;
    if (model != PNX_MODEL_TRI_REDUCED && model != PNX_MODEL_TRI_S0) return set_error(PNX_ERR_INVALID, "simplex merge: model %d", model);
    if (n_b < 1 || n_b > kMaxB) return set_error(PNX_ERR_INVALID, "simplex merge: n_b=%d", n_b);
    if (!status_d || !nfev_d) return set_error(PNX_ERR_INVALID, "simplex merge: status and nfev are required");
    MergeArgs a;
    memset(&a, 0, sizeof(a));
    a.idx = (const long long *)idx_d;
    a.y2 = y2_d;
    a.popt2 = popt2_d;
    a.status2 = status2_d;
    a.nfev2 = nfev2_d;
    a.cost2 = cost2_d;
    a.popt = popt_d;
    a.pcov = pcov_d;
    a.status = status_d;
    a.nfev = nfev_d;
    a.cost = cost_d;
    a.lambda = lambda_d;
    a.face = face_d;
    a.n_vox = n_vox;
    a.m = m;
    a.n_b = n_b;
    a.per_voxel = per_voxel;
    if (per_voxel)
        a.p0 = p0;
    else
        for (int k = 0; k < (model == PNX_MODEL_TRI_S0 ? 6 : 5); ++k) a.p0s[k] = p0[k];
    for (int i = 0; i < n_b; ++i) a.b[i] = b_host[i];
    return model == PNX_MODEL_TRI_S0 ? launch_merge<PNX_MODEL_TRI_S0>(a, st) : launch_merge<PNX_MODEL_TRI_REDUCED>(a, st);
}

}  // namespace pnx
