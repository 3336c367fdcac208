// pnx_curvefit_f32_kernel.hpp -- batched bounded NLLS (Trust-Region-Reflective) for gfx950 with fp32 ARITHMETIC.
//
// The design of pnx_curvefit_kernel.hpp (one lane per voxel, persistent lanes on a work queue with asynchronous refill, one
// fused row pass per trial point, QR + one-sided Jacobi instead of an SVD of the augmented matrix, the order of operations of
// scipy/optimize/_lsq/trf.py per iteration, the same statuses and failure sentinels) with every quantity of the iteration a
// float: v_exp_f32 instead of a software fp64 exp, half the registers per lane, two waves per SIMD.  The covariance epilogue
// alone computes in fp64 (one n x n SVD per voxel, all lanes busy, off the critical path).
//
// What fp32 cannot do and this kernel therefore does not offer: SciPy's 2-point finite differences (a step of 1.5e-8 is below
// fp32 resolution: analytic Jacobian only) and termination tolerances below fp32 resolution (the caller's ftol / xtol / gtol are
// raised to the floors of include/pnx.h on the host).  Results are float32-quality minima, not SciPy's iterates.
// Scope: all parameters free, no T1 / STEAM factor, no sigma, no queue order (pnx_curvefit_fast_f32 refuses the rest).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_curvefit_kernel.hpp"  // Model<>, colperm<>, kWave / kMaxB / kMaxP, LaneState, Park<>, BoolC, lds_void, ColPerm
#include "pnx_model_t.hpp"
#include "pnx_trf_math.hpp"  // the TRF algebra with T = float: qr_merge, jacobi_svd, solve_lsq_trust_region, select_step, ...

namespace pnx {
namespace f32 {

constexpr float kEpsF = TrfTraits<float>::eps;  // FLT_EPSILON
// rows merged into the QR factor per Householder block step (RB x (N + 1) floats of registers)
template <int N> constexpr int row_blk() { return N >= 6 ? 4 : 8; }

struct CurvefitF32Args {
    const float *y;   // (n_vox, n_b)
    const float *p0;  // (N, n_vox) when per_voxel
    const float *lo;
    const float *hi;
    float *popt;      // (N, n_vox)
    float *pcov;      // (n_vox, N, N) or null
    int8_t *status;
    int32_t *nfev;
    float *cost;
    unsigned long long *queue;  // work-queue head, zeroed before launch
    long long n_vox;
    int n_b;
    int per_voxel;
    int max_nfev;
    float ftol, xtol, gtol;  // already raised to the fp32 floors
    float p0s[kMaxP], los[kMaxP], his[kMaxP];
    float b[kMaxB];
};

// ---------------------------------------------------------------------------------------------
// The kernel.  Block = up to 4 wavefronts; LDS: b-values + per wave the signal tile y[row][lane] (floats: one conflict-free
// ds_read_b32 per row), the packed R factor of the current iterate and (N <= 5) the right singular vectors: Park<N> with a
// tile of n_b rows, counted in floats.
// ---------------------------------------------------------------------------------------------

// Loop order as curvefit_kernel: refill, row pass at x_new, D (accept / reject, radius, ftol / xtol), B-light (Coleman-Li
// scaling, gtol), outputs of finished voxels + refill, B-heavy (augmented QR + Jacobi SVD), C (trust-region step).
template <int MODEL, bool PV>
__global__ void __launch_bounds__(64 * 4, 2) curvefit_f32_kernel(const CurvefitF32Args A) {
    using MT = ModelT<MODEL, float>;
    using PK = Park<MT::NALL>;
    constexpr int N = MT::NALL;
    auto CP = [](int k) constexpr { return colperm<MODEL>(k); };  // factor column k = parameter CP(k)

    extern __shared__ float smem_f[];
    const int n_b = A.n_b;
    float *bsh = smem_f;  // [kMaxB]
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    float *ytile = smem_f + kMaxB + (size_t)wave * PK::per_wave(n_b);  // [n_b][64], wave-uniform base
    float *ysh = ytile + lane;                                         // this lane's column
    float *rpark = ytile + (size_t)n_b * kWave + lane;                 // [NR][64]
    float *vpark = rpark + (size_t)PK::NR * kWave;                     // [NV][64]
    for (int i = threadIdx.x; i < n_b; i += blockDim.x) bsh[i] = A.b[i];
    __syncthreads();
    // the refill uses asynchronous 4-byte global->LDS loads, one per b-value: every load reads exactly one element of the
    // voxel's row, so nothing beyond the caller's buffer is touched whatever n_b is
    const bool dma_ok = ((reinterpret_cast<uintptr_t>(A.y) & 3) == 0);

    int state = ST_IDLE;
    long long vox = -1;
    float x[N], lb[N], ub[N];
    float g[N];
    float s[N], uf[N], R2[N][N], d[N], g_h[N];
    float Vreg[PK::kParkV ? 1 : N][PK::kParkV ? 1 : N];
    float smax = 0, smin = 0, theta = 0;
    float cost = 0, Delta = 0, alpha = 0;
    int nfev = 0, term = -99;
    bool first = false;
    float xn[N], step_h_norm = 0, step_norm = 0, predicted = 0;
    if (!PV) {
#pragma unroll
        for (int k = 0; k < N; ++k) {  // wave-uniform, never written again: stays in SGPRs
            lb[k] = A.los[k];
            ub[k] = A.his[k];
        }
    }

    auto refill = [&]() {
        while (state == ST_IDLE) {
            const unsigned long long idx = atomicAdd(A.queue, 1ULL);
            if (idx >= (unsigned long long)A.n_vox) break;  // queue empty: this lane is done for good
            vox = (long long)idx;
            const float *yv = A.y + (size_t)vox * n_b;
            if (dma_ok) {
                for (int i = 0; i < n_b; ++i)
                    __builtin_amdgcn_global_load_lds((const void *)(yv + i), (lds_void *)(ytile + i * kWave), 4, 0, 0);
            } else {
                for (int i = 0; i < n_b; ++i) ysh[i * kWave] = yv[i];
            }
            bool okb = true, okp = true;
            float p0v[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                if (PV) {
                    p0v[k] = A.p0[(size_t)k * A.n_vox + vox];
                    lb[k] = A.lo[(size_t)k * A.n_vox + vox];
                    ub[k] = A.hi[(size_t)k * A.n_vox + vox];
                } else
                    p0v[k] = A.p0s[k];
                okb = okb && (lb[k] < ub[k]);                          // least_squares.py:814-816
                okp = okp && (p0v[k] >= lb[k]) && (p0v[k] <= ub[k]);  // least_squares.py:818-819
            }
            if (!okb || !okp) {
                // reference: ValueError inside curve_fit -> params = p0, cov = NaN, success = False
                const int st = !okb ? -1 : -3;
#pragma unroll
                for (int k = 0; k < N; ++k) A.popt[(size_t)k * A.n_vox + vox] = p0v[k];
                if (A.status) A.status[vox] = (int8_t)st;  // pcov_f32_kernel writes the NaN covariance
                if (A.nfev) A.nfev[vox] = 0;
                if (A.cost) A.cost[vox] = NAN;
                continue;  // stays IDLE -> next voxel
            }
#pragma unroll
            for (int k = 0; k < N; ++k) xn[k] = strictly_feasible0(strictly_feasible_r(p0v[k], lb[k], ub[k]), lb[k], ub[k]);
            state = ST_INIT;
            nfev = 0;
            term = -99;
            alpha = 0.0f;
        }
    };
    refill();
    for (;;) {
        if (state == ST_IDLE) break;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // LDS-DMA signal tiles have landed

        // ------------------------------------------------------------------ row pass at xn
        // residual f = model(xn) - y, cost, analytic Jacobian, g = J^T f, QR of J -- fp32 throughout
        float Rn[N][N], qn[N], gn[N], cost_new = 0, ymax = 0;
        bool yfinite = true;
        {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                qn[i] = 0;
                gn[i] = 0;
#pragma unroll
                for (int j = 0; j < N; ++j) Rn[i][j] = 0;
            }
            constexpr int kRowBlk = row_blk<N>();
            // One block of kRowBlk rows, then the Householder merge.  TAIL: the last, partial block -- rows beyond n_b are
            // evaluated at row 0 and replaced by zeros.
            auto row_block = [&](auto tail_c, const int i0) __attribute__((always_inline)) {
                constexpr bool TAIL = decltype(tail_c)::value;
                float blk[kRowBlk][N + 1];
                float csum = 0;
#pragma unroll
                for (int r = 0; r < kRowBlk; ++r) {
                    const bool live = !TAIL || (i0 + r < n_b);
                    const int ii = live ? i0 + r : 0;
                    const float bb = bsh[ii];
                    const float yi = ysh[ii * kWave];
                    yfinite = yfinite && (fabsf(yi) < INFINITY);
                    ymax = fmaxf(ymax, fabsf(yi));
                    float sig, ja[N];
                    MT::eval(xn, bb, sig, ja);
                    const float rr = live ? sig - yi : 0.0f;
                    csum = fmaf(rr, rr, csum);
#pragma unroll
                    for (int k = 0; k < N; ++k) gn[k] = fmaf(live ? ja[k] : 0.0f, rr, gn[k]);
#pragma unroll
                    for (int k = 0; k < N; ++k) blk[r][k] = live ? ja[CP(k)] : 0.0f;
                    blk[r][N] = rr;
                }
                cost_new += csum;  // block sums first: shorter accumulation chains, smaller rounding error of the cost
                qr_merge<N, kRowBlk>(Rn, qn, blk);
            };
            int i0 = 0;
            for (; i0 + kRowBlk <= n_b; i0 += kRowBlk) row_block(BoolC<false>{}, i0);
            if (i0 < n_b) row_block(BoolC<true>{}, i0);
            cost_new *= 0.5f;
        }
        const bool finite_f = fabsf(cost_new) < INFINITY;  // a non-finite residual makes the sum of squares non-finite

        // ------------------------------------------------------------------ phase D: accept / reject
        bool accepted = false;
        int final_status = 0;
        if (state == ST_INIT) {
            if (!finite_f) {
                final_status = yfinite ? -4 : -2;
                cost = NAN;
                nfev = 0;
                state = ST_FINAL;
            } else {
                accepted = true;
                nfev = 1;
                first = true;
                state = ST_RUN;
            }
        } else {  // ST_RUN
            nfev += 1;
            if (!finite_f) {
                Delta = 0.25f * step_h_norm;  // trf.py:337-339
            } else {
                const float actual = cost - cost_new;
                float ratio;  // update_tr_radius (common.py:222-245)
                if (predicted > 0)
                    ratio = actual / predicted;
                else if (predicted == 0 && actual == 0)
                    ratio = 1;
                else
                    ratio = 0;
                float Delta_new = Delta;
                if (ratio < 0.25f)
                    Delta_new = 0.25f * step_h_norm;
                else if (ratio > 0.75f && step_h_norm > 0.95f * Delta)
                    Delta_new = Delta * 2.0f;
                // check_termination (common.py:705-717) at fp32 resolution.  SciPy's ftol test, then the stop it has no need for
                // in fp64: a step that neither the model (predicted) nor the evaluation (|actual|) can tell from zero ends the
                // fit as an ftol stop instead of shrinking the radius until xtol trips.  "Zero" is ftol * cost plus a quarter of
                // the cost of fp32 rounding of the model itself, 0.5 n_b (FLT_EPSILON max|y|)^2: a noise-free voxel ends AT that
                // level, where ftol * cost resolves nothing.
                const float eym = kEpsF * ymax;
                const float res_rel = A.ftol * cost;
                const float res_abs = res_rel + 0.125f * (float)n_b * eym * eym;
                const bool ftol_ok = ((actual < res_rel) && (ratio > 0.25f)) || ((fabsf(actual) < res_abs) && (predicted < res_abs));
                const bool xtol_ok = step_norm < A.xtol * (A.xtol + normn<N>(x));
                if (ftol_ok && xtol_ok)
                    term = 4;
                else if (ftol_ok)
                    term = 2;
                else if (xtol_ok)
                    term = 3;
                if (term == -99) {
                    alpha *= Delta / Delta_new;
                    Delta = Delta_new;
                }
                accepted = actual > 0;
            }
        }
        if (accepted) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                x[i] = xn[i];
                g[i] = gn[i];
            }
            cost = cost_new;
            int t = 0;
#pragma unroll
            for (int i = 0; i < N; ++i)
#pragma unroll
                for (int j = i; j < N; ++j) rpark[(t++) * kWave] = Rn[i][j];
        }

        // ------------------------------------------------------------------ light head of phase B (trf.py:260-272)
        float v[N], dv[N], g_norm = 0;
        if (state == ST_RUN && (accepted || term != -99 || nfev >= A.max_nfev)) {
#pragma unroll
            for (int i = 0; i < N; ++i) {  // CL_scaling_vector (common.py:467-508)
                v[i] = 1.0f;
                dv[i] = 0.0f;
                if (g[i] < 0 && isfinite(ub[i])) {
                    v[i] = ub[i] - x[i];
                    dv[i] = -1;
                }
                if (g[i] > 0 && isfinite(lb[i])) {
                    v[i] = x[i] - lb[i];
                    dv[i] = 1;
                }
                g_norm = fmaxf(g_norm, fabsf(g[i] * v[i]));
            }
            if (first) {  // trf.py:232-236
                float t = 0;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const float q = x[i] / sqrtf(v[i]);
                    t += q * q;
                }
                Delta = sqrtf(t);
                if (Delta == 0) Delta = 1.0f;
                first = false;
            }
            if (g_norm < A.gtol) term = 1;
            if (term != -99 || nfev >= A.max_nfev) {
                final_status = (term == -99) ? 0 : term;
                state = ST_FINAL;
            }
        }

        // ------------------------------------------------------------------ outputs of finished voxels
        if (state == ST_FINAL) {
            const bool ok = final_status > 0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                // failure: the reference returns the p0 it was given (curvefit.py:308-317)
                const float pk = ok ? x[k] : (PV ? A.p0[(size_t)k * A.n_vox + vox] : A.p0s[k]);
                A.popt[(size_t)k * A.n_vox + vox] = pk;
            }
            if (A.status) A.status[vox] = (int8_t)final_status;
            if (A.nfev) A.nfev[vox] = nfev;
            if (A.cost) A.cost[vox] = cost;
            if (A.pcov && ok) {
                // the packed R factor of the final Jacobian goes to the voxel's pcov slot; pcov_f32_kernel turns it into pcov
                float *pc = A.pcov + (size_t)vox * N * N;
#pragma unroll
                for (int t = 0; t < PK::NR; ++t) pc[t] = rpark[t * kWave];
            }
            state = ST_IDLE;
        }
        if (state == ST_IDLE) refill();  // claim the next voxel now: its signal streams in behind phases B / C

        if (state == ST_RUN) {
            // -------------------------------------------------------------- heavy phase B (iterate changed)
            if (accepted) {
                float diag_h[N];
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    d[i] = sqrtf(v[i]);
                    diag_h[i] = g[i] * dv[i];
                    g_h[i] = d[i] * g[i];
                }
                // QR of [R*D; diag(sqrt(diag_h))] -> R2, q2 ;  J_aug = Q R2 (trf.py:300-306)
                float q2[N];
                float blk[N][N + 1];
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    q2[i] = qn[i];
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        R2[i][j] = (j >= i) ? Rn[i][j] * d[CP(j)] : 0.0f;
                        blk[i][j] = (i == j) ? sqrtf(diag_h[CP(i)]) : 0.0f;
                    }
                    blk[i][N] = 0.0f;
                }
                qr_merge<N, N>(R2, q2, blk);
                // SVD of R2 through one-sided Jacobi on W = R2^T (lower triangular):  W Vw = Uw S  =>  R2 = Vw S Uw^T
                float W[N][N], Vw[N][N];
#pragma unroll
                for (int i = 0; i < N; ++i)
#pragma unroll
                    for (int j = 0; j < N; ++j) W[i][j] = (i >= j) ? R2[j][i] : 0.0f;
                jacobi_svd<N>(W, Vw);
                smax = 0;
                smin = INFINITY;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    float nn = 0, dq = 0;
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        nn += W[i][k] * W[i][k];
                        dq += Vw[i][k] * q2[i];
                    }
                    float inv = 0.0f;
                    if (nn > 0) nn = fast_sqrt_rsqrt(nn, &inv);
                    s[k] = nn;
                    uf[k] = dq;
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        if (PK::kParkV)
                            vpark[(i * N + k) * kWave] = W[i][k] * inv;
                        else
                            Vreg[PK::kParkV ? 0 : i][PK::kParkV ? 0 : k] = W[i][k] * inv;
                    }
                    smax = fmaxf(smax, nn);
                    smin = fminf(smin, nn);
                }
                theta = fmaxf(0.995f, 1 - g_norm);
            }
            // -------------------------------------------------------------- phase C: trial step
            float V[N][N];
#pragma unroll
            for (int i = 0; i < N; ++i)
#pragma unroll
                for (int k = 0; k < N; ++k)
                    V[i][k] = PK::kParkV ? vpark[(i * N + k) * kWave] : Vreg[PK::kParkV ? 0 : i][PK::kParkV ? 0 : k];
            // everything below works in the factor's column order (a relabelling of the parameters)
            float xP[N], lbP[N], ubP[N], dP[N], ghP[N];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                xP[i] = x[CP(i)];
                lbP[i] = lb[CP(i)];
                ubP[i] = ub[CP(i)];
                dP[i] = d[CP(i)];
                ghP[i] = g_h[CP(i)];
            }
            float p_h[N], p[N], step[N], step_h[N];
            alpha = solve_lsq_trust_region<N>(n_b, uf, s, V, smax, smin, Delta, alpha, p_h);
#pragma unroll
            for (int i = 0; i < N; ++i) p[i] = dP[i] * p_h[i];
            predicted = select_step<N>(xP, R2, ghP, p, p_h, dP, Delta, lbP, ubP, theta, step, step_h);
#pragma unroll
            for (int i = 0; i < N; ++i) xn[CP(i)] = strictly_feasible0(xP[i] + step[i], lbP[i], ubP[i]);
            step_h_norm = normn<N>(step_h);
            step_norm = normn<N>(step);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Covariance epilogue (one lane per voxel): the packed fp32 R factor that curvefit_f32_kernel parked in pcov[vox] ->
//   pinv(J^T J) * 2 cost / (m - n)  (scipy/optimize/_minpack_py.py:1036-1066), NaN for failed voxels.
// Computed in fp64 (jacobi_svd<N, double> of pnx_trf_math.hpp) and stored as float.  Singular values are dropped below
// FLT_EPSILON * max(m, n) * s_max -- the factor is an fp32 one -- where SciPy uses the fp64 epsilon.
// ---------------------------------------------------------------------------------------------
template <int N>
__global__ void __launch_bounds__(256) pcov_f32_kernel(float *pcov, const int8_t *status, const float *cost, long long n_vox,
                                                       int n_b, const ColPerm cp) {
    const long long vox = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (vox >= n_vox) return;
    float *pc = pcov + (size_t)vox * N * N;
    if (status[vox] <= 0) {
#pragma unroll
        for (int k = 0; k < N * N; ++k) pc[k] = NAN;
        return;
    }
    double W[N][N], Vw[N][N];
    {
        int t = 0;
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N; ++j) W[i][j] = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = i; j < N; ++j) W[j][i] = (double)pc[t++];  // W = R^T
    }
    jacobi_svd<N>(W, Vw);
    double s2[N], sm = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double nn = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) nn += W[i][k] * W[i][k];
        s2[k] = nn;
        sm = fmax(sm, nn);
    }
    const double thr = (double)kEpsF * (n_b > N ? n_b : N) * sqrt(sm);
    const bool dof = n_b > N;
    const double s_sq = dof ? 2.0 * (double)cost[vox] / (double)(n_b - N) : 0.0;
    double wgt[N];
#pragma unroll
    for (int k = 0; k < N; ++k) wgt[k] = (sqrt(s2[k]) > thr) ? 1.0 / (s2[k] * s2[k]) : 0.0;  // V_k V_k^T / s_k^2 = w_k w_k^T / s_k^4
    bool bad = false;
    double out[N][N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double a = 0;
#pragma unroll
            for (int k = 0; k < N; ++k) a += W[i][k] * W[j][k] * wgt[k];
            out[i][j] = a;
            bad = bad || isnan(a);
        }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) pc[cp.p[i] * N + cp.p[j]] = (bad || !dof) ? INFINITY : (float)(out[i][j] * s_sq);  // factor order -> parameter order
}

}  // namespace f32
}  // namespace pnx
