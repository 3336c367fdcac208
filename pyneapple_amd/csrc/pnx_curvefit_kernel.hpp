// pnx_curvefit_kernel.hpp -- batched bounded NLLS (Trust-Region-Reflective) for gfx950, fp64.
//
// Hot path replaced: CurveFitSolver._fit_single_pixel (reference src/pyneapple/solvers/curvefit.py:246-317)
// -> scipy curve_fit(method="trf") -> least_squares -> trf_bounds (scipy/optimize/_lsq/trf.py:205-394),
// for every voxel of a volume at once.
//
// Mapping to the machine (see DESIGN.md for the measurements behind these choices):
//   * ONE LANE OWNS ONE VOXEL.  All of TRF's per-voxel algebra (n x n SVD, More' root find, reflective
//     step selection) is scalar work per problem; giving a voxel a whole wavefront would run that part
//     at 1/64 efficiency.  The wavefront is the unit that shares the b-value table (LDS), the signal
//     tile (LDS, [row][lane] so every ds_read_b64 is conflict-free) and the work queue.
//   * PERSISTENT LANES + WORK QUEUE.  Voxels need 5..60 function evaluations; a lane that finishes pulls the
//     next voxel from a global atomic counter instead of idling until the slowest voxel of its wave is done.
//     Every lane leaves the loop as soon as the queue is empty, so the grid always drains.
//   * ONE FUSED "ROW PASS" per trial point: residual, cost, Jacobian row (2-point FD exactly as
//     scipy/_numdiff.py:584-625, or analytic), J^T f and a Householder QR of J accumulated row_blk<N>() rows at a time.
//     The Jacobian never exists in memory; TRF's SVD of the (m+n) x n augmented matrix is taken from the
//     n x n triangular factor (QR then one-sided Jacobi), which is as accurate as LAPACK's SVD of J_aug.
//   * The Jacobian at the trial point is computed speculatively together with f(x_new): an accepted step
//     (the common case) then needs no second pass.
//   * ASYNCHRONOUS REFILL: a lane that has written its results claims the next voxel and issues global->LDS DMA loads
//     (global_load_lds) of its signal row; they land while the other lanes run the heavy phases and are collected by
//     one s_waitcnt vmcnt(0) in front of the next row pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_trf_math.hpp"  // the TRF algebra shared with the fp32 kernel: qr_merge, jacobi_svd, solve_lsq_trust_region, select_step, ...

namespace pnx {

constexpr int kWave = 64;
constexpr int kMaxB = 128;
constexpr int kMaxP = 8;
// rows merged into the QR factor per Householder block step: the block is RB x (N + 1) doubles of registers.  Measured
// (1 Mi voxels, profiles/model_probe.py): N = 3: 321 (RB 8) vs 288 (RB 4) M voxels/s; N = 5: 72.6 vs 75.8; N = 6: 46-49 vs 58
// (RB 8 spills ~500 B per lane there, RB 4 none).  PNX_ROW_BLK overrides for experiments.
#ifdef PNX_ROW_BLK
template <int N> constexpr int row_blk() { return PNX_ROW_BLK; }
#else
template <int N> constexpr int row_blk() { return N >= 7 ? 2 : (N >= 5 ? 4 : 8); }  // N = 7: 450 -> 200 B of spills with 2
#endif
constexpr double kEps = TrfTraits<double>::eps;
constexpr double kSqrtEps = 1.4901161193847656e-08;
template <bool B> struct BoolC {  // compile-time flag handed to a generic lambda
    static constexpr bool value = B;
};
typedef __attribute__((address_space(3))) void lds_void;

// Control block of a streamed launch.  `ready` is written by 8-byte H2D copies enqueued behind each granule's upload (stream
// order = data before watermark); `done[g]` counts the waves that will never touch granule g again.
struct StreamCtl {
    unsigned long long ready;  // voxels [0, ready) are resident
    unsigned int abort;        // (unused since round 4: the abort word is host_flags[n_granules], see CurvefitArgs)
    unsigned int timed_out;    // kernel -> host: a lane gave up waiting for the watermark
    unsigned int done[1];      // [n_granules]
};

struct CurvefitArgs {
    const double *y;      // (n_vox, n_b)
    const double *p0;     // (N, n_vox) when per_voxel
    const double *lo;
    const double *hi;
    const double *fixed;  // (n_fixed, n_vox) when fixed_per_voxel
    double *popt;         // (N, n_vox)
    double *pcov;         // (n_vox, N, N) or null
    int8_t *status;
    int32_t *nfev;
    double *cost;
    unsigned long long *queue;  // work-queue head, zeroed before launch
    const int32_t *order;       // null, or (n_vox) a permutation: the queue's k-th pull fits voxel order[k] (longest fits first, see
                                // pnx_curvefit_opts::queue_order); never with a streamed launch (granules complete in index order)
    // Streamed launch (host-pointer calls, pnx_api.hip `curvefit_streamed`): ONE persistent kernel runs while the volume is
    // still being uploaded and its results are already being downloaded.  ctl != null selects the STREAM instantiation.
    StreamCtl *ctl;             // device memory: upload watermark, abort word, per-granule wave counts
    unsigned int *host_flags;   // pinned host memory: host_flags[g] = 1 once every wave has left granule g behind; host_flags[n_granules]
                                // is the ABORT word (host -> kernel: stop waiting for the watermark and leave).  It lives in host
                                // memory so that the host can raise it with a plain store -- a copy into device memory would queue up
                                // behind whatever stalls the upload stream, which is exactly when it is needed
    int granule_shift;          // granule = 1 << granule_shift voxels
    unsigned int stream_spins;  // watermark polls before a lane gives up (ctl->timed_out = 1)
    int phase;                  // 0: fit + covariance epilogue, 1: fit only, 2: covariance epilogue only
    int team;                   // 1: a drained wave evaluates its last voxel's rows across its lanes (team mode, see the kernel); 0 only
                                // through the test hook PNX_CF_TEAM=0, so that one library gives both sides of a bit-for-bit comparison
    long long n_vox;
    int n_b;
    int per_voxel;
    int fixed_per_voxel;
    int max_nfev;
    int n_fixed;
    int t1_mode;          // 0 none, 1 T1: S*(1-exp(-TR/T1)), 2 STEAM: additionally *exp(-TM/T1) (multiexp.py:210-241)
    double tr, tm;
    double ftol, xtol, gtol;
    double p0s[kMaxP], los[kMaxP], his[kMaxP], fixeds[kMaxP];
    int free_idx[kMaxP];
    int fixed_idx[kMaxP];
    int use_sigma;       // curve_fit(sigma = 1-D): residual and Jacobian rows are scaled by w[i] = 1 / sigma_i (scipy:_minpack_py.py:958-960, 545-562)
    int absolute_sigma;  // curve_fit(absolute_sigma = True): the covariance is not scaled by 2 cost / (n_b - n_free) (:1057-1063)
    double b[kMaxB];
    double w[kMaxB];     // 1 / sigma per measurement (use_sigma only)
};

// ---------------------------------------------------------------------------------------------
// Forward models.  Parameter order and operation order follow model_functions/multiexp.py:35-202;
// analytic Jacobian columns follow models/{monoexp.py:143-148, biexp.py:172-204, triexp.py:190-230}.
// E[c] = exp(-b * D_c).
// ---------------------------------------------------------------------------------------------
template <int MODEL> struct Model;

template <> struct Model<0> {  // mono [S0, D]
    static constexpr int NALL = 2, NC = 1;
    __device__ static constexpr int dpos(int c) { return 1; }
    __device__ static double signal(const double *p, const double *E) { return p[0] * E[0]; }
    __device__ static void jac(const double *p, const double *E, double x, double *r) {
        r[0] = E[0];
        r[1] = -x * p[0] * E[0];
    }
};
template <> struct Model<1> {  // bi reduced [f1, D1, D2]
    static constexpr int NALL = 3, NC = 2;
    __device__ static constexpr int dpos(int c) { return c == 0 ? 1 : 2; }
    __device__ static double signal(const double *p, const double *E) { return p[0] * E[0] + (1 - p[0]) * E[1]; }
    __device__ static void jac(const double *p, const double *E, double x, double *r) {
        r[0] = E[0] - E[1];
        r[1] = -x * p[0] * E[0];
        r[2] = -x * (1 - p[0]) * E[1];
    }
};
template <> struct Model<2> {  // bi S0 [f1, D1, D2, S0]
    static constexpr int NALL = 4, NC = 2;
    __device__ static constexpr int dpos(int c) { return c == 0 ? 1 : 2; }
    __device__ static double signal(const double *p, const double *E) {
        return p[3] * (p[0] * E[0] + (1 - p[0]) * E[1]);
    }
    __device__ static void jac(const double *p, const double *E, double x, double *r) {
        r[0] = p[3] * (E[0] - E[1]);
        r[1] = -x * p[3] * p[0] * E[0];
        r[2] = -x * p[3] * (1 - p[0]) * E[1];
        r[3] = p[0] * E[0] + (1 - p[0]) * E[1];
    }
};
template <> struct Model<3> {  // bi full [f1, D1, f2, D2]
    static constexpr int NALL = 4, NC = 2;
    __device__ static constexpr int dpos(int c) { return c == 0 ? 1 : 3; }
    __device__ static double signal(const double *p, const double *E) { return p[0] * E[0] + p[2] * E[1]; }
    __device__ static void jac(const double *p, const double *E, double x, double *r) {
        r[0] = E[0];
        r[1] = -x * p[0] * E[0];
        r[2] = E[1];
        r[3] = -x * p[2] * E[1];
    }
};
template <> struct Model<4> {  // tri reduced [f1, D1, f2, D2, D3]
    static constexpr int NALL = 5, NC = 3;
    __device__ static constexpr int dpos(int c) { return c == 0 ? 1 : (c == 1 ? 3 : 4); }
    __device__ static double signal(const double *p, const double *E) {
        return p[0] * E[0] + p[2] * E[1] + (1 - p[0] - p[2]) * E[2];
    }
    __device__ static void jac(const double *p, const double *E, double x, double *r) {
        const double f3 = 1 - p[0] - p[2];
        r[0] = E[0] - E[2];
        r[1] = -x * p[0] * E[0];
        r[2] = E[1] - E[2];
        r[3] = -x * p[2] * E[1];
        r[4] = -x * f3 * E[2];
    }
};
template <> struct Model<5> {  // tri S0 [f1, D1, f2, D2, D3, S0]
    static constexpr int NALL = 6, NC = 3;
    __device__ static constexpr int dpos(int c) { return c == 0 ? 1 : (c == 1 ? 3 : 4); }
    __device__ static double signal(const double *p, const double *E) {
        return p[5] * (p[0] * E[0] + p[2] * E[1] + (1 - p[0] - p[2]) * E[2]);
    }
    __device__ static void jac(const double *p, const double *E, double x, double *r) {
        const double f3 = 1 - p[0] - p[2], S0 = p[5];
        r[0] = S0 * (E[0] - E[2]);
        r[1] = -x * S0 * p[0] * E[0];
        r[2] = S0 * (E[1] - E[2]);
        r[3] = -x * S0 * p[2] * E[1];
        r[4] = -x * S0 * f3 * E[2];
        r[5] = p[0] * E[0] + p[2] * E[1] + f3 * E[2];
    }
};
template <> struct Model<6> {  // tri full [f1, D1, f2, D2, f3, D3]
    static constexpr int NALL = 6, NC = 3;
    __device__ static constexpr int dpos(int c) { return c == 0 ? 1 : (c == 1 ? 3 : 5); }
    __device__ static double signal(const double *p, const double *E) {
        return p[0] * E[0] + p[2] * E[1] + p[4] * E[2];
    }
    __device__ static void jac(const double *p, const double *E, double x, double *r) {
        r[0] = E[0];
        r[1] = -x * p[0] * E[0];
        r[2] = E[1];
        r[3] = -x * p[2] * E[1];
        r[4] = E[2];
        r[5] = -x * p[4] * E[2];
    }
};

// Column order used inside the QR / SVD (speed only, any order gives the same step): columns sorted by typical
// norm, largest first.  One-sided Jacobi then needs 2.6-3.6 sweeps instead of 3-6 (measured offline on synthetic
// Jacobians of every model).  Index k of the factor <-> parameter colperm<MODEL>(k).
template <int MODEL> __host__ __device__ constexpr int colperm(int k) {
    constexpr int P[7][6] = {{0, 1, 2, 3, 4, 5}, {2, 0, 1, 3, 4, 5}, {2, 0, 1, 3, 4, 5}, {3, 1, 2, 0, 4, 5},
                             {4, 3, 0, 2, 1, 5}, {4, 3, 0, 2, 1, 5}, {5, 3, 1, 4, 2, 0}};
    return P[MODEL][k];
}

template <int MODEL> __device__ constexpr int comp_of_param(int j) {
    for (int c = 0; c < Model<MODEL>::NC; ++c)
        if (Model<MODEL>::dpos(c) == j) return c;
    return -1;
}

// exp(x), fp64, <= 1 ulp class: the reduction and the degree-11 polynomial of the device library's exp (k = rint(x / ln 2),
// r = x - k ln2_hi - k ln2_lo, |r| <= 0.347) without its overflow / underflow selects -- v_ldexp_f64 saturates to inf / 0
// by itself, v_cvt_i32_f64 saturates k, NaN propagates through the polynomial -- and with the polynomial split into
// even / odd halves (two dependent chains of 6 instead of one of 11: the row pass evaluates 3 of these per row at one
// wave per SIMD, where the FMA latency of a single chain is exposed).
#ifndef PNX_CF_FAST_EXP
#define PNX_CF_FAST_EXP 1
#endif
// branch-weight hint for the rare fallbacks inside the row loop (expm1(z)/z with its division): the compiler lays them out
// behind the loop, which halves the instruction footprint of the row pass (1 991 -> 993 lines of assembly)
#ifndef PNX_CF_HINTS
#define PNX_CF_HINTS 1
#endif
#if PNX_CF_HINTS
#define PNX_LIKELY(x) __builtin_expect(!!(x), 1)
#else
#define PNX_LIKELY(x) (x)
#endif
__device__ inline double exp_fast(double x) {
#if PNX_CF_FAST_EXP
    const double k = __builtin_rint(x * 1.4426950408889634);
    double r = fma(k, -0.6931471805599453, x);
    r = fma(k, -2.3190468138462996e-17, r);
    const double r2 = r * r;
    // exp(r) = 1 + r (1 + r q(r)), q = c2 + c3 r + ... + c11 r^9 with the library's minimax coefficients
    double qe = 2.7630903490112654e-07;         // c10
    qe = fma(qe, r2, 2.480149103909504e-05);    // c8
    qe = fma(qe, r2, 0.0013888888945916382);    // c6
    qe = fma(qe, r2, 0.041666666666519754);     // c4
    qe = fma(qe, r2, 0.5000000000000012);       // c2
    double qo = 2.502232256764614e-08;          // c11
    qo = fma(qo, r2, 2.755751454582531e-06);    // c9
    qo = fma(qo, r2, 0.00019841269589115522);   // c7
    qo = fma(qo, r2, 0.008333333333455043);     // c5
    qo = fma(qo, r2, 0.16666666666666477);      // c3
    const double q = fma(r, qo, qe);
    return ldexp(fma(r, fma(r, q, 1.0), 1.0), __double2int_rz(k));  // v_cvt_i32_f64 saturates, v_ldexp_f64 over / underflows by itself
#else
    return exp(x);
#endif
}

// the value lane `src` (wave uniform) holds, in every lane: two v_readlane_b32
__device__ inline double lane_bcast(double v, int src) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned int lo = __builtin_amdgcn_readlane((int)(unsigned int)u, src), hi = __builtin_amdgcn_readlane((int)(unsigned int)(u >> 32), src);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// ---------------------------------------------------------------------------------------------
// The kernel.  Block = WAVES wavefronts; LDS: b-values + per-wave signal tile y[row][lane].
// ---------------------------------------------------------------------------------------------
enum LaneState : int { ST_IDLE = 0, ST_INIT = 1, ST_RUN = 2, ST_FINAL = 3 };

template <int N> struct Park {
    static constexpr int NR = N * (N + 1) / 2;          // packed R factor of J at the current iterate (for pcov)
    static constexpr bool kParkV = (N <= 5);            // right singular vectors live in LDS between B and C
    static constexpr int NV = kParkV ? N * N : 0;
    // scalars of LDS per wave besides the b-value table; tile_rows = rows of the wave's signal tile
    __host__ __device__ static constexpr int per_wave(int tile_rows) { return kWave * (tile_rows + NR + NV); }
    // the fp64 signal tile is [ceil(n_b / 2)][64 lanes][2] (the layout a 16-byte LDS-DMA load per lane produces): an even row count
    // (= per_wave((n_b + 1) & ~1), written out: folded as one expression the compiler emits the same code as it always did)
    __host__ __device__ static constexpr int per_wave_f64(int n_b) { return kWave * (((n_b + 1) & ~1) + NR + NV); }
};

// Loop order -- one iteration = one row pass per lane:
//   refill   idle lanes pull the next voxel (x_new = strictly feasible p0) or leave for good;
//   pass     residual / cost / Jacobian / J^T f / QR(J) at x_new  (every lane);
//   D        accept or reject, trust radius, ftol / xtol tests;
//   B-light  Coleman-Li scaling + gtol test for lanes whose iterate changed or that are about to stop;
//   final    lanes that stop write their outputs and become idle (refilled at the top of the next iteration,
//            so a finished voxel never costs a wasted pass);
//   B-heavy  lanes that accepted: QR of the augmented factor + Jacobi SVD (consumes the pass's R directly);
//   C        trust-region step -> next x_new.
// Register diet: bounds stay in SGPRs unless they are per voxel (PV); R (for the covariance) and the
// singular vectors V are parked in LDS; nothing produced by the pass stays live across the next pass.
#ifndef PNX_CF_WAVES_PER_SIMD
#define PNX_CF_WAVES_PER_SIMD 1  // 2 was measured at 47-60 M voxels/s (spills, and the LDS park of 8 waves does not fit for n_b = 32)
#endif
#ifndef PNX_CF_BLOCK_WAVES
#define PNX_CF_BLOCK_WAVES 4
#endif
template <int MODEL, int N, bool FD, bool PV, bool T1, bool STREAM = false>
__global__ void __launch_bounds__(64 * PNX_CF_BLOCK_WAVES, PNX_CF_WAVES_PER_SIMD) curvefit_kernel(const CurvefitArgs A) {
    using M = Model<MODEL>;
    using PK = Park<N>;
    constexpr int NALL = M::NALL;            // parameters of the diffusion model
    constexpr int NP = NALL + (T1 ? 1 : 0);  // + T1 as the last parameter (models/*.py: `names.append("T1")`)
    constexpr int NC = M::NC;
    constexpr bool HASFIXED = (N != NP);
    static_assert(!(FD && HASFIXED), "finite-difference mode is only built without fixed parameters");
    // factor column order: static per model when all parameters are free, natural order with fixed parameters
    auto CP = [](int k) constexpr { return (HASFIXED || k >= NALL) ? k : colperm<MODEL>(k); };

    extern __shared__ double smem[];
    const int n_b = A.n_b;
    double *bsh = smem;                                   // [kMaxB]
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const bool use_w = A.use_sigma != 0;                  // wave uniform: selects the row loop of a pass, nothing else changes without sigma
    const double *wsh = smem + kMaxB;                     // [kMaxB] 1 / sigma per measurement -- only allocated with sigma
    double *ytile = smem + (use_w ? 2 * kMaxB : kMaxB) + (size_t)wave * PK::per_wave_f64(n_b);  // [ceil(n_b/2)][64][2], wave-uniform base
    double *ysh = ytile + 2 * lane;                                         // this lane's pair column
    double *rpark = ytile + (size_t)((n_b + 1) & ~1) * kWave + lane;        // [NR][64]
    double *vpark = rpark + (size_t)PK::NR * kWave;                           // [NV][64]
    for (int i = threadIdx.x; i < n_b; i += blockDim.x) bsh[i] = A.b[i];
    if (use_w)
        for (int i = threadIdx.x; i < n_b; i += blockDim.x) smem[kMaxB + i] = A.w[i];
    // largest |b| of the table (wave uniform; infinite when a b-value is not finite): the row pass tests the range of the FD
    // factor's argument against it once per pass instead of once per row
    double bmax = 0;
    for (int i = 0; i < n_b; ++i) {
        const double ab = fabs(A.b[i]);
        bmax = (ab < INFINITY) ? fmax(bmax, ab) : INFINITY;
    }
    __syncthreads();
    // the refill uses asynchronous 16-byte global->LDS loads, one per pair of b-values.  The global side needs no more than the
    // 8-byte alignment every row of doubles has (rows of an odd number of b-values start on odd multiples of 8), and the last
    // value of such a row travels with the first value of the next row as its unused partner (round 4: 31 b-values had cost
    // 18 % against 32 on the synchronous row copy, 23 against 24 12 %: profiles/odd_nb_probe.py)
    const bool dma_ok = ((reinterpret_cast<uintptr_t>(A.y) & 7) == 0);

    // ---- per-lane persistent state
    int state = ST_IDLE;
    long long vox = -1;
    unsigned long long ready_seen = 0;  // STREAM: last upload watermark this lane saw
    int pub = 0;                        // STREAM: granules [0, pub) published as left behind by this wave (wave-uniform)
    // STREAM: the queue hands out ascending indices, so once no lane of the wave holds a voxel of granule <= g the wave
    // never writes to granule g again.  It then makes its stores visible (system-scope release) and counts itself out of
    // g; the wave that completes the count raises the host's flag, and the host starts that granule's download while the
    // kernel keeps running.
    auto publish = [&](bool all) {
        const int n_gran = (int)((A.n_vox + (1ll << A.granule_shift) - 1) >> A.granule_shift);
        int upto = pub;
        while (upto < n_gran && (all || !__ballot(state != ST_IDLE && (vox >> A.granule_shift) <= upto))) ++upto;
        if (upto == pub) return;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        const unsigned int n_waves = gridDim.x * (blockDim.x / kWave);
        if ((threadIdx.x & (kWave - 1)) == __ffsll((unsigned long long)__ballot(1)) - 1) {
            for (int g = pub; g < upto; ++g) {
                const unsigned int old = __hip_atomic_fetch_add(&A.ctl->done[g], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM);
                if (old + 1 == n_waves) __hip_atomic_store(&A.host_flags[g], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        pub = upto;
    };
    double x[N], lb[N], ub[N];
    double pfull[NP];
    double g[N];
    double s[N], uf[N], R2[N][N], d[N], g_h[N];
    double Vreg[PK::kParkV ? 1 : N][PK::kParkV ? 1 : N];
    double smax = 0, smin = 0, theta = 0;
    double cost = 0, Delta = 0, alpha = 0;
    int nfev = 0, term = -99;
    bool first = false;
    double xn[N], step_h_norm = 0, step_norm = 0, predicted = 0;
    if (!PV) {
#pragma unroll
        for (int k = 0; k < N; ++k) {  // wave-uniform, never written again: stays in SGPRs
            lb[k] = A.los[k];
            ub[k] = A.his[k];
        }
    }

#ifdef PNX_CF_STAMP
    unsigned long long seg[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, act[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tl = __builtin_amdgcn_s_memtime();
    bool cf_in_team = false;
// (the stamps inside a team iteration are skipped: the whole iteration is booked under segment 8 behind it)
#define CFSTAMP(k) do { __builtin_amdgcn_s_waitcnt(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if ((k) == 8 || !cf_in_team) { seg[k] += t_ - tl; tl = t_; } } while (0)
#define CFACT(k, cond) do { act[k] += __popcll(__ballot(cond)); cnt[k] += 1; } while (0)
#else
#define CFSTAMP(k) do {} while (0)
#define CFACT(k, cond) do {} while (0)
#endif
    auto refill = [&]() {
    while (state == ST_IDLE) {
        const unsigned long long idx = atomicAdd(A.queue, 1ULL);
        if (idx >= (unsigned long long)A.n_vox) break;  // queue empty: this lane is done for good
        if constexpr (STREAM) {
            // the voxel's signal may still be on its way: wait for the upload watermark (acquire: the rows behind it are
            // visible).  Bounded: on abort or after stream_spins polls the lane leaves, so the grid always drains.
            if (idx >= ready_seen) {
                bool got = false;
                const unsigned int *abort_word = A.host_flags + ((A.n_vox + (1ll << A.granule_shift) - 1) >> A.granule_shift);
                for (unsigned int spins = 0; spins < A.stream_spins; ++spins) {
                    ready_seen = __hip_atomic_load(&A.ctl->ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
                    if (idx < ready_seen) {
                        got = true;
                        break;
                    }
                    // the abort word lives in pinned HOST memory: every read crosses PCIe, beside the upload the lanes are waiting
                    // for -- so it is looked at on every 16th poll only (an abort is seen within ~100 us instead of ~6)
                    if ((spins & 15u) == 15u && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) break;
                    __builtin_amdgcn_s_sleep(127);
                }
                if (!got) {
                    if (!__hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM))
                        __hip_atomic_store(&A.ctl->timed_out, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;  // leaves with state IDLE
                }
            }
        }
        vox = (long long)idx;
        if constexpr (!STREAM) {
            if (A.order) vox = A.order[idx];
        }
        const double *yv = A.y + (size_t)vox * n_b;
        if (dma_ok) {
            // asynchronous refill: 16-byte global->LDS loads (no VGPR round trip, nothing waits here); they land
            // while the other lanes run phases B / C and are waited for (vmcnt) right before the next row pass
            const int pairs = n_b >> 1;
            for (int c = 0; c < pairs; ++c)
                __builtin_amdgcn_global_load_lds((const void *)(yv + 2 * c), (lds_void *)(ytile + c * 2 * kWave), 16, 0, 0);
            if (n_b & 1) {
                if (vox + 1 < A.n_vox)  // the pair (last value, first value of the next row): the second half is never read
                    __builtin_amdgcn_global_load_lds((const void *)(yv + n_b - 1), (lds_void *)(ytile + pairs * 2 * kWave), 16, 0, 0);
                else  // the last row of the array has no row behind it: nothing is read beyond the caller's buffer
                    ysh[pairs * 2 * kWave] = yv[n_b - 1];
            }
        } else {
            for (int i = 0; i < n_b; ++i) ysh[(i >> 1) * 2 * kWave + (i & 1)] = yv[i];
        }
        bool okb = true, okp = true;
        double p0v[N];
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
        if (HASFIXED) {
#pragma unroll
            for (int j = 0; j < NP; ++j) pfull[j] = 0;
            for (int f = 0; f < A.n_fixed; ++f) {
                const double fv = A.fixed_per_voxel ? A.fixed[(size_t)f * A.n_vox + vox] : A.fixeds[f];
#pragma unroll
                for (int j = 0; j < NP; ++j)
                    if (A.fixed_idx[f] == j) pfull[j] = fv;
            }
        }
        if (!okb || !okp) {
            // reference: ValueError inside curve_fit -> params = p0, cov = NaN, success = False
            // (a non-finite signal is detected in the voxel's first row pass)
            const int st = !okb ? -1 : -3;
#pragma unroll
            for (int k = 0; k < N; ++k) A.popt[(size_t)k * A.n_vox + vox] = p0v[k];
            if (A.status) A.status[vox] = (int8_t)st;  // pcov_kernel writes the NaN covariance
            if (A.nfev) A.nfev[vox] = 0;
            if (A.cost) A.cost[vox] = NAN;
            continue;  // stays IDLE -> next voxel
        }
#pragma unroll
        for (int k = 0; k < N; ++k) xn[k] = strictly_feasible_r(p0v[k], lb[k], ub[k]);
        state = ST_INIT;
        nfev = 0;
        term = -99;
        alpha = 0.0;
    }
    };
    refill();
    if constexpr (STREAM) {
        // `pub` is only uniform among the lanes that are still in the loop below (a lane that left keeps the value it left
        // with), so nothing is published behind the loop: the last lane of the wave to run dry publishes the rest from inside
        // it, and a wave that never got a voxel does so here.
        if (!__ballot(state != ST_IDLE)) publish(true);
    }
    // One loop iteration as listed above.  team_c = false: every lane that is in the loop holds a voxel and walks its rows itself.
    // team_c = true (team mode, below): all 64 lanes are here, lane `owner` holds the wave's last voxel, the others evaluate its rows.
    auto iterate = [&](auto team_c, const int owner) __attribute__((always_inline)) {
        constexpr bool TM = decltype(team_c)::value;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // LDS-DMA signal tiles have landed
        CFSTAMP(0);
        CFACT(1, true);

        // ------------------------------------------------------------------ row pass at xn
        // residual f = model(xn) - y, cost, Jacobian (closed-form 2-point FD or analytic), g = J^T f, QR of J
        double Rn[N][N], qn[N], gn[N], cost_new = 0;
        bool finite_f = true, yfinite = true;
        {
            if constexpr (TM) {
                // the evaluation point is the owner's: with it in every lane, the lines below give every lane the owner's pe, dxv
                // and T1 factors.  (A helper is idle for good: its own copies are dead.)
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    xn[k] = lane_bcast(xn[k], owner);
                    if (PV) {
                        lb[k] = lane_bcast(lb[k], owner);
                        ub[k] = lane_bcast(ub[k], owner);
                    }
                }
                if (HASFIXED) {
#pragma unroll
                    for (int j = 0; j < NP; ++j) pfull[j] = lane_bcast(pfull[j], owner);
                }
            }
            double pe[NP];  // full parameter vector at the evaluation point
            if (HASFIXED) {
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    pe[j] = pfull[j];
#pragma unroll
                    for (int k = 0; k < N; ++k)
                        if (A.free_idx[k] == j) pe[j] = xn[k];
                }
            } else {
#pragma unroll
                for (int j = 0; j < NP; ++j) pe[j] = xn[j];
            }
            double dxv[N];
            if (FD) {
                // _numdiff.py:146-163 (_compute_absolute_step) and :13-90 ('1-sided', num_steps = 1)
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double sign = (xn[k] >= 0) ? 1.0 : -1.0;
                    double h = kSqrtEps * sign * fmax(1.0, fabs(xn[k]));
                    const double lower_dist = xn[k] - lb[k], upper_dist = ub[k] - xn[k];
                    const double xx = xn[k] + h;
                    const bool violated = (xx < lb[k]) || (xx > ub[k]);
                    const bool fitting = fabs(h) <= fmax(lower_dist, upper_dist);
                    if (violated && fitting) h = -h;
                    if (!fitting) h = (upper_dist >= lower_dist) ? upper_dist : -lower_dist;
                    dxv[k] = (xn[k] + h) - xn[k];  // _numdiff.py:596 "recompute dx as exactly representable number"
                }
            }
            // T1 / STEAM relaxation factor (row independent): S = base * A1 [* eTM], A1 = 1 - exp(-TR/T1)
            // (model_functions/multiexp.py:210-241); its T1 derivative analytically (multiexp.py:244-302) or as
            // SciPy's 2-point quotient (fac(T1 + dx) - fac(T1)) / dx -- two extra exp per PASS, not per row.
            double A1 = 1.0, eTM = 1.0, fac = 1.0, dfac = 0.0;
            if (T1) {
                const bool steam = A.t1_mode == 2;
                const double T1v = pe[T1 ? NALL : 0];
                const double eTR = exp(-A.tr / T1v);
                A1 = 1 - eTR;
                eTM = steam ? exp(-A.tm / T1v) : 1.0;
                fac = A1 * eTM;
                dfac = steam ? eTM / (T1v * T1v) * (-A.tr * eTR + A.tm * A1) : (-eTR * A.tr / (T1v * T1v));
                if (FD) {  // T1 is the last free parameter in FD mode (no fixed parameters there)
                    const double dx = dxv[N - 1];
                    const double T2 = T1v + dx;
                    const double fac2 = (1 - exp(-A.tr / T2)) * (steam ? exp(-A.tm / T2) : 1.0);
                    dfac = (fac2 - fac) / dx;
                }
            }
#pragma unroll
            for (int i = 0; i < N; ++i) {
                qn[i] = 0;
                gn[i] = 0;
#pragma unroll
                for (int j = 0; j < N; ++j) Rn[i][j] = 0;
            }
            constexpr int kRowBlk = row_blk<N>();
            static_assert(kRowBlk % 2 == 0, "a block reads its signal values as [pair][lane][2] pairs");
            // One block of kRowBlk rows: residuals, Jacobian rows, J^T f, then the Householder merge.  The variants differ in
            // control flow only, never in an arithmetic operation or its order:
            //   FASTGZ  the pass has established that |b dx| < 2e-4 holds for every row and every lane, so the FD factor is the
            //           cubic the per-row test would have selected -- no compare, no branch;
            //   USEW    rows are scaled by 1 / sigma (the tail block tests use_w at run time instead);
            //   TAIL    the last, partial block of an n_b that is no multiple of kRowBlk: rows beyond n_b are evaluated at row 0
            //           and replaced by zeros.  A full block needs none of those selects and reads b and y as 16-byte pairs up
            //           front, which leaves it one basic block up to qr_merge's sig > 0 tests: the scheduler is free to
            //           interleave the exp chains of all its rows and to cover the LDS latency once per block.
            // The body of one row -- exp, model, Jacobian row, FD factor, 1 / sigma -- at row ii (b-value bb, signal yi): the residual
            // in r0_out, the Jacobian row in jr.  One text for the lane that walks all rows of its own voxel (row_block) and for
            // the lanes of a team, which take one row each of the owner's voxel (team_rows).
            auto row_eval = [&](auto fastgz_c, auto usew_c, auto tail_c, const int ii, const double bb, const double yi, double &r0_out,
                                double (&jr)[N]) __attribute__((always_inline)) {
                constexpr bool FASTGZ = decltype(fastgz_c)::value, USEW = decltype(usew_c)::value, TAIL = decltype(tail_c)::value;
                const double nb = -bb;
                double E[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) E[c] = exp_fast(nb * pe[M::dpos(c)]);
                const double base = M::signal(pe, E);
                double r0 = (T1 ? base * A1 * eTM : base) - yi;
                {
                    double ja[NP];
                    M::jac(pe, E, bb, ja);
                    if (FD) {
                        // SciPy's 2-point quotient (f(x + dx e_k) - f(x)) / dx in closed form.  The models are
                        // linear in every parameter except the D_c, and for a D_c
                        //   f(D_c + dx) - f(D_c) = w_c exp(-b D_c) (exp(-b dx) - 1),
                        // so the quotient is the analytic column times g(z) = expm1(z)/z, z = -b dx: no second
                        // exp per column, no cancellation, and SciPy's deterministic O(dx) bias (up to 1e-5
                        // relative at b = 1200) -- which is what separates its iterates from an
                        // analytic-Jacobian run -- is kept exactly.
#pragma unroll
                        for (int k = 0; k < NALL; ++k) {
                            if (comp_of_param<MODEL>(k) >= 0) {
                                const double z = nb * dxv[k];
                                double gz;
#if PNX_CF_FAST_EXP
                                if (FASTGZ || PNX_LIKELY(fabs(z) < 2e-4))  // dx ~ 1.5e-8 max(1, |D|): the normal case; z^4 / 120 < 2e-17
                                    gz = fma(z, fma(z, fma(z, 1.0 / 24, 1.0 / 6), 0.5), 1.0);
                                else
#endif
                                if (fabs(z) < 1e-3)
                                    gz = 1.0 + z * (0.5 + z * (1.0 / 6 + z * (1.0 / 24 + z * (1.0 / 120 + z * (1.0 / 720)))));
                                else
                                    gz = expm1(z) / z;
                                ja[k] *= gz;
                            }
                        }
                    }
                    if (T1) {
#pragma unroll
                        for (int k = 0; k < NALL; ++k) ja[k] *= fac;
                        ja[NP - 1] = base * dfac;
                    }
                    if (TAIL ? use_w : USEW) {  // transform * (f - y), transform[:, None] * jac (the 2-point quotient of scaled residuals)
                        const double t = wsh[ii];
                        r0 *= t;
#pragma unroll
                        for (int k = 0; k < NP; ++k) ja[k] *= t;
                    }
                    if (HASFIXED) {
#pragma unroll
                        for (int k = 0; k < N; ++k) {
                            jr[k] = 0;
#pragma unroll
                            for (int j = 0; j < NP; ++j)
                                jr[k] = (A.free_idx[k] == j) ? ja[j] : jr[k];
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < N; ++k) jr[k] = ja[k];
                    }
                }
                r0_out = r0;
            };
            // What a finished row adds to the pass, in row order: cost, J^T f, and its line of the block that is merged next.
            auto row_consume = [&](double (&brow)[N + 1], const bool live, const double r0, const double (&jr)[N]) __attribute__((always_inline)) {
                const double rr = live ? r0 : 0.0;
                finite_f = finite_f && isfinite(rr);
                cost_new += rr * rr;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double jk = live ? jr[k] : 0.0;
                    gn[k] += jk * rr;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) brow[k] = live ? jr[CP(k)] : 0.0;  // factor column k = parameter CP(k)
                brow[N] = rr;
            };
            auto row_block = [&](auto fastgz_c, auto usew_c, auto tail_c, const int i0) __attribute__((always_inline)) {
                constexpr bool TAIL = decltype(tail_c)::value;
                double blk[kRowBlk][N + 1];
                double bv[TAIL ? 1 : kRowBlk], yv[TAIL ? 1 : kRowBlk];
                if constexpr (!TAIL) {
#pragma unroll
                    for (int r = 0; r < kRowBlk; r += 2) {  // i0 is even: rows (i0 + r, i0 + r + 1) are one pair of the tile
                        const double2 b2 = *reinterpret_cast<const double2 *>(bsh + i0 + r);
                        const double2 y2 = *reinterpret_cast<const double2 *>(ysh + (size_t)(i0 + r) * kWave);
                        bv[r] = b2.x;
                        bv[r + 1] = b2.y;
                        yv[r] = y2.x;
                        yv[r + 1] = y2.y;
                    }
                }
#pragma unroll
                for (int r = 0; r < kRowBlk; ++r) {
                    const bool live = !TAIL || (i0 + r < n_b);
                    const int ii = live ? i0 + r : 0;
                    const double bb = TAIL ? bsh[ii] : bv[TAIL ? 0 : r];
                    const double yi = TAIL ? ysh[(ii >> 1) * 2 * kWave + (ii & 1)] : yv[TAIL ? 0 : r];
                    yfinite = yfinite && isfinite(yi);
                    double r0, jr[N];
                    row_eval(fastgz_c, usew_c, tail_c, ii, bb, yi, r0, jr);
                    row_consume(blk[r], live, r0, jr);
                }
                CFSTAMP(1);  // rows of the block: exp, model, Jacobian row, J^T f (diagnostic builds: -DPNX_CF_STAMP)
                qr_merge<N, kRowBlk>(Rn, qn, blk);
                CFSTAMP(6);  // the sequential Householder merge of the block into R
            };
            auto row_loop = [&](auto fastgz_c, auto usew_c) __attribute__((always_inline)) {
                int i0 = 0;
                for (; i0 + kRowBlk <= n_b; i0 += kRowBlk) row_block(fastgz_c, usew_c, BoolC<false>{}, i0);
                if (i0 < n_b) row_block(BoolC<false>{}, BoolC<false>{}, BoolC<true>{}, i0);
            };
            // FD factor range test, once per pass instead of once per row and column: rounded multiplication is monotone in |b|,
            // so a lane whose |bmax dx_k| is below the threshold passes the per-row test in every row; with every lane of the
            // wave passing (the normal case: dx ~ 1.5e-8 max(1, |D|)) the loop without the test computes the same bits.  A NaN
            // dx fails the comparison and takes the generic loop.
            // The instantiations with six and more free parameters use all 512 registers of a lane and spill: the specialised
            // loops cost them scratch, so they keep the one generic loop (the tail variant run over every block).
            constexpr bool kOneLoop = (N >= 6);
            bool gz_cubic = FD && PNX_CF_FAST_EXP && !kOneLoop;
            if (FD && PNX_CF_FAST_EXP && !kOneLoop) {
                bool in_range = true;
#pragma unroll
                for (int k = 0; k < NALL; ++k)
                    if (comp_of_param<MODEL>(k) >= 0) in_range = in_range && (fabs(bmax * dxv[k]) < 2e-4);
                gz_cubic = __ballot(!in_range) == 0;
            }
            if constexpr (TM) {
                // Team row pass: lane l evaluates rows l and l + 64 of the owner's voxel with the generic row body (per-row FD factor
                // test, run-time use_w: the bits of the loops the owner would have picked) and leaves [jr | r] in the wave's
                // signal tile, in the columns of idle lanes (the half of the tile the owner's column is not in).  Then every
                // lane reads the rows back in index order -- same address in all lanes: a broadcast read -- and accumulates cost,
                // J^T f and the QR factor exactly as row_block does; the owner's copy is the one that is used.  LDS operations of a
                // wave execute in order and nothing here waits for another lane or wave: the fences only keep the compiler from
                // moving the reads over the writes.
                static_assert(N + 1 <= 8 && 2 * kWave == kMaxB, "a team row is 8 doubles; two rows per lane cover every n_b");
                double *trow = ytile + (owner < kWave / 2 ? kWave : 0);  // row i: trow[(i >> 1) * 2 * kWave + (i & 1) * 8 + 0 .. N]
                const double *yown = ytile + 2 * owner;
                bool ybad = false;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
                for (int h = 0; h < kMaxB / kWave; ++h) {
                    if (h * kWave < n_b) {
                        const int i = lane + h * kWave;
                        const bool live = i < n_b;
                        const int ii = live ? i : 0;
                        const double yi = yown[(ii >> 1) * 2 * kWave + (ii & 1)];
                        ybad = ybad || !isfinite(yi);
                        double r0, jr[N];
                        row_eval(BoolC<false>{}, BoolC<false>{}, BoolC<true>{}, ii, bsh[ii], yi, r0, jr);
                        if (live) {
                            double *tr = trow + (i >> 1) * 2 * kWave + (i & 1) * 8;
#pragma unroll
                            for (int k = 0; k < N; ++k) tr[k] = jr[k];
                            tr[N] = r0;
                        }
                    }
                }
                yfinite = __ballot(ybad) == 0;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int i0 = 0; i0 < n_b; i0 += kRowBlk) {
                    double blk[kRowBlk][N + 1];
#pragma unroll
                    for (int r = 0; r < kRowBlk; ++r) {
                        const bool live = i0 + r < n_b;
                        const int ii = live ? i0 + r : 0;
                        const double *tr = trow + (ii >> 1) * 2 * kWave + (ii & 1) * 8;
                        double jr[N];
#pragma unroll
                        for (int k = 0; k < N; ++k) jr[k] = tr[k];
                        row_consume(blk[r], live, tr[N], jr);
                    }
                    qr_merge<N, kRowBlk>(Rn, qn, blk);
                }
            } else if constexpr (kOneLoop) {
                for (int i0 = 0; i0 < n_b; i0 += kRowBlk) row_block(BoolC<false>{}, BoolC<false>{}, BoolC<true>{}, i0);
            } else if (PNX_LIKELY(!use_w && (gz_cubic || !FD))) {
                if constexpr (FD && PNX_CF_FAST_EXP)
                    row_loop(BoolC<true>{}, BoolC<false>{});
                else
                    row_loop(BoolC<false>{}, BoolC<false>{});
            } else if (use_w) {
                row_loop(BoolC<false>{}, BoolC<true>{});
            } else {
                if constexpr (FD) row_loop(BoolC<false>{}, BoolC<false>{});
            }
            cost_new *= 0.5;
        }

        CFSTAMP(1);
        if constexpr (TM) {
            if (state == ST_IDLE) return;  // helpers: the scalar phases are the owner's
        }
        // ------------------------------------------------------------------ phase D: accept / reject
        bool accepted = false;
        int final_status = 0;
        if (state == ST_INIT) {
            if (!finite_f) {
                // non-finite signal: curve_fit's asarray_chkfinite raises (-2); otherwise least_squares.py:857-858
                // "Residuals are not finite in the initial point" (-4) -> failure sentinel either way
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
                Delta = 0.25 * step_h_norm;  // trf.py:337-339
            } else {
                const double actual = cost - cost_new;
                double ratio;  // update_tr_radius (common.py:222-245)
                if (predicted > 0)
                    ratio = actual / predicted;
                else if (predicted == 0 && actual == 0)
                    ratio = 1;
                else
                    ratio = 0;
                double Delta_new = Delta;
                if (ratio < 0.25)
                    Delta_new = 0.25 * step_h_norm;
                else if (ratio > 0.75 && step_h_norm > 0.95 * Delta)
                    Delta_new = Delta * 2.0;
                // check_termination (common.py:705-717)
                const bool ftol_ok = (actual < A.ftol * cost) && (ratio > 0.25);
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

        // ------------------------------------------------------------------ light head of phase B
        // (trf.py:260-272: scaling vector, first trust radius, gtol test, leave when done or out of evaluations)
        double v[N], dv[N], g_norm = 0;
        if (state == ST_RUN && (accepted || term != -99 || nfev >= A.max_nfev)) {
#pragma unroll
            for (int i = 0; i < N; ++i) {  // CL_scaling_vector (common.py:467-508)
                v[i] = 1.0;
                dv[i] = 0.0;
                if (g[i] < 0 && isfinite(ub[i])) {
                    v[i] = ub[i] - x[i];
                    dv[i] = -1;
                }
                if (g[i] > 0 && isfinite(lb[i])) {
                    v[i] = x[i] - lb[i];
                    dv[i] = 1;
                }
                g_norm = fmax(g_norm, fabs(g[i] * v[i]));
            }
            if (first) {  // trf.py:232-236
                double t = 0;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const double q = x[i] / sqrt(v[i]);
                    t += q * q;
                }
                Delta = sqrt(t);
                if (Delta == 0) Delta = 1.0;
                first = false;
            }
            if (g_norm < A.gtol) term = 1;
            if (term != -99 || nfev >= A.max_nfev) {
                final_status = (term == -99) ? 0 : term;
                state = ST_FINAL;
            }
        }

        CFSTAMP(2);
        CFACT(3, state == ST_FINAL);
        // ------------------------------------------------------------------ outputs of finished voxels
        if (state == ST_FINAL) {
            const bool ok = final_status > 0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                // failure: the reference returns the p0 it was given (curvefit.py:308-317)
                const double pk = ok ? x[k] : (PV ? A.p0[(size_t)k * A.n_vox + vox] : A.p0s[k]);
                A.popt[(size_t)k * A.n_vox + vox] = pk;
            }
            if (A.status) A.status[vox] = (int8_t)final_status;
            if (A.nfev) A.nfev[vox] = nfev;
            if (A.cost) A.cost[vox] = cost;
            if (A.pcov && ok) {
                // The covariance needs another n x n SVD; done here it would run with a handful of lanes active
                // in (almost) every loop iteration.  The packed R factor of the final Jacobian goes to the voxel's
                // pcov slot instead and pcov_kernel turns it into pcov with all lanes busy.
                double *pc = A.pcov + (size_t)vox * N * N;
#pragma unroll
                for (int t = 0; t < PK::NR; ++t) pc[t] = rpark[t * kWave];
            }
            state = ST_IDLE;
        }
        CFACT(0, state == ST_IDLE);
        if constexpr (STREAM) {
            const bool any_idle = __ballot(state == ST_IDLE) != 0;
            if (state == ST_IDLE) refill();
            if (any_idle) publish(false);
        } else if constexpr (!TM) {  // (a team only forms behind a dry queue)
            if (state == ST_IDLE) refill();  // claim the next voxel now: its signal streams in behind phases B / C
        }

        CFSTAMP(3);
        CFACT(4, state == ST_RUN && accepted);
        CFACT(5, state == ST_RUN);
        if (state == ST_RUN) {
            // -------------------------------------------------------------- heavy phase B (iterate changed)
            if (accepted) {
                double diag_h[N];
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    d[i] = sqrt(v[i]);
                    diag_h[i] = g[i] * dv[i];
                    g_h[i] = d[i] * g[i];
                }
                // QR of [R*D; diag(sqrt(diag_h))] -> R2, q2 ;  J_aug = Q R2 (trf.py:300-306)
                double q2[N];
                double blk[N][N + 1];
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    q2[i] = qn[i];
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        R2[i][j] = (j >= i) ? Rn[i][j] * d[CP(j)] : 0.0;
                        blk[i][j] = (i == j) ? sqrt(diag_h[CP(i)]) : 0.0;
                    }
                    blk[i][N] = 0.0;
                }
                qr_merge<N, N>(R2, q2, blk);
                // SVD of R2 through one-sided Jacobi on W = R2^T (lower triangular):  W Vw = Uw S  =>
                // R2 = Vw S Uw^T: right singular vectors of J_aug = normalised columns of W, uf = Vw^T q2.
                double W[N][N], Vw[N][N];
#pragma unroll
                for (int i = 0; i < N; ++i)
#pragma unroll
                    for (int j = 0; j < N; ++j) W[i][j] = (i >= j) ? R2[j][i] : 0.0;
                jacobi_svd<N>(W, Vw);
                smax = 0;
                smin = INFINITY;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    double nn = 0, dq = 0;
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        nn += W[i][k] * W[i][k];
                        dq += Vw[i][k] * q2[i];
                    }
                    double inv = 0.0;  // singular value and its reciprocal from one v_rsq_f64 seed (normalisation only: ~1 ulp is fine)
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
                    smax = fmax(smax, nn);
                    smin = fmin(smin, nn);
                }
                theta = fmax(0.995, 1 - g_norm);
            }
            CFSTAMP(4);
            // -------------------------------------------------------------- phase C: trial step
            double V[N][N];
#pragma unroll
            for (int i = 0; i < N; ++i)
#pragma unroll
                for (int k = 0; k < N; ++k)
                    V[i][k] = PK::kParkV ? vpark[(i * N + k) * kWave] : Vreg[PK::kParkV ? 0 : i][PK::kParkV ? 0 : k];
            // everything below works in the factor's column order (a relabelling of the parameters)
            double xP[N], lbP[N], ubP[N], dP[N], ghP[N];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                xP[i] = x[CP(i)];
                lbP[i] = lb[CP(i)];
                ubP[i] = ub[CP(i)];
                dP[i] = d[CP(i)];
                ghP[i] = g_h[CP(i)];
            }
            double p_h[N], p[N], step[N], step_h[N];
            alpha = solve_lsq_trust_region<N>(n_b, uf, s, V, smax, smin, Delta, alpha, p_h);
#pragma unroll
            for (int i = 0; i < N; ++i) p[i] = dP[i] * p_h[i];
            predicted = select_step<N>(xP, R2, ghP, p, p_h, dP, Delta, lbP, ubP, theta, step, step_h);
#pragma unroll
            for (int i = 0; i < N; ++i) xn[CP(i)] = strictly_feasible0(xP[i] + step[i], lbP[i], ubP[i]);
            step_h_norm = normn<N>(step_h);
            step_norm = normn<N>(step);
            CFSTAMP(5);
        }
    };
    // Team mode (fp64, not streamed, N <= 5; the 6- and 7-parameter instantiations have no register to spare): a lane leaves the loop
    // only after the queue has run dry, so a wave with kTeamMax lanes left in it is drained -- nothing will refill it -- and its
    // other lanes wait behind the loop.  Such a wave leaves the loop as a whole and finishes its last voxel in the second loop,
    // where the fifth of an evaluation that is independent across rows (exp, model, Jacobian row) runs one row per lane instead of
    // one after the other in a single lane: the wave that everything waits for at the end of a launch gets there sooner.
    // Every value is computed by the source expression the lone lane would have used, sums run in the same order: bit-identical.
    constexpr bool kTeam = !STREAM && N <= 5;
    constexpr int kTeamMax = 1;  // two to four owners served one after the other: not built
    for (;;) {
        CFSTAMP(7);
        if (state == ST_IDLE) break;
        if constexpr (kTeam) {
            if (!PNX_LIKELY(__popcll(__ballot(1)) > kTeamMax || !A.team)) break;
        }
        iterate(BoolC<false>{}, 0);
    }
    if constexpr (kTeam) {
        // all 64 lanes are back together here; no lane touches the queue or global memory again except the owner's result stores
#ifdef PNX_CF_STAMP
        cf_in_team = true;
#endif
        for (;;) {
            const unsigned long long livem = __ballot(state != ST_IDLE);
            if (!livem) break;
            iterate(BoolC<true>{}, __ffsll(livem) - 1);
            CFSTAMP(8);
            CFACT(8, true);
        }
    }
#ifdef PNX_CF_STAMP
    if (threadIdx.x == 0 && blockIdx.x == 3)
        printf("CFSTAMP refill=%llu pass_rows=%llu pass_qr_merge=%llu D+Blight=%llu final=%llu Bheavy=%llu C=%llu loop=%llu team=%llu | iters=%llu team_iters=%llu idle_at_top=%.2f final=%.2f Bheavy=%.2f run=%.2f\n",
               seg[0], seg[1], seg[6], seg[2], seg[3], seg[4], seg[5], seg[7], seg[8], cnt[1], cnt[8], (double)act[0] / cnt[0], (double)act[3] / cnt[3],
               (double)act[4] / cnt[4], (double)act[5] / cnt[5]);
#endif
}

// ---------------------------------------------------------------------------------------------
// Covariance epilogue (one lane per voxel, fully convergent): turns the packed R factor of the final
// Jacobian that curvefit_kernel parked in pcov[vox] into SciPy's pcov
//   pinv(J^T J) * 2 cost / (m - n)   with singular values <= eps * max(m, n) * s_max dropped  (absolute_sigma: unscaled)
// (scipy/optimize/_minpack_py.py:1036-1066), NaN for failed voxels (curvefit.py:236-243, 312-317).
// ---------------------------------------------------------------------------------------------
struct ColPerm {
    int p[kMaxP];
};

template <int N>
__global__ void __launch_bounds__(256) pcov_kernel(double *pcov, const int8_t *status, const double *cost,
                                                   long long n_vox, int n_b, const ColPerm cp, int absolute_sigma) {
    const long long vox = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (vox >= n_vox) return;
    double *pc = pcov + (size_t)vox * N * N;
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
            for (int j = i; j < N; ++j) W[j][i] = pc[t++];  // W = R^T
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
    const double thr = kEps * (n_b > N ? n_b : N) * sqrt(sm);
    const bool dof = absolute_sigma || n_b > N;  // absolute_sigma: no scaling, hence no degrees-of-freedom condition (_minpack_py.py:1057-1063)
    const double s_sq = absolute_sigma ? 1.0 : (dof ? 2.0 * cost[vox] / (double)(n_b - N) : 0.0);
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
        for (int j = 0; j < N; ++j) pc[cp.p[i] * N + cp.p[j]] = (bad || !dof) ? INFINITY : out[i][j] * s_sq;  // factor order -> parameter order
}

}  // namespace pnx
