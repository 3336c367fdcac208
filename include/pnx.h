/*
 * pnx.h -- C ABI of the MI355X (gfx950) batched per-voxel fitting library (libpnx_hip.so).
 *
 * This is the drop-in boundary for the hot path of darksim33/Pyneapple's pixelwise fitter:
 * everything a solver plugin needs in order to replace
 *     CurveFitSolver._fit_data / _fit_single_pixel   (src/pyneapple/solvers/curvefit.py:171-317)
 *     NNLSSolver._fit_data / _fit_single_pixel       (src/pyneapple/solvers/nnls_solver.py:129-210)
 * i.e. the per-voxel calls into scipy.optimize.curve_fit (method="trf") and scipy.optimize.nnls.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch/numpy types.
 *   - Every function returns 0 on success or a negative pnx_error; the message of the last
 *     error of the calling thread is available through pnx_last_error().
 *   - `mem` says where the *per-voxel* arrays live: PNX_MEM_HOST (pageable host memory; the library
 *     moves the volume over PCIe on its own streams and helper threads while the kernels run -- a curve fit
 *     as ONE kernel that waits at an upload watermark and whose finished voxels are
 *     downloaded while it is still fitting, everything else as chunks through a ring of device slots --
 *     and returns when every result is in place; `stream` is synchronised on entry) or PNX_MEM_DEVICE (pointers are HBM addresses on `device`; the call only
 *     enqueues work on `stream` and returns; the caller synchronises).  Small shared inputs
 *     (b-values, shared p0/bounds, basis, regulariser) are ALWAYS host pointers.
 *   - Thread safety: every entry point may be called from several host threads (e.g. one per
 *     device).  An NNLS plan owns device scratch that serves one solve at a time: host-mode solves
 *     on one plan serialise internally, device-mode solves on one plan must be enqueued on ONE
 *     stream (or be ordered by the caller).
 *   - Throughput: a curve-fit batch ends in a tail -- a few voxels that need ten times the average number of evaluations
 *     keep their lanes busy after the work queue is empty (about 6 of 37 ms for 4 M triexp voxels).  Device-mode callers
 *     with independent batches should enqueue them on two or more streams: the next batch fills the idle SIMDs (the host
 *     mode pays one tail per call and downloads during it).
 *   - The caller allocates all outputs.  The library owns only device scratch.
 *   - Per-voxel numerical failure never produces an error code: it is reported in `status[]`
 *     with the reference's sentinel outputs (curvefit.py:308-317, nnls_solver.py:201-210).
 *   - Environment.  A production process reads five variables, none of which changes a result or selects a kernel:
 *     PNX_STREAM_CACHE_MB (staging slab a host-array curve fit keeps per device, default 8192), PNX_COPY_PIECE_MB (32) and
 *     PNX_COPY_THREADS (4) of pnx_upload / pnx_download, PNX_HOST_TOUCHERS and PNX_STREAM_OUT_THREADS (helper threads of a
 *     host-array call).  Everything else the sources know -- the NNLS switches PNX_NNLS_NO_BLK (banded regularisers take the
 *     Gram form), PNX_BLK_ROUTE_PERMILLE and PNX_BLK_ROUTE_DEBUG (the block kernel's pilot), PNX_NNLS_DEFER_CAP (deferred
 *     hand-over), chunk sizes of the host pipelines, trace output (PNX_HOST_TRACE; PNX_LAUNCH_TRACE: one stderr line per
 *     curve-fit launch -- model, free parameters, FD / PV / T1 / STREAM instantiation, n_b, waves per block, LDS bytes, grid --
 *     and per sweep call the kernel it chose: full-tile 16 / 32, generic, or full-tile then generic, the generic kernel with
 *     its block size and copy path) and the test hooks PNX_NNLS_TEST_REJECT (forces rejected
 *     candidate columns in the NNLS block kernel) and PNX_CF_TEAM=0 (the curve fit's drained waves keep their last voxel in
 *     one lane instead of evaluating its rows as a team: same bits, longer tail) -- is read ONLY when the
 *     process was started with PNX_ENABLE_TEST_HOOKS=1 (looked at once, at the first query); the test-suite and the
 *     profiling scripts set it, bench.py and the plugin never do.
 */
#ifndef PNX_H
#define PNX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared here are its only exports. */
#if defined(__GNUC__) || defined(__clang__)
#define PNX_API __attribute__((visibility("default")))
#else
#define PNX_API
#endif

#define PNX_VERSION_MAJOR 0
#define PNX_VERSION_MINOR 2
#define PNX_MAX_PARAMS 8  /* max model parameters (free + fixed) */
#define PNX_MAX_BVALUES 128

/* Forward models: parameter order is the reference's `_all_param_names`
 * (models/monoexp.py:91-101, biexp.py:103-118, triexp.py:103-121; formulas
 * model_functions/multiexp.py:35-202). */
typedef enum pnx_model {
    PNX_MODEL_MONO = 0,        /* [S0, D]                      S0*exp(-b D)                          */
    PNX_MODEL_BI_REDUCED = 1,  /* [f1, D1, D2]                 f1 e1 + (1-f1) e2                      */
    PNX_MODEL_BI_S0 = 2,       /* [f1, D1, D2, S0]             S0 (f1 e1 + (1-f1) e2)                 */
    PNX_MODEL_BI_FULL = 3,     /* [f1, D1, f2, D2]             f1 e1 + f2 e2                          */
    PNX_MODEL_TRI_REDUCED = 4, /* [f1, D1, f2, D2, D3]         f1 e1 + f2 e2 + (1-f1-f2) e3           */
    PNX_MODEL_TRI_S0 = 5,      /* [f1, D1, f2, D2, D3, S0]     S0 (...)                               */
    PNX_MODEL_TRI_FULL = 6     /* [f1, D1, f2, D2, f3, D3]     f1 e1 + f2 e2 + f3 e3                  */
} pnx_model;

typedef enum pnx_jac_mode {
    PNX_JAC_FD = 0,       /* SciPy '2-point' finite differences -- what the reference uses when no
                             parameter is fixed (curvefit.py:289-293 -> _minpack_py.py:1000-1001) */
    PNX_JAC_ANALYTIC = 1  /* model.jacobian() -- what the reference uses with fixed parameters
                             (curvefit.py:274-288) */
} pnx_jac_mode;

typedef enum pnx_mem { PNX_MEM_HOST = 0, PNX_MEM_DEVICE = 1 } pnx_mem;

typedef enum pnx_error {
    PNX_OK = 0,
    PNX_ERR_INVALID = -1,     /* bad argument (shape, enum, NULL) -- the reference raises ValueError */
    PNX_ERR_UNSUPPORTED = -2, /* combination not built into this library */
    PNX_ERR_NO_DEVICE = -3,   /* no usable MI355X / HIP runtime error at start-up */
    PNX_ERR_HIP = -4,         /* HIP runtime error during the call */
    PNX_ERR_NOMEM = -5
} pnx_error;

/* Per-voxel status written by pnx_curvefit_batch_f64 (int8):
 *    1..4  SciPy termination status (gtol / ftol / xtol / ftol+xtol): success
 *    0     max_nfev reached            -> reference: RuntimeError -> params=p0, cov=NaN, success=False
 *   -1     some lb >= ub               -> reference: ValueError   -> same sentinel
 *   -2     non-finite signal           -> reference: ValueError (asarray_chkfinite) -> same sentinel
 *   -3     p0 outside its bounds       -> reference: ValueError   -> same sentinel
 *   -4     non-finite residual at p0   -> reference: ValueError   -> same sentinel          */
/* Per-voxel status written by pnx_nnls_batch_f64 (int8):
 *    1 converged; 0 iteration limit (`iteration == max_iter`) -> zeros, ||y||; -2 non-finite input */

typedef struct pnx_curvefit_opts {
    int32_t model;                       /* pnx_model */
    int32_t n_b;                         /* number of b-values (<= PNX_MAX_BVALUES) */
    int32_t n_free;                      /* free parameters being fitted */
    int32_t n_fixed;                     /* fixed parameters; n_free + n_fixed == model's parameter count */
    int32_t free_idx[PNX_MAX_PARAMS];    /* ascending positions of the free parameters in the model's order
                                            (models/base.py:167-173 _free_indices) */
    int32_t fixed_idx[PNX_MAX_PARAMS];   /* positions of the fixed parameters */
    int32_t per_voxel_p0_bounds;         /* 0: p0/lo/hi are (n_free,) shared; 1: (n_free, n_vox) parameter-major
                                            (utility/validation.py:177-203,248-297; fitters/ideal.py:240-242) */
    int32_t fixed_per_voxel;             /* 0: fixed is (n_fixed,); 1: (n_fixed, n_vox)  (curvefit.py:161-169) */
    int32_t max_nfev;                    /* reference's max_iter -> SciPy max_nfev (curvefit.py:303) */
    int32_t jac_mode;                    /* pnx_jac_mode */
    int32_t t1_mode;                     /* 0 none; 1 T1: S*(1-exp(-TR/T1)); 2 STEAM: additionally *exp(-TM/T1).
                                            T1 is then one more model parameter, appended last
                                            (model_functions/multiexp.py:210-241, each model class appends "T1" to its names) */
    int32_t absolute_sigma;              /* curve_fit(absolute_sigma=True): pcov is returned unscaled instead of
                                            multiplied by 2 cost / (n_b - n_free) (scipy:_minpack_py.py:1057-1063) */
    double tr;                           /* repetition time, same unit as T1 */
    double tm;                           /* mixing time (STEAM) */
    double ftol;                         /* reference's tol (curvefit.py:304) */
    double xtol;                         /* SciPy default 1e-8 */
    double gtol;                         /* SciPy default 1e-8 */
    const double *sigma;                 /* NULL, or (n_b,) doubles on the HOST (also for the _f32 entry point): curve_fit's 1-D
                                            `sigma`, shared by all voxels -- the two keyword arguments the reference's solver
                                            names and forwards (curvefit.py:33, 295-306).  Residual and Jacobian rows are
                                            multiplied by 1 / sigma_i (_minpack_py.py:958-960, 545-562); cost is the weighted
                                            0.5 * sum.  A scalar sigma is n_b equal entries; a 2-D sigma (covariance matrix of
                                            the measurements) is not implemented */
    const int32_t *queue_order;          /* NULL, or n_vox int32 on the DEVICE, a permutation of 0 .. n_vox - 1 (PNX_MEM_DEVICE
                                            calls only, PNX_ERR_INVALID otherwise): the kernel's k-th queue pull fits voxel
                                            queue_order[k].  Results do not depend on the order (a voxel's arithmetic is its own);
                                            the run time does: a pass ends in the longest fits that were started last, so a caller
                                            with a predictor of the evaluation counts -- the nfev map of a previous fit of the
                                            same volume (refits, the second step of the reference's SegmentedFitter) or of the
                                            previous level of the IDEAL pyramid (fitters/ideal.py:150-190) -- passes them longest
                                            first (pnx_queue_order_f64 builds the permutation).  The array must stay valid until
                                            the call's work on `stream` has finished */
} pnx_curvefit_opts;

PNX_API int pnx_version(void);
/* Number of visible HIP devices (0 if none); never fails. */
PNX_API int pnx_device_count(void);
/* Copies the calling thread's last error message (NUL-terminated) into buf; returns its length. */
PNX_API int pnx_last_error(char *buf, int n);
/* Number of parameters of a model without the optional T1 parameter, or PNX_ERR_INVALID. */
PNX_API int pnx_model_n_params(int model);

/*
 * Device memory the library keeps between calls, per device: (i) PNX_MEM_HOST curve-fit calls keep one staging slab (the
 * volume's signal and results, up to PNX_STREAM_CACHE_MB, default 8192), a pinned control block and their streams for the next
 * call; (ii) the NNLS plans of the reference's regularised configurations share ONE set of slabs for the kernels behind their
 * first pass (1.55 GB, see pnx_nnls_plan_create), which stays allocated when the last plan is destroyed.
 * This frees both -- (i) unless such a call is running on the device (PNX_ERR_INVALID), (ii) unless a plan still exists.
 */
PNX_API int pnx_release_staging(int device);

/* order (n int32, device) = the voxel indices by descending key (n doubles, device), equal keys in index order: the queue order
 * for pnx_curvefit_opts::queue_order from a predicted evaluation count per voxel.  Synchronises `stream`. */
PNX_API int pnx_queue_order_f64(const double *key_device, int64_t n, int32_t *order_device, int device, void *stream);

/*
 * Batched bounded non-linear least squares, fp64, results matching SciPy 1.15 curve_fit(method="trf").
 * Replaces: CurveFitSolver._fit_data (curvefit.py:171-244) for all voxels at once.
 *
 *   b      (n_b,)                     host
 *   y      (n_vox, n_b) row-major     host|device    -- fitters/pixelwise.py:91-96 hands exactly this
 *   p0,lo,hi  (n_free,) host  or (n_free, n_vox) host|device when opts->per_voxel_p0_bounds
 *   fixed  (n_fixed,) host or (n_fixed, n_vox) host|device when opts->fixed_per_voxel; NULL if n_fixed==0
 *   popt   (n_free, n_vox)            out, host|device  (curvefit.py:235)
 *   pcov   (n_vox, n_free, n_free)    out or NULL       (curvefit.py:236-243; NaN on failure)
 *   status (n_vox) int8, nfev (n_vox) int32, cost (n_vox) = 0.5*sum(res^2): out, each may be NULL
 *          (PNX_MEM_DEVICE: status and cost are required when pcov is requested)
 */
PNX_API int pnx_curvefit_batch_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                           const double *p0, const double *lo, const double *hi, const double *fixed,
                           double *popt, double *pcov, int8_t *status, int32_t *nfev, double *cost,
                           int mem, int device, void *stream);

/*
 * The same fit with fp32 STORAGE: b, y, p0 / lo / hi, fixed in and popt, pcov, cost out are float; the arithmetic is
 * the fp64 of pnx_curvefit_batch_f64 (values are widened on the device, results narrowed there).  This is what the
 * reference computes for a float32 image -- curve_fit casts ydata to float64 (scipy:_minpack_py.py:930) -- without
 * the host-side float64 copy and with half the PCIe traffic.  SURVEY.md 8b: "T in {f32, f64} via suffix".
 */
PNX_API int pnx_curvefit_batch_f32(const pnx_curvefit_opts *opts, int64_t n_vox, const float *b, const float *y, const float *p0,
                           const float *lo, const float *hi, const float *fixed, float *popt, float *pcov,
                           int8_t *status, int32_t *nfev, float *cost, int mem, int device, void *stream);

/*
 * The same bounded TRF fit with fp32 ARITHMETIC: a second, independent kernel whose every operation of the iteration is float
 * (native v_exp_f32, half the registers per lane, two waves per SIMD).  Argument list of pnx_curvefit_batch_f32, float arrays
 * in and out; PNX_MEM_DEVICE only enqueues, PNX_MEM_HOST goes through the chunk ring.  Statuses, failure sentinels (popt = p0,
 * NaN pcov) and the meaning of max_nfev are those of pnx_curvefit_batch_f64.  Results are minima as good as float32 arithmetic
 * allows, NOT SciPy-parity results (measured agreement: DESIGN.md).  Differences from the fp64 fit:
 *   - analytic Jacobian only (SciPy's 2-point step of 1.5e-8 is below fp32 resolution);
 *   - tolerances below fp32 resolution cannot be honoured and are raised to floors (FLT_EPSILON = 2^-23 = 1.19e-7):
 *       ftol -> max(ftol, 4 FLT_EPSILON),  xtol -> max(xtol, FLT_EPSILON)  (a smaller step does not change a float);
 *     gtol is an ABSOLUTE test on the scaled gradient and has no floor that fits every signal amplitude: it is used as given --
 *     one below the gradient's rounding noise never fires and the fit ends through the tests above (a floor of 4 FLT_EPSILON
 *     was measured to stop noise-free unit-amplitude voxels 10 to 900 times the rounding cost above their minimum);
 *     besides SciPy's ftol test, a step whose predicted AND actual cost change both lie below
 *     ftol * cost + n_b (FLT_EPSILON max|y|)^2 / 8  (the second term is a quarter of the cost of fp32 rounding of the model
 *     itself) ends the fit with status 2 instead of shrinking the trust radius until xtol trips;
 *   - a start value on a bound is moved 8 FLT_EPSILON max(1, |bound|) inside (SciPy: 1e-10);
 *   - pcov drops singular values below FLT_EPSILON max(n_b, n_free) s_max (SciPy: the fp64 epsilon); the epilogue is fp64.
 * Not built, PNX_ERR_UNSUPPORTED with a message: fixed parameters (fixed must be NULL), the T1 / STEAM factor, sigma,
 * queue_order, PNX_JAC_FD.
 */
PNX_API int pnx_curvefit_fast_f32(const pnx_curvefit_opts *opts, int64_t n_vox, const float *b, const float *y, const float *p0,
                          const float *lo, const float *hi, const float *fixed, float *popt, float *pcov,
                          int8_t *status, int32_t *nfev, float *cost, int mem, int device, void *stream);

/*
 * The bounded fit with the volume-fraction constraint f1 + f2 <= 1 (the reference's ConstrainedCurveFitSolver, solvers/
 * constrained_curvefit.py):  minimise 0.5 ||model(p) - y||^2  subject to  lo <= p <= hi  and  f1 + f2 <= 1,  for the two reduced
 * tri-exponential layouts PNX_MODEL_TRI_REDUCED [f1, D1, f2, D2, D3] and PNX_MODEL_TRI_S0 [f1, D1, f2, D2, D3, S0] -- the models the
 * reference admits the constraint for; any other model is PNX_ERR_INVALID.  Not the reference's SLSQP iteration: the constrained
 * PROBLEM is solved by two box-bounded TRF fits and certified:
 *   1. pnx_curvefit_batch_f64's fit of every voxel.  A result with f1 + f2 <= 1 is a KKT point of the constrained problem with
 *      multiplier 0: it is returned as it is, covariance included (face = 0, lambda = 0), bit-identical to the box-only call.
 *   2. A voxel with status > 0 and f1 + f2 > 1 is fitted again on the face f1 + f2 = 1, which is the bi-exponential model
 *      (f3 = 0, D3 drops out): start f1 / (f1 + f2), D1, D2 (, S0), clipped into the bounds of f1 intersected with 1 - those of
 *      f2, [max(lo_f1, 1 - hi_f2), min(hi_f1, 1 - lo_f2)]; same Jacobian mode and tolerances; one evaluation limit per launch,
 *      max(1, max_nfev - the smallest phase-1 count among the launch's violators).
 *   3. Its result is written back as f1, D1, f2 = 1 - f1, D2, the phase-1 D3 (unidentifiable on the face), (S0); cost is
 *      evaluated there; nfev is the sum of both fits; status is the second fit's; pcov is NaN (J^T J is singular on the face, the
 *      reference's _estimate_covariance returns NaN for a singular matrix).  lambda = -(g_f1 + g_f2) / 2 from the gradient
 *      g = J^T r of the FULL model at that point is the multiplier of the constraint: face = 1 when lambda >= 0 (a KKT point of
 *      the constrained problem), 2 when lambda < 0 -- NOT certified: the box-only minimum was infeasible, yet the face point
 *      wants to move inwards.  A second fit that fails (empty intersection of the bounds: status -1) returns the usual sentinel
 *      popt = p0, NaN pcov, its status, with lambda = NaN and face = 2.
 * Arguments of pnx_curvefit_batch_f64, then lambda (n_vox) double and face (n_vox) int8, either may be NULL.  Host and device
 * memory.  PNX_MEM_DEVICE: the call synchronises `stream` ONCE, behind the first fit, to read the number of violators (it sizes
 * the second fit's scratch); when there are none nothing else runs, otherwise the rest is enqueued and the call returns.
 * PNX_MEM_HOST: the chunk ring, both fits per chunk (not the single streamed kernel of pnx_curvefit_batch_f64).
 * Not built, PNX_ERR_UNSUPPORTED with a message: fixed parameters (fixed must be NULL), the T1 / STEAM factor, sigma, queue_order.
 */
PNX_API int pnx_curvefit_simplex_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                             const double *p0, const double *lo, const double *hi, const double *fixed, double *popt,
                             double *pcov, int8_t *status, int32_t *nfev, double *cost, double *lambda, int8_t *face,
                             int mem, int device, void *stream);

/*
 * NNLS plan: everything that is shared by all voxels of one fit -- the regularised design matrix
 * A = [basis; reg] (nnls_solver.py:61-73) -- is uploaded and factored into its Gram form once.
 *   basis (n_meas, n_bins) row-major host;  reg (n_reg, n_bins) row-major host or NULL (n_reg = 0).
 * The plan picks the kernel; all of them walk the Lawson-Hanson path of scipy.optimize.nnls (same iteration counts):
 *   - reg = one of the reference's banded matrices (model_functions/nnls.py:46-85, orders 1-3) and n_meas <= 32 (every
 *     configuration the reference ships): basis resident in LDS, residual-form dual (csrc/pnx_nnls_blk.hip).  Its first
 *     instantiation holds 128 passive-set positions (twelve voxels in flight per CU); a voxel that wants more is solved again
 *     by a second instantiation with 256 positions (eight per CU) in one pass behind the call.  With a regulariser several
 *     times stronger than the reference's mu = 0.02 that concerns many voxels, so a call of >= 49 152 voxels solves a pilot of
 *     its first 12 288 and, when more than 15 % of those are handed over, the rest of the call goes to the second instantiation
 *     directly -- decided on the device, from the pilot's voxels only.  Device memory: a plan owns 0.2 GB of per-wave
 *     slabs (the first instantiation); the slabs of the two kernels behind it -- 0.55 GB the second instantiation, 1 GB the
 *     Gram-form kernel that remains the last resort -- exist ONCE per device and are shared by all such plans on it (N plans:
 *     1.55 + N x 0.2 GB; their uses are ordered on the device by events, calls stay asynchronous; pnx_release_staging frees the
 *     set once no plan is left).  Passive sets of up to 16 bins evaluate the dual in Gram form, w = A^T y - G[:, P] x_P (16 rows
 *     of G out of L2 instead of the 64 KB basis out of LDS), larger ones in residual form;
 *   - no regulariser / an all-zero one (reg_order = 0, the reference default): QR form (pnx_nnls_qr.hip) -- Q and R in LDS
 *     up to 32 measurements, in a per-wave global slab from 33 to 128 (264 KB per resident wave, allocated on the first
 *     solve of such a plan; up to round 3 more than 64 measurements were refused); the normal-equation kernel would pick other columns than SciPy on a rank-deficient basis, and
 *     this library never changes the algorithm silently;
 *   - anything else (dense regularisers, 33..128 measurements): Gram form (pnx_nnls.hip).
 * n_bins <= 512 (PNX_ERR_UNSUPPORTED beyond; the reference has no such limit, model_functions/nnls.py:37-77; up to round 3 the
 * limit was 256).  Up to 256 bins a lane of the wavefront that owns a voxel holds four bins, and every fast path is built on
 * that: the block kernel's LDS copy of the basis (32 x 258 doubles = 66 KB; at eight bins per lane 131 KB of a CU's 160 KB, two
 * voxels in flight per CU instead of twelve), the general kernel's 128 registers (sixteen waves per CU), the MFMA Gram step's
 * 256-column product.  257 .. 512 bins run on SEPARATE, SLOWER instantiations (a "wide" plan): the Gram-form kernel with six
 * (up to 384 bins) or eight bins per lane and the 256 passive-set positions of the narrow kernel (twelve waves per CU, A^T y
 * on the vector unit, no block kernel, no MFMA step; a voxel whose passive set wants a 257th position is handed to a
 * 512-position instantiation), and the QR-form kernels with a wider dual.  Same algorithm and decisions on the reference
 * fixtures g11_* and the oracle tests; NOT the same parity bar everywhere: a REGULARISED wide plan evaluates everything in Gram
 * form (condition number squared; the narrow plans' residual-form dual does not exist at eight bins per lane), and on random
 * ill-conditioned cases 2-3 % of them leave the oracle's path -- status flips at the iteration limit, coefficients off by up to
 * 1.5e-4 of the peak against the narrow plans' 1e-6 (profiles/r05_fuzz_nnls_wide.json: 7 of 200 cases; the listed cases are
 * the expected failures of `tests/fuzz_gpu_vs_oracle_nnls.py --wide`).  Measured on the C4 signal with 32 b-values: 3.4 M voxels/s at 300 bins, 2.7 M at
 * 384 and 1.7 M at 512 with the order-2 regulariser (10.3 M at 250 on 2^20 voxels: the step at 257 bins is a factor of 3), 8.8 M / 7.9 M
 * without (10.5 M at 250).
 * pnx_nnls_aty_f64 (the MFMA step on its own) stays a 256-column layout and refuses a wide plan.
 */
typedef struct pnx_nnls_plan pnx_nnls_plan;
PNX_API int pnx_nnls_plan_create(pnx_nnls_plan **plan, int n_meas, int n_bins, const double *basis, const double *reg,
                         int n_reg, int device);
PNX_API int pnx_nnls_plan_destroy(pnx_nnls_plan *plan);

/*
 * Batched NNLS  min ||A x - [y;0]||_2, x >= 0  per voxel, fp64, results matching scipy.optimize.nnls.
 * Replaces: NNLSSolver._fit_data (nnls_solver.py:129-180) incl. _extend_signal (never materialised).
 *   y (n_vox, n_meas) in;  coeff (n_vox, n_bins) out;  rnorm (n_vox) out = ||A x - y_ext||_2;
 *   status (n_vox) int8, iters (n_vox) int32: out, may be NULL.  max_iter: reference's max_iter
 *   (0 -> 3*n_bins like SciPy).
 */
PNX_API int pnx_nnls_solve_f64(pnx_nnls_plan *plan, int64_t n_vox, const double *y, int max_iter, double *coeff,
                       double *rnorm, int8_t *status, int32_t *iters, int mem, void *stream);
/* fp32 storage of y, coeff and rnorm, fp64 arithmetic (halves the 8.4 GB coefficient volume of the C4 workload). */
PNX_API int pnx_nnls_solve_f32(pnx_nnls_plan *plan, int64_t n_vox, const float *y, int max_iter, float *coeff, float *rnorm,
                       int8_t *status, int32_t *iters, int mem, void *stream);

/*
 * The MFMA Gram step of the NNLS path on its own: aty (n_vox, 256) = y (n_vox, n_meas) . basis (n_meas, n_bins),
 * columns >= n_bins zero (the layout the active-set kernel consumes).  n_bins <= 256, n_meas <= 64 (PNX_ERR_UNSUPPORTED otherwise).  Device pointers only; n_vox <= 2^20 per call.
 * This is the batched-GEMM part of what NNLSSolver._fit_single_pixel hands to scipy.optimize.nnls per voxel
 * (nnls_solver.py:195-197: A^T y of the normal equations); exposed so that it can be timed and checked by itself.
 */
PNX_API int pnx_nnls_aty_f64(pnx_nnls_plan *plan, int64_t n_vox, const double *y_dev, double *aty_dev, void *stream);

/* One-shot convenience: plan_create + solve + plan_destroy with host pointers. */
PNX_API int pnx_nnls_batch_f64(int64_t n_vox, int n_meas, int n_bins, const double *basis, const double *reg, int n_reg,
                       const double *y, int max_iter, double *coeff, double *rnorm, int8_t *status,
                       int32_t *iters, int device);

/*
 * Design-matrix builders (model_functions/nnls.py:17-85), host in / host out, computed on the device
 * in fp64 so that a host language without numpy can build the same matrices.
 */
PNX_API int pnx_nnls_bins(double d_min, double d_max, int n_bins, double *bins);
PNX_API int pnx_nnls_basis(int n_meas, const double *b, int n_bins, const double *bins, double *basis, int device);
PNX_API int pnx_nnls_regularization_matrix(int n_bins, int order, double mu, double *reg);

/*
 * NNLS spectrum post-processing on the device: what pyneapple.utility.spectrum does per voxel
 * (src/pyneapple/utility/spectrum.py:13-215) for all voxels at once.
 *   find_spectrum_peaks(spectrum, bins, height, regularized): scipy.signal.find_peaks(spectrum, height=height); fractions
 *     = peak heights, or -- regularized != 0 -- the Gaussian area height * FWHM / (2 sqrt(2 ln 2)) * sqrt(2 pi) with the FWHM
 *     of scipy.signal.peak_widths(rel_height) (calculate_peak_area); normalised to sum 1; d = bins[peak].
 *   apply_cutoffs(d, f, cutoffs): per range (lo, hi) no peak -> NaN, one -> kept, several -> geometric_mean_peak
 *     (log10 of the weighted geometric mean position -- the reference's own convention -- and the summed fraction);
 *     fractions renormalised over the ranges.
 *   spectrum (n_vox, n_bins) host|device, 3 <= n_bins <= 512; bins (n_bins,) host (up to 256 bins they travel in the kernel
 *     arguments, beyond in a stream-ordered device buffer: a device-mode call only enqueues either way); cutoffs (n_cut, 2) host.
 *   n_peaks (n_vox) int32: peaks found (may exceed max_peaks: the first max_peaks <= 64 are reported; a spectrum with more
 *     than 64 peaks -- 16 when it has a flat-topped rise, which takes SciPy's sequential scan on one lane -- gets NaN rows:
 *     its fractions would have to be normalised over peaks the table cannot hold; a 250-bin spectrum has at most 124 maxima);
 *   d_values / f_values (n_vox, max_peaks) NaN padded; d_cut / f_cut (n_vox, n_cut <= 8).  Outputs host|device as `mem`.
 */
PNX_API int pnx_nnls_spectrum_peaks_f64(int64_t n_vox, int n_bins, const double *spectrum, const double *bins_host, double height,
                                int regularized, double rel_height, int max_peaks, int32_t *n_peaks, double *d_values,
                                double *f_values, int n_cut, const double *cutoffs_host, double *d_cut, double *f_cut, int mem,
                                int device, void *stream);
/*
 * NNLS solve + spectrum post-processing in one call: the (n_vox, n_bins) spectra never leave the device (2 KB per voxel,
 * 8.4 GB for a 256 x 256 x 64 volume); per voxel only the peak table, the cutoff table, rnorm / status / iters come back.
 * Arguments as pnx_nnls_solve_f64 and pnx_nnls_spectrum_peaks_f64; y and every output host|device as `mem`.
 */
PNX_API int pnx_nnls_solve_peaks_f64(pnx_nnls_plan *plan, int64_t n_vox, const double *y, int max_iter, const double *bins_host,
                             double height, int regularized, double rel_height, int max_peaks, int32_t *n_peaks,
                             double *d_values, double *f_values, int n_cut, const double *cutoffs_host, double *d_cut,
                             double *f_cut, double *rnorm, int8_t *status, int32_t *iters, int mem, void *stream);
/*
 * The same call with the data-term residual of every voxel: solve -> ss_res -> peak table on the device while the chunk's spectra
 * are resident.  Every argument of pnx_nnls_solve_peaks_f64, in its order, then ss_res (n_vox,) host|device as `mem`, required:
 * 8 bytes per voxel of download instead of the 2 KB spectrum, so that R^2 exists on the peak-table path too.
 */
PNX_API int pnx_nnls_solve_peaks_stats_f64(pnx_nnls_plan *plan, int64_t n_vox, const double *y, int max_iter, const double *bins_host,
                                   double height, int regularized, double rel_height, int max_peaks, int32_t *n_peaks,
                                   double *d_values, double *f_values, int n_cut, const double *cutoffs_host, double *d_cut,
                                   double *f_cut, double *rnorm, int8_t *status, int32_t *iters, int mem, void *stream,
                                   double *ss_res);
/*
 * Prediction and data-term residual of a batch of spectra (what BaseFitter._compute_r_squared and predict do with
 * `coefficients @ basis.T`, fitters/base.py:90-186):  pred (n_vox, n_meas) = coeff . basis^T,
 * ss_res (n_vox,) = sum_j (y_ij - pred_ij)^2 over the plan's n_meas data rows -- NOT rnorm^2, which contains the regulariser rows.
 *   y (n_vox, n_meas), coeff (n_vox, n_bins) in; ss_res and pred out, either may be NULL but not both (y may be NULL when ss_res
 *   is); all host|device as `mem`; `device` must be the plan's.  The product runs on the fp64 matrix cores for every plan
 *   (any n_meas <= 128, n_bins <= 512); the plan is only read, so calls need no ordering against solves.
 */
PNX_API int pnx_nnls_fit_stats_f64(pnx_nnls_plan *plan, int64_t n_vox, const double *y, const double *coeff, double *ss_res,
                           double *pred, int mem, int device, void *stream);
/*
 * Forward model of the seven parametric layouts for all voxels (model.forward per voxel in the reference, fitters/base.py:90-131,
 * 142-186), at n_x <= PNX_MAX_BVALUES x-values that need not be the fitted b-values (PNX_ERR_INVALID beyond).
 *   opts: only model, n_free, n_fixed, free_idx, fixed_idx, fixed_per_voxel, t1_mode, tr, tm are read (n_b is ignored);
 *   x (n_x,) host; params (n_free, n_vox) parameter-major as popt of the fit; fixed (n_fixed,) host or (n_fixed, n_vox) as the fit
 *   takes it; y (n_vox, n_x) or NULL; pred (n_vox, n_x) or NULL; ss_res (n_vox,) = sum_i (pred_i - y_i)^2 or NULL (needs y);
 *   pred and ss_res may not both be NULL.  params, per-voxel fixed, y, pred, ss_res host|device as `mem`.
 *   The arithmetic is the fit's own (same exp, same operation order, same T1 / STEAM factor).
 */
PNX_API int pnx_curvefit_predict_f64(const pnx_curvefit_opts *opts, int64_t n_vox, int n_x, const double *x, const double *params,
                             const double *fixed, const double *y, double *pred, double *ss_res, int mem, int device,
                             void *stream);
/*
 * Per-voxel start values for the curve fit from a dictionary search.  The reference starts every voxel of a
 * volume from one p0; here every voxel is matched against n_atoms candidate parameter vectors ("atoms") and starts from the best:
 *   s_g = model(b; atom_g, fixed), evaluated by pnx_curvefit_predict_f64's kernel (the fit's own arithmetic: all seven layouts,
 *     shared fixed parameters, the T1 / STEAM factor); with opts->sigma rows and signals are multiplied by 1 / sigma_i, as the fit does;
 *   cost_g(v) = 0.5 (||y_v||^2 - 2 y_v . s_g + ||s_g||^2);  best[v] = the argmin over g, the lowest index among equal costs;
 *   p0_out[:, v] = atoms[:, best[v]], copied;  cost[v] = the cost of the chosen atom.
 * The product y . s_g runs on the fp64 matrix cores and never reaches memory: a voxel costs its signal row in and p0 / best / cost
 * out.  The cost is evaluated in the expanded form above: it carries the rounding of two dot products of n_b terms, at most
 * 4 n_b 2^-52 (||y||^2 + max_g ||s_g||^2), so two atoms whose costs differ by less than that may swap.
 * project_amplitude != 0: for the layouts with a free linear amplitude S0 (PNX_MODEL_MONO, PNX_MODEL_BI_S0, PNX_MODEL_TRI_S0;
 *   PNX_ERR_INVALID otherwise) the dictionary is built with S0 = 1 whatever the atoms' S0 row holds, and per voxel and atom
 *   a = clip(y . s_g / ||s_g||^2, lo_S0, hi_S0) (lo_S0 for an all-zero row),  cost_g = 0.5 (||y||^2 - 2 a y . s_g + a^2 ||s_g||^2);
 *   the chosen a is written into the S0 row of p0_out.  A small dictionary then serves signals of any amplitude.
 * A voxel with a non-finite (weighted) signal gets best = -1, cost = NaN and p0_out = atoms[:, 0]; the fit behind it reports its
 * usual status for it.  Its neighbours are not affected.
 *   opts: model, n_b, n_free, n_fixed, free_idx, fixed_idx, t1_mode, tr, tm, sigma are read;
 *   b (n_b,) host; y (n_vox, n_b) host|device; atoms (n_free, n_atoms) host, parameter-major like p0, 1 <= n_atoms <= 4096;
 *   fixed (n_fixed,) host or NULL; lo, hi (n_free,) host: every atom must lie inside them (the fit refuses a start value outside
 *   its bounds), PNX_ERR_INVALID names the first that does not;
 *   p0_out (n_free, n_vox), best (n_vox) int32 or NULL, cost (n_vox) or NULL: out, host|device as `mem`.
 * PNX_MEM_DEVICE only enqueues (the dictionary lives in a stream-ordered buffer); PNX_MEM_HOST goes through the chunk ring.
 * Not built, PNX_ERR_UNSUPPORTED with a message before any device work: per_voxel_p0_bounds, fixed_per_voxel, queue_order.
 */
PNX_API int pnx_curvefit_grid_start_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                double *p0_out, int32_t *best, double *cost, int mem, int device, void *stream);
/*
 * Posterior over a dictionary of parameter vectors: the Bayesian grid fit of noisy IVIM data.  The arguments,
 * the dictionary, the weighting, the (projected) amplitude a_g(v) and the cost c_g(v) are pnx_curvefit_grid_start_f64's, and so
 * are its refusals (per_voxel_p0_bounds, fixed_per_voxel, queue_order, projection without a free S0, an atom outside lo / hi).
 *   log_prior (n_atoms,) host or NULL (uniform): every entry finite or -inf, at least one finite (PNX_ERR_INVALID otherwise);
 *     an atom at -inf is excluded.
 *   noise_sd > 0: known Gaussian noise sd in the units of the (sigma-weighted) signal; == 0: the noise scale is marginalised under
 *     a Jeffreys prior; negative or non-finite: PNX_ERR_INVALID.
 * Per voxel v, in fp64, with tol_v = 4 n_b 2^-52 (||y_v||^2 + max_g ||s_g||^2), the rounding bound of the expanded cost:
 *   l_g = log_prior_g - c_g / noise_sd^2                      (known noise)
 *   l_g = log_prior_g - (nu / 2) log(max(c_g, tol_v))         (marginalised; nu = n_b, n_b - 1 with project_amplitude)
 *   L = log sum_g exp(l_g);  W_g = exp(l_g - L);  padded and excluded atoms have weight 0.
 *   mean[k] = sum_g W_g theta_kg, theta_kg = atoms[k, g], or a_g(v) in a projected S0 row;
 *   sd[k] = sqrt(max(0, sum_g W_g (theta_kg - mean[k])^2)), accumulated by a weighted Welford / Chan merge (no E[x^2] - mean^2);
 *   map_atom = argmax_g l_g, the lowest index among equal l;  map_p = that atom's parameters, copied (its S0 row holds a_g(v)
 *     under projection);  log_evidence = L - log sum_g exp(log_prior_g);  ess = (sum W)^2 / sum W^2 in [1, n_atoms].
 * A voxel with a non-finite (weighted) signal gets NaN in every floating output and map_atom = -1; its neighbours are not affected.
 *   mean, sd, map_p (n_free, n_vox); map_atom (n_vox) int32; log_evidence, ess (n_vox): out, host|device as `mem`; all but mean
 *   may be NULL.  PNX_MEM_DEVICE only enqueues; PNX_MEM_HOST goes through the chunk ring.  The (n_vox, n_atoms) matrix never
 *   reaches memory.
 */
PNX_API int pnx_curvefit_grid_posterior_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                    const double *atoms, const double *fixed, const double *lo, const double *hi,
                                    int project_amplitude, const double *log_prior, double noise_sd, double *mean, double *sd,
                                    int32_t *map_atom, double *map_p, double *log_evidence, double *ess, int mem, int device,
                                    void *stream);
/*
 * pnx_curvefit_grid_posterior_f64 under a Rician likelihood with a known noise sd, for magnitude data.  Its
 * arguments without project_amplitude; its dictionary, cost c_g(v), fold and outputs, term for term.  The signals are magnitudes
 * y_i >= 0 with y_i ~ Rice(s_gi, noise_sd).  With h(z) = log(exp(-z) I0(z)) (pnx_log_i0e_f64 below) and inv = 1 / noise_sd^2:
 *   z_vgi  = |(y_vi * s_gi) * inv|                          two multiplications in this order
 *   C_g(v) = sum_i h(z_vgi)                                 i = 0 .. n_b - 1 ascending, one chain of additions from 0
 *   l_g(v) = fma(-c_g(v), inv, log_prior_g) + C_g(v)        the first term is the Gaussian call's l_g (known noise), the same bytes
 * and everything behind l_g is that call's: L, W_g, mean, sd (Welford / Chan), map_atom, map_p, ess, excluded and padded atoms.
 *   log_evidence = (L - log sum_g exp(log_prior_g)) + K_v,  K_v = sum_i log(y_vi * inv), summed over i = kq, kq + 4, ... ascending for
 *     kq = 0 .. 3 into p_kq, then (p_kq + p_kq^1) + (p_kq^2 + p_kq^3) (the same value for every kq).
 *   That is log sum_g pi_g prod_i Rice(y_vi | s_gi, noise_sd) with pi the normalised prior: the Rice log-density is
 *   log(y / sd^2) - (y^2 + s^2) / (2 sd^2) + log I0(y s / sd^2) and log I0(z) = h(z) + z, so its sum over i is K_v - c_g / sd^2 + C_g.
 *   It is comparable between models, as the Gaussian one is.
 * The product y . s_g stays on the fp64 matrix cores; C_g(v) is not a matrix product and runs on the fp64 vector units between
 * the product and the fold.  The model values are taken as non-negative: a negative s_gi enters h through |z| only.
 * A voxel with a non-finite or a NEGATIVE signal entry gets NaN in every floating output and map_atom = -1; its neighbours are not
 * affected.  A zero entry is allowed: h(0) = 0, log_evidence is -inf and every other output stays finite.
 * PNX_ERR_INVALID before any device work: everything pnx_curvefit_grid_posterior_f64 refuses, and noise_sd <= 0 or non-finite (a
 * marginalised noise scale has no closed form under this likelihood).  PNX_ERR_UNSUPPORTED, by name: opts->sigma (per-b-value
 * weights: the Rice density has one sd).  The amplitude cannot be projected under this likelihood (the optimum has no closed form
 * and the likelihood is not Gaussian in it): a free S0 must sit on the grid as a row of `atoms`.
 * No floating-point atomics; the outputs are the same bytes from call to call and for PNX_MEM_HOST and PNX_MEM_DEVICE.
 */
PNX_API int pnx_curvefit_grid_posterior_rician_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                           int n_atoms, const double *atoms, const double *fixed, const double *lo, const double *hi,
                                           const double *log_prior, double noise_sd, double *mean, double *sd, int32_t *map_atom,
                                           double *map_p, double *log_evidence, double *ess, int mem, int device, void *stream);
/*
 * out[i] = h(z[i]) = log(exp(-z[i]) I0(z[i])), the log of the exponentially scaled modified Bessel function of order zero, one lane
 * per element (csrc/pnx_bessel.hpp: four polynomial pieces, split at 2, 4 and 8, the last behind -log(2 pi z) / 2).  Finite for
 * 0 <= z <= 1e300 with |error| <= 4.5 * 2^-52 max(|h|, 1); h(0) = 0; a negative or NaN input gives NaN.  z, out (n,) host|device.
 */
PNX_API int pnx_log_i0e_f64(int64_t n, const double *z, double *out, int mem, int device, void *stream);
/*
 * A second, fine grid per voxel and the posterior fold on it: resolution where a voxel's posterior sits, for a
 * caller that has a coarse posterior (pnx_curvefit_grid_posterior_f64) and forms a box around its mean.  No dictionary is shared:
 * every voxel builds its own atoms from its centre and half-width.  opts, n_vox, b, y, fixed, lo, hi, project_amplitude as the
 * posterior call takes them; noise_sd > 0: known noise, <= 0: marginalised (Jeffreys), non-finite: PNX_ERR_INVALID.
 *   n_points (n_free,) int32 host, each in [1, 9]; their product, the most atoms a voxel can have, at most 4096; 1 on a projected S0 row;
 *   centre, half_width (n_free, n_vox) host|device as `mem` (the rows of a projected S0 are not read).
 * Per voxel v, in fp64, in this order:
 *   axis of free row k (m = n_points[k], c = centre[k, v], h = half_width[k, v]):
 *     a = max(lo_k, c - h), b = min(hi_k, c + h);  m == 1 or not (b > a): the single value min(max(c, lo_k), hi_k);
 *     else step = (b - a) / (m - 1), x_j = fma(j, step, a) for j < m - 1 and x_{m-1} = b (no value leaves [lo_k, hi_k]).
 *     A fixed parameter is an axis of its one value; a projected S0 is an axis of the value 1.
 *   atoms: the Cartesian product of the axes in the model's parameter order, the first row slowest; index g counts them.
 *   admitted atoms (the fraction-sum rule): the implied last fraction of a reduced layout may not be negative -- f1 <= 1 for
 *     [f1, D1, D2 (, S0)], f1 + f2 <= 1 (one addition) for [f1, D1, f2, D2, D3 (, S0)], fixed fractions included; every atom of the
 *     other layouts is admitted.  This is the feasible set of pnx_curvefit_simplex_f64.  The coarse grid builders admit whatever
 *     lies inside lo / hi, so a box around a coarse mean can reach across the face f1 + f2 = 1 even where no coarse atom does; the
 *     atoms beyond it are dropped here.  The prior is uniform over the admitted atoms.
 *   s_gi = model(b_i; atom_g) with E = exp(-b_i x) taken from a per-voxel table of the rate axes (the fit's own exp and argument);
 *   project_amplitude: dot = sum_i fma(y_i, s_gi, .), nrm = sum_i fma(s_gi, s_gi, .), i ascending, with S0 = 1;
 *     a_g = min(max(dot / nrm, lo_S0), hi_S0), lo_S0 when nrm == 0;  d_i = fma(-a_g, s_gi, y_i);   otherwise d_i = y_i - s_gi;
 *   c_g = 0.5 * sum_i fma(d_i, d_i, .), i ascending from 0: the DIRECT cost.  The expanded form 1/2 ||y||^2 - y . s + 1/2 ||s||^2 is not
 *     used: its cancellation term is what a fine grid at high SNR would run into.
 *   l_g = -c_g / noise_sd^2  (known noise);   l_g = -(nu / 2) log(max(c_g, tol_v))  (marginalised; nu = n_b, n_b - 1 with projection;
 *     tol_v = max(4 n_b 2^-52 ||y_v||^2, 2^-1022), a floor against log 0 only: the direct cost has no cancellation to bound);
 *   the fold is the posterior call's: each of 64 lanes takes the atoms g = lane, lane + 64, ... through a running log-sum-exp and
 *     weighted Welford moments about the clipped centre, then a Chan merge over the lanes (xor 32, 16, ..., 1).
 *   mean, sd, map_p (the values of the atom with the largest l, the lowest index among equals; a_g in a projected S0 row), ess as
 *     the posterior call; log_norm = L - log(number of admitted atoms): the log of the MEAN weight over the voxel's own atoms -- a local
 *     normaliser, NOT an evidence (the box differs from voxel to voxel and from level to level);
 *   edge_mass[k] = sum of W_g over the atoms on the first or last value of row k, 0 for a one-value row: near 0 the box holds the
 *     posterior, large values say the box truncates it.
 * A voxel with a non-finite signal, a non-finite centre or half-width, or a negative half-width gets NaN in every output, and so
 * does a voxel none of whose atoms is admitted; its neighbours are not affected.  An atom whose cost overflows has l = -inf and
 * weight 0; when that holds for every admitted atom of a voxel (a finite but enormous signal under known noise) the weights are
 * equal: log_norm = -inf, ess = the number of admitted atoms, mean and sd those of the uniform distribution over them, map_p the
 *   first admitted atom.
 *   mean, sd, map_p, edge_mass (n_free, n_vox); ess, log_norm (n_vox): out, host|device as `mem`; all but mean may be NULL.
 * PNX_ERR_INVALID before any device work: n_points outside [1, 9] or spanning more than 4096 atoms, more than one point on a
 * projected S0 row, bounds that are not finite with lo <= hi, a NULL pointer, projection without a free S0.  PNX_ERR_UNSUPPORTED, by
 * name: opts->sigma, the T1 / STEAM factor (t1_mode: T1 would need a table of its own), per_voxel_p0_bounds, fixed_per_voxel, queue_order.
 * No floating-point atomics; the outputs are the same bytes from call to call and for PNX_MEM_HOST and PNX_MEM_DEVICE.
 */
PNX_API int pnx_curvefit_grid_refine_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y, const double *fixed,
                                 const double *lo, const double *hi, int project_amplitude, double noise_sd, const int32_t *n_points,
                                 const double *centre, const double *half_width, double *mean, double *sd, double *map_p, double *ess,
                                 double *log_norm, double *edge_mass, int mem, int device, void *stream);
/*
 * The prior of pnx_curvefit_grid_posterior_f64 learned from the volume itself (empirical Bayes): the
 * non-parametric maximum-likelihood mixture over the dictionary, by EM.  The arguments up to noise_sd, the weighting, the refusals
 * and l_g are pnx_curvefit_grid_posterior_f64's.  With pi the current prior (log_prior_g = log pi_g inside l_g), one update is
 *   L_v = log sum_g exp(l_g(v));  W_vg = exp(l_g(v) - L_v);  S_g = sum over the finite voxels of W_vg;
 *   pi_g <- (S_g + pseudo_count) / (n_eff + pseudo_count n_adm)        n_adm: the atoms the start prior admits (finite entries)
 * and log_prior_g <- log pi_g, -inf where pi_g == 0 and always -inf for an atom that started at -inf.  The (n_vox, n_atoms) matrix
 * W never reaches memory; no sum uses an atomic, so a call is reproducible bit for bit on a given device.
 *   log_prior (n_atoms,) host or NULL (uniform): the start, as the posterior takes it; it is normalised first,
 *     log_prior - log sum exp(log_prior), and every reported prior sums to 1 over its finite entries -- so the sum of log_evidence
 *     of a later posterior call under log_prior_out is the last entry of the trace;
 *   n_iter in [1, 1000]: the most updates; pseudo_count finite, >= 0; rel_tol finite, >= 0 (PNX_ERR_INVALID otherwise, with a
 *     message, before any device work);
 *   log_prior_out (n_atoms,) host, not NULL: the prior after `done` updates;
 *   loglik (n_iter + 1,) host or NULL: loglik[t] = sum over the finite voxels of L_v under the prior BEFORE update t, t = 0 .. done;
 *     loglik[done] belongs to the returned prior (one more normaliser pass); entries past `done` are NaN;
 *   n_iter_done: `done`.  After update t >= 1 the call stops when loglik[t] - loglik[t-1] <= rel_tol |loglik[t]|; rel_tol = 0 runs
 *     all n_iter updates;
 *   n_eff: the number of voxels with a finite (weighted) signal; the others take no part.  Without one the call returns PNX_OK
 *     with the normalised start prior, done = 0 and loglik[0] = 0.
 * The prior is learned from the voxels it will be applied to: it needs many more voxels than atoms carry weight, and a few dozen
 * voxels over-fit.
 *   y (n_vox, n_b) host|device as `mem`.  PNX_MEM_DEVICE: read in place.  PNX_MEM_HOST: uploaded once (pnx_upload's path) into a
 *   stream-ordered buffer that stays for all iterations -- every pass reads the same signals, so there is no chunk ring;
 *   PNX_ERR_NOMEM names the size and points to a sub-sample.  The outputs are small host arrays: for both `mem` values the call
 *   SYNCHRONISES `stream` before it returns (once per iteration, for 16 bytes, and at the end).
 */
PNX_API int pnx_curvefit_grid_prior_em_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                   const double *atoms, const double *fixed, const double *lo, const double *hi,
                                   int project_amplitude, const double *log_prior, double noise_sd, int n_iter, double pseudo_count,
                                   double rel_tol, double *log_prior_out, double *loglik, int *n_iter_done, int64_t *n_eff, int mem,
                                   int device, void *stream);
/*
 * pnx_curvefit_grid_posterior_f64 with one prior row per segmentation label.  Every argument of that call, its
 * weighting, refusals and outputs, and
 *   n_classes in [1, 16] (PNX_ERR_INVALID otherwise);
 *   labels (n_vox,) int32, host|device as `mem`: the row of the table voxel v is judged under;
 *   log_prior (n_classes, n_atoms) row-major, host, or NULL (every row uniform): every entry finite or -inf; rows may exclude
 *     different atoms; every row needs at least one finite entry -- otherwise PNX_ERR_INVALID with a message that names the row,
 *     before any device work.
 * Per voxel v, with c = labels[v]:
 *   l_g(v) = log_prior[c, g] - ...           everything right of the prior term is pnx_curvefit_grid_posterior_f64's, term for term;
 *   log_evidence_v = L_v - log sum_g exp(log_prior[c, g]);  a pair whose table entry is -inf has weight exactly 0.
 * Labels may live on the device and are not validated on the host: a voxel whose label lies outside [0, n_classes) is treated
 * exactly as a voxel with a non-finite signal -- NaN in every floating output, map_atom = -1 -- and its neighbours are
 * bit-identical to a run without it.  This is how a caller marks background (label -1).
 * Every sum of a voxel depends on the order of the atoms only: a voxel's outputs are the bytes pnx_curvefit_grid_posterior_f64
 * returns for it under log_prior[c, :] whenever the rows admit the same atoms (the moments are accumulated about the mid-range of
 * the atoms that ANY row admits; with rows that exclude different atoms mean and sd agree within the posterior's rounding bound
 * taken over that range).  With n_classes == 1 and every label 0 the call returns the unlabelled call's bytes.
 * PNX_MEM_DEVICE only enqueues; PNX_MEM_HOST goes through the chunk ring, the labels beside the signals.
 */
PNX_API int pnx_curvefit_grid_posterior_classes_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                    int n_atoms, const double *atoms, const double *fixed, const double *lo, const double *hi,
                                    int project_amplitude, int n_classes, const int32_t *labels, const double *log_prior,
                                    double noise_sd, double *mean, double *sd, int32_t *map_atom, double *map_p, double *log_evidence,
                                    double *ess, int mem, int device, void *stream);
/*
 * pnx_curvefit_grid_prior_em_f64 with one prior row per segmentation label, all rows learned in one pass pair over the volume
 * (DESIGN.md 4.1n).  n_classes, labels and log_prior (n_classes, n_atoms) as pnx_curvefit_grid_posterior_classes_f64 takes
 * them, with its l_g, its refusals and its rule for a label outside [0, n_classes): such a voxel takes no part.  Every row of the
 * start is normalised first.  One update, per class c:
 *   S_cg = sum of W_vg over the voxels of class c that take part (finite signal, label in range);
 *   pi_cg <- (S_cg + pseudo_count) / (n_eff_c + pseudo_count n_adm_c)      n_adm_c: the finite entries of row c of the start
 * and log_prior[c, g] <- log pi_cg; an entry that started at -inf stays there; a class without a voxel that takes part keeps its
 * normalised start row.
 *   log_prior_out (n_classes, n_atoms) host, not NULL;
 *   loglik (n_iter + 1,) host or NULL: the sum over the classes, in class order, of
 *   loglik_class (n_iter + 1, n_classes) host or NULL: per class the sum of L_v over its voxels that take part, under the table
 *     before update t; entries past `done` are NaN in both;
 *   n_iter_done: `done`; the stopping rule is pnx_curvefit_grid_prior_em_f64's, applied to loglik (the sum);
 *   n_eff (n_classes,) int64 host or NULL: per class the voxels that take part.  Without any the call returns PNX_OK with the
 *     normalised start, done = 0 and loglik[0] = 0.
 * No floating-point atomics; every sum has one order for a given launch grid: two calls return the same bytes, PNX_MEM_HOST or
 * PNX_MEM_DEVICE; the (n_vox, n_atoms) matrix W never reaches memory.  With n_classes == 1 and every label 0 the call returns the
 * bytes of pnx_curvefit_grid_prior_em_f64.  The accumulate pass separates the classes that meet in a strip of 16 voxels in a
 * loop over the classes present there: a label map sorted by class pays for one class per strip (DESIGN.md 4.1n has the cost).
 *   y, labels host|device as `mem`; PNX_MEM_HOST uploads both once for all iterations (no chunk ring; PNX_ERR_NOMEM names the
 *   size).  For both `mem` values the call SYNCHRONISES `stream` before it returns.
 */
PNX_API int pnx_curvefit_grid_prior_em_classes_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                   int n_atoms, const double *atoms, const double *fixed, const double *lo, const double *hi,
                                   int project_amplitude, int n_classes, const int32_t *labels, const double *log_prior,
                                   double noise_sd, int n_iter, double pseudo_count, double rel_tol, double *log_prior_out,
                                   double *loglik, double *loglik_class, int *n_iter_done, int64_t *n_eff, int mem, int device,
                                   void *stream);
/*
 * A neighbourhood (MRF) prior for pnx_curvefit_grid_posterior_f64 by coloured mean-field sweeps: three calls,
 * the gather, one colour update, and the driver that composes them.  Over a symmetric neighbour graph of the voxels and with a
 * precision lambda_k >= 0 per free parameter the prior is
 *   p(theta) ~ prod_v pi(theta_v) exp(-1/2 sum_{edges (u,v)} sum_k lambda_k (theta_vk - theta_uk)^2),
 * and mean field with q = prod_v q_v over the atoms updates one voxel, its neighbours held fixed, by
 *   l_g(v) = [pnx_curvefit_grid_posterior_f64's l_g(v), term for term] + sum_k thetac_kg q_vk - 1/2 n_v r_g
 *   thetac_kg = atoms[k, g] - centre_k     centre_k: the posterior's own centre, min + (max - min) / 2 over the admissible atoms,
 *                                          0 for a projected S0 row
 *   q_vk = lambda_k sum_{u in N(v), present} (mean[k, u] - centre_k)       summed in slot order, then one multiply
 *   n_v = the number of present neighbours;  r_g = sum_k lambda_k thetac_kg^2   (host, fp64, k ascending)
 * A neighbour is present when its slot holds an index >= 0 and mean[0, u] is finite; a voxel with a non-finite signal is NaN in
 * every output, as in the posterior, and so counts for nobody.  The neighbours' variances are constant in theta_v and drop out.
 * The centred form matters: uncentred, a narrow axis far from zero cancels catastrophically.
 *
 * pnx_curvefit_grid_neighbour_field_f64: the gather.  One lane per voxel of [first, first + count).
 *   n_vox in [0, 2^31 - 1]; n_free in [1, 8]; n_nb in [1, 8];
 *   neighbours (n_vox, n_nb) int32, -1 where a slot is empty; mean (n_free, n_vox): host|device as `mem`;
 *   centre, precision (n_free,) host: finite, precision >= 0;
 *   field_q (n_free, n_vox), field_n (n_vox) int32: out, host|device as `mem`, written for the range only;
 *   flag: an index outside [-1, n_vox) is never dereferenced (the slot counts as empty); it is an argument error.
 *     PNX_MEM_DEVICE only enqueues and cannot report: flag is a device int32 or NULL, which the caller sets to INT32_MAX and which
 *     receives (integer atomicMin) the lowest voxel of the range with such an index -- the call that synchronises reports it, as
 *     pnx_curvefit_grid_posterior_mrf_f64 does.  PNX_MEM_HOST uploads the table and the means, synchronises `stream` and returns
 *     PNX_ERR_INVALID naming that voxel; flag is then a host int32 or NULL.
 */
PNX_API int pnx_curvefit_grid_neighbour_field_f64(int64_t n_vox, int64_t first, int64_t count, int n_free, int n_nb,
                                   const int32_t *neighbours, const double *mean, const double *centre, const double *precision,
                                   double *field_q, int32_t *field_n, int32_t *flag, int mem, int device, void *stream);
/*
 * pnx_curvefit_grid_posterior_field_f64: one colour update.  Every argument of pnx_curvefit_grid_posterior_f64, its weighting,
 * refusals and outputs, for the voxels [first, first + count) under the l_g above, written IN PLACE into the full-length output
 * arrays (n_free, n_vox) / (n_vox); the other voxels' entries are not touched.
 *   field_q (n_free, n_vox), field_n (n_vox) int32: device, as the gather wrote them (only the range is read);
 *   precision (n_free,) host: finite, >= 0, and 0 on a projected S0 row, which has no grid value (PNX_ERR_INVALID otherwise);
 *   delta_max: device scalar or NULL; receives max over { k: precision_k > 0 and range_k > 0; v in the range, finite } of
 *     |mean_new[k, v] - mean_old[k, v]| / range_k,  range_k = max_g theta_kg - min_g theta_kg over the admissible atoms.  Each lane
 *     reads its old mean before it overwrites it; the maximum is reduced per block and then over the blocks by a small kernel:
 *     no floating-point atomics.  0 for an empty range.
 * With field_q = 0 and field_n = 0 the added terms are exactly +0.0 and the call returns the bytes of
 * pnx_curvefit_grid_posterior_f64 for those voxels; with every precision 0 the field is not read and the same holds.
 * log_evidence is L_v - log sum_g exp(log_prior_g) with the field inside L_v: a LOCAL NORMALISER of the voxel's update given its
 * neighbours, not a model evidence -- do not sum it over voxels or compare it between models.
 * A pair at log_prior = -inf is skipped before any arithmetic.  The field product runs on the fp64 matrix cores in an accumulator
 * of its own (adding it to y . s would be wrong outside known noise without projection).  PNX_MEM_DEVICE only (PNX_ERR_INVALID
 * otherwise); the call only enqueues.
 */
PNX_API int pnx_curvefit_grid_posterior_field_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                   int n_atoms, const double *atoms, const double *fixed, const double *lo, const double *hi,
                                   int project_amplitude, const double *log_prior, double noise_sd, int64_t first, int64_t count,
                                   const double *field_q, const int32_t *field_n, const double *precision, double *mean, double *sd,
                                   int32_t *map_atom, double *map_p, double *log_evidence, double *ess, double *delta_max, int mem,
                                   int device, void *stream);
/*
 * pnx_curvefit_grid_posterior_mrf_f64: the driver.  The arguments and outputs of pnx_curvefit_grid_posterior_f64, and
 *   n_nb in [1, 8]; neighbours (n_vox, n_nb) int32, host|device as `mem`; the graph must be symmetric (not checked);
 *   n_colours in [1, 8]; colour_start (n_colours + 1,) int64 host, ascending from 0 to n_vox: the voxels of colour c are the
 *     contiguous range [colour_start[c], colour_start[c+1]) -- the caller sorts the voxels by colour; a colour may be empty;
 *   precision (n_free,) host; n_sweeps in [0, 100]; tol finite, >= 0;
 *   delta (n_sweeps,) host or NULL; n_sweeps_done host or NULL.
 * Sweep 0 is the plain posterior on all voxels (the bytes of pnx_curvefit_grid_posterior_f64).  Sweep s = 1 .. n_sweeps runs, for
 * each colour in order, the gather and then the field posterior on that colour's range.  No voxel of a colour has a neighbour in
 * it, so colour after colour is coordinate ascent on the variational free energy, which never decreases; a simultaneous update
 * of all voxels would not be monotone.  delta[s-1] is the maximum of delta_max over the sweep's colour updates; the call stops
 * after sweep s when delta[s-1] <= tol (tol = 0 runs all sweeps, without a host round trip per sweep); entries of delta past
 * n_sweeps_done are NaN.  log_evidence is the local normaliser described above.
 * A small kernel verifies the table before any sweep: an index outside [-1, n_vox), or a neighbour of a voxel inside the voxel's
 * own colour range, returns PNX_ERR_INVALID and names the first offending voxel.  Refused before any device work: everything the
 * posterior refuses; n_nb, n_colours, n_sweeps or tol out of range; colour_start not ascending from 0 to n_vox; a negative or
 * non-finite precision; a positive precision on a projected S0 row.
 * Every sum of a voxel depends on the order of the atoms and of its slots only: two calls return the same bytes, PNX_MEM_HOST or
 * PNX_MEM_DEVICE, and the call returns the bytes of the same sequence composed from the three calls above.
 *   PNX_MEM_HOST: y and neighbours are uploaded once (pnx_upload's path) and the outputs come back from one stream-ordered
 *   buffer, as pnx_curvefit_grid_prior_em_f64 stages its signals -- no chunk ring; PNX_ERR_NOMEM names the size.  For both `mem`
 *   values the call SYNCHRONISES `stream` before it returns.
 */
PNX_API int pnx_curvefit_grid_posterior_mrf_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                   int n_atoms, const double *atoms, const double *fixed, const double *lo, const double *hi,
                                   int project_amplitude, const double *log_prior, double noise_sd, int n_nb, const int32_t *neighbours,
                                   int n_colours, const int64_t *colour_start, const double *precision, int n_sweeps, double tol,
                                   double *mean, double *sd, int32_t *map_atom, double *map_p, double *log_evidence, double *ess,
                                   double *delta, int *n_sweeps_done, int mem, int device, void *stream);
/*
 * An edge-preserving neighbourhood prior for pnx_curvefit_grid_posterior_f64: the Gaussian pair potential above
 * replaced by a multivariate Student-t with dof = nu > 0 degrees of freedom, written as a Gaussian scale mixture with one latent
 * precision tau_uv per undirected edge,
 *   p(theta, tau) ~ prod_v pi(theta_v) prod_{edges} Gamma(tau_uv; nu/2, nu/2) tau_uv^{K/2} exp(-1/2 tau_uv sum_k lambda_k (theta_vk - theta_uk)^2),
 * K the number of rows with lambda_k > 0.  Mean field with q = prod_v q_v prod_edges q(tau_uv) keeps the voxel update above with
 * every neighbour weighted by w_uv = E[tau_uv] and the count n_v replaced by the weight sum W_v:
 *   s_uv = sum_k lambda_k (sd[k, v]^2 + sd[k, u]^2 + (mean[k, v] - mean[k, u])^2)     rows with lambda_k = 0 skipped
 *   w_uv = (nu + K) / (nu + s_uv)
 *   q_vk = lambda_k sum_{u in N(v), present} w_uv (mean[k, u] - centre_k);   W_v = sum_{u present} w_uv
 *   l_g(v) = [pnx_curvefit_grid_posterior_f64's l_g(v)] + sum_k thetac_kg q_vk - 1/2 W_v r_g
 * nu -> infinity is the Gaussian prior (w = 1, W_v = n_v).  The weights are computed on the fly from the current moments in the
 * gather of every colour update and never stored, which is exact coordinate ascent on the free energy of DESIGN.md 4.1s.
 *
 * pnx_curvefit_grid_neighbour_wfield_f64: the weighted gather.  The arguments of pnx_curvefit_grid_neighbour_field_f64, and
 *   sd (n_free, n_vox): host|device as `mem`; dof: finite, > 0 (PNX_ERR_INVALID otherwise);
 *   field_w (n_vox) double, field_n (n_vox) int32 (the present count): out, written for the range only, as field_q;
 *   edge_weight (n_vox, n_nb) double or NULL: w_uv per slot, 0 in a slot that is not present; written for the range only.
 * The order of operations per voxel v, in fp64 (fma: one rounding):
 *   a voxel whose own mean[0, v] is non-finite gets q = 0, W = 0, n = 0 and every edge_weight 0;
 *   per present slot, in slot order:  s = 0;  for k ascending with lambda_k > 0:
 *       t = fma(sd[k,u], sd[k,u], sd[k,v] * sd[k,v]);  d = mean[k,v] - mean[k,u];  s = fma(lambda_k, fma(d, d, t), s);
 *     w = (nu + K) / (nu + s)   (nu + K rounded once on the host);  W += w;  acc_k = fma(w, mean[k,u] - centre_k, acc_k) for every k;
 *   q_vk = lambda_k * acc_k.
 * Every index is checked before it is dereferenced and reported through `flag` as the Gaussian gather does; no floating-point
 * atomics.  Beside the Gaussian gather's reads (the table, n_free means per present neighbour) it reads the sd of the neighbour's
 * rows with lambda_k > 0 and the voxel's own mean and sd of those rows: at most (2 n_nb + 2) / n_nb of the Gaussian gather's
 * moment bytes, twice plus the voxel's own row.
 */
PNX_API int pnx_curvefit_grid_neighbour_wfield_f64(int64_t n_vox, int64_t first, int64_t count, int n_free, int n_nb,
                                   const int32_t *neighbours, const double *mean, const double *sd, const double *centre,
                                   const double *precision, double dof, double *field_q, double *field_w, int32_t *field_n,
                                   double *edge_weight, int32_t *flag, int mem, int device, void *stream);
/*
 * pnx_curvefit_grid_posterior_wfield_f64: one colour update with a real weight.  pnx_curvefit_grid_posterior_field_f64 with
 * field_w (n_vox) double, device, in field_n's place: l = l0 + fma(-1/2 W_v, r_g, fld), W_v / 2 held in doubles.  With
 * field_w = (double) field_n it returns the bytes of pnx_curvefit_grid_posterior_field_f64; with field_q = 0 and field_w = 0, or
 * every precision 0 (the field is then not read), those of pnx_curvefit_grid_posterior_f64.  Everything else -- refusals, delta_max,
 * the local normaliser, PNX_MEM_DEVICE only -- is that call's.
 */
PNX_API int pnx_curvefit_grid_posterior_wfield_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                   int n_atoms, const double *atoms, const double *fixed, const double *lo, const double *hi,
                                   int project_amplitude, const double *log_prior, double noise_sd, int64_t first, int64_t count,
                                   const double *field_q, const double *field_w, const double *precision, double *mean, double *sd,
                                   int32_t *map_atom, double *map_p, double *log_evidence, double *ess, double *delta_max, int mem,
                                   int device, void *stream);
/*
 * pnx_curvefit_grid_posterior_tmrf_f64: the driver.  pnx_curvefit_grid_posterior_mrf_f64 with dof behind precision, sd REQUIRED
 * (the weights need the variances), and two optional outputs in front of delta:
 *   field_w (n_vox) double, field_n (n_vox) int32, host|device as `mem`, or NULL: W_v and the present count of every voxel at its
 *     last update; 0 for a voxel that no sweep updated (n_sweeps = 0, an empty colour).
 * Sweep 0 is the plain posterior; sweep s runs, for each colour in order, the weighted gather and then the weighted field
 * posterior on that colour's range.  delta, tol, the colour check, the staging of PNX_MEM_HOST and the synchronisation are the
 * Gaussian driver's, and the call returns the bytes of the same sequence composed from the calls above.  Refused with
 * PNX_ERR_INVALID before any device work: a non-finite or non-positive dof, a NULL sd, and everything the Gaussian driver refuses.
 * With every precision 0 (K = 0) the result is the plain posterior's bytes.
 */
PNX_API int pnx_curvefit_grid_posterior_tmrf_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                   int n_atoms, const double *atoms, const double *fixed, const double *lo, const double *hi,
                                   int project_amplitude, const double *log_prior, double noise_sd, int n_nb, const int32_t *neighbours,
                                   int n_colours, const int64_t *colour_start, const double *precision, double dof, int n_sweeps,
                                   double tol, double *mean, double *sd, int32_t *map_atom, double *map_p, double *log_evidence,
                                   double *ess, double *field_w, int32_t *field_n, double *delta, int *n_sweeps_done, int mem,
                                   int device, void *stream);
/*
 * Marginal posterior of every free parameter over the dictionary, and credible-interval quantiles from it.  The
 * arguments up to noise_sd, the weighting, the dictionary, a_g(v), c_g(v), tol_v, l_g and every refusal are
 * pnx_curvefit_grid_posterior_f64's.  The atoms sit on a grid: along free parameter k every atom holds one of n_bins[k] values.
 *   n_bins (n_free,) int32 host: the number of distinct grid values of each free parameter; 0: no marginal for that parameter.
 *     B = sum n_bins must lie in [1, 128]; under project_amplitude the S0 row must hold 0 (its value is a_g(v), not a grid value);
 *   bin_of (n_free, n_atoms) int32 host: the bin of atom g along parameter k, in [0, n_bins[k]); rows with n_bins[k] == 0 are
 *     not read;
 *   bin_value (B,) host: the grid value of every bin, parameter k's at offset off_k = sum_{i<k} n_bins[i], strictly ascending within
 *     a parameter; every atom must satisfy atoms[k, g] == bin_value[off_k + bin_of[k, g]] exactly;
 *   n_q in [0, 8], probs (n_q,) host, each in the open interval (0, 1).
 * Every violation is PNX_ERR_INVALID with a message that names the first offender, before any device work.
 * Per finite voxel v, in fp64:  L = log sum_g exp(l_g);  W_g = exp(l_g - L), exactly 0 for a padded or excluded atom;
 *   marginal[off_k + j, v] = sum over the atoms with bin_of[k, g] == j of W_g      (not renormalised afterwards)
 *   cdf_j = the running sum of marginal over j in bin order;  quantile[i, k, v] = bin_value of the first bin with
 *     cdf_j >= probs[i], of the last bin of k when none reaches it (no interpolation), NaN for a parameter with n_bins[k] == 0;
 *   log_evidence = L - log sum_g exp(log_prior_g), the posterior's (from the normaliser pass: equal within its rounding bound).
 * A voxel with a non-finite (weighted) signal gets NaN in every output; its neighbours are not affected.
 *   marginal (B, n_vox) bin-major, not NULL; quantile (n_q, n_free, n_vox), NULL only when n_q == 0; log_evidence (n_vox) or NULL:
 *   out, host|device as `mem`.
 * Two passes over the product y_v . s_g (the normaliser of pnx_curvefit_grid_prior_em_f64, then the weights times a 0/1 indicator
 * matrix on the matrix cores); the (n_vox, n_atoms) matrix W never reaches memory.  No sum uses an atomic and every sum of a voxel
 * depends on the order of the atoms only: results are bit-identical between two calls, between PNX_MEM_HOST and PNX_MEM_DEVICE,
 * and whatever the number of voxels in the call.
 *   PNX_MEM_DEVICE only enqueues.  PNX_MEM_HOST: y is uploaded once (pnx_upload's path) and the outputs come back from one
 *   stream-ordered buffer (pnx_download's path), as pnx_curvefit_grid_prior_em_f64 stages its signals -- no chunk ring;
 *   PNX_ERR_NOMEM names the sizes.
 */
PNX_API int pnx_curvefit_grid_marginals_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                    const double *atoms, const double *fixed, const double *lo, const double *hi,
                                    int project_amplitude, const double *log_prior, double noise_sd, const int32_t *n_bins,
                                    const int32_t *bin_of, const double *bin_value, int n_q, const double *probs, double *marginal,
                                    double *quantile, double *log_evidence, int mem, int device, void *stream);
/*
 * Variable-projection dictionary fit (VARPRO, separable least squares): only the NON-LINEAR parameters of a
 * layout -- the K rates, and T1 where it is free -- are on the grid; the fractions and S0 of every voxel-atom pair come in closed
 * form.  Every layout is sum_j a_j phi_j(b) with K = 1 (mono), 2 (bi) or 3 (tri) unit columns phi_j = model(b; one-hot fractions,
 * S0 = 1) / sigma -- bi reduced: f1 = 1 and f1 = 0; tri reduced and tri S0: (f1, f2) = (1,0), (0,1), (0,0); full layouts: one
 * f_j = 1 -- evaluated by pnx_curvefit_predict_f64's kernel (the fit's own exp, T1 / STEAM factor, shared fixed rates).
 * Per atom g: M = Phi^T Phi.  Per voxel v and atom g, with y_w = y / sigma and c = Phi^T y_w (on the fp64 matrix cores):
 *   free amplitudes (mono, bi / tri full, bi / tri S0):  a_hat = M^-1 c;
 *   sum-to-one (bi / tri reduced):  a_hat_{j<K} minimises || y_w - phi_K - sum_{j<K} a_j (phi_j - phi_K) ||;
 *   clip into the box (an exact feasible point, no division per pair):
 *     mono     S0 = clip(a_hat_1, lo_S0, hi_S0);
 *     full     a'_j = clip(a_hat_j, lo_fj, hi_fj);
 *     reduced  a'_j = clip(a_hat_j, lo_fj, hi_fj) for j < K,  a'_K = 1 - sum_{j<K} a'_j;
 *     S0       S = clip(sum a_hat, lo_S0, hi_S0),  a'_j = clip(a_hat_j, lo_fj S, hi_fj S) for j < K,  a'_K = S - sum_{j<K} a'_j;
 *              reported S0 = S, f_j = a'_j / S, or lo_fj when S = 0;
 *   cost_g(v) = 0.5 ||y_w||^2 - c^T a' + 0.5 a'^T M a': the true cost of the reported parameter vector.
 * best[v] = the argmin over g, the lowest index among equal costs; p_out[:, v] = that atom's non-linear values, copied, and the
 * clipped amplitudes mapped to the layout's fractions / S0; cost[v] its cost; clipped[v] = 1 when a clip was active at the winner.
 * The clipped optimum is exact for K = 1; for K > 1 it is a feasible point, optimal whenever no clip is active.  As in the bounded
 * fit the box is the feasible set: 1 - f1 - f2 may be negative (pnx_curvefit_simplex_f64 is the tool for that).  An atom whose M
 * is not positive definite in fp64 gets a_hat = 0.  The expanded cost carries the rounding of K + 1 dot products of n_b terms and
 * of the stored inverse: costs closer than about 4 (n_b + kappa(M)) 2^-52 (||y_w||^2 + ||a'||_1^2 max_j ||phi_j||^2) may swap.
 * A voxel with a non-finite (weighted) signal gets best = -1, cost = NaN, clipped = 0 and p_out = fallback; its neighbours are
 * bit-identical to a run without it.
 *   opts: model, n_b, n_free, n_fixed, free_idx, fixed_idx, t1_mode, tr, tm, sigma are read;
 *   b (n_b,) host; y (n_vox, n_b) host|device; nl_atoms (n_nl, n_atoms) host: the free non-linear parameters of every atom,
 *   one row per free rate / T1 in the order of free_idx, 1 <= n_atoms <= 4096; fixed (n_fixed,) host or NULL (rates and T1 only);
 *   lo, hi (n_free,) host; fallback (n_free,) host, inside lo / hi;
 *   p_out (n_free, n_vox), best (n_vox) int32 or NULL, cost (n_vox) or NULL, clipped (n_vox) int8 or NULL: out, host|device as `mem`.
 * PNX_MEM_DEVICE only enqueues (the dictionary lives in a stream-ordered buffer); PNX_MEM_HOST goes through the chunk ring.  The
 * (n_vox, n_atoms) product never reaches memory.
 * Refused with a message that names the argument, before any device work: per_voxel_p0_bounds, fixed_per_voxel, queue_order, a
 * fixed fraction or a fixed S0 (PNX_ERR_UNSUPPORTED); n_atoms out of range, n_b <= K, an atom with two exactly equal rates (M is
 * singular), a non-linear value outside its bounds, lo > hi of a fraction or S0, lo_S0 < 0, a fallback outside the bounds
 * (PNX_ERR_INVALID).
 */
PNX_API int pnx_curvefit_varpro_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y, int n_atoms,
                            const double *nl_atoms, const double *fixed, const double *lo, const double *hi, const double *fallback,
                            double *p_out, int32_t *best, double *cost, int8_t *clipped, int mem, int device, void *stream);
/*
 * Posterior over the variable-projection dictionary: the Bayesian treatment of sums of exponentials in which the
 * linear amplitudes are eliminated per atom (Bretthorst) and the posterior lives on the grid of the NON-LINEAR parameters only.
 * The dictionary nl_atoms, the unit columns, the 1 / sigma weighting, the per-atom constants, the amplitude solve and the clip rule
 * per class, the true cost c_g(v) = 0.5 ||y_w||^2 - c . a' + 0.5 a'^T M a' and every refusal are pnx_curvefit_varpro_f64's; there
 * is no fallback argument.
 *   log_prior (n_atoms,) host or NULL (uniform): every entry finite or -inf, at least one finite (PNX_ERR_INVALID otherwise);
 *     an atom at -inf is excluded.
 *   noise_sd > 0: known Gaussian noise sd in the units of the (sigma-weighted) signal; == 0: the noise scale is marginalised under
 *     a Jeffreys prior; negative or non-finite: PNX_ERR_INVALID.
 *   marginal_amplitudes 0 / 1 (anything else PNX_ERR_INVALID), see below.
 * With n_lin the number of amplitudes solved per atom (K for the free and S0 classes, K - 1 for the sum-to-one layouts), N_g the
 * matrix that solve inverts (M, or the difference system) and nu = n_b - n_lin, per voxel v and atom g, in fp64:
 *   lw_g = log_prior_g + (marginal_amplitudes ? -0.5 log det N_g : 0), built once per call on the device; an atom whose N is not
 *          positive definite in fp64 (the variable projection's a_hat = 0 atoms) gets lw = -inf when marginal_amplitudes is set;
 *   l_g  = lw_g - c_g / noise_sd^2                              (known noise)
 *   l_g  = lw_g - (nu / 2) log(max(c_g, tol_v))                 (marginalised)
 *   tol_v = 4 n_b 2^-52 (||y_w||^2 + A^2 max_{g,j} ||phi_j||^2), the rounding bound of the expanded cost, with A the largest
 *          ||a'||_1 the class's clip rule can return for the call's box, computed on the host:
 *            free (mono, bi / tri full)  A = sum_j max(|lo_j|, |hi_j|) over the amplitudes (mono: S0);
 *            reduced                     A = F = sum_{j<K} max(|lo_fj|, |hi_fj|) + max(|1 - sum_{j<K} lo_fj|, |1 - sum_{j<K} hi_fj|);
 *            S0                          A = hi_S0 F   (lo_S0 >= 0 is required, so |S| <= hi_S0);
 *   L = log sum_g exp(l_g);  W_g = exp(l_g - L);  padded and excluded atoms have weight 0.
 *   mean[k] = sum_g W_g theta_kg;  theta_kg = nl_atoms[row, g] in a non-linear row; in a fraction / S0 row the reported linear
 *     parameter of the pair (v, g): the clipped a' mapped as the variable projection maps it (f_j = a'_j / S kept inside the box);
 *   sd[k] = sqrt(max(0, sum_g W_g (theta_kg - mean[k])^2)), accumulated by a weighted Welford / Chan merge (no E[x^2] - mean^2);
 *   map_atom = argmax_g l_g, the lowest index among equal l;  map_p = that atom's rates / T1 copied bit for bit and its reported
 *     linear parameters;  log_evidence = L - log sum_g exp(log_prior_g);  ess = (sum W)^2 / sum W^2 in [1, n_atoms];
 *   clipped_mass = sum_g W_g [a clip was active at (v, g)]: the posterior share that rests on clipped amplitudes.
 * marginal_amplitudes = 1: the weight is the exact marginal over unconstrained amplitudes under a flat prior -- Gaussian for known
 *   noise, Student-t with nu degrees of freedom for marginalised noise -- wherever no clip is active.  Where a clip is active it is
 *   a Laplace-style approximation at the clipped point: the cost of the clipped a' with the curvature term of the free solve.
 *   marginal_amplitudes = 0 is the profile weight (the amplitudes at their clipped optimum, no Occam term).
 * Known understatement: the sd of a linear row (a fraction, S0) is the between-atom spread of the clipped optimum only; the
 *   conditional variance of the amplitudes given the rates is left out.
 * A voxel with a non-finite (weighted) signal, and a voxel for which no atom has a finite l, gets NaN in every floating output
 * and map_atom = -1; its neighbours are bit-identical to a run without it.
 *   opts, b, y, nl_atoms, fixed, lo, hi: as pnx_curvefit_varpro_f64 takes them;
 *   mean, sd, map_p (n_free, n_vox); map_atom (n_vox) int32; log_evidence, ess, clipped_mass (n_vox): out, host|device as `mem`;
 *   all but mean may be NULL.  PNX_MEM_DEVICE only enqueues; PNX_MEM_HOST goes through the chunk ring.  The (n_vox, n_atoms)
 *   matrix never reaches memory.
 */
PNX_API int pnx_curvefit_varpro_posterior_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                      const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                      const double *log_prior, double noise_sd, int marginal_amplitudes, double *mean, double *sd,
                                      int32_t *map_atom, double *map_p, double *log_evidence, double *ess, double *clipped_mass,
                                      int mem, int device, void *stream);
/*
 * Marginal posterior of every free NON-LINEAR parameter (a rate, a free T1) over the variable-projection dictionary, credible-
 * interval quantiles and a geometric posterior mean from it.  The arguments up to marginal_amplitudes, the
 * weighting, the dictionary, the amplitude solve, the clip rule, c_g(v), tol_v, l_g and every refusal are
 * pnx_curvefit_varpro_posterior_f64's.  The atoms sit on a grid: along a non-linear free parameter k every atom holds one of
 * n_bins[k] values.
 *   n_bins (n_free,) int32 host: the number of distinct grid values of each free parameter; 0: no marginal for that parameter.
 *     n_bins[k] must be 0 for every linear row (a fraction, S0): its value belongs to the voxel-atom pair, not to the atom, and an
 *     indicator that depends on the voxel is not a matrix product.  B = sum n_bins must lie in [1, 128];
 *   bin_of (n_free, n_atoms) int32 host: the bin of atom g along parameter k, in [0, n_bins[k]); rows with n_bins[k] == 0 are
 *     not read;
 *   bin_value (B,) host: the grid value of every bin, parameter k's at offset off_k = sum_{i<k} n_bins[i], strictly ascending within
 *     a parameter; every atom must satisfy nl_atoms[row_k, g] == bin_value[off_k + bin_of[k, g]] exactly (row_k: the row of
 *     nl_atoms that holds free parameter k);
 *   n_q in [0, 8], probs (n_q,) host, each in the open interval (0, 1).
 * Every violation is PNX_ERR_INVALID (PNX_ERR_UNSUPPORTED where the posterior says so) with a message that names the first
 * offender, before any device work.
 * Per finite voxel v, in fp64:  L = log sum_g exp(l_g);  W_g = exp(l_g - L), exactly 0 for a padded or excluded atom;
 *   marginal[off_k + j, v] = sum over the atoms with bin_of[k, g] == j of W_g      (not renormalised afterwards)
 *   cdf_j = the running sum of marginal over j in bin order;  quantile[i, k, v] = bin_value of the first bin with
 *     cdf_j >= probs[i], of the last bin of k when none reaches it (no interpolation), NaN for a parameter with n_bins[k] == 0;
 *   geo_mean[k, v] = exp(sum_j marginal_j log bin_value_j / sum_j marginal_j): the posterior mean of log(parameter k), the natural
 *     point estimate on a log-spaced axis; NaN for a parameter with n_bins[k] == 0 or with a bin value <= 0;
 *   log_evidence = L - log sum_g exp(log_prior_g), the posterior's within its rounding bound.
 * A voxel with a non-finite (weighted) signal, or without an admissible atom, gets NaN in every output; its neighbours are not
 * affected.
 *   marginal (B, n_vox) bin-major, not NULL; quantile (n_q, n_free, n_vox), NULL only when n_q == 0; geo_mean (n_free, n_vox) or
 *   NULL; log_evidence (n_vox) or NULL: out, host|device as `mem`.
 * One pass over the products Phi^T y: the weights are formed about a running maximum of l_g per voxel (the sums are rescaled when
 * it moves) and summed per bin by a 0/1 indicator matrix on the matrix cores; the (n_vox, n_atoms) matrix W never reaches memory.
 * No sum uses an atomic and every sum of a voxel depends on the order of the atoms only: results are bit-identical between two
 * calls, between PNX_MEM_HOST and PNX_MEM_DEVICE, and whatever the number of voxels in the call.
 *   PNX_MEM_DEVICE only enqueues.  PNX_MEM_HOST: y is uploaded once (pnx_upload's path) and the outputs come back from one
 *   stream-ordered buffer (pnx_download's path), as pnx_curvefit_grid_marginals_f64 stages them -- no chunk ring; PNX_ERR_NOMEM
 *   names the sizes.
 */
PNX_API int pnx_curvefit_varpro_marginals_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                      const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                      const double *log_prior, double noise_sd, int marginal_amplitudes, const int32_t *n_bins,
                                      const int32_t *bin_of, const double *bin_value, int n_q, const double *probs, double *marginal,
                                      double *quantile, double *geo_mean, double *log_evidence, int mem, int device, void *stream);
/*
 * The prior of pnx_curvefit_varpro_posterior_f64 learned from the volume itself (empirical Bayes): the
 * non-parametric maximum-likelihood mixture over the rate dictionary, by EM.  The arguments up to marginal_amplitudes, the
 * weighting, the dictionary, the amplitude solve, the clip rule, c_g(v), tol_v and every refusal are
 * pnx_curvefit_varpro_posterior_f64's; the range rules and messages of n_iter, pseudo_count, rel_tol and log_prior_out, the
 * normalisation of the start, loglik, the stopping rule, the NaN tail, n_eff and the synchronisation are
 * pnx_curvefit_grid_prior_em_f64's.  Every refusal comes before any device work.  In fp64:
 *   Likelihood.  The Occam term belongs to the likelihood, not to the learned table:
 *     occ_g = marginal_amplitudes ? -0.5 log det N_g : 0;   lw_g = log pi_g + occ_g;   l_g(v) is the posterior's with this lw_g.
 *   Admissible atoms.  An atom is admissible when its start log_prior is finite and occ_g is finite (a non-finite occ_g marks the
 *     variable projection's a_hat = 0 atoms under marginal_amplitudes).  n_adm counts them.  A non-admissible atom has weight
 *     exactly 0 and log_prior_out = -inf, always.
 *   Voxels that take part.  A voxel takes part when its weighted signal is finite and at least one atom has a finite l.  n_eff
 *     counts them.  The others change nothing: their neighbours are bit-identical to a run without them.
 *   Update.  L_v = log sum_g exp l_g(v);  W_vg = exp(l_g(v) - L_v);  S_g = sum_v W_vg over the voxels that take part;
 *     pi_g <- (S_g + pseudo_count) / (n_eff + pseudo_count n_adm);  log_prior_g <- log pi_g, -inf where pi_g == 0.
 *   Memory and reproducibility.  The (n_vox, n_atoms) matrix W never reaches memory.  No sum uses an atomic.  Every sum has one
 *     order for a given launch grid.  Two calls return the same bytes, PNX_MEM_HOST or PNX_MEM_DEVICE.
 * The start is normalised over its finite entries, log_prior - log sum exp(log_prior), before occ_g is known: loglik[0] is the
 * log-likelihood under that start with the inadmissible atoms at weight 0; from the first update on every reported prior sums to
 * 1 over the admissible atoms, so the sum of log_evidence of a later posterior call under log_prior_out is loglik[done].
 *   log_prior_out (n_atoms,) host, not NULL; loglik (n_iter + 1,) host or NULL; n_iter_done, n_eff: host or NULL.
 *   Without a voxel that takes part the call returns PNX_OK with the start (n_vox == 0: the normalised start), done = 0 and
 *   loglik[0] = 0.
 *   y (n_vox, n_b) host|device as `mem`.  PNX_MEM_DEVICE: read in place.  PNX_MEM_HOST: uploaded once into a stream-ordered buffer
 *   that stays for all passes -- no chunk ring; PNX_ERR_NOMEM names the size and points to a sub-sample.  For both `mem` values
 *   the call SYNCHRONISES `stream` before it returns (once per update, for 16 bytes, and at the end).
 * An update is two passes that both pay the K x K amplitude solve of every voxel-atom pair (the measured price).
 */
PNX_API int pnx_curvefit_varpro_prior_em_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                     const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                     const double *log_prior, double noise_sd, int marginal_amplitudes, int n_iter,
                                     double pseudo_count, double rel_tol, double *log_prior_out, double *loglik, int *n_iter_done,
                                     int64_t *n_eff, int mem, int device, void *stream);
/*
 * pnx_curvefit_varpro_posterior_f64 with one prior row per segmentation label.  Every argument of that call, its
 * weighting, refusals and outputs (clipped_mass included), and
 *   n_classes in [1, 16] (PNX_ERR_INVALID otherwise);
 *   labels (n_vox,) int32, host|device as `mem`: the row of the table voxel v is judged under;
 *   log_prior (n_classes, n_atoms) row-major, host, or NULL (every row uniform): every entry finite or -inf (NaN or +inf is
 *     PNX_ERR_INVALID and names log_prior[c, g]); rows may exclude different atoms; every row needs at least one finite entry --
 *     otherwise PNX_ERR_INVALID with a message that names the row, before any device work.
 * Per voxel v, with c = labels[v]:
 *   occ_g = marginal_amplitudes ? -0.5 log det N_g : 0, shared by all classes and built once per call on the device;
 *   lw_cg = log_prior[c, g] + occ_g;   l_g(v) is pnx_curvefit_varpro_posterior_f64's, term for term, with lw taken from row c;
 *   log_evidence_v = L_v - log sum_g exp(log_prior[c, g]);  a pair whose lw is -inf has weight exactly 0.
 * An atom whose occ_g is not finite is inadmissible in every row; a voxel whose row has no atom with a finite l is reported as the
 * unlabelled call reports it (NaN, map_atom = -1).
 * Labels may live on the device and are not validated on the host: a voxel whose label lies outside [0, n_classes) is treated
 * exactly as a voxel with a non-finite signal -- NaN in every floating output, map_atom = -1 -- and its neighbours are
 * bit-identical to a run without it.  This is how a caller marks background (label -1).
 * Every sum of a voxel depends on the order of the atoms only: a voxel's outputs are the bytes
 * pnx_curvefit_varpro_posterior_f64 returns for it under log_prior[c, :] whenever the rows admit the same atoms.  The moments of
 * the non-linear rows are accumulated about the mid-range of the atoms that ANY row admits (linear rows about 0): with rows that
 * exclude different atoms mean and sd of the non-linear rows agree within the posterior's rounding bound taken over that range,
 * every other output stays byte-equal.  With n_classes == 1 and every label 0 the call returns the unlabelled call's bytes.
 * PNX_MEM_DEVICE only enqueues; PNX_MEM_HOST goes through the chunk ring, the labels beside the signals.
 */
PNX_API int pnx_curvefit_varpro_posterior_classes_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                      int n_atoms, const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                      int n_classes, const int32_t *labels, const double *log_prior, double noise_sd,
                                      int marginal_amplitudes, double *mean, double *sd, int32_t *map_atom, double *map_p,
                                      double *log_evidence, double *ess, double *clipped_mass, int mem, int device, void *stream);
/*
 * pnx_curvefit_varpro_prior_em_f64 with one prior row per segmentation label, all rows learned in one pass pair over the volume
 * (DESIGN.md 4.1o).  n_classes, labels and log_prior (n_classes, n_atoms) as pnx_curvefit_varpro_posterior_classes_f64 takes
 * them, with its lw_cg, its refusals and its rule for a label outside [0, n_classes): such a voxel takes no part.  Every row of
 * the start is normalised first.  One update, per class c:
 *   n_adm_c: the atoms with a finite start entry in row c and a finite occ_g; every other entry of row c is -inf, always;
 *   S_cg = sum of W_vg over the voxels of class c that take part (finite signal, label in range, an atom with a finite l);
 *   pi_cg <- (S_cg + pseudo_count) / (n_eff_c + pseudo_count n_adm_c)
 * and log_prior[c, g] <- log pi_cg; an entry at -inf stays there; a class without a voxel that takes part keeps its normalised
 * start row (a class whose finite entries all sit on atoms without a finite occ_g has none).
 *   log_prior_out (n_classes, n_atoms) host, not NULL;
 *   loglik (n_iter + 1,) host or NULL: the sum over the classes, in class order, of
 *   loglik_class (n_iter + 1, n_classes) host or NULL: per class the sum of L_v over its voxels that take part, under the table
 *     before update t; entries past `done` are NaN in both;
 *   n_iter_done: `done`; the stopping rule is pnx_curvefit_varpro_prior_em_f64's, applied to loglik (the sum);
 *   n_eff (n_classes,) int64 host or NULL: per class the voxels that take part.  Without any the call returns PNX_OK with the
 *     normalised start, done = 0 and loglik[0] = 0.
 * No atomics; every sum has one order for a given launch grid: two calls return the same bytes, PNX_MEM_HOST or PNX_MEM_DEVICE;
 * the (n_vox, n_atoms) matrix W never reaches memory.  With n_classes == 1 and every label 0 the call returns the bytes of
 * pnx_curvefit_varpro_prior_em_f64.  The accumulate pass separates the classes that meet in a strip of 16 voxels in a loop over
 * the classes present there: a label map sorted by class pays for one class per strip (DESIGN.md 4.1o has the cost).
 *   y, labels host|device as `mem`; PNX_MEM_HOST uploads both once for all iterations (no chunk ring; PNX_ERR_NOMEM names the
 *   size).  For both `mem` values the call SYNCHRONISES `stream` before it returns.
 */
PNX_API int pnx_curvefit_varpro_prior_em_classes_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                     int n_atoms, const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                     int n_classes, const int32_t *labels, const double *log_prior, double noise_sd,
                                     int marginal_amplitudes, int n_iter, double pseudo_count, double rel_tol, double *log_prior_out,
                                     double *loglik, double *loglik_class, int *n_iter_done, int64_t *n_eff, int mem, int device,
                                     void *stream);
/*
 * Neighbourhood (MRF) prior for pnx_curvefit_varpro_posterior_f64 by coloured mean-field sweeps: the prior of
 * pnx_curvefit_grid_posterior_mrf_f64 with theta restricted to the NON-LINEAR free rows (the rates, a free T1).  A fraction or S0
 * row has no grid value -- its value belongs to the voxel-atom pair -- so its precision must be 0 (PNX_ERR_INVALID otherwise), the
 * rule of the projected S0 row of the grid solver and of n_bins of pnx_curvefit_varpro_marginals_f64.  With lambda = precision:
 *   l_g(v) = [pnx_curvefit_varpro_posterior_f64's l_g(v), term for term] + sum_{k non-linear} thetac_kg q_vk - 1/2 n_v r_g
 *   thetac_kg = nl_atoms[row_k, g] - centre_k   centre_k: the posterior's own centre, min + (max - min) / 2 over the admissible atoms
 *   q_vk = lambda_k sum_{u in N(v), present} (mean[k, u] - centre_k)      pnx_curvefit_grid_neighbour_field_f64 with centre = 0 and
 *                                                                         precision = 0 on the linear rows: q is 0 there
 *   n_v = the number of present neighbours;  r_g = sum_k lambda_k thetac_kg^2   (host, fp64, k ascending over the non-linear rows)
 * A neighbour is present when its slot holds an index >= 0 and mean[0, u] is finite.  The Occam term of marginal_amplitudes and the
 * exclusions lw = -inf stay as they are; a pair at lw = -inf is skipped before any arithmetic.
 *
 * pnx_curvefit_varpro_posterior_field_f64: one colour update.  Every argument of pnx_curvefit_varpro_posterior_f64 up to
 * marginal_amplitudes, its weighting, refusals and outputs, for the voxels [first, first + count) under the l_g above, written IN
 * PLACE into the full-length output arrays (n_free, n_vox) / (n_vox); the other voxels' entries are not touched.
 *   n_vox in [0, 2^31 - 1];
 *   field_q (n_free, n_vox), field_n (n_vox) int32: device, as the gather wrote them (only the range, and of field_q only the
 *     non-linear rows, are read);
 *   precision (n_free,) host: finite, >= 0, and 0 on a fraction / S0 row;
 *   delta_max: device scalar or NULL; receives max over { k: non-linear, precision_k > 0 and range_k > 0; v in the range, finite } of
 *     |mean_new[k, v] - mean_old[k, v]| / range_k,  range_k = max_g theta_kg - min_g theta_kg over the admissible atoms.  Each lane
 *     reads its old mean before it overwrites it; the maximum is reduced per block by shuffles and then over the blocks by a small
 *     kernel: no floating-point atomics.  0 for an empty range.
 * With field_q = 0 and field_n = 0 the added terms are exactly +0.0 and the call returns the bytes of
 * pnx_curvefit_varpro_posterior_f64 for those voxels, clipped_mass included; with every precision 0 the field is not read and the
 * same holds.
 * log_evidence is L_v - log sum_g exp(log_prior_g) with the field inside L_v: a LOCAL NORMALISER of the voxel's update given its
 * neighbours, not a model evidence -- do not sum it over voxels or compare it between models.
 * The field product runs on the fp64 matrix cores, one k-step (at most K + 1 <= 4 non-linear rows) into an accumulator of its own.
 * PNX_MEM_DEVICE only (PNX_ERR_INVALID otherwise); the call only enqueues.
 */
PNX_API int pnx_curvefit_varpro_posterior_field_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                     int n_atoms, const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                     const double *log_prior, double noise_sd, int marginal_amplitudes, int64_t first, int64_t count,
                                     const double *field_q, const int32_t *field_n, const double *precision, double *mean, double *sd,
                                     int32_t *map_atom, double *map_p, double *log_evidence, double *ess, double *clipped_mass,
                                     double *delta_max, int mem, int device, void *stream);
/*
 * pnx_curvefit_varpro_posterior_mrf_f64: the driver.  The arguments and outputs of pnx_curvefit_varpro_posterior_f64, and
 *   n_nb in [1, 8]; neighbours (n_vox, n_nb) int32, -1 where a slot is empty, host|device as `mem`; the graph must be symmetric
 *     (not checked);
 *   n_colours in [1, 8]; colour_start (n_colours + 1,) int64 host, ascending from 0 to n_vox: the voxels of colour c are the
 *     contiguous range [colour_start[c], colour_start[c+1]) -- the caller sorts the voxels by colour; a colour may be empty;
 *   precision (n_free,) host; n_sweeps in [0, 100]; tol finite, >= 0;
 *   delta (n_sweeps,) host or NULL; n_sweeps_done host or NULL.
 * Sweep 0 is the plain posterior on all voxels (the bytes of pnx_curvefit_varpro_posterior_f64).  Sweep s = 1 .. n_sweeps runs, for
 * each colour in order, pnx_curvefit_grid_neighbour_field_f64's gather and then the field posterior on that colour's range: colour
 * after colour is coordinate ascent on the variational free energy, which never decreases.  delta[s-1] is the maximum of delta_max
 * over the sweep's colour updates; the call stops after sweep s when delta[s-1] <= tol (tol = 0 runs all sweeps, without a host
 * round trip per sweep); entries of delta past n_sweeps_done are NaN.  log_evidence is the local normaliser described above.
 * A small kernel verifies the table before sweep 0, and nothing is dereferenced before it is bound-checked: an index outside
 * [-1, n_vox), or a neighbour of a voxel inside the voxel's own colour range, returns PNX_ERR_INVALID and names the first offending
 * voxel.  Refused before any device work: everything the posterior refuses; n_nb, n_colours, n_sweeps or tol out of range;
 * colour_start not ascending from 0 to n_vox; a negative or non-finite precision; a positive precision on a fraction / S0 row.
 * Every sum of a voxel depends on the order of the atoms and of its slots only: two calls return the same bytes, PNX_MEM_HOST or
 * PNX_MEM_DEVICE, and the call returns the bytes of the same sequence composed from the gather and the field call.
 *   PNX_MEM_HOST: y and neighbours are uploaded once (pnx_upload's path) and the outputs come back from one stream-ordered
 *   buffer, as pnx_curvefit_grid_posterior_mrf_f64 does -- no chunk ring; PNX_ERR_NOMEM names the size.  For both `mem` values the
 *   call SYNCHRONISES `stream` before it returns.
 */
PNX_API int pnx_curvefit_varpro_posterior_mrf_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                     int n_atoms, const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                     const double *log_prior, double noise_sd, int marginal_amplitudes, int n_nb,
                                     const int32_t *neighbours, int n_colours, const int64_t *colour_start, const double *precision,
                                     int n_sweeps, double tol, double *mean, double *sd, int32_t *map_atom, double *map_p,
                                     double *log_evidence, double *ess, double *clipped_mass, double *delta, int *n_sweeps_done,
                                     int mem, int device, void *stream);
/*
 * The neighbourhood (MRF) prior above with a per-row choice of the coupled quantity.  Every free non-linear row k
 * is coupled in f_k = nl_atoms[row_k] (coupling[k] = 0, the calls above) or in f_k = log nl_atoms[row_k] (coupling[k] = 1): on a
 * geometric rate axis the prior then pulls the neighbours' E[log theta] together, not the means that the large atoms carry.
 *   l_g(v) = [pnx_curvefit_varpro_posterior_f64's l_g(v), term for term] + sum_k fc_kg q_vk - 1/2 n_v r_g
 *   fc_kg = f_kg - fcentre_k      fcentre_k = min + (max - min) / 2 of f_k over the admissible atoms
 *   q_vk = lambda_k sum_{u in N(v), present} (field_mean[k, u] - fcentre_k)   pnx_curvefit_grid_neighbour_field_f64 fed field_mean
 *                                                                             and fcentre (0 on the fraction / S0 rows)
 *   r_g = sum_k lambda_k fc_kg^2  (host, fp64, k ascending);   field_mean[k, v] = E_W[f_k] under the weights W behind mean
 * mean, sd, map_p, map_atom, log_evidence, ess and clipped_mass keep their meaning and layout: the moments stay over the linear
 * theta.  Both moment sets come out of one fold, so they describe the same weights.
 *
 * pnx_curvefit_varpro_posterior_logfield_f64: one colour update.  The arguments of pnx_curvefit_varpro_posterior_field_f64, and
 *   coupling (n_free,) int32 host: 0 or 1; must be 0 on a fraction / S0 row and where precision is 0; on a log row every
 *     admissible atom must be > 0 -- each PNX_ERR_INVALID before any device work, by name;
 *   field_mean (n_free, n_vox) device, not NULL: written in place for the range (NaN where mean is NaN); on a coupling-0 row
 *     (every fraction / S0 row among them) it holds the bytes of mean;
 *     mean and field_mean must not overlap (where the fold runs in two passes the second reads back the fraction / S0 rows of
 *     mean that the first stored);
 *   field_q: what the gather wrote from field_mean and fcentre;
 *   delta_max: as above with |field_mean_new[k, v] - field_mean_old[k, v]| / range(f_k); the old field_mean is read before it
 *     is overwritten.
 * With every coupling 0 the call returns the bytes of pnx_curvefit_varpro_posterior_field_f64; with field_q = 0 and field_n = 0, or
 * every precision 0, the bytes of pnx_curvefit_varpro_posterior_f64, clipped_mass included.
 *
 * pnx_curvefit_varpro_posterior_logmrf_f64: the driver.  The arguments of pnx_curvefit_varpro_posterior_mrf_f64, its sequence,
 * checks, refusals, PNX_MEM_HOST path and synchronisation, and coupling as above; field_mean (n_free, n_vox) host|device as `mem`
 * or NULL.  Sweep 0 runs the same fold without a field: the bytes of pnx_curvefit_varpro_posterior_f64 for every output above and
 * field_mean from the same weights.  The call returns the bytes of the same sequence composed from the gather and the logfield
 * call; with every coupling 0 the bytes of pnx_curvefit_varpro_posterior_mrf_f64.
 */
PNX_API int pnx_curvefit_varpro_posterior_logfield_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                     int n_atoms, const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                     const double *log_prior, double noise_sd, int marginal_amplitudes, int64_t first, int64_t count,
                                     const double *field_q, const int32_t *field_n, const double *precision, const int32_t *coupling,
                                     double *mean, double *sd, int32_t *map_atom, double *map_p, double *log_evidence, double *ess,
                                     double *clipped_mass, double *field_mean, double *delta_max, int mem, int device, void *stream);
PNX_API int pnx_curvefit_varpro_posterior_logmrf_f64(const pnx_curvefit_opts *opts, int64_t n_vox, const double *b, const double *y,
                                     int n_atoms, const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                     const double *log_prior, double noise_sd, int marginal_amplitudes, int n_nb,
                                     const int32_t *neighbours, int n_colours, const int64_t *colour_start, const double *precision,
                                     const int32_t *coupling, int n_sweeps, double tol, double *mean, double *sd, int32_t *map_atom,
                                     double *map_p, double *log_evidence, double *ess, double *clipped_mass, double *field_mean,
                                     double *delta, int *n_sweeps_done, int mem, int device, void *stream);
/*
 * Log-linear mono-exponential fit, ln S = ln S0 - b D by (weighted) linear least squares per voxel: the ADC
 * map, step 1 of a segmented IVIM fit, a cheap source of S0 / D start values.  A closed form over one pass of the data: a voxel
 * costs its signal row in and its results out.  Per voxel, in fp64, in the order written:
 *   use[i]: the caller's 0/1 mask over the b-values (NULL = all).  A non-finite y_i with use[i]: status -2, every output NaN
 *     (n_used 0), the curve fit's convention; the voxel's neighbours are not affected.
 *   U = { i : use[i] and y_i > 0 }, n_used = |U|: a non-positive sample has no logarithm and is left out, not clamped.
 *   l_i = log(y_i);  w_i = 1 (weighting 0) or y_i^2 (weighting 1, the usual weights of log-transformed data).
 *   bm = sum w b / sum w;  lm = sum w l / sum w;  Sbb = sum w (b - bm)^2;  D = -sum w (b - bm)(l - lm) / Sbb;  a = lm + D bm;
 *   S0 = exp(a) -- the centred form, never the raw 2 x 2 normal matrix.
 *   n_reweight (0 .. 8) further passes repeat the fit over the same U with w_i = exp(a - b_i D)^2 of the previous estimate.
 *   status 0, parameters / pcov / ss_res NaN: n_used < 2, Sbb == 0 in any pass, or a non-finite a or D (weights that overflow);
 *   status 1 otherwise.
 *   pcov of (S0, D): for n_used >= 3, s^2 = sum w r^2 / (n_used - 2) with r_i = l_i - (a - b_i D) and the last pass's weights,
 *     var a = s^2 (1 / sum w + bm^2 / Sbb), cov(a, D) = s^2 bm / Sbb, var D = s^2 / Sbb (s^2 (X^T W X)^-1 from the centred sums),
 *     mapped to (S0, D) by the delta method: [[S0^2 var a, S0 cov], [S0 cov, var D]].  n_used == 2: NaN, status stays 1.
 *   clip != 0: S0 and D are clipped into [lo[0], hi[0]] and [lo[1], hi[1]] after the fit; a voxel that was moved gets status 2;
 *     pcov stays as computed.
 *   ss_res = sum over use[i] of (S0 exp(-b_i D) - y_i)^2: the SIGNAL-domain residual at the returned (clipped) point over every
 *     masked-in sample, the non-positive ones included, so that R^2 follows from pnx_row_ss_tot_f64 as for the other solvers.
 *   b (n_b,) host; use (n_b,) uint8 host or NULL; lo, hi (2,) host when clip (not read otherwise);
 *   y (n_vox, n_b) in; params (2, n_vox) parameter-major [S0, D]; pcov (n_vox, 2, 2) or NULL; status (n_vox) int8 or NULL;
 *   n_used (n_vox) int32 or NULL; ss_res (n_vox) or NULL: host|device as `mem`.
 * pnx_loglinear_f32: fp32 storage of b, lo, hi, y, params, pcov and ss_res, the same fp64 arithmetic (as pnx_curvefit_batch_f32;
 *   the kernel reads and writes float, nothing is staged).
 * PNX_MEM_DEVICE only enqueues; PNX_MEM_HOST goes through the chunk ring.  PNX_ERR_INVALID with a message that names the
 * argument, before any device work: n_b outside 2 .. PNX_MAX_BVALUES, a NULL b / y / params, a non-finite b, weighting not 0 / 1,
 * n_reweight outside 0 .. 8, a mask that leaves fewer than 2 b-values or fewer than 2 distinct ones, clip with NULL bounds or
 * lo >= hi, mem not host / device.
 */
PNX_API int pnx_loglinear_f64(int64_t n_vox, int n_b, const double *b_host, const uint8_t *use_host, int weighting, int n_reweight,
                      int clip, const double *lo_host, const double *hi_host, const double *y, double *params, double *pcov,
                      int8_t *status, int32_t *n_used, double *ss_res, int mem, int device, void *stream);
PNX_API int pnx_loglinear_f32(int64_t n_vox, int n_b, const float *b_host, const uint8_t *use_host, int weighting, int n_reweight,
                      int clip, const float *lo_host, const float *hi_host, const float *y, float *params, float *pcov,
                      int8_t *status, int32_t *n_used, float *ss_res, int mem, int device, void *stream);
/*
 * Exponential peeling ("curve stripping", the fully segmented IVIM estimate) of the mono-, bi- and tri-exponential layouts
 * (DESIGN.md 4.1f): the slowest compartment is fitted log-linearly on the high b-values and subtracted, the next faster one is
 * fitted on what is left of the lower b-values, and once more for a third.  A closed form: the clinical estimator where a
 * non-linear fit is too noisy, and a per-voxel start value for the non-linear fit.  K = the number of exponentials of `model`
 * (1 for PNX_MODEL_MONO, 2 for the bi-, 3 for the tri-exponential layouts; all seven are served).  No T1 / STEAM factor, nothing
 * fixed.  Per voxel, in fp64, in the order written:
 *   use: a (K, n_b) 0/1 mask.  Row k is the set of b-values of stage k; stage 0 is the SLOWEST compartment and is fitted first.
 *     M = the union of the rows.  A non-finite y_i with i in M: status -2, every output NaN (n_used 0); the voxel's neighbours
 *     are not affected.  A non-finite sample outside M is ignored.
 *   r(0) = y.  For k = 0 .. K-1:
 *     U_k = { i : use[k][i] and r(k)_i > 0 }, n_used[k] = |U_k|: a non-positive residual is left out, not clamped.
 *     l_i = log r(k)_i;  w_i = 1 (weighting 0) or (r(k)_i)^2 (weighting 1).
 *     The centred weighted line of pnx_loglinear_f64 over U_k: bm = sum w b / sum w;  lm = sum w l / sum w;
 *     Sbb = sum w (b - bm)^2;  D_k = -sum w (b - bm)(l - lm) / Sbb;  a_k = lm + D_k bm;  A_k = exp(a_k).
 *     The stage fails when n_used[k] < 2, Sbb == 0, or any of a_k, D_k, A_k is non-finite: status 0, parameters and ss_res NaN,
 *     n_used of the stages not reached 0.
 *     Otherwise r(k+1)_i = r(k)_i - A_k exp(-b_i D_k) for EVERY i.
 *   Stage k is component K - k of the layout (component 1 is the fastest).  With S = sum A_k:
 *     mono [S0, D]: [A_0, D_0];  bi reduced [f1, D1, D2]: [A_1 / S, D_1, D_0];  bi S0: the reduced layout, then S;
 *     bi full [f1, D1, f2, D2]: [A_1, D_1, A_0, D_0] (amplitudes);  tri reduced [f1, D1, f2, D2, D3]:
 *     [A_2 / S, D_2, A_1 / S, D_1, D_0];  tri S0: the reduced layout, then S;  tri full: [A_2, D_2, A_1, D_1, A_0, D_0].
 *   clip != 0: every parameter is clipped into [lo[j], hi[j]] after the mapping (comparisons that keep a NaN, as
 *     pnx_loglinear_f64); a voxel that was moved gets status 2, a complete voxel that was not moved status 1.
 *   fallback (n_params,) or NULL: when given, a voxel with status 0 or -2 returns this vector instead of NaN (its ss_res stays
 *     NaN), which makes `params` usable as a device-resident per-voxel p0 of pnx_curvefit_batch_f64.
 *   ss_res = sum over i in M of (model(b_i; returned parameters) - y_i)^2: the SIGNAL-domain residual at the returned (clipped)
 *     point over every masked-in sample, so that R^2 follows from pnx_row_ss_tot_f64 as for the other solvers.
 *   No covariance and no re-weighting passes: peeling has no honest closed-form covariance, so none is invented.
 *   b (n_b,) host; use (K, n_b) uint8 host; lo, hi (n_params,) host when clip (not read otherwise); fallback (n_params,) host or
 *   NULL; y (n_vox, n_b) in; params (n_params, n_vox) parameter-major; status (n_vox) int8 or NULL; n_used (K, n_vox) int32 or
 *   NULL; ss_res (n_vox) or NULL: host|device as `mem`.
 * pnx_peel_f32: fp32 storage of b, lo, hi, fallback, y, params and ss_res, the same fp64 arithmetic.
 * PNX_MEM_DEVICE only enqueues; PNX_MEM_HOST goes through the chunk ring.  PNX_ERR_INVALID with a message that names the
 * argument, before any device work: an unknown model, n_b outside 2K .. PNX_MAX_BVALUES, a NULL b / use / y / params, a
 * non-finite b, weighting not 0 / 1, a mask row with fewer than 2 b-values or fewer than 2 distinct ones, clip with NULL bounds
 * or lo >= hi, mem not host / device.
 */
PNX_API int pnx_peel_f64(int model, int64_t n_vox, int n_b, const double *b_host, const uint8_t *use_host, int weighting, int clip,
                 const double *lo_host, const double *hi_host, const double *fallback_host, const double *y, double *params,
                 int8_t *status, int32_t *n_used, double *ss_res, int mem, int device, void *stream);
PNX_API int pnx_peel_f32(int model, int64_t n_vox, int n_b, const float *b_host, const uint8_t *use_host, int weighting, int clip,
                 const float *lo_host, const float *hi_host, const float *fallback_host, const float *y, float *params, int8_t *status,
                 int32_t *n_used, float *ss_res, int mem, int device, void *stream);
/*
 * float32 parameter maps (io/nifti.py:279-312 reconstruct_maps): out (n_spatial, k) zero filled, then
 * out[linear_index[i], :] = (float) values[i, :] for the n_px fitted voxels (linear_index = C-order index into the
 * (X, Y, Z) grid).  values (n_px, k) float64, linear_index (n_px) int64, out float32: host|device as `mem`.
 */
PNX_API int pnx_scatter_maps_f32(const double *values, const int64_t *linear_index, int64_t n_px, int k, int64_t n_spatial, float *out,
                         int mem, int device, void *stream);

/*
 * IDEAL level plumbing on the device.
 * pnx_resize2d_f64: resize the first two axes of an (X, Y, C) array (C = product of the trailing axes, contiguous)
 *   to (TX, TY, C) with OpenCV's INTER_LINEAR (method 0) / INTER_CUBIC (method 1) arithmetic -- half-pixel centres,
 *   cubic a = -0.75, replicated border, no anti-aliasing.  Replaces IDEALFitter._interpolate_array, which calls
 *   cv2.resize per slice and channel (fitters/ideal.py:299-320).  in / out: host or device (mem).
 * pnx_ideal_bounds_f64: from a parameter map (n_px, n_params) -- the previous level's result, resized -- the next
 *   level's start values and bounds, parameter-major (n_params, n_px): p0 = clip(map, lo, hi),
 *   lower = clip(p0 (1 - tol), lo, hi), upper = clip(p0 (1 + tol), lo, hi)  (ideal.py:167-198).  Device pointers;
 *   lo / hi / tol (n_params,) on the host.
 * pnx_ideal_bounds_simplex_f64: the same for a level fitted under f1 + f2 <= 1 (pnx_curvefit_simplex_f64); i_f1 / i_f2 are the
 *   rows of the two fractions.  Interpolating a feasible map overshoots, and a window around a start with f1 + f2 > 1 can hold
 *   no feasible point (the face problem's intersected bounds are then empty: status -1).  Per voxel, in fp64 as written:
 *   p = clip(map, lo, hi); if e = f1 + f2 - 1 > 0: f1 -= e / 2, f2 -= e / 2, both clipped to their bounds again; then p0 /
 *   lower / upper from p as above.  A voxel with f1 + f2 <= 1 after the first clip gets pnx_ideal_bounds_f64's output bit for
 *   bit.  PNX_ERR_INVALID before any device work: n_params outside 1 .. 8, i_f1 or i_f2 outside [0, n_params), i_f1 == i_f2.
 *   Both calls only enqueue; the small arguments travel by value.
 */
PNX_API int pnx_resize2d_f64(const double *in, int X, int Y, int64_t C, double *out, int TX, int TY, int method, int mem,
                     int device, void *stream);
PNX_API int pnx_ideal_bounds_f64(const double *map, int64_t n_px, int n_params, const double *lo_host, const double *hi_host,
                         const double *tol_host, double *p0, double *lower, double *upper, int device, void *stream);
PNX_API int pnx_ideal_bounds_simplex_f64(const double *map, int64_t n_px, int n_params, const double *lo_host, const double *hi_host,
                                 const double *tol_host, int i_f1, int i_f2, double *p0, double *lower, double *upper,
                                 int device, void *stream);

/*
 * IDEAL level plumbing between the resize and the fit (fitters/ideal.py:199-254), device pointers:
 * pnx_mask_select_f64: C-order indices of mask[i] > threshold (ideal.py:199 thresholds the resized segmentation) into idx,
 *   their number into *n_selected (host) -- synchronises the stream, the caller sizes the level's arrays with it;
 * pnx_gather_rows_f64: dst (n_sel, c) = src[idx, :] (signal rows / start values of the fitted voxels, ideal.py:211-216);
 * pnx_scatter_rows_t_f64: the level's parameter map (n_total, k), zero outside the fitted voxels, from the solver's
 *   parameter-major estimates popt (k, n_sel) (ideal.py:243-252); idx NULL = every voxel in order;
 * pnx_row_ss_tot_f64: sum_j (y_ij - mean_i)^2 per row, the SS_tot of R^2 (fitters/base.py:179-183).
 * The last three only enqueue.
 */
PNX_API int pnx_mask_select_f64(const double *mask, int64_t n, double threshold, int64_t *idx, int64_t *n_selected, int device,
                        void *stream);
PNX_API int pnx_gather_rows_f64(const double *src, int64_t c, const int64_t *idx, int64_t n_sel, double *dst, int device, void *stream);
PNX_API int pnx_scatter_rows_t_f64(const double *popt, const int64_t *idx, int64_t n_sel, int k, int64_t n_total, double *pmap, int device,
                           void *stream);
PNX_API int pnx_row_ss_tot_f64(const double *y, int64_t n, int c, double *out, int device, void *stream);

/*
 * Bulk copies between pageable host arrays and device buffers -- what torch's tensor.to(device) / tensor.cpu() (or a plain
 * hipMemcpy) do for the callers that keep a volume resident across calls (the IDEAL level driver: fitters/ideal.py:226-259
 * holds image, masks and maps in host arrays; here they live in HBM and cross PCIe once each way).  The range is cut into
 * 32 MiB pieces (PNX_COPY_PIECE_MB) copied by `threads` host threads (0 = PNX_COPY_THREADS, default 4) on their own streams, a
 * download touches its destination pages first.  Both synchronise `stream` before they start and return when the bytes have
 * landed.
 */
PNX_API int pnx_upload(void *dst_device, const void *src_host, int64_t bytes, int device, void *stream, int threads);
PNX_API int pnx_download(void *dst_host, const void *src_device, int64_t bytes, int device, void *stream, int threads);

/*
 * Per-label column sums of an (n, c) row matrix and the rows per label: the reduction SegmentationWiseFitter performs with a
 * boolean gather + np.mean per label before it fits one row per label (fitters/segmentationwise.py:101-123).  labels[i] in
 * [0, n_labels) is the row's label POSITION (np.unique order); rows with a label outside that range are skipped.
 * sums (n_labels, c), counts (n_labels).  Deterministic (fixed summation order, no atomics).  mem: host pointers (the rows are
 * uploaded with pnx_upload's threaded copy) or device pointers; n_labels * (c + 1) <= 8192.  Synchronises the stream.
 */
PNX_API int pnx_label_sums_f64(const double *rows, const int32_t *labels, int64_t n, int c, int n_labels, double *sums, int64_t *counts,
                       int mem, int device, void *stream);

/*
 * Residual / Jacobian / normal-equation sweep at given parameters (one pass of the LM inner loop as a
 * standalone, HBM-streaming kernel): for every voxel reads y (n_b) and params (n_all), writes
 * cost = 0.5*||r||^2, g = J^T r (n_all) and the upper triangle of J^T J (n_all(n_all+1)/2).
 * Device pointers only.  T = float (f32) or double (f64).  1 <= n_b <= PNX_MAX_BVALUES for both (PNX_ERR_INVALID beyond): the
 * tile of a block lives in LDS, so the generic kernel runs 256 threads per block up to 78 b-values in f64 (any count in f32)
 * and 128 from 79 to 128; 16 and 32 b-values with a 16-byte aligned y take full-tile instantiations.
 *   y (n_vox, n_b); params (n_all, n_vox); out_cost (n_vox); out_g (n_all, n_vox); out_jtj (n_tri, n_vox)
 */
PNX_API int pnx_sweep_f32(int model, int64_t n_vox, int n_b, const float *b_host, const float *y, const float *params,
                  float *out_cost, float *out_g, float *out_jtj, int device, void *stream);
PNX_API int pnx_sweep_f64(int model, int64_t n_vox, int n_b, const double *b_host, const double *y, const double *params,
                  double *out_cost, double *out_g, double *out_jtj, int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PNX_H */
