// pnx_api.hip -- the C ABI declared in include/pnx.h (host side: argument checks, staging, launches).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pnx_curvefit_f32_kernel.hpp"
#include "pnx_curvefit_kernel.hpp"
#include "pnx_grid.hpp"
#include "pnx_grid_args.hpp"
#include "pnx_grid_class.hpp"
#include "pnx_grid_posterior.hpp"
#include "pnx_grid_refine.hpp"
#include "pnx_grid_rician.hpp"
#include "pnx_grid_marginal.hpp"
#include "pnx_grid_mrf.hpp"
#include "pnx_grid_tmrf.hpp"
#include "pnx_grid_prior.hpp"
#include "pnx_host_pipeline.hpp"
#include "pnx_launch.hpp"
#include "pnx_loglin.hpp"
#include "pnx_nnls.hpp"
#include "pnx_peel.hpp"
#include "pnx_predict.hpp"
#include "pnx_simplex.hpp"
#include "pnx_varpro.hpp"
#include "pnx_varpro_class.hpp"
#include "pnx_varpro_logmrf.hpp"
#include "pnx_varpro_mrf.hpp"
#include "pnx_varpro_marginal.hpp"
#include "pnx_varpro_posterior.hpp"
#include "pnx_varpro_prior.hpp"

namespace pnx {

static thread_local char g_err[512] = "";

int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    char tmp[sizeof(g_err)];  // the format arguments may point into g_err (a message passed on from another thread)
    vsnprintf(tmp, sizeof(tmp), fmt, ap);
    va_end(ap);
    memcpy(g_err, tmp, sizeof(g_err));
    return code;
}
const char *last_error_text() { return g_err; }

struct DeviceInfo {
    bool ok = false;
    int cus = 0;
    // ring of work-queue counters so that asynchronous (device-mode) calls never share one
    unsigned long long *queues = nullptr;
    int next_queue = 0;
};
static constexpr int kQueueRing = 256;
static std::mutex g_mu;
static DeviceInfo g_dev[64];

static int get_device(int device, DeviceInfo **out) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return set_error(PNX_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n || device >= 64) return set_error(PNX_ERR_INVALID, "device %d out of range (%d visible)", device, n);
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceInfo &d = g_dev[device];
    if (!d.ok) {
        hipDeviceProp_t prop;
        PNX_HIP(hipGetDeviceProperties(&prop, device));
        d.cus = prop.multiProcessorCount;
        PNX_HIP(hipSetDevice(device));
        PNX_HIP(hipMalloc(&d.queues, sizeof(unsigned long long) * kQueueRing));
        d.ok = true;
    }
    *out = &d;
    return PNX_OK;
}

// get_device, and the calling thread bound to it
static int use_device(int device, DeviceInfo **out) {
    if (int rc = get_device(device, out)) return rc;
    PNX_HIP(hipSetDevice(device));
    return PNX_OK;
}

static unsigned long long *next_queue(DeviceInfo *d) {
    std::lock_guard<std::mutex> lk(g_mu);
    unsigned long long *q = d->queues + d->next_queue;
    d->next_queue = (d->next_queue + 1) % kQueueRing;
    return q;
}

// RAII device buffer for the host-staging path
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t bytes) {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 8);
        if (e != hipSuccess) return set_error(PNX_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        return PNX_OK;
    }
};


// ---- host-staging pipeline: pnx_host_pipeline.hpp on the HIP runtime ------------------------------------------
struct HipBackend {
    typedef hipStream_t stream_t;
    typedef hipEvent_t event_t;
    static bool bind_device(int device) { return hipSetDevice(device) == hipSuccess; }
    // kernel streams at the lowest priority: hardware queues are pooled per priority, so a copy never sits in a queue
    // behind a chunk's kernel (see curvefit_streamed)
    static bool stream_create(stream_t *s, bool kernel) {
        int prio_least = 0, prio_greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) return false;
        const int prio_other = prio_least > 0 ? 0 : prio_greatest;
        return hipStreamCreateWithPriority(s, hipStreamNonBlocking, kernel ? prio_least : prio_other) == hipSuccess;
    }
    static void stream_destroy(stream_t s) { (void)hipStreamDestroy(s); }
    static bool stream_sync(stream_t s) { return hipStreamSynchronize(s) == hipSuccess; }
    static bool event_create(event_t *e) { return hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess; }
    static void event_destroy(event_t e) { (void)hipEventDestroy(e); }
    static bool event_record(event_t e, stream_t s) { return hipEventRecord(e, s) == hipSuccess; }
    static bool event_sync(event_t e) { return hipEventSynchronize(e) == hipSuccess; }
};
typedef PipeOpsT<hipStream_t> PipeOps;

static int run_pipeline(int n_chunks, int n_slots, int k_streams, int touchers, int device, hipStream_t user_stream,
                        const PipeOps &ops) {
    return run_pipeline_t<HipBackend>(n_chunks, n_slots, k_streams, touchers, device, user_stream, ops, dev_getenv("PNX_HOST_TRACE") != nullptr);
}

// write one byte per page of [p, p + bytes): first-touch faults taken here, in parallel with the running kernel,
// instead of serially inside the D2H copy.  Only bytes inside the range are written (the range is this chunk's own
// slice of a result array, about to be overwritten by its D2H copy).
static void touch_pages(void *p, size_t bytes) {
    if (!p || !bytes) return;
    volatile char *c = (volatile char *)p;
    const uintptr_t a = (uintptr_t)p;
    c[0] = 0;
    for (size_t off = (4096 - (a & 4095)) & 4095; off < bytes; off += 4096) c[off] = 0;
}

// the environment helpers are shared by the translation units (pnx_internal.hpp)
int env_int(const char *name, int dflt, int lo, int hi) {
    const char *e = getenv(name);
    if (!e) return dflt;
    const long v = atol(e);
    return v < lo ? lo : (v > hi ? hi : (int)v);
}
const char *dev_getenv(const char *name) {
    static const bool enabled = [] {
        const char *e = getenv("PNX_ENABLE_TEST_HOOKS");
        return e && e[0] == '1' && e[1] == 0;
    }();
    return enabled ? getenv(name) : nullptr;
}
int dev_env_int(const char *name, int dflt, int lo, int hi) { return dev_getenv(name) ? env_int(name, dflt, lo, hi) : dflt; }

// Helper threads of a host-array call.  One call uses an upload thread, one or two download threads and two page-touch
// helpers; the plugin's n_gpus = N (one call per device at once) and callers with several volumes in flight multiply that,
// on a CPU share of 16 cores per GPU.  The page-touch helpers only pay off while cores are idle: with two calls in flight each
// gets one, with three or more none (the download threads touch their own pages then); PNX_HOST_TOUCHERS / _OUT_THREADS
// set explicitly win.
static std::atomic<int> g_host_calls(0);
struct HostCallGuard {
    int in_flight;
    HostCallGuard() : in_flight(g_host_calls.fetch_add(1) + 1) {}
    ~HostCallGuard() { g_host_calls.fetch_sub(1); }
    int touchers() const { return getenv("PNX_HOST_TOUCHERS") ? env_int("PNX_HOST_TOUCHERS", 2, 0, 8) : (in_flight >= 3 ? 0 : (in_flight == 2 ? 1 : 2)); }
    int out_threads() const { return getenv("PNX_STREAM_OUT_THREADS") ? env_int("PNX_STREAM_OUT_THREADS", 2, 1, 4) : (in_flight >= 4 ? 1 : 2); }
};

struct Carver {  // hands out 256-byte aligned pieces of one device slab
    char *base = nullptr;
    size_t off = 0;
    void *take(size_t bytes) {
        void *p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    }
};

static int model_n_params(int model) {
    switch (model) {
    case PNX_MODEL_MONO: return 2;
    case PNX_MODEL_BI_REDUCED: return 3;
    case PNX_MODEL_BI_S0: return 4;
    case PNX_MODEL_BI_FULL: return 4;
    case PNX_MODEL_TRI_REDUCED: return 5;
    case PNX_MODEL_TRI_S0: return 6;
    case PNX_MODEL_TRI_FULL: return 6;
    }
    return -1;
}

typedef int (*launch_fn)(int, int, const CurvefitArgs *, int, void *);
static launch_fn g_launch[7] = {pnx_launch_curvefit_m0, pnx_launch_curvefit_m1, pnx_launch_curvefit_m2,
                                pnx_launch_curvefit_m3, pnx_launch_curvefit_m4, pnx_launch_curvefit_m5,
                                pnx_launch_curvefit_m6};

// what a streamed launch adds to the kernel arguments (CurvefitArgs::ctl ...); phase 2 = covariance epilogue only
struct StreamLaunch {
    StreamCtl *ctl = nullptr;
    unsigned int *host_flags = nullptr;
    int granule_shift = 0;
    unsigned int spins = 0;
    int phase = 0;
};

static int curvefit_device(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y_d,
                           const double *p0, const double *lo, const double *hi, const double *fixed, double *popt_d,
                           double *pcov_d, int8_t *status_d, int32_t *nfev_d, double *cost_d, DeviceInfo *dev,
                           hipStream_t stream, const StreamLaunch *sl = nullptr, const int32_t *order = nullptr) {
    CurvefitArgs a;
    memset(&a, 0, sizeof(a));
    if (sl) {
        a.ctl = sl->ctl;
        a.host_flags = sl->host_flags;
        a.granule_shift = sl->granule_shift;
        a.stream_spins = sl->spins;
        a.phase = sl->phase;
    }
    a.team = dev_env_int("PNX_CF_TEAM", 1, 0, 1);  // test hook: 0 keeps a drained wave's last voxel in its one lane (same bits, slower tail)
    a.order = sl ? nullptr : order;  // device-mode calls only (pnx_curvefit_opts::queue_order): a streamed launch completes its granules in index order
    a.y = y_d;
    a.popt = popt_d;
    a.pcov = pcov_d;
    a.status = status_d;
    a.nfev = nfev_d;
    a.cost = cost_d;
    a.n_vox = n_vox;
    a.n_b = o->n_b;
    a.per_voxel = o->per_voxel_p0_bounds;
    a.fixed_per_voxel = o->fixed_per_voxel;
    a.max_nfev = o->max_nfev > 0 ? o->max_nfev : 100 * o->n_free;  // least_squares: max_nfev=None -> 100*n
    a.n_fixed = o->n_fixed;
    a.t1_mode = o->t1_mode;
    a.tr = o->tr;
    a.tm = o->tm;
    a.ftol = o->ftol;
    a.xtol = o->xtol;
    a.gtol = o->gtol;
    for (int k = 0; k < o->n_free; ++k) a.free_idx[k] = o->free_idx[k];
    for (int k = 0; k < o->n_fixed; ++k) a.fixed_idx[k] = o->fixed_idx[k];
    for (int i = 0; i < o->n_b; ++i) a.b[i] = b[i];
    a.absolute_sigma = o->absolute_sigma != 0;
    a.use_sigma = o->sigma != nullptr;
    if (o->sigma)
        for (int i = 0; i < o->n_b; ++i) a.w[i] = 1.0 / o->sigma[i];  // transform = 1.0 / sigma (a zero sigma gives the reference's "Residuals are not finite" failure)
    if (o->per_voxel_p0_bounds) {
        a.p0 = p0;
        a.lo = lo;
        a.hi = hi;
    } else {
        for (int k = 0; k < o->n_free; ++k) {
            a.p0s[k] = p0[k];
            a.los[k] = lo[k];
            a.his[k] = hi[k];
        }
    }
    if (o->n_fixed) {
        if (o->fixed_per_voxel)
            a.fixed = fixed;
        else
            for (int k = 0; k < o->n_fixed; ++k) a.fixeds[k] = fixed[k];
    }
    if (a.phase != 2) {
        a.queue = next_queue(dev);
        PNX_HIP(hipMemsetAsync(a.queue, 0, sizeof(unsigned long long), stream));
    }
    return g_launch[o->model](o->n_free, o->jac_mode, &a, dev->cus, (void *)stream);
}

static int check_curvefit_opts(const pnx_curvefit_opts *o) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    int n_all = model_n_params(o->model);
    if (n_all < 0) return set_error(PNX_ERR_INVALID, "unknown model %d", o->model);
    if (o->t1_mode < 0 || o->t1_mode > 2) return set_error(PNX_ERR_INVALID, "t1_mode %d", o->t1_mode);
    if (o->t1_mode) n_all += 1;
    if (o->n_b < 1 || o->n_b > PNX_MAX_BVALUES) return set_error(PNX_ERR_INVALID, "n_b=%d out of range [1,%d]", o->n_b, PNX_MAX_BVALUES);
    if (o->n_free < 1 || o->n_fixed < 0 || o->n_free + o->n_fixed != n_all)
        return set_error(PNX_ERR_INVALID, "n_free=%d + n_fixed=%d != %d parameters of model %d", o->n_free, o->n_fixed, n_all, o->model);
    bool seen[PNX_MAX_PARAMS] = {false};
    for (int k = 0; k < o->n_free; ++k) {
        const int j = o->free_idx[k];
        if (j < 0 || j >= n_all || seen[j] || (k && j <= o->free_idx[k - 1]))
            return set_error(PNX_ERR_INVALID, "free_idx must be ascending, unique positions in [0,%d)", n_all);
        seen[j] = true;
    }
    for (int k = 0; k < o->n_fixed; ++k) {
        const int j = o->fixed_idx[k];
        if (j < 0 || j >= n_all || seen[j]) return set_error(PNX_ERR_INVALID, "fixed_idx overlaps free_idx or is out of range");
        seen[j] = true;
    }
    if (o->jac_mode != PNX_JAC_FD && o->jac_mode != PNX_JAC_ANALYTIC) return set_error(PNX_ERR_INVALID, "jac_mode %d", o->jac_mode);
    if (o->jac_mode == PNX_JAC_FD && o->n_fixed)
        return set_error(PNX_ERR_UNSUPPORTED,
                         "finite-difference Jacobian with fixed parameters: the reference uses the analytic Jacobian "
                         "there (curvefit.py:274-288); pass PNX_JAC_ANALYTIC");
    if (!(o->ftol >= 0) || !(o->xtol >= 0) || !(o->gtol >= 0)) return set_error(PNX_ERR_INVALID, "tolerances must be >= 0");
    return PNX_OK;
}

}  // namespace pnx

using namespace pnx;

extern "C" {

int pnx_version(void) { return PNX_VERSION_MAJOR * 100 + PNX_VERSION_MINOR; }

int pnx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pnx_last_error(char *buf, int n) {
    const int len = (int)strlen(g_err);
    if (buf && n > 0) {
        strncpy(buf, g_err, (size_t)n - 1);
        buf[n - 1] = 0;
    }
    return len;
}

int pnx_model_n_params(int model) {
    const int n = model_n_params(model);
    return n < 0 ? set_error(PNX_ERR_INVALID, "unknown model %d", model) : n;
}

}  // extern "C"

// element-wise conversion between the storage type of an _f32 entry point and the fp64 the kernels compute in
template <typename S, typename D> __global__ void cvt_kernel(const S *__restrict__ src, D *__restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = (D)src[i];
}
template <typename S, typename D> static int cvt(const S *src, D *dst, size_t n, hipStream_t st) {
    if (!n) return PNX_OK;
    size_t blocks = (n + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL((cvt_kernel<S, D>), dim3((unsigned)blocks), dim3(256), 0, st, src, dst, n);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

// stream-ordered scratch for the device-pointer _f32 path
struct AsyncBuf {
    void *p = nullptr;
    hipStream_t st = nullptr;
    int alloc(size_t bytes, hipStream_t s) {
        st = s;
        hipError_t e = hipMallocAsync(&p, bytes ? bytes : 8, s);
        if (e != hipSuccess) return set_error(PNX_ERR_NOMEM, "hipMallocAsync(%zu): %s", bytes, hipGetErrorString(e));
        return PNX_OK;
    }
    ~AsyncBuf() {
        if (p) (void)hipFreeAsync(p, st);
    }
};

// ---- the staging steps of a call, each written once as a loop over its ArrayTable (pnx_host_pipeline.hpp) ------------
// Device buffers of an ArrayTable: the fp64 working copy the kernels read or write (dev) and the buffer the caller's array is
// copied to or from (xfer: a float buffer beside it for a widened array, the same memory otherwise).
struct DevSet {
    void *dev[ArrayTable::kMax] = {};
    void *xfer[ArrayTable::kMax] = {};
    double *d(int k) const { return (double *)dev[k]; }
};
// Staged: every buffer of a host-array call for `cap` voxels.  Results: the outputs only, fp64 (the deferred hand-over's batch).
// CallerDevice: PNX_MEM_DEVICE calls -- the caller's arrays from voxel v0 on are the transfer buffers; only the fp64 copies of
// widened arrays are carved.
enum class Carve { Staged, Results, CallerDevice };
static void carve(Carver &cv, const ArrayTable &A, size_t cap, DevSet &D, Carve mode = Carve::Staged, size_t v0 = 0) {
    for (int k = 0; k < A.n; ++k) {
        const HostArray &a = A.a[k];
        D.dev[k] = D.xfer[k] = nullptr;
        if (mode == Carve::CallerDevice) {
            if (!a.host) continue;
            D.xfer[k] = (char *)a.host + v0 * a.w * a.esize;
            D.dev[k] = a.widen ? cv.take(cap * a.w * sizeof(double)) : D.xfer[k];
        } else if ((a.host || a.always) && (a.out || mode == Carve::Staged)) {
            D.dev[k] = cv.take(cap * a.w * (a.widen ? sizeof(double) : a.esize));
            D.xfer[k] = a.widen && a.host && mode == Carve::Staged ? cv.take(cap * a.w * a.esize) : D.dev[k];
        }
    }
}
static int alloc_carved(DevBuf &slab, const ArrayTable &A, size_t cap, DevSet &D) {
    for (int pass = 0; pass < 2; ++pass) {  // pass 0 sizes the slab, pass 1 carves it
        Carver cv;
        cv.base = (char *)slab.p;
        carve(cv, A, cap, D);
        if (pass == 0)
            if (int rc = slab.alloc(cv.off)) return rc;
    }
    return PNX_OK;
}

// Voxels [v0, v0 + c) of a call of nv voxels, at voxel dv0 of the device buffers, whose parameter-major rows lie `stride` voxels
// apart.  An array is `rows` pieces of `len` contiguous elements within the span.
struct Span {
    size_t nv, v0, c, dv0, stride;
    size_t rows(const HostArray &a) const { return a.pmajor ? a.w : 1; }
    size_t len(const HostArray &a) const { return a.pmajor ? c : c * a.w; }
    size_t host_at(const HostArray &a, size_t r) const { return a.pmajor ? r * nv + v0 : v0 * a.w; }
    size_t dev_at(const HostArray &a, size_t r) const { return a.pmajor ? r * stride + dv0 : dv0 * a.w; }
    bool dense(const HostArray &a) const { return !a.pmajor || (stride == c && dv0 == 0); }  // one block on the device
};
static Span ring_span(const std::vector<size_t> &bounds, int k) {  // chunk k of the ring: device stride = the chunk's own count
    const size_t v0 = bounds[(size_t)k], c = bounds[(size_t)k + 1] - v0;
    return Span{bounds.back(), v0, c, 0, c};
}

// fp32 <-> fp64 of the widened arrays of one direction (out: fp64 -> float) within the span
static int convert(const ArrayTable &A, const DevSet &D, const Span &s, bool out, hipStream_t st) {
    for (int k = 0; k < A.n; ++k) {
        const HostArray &a = A.a[k];
        if (!a.widen || !a.host || a.out != out) continue;
        const bool one = s.dense(a);
        for (size_t r = 0; r < (one ? 1 : s.rows(a)); ++r) {
            const size_t at = one ? s.dv0 * a.w : s.dev_at(a, r), n = one ? s.c * a.w : s.len(a);
            const int rc = out ? cvt(D.d(k) + at, (float *)D.xfer[k] + at, n, st) : cvt((const float *)D.xfer[k] + at, D.d(k) + at, n, st);
            if (rc) return rc;
        }
    }
    return PNX_OK;
}
static int widen(const ArrayTable &A, const DevSet &D, const Span &s, hipStream_t st) { return convert(A, D, s, false, st); }
static int narrow(const ArrayTable &A, const DevSet &D, const Span &s, hipStream_t st) { return convert(A, D, s, true, st); }

// H2D of the requested inputs within the span, in table order; widen_each: each piece's conversion right behind its copy
static int h2d(const ArrayTable &A, const DevSet &D, const Span &s, hipStream_t st, bool widen_each = false) {
    for (int k = 0; k < A.n; ++k) {
        const HostArray &a = A.a[k];
        if (a.out || !a.host) continue;
        for (size_t r = 0; r < s.rows(a); ++r) {
            const size_t h = s.host_at(a, r), d = s.dev_at(a, r), n = s.len(a);
            PNX_HIP(hipMemcpyAsync((char *)D.xfer[k] + d * a.esize, (const char *)a.host + h * a.esize, n * a.esize, hipMemcpyHostToDevice, st));
            if (widen_each && a.widen)
                if (int rc = cvt((const float *)D.xfer[k] + d, D.d(k) + d, n, st)) return rc;
        }
    }
    return PNX_OK;
}
static int d2h(const ArrayTable &A, const DevSet &D, const Span &s, hipStream_t st) {
    for (int k = 0; k < A.n; ++k) {
        const HostArray &a = A.a[k];
        if (!a.out || !a.host) continue;
        for (size_t r = 0; r < s.rows(a); ++r)
            PNX_HIP(hipMemcpyAsync((char *)a.host + s.host_at(a, r) * a.esize, (const char *)D.xfer[k] + s.dev_at(a, r) * a.esize,
                                   s.len(a) * a.esize, hipMemcpyDeviceToHost, st));
    }
    return PNX_OK;
}
static void touch(const ArrayTable &A, const Span &s) {  // the result pages of the span (touch_pages)
    for (int k = 0; k < A.n; ++k) {
        const HostArray &a = A.a[k];
        if (!a.out || !a.host) continue;
        for (size_t r = 0; r < s.rows(a); ++r) touch_pages((char *)a.host + s.host_at(a, r) * a.esize, s.len(a) * a.esize);
    }
}

// The chunk ring of a host-array call whose kernels keep no state between chunks: three device slots, `launch` enqueues the
// work of c voxels on the slot's fp64 buffers; widening, narrowing, the page touches and both copies are the table's.
typedef std::function<int(size_t c, const DevSet &D, hipStream_t st)> ChunkLaunch;
static int chunk_ring(const ArrayTable &A, size_t nv, size_t chunk, int max_slots, int k_streams, int touchers, int device,
                      hipStream_t user_stream, const ChunkLaunch &launch) {
    const std::vector<size_t> bounds = chunk_bounds(nv, chunk, true);
    const int n_chunks = (int)bounds.size() - 1;
    const int n_slots = n_chunks < 3 ? n_chunks : max_slots;
    struct Slot {
        DevBuf slab;
        DevSet D;
    };
    std::vector<Slot> slots(n_slots);
    for (auto &S : slots)
        if (int rc = alloc_carved(S.slab, A, nv < chunk ? nv : chunk, S.D)) return rc;
    PipeOps ops;
    ops.h2d = [&](int k, int slot, hipStream_t st) { return h2d(A, slots[slot].D, ring_span(bounds, k), st); };
    ops.launch = [&](int k, int slot, hipStream_t st) -> int {
        const DevSet &D = slots[slot].D;
        const Span s = ring_span(bounds, k);
        int r;
        if ((r = widen(A, D, s, st)) || (r = launch(s.c, D, st))) return r;
        return narrow(A, D, s, st);
    };
    ops.touch = [&](int k) { touch(A, ring_span(bounds, k)); };
    ops.d2h = [&](int k, int slot, hipStream_t st) { return d2h(A, slots[slot].D, ring_span(bounds, k), st); };
    return run_pipeline(n_chunks, n_slots, k_streams, touchers, device, user_stream, ops);
}

// The ring with the settings every host-array call shares: default_chunk voxels per chunk (PNX_HOST_CHUNK), three slots
// (PNX_HOST_SLOTS), two kernel streams (PNX_HOST_KSTREAMS) and the page-touch helpers the calls in flight leave room for.
static int ring_call(const ArrayTable &A, size_t nv, int default_chunk, int device, hipStream_t st, const ChunkLaunch &launch,
                     const HostCallGuard &hg) {
    const size_t chunk = (size_t)dev_env_int("PNX_HOST_CHUNK", default_chunk, 1024, 1 << 26);
    return chunk_ring(A, nv, chunk, dev_env_int("PNX_HOST_SLOTS", 3, 2, 8), dev_env_int("PNX_HOST_KSTREAMS", 2, 1, 4), hg.touchers(), device, st,
                      launch);
}
static int ring_call(const ArrayTable &A, size_t nv, int default_chunk, int device, hipStream_t st, const ChunkLaunch &launch) {
    HostCallGuard hg;  // this call is in flight from here on
    return ring_call(A, nv, default_chunk, device, st, launch, hg);
}

// ---- host-pointer calls, streamed --------------------------------------------------------------------------------
// The chunk ring above launches one persistent kernel per chunk, and every one of them ends in a drain tail (lanes whose
// queue ran dry idle until the slowest voxel of their wave has converged): seven tails cost C3 about 10 ms of its 50.
// The whole call is ONE kernel instead (CurvefitArgs::ctl; per-voxel start values, bounds and fixed maps are uploaded piece by
// piece like the signal):
//   IN    uploads the signal piece by piece and moves the kernel's watermark behind each piece (an 8-byte copy on the
//         same stream, so the data is there before the watermark says so);
//   the kernel's lanes pull voxels in ascending order and wait at the watermark; each wave counts itself out of a granule
//         of voxels once it holds nothing below the granule's end, after a system-scope release of its stores; the wave
//         that completes a granule's count raises a flag in pinned host memory;
//   OUT   polls the flags and, granule by granule, runs the covariance epilogue and downloads the results while the
//         kernel is still fitting.
// The kernel never waits for another kernel, only for the watermark, and that wait is bounded (stream_spins polls, or the
// abort word) so the grid drains whatever happens on the host; a call whose kernel gave up is run again through the ring.
static constexpr int kStreamRetry = -1000;  // internal: "use the chunk ring"

// Device slab, pinned control block and streams of a streamed call.  One set per device is kept between calls (a 2 GB
// hipMalloc / hipFree pair and five stream creations cost 2-3 ms of a 42 ms call); a second call arriving while it is in use
// works on a private set.  pnx_release_staging() frees the kept set.
struct StreamRes {
    void *slab = nullptr;
    size_t slab_bytes = 0;
    void *pin = nullptr;
    size_t pin_bytes = 0;
    std::vector<hipStream_t> s;  // [0] uploads, [1] the persistent kernel (lowest priority), [2..] downloads
    int ensure_slab(size_t bytes) {
        if (slab_bytes >= bytes) return PNX_OK;
        if (slab) (void)hipFree(slab);
        slab = nullptr;
        slab_bytes = 0;
        hipError_t e = hipMalloc(&slab, bytes);
        if (e != hipSuccess) return set_error(PNX_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        slab_bytes = bytes;
        return PNX_OK;
    }
    int ensure_pin(size_t bytes) {
        if (pin_bytes >= bytes) return PNX_OK;
        if (pin) (void)hipHostFree(pin);
        pin = nullptr;
        pin_bytes = 0;
        bytes = (bytes + 65535) & ~(size_t)65535;
        PNX_HIP(hipHostMalloc(&pin, bytes, hipHostMallocCoherent | hipHostMallocMapped));
        pin_bytes = bytes;
        return PNX_OK;
    }
    int ensure_streams(int n) {
        // The runtime multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and a packet queued
        // behind the persistent kernel in ITS hardware queue would wait for the kernel's end -- which, for the upload, never
        // comes (measured: with torch's streams in the process the uploads sat behind the kernel until its poll limit).
        // Queues are pooled per priority, so the kernel's stream gets the lowest priority and a queue of its own; copies and
        // epilogues stay at the default priority (and win the dispatch arbitration against the fit, which is what one wants).
        while ((int)s.size() < n) {
            hipStream_t q = nullptr;
            if (!HipBackend::stream_create(&q, s.size() == 1)) return set_error(PNX_ERR_HIP, "streamed curve fit: stream setup failed");
            s.push_back(q);
        }
        return PNX_OK;
    }
    void release() {
        if (slab) (void)hipFree(slab);
        if (pin) (void)hipHostFree(pin);
        for (auto q : s)
            if (q) (void)hipStreamDestroy(q);
        slab = pin = nullptr;
        slab_bytes = pin_bytes = 0;
        s.clear();
    }
};
static StreamRes g_sres[64];
static bool g_sres_busy[64] = {false};
// A streamed launch whose watermark did not move (another library's streams share the hardware queue of the upload, DESIGN
// section 5) is an environmental condition that will hold for the next call too: the device's host-array fits then go through
// the chunk ring for the next PNX_STREAM_COOLDOWN calls (or until pnx_release_staging) instead of paying the stall every time.
static std::atomic<int> g_stream_cooldown[64];

struct StreamLease {
    StreamRes *r = nullptr;
    int device = 0;
    bool kept = false;
    explicit StreamLease(int dev) : device(dev) {
        std::lock_guard<std::mutex> lk(g_mu);
        if (!g_sres_busy[dev]) {
            g_sres_busy[dev] = true;
            r = &g_sres[dev];
            kept = true;
        } else {
            r = new StreamRes();
        }
    }
    ~StreamLease() {
        if (kept) {
            // the slab stays for the next call (a 2 GB hipMalloc / hipFree pair costs 2-3 ms of a 40 ms call) unless it is larger than
            // PNX_STREAM_CACHE_MB or than a quarter of the HBM that would be free without it: on a device that is shared with a
            // framework's caching allocator the library does not sit on memory others are short of
            const size_t cap = (size_t)env_int("PNX_STREAM_CACHE_MB", 8192, 0, 1 << 20) << 20;
            size_t free_b = 0, total_b = 0;
            const bool crowded = r->slab_bytes && hipMemGetInfo(&free_b, &total_b) == hipSuccess && r->slab_bytes > (free_b + r->slab_bytes) / 4;
            if (r->slab_bytes > cap || crowded) {
                (void)hipFree(r->slab);
                r->slab = nullptr;
                r->slab_bytes = 0;
            }
            std::lock_guard<std::mutex> lk(g_mu);
            g_sres_busy[device] = false;
        } else {
            r->release();
            delete r;
        }
    }
};

// the arrays of a curve fit, in the order of their copies (ArrayTable)
enum { CF_Y, CF_P0, CF_LO, CF_HI, CF_FX, CF_POPT, CF_PCOV, CF_STAT, CF_NFEV, CF_COST };
struct CurvefitShared {  // the b-values and the start values, bounds and fixed values that are not per voxel, as fp64
    double b[PNX_MAX_BVALUES], p0[PNX_MAX_PARAMS], lo[PNX_MAX_PARAMS], hi[PNX_MAX_PARAMS], fx[PNX_MAX_PARAMS];
};
static const double *per_voxel_or(const ArrayTable &A, const DevSet &D, int k, const double *shared) { return A.a[k].host ? D.d(k) : shared; }
// the fit of c voxels on the fp64 buffers of D
static int curvefit_on(const pnx_curvefit_opts *o, const ArrayTable &A, const CurvefitShared &sh, const DevSet &D, size_t c, DeviceInfo *dev,
                       hipStream_t st, const StreamLaunch *sl = nullptr, const int32_t *order = nullptr) {
    return curvefit_device(o, (int64_t)c, sh.b, D.d(CF_Y), per_voxel_or(A, D, CF_P0, sh.p0), per_voxel_or(A, D, CF_LO, sh.lo),
                           per_voxel_or(A, D, CF_HI, sh.hi), per_voxel_or(A, D, CF_FX, sh.fx), D.d(CF_POPT), D.d(CF_PCOV),
                           (int8_t *)D.dev[CF_STAT], (int32_t *)D.dev[CF_NFEV], D.d(CF_COST), dev, st, sl, order);
}

static int curvefit_streamed(const pnx_curvefit_opts *o, const ArrayTable &A, const CurvefitShared &sh, size_t nv, int gshift,
                             DeviceInfo *dev, int device, hipStream_t user_stream, const HostCallGuard &hg) {
    const int n = o->n_free;
    const bool pv = A.a[CF_P0].host != nullptr;  // per-voxel p0 / bounds (n_free, n_vox) each: uploaded piece by piece like the signal
    const size_t G = (size_t)1 << gshift;
    const int n_gran = (int)((nv + G - 1) >> gshift);
    // voxels per upload / watermark step.  Per-voxel p0 / bounds ride along as 3 n row slices per piece: at 128 Ki voxels those
    // are 1 MB copies and the upload (1.57 GB for C3) runs at 36 GB/s and holds the kernel back (53-58 ms, the ring's 55); at
    // 512 Ki 47-50 ms (profiles/stream_pv_probe.py)
    const size_t in_piece = (size_t)dev_env_int("PNX_STREAM_IN_CHUNK", pv ? 1 << 19 : 1 << 17, 1024, 1 << 26);
    const int n_in = (int)((nv + in_piece - 1) / in_piece);
    const bool trace = dev_getenv("PNX_HOST_TRACE") != nullptr;
    const auto t_call = std::chrono::steady_clock::now();
    auto now = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); };
    if (user_stream) PNX_HIP(hipStreamSynchronize(user_stream));

    // device: the whole volume's fp64 working set (+ the float transfer buffers of the float32 entry point) + control block
    StreamLease lease(device);
    StreamRes &res = *lease.r;
    DevSet D;
    StreamCtl *ctl = nullptr;
    const size_t ctl_bytes = sizeof(StreamCtl) + sizeof(unsigned int) * (size_t)n_gran;
    int rc;
    for (int pass = 0; pass < 2; ++pass) {
        Carver c;
        c.base = (char *)res.slab;
        carve(c, A, nv, D);
        ctl = (StreamCtl *)c.take(ctl_bytes);
        if (pass == 0 && res.ensure_slab(c.off)) return kStreamRetry;  // no room for the whole volume: the ring needs three chunks
    }
    // a span of the volume: the device buffers hold the whole volume, parameter-major rows nv voxels apart
    auto span = [&](size_t v0, size_t c) { return Span{nv, v0, c, v0, nv}; };
    auto granule = [&](int g) {
        const size_t v0 = (size_t)g << gshift;
        return span(v0, std::min(G, nv - v0));
    };
    // pinned host: watermark values (source of the 8-byte copies), granule flags (written by the kernel) and, behind them, the
    // abort word the kernel polls while it waits for the watermark (a plain host store raises it: no stream is involved)
    const size_t pin_bytes = sizeof(unsigned long long) * (size_t)(n_in + 1) + sizeof(unsigned int) * (size_t)(n_gran + 1);
    if (res.ensure_pin(pin_bytes)) return kStreamRetry;  // no pinned memory to be had: the ring does without
    memset(res.pin, 0, pin_bytes);
    unsigned long long *wm = (unsigned long long *)res.pin;  // [n_in] (+ one spare word)
    volatile unsigned int *flags = (volatile unsigned int *)(wm + n_in + 1);
    unsigned int *abort_word = (unsigned int *)(flags + n_gran);
    unsigned int *flags_dev = nullptr;
    PNX_HIP(hipHostGetDevicePointer((void **)&flags_dev, (void *)flags, 0));

    // the downloads are pageable copies (the runtime pins the destination pages piece by piece): two threads, each with its
    // own stream and every other granule, keep up with the kernel where one falls 13 ms behind (C3, profiles/stream_sweep.py)
    const int n_out = hg.out_threads();
    if ((rc = res.ensure_streams(2 + n_out))) return rc;
    hipStream_t s_in = res.s[0], s_main = res.s[1];
    PNX_HIP(hipMemsetAsync(ctl, 0, ctl_bytes, s_main));
    PNX_HIP(hipStreamSynchronize(s_main));  // the control block is clean before anybody moves the watermark

    StreamLaunch sl;
    sl.ctl = ctl;
    sl.host_flags = flags_dev;
    sl.granule_shift = gshift;
    sl.spins = (unsigned int)dev_env_int("PNX_STREAM_SPINS", 400000, 1000, 1 << 20);  // ~6 us per poll: 2.4 s, at most ~6 s (the host's own
                                                                                   // watchdog below gives up after PNX_STREAM_STALL_MS)
    sl.phase = 1;
    rc = curvefit_on(o, A, sh, D, nv, dev, s_main, &sl);
    if (rc == PNX_ERR_UNSUPPORTED) return kStreamRetry;  // no streamed instantiation for this combination: the ring has one
    if (rc) return rc;
    const double t_launched = now();

    // the first watermark move, observed on the device: an event behind it on the upload stream
    hipEvent_t ev_first = nullptr;
    PNX_HIP(hipEventCreateWithFlags(&ev_first, hipEventDisableTiming));
    std::atomic<int> first_recorded(0);
    StreamedOps ops;
    ops.bind_device = [&]() { return hipSetDevice(device) == hipSuccess; };
    ops.upload_piece = [&](int i) -> int {
        const size_t v0 = (size_t)i * in_piece, c = std::min(in_piece, nv - v0);
        if (int r = h2d(A, D, span(v0, c), s_in, true)) return r;
        wm[i] = v0 + c;
        PNX_HIP(hipMemcpyAsync(&ctl->ready, &wm[i], sizeof(unsigned long long), hipMemcpyHostToDevice, s_in));
        if (i == 0) {
            PNX_HIP(hipEventRecord(ev_first, s_in));
            first_recorded.store(1);
        }
        return PNX_OK;
    };
    ops.upload_sync = [&]() -> int {
        PNX_HIP(hipStreamSynchronize(s_in));
        return PNX_OK;
    };
    ops.first_piece_landed = [&]() { return first_recorded.load() && hipEventQuery(ev_first) == hipSuccess; };
    ops.granule_ready = [&](int g) { return __atomic_load_n(&flags[g], __ATOMIC_ACQUIRE) != 0; };
    ops.download = [&](int g, int ot) -> int {
        hipStream_t s_out = res.s[2 + ot];
        const Span s = granule(g);
        if (A.a[CF_PCOV].host) {  // the covariance epilogue of the granule
            StreamLaunch s2;
            s2.phase = 2;
            int r = curvefit_device(o, (int64_t)s.c, sh.b, nullptr, per_voxel_or(A, D, CF_P0, sh.p0), per_voxel_or(A, D, CF_LO, sh.lo),
                                    per_voxel_or(A, D, CF_HI, sh.hi), per_voxel_or(A, D, CF_FX, sh.fx), nullptr,
                                    D.d(CF_PCOV) + s.v0 * n * n, (int8_t *)D.dev[CF_STAT] + s.v0, nullptr, D.d(CF_COST) + s.v0, dev, s_out, &s2);
            if (r) return r;
        }
        if (int r = narrow(A, D, s, s_out)) return r;
        if (int r = d2h(A, D, s, s_out)) return r;
        PNX_HIP(hipStreamSynchronize(s_out));
        return PNX_OK;
    };
    ops.touch = [&](int g) { touch(A, granule(g)); };
    ops.abort_kernel = [&]() { __atomic_store_n(abort_word, 1u, __ATOMIC_RELEASE); };
    ops.kernel_state = [&]() -> int {
        const hipError_t e = hipStreamQuery(s_main);
        if (e == hipErrorNotReady) return 0;
        return e == hipSuccess ? 1 : set_error(PNX_ERR_HIP, "streamed curve fit kernel: %s", hipGetErrorString(e));
    };
    ops.kernel_wait = [&]() -> int {
        const hipError_t e = hipStreamSynchronize(s_main);
        return e == hipSuccess ? PNX_OK : set_error(PNX_ERR_HIP, "streamed curve fit kernel: %s", hipGetErrorString(e));
    };
    // a watermark that has not moved this long after the launch will not move: the first piece lands after 0.7 ms (C3), a
    // 512 Ki-voxel piece with per-voxel arrays after 3-4 ms
    const double stall_ms = dev_env_int("PNX_STREAM_STALL_MS", 50, 1, 60000);
    bool stalled = false;
    StreamedTimes times;
    rc = run_streamed(n_in, n_gran, n_out, hg.touchers(), stall_ms, dev_env_int("PNX_STREAM_TEST_DELAY_MS", 0, 0, 60000),
                      ops, &stalled, trace ? &times : nullptr, now);
    (void)hipStreamSynchronize(s_in);  // nothing of this call is left on the kept streams
    (void)hipEventDestroy(ev_first);
    if (rc) return rc;
    StreamCtl head;
    PNX_HIP(hipMemcpy(&head, ctl, sizeof(StreamCtl), hipMemcpyDeviceToHost));
    if (trace) {
        fprintf(stderr, "[pnx stream] %d granules of %zu voxels, %d upload pieces; launched %.2f kernel_done %.2f all_done %.2f ms%s%s\n",
                n_gran, G, n_in, t_launched, times.t_kernel, now(), head.timed_out ? " TIMED OUT" : "", stalled ? " STALLED (gave up)" : "");
        for (int i = 0; i < n_in; i += std::max(1, n_in / 8)) fprintf(stderr, "[pnx stream] upload piece %d enqueued by %.2f ms\n", i, times.t_in[i]);
        for (int g = 0; g < n_gran; g += std::max(1, n_gran / 8))
            fprintf(stderr, "[pnx stream] granule %d complete at %.2f, downloaded by %.2f ms\n", g, times.t_flag[g], times.t_out[g]);
    }
    if (stalled || head.timed_out) {
        g_stream_cooldown[device].store(dev_env_int("PNX_STREAM_COOLDOWN", 32, 0, 1 << 20));
        return kStreamRetry;
    }
    return PNX_OK;
}

// T = double: the fp64 entry point.  T = float: fp32 STORAGE (signal, p0 / bounds / fixed maps in, popt / pcov / cost
// out) with the same fp64 arithmetic -- what the reference does with a float32 image (curve_fit casts ydata to float64).
template <typename T>
static int curvefit_batch(const pnx_curvefit_opts *o, int64_t n_vox, const T *b, const T *y, const T *p0, const T *lo,
                          const T *hi, const T *fixed, T *popt, T *pcov, int8_t *status, int32_t *nfev, T *cost, int mem,
                          int device, void *stream) {
    constexpr bool F32 = sizeof(T) == 4;
    int rc = check_curvefit_opts(o);
    if (rc) return rc;
    if (n_vox < 0) return set_error(PNX_ERR_INVALID, "n_vox < 0");
    if (!b || !p0 || !lo || !hi || !popt || (n_vox && !y)) return set_error(PNX_ERR_INVALID, "NULL data pointer");
    if (o->n_fixed && !fixed) return set_error(PNX_ERR_INVALID, "fixed is NULL but n_fixed=%d", o->n_fixed);
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    if (o->queue_order && mem != PNX_MEM_DEVICE)
        return set_error(PNX_ERR_INVALID, "opts->queue_order is for PNX_MEM_DEVICE calls (a host-array call completes its pieces in index order)");
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    const int n = o->n_free;
    const size_t nv = (size_t)n_vox;
    const bool pv = o->per_voxel_p0_bounds != 0, fpv = o->n_fixed && o->fixed_per_voxel;
    CurvefitShared sh;  // the small shared host arrays as fp64
    for (int i = 0; i < o->n_b; ++i) sh.b[i] = (double)b[i];
    if (!pv)
        for (int k = 0; k < n; ++k) {
            sh.p0[k] = (double)p0[k];
            sh.lo[k] = (double)lo[k];
            sh.hi[k] = (double)hi[k];
        }
    if (o->n_fixed && !fpv)
        for (int k = 0; k < o->n_fixed; ++k) sh.fx[k] = (double)fixed[k];
    ArrayTable A;  // CF_* order; per-voxel p0 / bounds / fixed maps and popt are parameter-major
    A.add(y, sizeof(T), o->n_b, false, F32);
    A.add(pv ? p0 : nullptr, sizeof(T), n, false, F32).pmajor = true;
    A.add(pv ? lo : nullptr, sizeof(T), n, false, F32).pmajor = true;
    A.add(pv ? hi : nullptr, sizeof(T), n, false, F32).pmajor = true;
    A.add(fpv ? fixed : nullptr, sizeof(T), o->n_fixed, false, F32).pmajor = true;
    A.add(popt, sizeof(T), n, true, F32).pmajor = true;
    A.add(pcov, sizeof(T), (size_t)n * n, true, F32);
    A.add(status, 1, 1, true).always = pcov != nullptr;  // the covariance epilogue reads status and cost
    A.add(nfev, sizeof(int32_t), 1, true);
    A.add(cost, sizeof(T), 1, true, F32).always = pcov != nullptr;

    if (mem == PNX_MEM_DEVICE) {
        if (pcov && (!status || !cost))
            return set_error(PNX_ERR_INVALID, "device mode: pcov needs the status and cost outputs too (the covariance "
                                              "epilogue kernel reads them)");
        hipStream_t st = (hipStream_t)stream;
        AsyncBuf scratch;  // float32: fp64 copies of the widened arrays, stream-ordered
        DevSet D;
        const Span all{nv, 0, nv, 0, nv};
        for (int pass = 0; pass < 2; ++pass) {
            Carver cv;
            cv.base = (char *)scratch.p;
            carve(cv, A, nv, D, Carve::CallerDevice);
            if (pass == 0 && cv.off && (rc = scratch.alloc(cv.off, st))) return rc;
        }
        if ((rc = widen(A, D, all, st)) || (rc = curvefit_on(o, A, sh, D, nv, dev, st, nullptr, o->queue_order))) return rc;
        return narrow(A, D, all, st);  // the AsyncBuf destructor enqueues the free behind the conversions
    }

    HostCallGuard hg;  // this call is in flight from here on (helper-thread budget)
    // ---- host staging, streamed: one persistent kernel for the whole volume (curvefit_streamed above)
    {
        // granule = unit of the download (and of the completion flags): 256 Ki voxels for volumes of 2 Mi voxels and more,
        // 128 Ki below (C3: 2^17 41.4-44 ms, 2^18 40.6-43.9 ms, 2^16 and 2^19 42-45 ms; profiles/stream_sweep.py)
        const int gshift = dev_env_int("PNX_STREAM_GRANULE_SHIFT", nv >= ((size_t)1 << 21) ? 18 : 17, 10, 24);
        const size_t per_vox = (size_t)(o->n_b + n + (pcov ? n * n : 0) + 2 + (fpv ? o->n_fixed : 0) + (pv ? 3 * n : 0)) * (F32 ? 12 : 8);
        size_t max_bytes = (size_t)dev_env_int("PNX_STREAM_MAX_MB", 65536, 1, 1 << 20) << 20;
        {   // never more than half of what is free now (plus the kept slab, which would be reused): a volume beyond that goes
            // through the ring's three chunk slots instead of one huge hipMalloc that fails or starves the process
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
                size_t kept = 0;
                {
                    std::lock_guard<std::mutex> lk(g_mu);
                    if (!g_sres_busy[device]) kept = g_sres[device].slab_bytes;
                }
                max_bytes = std::min(max_bytes, free_b / 2 + kept);
            }
        }
        // not for the kernels that need (almost) every register of a lane (pnx_curvefit_inst.hip launch_pv): the copies that
        // feed a streamed kernel have to fit beside it
        const bool tight = n >= 6 || (n >= 4 && o->t1_mode);
        bool cooling = false;
        if (g_stream_cooldown[device].load() > 0) {  // a recent launch on this device stalled: the ring, without trying again
            g_stream_cooldown[device].fetch_sub(1);
            cooling = true;
        }
        if (!cooling && dev_env_int("PNX_HOST_STREAM", 1, 0, 1) && !(pv && o->n_fixed) && !tight && nv > ((size_t)1 << gshift) &&
            nv < ((size_t)1 << 31) && nv * per_vox <= max_bytes) {
            rc = curvefit_streamed(o, A, sh, nv, gshift, dev, device, (hipStream_t)stream, hg);
            if (rc != kStreamRetry) return rc;
            static std::atomic<bool> warned(false);
            if (dev_getenv("PNX_HOST_TRACE") || !warned.exchange(true))
                fprintf(stderr, "[pnx stream] the streamed launch could not be used (no room for the staging slab, or its upload did not "
                                "start within PNX_STREAM_STALL_MS); running the call through the chunk ring, and after a stall the next "
                                "PNX_STREAM_COOLDOWN calls of this device too. With PNX_ENABLE_TEST_HOOKS=1, PNX_HOST_STREAM=0 skips "
                                "the attempt.\n");
        }
    }

    // ---- host staging: chunk ring (run_pipeline above)
    // float32 transfers are half as long per voxel: a larger chunk (fewer drain tails of the persistent kernel) at the same
    // exposed transfer latency -- C3 float32: 86.3 M voxels/s at 768 Ki, 89.8 M at 1 Mi, 82.5 M at 2 Mi (profiles/host_chunk_sweep_f32.py)
    return ring_call(A, nv, F32 ? 1 << 20 : 3 << 18, device, (hipStream_t)stream,
                     [&](size_t c, const DevSet &D, hipStream_t st) { return curvefit_on(o, A, sh, D, c, dev, st); }, hg);
}

// ---- constrained curve fit, f1 + f2 <= 1: pnx_curvefit_simplex_f64 (streaming kernels: pnx_simplex.hip) -----------------
// Two box-bounded fits and a certificate on the device buffers of n_vox voxels.  p0 / lo / hi: (n_free,) host
// arrays, or (n_free, n_vox) device arrays when o->per_voxel_p0_bounds.  status, nfev and cost may be null (scratch then);
// lambda, face and pcov may be null.  Synchronises `st` once, to read the number of violators; nothing else waits.
static int simplex_on(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y_d, const double *p0, const double *lo,
                      const double *hi, double *popt_d, double *pcov_d, int8_t *status_d, int32_t *nfev_d, double *cost_d,
                      double *lambda_d, int8_t *face_d, DeviceInfo *dev, hipStream_t st) {
    const size_t nv = (size_t)n_vox;
    int rc;
    AsyncBuf scratch;  // outputs the caller did not ask for, the violator flags and their compacted indices
    int8_t *status = status_d;
    int32_t *nfev = nfev_d;
    double *cost = cost_d;
    unsigned char *flags = nullptr;
    int64_t *idx = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Carver cv;
        cv.base = (char *)scratch.p;
        idx = (int64_t *)cv.take(nv * sizeof(int64_t));
        if (!cost_d) cost = (double *)cv.take(nv * sizeof(double));
        if (!nfev_d) nfev = (int32_t *)cv.take(nv * sizeof(int32_t));
        if (!status_d) status = (int8_t *)cv.take(nv);
        flags = (unsigned char *)cv.take(nv);
        if (pass == 0 && (rc = scratch.alloc(cv.off, st))) return rc;
    }
    // phase 1: the box-bounded fit of every voxel, covariance included -- the unchanged launch path
    if ((rc = curvefit_device(o, n_vox, b, y_d, p0, lo, hi, nullptr, popt_d, pcov_d, status, nfev, cost, dev, st))) return rc;
    int64_t m = 0;
    int min_nfev = 0;
    if ((rc = simplex_select(popt_d, n_vox, status, nfev, flags, idx, lambda_d, face_d, &m, &min_nfev, st))) return rc;
    if (m == 0) return PNX_OK;  // every box-only minimum is feasible: nothing else runs
    // phase 2: the violators on the face f1 + f2 = 1, i.e. the bi-exponential model with per-voxel start values and bounds
    const bool s0 = o->model == PNX_MODEL_TRI_S0;
    pnx_curvefit_opts o2 = *o;
    o2.model = s0 ? PNX_MODEL_BI_S0 : PNX_MODEL_BI_REDUCED;
    o2.n_free = s0 ? 4 : 3;
    for (int k = 0; k < o2.n_free; ++k) o2.free_idx[k] = k;
    o2.per_voxel_p0_bounds = 1;
    // the kernel takes ONE evaluation limit per launch: what the cheapest violator of this launch has left of max_nfev, at least 1
    const int limit = o->max_nfev > 0 ? o->max_nfev : 100 * o->n_free;
    o2.max_nfev = std::max(1, limit - min_nfev);
    const int n2 = o2.n_free;
    const size_t mm = (size_t)m;
    AsyncBuf face_buf;
    double *y2 = nullptr, *p02 = nullptr, *lo2 = nullptr, *hi2 = nullptr, *popt2 = nullptr, *cost2 = nullptr;
    int32_t *nfev2 = nullptr;
    int8_t *status2 = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        Carver cv;
        cv.base = (char *)face_buf.p;
        y2 = (double *)cv.take(mm * o->n_b * sizeof(double));
        p02 = (double *)cv.take(mm * n2 * sizeof(double));
        lo2 = (double *)cv.take(mm * n2 * sizeof(double));
        hi2 = (double *)cv.take(mm * n2 * sizeof(double));
        popt2 = (double *)cv.take(mm * n2 * sizeof(double));
        cost2 = (double *)cv.take(mm * sizeof(double));
        nfev2 = (int32_t *)cv.take(mm * sizeof(int32_t));
        status2 = (int8_t *)cv.take(mm);
        if (pass == 0 && (rc = face_buf.alloc(cv.off, st))) return rc;
    }
    if ((rc = simplex_gather(o->model, o->n_b, y_d, popt_d, n_vox, idx, m, o->per_voxel_p0_bounds, lo, hi, y2, p02, lo2, hi2, st))) return rc;
    if ((rc = curvefit_device(&o2, m, b, y2, p02, lo2, hi2, nullptr, popt2, nullptr, status2, nfev2, cost2, dev, st))) return rc;
    return simplex_merge(o->model, o->n_b, b, m, idx, y2, popt2, status2, nfev2, cost2, o->per_voxel_p0_bounds, p0, n_vox, popt_d, pcov_d,
                         status, nfev, cost, lambda_d, face_d, st);  // the AsyncBuf destructors enqueue the frees behind it
}

extern "C" int pnx_curvefit_simplex_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, const double *p0,
                                        const double *lo, const double *hi, const double *fixed, double *popt, double *pcov,
                                        int8_t *status, int32_t *nfev, double *cost, double *lambda, int8_t *face, int mem, int device,
                                        void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    if (o->model != PNX_MODEL_TRI_REDUCED && o->model != PNX_MODEL_TRI_S0)
        return set_error(PNX_ERR_INVALID, "the constraint f1 + f2 <= 1 is defined for the reduced tri-exponential models "
                                          "(PNX_MODEL_TRI_REDUCED, PNX_MODEL_TRI_S0), not for model %d", o->model);
    int rc = check_curvefit_opts(o);
    if (rc) return rc;
    // what the constrained fit is not built for: refused by name, never served by the box-only fit behind the caller's back
    if (o->n_fixed || fixed) return set_error(PNX_ERR_UNSUPPORTED, "constrained fit: fixed parameters are not built (the face problem would need its own set)");
    if (o->t1_mode) return set_error(PNX_ERR_UNSUPPORTED, "constrained fit: the T1 / STEAM factor is not built");
    if (o->sigma) return set_error(PNX_ERR_UNSUPPORTED, "constrained fit: sigma is not built");
    if (o->queue_order) return set_error(PNX_ERR_UNSUPPORTED, "constrained fit: queue_order is not built");
    if (n_vox < 0) return set_error(PNX_ERR_INVALID, "n_vox < 0");
    if (!b || !p0 || !lo || !hi || !popt || (n_vox && !y)) return set_error(PNX_ERR_INVALID, "NULL data pointer");
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    const int n = o->n_free;
    const bool pv = o->per_voxel_p0_bounds != 0;
    if (mem == PNX_MEM_DEVICE) {
        if (pcov && (!status || !cost))
            return set_error(PNX_ERR_INVALID, "device mode: pcov needs the status and cost outputs too (the covariance "
                                              "epilogue kernel reads them)");
        return simplex_on(o, n_vox, b, y, p0, lo, hi, popt, pcov, status, nfev, cost, lambda, face, dev, (hipStream_t)stream);
    }
    // host arrays: the chunk ring, both phases per chunk (the streamed single-kernel launch has no place for a second fit)
    CurvefitShared sh;
    for (int i = 0; i < o->n_b; ++i) sh.b[i] = b[i];
    if (!pv)
        for (int k = 0; k < n; ++k) {
            sh.p0[k] = p0[k];
            sh.lo[k] = lo[k];
            sh.hi[k] = hi[k];
        }
    enum { SX_LAMBDA = CF_COST + 1, SX_FACE };
    ArrayTable A;  // CF_* order, then the two outputs of the certificate
    A.add(y, sizeof(double), o->n_b, false);
    A.add(pv ? p0 : nullptr, sizeof(double), n, false).pmajor = true;
    A.add(pv ? lo : nullptr, sizeof(double), n, false).pmajor = true;
    A.add(pv ? hi : nullptr, sizeof(double), n, false).pmajor = true;
    A.add(nullptr, sizeof(double), 0, false).pmajor = true;
    A.add(popt, sizeof(double), n, true).pmajor = true;
    A.add(pcov, sizeof(double), (size_t)n * n, true);
    A.add(status, 1, 1, true).always = true;  // the classification reads status, the merge adds to nfev
    A.add(nfev, sizeof(int32_t), 1, true).always = true;
    A.add(cost, sizeof(double), 1, true).always = pcov != nullptr;
    A.add(lambda, sizeof(double), 1, true);
    A.add(face, 1, 1, true);
    return ring_call(A, (size_t)n_vox, 3 << 18, device, (hipStream_t)stream, [&](size_t c, const DevSet &D, hipStream_t st) {
        return simplex_on(o, (int64_t)c, sh.b, D.d(CF_Y), per_voxel_or(A, D, CF_P0, sh.p0), per_voxel_or(A, D, CF_LO, sh.lo),
                          per_voxel_or(A, D, CF_HI, sh.hi), D.d(CF_POPT), D.d(CF_PCOV), (int8_t *)D.dev[CF_STAT], (int32_t *)D.dev[CF_NFEV],
                          D.d(CF_COST), D.d(SX_LAMBDA), (int8_t *)D.dev[SX_FACE], dev, st);
    });
}

// ---- fp32 arithmetic: pnx_curvefit_fast_f32 (kernel: pnx_curvefit_f32_kernel.hpp, launch: pnx_curvefit_f32.hip) ---------
extern "C" int pnx_launch_curvefit_f32(int model, const pnx::f32::CurvefitF32Args *args, int cus, void *stream);

// the fit of n_vox voxels on float device buffers; shared p0 / bounds come from the host arrays p0 / lo / hi
static int curvefit_f32_device(const pnx_curvefit_opts *o, int64_t n_vox, const float *b, const float *y_d, const float *p0, const float *lo,
                               const float *hi, float *popt_d, float *pcov_d, int8_t *status_d, int32_t *nfev_d, float *cost_d,
                               DeviceInfo *dev, hipStream_t stream) {
    f32::CurvefitF32Args a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.popt = popt_d;
    a.pcov = pcov_d;
    a.status = status_d;
    a.nfev = nfev_d;
    a.cost = cost_d;
    a.n_vox = n_vox;
    a.n_b = o->n_b;
    a.per_voxel = o->per_voxel_p0_bounds;
    a.max_nfev = o->max_nfev > 0 ? o->max_nfev : 100 * o->n_free;  // least_squares: max_nfev=None -> 100*n
    // tolerances below fp32 resolution cannot be honoured: the floors of include/pnx.h (measured: DESIGN.md 4.1b)
    a.ftol = (float)std::max(o->ftol, 4.0 * (double)f32::kEpsF);
    a.xtol = (float)std::max(o->xtol, (double)f32::kEpsF);
    a.gtol = (float)o->gtol;  // no floor: see include/pnx.h
    for (int i = 0; i < o->n_b; ++i) a.b[i] = b[i];
    if (o->per_voxel_p0_bounds) {
        a.p0 = p0;
        a.lo = lo;
        a.hi = hi;
    } else {
        for (int k = 0; k < o->n_free; ++k) {
            a.p0s[k] = p0[k];
            a.los[k] = lo[k];
            a.his[k] = hi[k];
        }
    }
    a.queue = next_queue(dev);
    PNX_HIP(hipMemsetAsync(a.queue, 0, sizeof(unsigned long long), stream));
    return pnx_launch_curvefit_f32(o->model, &a, dev->cus, (void *)stream);
}

extern "C" int pnx_curvefit_fast_f32(const pnx_curvefit_opts *o, int64_t n_vox, const float *b, const float *y, const float *p0,
                                     const float *lo, const float *hi, const float *fixed, float *popt, float *pcov, int8_t *status,
                                     int32_t *nfev, float *cost, int mem, int device, void *stream) {
    int rc = check_curvefit_opts(o);
    if (rc) return rc;
    // what the fp32 kernel is not built for: refused by name, never served by the fp64 kernel behind the caller's back
    if (o->jac_mode == PNX_JAC_FD)
        return set_error(PNX_ERR_UNSUPPORTED, "fp32 arithmetic: SciPy's 2-point step (1.5e-8) is below fp32 resolution; pass PNX_JAC_ANALYTIC");
    if (o->n_fixed || fixed) return set_error(PNX_ERR_UNSUPPORTED, "fp32 arithmetic: fixed parameters are not built (use pnx_curvefit_batch_f32)");
    if (o->t1_mode) return set_error(PNX_ERR_UNSUPPORTED, "fp32 arithmetic: the T1 / STEAM factor is not built (use pnx_curvefit_batch_f32)");
    if (o->sigma) return set_error(PNX_ERR_UNSUPPORTED, "fp32 arithmetic: sigma is not built (use pnx_curvefit_batch_f32)");
    if (o->queue_order) return set_error(PNX_ERR_UNSUPPORTED, "fp32 arithmetic: queue_order is not built (use pnx_curvefit_batch_f32)");
    if (n_vox < 0) return set_error(PNX_ERR_INVALID, "n_vox < 0");
    if (!b || !p0 || !lo || !hi || !popt || (n_vox && !y)) return set_error(PNX_ERR_INVALID, "NULL data pointer");
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    const int n = o->n_free;
    const size_t nv = (size_t)n_vox;
    const bool pv = o->per_voxel_p0_bounds != 0;
    if (mem == PNX_MEM_DEVICE) {
        if (pcov && (!status || !cost))
            return set_error(PNX_ERR_INVALID, "device mode: pcov needs the status and cost outputs too (the covariance "
                                              "epilogue kernel reads them)");
        return curvefit_f32_device(o, n_vox, b, y, p0, lo, hi, popt, pcov, status, nfev, cost, dev, (hipStream_t)stream);
    }
    // host arrays: the chunk ring on float buffers (nothing is widened: the kernel reads and writes float)
    ArrayTable A;  // CF_* order without the fixed maps' content; per-voxel p0 / bounds and popt are parameter-major
    A.add(y, sizeof(float), o->n_b, false);
    A.add(pv ? p0 : nullptr, sizeof(float), n, false).pmajor = true;
    A.add(pv ? lo : nullptr, sizeof(float), n, false).pmajor = true;
    A.add(pv ? hi : nullptr, sizeof(float), n, false).pmajor = true;
    A.add(nullptr, sizeof(float), 0, false).pmajor = true;
    A.add(popt, sizeof(float), n, true).pmajor = true;
    A.add(pcov, sizeof(float), (size_t)n * n, true);
    A.add(status, 1, 1, true).always = pcov != nullptr;  // the covariance epilogue reads status and cost
    A.add(nfev, sizeof(int32_t), 1, true);
    A.add(cost, sizeof(float), 1, true).always = pcov != nullptr;
    return ring_call(A, nv, 1 << 20, device, (hipStream_t)stream, [&](size_t c, const DevSet &D, hipStream_t st) {
        auto f = [&](int k) { return (float *)D.dev[k]; };
        return curvefit_f32_device(o, (int64_t)c, b, f(CF_Y), pv ? f(CF_P0) : p0, pv ? f(CF_LO) : lo, pv ? f(CF_HI) : hi, f(CF_POPT), f(CF_PCOV),
                                   (int8_t *)D.dev[CF_STAT], (int32_t *)D.dev[CF_NFEV], f(CF_COST), dev, st);
    });
}

// ---- log-linear mono-exponential fit: pnx_loglinear_f64 / _f32 (kernel: pnx_loglin.hip, argument checks: pnx_loglin_args.hpp) ---
// T = double or float: the storage type on both sides of the kernel, which reads and writes it directly (nothing is widened).
template <typename T>
static int loglinear(int64_t n_vox, int n_b, const T *b, const uint8_t *use, int weighting, int n_reweight, int clip, const T *lo,
                     const T *hi, const T *y, T *params, T *pcov, int8_t *status, int32_t *n_used, T *ss_res, int mem, int device,
                     void *stream) {
    LogLinOpts o;
    int rc = loglin_check_args<T>(n_vox, n_b, b, use, weighting, n_reweight, clip, lo, hi, y, params, mem, &o);
    if (rc) return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (mem == PNX_MEM_DEVICE) return loglinear_device<T>(o, n_vox, y, params, pcov, status, n_used, ss_res, st);
    enum { LL_Y, LL_P, LL_PCOV, LL_STAT, LL_NUSED, LL_SS };
    ArrayTable A;  // the parameters are parameter-major, as popt of the curve fit
    A.add(y, sizeof(T), (size_t)n_b, false);
    A.add(params, sizeof(T), 2, true).pmajor = true;
    A.add(pcov, sizeof(T), 4, true);
    A.add(status, 1, 1, true);
    A.add(n_used, sizeof(int32_t), 1, true);
    A.add(ss_res, sizeof(T), 1, true);
    return ring_call(A, (size_t)n_vox, sizeof(T) == 4 ? 1 << 20 : 3 << 18, device, st, [&](size_t n, const DevSet &D, hipStream_t s) {
        return loglinear_device<T>(o, (int64_t)n, (const T *)D.dev[LL_Y], (T *)D.dev[LL_P], (T *)D.dev[LL_PCOV], (int8_t *)D.dev[LL_STAT],
                                   (int32_t *)D.dev[LL_NUSED], (T *)D.dev[LL_SS], s);
    });
}

// ---- exponential peeling: pnx_peel_f64 / _f32 (kernel: pnx_peel.hip, argument checks: pnx_peel_args.hpp) -----------------------
// T = double or float: the storage type on both sides of the kernel, which reads and writes it directly (nothing is widened).
template <typename T>
static int peel(int model, int64_t n_vox, int n_b, const T *b, const uint8_t *use, int weighting, int clip, const T *lo, const T *hi,
                const T *fallback, const T *y, T *params, int8_t *status, int32_t *n_used, T *ss_res, int mem, int device, void *stream) {
    PeelOpts o;
    int rc = peel_check_args<T>(model, n_vox, n_b, b, use, weighting, clip, lo, hi, fallback, y, params, mem, &o);
    if (rc) return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (mem == PNX_MEM_DEVICE) return peel_device<T>(o, n_vox, y, params, status, n_used, ss_res, st);
    enum { PL_Y, PL_P, PL_STAT, PL_NUSED, PL_SS };
    ArrayTable A;  // the parameters and n_used are parameter-major, as popt of the curve fit
    A.add(y, sizeof(T), (size_t)n_b, false);
    A.add(params, sizeof(T), (size_t)o.n_params, true).pmajor = true;
    A.add(status, 1, 1, true);
    A.add(n_used, sizeof(int32_t), (size_t)o.n_stage, true).pmajor = true;
    A.add(ss_res, sizeof(T), 1, true);
    return ring_call(A, (size_t)n_vox, sizeof(T) == 4 ? 1 << 20 : 3 << 18, device, st, [&](size_t n, const DevSet &D, hipStream_t s) {
        return peel_device<T>(o, (int64_t)n, (const T *)D.dev[PL_Y], (T *)D.dev[PL_P], (int8_t *)D.dev[PL_STAT], (int32_t *)D.dev[PL_NUSED],
                              (T *)D.dev[PL_SS], s);
    });
}

extern "C" {
int pnx_release_staging(int device) {
    if (device < 0 || device >= 64) return set_error(PNX_ERR_INVALID, "device %d out of range", device);
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_sres_busy[device]) return set_error(PNX_ERR_INVALID, "device %d: a streamed call is using the staging set", device);
    g_stream_cooldown[device].store(0);  // and the next host-array fit may try the streamed launch again
    int cur = 0;
    if (g_sres[device].slab || g_sres[device].pin || !g_sres[device].s.empty()) {
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(device);
        g_sres[device].release();
        (void)hipSetDevice(cur);
    }
    // the slab set the block-kernel NNLS plans of this device share (pnx_nnls.hpp): freed when no plan holds it, kept otherwise
    (void)nnls_shared_slabs_trim(device);
    return PNX_OK;
}

int pnx_curvefit_batch_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y,
                           const double *p0, const double *lo, const double *hi, const double *fixed, double *popt,
                           double *pcov, int8_t *status, int32_t *nfev, double *cost, int mem, int device,
                           void *stream) {
    return curvefit_batch<double>(o, n_vox, b, y, p0, lo, hi, fixed, popt, pcov, status, nfev, cost, mem, device, stream);
}

int pnx_curvefit_batch_f32(const pnx_curvefit_opts *o, int64_t n_vox, const float *b, const float *y, const float *p0,
                           const float *lo, const float *hi, const float *fixed, float *popt, float *pcov, int8_t *status,
                           int32_t *nfev, float *cost, int mem, int device, void *stream) {
    return curvefit_batch<float>(o, n_vox, b, y, p0, lo, hi, fixed, popt, pcov, status, nfev, cost, mem, device, stream);
}

int pnx_curvefit_predict_f64(const pnx_curvefit_opts *o, int64_t n_vox, int n_x, const double *x, const double *params,
                             const double *fixed, const double *y, double *pred, double *ss_res, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    if (n_x < 1 || n_x > PNX_MAX_BVALUES) return set_error(PNX_ERR_INVALID, "n_x=%d out of range [1,%d]", n_x, PNX_MAX_BVALUES);
    // the fields predict reads, checked as the fit checks them: n_b, jac_mode and the tolerances are not looked at
    pnx_curvefit_opts c = *o;
    c.n_b = n_x;
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    if (!pred && !ss_res) return set_error(PNX_ERR_INVALID, "pred and ss_res are both NULL");
    if (ss_res && !y) return set_error(PNX_ERR_INVALID, "ss_res needs the signal y");
    if (n_vox < 0 || !x || (n_vox && !params)) return set_error(PNX_ERR_INVALID, "NULL data pointer");
    if (c.n_fixed && !fixed) return set_error(PNX_ERR_INVALID, "fixed is NULL but n_fixed=%d", c.n_fixed);
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!ss_res) y = nullptr;
    if (mem == PNX_MEM_DEVICE) return model_predict_device(&c, n_vox, n_x, x, params, fixed, y, pred, ss_res, st);
    const bool fpv = c.n_fixed && c.fixed_per_voxel;
    enum { PR_P, PR_FX, PR_Y, PR_PRED, PR_SS };
    ArrayTable A;
    A.add(params, sizeof(double), c.n_free, false).pmajor = true;
    A.add(fpv ? fixed : nullptr, sizeof(double), c.n_fixed, false).pmajor = true;
    A.add(y, sizeof(double), n_x, false);
    A.add(pred, sizeof(double), n_x, true);
    A.add(ss_res, sizeof(double), 1, true);
    HostCallGuard hg;
    return chunk_ring(A, (size_t)n_vox, (size_t)dev_env_int("PNX_PREDICT_HOST_CHUNK", 3 << 18, 1024, 1 << 22), 3, 2, hg.touchers(), device, st,
                      [&](size_t n, const DevSet &D, hipStream_t s) {
                          return model_predict_device(&c, (int64_t)n, n_x, x, D.d(PR_P), fpv ? D.d(PR_FX) : fixed, D.d(PR_Y), D.d(PR_PRED),
                                                      D.d(PR_SS), s);
                      });
}

// ---- per-voxel start values from a dictionary search (kernels: pnx_grid.hip, argument checks: pnx_grid_args.hpp) ------------
int pnx_curvefit_grid_start_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                double *p0_out, int32_t *best, double *cost, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    // the fields the search reads, checked as the fit checks them: jac_mode and the tolerances are not looked at
    pnx_curvefit_opts c = *o;
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    int s0_row = -1;
    if ((rc = grid_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, p0_out, mem, &s0_row))) return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf;  // the dictionary: built once per call, stream-ordered, freed behind the work that reads it
    GridDict D;
    if ((rc = dict_buf.alloc(grid_dict_bytes(c.n_free, n_atoms, c.n_b), st))) return rc;
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, s0_row, dict_buf.p, &D, st))) return rc;
    if (mem == PNX_MEM_DEVICE) return grid_match_device(D, n_vox, y, p0_out, best, cost, dev->cus, st);
    // host arrays: the chunk ring; its streams read the dictionary, so it is complete before the first chunk starts
    PNX_HIP(hipStreamSynchronize(st));
    enum { GS_Y, GS_P0, GS_BEST, GS_COST };
    ArrayTable A;
    A.add(y, sizeof(double), c.n_b, false);
    A.add(p0_out, sizeof(double), c.n_free, true).pmajor = true;
    A.add(best, sizeof(int32_t), 1, true);
    A.add(cost, sizeof(double), 1, true);
    return ring_call(A, (size_t)n_vox, 3 << 18, device, st, [&](size_t n, const DevSet &S, hipStream_t s) {
        return grid_match_device(D, (int64_t)n, S.d(GS_Y), S.d(GS_P0), (int32_t *)S.dev[GS_BEST], S.d(GS_COST), dev->cus, s);
    });
}

// ---- posterior over the dictionary (kernels: pnx_grid_posterior.hip, argument checks: pnx_grid_posterior_args.hpp) ----------
int pnx_curvefit_grid_posterior_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                    const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                    const double *log_prior, double noise_sd, double *mean, double *sd, int32_t *map_atom, double *map_p,
                                    double *log_evidence, double *ess, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridPosteriorHost H;
    if ((rc = grid_posterior_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, mean, mem, &H)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf;  // built once per call, stream-ordered, freed behind the work that reads them
    GridDict D;
    GridPosterior P;
    if ((rc = dict_buf.alloc(grid_dict_bytes(c.n_free, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(grid_posterior_bytes(c.n_free, n_atoms), st))) return rc;
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, H.s0_row, dict_buf.p, &D, st))) return rc;
    if ((rc = grid_posterior_prepare(D, H, log_prior, noise_sd, post_buf.p, &P, st))) return rc;
    if (mem == PNX_MEM_DEVICE) return grid_posterior_device(D, P, n_vox, y, mean, sd, map_atom, map_p, log_evidence, ess, dev->cus, st);
    PNX_HIP(hipStreamSynchronize(st));  // the ring's streams read the dictionary: complete before the first chunk starts
    enum { GP_Y, GP_MEAN, GP_SD, GP_ATOM, GP_MAPP, GP_LOGEV, GP_ESS };
    ArrayTable A;
    A.add(y, sizeof(double), c.n_b, false);
    A.add(mean, sizeof(double), c.n_free, true).pmajor = true;
    A.add(sd, sizeof(double), c.n_free, true).pmajor = true;
    A.add(map_atom, sizeof(int32_t), 1, true);
    A.add(map_p, sizeof(double), c.n_free, true).pmajor = true;
    A.add(log_evidence, sizeof(double), 1, true);
    A.add(ess, sizeof(double), 1, true);
    return ring_call(A, (size_t)n_vox, 3 << 18, device, st, [&](size_t n, const DevSet &S, hipStream_t s) {
        return grid_posterior_device(D, P, (int64_t)n, S.d(GP_Y), S.d(GP_MEAN), S.d(GP_SD), (int32_t *)S.dev[GP_ATOM], S.d(GP_MAPP), S.d(GP_LOGEV),
                                     S.d(GP_ESS), dev->cus, s);
    });
}

// ---- posterior under a Rician likelihood (kernels: pnx_grid_rician.hip, argument checks: pnx_grid_rician_args.hpp) -------------
int pnx_curvefit_grid_posterior_rician_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                           const double *atoms, const double *fixed, const double *lo, const double *hi,
                                           const double *log_prior, double noise_sd, double *mean, double *sd, int32_t *map_atom,
                                           double *map_p, double *log_evidence, double *ess, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridPosteriorHost H;
    if ((rc = grid_rician_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, log_prior, noise_sd, mean, mem, &H))) return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf;  // built once per call, stream-ordered, freed behind the work that reads them
    GridDict D;
    GridPosterior P;
    if ((rc = dict_buf.alloc(grid_dict_bytes(c.n_free, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(grid_posterior_bytes(c.n_free, n_atoms), st))) return rc;
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, -1, dict_buf.p, &D, st))) return rc;
    if ((rc = grid_posterior_prepare(D, H, log_prior, noise_sd, post_buf.p, &P, st))) return rc;
    if (mem == PNX_MEM_DEVICE) return grid_rician_posterior_device(D, P, n_vox, y, mean, sd, map_atom, map_p, log_evidence, ess, dev->cus, st);
    PNX_HIP(hipStreamSynchronize(st));  // the ring's streams read the dictionary: complete before the first chunk starts
    enum { GP_Y, GP_MEAN, GP_SD, GP_ATOM, GP_MAPP, GP_LOGEV, GP_ESS };
    ArrayTable A;
    A.add(y, sizeof(double), c.n_b, false);
    A.add(mean, sizeof(double), c.n_free, true).pmajor = true;
    A.add(sd, sizeof(double), c.n_free, true).pmajor = true;
    A.add(map_atom, sizeof(int32_t), 1, true);
    A.add(map_p, sizeof(double), c.n_free, true).pmajor = true;
    A.add(log_evidence, sizeof(double), 1, true);
    A.add(ess, sizeof(double), 1, true);
    return ring_call(A, (size_t)n_vox, 3 << 18, device, st, [&](size_t n, const DevSet &S, hipStream_t s) {
        return grid_rician_posterior_device(D, P, (int64_t)n, S.d(GP_Y), S.d(GP_MEAN), S.d(GP_SD), (int32_t *)S.dev[GP_ATOM], S.d(GP_MAPP),
                                            S.d(GP_LOGEV), S.d(GP_ESS), dev->cus, s);
    });
}

int pnx_log_i0e_f64(int64_t n, const double *z, double *out, int mem, int device, void *stream) {
    int rc = log_i0e_check_args(n, z, out, mem);
    if (rc) return rc;
    if (n == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (mem == PNX_MEM_DEVICE) return log_i0e_device(n, z, out, st);
    enum { LI_Z, LI_OUT };
    ArrayTable A;
    A.add(z, sizeof(double), 1, false);
    A.add(out, sizeof(double), 1, true);
    return ring_call(A, (size_t)n, 3 << 18, device, st,
                     [&](size_t m, const DevSet &S, hipStream_t s) { return log_i0e_device((int64_t)m, S.d(LI_Z), S.d(LI_OUT), s); });
}

// ---- a fine grid per voxel (kernel: pnx_grid_refine.hip, argument checks: pnx_grid_refine_args.hpp) -------------------------------
int pnx_curvefit_grid_refine_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, const double *fixed,
                                 const double *lo, const double *hi, int project_amplitude, double noise_sd, const int32_t *n_points,
                                 const double *centre, const double *half_width, double *mean, double *sd, double *map_p, double *ess,
                                 double *log_norm, double *edge_mass, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridRefineHost H;
    if ((rc = grid_refine_check_args(&c, n_vox, b, y, fixed, lo, hi, project_amplitude, noise_sd, n_points, centre, half_width, mean, mem, &H)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (mem == PNX_MEM_DEVICE)
        return grid_refine_device(&c, H, n_vox, b, y, fixed, lo, hi, noise_sd, n_points, centre, half_width, mean, sd, map_p, ess, log_norm,
                                  edge_mass, dev->cus, st);
    enum { GR_Y, GR_CENTRE, GR_HW, GR_MEAN, GR_SD, GR_MAPP, GR_ESS, GR_LOGN, GR_EDGE };
    ArrayTable A;
    A.add(y, sizeof(double), c.n_b, false);
    A.add(centre, sizeof(double), c.n_free, false).pmajor = true;
    A.add(half_width, sizeof(double), c.n_free, false).pmajor = true;
    A.add(mean, sizeof(double), c.n_free, true).pmajor = true;
    A.add(sd, sizeof(double), c.n_free, true).pmajor = true;
    A.add(map_p, sizeof(double), c.n_free, true).pmajor = true;
    A.add(ess, sizeof(double), 1, true);
    A.add(log_norm, sizeof(double), 1, true);
    A.add(edge_mass, sizeof(double), c.n_free, true).pmajor = true;
    return ring_call(A, (size_t)n_vox, 3 << 18, device, st, [&](size_t n, const DevSet &S, hipStream_t s) {
        return grid_refine_device(&c, H, (int64_t)n, b, S.d(GR_Y), fixed, lo, hi, noise_sd, n_points, S.d(GR_CENTRE), S.d(GR_HW), S.d(GR_MEAN),
                                  S.d(GR_SD), S.d(GR_MAPP), S.d(GR_ESS), S.d(GR_LOGN), S.d(GR_EDGE), dev->cus, s);
    });
}

// ---- the prior over the dictionary learned from the volume (kernels: pnx_grid_prior.hip, argument checks: pnx_grid_prior_args.hpp)
int pnx_curvefit_grid_prior_em_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                   const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                   const double *log_prior, double noise_sd, int n_iter, double pseudo_count, double rel_tol,
                                   double *log_prior_out, double *loglik, int *n_iter_done, int64_t *n_eff, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridPosteriorHost H;
    if ((rc = grid_prior_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, n_iter, pseudo_count,
                                    rel_tol, log_prior_out, mem, &H)))
        return rc;
    const int n_adm = grid_prior_start(n_atoms, log_prior, H.log_prior_norm, log_prior_out);  // the start, normalised
    if (loglik) loglik[0] = 0.0;
    if (n_vox == 0) {
        grid_prior_report(n_iter, 0, 0, loglik, n_iter_done, n_eff);
        return PNX_OK;
    }
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, work_buf, y_buf;  // stream-ordered, freed behind the work that reads them
    GridDict D;
    GridPosterior P;
    GridPriorWork W;
    if ((rc = dict_buf.alloc(grid_dict_bytes(c.n_free, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(grid_posterior_bytes(c.n_free, n_atoms), st))) return rc;
    if ((rc = work_buf.alloc(grid_prior_bytes(n_vox, n_atoms, dev->cus), st))) return rc;
    if (mem == PNX_MEM_HOST) {  // every pass of every iteration reads the same signals: one upload, kept for the call
        const size_t bytes = (size_t)n_vox * c.n_b * sizeof(double);
        if (y_buf.alloc(bytes, st) != PNX_OK)
            return set_error(PNX_ERR_NOMEM, "grid prior: no device memory for the %zu bytes of y (%lld voxels x %d), which stay resident for all "
                                            "iterations: learn the prior from a sub-sample of the voxels", bytes, (long long)n_vox, c.n_b);
        if ((rc = pnx_upload(y_buf.p, y, (int64_t)bytes, device, st, 0))) return rc;
        y = (const double *)y_buf.p;
    }
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, H.s0_row, dict_buf.p, &D, st))) return rc;
    if ((rc = grid_posterior_prepare(D, H, log_prior_out, noise_sd, post_buf.p, &P, st))) return rc;
    grid_prior_carve(n_vox, n_atoms, dev->cus, work_buf.p, &W);
    std::vector<double> trace((size_t)n_iter + 1, 0.0);
    GridPriorStats stats = {0.0, 0};
    int done = 0;
    for (int t = 0;; ++t) {  // trace[t]: the log-likelihood under the prior before update t, the returned prior's at t = done
        if ((rc = grid_prior_normalise(D, P, n_vox, y, W, st))) return rc;
        PNX_HIP(hipMemcpyAsync(&stats, W.stats, sizeof(stats), hipMemcpyDeviceToHost, st));
        PNX_HIP(hipStreamSynchronize(st));
        trace[t] = stats.loglik;
        done = t;
        if (stats.n_finite == 0 || t == n_iter || grid_prior_converged(trace.data(), t, rel_tol)) break;
        if ((rc = grid_prior_update(D, P, n_vox, y, W, pseudo_count, n_adm, st))) return rc;
    }
    PNX_HIP(hipMemcpyAsync(log_prior_out, P.lp, (size_t)n_atoms * sizeof(double), hipMemcpyDeviceToHost, st));
    PNX_HIP(hipStreamSynchronize(st));
    if (loglik)
        for (int t = 0; t <= done; ++t) loglik[t] = trace[t];
    grid_prior_report(n_iter, done, stats.n_finite, loglik, n_iter_done, n_eff);
    return PNX_OK;
}

// ---- one prior row per segmentation label (kernels: pnx_grid_class.hip, argument checks: pnx_grid_class_args.hpp) ------------
int pnx_curvefit_grid_posterior_classes_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                            const double *atoms, const double *fixed, const double *lo, const double *hi,
                                            int project_amplitude, int n_classes, const int32_t *labels, const double *log_prior,
                                            double noise_sd, double *mean, double *sd, int32_t *map_atom, double *map_p,
                                            double *log_evidence, double *ess, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridPosteriorHost H;
    GridClassHost K;
    if ((rc = grid_class_posterior_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, n_classes, labels, log_prior,
                                              noise_sd, mean, mem, &H, &K)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, table_buf;  // built once per call, stream-ordered, freed behind the work that reads them
    GridDict D;
    GridPosterior P;
    GridClassTable T;
    if ((rc = dict_buf.alloc(grid_dict_bytes(c.n_free, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(grid_posterior_bytes(c.n_free, n_atoms), st))) return rc;
    if ((rc = table_buf.alloc(grid_class_table_bytes(n_classes, n_atoms), st))) return rc;
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, H.s0_row, dict_buf.p, &D, st))) return rc;
    if ((rc = grid_posterior_prepare(D, H, nullptr, noise_sd, post_buf.p, &P, st))) return rc;  // theta about H.centre, the floor
    if ((rc = grid_class_table_prepare(D, K, n_classes, log_prior, table_buf.p, &T, st))) return rc;
    if (mem == PNX_MEM_DEVICE)
        return grid_class_posterior_device(D, P, T, n_vox, y, labels, mean, sd, map_atom, map_p, log_evidence, ess, dev->cus, st);
    PNX_HIP(hipStreamSynchronize(st));  // the ring's streams read the dictionary: complete before the first chunk starts
    enum { GC_Y, GC_LAB, GC_MEAN, GC_SD, GC_ATOM, GC_MAPP, GC_LOGEV, GC_ESS };
    ArrayTable A;
    A.add(y, sizeof(double), c.n_b, false);
    A.add(labels, sizeof(int32_t), 1, false);
    A.add(mean, sizeof(double), c.n_free, true).pmajor = true;
    A.add(sd, sizeof(double), c.n_free, true).pmajor = true;
    A.add(map_atom, sizeof(int32_t), 1, true);
    A.add(map_p, sizeof(double), c.n_free, true).pmajor = true;
    A.add(log_evidence, sizeof(double), 1, true);
    A.add(ess, sizeof(double), 1, true);
    return ring_call(A, (size_t)n_vox, 3 << 18, device, st, [&](size_t n, const DevSet &S, hipStream_t s) {
        return grid_class_posterior_device(D, P, T, (int64_t)n, S.d(GC_Y), (const int32_t *)S.dev[GC_LAB], S.d(GC_MEAN), S.d(GC_SD),
                                           (int32_t *)S.dev[GC_ATOM], S.d(GC_MAPP), S.d(GC_LOGEV), S.d(GC_ESS), dev->cus, s);
    });
}

int pnx_curvefit_grid_prior_em_classes_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                           const double *atoms, const double *fixed, const double *lo, const double *hi,
                                           int project_amplitude, int n_classes, const int32_t *labels, const double *log_prior,
                                           double noise_sd, int n_iter, double pseudo_count, double rel_tol, double *log_prior_out,
                                           double *loglik, double *loglik_class, int *n_iter_done, int64_t *n_eff, int mem, int device,
                                           void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridPosteriorHost H;
    GridClassHost K;
    if ((rc = grid_class_prior_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, n_classes, labels, log_prior,
                                          noise_sd, n_iter, pseudo_count, rel_tol, log_prior_out, mem, &H, &K)))
        return rc;
    grid_class_start(n_classes, n_atoms, log_prior, K, log_prior_out);  // the start, every row normalised
    for (int cl = 0; cl < n_classes; ++cl) K.norm[cl] = 0.0;           // and so is the table every pass reads
    if (loglik) loglik[0] = 0.0;
    if (loglik_class)
        for (int cl = 0; cl < n_classes; ++cl) loglik_class[cl] = 0.0;
    if (n_vox == 0) {
        grid_class_report(n_iter, 0, n_classes, nullptr, loglik, loglik_class, n_iter_done, n_eff);
        return PNX_OK;
    }
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, table_buf, work_buf, y_buf, lab_buf;  // stream-ordered, freed behind the work that reads them
    GridDict D;
    GridPosterior P;
    GridClassTable T;
    GridClassWork W;
    if ((rc = dict_buf.alloc(grid_dict_bytes(c.n_free, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(grid_posterior_bytes(c.n_free, n_atoms), st))) return rc;
    if ((rc = table_buf.alloc(grid_class_table_bytes(n_classes, n_atoms), st))) return rc;
    if ((rc = work_buf.alloc(grid_class_prior_bytes(n_vox, n_atoms, n_classes, dev->cus), st))) return rc;
    if (mem == PNX_MEM_HOST) {  // every pass of every iteration reads the same signals and labels: one upload, kept for the call
        const size_t bytes = (size_t)n_vox * c.n_b * sizeof(double), lbytes = (size_t)n_vox * sizeof(int32_t);
        if (y_buf.alloc(bytes, st) != PNX_OK || lab_buf.alloc(lbytes, st) != PNX_OK)
            return set_error(PNX_ERR_NOMEM, "grid prior: no device memory for the %zu bytes of y and labels (%lld voxels x %d), which stay "
                                            "resident for all iterations: learn the prior from a sub-sample of the voxels",
                             bytes + lbytes, (long long)n_vox, c.n_b);
        if ((rc = pnx_upload(y_buf.p, y, (int64_t)bytes, device, st, 0))) return rc;
        if ((rc = pnx_upload(lab_buf.p, labels, (int64_t)lbytes, device, st, 0))) return rc;
        y = (const double *)y_buf.p;
        labels = (const int32_t *)lab_buf.p;
    }
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, H.s0_row, dict_buf.p, &D, st))) return rc;
    if ((rc = grid_posterior_prepare(D, H, nullptr, noise_sd, post_buf.p, &P, st))) return rc;
    if ((rc = grid_class_table_prepare(D, K, n_classes, log_prior_out, table_buf.p, &T, st))) return rc;
    grid_class_prior_carve(n_vox, n_atoms, n_classes, dev->cus, work_buf.p, &W);
    std::vector<double> trace((size_t)n_iter + 1, 0.0), trace_class(((size_t)n_iter + 1) * n_classes, 0.0);
    GridClassStats stats;
    memset(&stats, 0, sizeof(stats));
    int done = 0;
    for (int t = 0;; ++t) {  // trace[t]: the log-likelihood under the table before update t, the returned table's at t = done
        if ((rc = grid_class_prior_normalise(D, P, T, n_vox, y, labels, W, st))) return rc;
        PNX_HIP(hipMemcpyAsync(&stats, W.stats, sizeof(stats), hipMemcpyDeviceToHost, st));
        PNX_HIP(hipStreamSynchronize(st));
        trace[t] = stats.loglik;
        long long total = 0;
        for (int cl = 0; cl < n_classes; ++cl) {
            trace_class[(size_t)t * n_classes + cl] = stats.loglik_class[cl];
            total += stats.n_finite[cl];
        }
        done = t;
        if (total == 0 || t == n_iter || grid_prior_converged(trace.data(), t, rel_tol)) break;
        if ((rc = grid_class_prior_update(D, P, T, n_vox, y, labels, W, pseudo_count, K.n_adm, st))) return rc;
    }
    PNX_HIP(hipMemcpy2DAsync(log_prior_out, (size_t)n_atoms * sizeof(double), T.lp, (size_t)D.gp * sizeof(double),
                             (size_t)n_atoms * sizeof(double), (size_t)n_classes, hipMemcpyDeviceToHost, st));
    PNX_HIP(hipStreamSynchronize(st));
    for (int t = 0; t <= done; ++t) {
        if (loglik) loglik[t] = trace[t];
        if (loglik_class)
            for (int cl = 0; cl < n_classes; ++cl) loglik_class[(size_t)t * n_classes + cl] = trace_class[(size_t)t * n_classes + cl];
    }
    int64_t finite[kGridMaxClasses];
    for (int cl = 0; cl < n_classes; ++cl) finite[cl] = stats.n_finite[cl];
    grid_class_report(n_iter, done, n_classes, finite, loglik, loglik_class, n_iter_done, n_eff);
    return PNX_OK;
}

// ---- neighbourhood (MRF) prior by coloured mean-field sweeps (kernels: pnx_grid_mrf.hip, argument checks: pnx_grid_mrf_args.hpp)
int pnx_curvefit_grid_neighbour_field_f64(int64_t n_vox, int64_t first, int64_t count, int n_free, int n_nb, const int32_t *neighbours,
                                          const double *mean, const double *centre, const double *precision, double *field_q,
                                          int32_t *field_n, int32_t *flag, int mem, int device, void *stream) {
    int rc = grid_mrf_field_check_args(n_vox, first, count, n_free, n_nb, neighbours, mean, centre, precision, field_q, field_n, mem);
    if (rc) return rc;
    if (n_vox == 0 || count == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    GridMrfFieldArgs a;
    memset(&a, 0, sizeof(a));
    a.n_vox = n_vox;
    a.first = first;
    a.count = count;
    a.n_free = n_free;
    a.n_nb = n_nb;
    for (int k = 0; k < n_free; ++k) {
        a.centre[k] = centre[k];
        a.precision[k] = precision[k];
    }
    if (mem == PNX_MEM_DEVICE) {
        a.nb = neighbours;
        a.mean = mean;
        a.q = field_q;
        a.n = field_n;
        a.flag = flag;
        return grid_mrf_field_device(a, st);
    }
    // host arrays: the table and the means go up whole, the range of every row comes back; the call owns the flag and reports it
    AsyncBuf nb_buf, mean_buf, q_buf, n_buf, flag_buf;
    const size_t nbb = (size_t)n_vox * n_nb * sizeof(int32_t), mb = (size_t)n_free * n_vox * sizeof(double);
    if ((rc = nb_buf.alloc(nbb, st)) || (rc = mean_buf.alloc(mb, st)) || (rc = q_buf.alloc(mb, st)) ||
        (rc = n_buf.alloc((size_t)n_vox * sizeof(int32_t), st)) || (rc = flag_buf.alloc(sizeof(int32_t), st)))
        return rc;
    int32_t host_flag = INT32_MAX;
    if ((rc = pnx_upload(nb_buf.p, neighbours, (int64_t)nbb, device, st, 0))) return rc;
    if ((rc = pnx_upload(mean_buf.p, mean, (int64_t)mb, device, st, 0))) return rc;
    PNX_HIP(hipMemcpyAsync(flag_buf.p, &host_flag, sizeof(int32_t), hipMemcpyHostToDevice, st));
    a.nb = (const int32_t *)nb_buf.p;
    a.mean = (const double *)mean_buf.p;
    a.q = (double *)q_buf.p;
    a.n = (int32_t *)n_buf.p;
    a.flag = (int32_t *)flag_buf.p;
    if ((rc = grid_mrf_field_device(a, st))) return rc;
    for (int k = 0; k < n_free; ++k)
        PNX_HIP(hipMemcpyAsync(field_q + (size_t)k * n_vox + first, a.q + (size_t)k * n_vox + first, (size_t)count * sizeof(double),
                               hipMemcpyDeviceToHost, st));
    PNX_HIP(hipMemcpyAsync(field_n + first, a.n + first, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PNX_HIP(hipMemcpyAsync(&host_flag, flag_buf.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PNX_HIP(hipStreamSynchronize(st));
    if (flag) *flag = host_flag;
    if (host_flag != INT32_MAX)
        return set_error(PNX_ERR_INVALID, "grid neighbour field: neighbours of voxel %d hold an index outside [-1, %lld)", host_flag, (long long)n_vox);
    return PNX_OK;
}

int pnx_curvefit_grid_posterior_field_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                          const double *atoms, const double *fixed, const double *lo, const double *hi,
                                          int project_amplitude, const double *log_prior, double noise_sd, int64_t first, int64_t count,
                                          const double *field_q, const int32_t *field_n, const double *precision, double *mean, double *sd,
                                          int32_t *map_atom, double *map_p, double *log_evidence, double *ess, double *delta_max, int mem,
                                          int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridPosteriorHost H;
    GridMrfHost M;
    if ((rc = grid_mrf_posterior_field_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, first,
                                                  count, field_q, field_n, precision, mean, mem, &H, &M)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, mrf_buf;  // built once per call, stream-ordered, freed behind the work that reads them
    GridDict D;
    GridPosterior P;
    GridMrf F;
    if ((rc = dict_buf.alloc(grid_dict_bytes(c.n_free, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(grid_posterior_bytes(c.n_free, n_atoms), st))) return rc;
    if ((rc = mrf_buf.alloc(grid_mrf_bytes(n_atoms, dev->cus), st))) return rc;
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, H.s0_row, dict_buf.p, &D, st))) return rc;
    if ((rc = grid_posterior_prepare(D, H, log_prior, noise_sd, post_buf.p, &P, st))) return rc;
    if ((rc = grid_mrf_prepare(D, H, M, atoms, precision, dev->cus, mrf_buf.p, &F, st))) return rc;
    return grid_mrf_posterior_device(D, P, F, n_vox, first, count, y, field_q, field_n, mean, sd, map_atom, map_p, log_evidence, ess, delta_max,
                                     false, dev->cus, st);
}

int pnx_curvefit_grid_posterior_mrf_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                        const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                        const double *log_prior, double noise_sd, int n_nb, const int32_t *neighbours, int n_colours,
                                        const int64_t *colour_start, const double *precision, int n_sweeps, double tol, double *mean,
                                        double *sd, int32_t *map_atom, double *map_p, double *log_evidence, double *ess, double *delta,
                                        int *n_sweeps_done, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridPosteriorHost H;
    GridMrfHost M;
    if ((rc = grid_mrf_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, n_nb, neighbours,
                                  n_colours, colour_start, precision, n_sweeps, tol, mean, mem, &H, &M)))
        return rc;
    std::vector<double> trace((size_t)n_sweeps + 1, 0.0);
    if (n_vox == 0) {
        grid_mrf_report(n_sweeps, 0, trace.data(), delta, n_sweeps_done);
        return PNX_OK;
    }
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nf = c.n_free;
    const size_t nv = (size_t)n_vox, pb = (size_t)nf * nv * sizeof(double);
    AsyncBuf dict_buf, post_buf, mrf_buf, q_buf, n_buf, delta_buf, y_buf, nb_buf, out_buf;  // stream-ordered, freed behind the work that reads them
    GridDict D;
    GridPosterior P;
    GridMrf F;
    if ((rc = dict_buf.alloc(grid_dict_bytes(nf, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(grid_posterior_bytes(nf, n_atoms), st))) return rc;
    if ((rc = mrf_buf.alloc(grid_mrf_bytes(n_atoms, dev->cus), st))) return rc;
    if ((rc = q_buf.alloc(pb, st)) || (rc = n_buf.alloc(nv * sizeof(int32_t), st)) || (rc = delta_buf.alloc(((size_t)n_sweeps + 1) * 8, st)))
        return rc;
    double *mean_d = mean, *sd_d = sd, *mapp_d = map_p, *logev_d = log_evidence, *ess_d = ess;
    int32_t *atom_d = map_atom;
    size_t off_sd = 0, off_mapp = 0, off_logev = 0, off_ess = 0, off_atom = 0, out_bytes = 0;
    if (mem == PNX_MEM_HOST) {  // every sweep reads the same signals and table: one upload, kept for the call; the outputs in one buffer
        const size_t yb = nv * c.n_b * sizeof(double), nbb = nv * n_nb * sizeof(int32_t);
        out_bytes = pb;
        if (sd) off_sd = out_bytes, out_bytes += pb;
        if (map_p) off_mapp = out_bytes, out_bytes += pb;
        if (log_evidence) off_logev = out_bytes, out_bytes += nv * 8;
        if (ess) off_ess = out_bytes, out_bytes += nv * 8;
        if (map_atom) off_atom = out_bytes, out_bytes += nv * 4;
        if (y_buf.alloc(yb, st) != PNX_OK || nb_buf.alloc(nbb, st) != PNX_OK || out_buf.alloc(out_bytes, st) != PNX_OK)
            return set_error(PNX_ERR_NOMEM, "grid posterior mrf: no device memory for the %zu bytes of y, neighbours and the outputs (%lld voxels x "
                                            "%d), which stay resident for all sweeps", yb + nbb + out_bytes, (long long)n_vox, c.n_b);
        if ((rc = pnx_upload(y_buf.p, y, (int64_t)yb, device, st, 0))) return rc;
        if ((rc = pnx_upload(nb_buf.p, neighbours, (int64_t)nbb, device, st, 0))) return rc;
        y = (const double *)y_buf.p;
        neighbours = (const int32_t *)nb_buf.p;
        char *ob = (char *)out_buf.p;
        mean_d = (double *)ob;
        sd_d = sd ? (double *)(ob + off_sd) : nullptr;
        mapp_d = map_p ? (double *)(ob + off_mapp) : nullptr;
        logev_d = log_evidence ? (double *)(ob + off_logev) : nullptr;
        ess_d = ess ? (double *)(ob + off_ess) : nullptr;
        atom_d = map_atom ? (int32_t *)(ob + off_atom) : nullptr;
    }
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, H.s0_row, dict_buf.p, &D, st))) return rc;
    if ((rc = grid_posterior_prepare(D, H, log_prior, noise_sd, post_buf.p, &P, st))) return rc;
    if ((rc = grid_mrf_prepare(D, H, M, atoms, precision, dev->cus, mrf_buf.p, &F, st))) return rc;
    // the colouring: no index out of range, no edge inside a colour -- argument errors, found before any sweep
    int32_t flags[2] = {INT32_MAX, INT32_MAX};
    if ((rc = grid_mrf_colour_check_device(n_vox, n_nb, neighbours, n_colours, colour_start, F.flags, st))) return rc;
    PNX_HIP(hipMemcpyAsync(flags, F.flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    PNX_HIP(hipStreamSynchronize(st));
    if (flags[0] != INT32_MAX)
        return set_error(PNX_ERR_INVALID, "grid posterior mrf: neighbours of voxel %d hold an index outside [-1, %lld)", flags[0], (long long)n_vox);
    if (flags[1] != INT32_MAX)
        return set_error(PNX_ERR_INVALID, "grid posterior mrf: voxel %d has a neighbour inside its own colour range (an edge inside a colour: the "
                                          "update would not be coordinate ascent)", flags[1]);
    double *delta_d = (double *)delta_buf.p;
    PNX_HIP(hipMemsetAsync(delta_d, 0, ((size_t)n_sweeps + 1) * 8, st));
    // sweep 0: the plain posterior
    if ((rc = grid_posterior_device(D, P, n_vox, y, mean_d, sd_d, atom_d, mapp_d, logev_d, ess_d, dev->cus, st))) return rc;
    GridMrfFieldArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.nb = neighbours;
    ga.mean = mean_d;
    ga.q = (double *)q_buf.p;
    ga.n = (int32_t *)n_buf.p;
    ga.flag = nullptr;  // checked above
    ga.n_vox = n_vox;
    ga.n_free = nf;
    ga.n_nb = n_nb;
    for (int k = 0; k < nf; ++k) {
        ga.centre[k] = H.centre[k];
        ga.precision[k] = precision[k];
    }
    int done = 0;
    for (int s = 1; s <= n_sweeps; ++s) {
        for (int col = 0; col < n_colours; ++col) {
            ga.first = colour_start[col];
            ga.count = colour_start[col + 1] - colour_start[col];
            if (ga.count == 0) continue;
            if ((rc = grid_mrf_field_device(ga, st))) return rc;
            if ((rc = grid_mrf_posterior_device(D, P, F, n_vox, ga.first, ga.count, y, ga.q, ga.n, mean_d, sd_d, atom_d, mapp_d, logev_d, ess_d,
                                                delta_d + (s - 1), true, dev->cus, st)))
                return rc;
        }
        done = s;
        if (tol > 0.0) {  // the stopping rule needs this sweep's delta on the host; tol = 0 runs all sweeps without a round trip
            PNX_HIP(hipMemcpyAsync(&trace[s - 1], delta_d + (s - 1), 8, hipMemcpyDeviceToHost, st));
            PNX_HIP(hipStreamSynchronize(st));
            if (trace[s - 1] <= tol) break;
        }
    }
    if (n_sweeps > 0) PNX_HIP(hipMemcpyAsync(trace.data(), delta_d, (size_t)n_sweeps * 8, hipMemcpyDeviceToHost, st));
    if (mem == PNX_MEM_HOST) {
        const char *ob = (const char *)out_buf.p;
        PNX_HIP(hipMemcpyAsync(mean, ob, pb, hipMemcpyDeviceToHost, st));
        if (sd) PNX_HIP(hipMemcpyAsync(sd, ob + off_sd, pb, hipMemcpyDeviceToHost, st));
        if (map_p) PNX_HIP(hipMemcpyAsync(map_p, ob + off_mapp, pb, hipMemcpyDeviceToHost, st));
        if (log_evidence) PNX_HIP(hipMemcpyAsync(log_evidence, ob + off_logev, nv * 8, hipMemcpyDeviceToHost, st));
        if (ess) PNX_HIP(hipMemcpyAsync(ess, ob + off_ess, nv * 8, hipMemcpyDeviceToHost, st));
        if (map_atom) PNX_HIP(hipMemcpyAsync(map_atom, ob + off_atom, nv * 4, hipMemcpyDeviceToHost, st));
    }
    PNX_HIP(hipStreamSynchronize(st));
    grid_mrf_report(n_sweeps, done, trace.data(), delta, n_sweeps_done);
    return PNX_OK;
}

// ---- edge-preserving (Student-t) neighbourhood prior (kernels: pnx_grid_tmrf.hip, argument checks: pnx_grid_tmrf_args.hpp)
int pnx_curvefit_grid_neighbour_wfield_f64(int64_t n_vox, int64_t first, int64_t count, int n_free, int n_nb, const int32_t *neighbours,
                                           const double *mean, const double *sd, const double *centre, const double *precision, double dof,
                                           double *field_q, double *field_w, int32_t *field_n, double *edge_weight, int32_t *flag, int mem,
                                           int device, void *stream) {
    int rc = grid_tmrf_field_check_args(n_vox, first, count, n_free, n_nb, neighbours, mean, sd, centre, precision, dof, field_q, field_w,
                                        field_n, mem);
    if (rc) return rc;
    if (n_vox == 0 || count == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    GridTmrfFieldArgs a;
    memset(&a, 0, sizeof(a));
    a.n_vox = n_vox;
    a.first = first;
    a.count = count;
    a.n_free = n_free;
    a.n_nb = n_nb;
    a.dof = dof;
    a.dof_k = dof + grid_tmrf_rows(n_free, precision);
    for (int k = 0; k < n_free; ++k) {
        a.centre[k] = centre[k];
        a.precision[k] = precision[k];
    }
    if (mem == PNX_MEM_DEVICE) {
        a.nb = neighbours;
        a.mean = mean;
        a.sd = sd;
        a.q = field_q;
        a.w = field_w;
        a.n = field_n;
        a.edge = edge_weight;
        a.flag = flag;
        return grid_tmrf_field_device(a, st);
    }
    // host arrays: the table, the means and the sds go up whole, the range of every row comes back; the call owns the flag and reports it
    AsyncBuf nb_buf, mean_buf, sd_buf, q_buf, w_buf, n_buf, e_buf, flag_buf;
    const size_t nbb = (size_t)n_vox * n_nb * sizeof(int32_t), mb = (size_t)n_free * n_vox * sizeof(double);
    const size_t eb = (size_t)n_vox * n_nb * sizeof(double);
    if ((rc = nb_buf.alloc(nbb, st)) || (rc = mean_buf.alloc(mb, st)) || (rc = sd_buf.alloc(mb, st)) || (rc = q_buf.alloc(mb, st)) ||
        (rc = w_buf.alloc((size_t)n_vox * sizeof(double), st)) || (rc = n_buf.alloc((size_t)n_vox * sizeof(int32_t), st)) ||
        (rc = flag_buf.alloc(sizeof(int32_t), st)) || (edge_weight && (rc = e_buf.alloc(eb, st))))
        return rc;
    int32_t host_flag = INT32_MAX;
    if ((rc = pnx_upload(nb_buf.p, neighbours, (int64_t)nbb, device, st, 0))) return rc;
    if ((rc = pnx_upload(mean_buf.p, mean, (int64_t)mb, device, st, 0))) return rc;
    if ((rc = pnx_upload(sd_buf.p, sd, (int64_t)mb, device, st, 0))) return rc;
    PNX_HIP(hipMemcpyAsync(flag_buf.p, &host_flag, sizeof(int32_t), hipMemcpyHostToDevice, st));
    a.nb = (const int32_t *)nb_buf.p;
    a.mean = (const double *)mean_buf.p;
    a.sd = (const double *)sd_buf.p;
    a.q = (double *)q_buf.p;
    a.w = (double *)w_buf.p;
    a.n = (int32_t *)n_buf.p;
    a.edge = edge_weight ? (double *)e_buf.p : nullptr;
    a.flag = (int32_t *)flag_buf.p;
    if ((rc = grid_tmrf_field_device(a, st))) return rc;
    for (int k = 0; k < n_free; ++k)
        PNX_HIP(hipMemcpyAsync(field_q + (size_t)k * n_vox + first, a.q + (size_t)k * n_vox + first, (size_t)count * sizeof(double),
                               hipMemcpyDeviceToHost, st));
    PNX_HIP(hipMemcpyAsync(field_w + first, a.w + first, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st));
    PNX_HIP(hipMemcpyAsync(field_n + first, a.n + first, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (edge_weight)
        PNX_HIP(hipMemcpyAsync(edge_weight + (size_t)first * n_nb, a.edge + (size_t)first * n_nb, (size_t)count * n_nb * sizeof(double),
                               hipMemcpyDeviceToHost, st));
    PNX_HIP(hipMemcpyAsync(&host_flag, flag_buf.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PNX_HIP(hipStreamSynchronize(st));
    if (flag) *flag = host_flag;
    if (host_flag != INT32_MAX)
        return set_error(PNX_ERR_INVALID, "grid neighbour wfield: neighbours of voxel %d hold an index outside [-1, %lld)", host_flag, (long long)n_vox);
    return PNX_OK;
}

int pnx_curvefit_grid_posterior_wfield_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                           const double *atoms, const double *fixed, const double *lo, const double *hi,
                                           int project_amplitude, const double *log_prior, double noise_sd, int64_t first, int64_t count,
                                           const double *field_q, const double *field_w, const double *precision, double *mean, double *sd,
                                           int32_t *map_atom, double *map_p, double *log_evidence, double *ess, double *delta_max, int mem,
                                           int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridPosteriorHost H;
    GridMrfHost M;
    if ((rc = grid_tmrf_posterior_field_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, first,
                                                   count, field_q, field_w, precision, mean, mem, &H, &M)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, mrf_buf;  // built once per call, stream-ordered, freed behind the work that reads them
    GridDict D;
    GridPosterior P;
    GridMrf F;
    if ((rc = dict_buf.alloc(grid_dict_bytes(c.n_free, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(grid_posterior_bytes(c.n_free, n_atoms), st))) return rc;
    if ((rc = mrf_buf.alloc(grid_mrf_bytes(n_atoms, dev->cus), st))) return rc;
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, H.s0_row, dict_buf.p, &D, st))) return rc;
    if ((rc = grid_posterior_prepare(D, H, log_prior, noise_sd, post_buf.p, &P, st))) return rc;
    if ((rc = grid_mrf_prepare(D, H, M, atoms, precision, dev->cus, mrf_buf.p, &F, st))) return rc;
    return grid_tmrf_posterior_device(D, P, F, n_vox, first, count, y, field_q, field_w, mean, sd, map_atom, map_p, log_evidence, ess, delta_max,
                                      false, dev->cus, st);
}

int pnx_curvefit_grid_posterior_tmrf_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                         const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                         const double *log_prior, double noise_sd, int n_nb, const int32_t *neighbours, int n_colours,
                                         const int64_t *colour_start, const double *precision, double dof, int n_sweeps, double tol,
                                         double *mean, double *sd, int32_t *map_atom, double *map_p, double *log_evidence, double *ess,
                                         double *field_w, int32_t *field_n, double *delta, int *n_sweeps_done, int mem, int device,
                                         void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridPosteriorHost H;
    GridMrfHost M;
    if ((rc = grid_tmrf_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, n_nb, neighbours,
                                   n_colours, colour_start, precision, dof, n_sweeps, tol, mean, sd, mem, &H, &M)))
        return rc;
    std::vector<double> trace((size_t)n_sweeps + 1, 0.0);
    if (n_vox == 0) {
        grid_mrf_report(n_sweeps, 0, trace.data(), delta, n_sweeps_done);
        return PNX_OK;
    }
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nf = c.n_free;
    const size_t nv = (size_t)n_vox, pb = (size_t)nf * nv * sizeof(double);
    AsyncBuf dict_buf, post_buf, mrf_buf, q_buf, w_buf, n_buf, delta_buf, y_buf, nb_buf, out_buf;  // stream-ordered, freed behind the work that reads them
    GridDict D;
    GridPosterior P;
    GridMrf F;
    if ((rc = dict_buf.alloc(grid_dict_bytes(nf, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(grid_posterior_bytes(nf, n_atoms), st))) return rc;
    if ((rc = mrf_buf.alloc(grid_mrf_bytes(n_atoms, dev->cus), st))) return rc;
    if ((rc = q_buf.alloc(pb, st)) || (rc = delta_buf.alloc(((size_t)n_sweeps + 1) * 8, st))) return rc;
    const bool stage = mem == PNX_MEM_HOST;
    if ((stage || !field_w) && (rc = w_buf.alloc(nv * sizeof(double), st))) return rc;
    if ((stage || !field_n) && (rc = n_buf.alloc(nv * sizeof(int32_t), st))) return rc;
    double *w_d = (stage || !field_w) ? (double *)w_buf.p : field_w;  // device callers' arrays are written in place
    int32_t *n_d = (stage || !field_n) ? (int32_t *)n_buf.p : field_n;
    double *mean_d = mean, *sd_d = sd, *mapp_d = map_p, *logev_d = log_evidence, *ess_d = ess;
    int32_t *atom_d = map_atom;
    size_t off_sd = 0, off_mapp = 0, off_logev = 0, off_ess = 0, off_atom = 0, out_bytes = 0;
    if (stage) {  // every sweep reads the same signals and table: one upload, kept for the call; the outputs in one buffer
        const size_t yb = nv * c.n_b * sizeof(double), nbb = nv * n_nb * sizeof(int32_t);
        out_bytes = pb;
        off_sd = out_bytes, out_bytes += pb;
        if (map_p) off_mapp = out_bytes, out_bytes += pb;
        if (log_evidence) off_logev = out_bytes, out_bytes += nv * 8;
        if (ess) off_ess = out_bytes, out_bytes += nv * 8;
        if (map_atom) off_atom = out_bytes, out_bytes += nv * 4;
        if (y_buf.alloc(yb, st) != PNX_OK || nb_buf.alloc(nbb, st) != PNX_OK || out_buf.alloc(out_bytes, st) != PNX_OK)
            return set_error(PNX_ERR_NOMEM, "grid posterior tmrf: no device memory for the %zu bytes of y, neighbours and the outputs (%lld voxels x "
                                            "%d), which stay resident for all sweeps", yb + nbb + out_bytes, (long long)n_vox, c.n_b);
        if ((rc = pnx_upload(y_buf.p, y, (int64_t)yb, device, st, 0))) return rc;
        if ((rc = pnx_upload(nb_buf.p, neighbours, (int64_t)nbb, device, st, 0))) return rc;
        y = (const double *)y_buf.p;
        neighbours = (const int32_t *)nb_buf.p;
        char *ob = (char *)out_buf.p;
        mean_d = (double *)ob;
        sd_d = (double *)(ob + off_sd);
        mapp_d = map_p ? (double *)(ob + off_mapp) : nullptr;
        logev_d = log_evidence ? (double *)(ob + off_logev) : nullptr;
        ess_d = ess ? (double *)(ob + off_ess) : nullptr;
        atom_d = map_atom ? (int32_t *)(ob + off_atom) : nullptr;
    }
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, H.s0_row, dict_buf.p, &D, st))) return rc;
    if ((rc = grid_posterior_prepare(D, H, log_prior, noise_sd, post_buf.p, &P, st))) return rc;
    if ((rc = grid_mrf_prepare(D, H, M, atoms, precision, dev->cus, mrf_buf.p, &F, st))) return rc;
    // the colouring: no index out of range, no edge inside a colour -- argument errors, found before any sweep
    int32_t flags[2] = {INT32_MAX, INT32_MAX};
    if ((rc = grid_mrf_colour_check_device(n_vox, n_nb, neighbours, n_colours, colour_start, F.flags, st))) return rc;
    PNX_HIP(hipMemcpyAsync(flags, F.flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    PNX_HIP(hipStreamSynchronize(st));
    if (flags[0] != INT32_MAX)
        return set_error(PNX_ERR_INVALID, "grid posterior tmrf: neighbours of voxel %d hold an index outside [-1, %lld)", flags[0], (long long)n_vox);
    if (flags[1] != INT32_MAX)
        return set_error(PNX_ERR_INVALID, "grid posterior tmrf: voxel %d has a neighbour inside its own colour range (an edge inside a colour: the "
                                          "update would not be coordinate ascent)", flags[1]);
    double *delta_d = (double *)delta_buf.p;
    PNX_HIP(hipMemsetAsync(delta_d, 0, ((size_t)n_sweeps + 1) * 8, st));
    PNX_HIP(hipMemsetAsync(w_d, 0, nv * sizeof(double), st));  // a voxel no sweep updates reports W = 0, n = 0
    PNX_HIP(hipMemsetAsync(n_d, 0, nv * sizeof(int32_t), st));
    // sweep 0: the plain posterior
    if ((rc = grid_posterior_device(D, P, n_vox, y, mean_d, sd_d, atom_d, mapp_d, logev_d, ess_d, dev->cus, st))) return rc;
    GridTmrfFieldArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.nb = neighbours;
    ga.mean = mean_d;
    ga.sd = sd_d;
    ga.q = (double *)q_buf.p;
    ga.w = w_d;
    ga.n = n_d;
    ga.edge = nullptr;
    ga.flag = nullptr;  // checked above
    ga.n_vox = n_vox;
    ga.n_free = nf;
    ga.n_nb = n_nb;
    ga.dof = dof;
    ga.dof_k = dof + grid_tmrf_rows(nf, precision);
    for (int k = 0; k < nf; ++k) {
        ga.centre[k] = H.centre[k];
        ga.precision[k] = precision[k];
    }
    int done = 0;
    for (int s = 1; s <= n_sweeps; ++s) {
        for (int col = 0; col < n_colours; ++col) {
            ga.first = colour_start[col];
            ga.count = colour_start[col + 1] - colour_start[col];
            if (ga.count == 0) continue;
            if ((rc = grid_tmrf_field_device(ga, st))) return rc;
            if ((rc = grid_tmrf_posterior_device(D, P, F, n_vox, ga.first, ga.count, y, ga.q, ga.w, mean_d, sd_d, atom_d, mapp_d, logev_d, ess_d,
                                                 delta_d + (s - 1), true, dev->cus, st)))
                return rc;
        }
        done = s;
        if (tol > 0.0) {  // the stopping rule needs this sweep's delta on the host; tol = 0 runs all sweeps without a round trip
            PNX_HIP(hipMemcpyAsync(&trace[s - 1], delta_d + (s - 1), 8, hipMemcpyDeviceToHost, st));
            PNX_HIP(hipStreamSynchronize(st));
            if (trace[s - 1] <= tol) break;
        }
    }
    if (n_sweeps > 0) PNX_HIP(hipMemcpyAsync(trace.data(), delta_d, (size_t)n_sweeps * 8, hipMemcpyDeviceToHost, st));
    if (stage) {
        const char *ob = (const char *)out_buf.p;
        PNX_HIP(hipMemcpyAsync(mean, ob, pb, hipMemcpyDeviceToHost, st));
        PNX_HIP(hipMemcpyAsync(sd, ob + off_sd, pb, hipMemcpyDeviceToHost, st));
        if (map_p) PNX_HIP(hipMemcpyAsync(map_p, ob + off_mapp, pb, hipMemcpyDeviceToHost, st));
        if (log_evidence) PNX_HIP(hipMemcpyAsync(log_evidence, ob + off_logev, nv * 8, hipMemcpyDeviceToHost, st));
        if (ess) PNX_HIP(hipMemcpyAsync(ess, ob + off_ess, nv * 8, hipMemcpyDeviceToHost, st));
        if (map_atom) PNX_HIP(hipMemcpyAsync(map_atom, ob + off_atom, nv * 4, hipMemcpyDeviceToHost, st));
        if (field_w) PNX_HIP(hipMemcpyAsync(field_w, w_d, nv * sizeof(double), hipMemcpyDeviceToHost, st));
        if (field_n) PNX_HIP(hipMemcpyAsync(field_n, n_d, nv * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    PNX_HIP(hipStreamSynchronize(st));
    grid_mrf_report(n_sweeps, done, trace.data(), delta, n_sweeps_done);
    return PNX_OK;
}

// ---- per-parameter marginals of the grid posterior (kernels: pnx_grid_marginal.hip and the EM's normaliser pass, argument
// checks: pnx_grid_marginal_args.hpp)
int pnx_curvefit_grid_marginals_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                    const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                    const double *log_prior, double noise_sd, const int32_t *n_bins, const int32_t *bin_of,
                                    const double *bin_value, int n_q, const double *probs, double *marginal, double *quantile,
                                    double *log_evidence, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    GridPosteriorHost H;
    GridMarginalHost M;
    if ((rc = grid_marginal_check_args(&c, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, n_bins, bin_of,
                                       bin_value, n_q, probs, marginal, quantile, mem, &H, &M)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, work_buf, marg_buf, y_buf, out_buf;  // stream-ordered, freed behind the work that reads them
    GridDict D;
    GridPosterior P;
    GridPriorWork W;
    GridMarginal G;
    if ((rc = dict_buf.alloc(grid_dict_bytes(c.n_free, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(grid_posterior_bytes(c.n_free, n_atoms), st))) return rc;
    if ((rc = work_buf.alloc(grid_prior_bytes(n_vox, n_atoms, dev->cus), st))) return rc;
    if ((rc = marg_buf.alloc(grid_marginal_bytes(c.n_free, n_atoms), st))) return rc;
    const size_t B = (size_t)M.n_bins_total, nv = (size_t)n_vox;
    const size_t marg_bytes = B * nv * sizeof(double), quant_bytes = (size_t)n_q * c.n_free * nv * sizeof(double), ev_bytes = nv * sizeof(double);
    double *marg_d = marginal, *quant_d = n_q ? quantile : nullptr, *ev_d = log_evidence;
    if (mem == PNX_MEM_HOST) {  // both passes read the same signals: one upload, the outputs in one buffer, as the EM call stages
        const size_t y_bytes = nv * c.n_b * sizeof(double);
        const size_t r256 = 255, o_marg = 0, o_quant = (marg_bytes + r256) & ~r256, o_ev = o_quant + ((quant_bytes + r256) & ~r256);
        if (y_buf.alloc(y_bytes, st) != PNX_OK || out_buf.alloc(o_ev + ev_bytes, st) != PNX_OK)
            return set_error(PNX_ERR_NOMEM, "grid marginals: no device memory for the %zu bytes of y and the %zu bytes of the outputs "
                                            "(%lld voxels x %d b-values, %zu bins): call with fewer voxels at a time", y_bytes, o_ev + ev_bytes,
                             (long long)n_vox, c.n_b, B);
        if ((rc = pnx_upload(y_buf.p, y, (int64_t)y_bytes, device, st, 0))) return rc;
        y = (const double *)y_buf.p;
        marg_d = (double *)((char *)out_buf.p + o_marg);
        quant_d = n_q ? (double *)((char *)out_buf.p + o_quant) : nullptr;
        ev_d = log_evidence ? (double *)((char *)out_buf.p + o_ev) : nullptr;
    }
    if ((rc = grid_dict_build(&c, b, n_atoms, atoms, fixed, lo, hi, H.s0_row, dict_buf.p, &D, st))) return rc;
    if ((rc = grid_posterior_prepare(D, H, log_prior, noise_sd, post_buf.p, &P, st))) return rc;
    if ((rc = grid_marginal_prepare(D, M, bin_of, marg_buf.p, &G, st))) return rc;
    grid_prior_carve(n_vox, n_atoms, dev->cus, work_buf.p, &W);
    if ((rc = grid_prior_normalise(D, P, n_vox, y, W, st))) return rc;
    if ((rc = grid_marginal_device(D, P, G, n_vox, y, W, bin_value, n_q, probs, marg_d, quant_d, ev_d, st))) return rc;
    if (mem == PNX_MEM_DEVICE) return PNX_OK;
    if ((rc = pnx_download(marginal, marg_d, (int64_t)marg_bytes, device, st, 0))) return rc;
    if (quant_d && (rc = pnx_download(quantile, quant_d, (int64_t)quant_bytes, device, st, 0))) return rc;
    if (ev_d && (rc = pnx_download(log_evidence, ev_d, (int64_t)ev_bytes, device, st, 0))) return rc;
    return PNX_OK;
}

// ---- variable-projection dictionary fit (kernels: pnx_varpro.hip, argument checks: pnx_varpro_args.hpp) ---------------------
int pnx_curvefit_varpro_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                            const double *nl_atoms, const double *fixed, const double *lo, const double *hi, const double *fallback,
                            double *p_out, int32_t *best, double *cost, int8_t *clipped, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    VarproLayout L;
    if ((rc = varpro_check_args(&c, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, fallback, p_out, mem, &L))) return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf;  // the dictionary: built once per call, stream-ordered, freed behind the work that reads it
    VarproDict D;
    if ((rc = dict_buf.alloc(varpro_dict_bytes(c.n_free, L.n_nl, L.k, n_atoms, c.n_b), st))) return rc;
    if ((rc = varpro_dict_build(&c, L, b, n_atoms, nl_atoms, fixed, fallback, dict_buf.p, &D, st))) return rc;
    if (mem == PNX_MEM_DEVICE) return varpro_match_device(D, n_vox, y, p_out, best, cost, clipped, dev->cus, st);
    PNX_HIP(hipStreamSynchronize(st));  // the ring's streams read the dictionary: complete before the first chunk starts
    enum { VP_Y, VP_P, VP_BEST, VP_COST, VP_CLIP };
    ArrayTable A;
    A.add(y, sizeof(double), c.n_b, false);
    A.add(p_out, sizeof(double), c.n_free, true).pmajor = true;
    A.add(best, sizeof(int32_t), 1, true);
    A.add(cost, sizeof(double), 1, true);
    A.add(clipped, sizeof(int8_t), 1, true);
    return ring_call(A, (size_t)n_vox, 3 << 18, device, st, [&](size_t n, const DevSet &S, hipStream_t s) {
        return varpro_match_device(D, (int64_t)n, S.d(VP_Y), S.d(VP_P), (int32_t *)S.dev[VP_BEST], S.d(VP_COST), (int8_t *)S.dev[VP_CLIP],
                                   dev->cus, s);
    });
}

// ---- posterior over the variable-projection dictionary (kernels: pnx_varpro_posterior.hip, checks: pnx_varpro_posterior_args.hpp)
int pnx_curvefit_varpro_posterior_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                      const double *nl_atoms, const double *fixed, const double *lo, const double *hi, const double *log_prior,
                                      double noise_sd, int marginal_amplitudes, double *mean, double *sd, int32_t *map_atom, double *map_p,
                                      double *log_evidence, double *ess, double *clipped_mass, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    VarproLayout L;
    VarproPosteriorHost H;
    if ((rc = varpro_posterior_check_args(&c, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, mean, mem,
                                          &L, &H)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf;  // built once per call, stream-ordered, freed behind the work that reads them
    VarproDict D;
    VarproPosterior P;
    if ((rc = dict_buf.alloc(varpro_dict_bytes(c.n_free, L.n_nl, L.k, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(varpro_posterior_bytes(L.n_nl, n_atoms), st))) return rc;
    if ((rc = varpro_dict_build(&c, L, b, n_atoms, nl_atoms, fixed, lo, dict_buf.p, &D, st))) return rc;  // no fallback: lo is not read back
    if ((rc = varpro_posterior_prepare(D, H, log_prior, noise_sd, marginal_amplitudes, post_buf.p, &P, st))) return rc;
    if (mem == PNX_MEM_DEVICE)
        return varpro_posterior_device(D, P, n_vox, y, mean, sd, map_atom, map_p, log_evidence, ess, clipped_mass, dev->cus, st);
    PNX_HIP(hipStreamSynchronize(st));  // the ring's streams read the dictionary: complete before the first chunk starts
    enum { VQ_Y, VQ_MEAN, VQ_SD, VQ_ATOM, VQ_MAPP, VQ_LOGEV, VQ_ESS, VQ_CM };
    ArrayTable A;
    A.add(y, sizeof(double), c.n_b, false);
    A.add(mean, sizeof(double), c.n_free, true).pmajor = true;
    A.add(sd, sizeof(double), c.n_free, true).pmajor = true;
    A.add(map_atom, sizeof(int32_t), 1, true);
    A.add(map_p, sizeof(double), c.n_free, true).pmajor = true;
    A.add(log_evidence, sizeof(double), 1, true);
    A.add(ess, sizeof(double), 1, true);
    A.add(clipped_mass, sizeof(double), 1, true);
    return ring_call(A, (size_t)n_vox, 3 << 18, device, st, [&](size_t n, const DevSet &S, hipStream_t s) {
        return varpro_posterior_device(D, P, (int64_t)n, S.d(VQ_Y), S.d(VQ_MEAN), S.d(VQ_SD), (int32_t *)S.dev[VQ_ATOM], S.d(VQ_MAPP),
                                       S.d(VQ_LOGEV), S.d(VQ_ESS), S.d(VQ_CM), dev->cus, s);
    });
}

// ---- per-parameter marginals of the posterior over the variable-projection dictionary (kernels: pnx_varpro_marginal.hip and the
// posterior's preparation, argument checks: pnx_varpro_marginal_args.hpp)
int pnx_curvefit_varpro_marginals_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                      const double *nl_atoms, const double *fixed, const double *lo, const double *hi, const double *log_prior,
                                      double noise_sd, int marginal_amplitudes, const int32_t *n_bins, const int32_t *bin_of,
                                      const double *bin_value, int n_q, const double *probs, double *marginal, double *quantile,
                                      double *geo_mean, double *log_evidence, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    VarproLayout L;
    VarproPosteriorHost H;
    GridMarginalHost M;
    if ((rc = varpro_marginal_check_args(&c, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, n_bins,
                                         bin_of, bin_value, n_q, probs, marginal, quantile, mem, &L, &H, &M)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, marg_buf, lv_buf, y_buf, out_buf;  // stream-ordered, freed behind the work that reads them
    VarproDict D;
    VarproPosterior P;
    VarproMarginal G;
    const size_t B = (size_t)M.n_bins_total, nv = (size_t)n_vox;
    if ((rc = dict_buf.alloc(varpro_dict_bytes(c.n_free, L.n_nl, L.k, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(varpro_posterior_bytes(L.n_nl, n_atoms), st))) return rc;
    if ((rc = marg_buf.alloc(varpro_marginal_bytes(c.n_free, n_atoms), st))) return rc;
    if ((rc = lv_buf.alloc(nv * sizeof(double), st))) return rc;
    const size_t marg_bytes = B * nv * sizeof(double), quant_bytes = (size_t)n_q * c.n_free * nv * sizeof(double);
    const size_t geo_bytes = (size_t)c.n_free * nv * sizeof(double), ev_bytes = nv * sizeof(double);
    double *marg_d = marginal, *quant_d = n_q ? quantile : nullptr, *geo_d = geo_mean, *ev_d = log_evidence;
    if (mem == PNX_MEM_HOST) {  // one upload of the signals, the outputs in one buffer, as pnx_curvefit_grid_marginals_f64 stages them
        const size_t y_bytes = nv * c.n_b * sizeof(double);
        const size_t r256 = 255, o_quant = (marg_bytes + r256) & ~r256, o_geo = o_quant + ((quant_bytes + r256) & ~r256);
        const size_t o_ev = o_geo + ((geo_bytes + r256) & ~r256);
        if (y_buf.alloc(y_bytes, st) != PNX_OK || out_buf.alloc(o_ev + ev_bytes, st) != PNX_OK)
            return set_error(PNX_ERR_NOMEM, "varpro marginals: no device memory for the %zu bytes of y and the %zu bytes of the outputs "
                                            "(%lld voxels x %d b-values, %zu bins): call with fewer voxels at a time", y_bytes, o_ev + ev_bytes,
                             (long long)n_vox, c.n_b, B);
        if ((rc = pnx_upload(y_buf.p, y, (int64_t)y_bytes, device, st, 0))) return rc;
        y = (const double *)y_buf.p;
        marg_d = (double *)out_buf.p;
        quant_d = n_q ? (double *)((char *)out_buf.p + o_quant) : nullptr;
        geo_d = geo_mean ? (double *)((char *)out_buf.p + o_geo) : nullptr;
        ev_d = log_evidence ? (double *)((char *)out_buf.p + o_ev) : nullptr;
    }
    if ((rc = varpro_dict_build(&c, L, b, n_atoms, nl_atoms, fixed, lo, dict_buf.p, &D, st))) return rc;  // no fallback: lo is not read back
    if ((rc = varpro_posterior_prepare(D, H, log_prior, noise_sd, marginal_amplitudes, post_buf.p, &P, st))) return rc;
    if ((rc = varpro_marginal_prepare(D, M, bin_of, marg_buf.p, &G, st))) return rc;
    if ((rc = varpro_marginal_device(D, P, G, n_vox, y, bin_value, n_q, probs, marg_d, (double *)lv_buf.p, quant_d, geo_d, ev_d, dev->cus, st)))
        return rc;
    if (mem == PNX_MEM_DEVICE) return PNX_OK;
    if ((rc = pnx_download(marginal, marg_d, (int64_t)marg_bytes, device, st, 0))) return rc;
    if (quant_d && (rc = pnx_download(quantile, quant_d, (int64_t)quant_bytes, device, st, 0))) return rc;
    if (geo_d && (rc = pnx_download(geo_mean, geo_d, (int64_t)geo_bytes, device, st, 0))) return rc;
    if (ev_d && (rc = pnx_download(log_evidence, ev_d, (int64_t)ev_bytes, device, st, 0))) return rc;
    return PNX_OK;
}

// ---- the prior over the variable-projection dictionary learned from the volume (kernels: pnx_varpro_prior.hip and the posterior's
// preparation, argument checks: pnx_varpro_prior_args.hpp; the host loop is pnx_curvefit_grid_prior_em_f64's)
int pnx_curvefit_varpro_prior_em_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                     const double *nl_atoms, const double *fixed, const double *lo, const double *hi, const double *log_prior,
                                     double noise_sd, int marginal_amplitudes, int n_iter, double pseudo_count, double rel_tol,
                                     double *log_prior_out, double *loglik, int *n_iter_done, int64_t *n_eff, int mem, int device,
                                     void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    VarproLayout L;
    VarproPosteriorHost H;
    if ((rc = varpro_prior_check_args(&c, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, n_iter,
                                      pseudo_count, rel_tol, log_prior_out, mem, &L, &H)))
        return rc;
    grid_prior_start(n_atoms, log_prior, H.log_prior_norm, log_prior_out);  // the start, normalised; n_adm needs occ: on the device
    if (loglik) loglik[0] = 0.0;
    if (n_vox == 0) {
        grid_prior_report(n_iter, 0, 0, loglik, n_iter_done, n_eff);
        return PNX_OK;
    }
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, work_buf, y_buf;  // stream-ordered, freed behind the work that reads them
    VarproDict D;
    VarproPosterior P;
    VarproPriorWork W;
    if ((rc = dict_buf.alloc(varpro_dict_bytes(c.n_free, L.n_nl, L.k, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(varpro_posterior_bytes(L.n_nl, n_atoms), st))) return rc;
    if ((rc = work_buf.alloc(varpro_prior_bytes(n_vox, n_atoms, dev->cus), st))) return rc;
    if (mem == PNX_MEM_HOST) {  // every pass of every iteration reads the same signals: one upload, kept for the call
        const size_t bytes = (size_t)n_vox * c.n_b * sizeof(double);
        if (y_buf.alloc(bytes, st) != PNX_OK)
            return set_error(PNX_ERR_NOMEM, "varpro prior: no device memory for the %zu bytes of y (%lld voxels x %d), which stay resident for "
                                            "all iterations: learn the prior from a sub-sample of the voxels", bytes, (long long)n_vox, c.n_b);
        if ((rc = pnx_upload(y_buf.p, y, (int64_t)bytes, device, st, 0))) return rc;
        y = (const double *)y_buf.p;
    }
    if ((rc = varpro_dict_build(&c, L, b, n_atoms, nl_atoms, fixed, lo, dict_buf.p, &D, st))) return rc;  // no fallback: lo is not read back
    // without a prior the posterior's lw is the Occam term alone (0 with the profile weight): computed once per call
    if ((rc = varpro_posterior_prepare(D, H, nullptr, noise_sd, marginal_amplitudes, post_buf.p, &P, st))) return rc;
    varpro_prior_carve(n_vox, n_atoms, dev->cus, work_buf.p, &W);
    if ((rc = varpro_prior_begin(D, P, log_prior_out, W, st))) return rc;
    std::vector<double> trace((size_t)n_iter + 1, 0.0);
    VarproPriorStats stats = {0.0, 0};
    int done = 0;
    for (int t = 0;; ++t) {  // trace[t]: the log-likelihood under the prior before update t, the returned prior's at t = done
        if ((rc = varpro_prior_normalise(D, P, n_vox, y, W, st))) return rc;
        PNX_HIP(hipMemcpyAsync(&stats, W.stats, sizeof(stats), hipMemcpyDeviceToHost, st));
        PNX_HIP(hipStreamSynchronize(st));
        trace[t] = stats.loglik;
        done = t;
        if (stats.n_finite == 0 || t == n_iter || grid_prior_converged(trace.data(), t, rel_tol)) break;
        if ((rc = varpro_prior_update(D, P, n_vox, y, W, pseudo_count, st))) return rc;
    }
    PNX_HIP(hipMemcpyAsync(log_prior_out, W.lp, (size_t)n_atoms * sizeof(double), hipMemcpyDeviceToHost, st));
    PNX_HIP(hipStreamSynchronize(st));
    if (loglik)
        for (int t = 0; t <= done; ++t) loglik[t] = trace[t];
    grid_prior_report(n_iter, done, stats.n_finite, loglik, n_iter_done, n_eff);
    return PNX_OK;
}

// ---- one prior row per segmentation label over the variable-projection dictionary (kernels: pnx_varpro_class.hip and the
// posterior's preparation, argument checks: pnx_varpro_class_args.hpp; the host loop is pnx_curvefit_grid_prior_em_classes_f64's)
int pnx_curvefit_varpro_posterior_classes_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                              const double *nl_atoms, const double *fixed, const double *lo, const double *hi, int n_classes,
                                              const int32_t *labels, const double *log_prior, double noise_sd, int marginal_amplitudes,
                                              double *mean, double *sd, int32_t *map_atom, double *map_p, double *log_evidence, double *ess,
                                              double *clipped_mass, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    VarproLayout L;
    VarproPosteriorHost H;
    GridClassHost K;
    if ((rc = varpro_class_posterior_check_args(&c, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, n_classes, labels, log_prior, noise_sd,
                                                marginal_amplitudes, mean, mem, &L, &H, &K)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, table_buf;  // built once per call, stream-ordered, freed behind the work that reads them
    VarproDict D;
    VarproPosterior P;
    VarproClassTable T;
    if ((rc = dict_buf.alloc(varpro_dict_bytes(c.n_free, L.n_nl, L.k, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(varpro_posterior_bytes(L.n_nl, n_atoms), st))) return rc;
    if ((rc = table_buf.alloc(varpro_class_table_bytes(n_classes, n_atoms), st))) return rc;
    if ((rc = varpro_dict_build(&c, L, b, n_atoms, nl_atoms, fixed, lo, dict_buf.p, &D, st))) return rc;  // no fallback: lo is not read back
    // without a prior the posterior's lw is the Occam term alone (0 with the profile weight), theta is centred about H.centre
    if ((rc = varpro_posterior_prepare(D, H, nullptr, noise_sd, marginal_amplitudes, post_buf.p, &P, st))) return rc;
    if ((rc = varpro_class_table_prepare(D, P, K, n_classes, log_prior, table_buf.p, &T, st))) return rc;
    if (mem == PNX_MEM_DEVICE)
        return varpro_class_posterior_device(D, P, T, n_vox, y, labels, mean, sd, map_atom, map_p, log_evidence, ess, clipped_mass, dev->cus, st);
    PNX_HIP(hipStreamSynchronize(st));  // the ring's streams read the dictionary: complete before the first chunk starts
    enum { VC_Y, VC_LAB, VC_MEAN, VC_SD, VC_ATOM, VC_MAPP, VC_LOGEV, VC_ESS, VC_CM };
    ArrayTable A;
    A.add(y, sizeof(double), c.n_b, false);
    A.add(labels, sizeof(int32_t), 1, false);
    A.add(mean, sizeof(double), c.n_free, true).pmajor = true;
    A.add(sd, sizeof(double), c.n_free, true).pmajor = true;
    A.add(map_atom, sizeof(int32_t), 1, true);
    A.add(map_p, sizeof(double), c.n_free, true).pmajor = true;
    A.add(log_evidence, sizeof(double), 1, true);
    A.add(ess, sizeof(double), 1, true);
    A.add(clipped_mass, sizeof(double), 1, true);
    return ring_call(A, (size_t)n_vox, 3 << 18, device, st, [&](size_t n, const DevSet &S, hipStream_t s) {
        return varpro_class_posterior_device(D, P, T, (int64_t)n, S.d(VC_Y), (const int32_t *)S.dev[VC_LAB], S.d(VC_MEAN), S.d(VC_SD),
                                             (int32_t *)S.dev[VC_ATOM], S.d(VC_MAPP), S.d(VC_LOGEV), S.d(VC_ESS), S.d(VC_CM), dev->cus, s);
    });
}

int pnx_curvefit_varpro_prior_em_classes_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                             const double *nl_atoms, const double *fixed, const double *lo, const double *hi, int n_classes,
                                             const int32_t *labels, const double *log_prior, double noise_sd, int marginal_amplitudes,
                                             int n_iter, double pseudo_count, double rel_tol, double *log_prior_out, double *loglik,
                                             double *loglik_class, int *n_iter_done, int64_t *n_eff, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    VarproLayout L;
    VarproPosteriorHost H;
    GridClassHost K;
    if ((rc = varpro_class_prior_check_args(&c, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, n_classes, labels, log_prior, noise_sd,
                                            marginal_amplitudes, n_iter, pseudo_count, rel_tol, log_prior_out, mem, &L, &H, &K)))
        return rc;
    grid_class_start(n_classes, n_atoms, log_prior, K, log_prior_out);  // the start, every row normalised; n_adm needs occ: on the device
    for (int cl = 0; cl < n_classes; ++cl) K.norm[cl] = 0.0;           // and so is the table every pass reads
    if (loglik) loglik[0] = 0.0;
    if (loglik_class)
        for (int cl = 0; cl < n_classes; ++cl) loglik_class[cl] = 0.0;
    if (n_vox == 0) {
        grid_class_report(n_iter, 0, n_classes, nullptr, loglik, loglik_class, n_iter_done, n_eff);
        return PNX_OK;
    }
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, table_buf, work_buf, y_buf, lab_buf;  // stream-ordered, freed behind the work that reads them
    VarproDict D;
    VarproPosterior P;
    VarproClassTable T;
    VarproClassWork W;
    if ((rc = dict_buf.alloc(varpro_dict_bytes(c.n_free, L.n_nl, L.k, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(varpro_posterior_bytes(L.n_nl, n_atoms), st))) return rc;
    if ((rc = table_buf.alloc(varpro_class_table_bytes(n_classes, n_atoms), st))) return rc;
    if ((rc = work_buf.alloc(varpro_class_prior_bytes(n_vox, n_atoms, n_classes, dev->cus), st))) return rc;
    if (mem == PNX_MEM_HOST) {  // every pass of every iteration reads the same signals and labels: one upload, kept for the call
        const size_t bytes = (size_t)n_vox * c.n_b * sizeof(double), lbytes = (size_t)n_vox * sizeof(int32_t);
        if (y_buf.alloc(bytes, st) != PNX_OK || lab_buf.alloc(lbytes, st) != PNX_OK)
            return set_error(PNX_ERR_NOMEM, "varpro prior: no device memory for the %zu bytes of y and labels (%lld voxels x %d), which stay "
                                            "resident for all iterations: learn the prior from a sub-sample of the voxels",
                             bytes + lbytes, (long long)n_vox, c.n_b);
        if ((rc = pnx_upload(y_buf.p, y, (int64_t)bytes, device, st, 0))) return rc;
        if ((rc = pnx_upload(lab_buf.p, labels, (int64_t)lbytes, device, st, 0))) return rc;
        y = (const double *)y_buf.p;
        labels = (const int32_t *)lab_buf.p;
    }
    if ((rc = varpro_dict_build(&c, L, b, n_atoms, nl_atoms, fixed, lo, dict_buf.p, &D, st))) return rc;  // no fallback: lo is not read back
    if ((rc = varpro_posterior_prepare(D, H, nullptr, noise_sd, marginal_amplitudes, post_buf.p, &P, st))) return rc;
    if ((rc = varpro_class_table_prepare(D, P, K, n_classes, log_prior_out, table_buf.p, &T, st))) return rc;
    varpro_class_prior_carve(n_vox, n_atoms, n_classes, dev->cus, work_buf.p, &W);
    std::vector<double> trace((size_t)n_iter + 1, 0.0), trace_class(((size_t)n_iter + 1) * n_classes, 0.0);
    VarproClassStats stats;
    memset(&stats, 0, sizeof(stats));
    int done = 0;
    for (int t = 0;; ++t) {  // trace[t]: the log-likelihood under the table before update t, the returned table's at t = done
        if ((rc = varpro_class_prior_normalise(D, P, T, n_vox, y, labels, W, st))) return rc;
        PNX_HIP(hipMemcpyAsync(&stats, W.stats, sizeof(stats), hipMemcpyDeviceToHost, st));
        PNX_HIP(hipStreamSynchronize(st));
        trace[t] = stats.loglik;
        long long total = 0;
        for (int cl = 0; cl < n_classes; ++cl) {
            trace_class[(size_t)t * n_classes + cl] = stats.loglik_class[cl];
            total += stats.n_finite[cl];
        }
        done = t;
        if (total == 0 || t == n_iter || grid_prior_converged(trace.data(), t, rel_tol)) break;
        if ((rc = varpro_class_prior_update(D, P, T, n_vox, y, labels, W, pseudo_count, st))) return rc;
    }
    PNX_HIP(hipMemcpy2DAsync(log_prior_out, (size_t)n_atoms * sizeof(double), T.lp, (size_t)D.gp * sizeof(double),
                             (size_t)n_atoms * sizeof(double), (size_t)n_classes, hipMemcpyDeviceToHost, st));
    PNX_HIP(hipStreamSynchronize(st));
    for (int t = 0; t <= done; ++t) {
        if (loglik) loglik[t] = trace[t];
        if (loglik_class)
            for (int cl = 0; cl < n_classes; ++cl) loglik_class[(size_t)t * n_classes + cl] = trace_class[(size_t)t * n_classes + cl];
    }
    int64_t finite[kGridMaxClasses];
    for (int cl = 0; cl < n_classes; ++cl) finite[cl] = stats.n_finite[cl];
    grid_class_report(n_iter, done, n_classes, finite, loglik, loglik_class, n_iter_done, n_eff);
    return PNX_OK;
}

// ---- neighbourhood (MRF) prior over the variable-projection dictionary (kernels: pnx_varpro_mrf.hip and the grid prior's gather /
// colour check, argument checks: pnx_varpro_mrf_args.hpp)
int pnx_curvefit_varpro_posterior_field_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                            const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                            const double *log_prior, double noise_sd, int marginal_amplitudes, int64_t first, int64_t count,
                                            const double *field_q, const int32_t *field_n, const double *precision, double *mean, double *sd,
                                            int32_t *map_atom, double *map_p, double *log_evidence, double *ess, double *clipped_mass,
                                            double *delta_max, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    VarproLayout L;
    VarproPosteriorHost H;
    VarproMrfHost M;
    if ((rc = varpro_mrf_posterior_field_check_args(&c, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes,
                                                    first, count, field_q, field_n, precision, mean, mem, &L, &H, &M)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, mrf_buf;  // built once per call, stream-ordered, freed behind the work that reads them
    VarproDict D;
    VarproPosterior P;
    VarproMrf F;
    if ((rc = dict_buf.alloc(varpro_dict_bytes(c.n_free, L.n_nl, L.k, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(varpro_posterior_bytes(L.n_nl, n_atoms), st))) return rc;
    if ((rc = mrf_buf.alloc(varpro_mrf_bytes(n_atoms, dev->cus), st))) return rc;
    if ((rc = varpro_dict_build(&c, L, b, n_atoms, nl_atoms, fixed, lo, dict_buf.p, &D, st))) return rc;  // no fallback: lo is not read back
    if ((rc = varpro_posterior_prepare(D, H, log_prior, noise_sd, marginal_amplitudes, post_buf.p, &P, st))) return rc;
    if ((rc = varpro_mrf_prepare(D, H, M, nl_atoms, precision, dev->cus, mrf_buf.p, &F, st))) return rc;
    return varpro_mrf_posterior_device(D, P, F, n_vox, first, count, y, field_q, field_n, mean, sd, map_atom, map_p, log_evidence, ess,
                                       clipped_mass, delta_max, false, dev->cus, st);
}

int pnx_curvefit_varpro_posterior_mrf_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                          const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                          const double *log_prior, double noise_sd, int marginal_amplitudes, int n_nb,
                                          const int32_t *neighbours, int n_colours, const int64_t *colour_start, const double *precision,
                                          int n_sweeps, double tol, double *mean, double *sd, int32_t *map_atom, double *map_p,
                                          double *log_evidence, double *ess, double *clipped_mass, double *delta, int *n_sweeps_done, int mem,
                                          int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    VarproLayout L;
    VarproPosteriorHost H;
    VarproMrfHost M;
    if ((rc = varpro_mrf_check_args(&c, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, n_nb, neighbours,
                                    n_colours, colour_start, precision, n_sweeps, tol, mean, mem, &L, &H, &M)))
        return rc;
    std::vector<double> trace((size_t)n_sweeps + 1, 0.0);
    if (n_vox == 0) {
        grid_mrf_report(n_sweeps, 0, trace.data(), delta, n_sweeps_done);
        return PNX_OK;
    }
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nf = c.n_free;
    const size_t nv = (size_t)n_vox, pb = (size_t)nf * nv * sizeof(double);
    AsyncBuf dict_buf, post_buf, mrf_buf, q_buf, n_buf, delta_buf, y_buf, nb_buf, out_buf;  // stream-ordered, freed behind the work that reads them
    VarproDict D;
    VarproPosterior P;
    VarproMrf F;
    if ((rc = dict_buf.alloc(varpro_dict_bytes(nf, L.n_nl, L.k, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(varpro_posterior_bytes(L.n_nl, n_atoms), st))) return rc;
    if ((rc = mrf_buf.alloc(varpro_mrf_bytes(n_atoms, dev->cus), st))) return rc;
    if ((rc = q_buf.alloc(pb, st)) || (rc = n_buf.alloc(nv * sizeof(int32_t), st)) || (rc = delta_buf.alloc(((size_t)n_sweeps + 1) * 8, st)))
        return rc;
    double *mean_d = mean, *sd_d = sd, *mapp_d = map_p, *logev_d = log_evidence, *ess_d = ess, *cm_d = clipped_mass;
    int32_t *atom_d = map_atom;
    size_t off_sd = 0, off_mapp = 0, off_logev = 0, off_ess = 0, off_cm = 0, off_atom = 0, out_bytes = 0;
    if (mem == PNX_MEM_HOST) {  // every sweep reads the same signals and table: one upload, kept for the call; the outputs in one buffer
        const size_t yb = nv * c.n_b * sizeof(double), nbb = nv * n_nb * sizeof(int32_t);
        out_bytes = pb;
        if (sd) off_sd = out_bytes, out_bytes += pb;
        if (map_p) off_mapp = out_bytes, out_bytes += pb;
        if (log_evidence) off_logev = out_bytes, out_bytes += nv * 8;
        if (ess) off_ess = out_bytes, out_bytes += nv * 8;
        if (clipped_mass) off_cm = out_bytes, out_bytes += nv * 8;
        if (map_atom) off_atom = out_bytes, out_bytes += nv * 4;
        if (y_buf.alloc(yb, st) != PNX_OK || nb_buf.alloc(nbb, st) != PNX_OK || out_buf.alloc(out_bytes, st) != PNX_OK)
            return set_error(PNX_ERR_NOMEM, "varpro posterior mrf: no device memory for the %zu bytes of y, neighbours and the outputs (%lld voxels "
                                            "x %d), which stay resident for all sweeps", yb + nbb + out_bytes, (long long)n_vox, c.n_b);
        if ((rc = pnx_upload(y_buf.p, y, (int64_t)yb, device, st, 0))) return rc;
        if ((rc = pnx_upload(nb_buf.p, neighbours, (int64_t)nbb, device, st, 0))) return rc;
        y = (const double *)y_buf.p;
        neighbours = (const int32_t *)nb_buf.p;
        char *ob = (char *)out_buf.p;
        mean_d = (double *)ob;
        sd_d = sd ? (double *)(ob + off_sd) : nullptr;
        mapp_d = map_p ? (double *)(ob + off_mapp) : nullptr;
        logev_d = log_evidence ? (double *)(ob + off_logev) : nullptr;
        ess_d = ess ? (double *)(ob + off_ess) : nullptr;
        cm_d = clipped_mass ? (double *)(ob + off_cm) : nullptr;
        atom_d = map_atom ? (int32_t *)(ob + off_atom) : nullptr;
    }
    if ((rc = varpro_dict_build(&c, L, b, n_atoms, nl_atoms, fixed, lo, dict_buf.p, &D, st))) return rc;  // no fallback: lo is not read back
    if ((rc = varpro_posterior_prepare(D, H, log_prior, noise_sd, marginal_amplitudes, post_buf.p, &P, st))) return rc;
    if ((rc = varpro_mrf_prepare(D, H, M, nl_atoms, precision, dev->cus, mrf_buf.p, &F, st))) return rc;
    // the colouring: no index out of range, no edge inside a colour -- argument errors, found before any sweep
    int32_t flags[2] = {INT32_MAX, INT32_MAX};
    if ((rc = grid_mrf_colour_check_device(n_vox, n_nb, neighbours, n_colours, colour_start, F.flags, st))) return rc;
    PNX_HIP(hipMemcpyAsync(flags, F.flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    PNX_HIP(hipStreamSynchronize(st));
    if (flags[0] != INT32_MAX)
        return set_error(PNX_ERR_INVALID, "varpro posterior mrf: neighbours of voxel %d hold an index outside [-1, %lld)", flags[0], (long long)n_vox);
    if (flags[1] != INT32_MAX)
        return set_error(PNX_ERR_INVALID, "varpro posterior mrf: voxel %d has a neighbour inside its own colour range (an edge inside a colour: the "
                                          "update would not be coordinate ascent)", flags[1]);
    double *delta_d = (double *)delta_buf.p;
    PNX_HIP(hipMemsetAsync(delta_d, 0, ((size_t)n_sweeps + 1) * 8, st));
    // sweep 0: the plain posterior
    if ((rc = varpro_posterior_device(D, P, n_vox, y, mean_d, sd_d, atom_d, mapp_d, logev_d, ess_d, cm_d, dev->cus, st))) return rc;
    GridMrfFieldArgs ga;  // the grid prior's gather: centre and precision are 0 on the linear rows, so q is 0 there
    memset(&ga, 0, sizeof(ga));
    ga.nb = neighbours;
    ga.mean = mean_d;
    ga.q = (double *)q_buf.p;
    ga.n = (int32_t *)n_buf.p;
    ga.flag = nullptr;  // checked above
    ga.n_vox = n_vox;
    ga.n_free = nf;
    ga.n_nb = n_nb;
    for (int k = 0; k < nf; ++k) {
        ga.centre[k] = H.centre[k];
        ga.precision[k] = precision[k];
    }
    int done = 0;
    for (int s = 1; s <= n_sweeps; ++s) {
        for (int col = 0; col < n_colours; ++col) {
            ga.first = colour_start[col];
            ga.count = colour_start[col + 1] - colour_start[col];
            if (ga.count == 0) continue;
            if ((rc = grid_mrf_field_device(ga, st))) return rc;
            if ((rc = varpro_mrf_posterior_device(D, P, F, n_vox, ga.first, ga.count, y, ga.q, ga.n, mean_d, sd_d, atom_d, mapp_d, logev_d, ess_d,
                                                  cm_d, delta_d + (s - 1), true, dev->cus, st)))
                return rc;
        }
        done = s;
        if (tol > 0.0) {  // the stopping rule needs this sweep's delta on the host; tol = 0 runs all sweeps without a round trip
            PNX_HIP(hipMemcpyAsync(&trace[s - 1], delta_d + (s - 1), 8, hipMemcpyDeviceToHost, st));
            PNX_HIP(hipStreamSynchronize(st));
            if (trace[s - 1] <= tol) break;
        }
    }
    if (n_sweeps > 0) PNX_HIP(hipMemcpyAsync(trace.data(), delta_d, (size_t)n_sweeps * 8, hipMemcpyDeviceToHost, st));
    if (mem == PNX_MEM_HOST) {
        const char *ob = (const char *)out_buf.p;
        PNX_HIP(hipMemcpyAsync(mean, ob, pb, hipMemcpyDeviceToHost, st));
        if (sd) PNX_HIP(hipMemcpyAsync(sd, ob + off_sd, pb, hipMemcpyDeviceToHost, st));
        if (map_p) PNX_HIP(hipMemcpyAsync(map_p, ob + off_mapp, pb, hipMemcpyDeviceToHost, st));
        if (log_evidence) PNX_HIP(hipMemcpyAsync(log_evidence, ob + off_logev, nv * 8, hipMemcpyDeviceToHost, st));
        if (ess) PNX_HIP(hipMemcpyAsync(ess, ob + off_ess, nv * 8, hipMemcpyDeviceToHost, st));
        if (clipped_mass) PNX_HIP(hipMemcpyAsync(clipped_mass, ob + off_cm, nv * 8, hipMemcpyDeviceToHost, st));
        if (map_atom) PNX_HIP(hipMemcpyAsync(map_atom, ob + off_atom, nv * 4, hipMemcpyDeviceToHost, st));
    }
    PNX_HIP(hipStreamSynchronize(st));
    grid_mrf_report(n_sweeps, done, trace.data(), delta, n_sweeps_done);
    return PNX_OK;
}

// ---- the same prior with a per-row linear or log coupling (kernel: pnx_varpro_logmrf.hip, argument checks: pnx_varpro_logmrf_args.hpp)
int pnx_curvefit_varpro_posterior_logfield_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                               const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                               const double *log_prior, double noise_sd, int marginal_amplitudes, int64_t first, int64_t count,
                                               const double *field_q, const int32_t *field_n, const double *precision,
                                               const int32_t *coupling, double *mean, double *sd, int32_t *map_atom, double *map_p,
                                               double *log_evidence, double *ess, double *clipped_mass, double *field_mean,
                                               double *delta_max, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    VarproLayout L;
    VarproPosteriorHost H;
    VarproMrfHost M;
    VarproLogMrfHost G;
    if ((rc = varpro_logmrf_posterior_field_check_args(&c, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd,
                                                       marginal_amplitudes, first, count, field_q, field_n, precision, coupling, mean,
                                                       field_mean, mem, &L, &H, &M, &G)))
        return rc;
    if (n_vox == 0) return PNX_OK;
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    AsyncBuf dict_buf, post_buf, mrf_buf;  // built once per call, stream-ordered, freed behind the work that reads them
    VarproDict D;
    VarproPosterior P;
    VarproLogMrf F;
    if ((rc = dict_buf.alloc(varpro_dict_bytes(c.n_free, L.n_nl, L.k, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(varpro_posterior_bytes(L.n_nl, n_atoms), st))) return rc;
    if ((rc = mrf_buf.alloc(varpro_logmrf_bytes(L.n_nl, n_atoms, dev->cus), st))) return rc;
    if ((rc = varpro_dict_build(&c, L, b, n_atoms, nl_atoms, fixed, lo, dict_buf.p, &D, st))) return rc;  // no fallback: lo is not read back
    if ((rc = varpro_posterior_prepare(D, H, log_prior, noise_sd, marginal_amplitudes, post_buf.p, &P, st))) return rc;
    if ((rc = varpro_logmrf_prepare(D, G, nl_atoms, precision, coupling, dev->cus, mrf_buf.p, &F, st))) return rc;
    return varpro_logmrf_posterior_device(D, P, F, true, n_vox, first, count, y, field_q, field_n, mean, sd, map_atom, map_p, log_evidence, ess,
                                          clipped_mass, field_mean, delta_max, false, dev->cus, st);
}

int pnx_curvefit_varpro_posterior_logmrf_f64(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                             const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                             const double *log_prior, double noise_sd, int marginal_amplitudes, int n_nb,
                                             const int32_t *neighbours, int n_colours, const int64_t *colour_start, const double *precision,
                                             const int32_t *coupling, int n_sweeps, double tol, double *mean, double *sd, int32_t *map_atom,
                                             double *map_p, double *log_evidence, double *ess, double *clipped_mass, double *field_mean,
                                             double *delta, int *n_sweeps_done, int mem, int device, void *stream) {
    if (!o) return set_error(PNX_ERR_INVALID, "opts is NULL");
    pnx_curvefit_opts c = *o;  // as grid start: jac_mode and the tolerances are not looked at
    c.jac_mode = PNX_JAC_ANALYTIC;
    c.ftol = c.xtol = c.gtol = 0.0;
    int rc = check_curvefit_opts(&c);
    if (rc) return rc;
    VarproLayout L;
    VarproPosteriorHost H;
    VarproMrfHost M;
    VarproLogMrfHost G;
    if ((rc = varpro_logmrf_check_args(&c, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, n_nb,
                                       neighbours, n_colours, colour_start, precision, coupling, n_sweeps, tol, mean, mem, &L, &H, &M, &G)))
        return rc;
    std::vector<double> trace((size_t)n_sweeps + 1, 0.0);
    if (n_vox == 0) {
        grid_mrf_report(n_sweeps, 0, trace.data(), delta, n_sweeps_done);
        return PNX_OK;
    }
    DeviceInfo *dev;
    if ((rc = use_device(device, &dev))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nf = c.n_free;
    const size_t nv = (size_t)n_vox, pb = (size_t)nf * nv * sizeof(double);
    AsyncBuf dict_buf, post_buf, mrf_buf, q_buf, n_buf, delta_buf, y_buf, nb_buf, out_buf, fm_buf;  // stream-ordered, freed behind the work that reads them
    VarproDict D;
    VarproPosterior P;
    VarproLogMrf F;
    if ((rc = dict_buf.alloc(varpro_dict_bytes(nf, L.n_nl, L.k, n_atoms, c.n_b), st))) return rc;
    if ((rc = post_buf.alloc(varpro_posterior_bytes(L.n_nl, n_atoms), st))) return rc;
    if ((rc = mrf_buf.alloc(varpro_logmrf_bytes(L.n_nl, n_atoms, dev->cus), st))) return rc;
    if ((rc = q_buf.alloc(pb, st)) || (rc = n_buf.alloc(nv * sizeof(int32_t), st)) || (rc = delta_buf.alloc(((size_t)n_sweeps + 1) * 8, st)))
        return rc;
    double *mean_d = mean, *sd_d = sd, *mapp_d = map_p, *logev_d = log_evidence, *ess_d = ess, *cm_d = clipped_mass, *fm_d = field_mean;
    int32_t *atom_d = map_atom;
    size_t off_sd = 0, off_mapp = 0, off_logev = 0, off_ess = 0, off_cm = 0, off_atom = 0, off_fm = 0, out_bytes = 0;
    if (mem == PNX_MEM_HOST) {  // every sweep reads the same signals and table: one upload, kept for the call; the outputs in one buffer
        const size_t yb = nv * c.n_b * sizeof(double), nbb = nv * n_nb * sizeof(int32_t);
        out_bytes = pb;
        off_fm = out_bytes, out_bytes += pb;  // the sweeps need the means of f whether the caller asks for them or not
        if (sd) off_sd = out_bytes, out_bytes += pb;
        if (map_p) off_mapp = out_bytes, out_bytes += pb;
        if (log_evidence) off_logev = out_bytes, out_bytes += nv * 8;
        if (ess) off_ess = out_bytes, out_bytes += nv * 8;
        if (clipped_mass) off_cm = out_bytes, out_bytes += nv * 8;
        if (map_atom) off_atom = out_bytes, out_bytes += nv * 4;
        if (y_buf.alloc(yb, st) != PNX_OK || nb_buf.alloc(nbb, st) != PNX_OK || out_buf.alloc(out_bytes, st) != PNX_OK)
            return set_error(PNX_ERR_NOMEM, "varpro posterior logmrf: no device memory for the %zu bytes of y, neighbours and the outputs (%lld "
                                            "voxels x %d), which stay resident for all sweeps", yb + nbb + out_bytes, (long long)n_vox, c.n_b);
        if ((rc = pnx_upload(y_buf.p, y, (int64_t)yb, device, st, 0))) return rc;
        if ((rc = pnx_upload(nb_buf.p, neighbours, (int64_t)nbb, device, st, 0))) return rc;
        y = (const double *)y_buf.p;
        neighbours = (const int32_t *)nb_buf.p;
        char *ob = (char *)out_buf.p;
        mean_d = (double *)ob;
        fm_d = (double *)(ob + off_fm);
        sd_d = sd ? (double *)(ob + off_sd) : nullptr;
        mapp_d = map_p ? (double *)(ob + off_mapp) : nullptr;
        logev_d = log_evidence ? (double *)(ob + off_logev) : nullptr;
        ess_d = ess ? (double *)(ob + off_ess) : nullptr;
        cm_d = clipped_mass ? (double *)(ob + off_cm) : nullptr;
        atom_d = map_atom ? (int32_t *)(ob + off_atom) : nullptr;
    } else if (!fm_d) {
        if ((rc = fm_buf.alloc(pb, st))) return rc;
        fm_d = (double *)fm_buf.p;
    }
    if ((rc = varpro_dict_build(&c, L, b, n_atoms, nl_atoms, fixed, lo, dict_buf.p, &D, st))) return rc;  // no fallback: lo is not read back
    if ((rc = varpro_posterior_prepare(D, H, log_prior, noise_sd, marginal_amplitudes, post_buf.p, &P, st))) return rc;
    if ((rc = varpro_logmrf_prepare(D, G, nl_atoms, precision, coupling, dev->cus, mrf_buf.p, &F, st))) return rc;
    // the colouring: no index out of range, no edge inside a colour -- argument errors, found before any sweep
    int32_t flags[2] = {INT32_MAX, INT32_MAX};
    if ((rc = grid_mrf_colour_check_device(n_vox, n_nb, neighbours, n_colours, colour_start, F.flags, st))) return rc;
    PNX_HIP(hipMemcpyAsync(flags, F.flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    PNX_HIP(hipStreamSynchronize(st));
    if (flags[0] != INT32_MAX)
        return set_error(PNX_ERR_INVALID, "varpro posterior logmrf: neighbours of voxel %d hold an index outside [-1, %lld)", flags[0], (long long)n_vox);
    if (flags[1] != INT32_MAX)
        return set_error(PNX_ERR_INVALID, "varpro posterior logmrf: voxel %d has a neighbour inside its own colour range (an edge inside a colour: "
                                          "the update would not be coordinate ascent)", flags[1]);
    double *delta_d = (double *)delta_buf.p;
    PNX_HIP(hipMemsetAsync(delta_d, 0, ((size_t)n_sweeps + 1) * 8, st));
    // sweep 0: the plain posterior -- the same fold without a field, so that field_mean belongs to the weights behind mean
    if ((rc = varpro_logmrf_posterior_device(D, P, F, false, n_vox, 0, n_vox, y, nullptr, nullptr, mean_d, sd_d, atom_d, mapp_d, logev_d, ess_d, cm_d,
                                             fm_d, nullptr, false, dev->cus, st)))
        return rc;
    GridMrfFieldArgs ga;  // the grid prior's gather over the means of f: fcentre and precision are 0 on the linear rows, so q is 0 there
    memset(&ga, 0, sizeof(ga));
    ga.nb = neighbours;
    ga.mean = fm_d;
    ga.q = (double *)q_buf.p;
    ga.n = (int32_t *)n_buf.p;
    ga.flag = nullptr;  // checked above
    ga.n_vox = n_vox;
    ga.n_free = nf;
    ga.n_nb = n_nb;
    for (int k = 0; k < nf; ++k) {
        ga.centre[k] = G.fcentre[k];
        ga.precision[k] = precision[k];
    }
    int done = 0;
    for (int s = 1; s <= n_sweeps; ++s) {
        for (int col = 0; col < n_colours; ++col) {
            ga.first = colour_start[col];
            ga.count = colour_start[col + 1] - colour_start[col];
            if (ga.count == 0) continue;
            if ((rc = grid_mrf_field_device(ga, st))) return rc;
            if ((rc = varpro_logmrf_posterior_device(D, P, F, true, n_vox, ga.first, ga.count, y, ga.q, ga.n, mean_d, sd_d, atom_d, mapp_d, logev_d,
                                                     ess_d, cm_d, fm_d, delta_d + (s - 1), true, dev->cus, st)))
                return rc;
        }
        done = s;
        if (tol > 0.0) {  // the stopping rule needs this sweep's delta on the host; tol = 0 runs all sweeps without a round trip
            PNX_HIP(hipMemcpyAsync(&trace[s - 1], delta_d + (s - 1), 8, hipMemcpyDeviceToHost, st));
            PNX_HIP(hipStreamSynchronize(st));
            if (trace[s - 1] <= tol) break;
        }
    }
    if (n_sweeps > 0) PNX_HIP(hipMemcpyAsync(trace.data(), delta_d, (size_t)n_sweeps * 8, hipMemcpyDeviceToHost, st));
    if (mem == PNX_MEM_HOST) {
        const char *ob = (const char *)out_buf.p;
        PNX_HIP(hipMemcpyAsync(mean, ob, pb, hipMemcpyDeviceToHost, st));
        if (field_mean) PNX_HIP(hipMemcpyAsync(field_mean, ob + off_fm, pb, hipMemcpyDeviceToHost, st));
        if (sd) PNX_HIP(hipMemcpyAsync(sd, ob + off_sd, pb, hipMemcpyDeviceToHost, st));
        if (map_p) PNX_HIP(hipMemcpyAsync(map_p, ob + off_mapp, pb, hipMemcpyDeviceToHost, st));
        if (log_evidence) PNX_HIP(hipMemcpyAsync(log_evidence, ob + off_logev, nv * 8, hipMemcpyDeviceToHost, st));
        if (ess) PNX_HIP(hipMemcpyAsync(ess, ob + off_ess, nv * 8, hipMemcpyDeviceToHost, st));
        if (clipped_mass) PNX_HIP(hipMemcpyAsync(clipped_mass, ob + off_cm, nv * 8, hipMemcpyDeviceToHost, st));
        if (map_atom) PNX_HIP(hipMemcpyAsync(map_atom, ob + off_atom, nv * 4, hipMemcpyDeviceToHost, st));
    }
    PNX_HIP(hipStreamSynchronize(st));
    grid_mrf_report(n_sweeps, done, trace.data(), delta, n_sweeps_done);
    return PNX_OK;
}

int pnx_loglinear_f64(int64_t n_vox, int n_b, const double *b_host, const uint8_t *use_host, int weighting, int n_reweight, int clip,
                      const double *lo_host, const double *hi_host, const double *y, double *params, double *pcov, int8_t *status,
                      int32_t *n_used, double *ss_res, int mem, int device, void *stream) {
    return loglinear<double>(n_vox, n_b, b_host, use_host, weighting, n_reweight, clip, lo_host, hi_host, y, params, pcov, status, n_used,
                             ss_res, mem, device, stream);
}

int pnx_loglinear_f32(int64_t n_vox, int n_b, const float *b_host, const uint8_t *use_host, int weighting, int n_reweight, int clip,
                      const float *lo_host, const float *hi_host, const float *y, float *params, float *pcov, int8_t *status,
                      int32_t *n_used, float *ss_res, int mem, int device, void *stream) {
    return loglinear<float>(n_vox, n_b, b_host, use_host, weighting, n_reweight, clip, lo_host, hi_host, y, params, pcov, status, n_used,
                            ss_res, mem, device, stream);
}

int pnx_peel_f64(int model, int64_t n_vox, int n_b, const double *b_host, const uint8_t *use_host, int weighting, int clip,
                 const double *lo_host, const double *hi_host, const double *fallback_host, const double *y, double *params,
                 int8_t *status, int32_t *n_used, double *ss_res, int mem, int device, void *stream) {
    return peel<double>(model, n_vox, n_b, b_host, use_host, weighting, clip, lo_host, hi_host, fallback_host, y, params, status, n_used,
                        ss_res, mem, device, stream);
}

int pnx_peel_f32(int model, int64_t n_vox, int n_b, const float *b_host, const uint8_t *use_host, int weighting, int clip,
                 const float *lo_host, const float *hi_host, const float *fallback_host, const float *y, float *params, int8_t *status,
                 int32_t *n_used, float *ss_res, int mem, int device, void *stream) {
    return peel<float>(model, n_vox, n_b, b_host, use_host, weighting, clip, lo_host, hi_host, fallback_host, y, params, status, n_used,
                       ss_res, mem, device, stream);
}

// ------------------------------------------------------------------------------------------- NNLS
struct pnx_nnls_plan {
    NnlsPlanData d;
    std::mutex mu;  // the plan's device scratch (ATY chunk, M overflow, queue) serves one solve at a time
};

int pnx_nnls_plan_create(pnx_nnls_plan **plan, int n_meas, int n_bins, const double *basis, const double *reg,
                         int n_reg, int device) {
    if (!plan || !basis) return set_error(PNX_ERR_INVALID, "NULL pointer");
    if (n_meas < 1 || n_bins < 1 || n_reg < 0 || (n_reg && !reg)) return set_error(PNX_ERR_INVALID, "bad NNLS sizes");
    if (n_bins > kNnlsWideBins) return set_error(PNX_ERR_UNSUPPORTED, "n_bins=%d > %d", n_bins, kNnlsWideBins);
    if (n_meas > kNnlsMaxMeas) return set_error(PNX_ERR_UNSUPPORTED, "n_meas=%d > %d", n_meas, kNnlsMaxMeas);
    DeviceInfo *dev;
    int rc = use_device(device, &dev);
    if (rc) return rc;
    pnx_nnls_plan *p = new pnx_nnls_plan();
    rc = nnls_plan_init(&p->d, n_meas, n_bins, basis, reg, n_reg, device, dev->cus);
    if (rc) {
        nnls_plan_free(&p->d);
        delete p;
        return rc;
    }
    *plan = p;
    return PNX_OK;
}

int pnx_nnls_plan_destroy(pnx_nnls_plan *plan) {
    if (!plan) return PNX_OK;
    nnls_plan_free(&plan->d);
    delete plan;
    return PNX_OK;
}

}  // extern "C"

// the arrays of an NNLS call, in table order: the signal, the spectra, the solver's per-voxel outputs, the peak tables
enum { NN_Y, NN_SPEC, NN_RNORM, NN_STAT, NN_ITERS, NN_NPEAKS, NN_D, NN_F, NN_DC, NN_FC, NN_SS };
struct NnlsHostCall {
    ArrayTable A;          // NN_* order; the spectra are downloaded (solve) or only analysed on the device (solve_peaks)
    size_t chunk = 0;      // voxels per chunk of the ring
    bool ramp = false;     // quarter-chunk ramp at both ends (chunk_bounds)
    bool overlap = false;  // the first deferred pass runs behind the last chunk's solve, beside its download (else after the ring)
    // behind every solve, on its stream (may be empty); y: the n signal rows on the device (the deferred pass has them in its side buffer)
    std::function<int(size_t n, const double *y, const DevSet &D, hipStream_t s)> post;
};

// NNLS from host arrays: the chunk ring of the curve fit with ONE kernel stream -- the plan's device scratch (ATY chunk, M
// overflow, queue) serves one solve at a time, and in-order launches on one stream guarantee that.  The (n_vox, n_bins)
// coefficient array is 8.4 GB for the C4 volume: its D2H and first-touch faults hide behind the solves of the following chunks.
// The caller holds the plan's mutex.
static int nnls_host(NnlsPlanData &P, size_t nv, int max_iter, const NnlsHostCall &C, hipStream_t st) {
    const ArrayTable &A = C.A;
    const std::vector<size_t> bounds = chunk_bounds(nv, C.chunk, C.ramp);
    const int n_chunks = (int)bounds.size() - 1;
    const int n_slots = n_chunks < 3 ? n_chunks : 3;
    int rc;
    struct Slot {
        DevBuf slab;
        DevSet D;
    };
    std::vector<Slot> slots((size_t)n_slots);
    for (auto &S : slots)
        if ((rc = alloc_carved(S.slab, A, nv < C.chunk ? nv : C.chunk, S.D))) return rc;
    // Block-kernel plans hand a few voxels per chunk to the general kernel, and that pass costs ~8 ms per chunk whatever their
    // number (they are the longest solves there are): with several chunks the hand-over is deferred -- the chunks only
    // collect the voxels' indices and signal rows, ONE pass at the end of the call solves them, and their rows are patched
    // into the caller's arrays (C4 from numpy arrays: seven passes -> one).
    const int defer_cap = dev_env_int("PNX_NNLS_DEFER_CAP", 16384, 0, 1 << 22);
    const bool defer = P.path == NnlsPath::Blk && n_chunks >= 2 && defer_cap > 0 && nv < ((size_t)1 << 31);
    const size_t dcap = (size_t)defer_cap;
    DevBuf dslab;
    NnlsDefer dctx{};
    DevSet side;  // results of the deferred pass, sized for the side buffer's capacity
    int32_t *d_iota = nullptr;
    struct SideStream {  // where the deferred pass runs
        hipStream_t s = nullptr;
        hipEvent_t e = nullptr;
        ~SideStream() {
            if (s) (void)hipStreamDestroy(s);
            if (e) (void)hipEventDestroy(e);
        }
    } ss;
    if (defer) {
        for (int pass = 0; pass < 2; ++pass) {
            Carver c;
            c.base = (char *)dslab.p;
            dctx.counters = (int32_t *)c.take(2 * sizeof(int32_t));
            dctx.bail = (int32_t *)c.take(nv * sizeof(int32_t));
            dctx.y_side = (double *)c.take(dcap * P.n_meas * sizeof(double));
            carve(c, A, dcap, side, Carve::Results);
            d_iota = (int32_t *)c.take(dcap * sizeof(int32_t));
            if (pass == 0 && (rc = dslab.alloc(c.off))) return rc;
        }
        dctx.cap = defer_cap;
        std::vector<int32_t> idx(dcap);
        for (size_t i = 0; i < dcap; ++i) idx[i] = (int32_t)i;
        PNX_HIP(hipMemcpy(d_iota, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        // a kernel stream (lowest priority): a copy must never sit in a hardware queue behind a kernel (the download of the
        // last chunk would wait for this pass)
        if (!HipBackend::stream_create(&ss.s, true) || !HipBackend::event_create(&ss.e))
            return set_error(PNX_ERR_HIP, "deferred hand-over: stream/event setup failed");
        PNX_HIP(hipMemset(dctx.counters, 0, 2 * sizeof(int32_t)));
    }
    // the four-slot block kernel on the first n handed-over voxels (the list is 0 .. n - 1 and the count on the device is >= n:
    // the kernel stops at the n it is given), rows in the side buffer, results in `side`
    auto redo = [&](size_t n) {
        return nnls_blk_redo_device(&P, (int64_t)n, dctx.y_side, max_iter, side.d(NN_SPEC), side.d(NN_RNORM), (int8_t *)side.dev[NN_STAT],
                                    (int32_t *)side.dev[NN_ITERS], d_iota, dctx.counters, ss.s);
    };
    PipeOps ops;
    ops.h2d = [&](int k, int slot, hipStream_t s) { return h2d(A, slots[(size_t)slot].D, ring_span(bounds, k), s); };
    ops.launch = [&](int k, int slot, hipStream_t s) -> int {
        const DevSet &D = slots[(size_t)slot].D;
        const Span sp = ring_span(bounds, k);
        int r = widen(A, D, sp, s);
        if (r) return r;
        int8_t *stat = (int8_t *)D.dev[NN_STAT];
        int32_t *iters = (int32_t *)D.dev[NN_ITERS];
        if (defer) {
            NnlsDefer d = dctx;
            d.base = (int64_t)sp.v0;
            r = nnls_blk_solve_device(&P, (int64_t)sp.c, D.d(NN_Y), max_iter, D.d(NN_SPEC), D.d(NN_RNORM), stat, iters, s, &d);
            if (!r && C.overlap && k == n_chunks - 1) {
                // every chunk has appended its handed-over voxels: ONE pass over the side buffer, on a stream of its own behind
                // this chunk's solve, while the chunk's spectra go home (8 ms of download, 9 ms of pass) -- launched before the
                // host knows how many voxels it holds, so on the buffer's whole capacity
                PNX_HIP(hipEventRecord(ss.e, s));
                PNX_HIP(hipStreamWaitEvent(ss.s, ss.e, 0));
                r = redo(dcap);
            }
        } else {
            r = nnls_solve_device(&P, (int64_t)sp.c, D.d(NN_Y), max_iter, D.d(NN_SPEC), D.d(NN_RNORM), stat, iters, s);
        }
        if (!r && C.post) r = C.post(sp.c, D.d(NN_Y), D, s);
        return r ? r : narrow(A, D, sp, s);
    };
    ops.touch = [&](int k) { touch(A, ring_span(bounds, k)); };
    ops.d2h = [&](int k, int slot, hipStream_t s) { return d2h(A, slots[(size_t)slot].D, ring_span(bounds, k), s); };
    HostCallGuard hg;
    rc = run_pipeline(n_chunks, n_slots, 1, hg.touchers(), P.device, st, ops);
    if (rc || !defer) return rc;

    PNX_HIP(hipStreamSynchronize(ss.s));  // the pass behind the last chunk's solve
    int32_t cnt[2] = {0, 0};
    PNX_HIP(hipMemcpy(cnt, dctx.counters, sizeof(cnt), hipMemcpyDeviceToHost));
    if (cnt[0] == 0) return PNX_OK;
    if (cnt[0] < 0 || (size_t)cnt[0] > nv) return set_error(PNX_ERR_HIP, "deferred hand-over: %d voxels counted in a call of %zu", cnt[0], nv);
    const size_t n = (size_t)cnt[0], batch = n < dcap ? n : dcap;
    std::vector<int32_t> where(n);
    PNX_HIP(hipMemcpy(where.data(), dctx.bail, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if ((rc = check_rows(where.data(), n, nv))) return rc;
    // More handed-over voxels than the side buffer holds (stronger regularisers than the reference's: a few per cent of the
    // voxels): the first pass has solved the first defer_cap of them (the side buffer holds their signal rows, gathered chunk
    // by chunk on the device); the others follow in batches of defer_cap, their signal rows gathered from the caller's array.
    std::vector<std::vector<char>> res((size_t)A.n);
    const void *rows[ArrayTable::kMax] = {};
    for (int k = 0; k < A.n; ++k)
        if (A.a[k].out && A.a[k].host) {
            res[(size_t)k].resize(batch * A.a[k].w * (A.a[k].widen ? sizeof(double) : A.a[k].esize));
            rows[k] = res[(size_t)k].data();
        }
    std::vector<double> y_rows;
    for (size_t b0 = 0; b0 < n; b0 += batch) {
        const size_t nb = (n - b0) < batch ? (n - b0) : batch;
        if (b0 > 0) {
            y_rows.resize(nb * (size_t)P.n_meas);
            gather_rows(A.a[NN_Y], where.data() + b0, nb, y_rows.data());
            PNX_HIP(hipMemcpy(dctx.y_side, y_rows.data(), y_rows.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        if ((b0 > 0 || !C.overlap) && (rc = redo(nb))) return rc;
        if (C.post && (rc = C.post(nb, dctx.y_side, side, ss.s))) return rc;
        PNX_HIP(hipStreamSynchronize(ss.s));
        for (int k = 0; k < A.n; ++k)
            if (rows[k]) PNX_HIP(hipMemcpy((void *)rows[k], side.dev[k], nb * A.a[k].w * (A.a[k].widen ? sizeof(double) : A.a[k].esize), hipMemcpyDeviceToHost));
        if ((rc = patch_rows(A, rows, where.data() + b0, nb, nv))) return rc;
    }
    return PNX_OK;
}

// T = double: fp64 entry point.  T = float: fp32 storage of the signal, the coefficients and rnorm; fp64 arithmetic.
template <typename T>
static int nnls_solve(pnx_nnls_plan *plan, int64_t n_vox, const T *y, int max_iter, T *coeff, T *rnorm, int8_t *status,
                      int32_t *iters, int mem, void *stream) {
    constexpr bool F32 = sizeof(T) == 4;
    if (!plan) return set_error(PNX_ERR_INVALID, "plan is NULL");
    if (n_vox < 0 || (n_vox && (!y || !coeff || !rnorm))) return set_error(PNX_ERR_INVALID, "NULL data pointer");
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    if (n_vox == 0) return PNX_OK;
    NnlsPlanData &P = plan->d;
    PNX_HIP(hipSetDevice(P.device));
    hipStream_t st = (hipStream_t)stream;
    if (max_iter <= 0) max_iter = 3 * P.n_bins;  // scipy/optimize/_nnls.py:93-94
    const size_t nv = (size_t)n_vox;
    NnlsHostCall C;
    C.A.add(y, sizeof(T), P.n_meas, false, F32);
    C.A.add(coeff, sizeof(T), P.n_bins, true, F32);
    C.A.add(rnorm, sizeof(T), 1, true, F32);
    C.A.add(status, 1, 1, true).always = true;
    C.A.add(iters, sizeof(int32_t), 1, true).always = true;
    if (mem == PNX_MEM_DEVICE) {
        // float32: converted in pieces of the kernel's own chunk so that the fp64 scratch stays at 2.4 GB
        const size_t piece = F32 && (size_t)kAtyChunk < nv ? (size_t)kAtyChunk : nv;
        AsyncBuf scratch;
        DevSet D;
        Carver sizing;
        carve(sizing, C.A, piece, D, Carve::CallerDevice);
        int rc;
        if (sizing.off && (rc = scratch.alloc(sizing.off, st))) return rc;
        for (size_t off = 0; off < nv; off += piece) {
            const size_t c = (nv - off) < piece ? (nv - off) : piece;
            Carver cv;
            cv.base = (char *)scratch.p;
            carve(cv, C.A, piece, D, Carve::CallerDevice, off);
            const Span s{nv, off, c, 0, c};
            if ((rc = widen(C.A, D, s, st)) ||
                (rc = nnls_solve_device(&P, (int64_t)c, D.d(NN_Y), max_iter, D.d(NN_SPEC), D.d(NN_RNORM), (int8_t *)D.dev[NN_STAT],
                                        (int32_t *)D.dev[NN_ITERS], st)) ||
                (rc = narrow(C.A, D, s, st)))
                return rc;
        }
        return PNX_OK;
    }
    std::lock_guard<std::mutex> plan_lock(plan->mu);
    // every chunk is one launch of the solver plus (block kernel) one hand-over pass of ~8 ms: C4 from numpy arrays takes
    // 759 / 712 / 682 / 698 ms with chunks of 256 Ki / 512 Ki / 768 Ki / 1 Mi voxels (profiles/nnls_host_chunk.py) -- beyond
    // 768 Ki the last chunk's download (2 KB per voxel) is what grows.  The ramp only for block-kernel plans, whose hand-over
    // pass is deferred (a chunk more costs ~1.5 ms, not 8): the download left exposed at the end is 0.4 GB instead of 1.6.
    C.chunk = (size_t)dev_env_int("PNX_NNLS_HOST_CHUNK", 3 << 18, 1024, 1 << 22);
    C.ramp = P.path == NnlsPath::Blk;
    C.overlap = true;
    return nnls_host(P, nv, max_iter, C, st);
}

extern "C" {
int pnx_nnls_solve_f64(pnx_nnls_plan *plan, int64_t n_vox, const double *y, int max_iter, double *coeff,
                       double *rnorm, int8_t *status, int32_t *iters, int mem, void *stream) {
    return nnls_solve<double>(plan, n_vox, y, max_iter, coeff, rnorm, status, iters, mem, stream);
}

int pnx_nnls_solve_f32(pnx_nnls_plan *plan, int64_t n_vox, const float *y, int max_iter, float *coeff, float *rnorm,
                       int8_t *status, int32_t *iters, int mem, void *stream) {
    return nnls_solve<float>(plan, n_vox, y, max_iter, coeff, rnorm, status, iters, mem, stream);
}

// solve -> [data-term residual] -> peak table per chunk, while the chunk's spectra are resident; ss_res null: no residual pass
static int nnls_solve_peaks(pnx_nnls_plan *plan, int64_t n_vox, const double *y, int max_iter, const double *bins_host,
                            double height, int regularized, double rel_height, int max_peaks, int32_t *n_peaks,
                            double *d_values, double *f_values, int n_cut, const double *cutoffs_host, double *d_cut,
                            double *f_cut, double *rnorm, int8_t *status, int32_t *iters, int mem, void *stream, double *ss_res) {
    if (!plan) return set_error(PNX_ERR_INVALID, "plan is NULL");
    if (n_vox < 0 || (n_vox && (!y || !rnorm))) return set_error(PNX_ERR_INVALID, "NULL data pointer");
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    if (n_vox == 0) return PNX_OK;
    NnlsPlanData &P = plan->d;
    PNX_HIP(hipSetDevice(P.device));
    hipStream_t st = (hipStream_t)stream;
    if (max_iter <= 0) max_iter = 3 * P.n_bins;
    std::lock_guard<std::mutex> plan_lock(plan->mu);
    const size_t nv = (size_t)n_vox;
    if (mem == PNX_MEM_HOST) {
        // the chunk ring of nnls_solve with the peak analysis behind every chunk's solve (the chunk's spectra never leave the
        // device) and the same deferred hand-over: the handed-over voxels' spectra are solved in one pass after the ring,
        // analysed, and their rows of the peak tables patched on the host
        if (max_peaks > 0 && (!d_values || !f_values)) return set_error(PNX_ERR_INVALID, "d_values / f_values are NULL");
        if (n_cut > 0 && (!cutoffs_host || !d_cut || !f_cut)) return set_error(PNX_ERR_INVALID, "cutoffs / d_cut / f_cut are NULL");
        const size_t mp = (size_t)(max_peaks > 0 ? max_peaks : 1), nc = (size_t)(n_cut > 0 ? n_cut : 1);
        NnlsHostCall C;
        C.A.add(y, sizeof(double), P.n_meas, false);
        C.A.add(nullptr, sizeof(double), P.n_bins, true).always = true;
        C.A.add(rnorm, sizeof(double), 1, true);
        C.A.add(status, 1, 1, true).always = true;
        C.A.add(iters, sizeof(int32_t), 1, true).always = true;
        C.A.add(n_peaks, sizeof(int32_t), 1, true).always = true;
        C.A.add(max_peaks > 0 ? d_values : nullptr, sizeof(double), mp, true).always = true;
        C.A.add(max_peaks > 0 ? f_values : nullptr, sizeof(double), mp, true).always = true;
        C.A.add(n_cut > 0 ? d_cut : nullptr, sizeof(double), nc, true).always = true;
        C.A.add(n_cut > 0 ? f_cut : nullptr, sizeof(double), nc, true).always = true;
        C.A.add(ss_res, sizeof(double), 1, true);
        C.chunk = (size_t)dev_env_int("PNX_NNLS_PEAKS_CHUNK", 3 << 18, 1024, 1 << 22);
        C.post = [&](size_t n, const double *y_d, const DevSet &D, hipStream_t s) {
            if (ss_res)
                if (int r = nnls_fit_stats_device(&P, (int64_t)n, y_d, D.d(NN_SPEC), D.d(NN_SS), nullptr, s)) return r;
            return pnx_nnls_spectrum_peaks_f64((int64_t)n, P.n_bins, D.d(NN_SPEC), bins_host, height, regularized, rel_height, max_peaks,
                                               (int32_t *)D.dev[NN_NPEAKS], D.d(NN_D), D.d(NN_F), n_cut, cutoffs_host, D.d(NN_DC),
                                               D.d(NN_FC), PNX_MEM_DEVICE, P.device, s);
        };
        return nnls_host(P, nv, max_iter, C, st);
    }
    // device arrays: the spectra of one chunk live in device scratch only: solve -> peak analysis -> next chunk
    const size_t chunk = (size_t)dev_env_int("PNX_NNLS_PEAKS_CHUNK", 1 << 20, 1024, 1 << 22);
    DevBuf spec;
    int rc;
    if ((rc = spec.alloc((nv < chunk ? nv : chunk) * P.n_bins * sizeof(double)))) return rc;
    for (size_t off = 0; off < nv; off += chunk) {
        const size_t n = (nv - off) < chunk ? (nv - off) : chunk;
        if ((rc = nnls_solve_device(&P, (int64_t)n, y + off * P.n_meas, max_iter, (double *)spec.p, rnorm + off,
                                    status ? status + off : nullptr, iters ? iters + off : nullptr, st)))
            return rc;
        if (ss_res && (rc = nnls_fit_stats_device(&P, (int64_t)n, y + off * P.n_meas, (const double *)spec.p, ss_res + off, nullptr, st))) return rc;
        rc = pnx_nnls_spectrum_peaks_f64((int64_t)n, P.n_bins, (const double *)spec.p, bins_host, height, regularized, rel_height,
                                         max_peaks, n_peaks ? n_peaks + off : nullptr, d_values ? d_values + off * max_peaks : nullptr,
                                         f_values ? f_values + off * max_peaks : nullptr, n_cut, cutoffs_host,
                                         d_cut ? d_cut + off * n_cut : nullptr, f_cut ? f_cut + off * n_cut : nullptr,
                                         PNX_MEM_DEVICE, P.device, st);
        if (rc) return rc;
        // the spectrum scratch is reused by the next chunk: in-order on one stream
    }
    PNX_HIP(hipStreamSynchronize(st));  // the scratch buffer is freed on return
    return PNX_OK;
}

int pnx_nnls_solve_peaks_f64(pnx_nnls_plan *plan, int64_t n_vox, const double *y, int max_iter, const double *bins_host,
                             double height, int regularized, double rel_height, int max_peaks, int32_t *n_peaks,
                             double *d_values, double *f_values, int n_cut, const double *cutoffs_host, double *d_cut,
                             double *f_cut, double *rnorm, int8_t *status, int32_t *iters, int mem, void *stream) {
    return nnls_solve_peaks(plan, n_vox, y, max_iter, bins_host, height, regularized, rel_height, max_peaks, n_peaks, d_values, f_values,
                            n_cut, cutoffs_host, d_cut, f_cut, rnorm, status, iters, mem, stream, nullptr);
}

int pnx_nnls_solve_peaks_stats_f64(pnx_nnls_plan *plan, int64_t n_vox, const double *y, int max_iter, const double *bins_host,
                                   double height, int regularized, double rel_height, int max_peaks, int32_t *n_peaks,
                                   double *d_values, double *f_values, int n_cut, const double *cutoffs_host, double *d_cut,
                                   double *f_cut, double *rnorm, int8_t *status, int32_t *iters, int mem, void *stream,
                                   double *ss_res) {
    if (n_vox > 0 && !ss_res) return set_error(PNX_ERR_INVALID, "ss_res is NULL");
    return nnls_solve_peaks(plan, n_vox, y, max_iter, bins_host, height, regularized, rel_height, max_peaks, n_peaks, d_values, f_values,
                            n_cut, cutoffs_host, d_cut, f_cut, rnorm, status, iters, mem, stream, ss_res);
}

int pnx_nnls_fit_stats_f64(pnx_nnls_plan *plan, int64_t n_vox, const double *y, const double *coeff, double *ss_res, double *pred,
                           int mem, int device, void *stream) {
    if (!plan) return set_error(PNX_ERR_INVALID, "plan is NULL");
    if (!ss_res && !pred) return set_error(PNX_ERR_INVALID, "ss_res and pred are both NULL");
    if (n_vox < 0 || (n_vox && (!coeff || (ss_res && !y)))) return set_error(PNX_ERR_INVALID, "NULL data pointer");
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    const NnlsPlanData &P = plan->d;
    if (device != P.device) return set_error(PNX_ERR_INVALID, "device %d, but the plan lives on device %d", device, P.device);
    if (n_vox == 0) return PNX_OK;
    PNX_HIP(hipSetDevice(P.device));
    hipStream_t st = (hipStream_t)stream;
    if (mem == PNX_MEM_DEVICE) return nnls_fit_stats_device(&P, n_vox, y, coeff, ss_res, pred, st);
    // the kernel only reads the plan (its padded basis): no lock, two kernel streams
    enum { FS_Y, FS_X, FS_SS, FS_PRED };
    ArrayTable A;
    A.add(ss_res ? y : nullptr, sizeof(double), P.n_meas, false);
    A.add(coeff, sizeof(double), P.n_bins, false);
    A.add(ss_res, sizeof(double), 1, true);
    A.add(pred, sizeof(double), P.n_meas, true);
    HostCallGuard hg;
    return chunk_ring(A, (size_t)n_vox, (size_t)dev_env_int("PNX_STATS_HOST_CHUNK", 1 << 18, 1024, 1 << 22), 3, 2, hg.touchers(), P.device, st,
                      [&](size_t c, const DevSet &D, hipStream_t s) {
                          return nnls_fit_stats_device(&P, (int64_t)c, D.d(FS_Y), D.d(FS_X), D.d(FS_SS), D.d(FS_PRED), s);
                      });
}

int pnx_nnls_aty_f64(pnx_nnls_plan *plan, int64_t n_vox, const double *y_dev, double *aty_dev, void *stream) {
    if (!plan) return set_error(PNX_ERR_INVALID, "plan is NULL");
    if (n_vox < 0 || (n_vox && !y_dev)) return set_error(PNX_ERR_INVALID, "NULL data pointer");
    if (n_vox == 0) return PNX_OK;
    PNX_HIP(hipSetDevice(plan->d.device));
    return nnls_aty_device(&plan->d, n_vox, y_dev, aty_dev, (hipStream_t)stream);
}

int pnx_nnls_batch_f64(int64_t n_vox, int n_meas, int n_bins, const double *basis, const double *reg, int n_reg,
                       const double *y, int max_iter, double *coeff, double *rnorm, int8_t *status, int32_t *iters,
                       int device) {
    pnx_nnls_plan *plan = nullptr;
    int rc = pnx_nnls_plan_create(&plan, n_meas, n_bins, basis, reg, n_reg, device);
    if (rc) return rc;
    rc = pnx_nnls_solve_f64(plan, n_vox, y, max_iter, coeff, rnorm, status, iters, PNX_MEM_HOST, nullptr);
    pnx_nnls_plan_destroy(plan);
    return rc;
}

// model_functions/nnls.py:17-28  np.logspace(log10(dmin), log10(dmax), n) = 10 ** linspace(...)
int pnx_nnls_bins(double d_min, double d_max, int n_bins, double *bins) {
    if (!bins || n_bins < 1 || !(d_min > 0) || !(d_max > 0)) return set_error(PNX_ERR_INVALID, "bad bins arguments");
    const double a = log10(d_min), b = log10(d_max);
    const double step = n_bins > 1 ? (b - a) / (double)(n_bins - 1) : 0.0;
    for (int i = 0; i < n_bins; ++i) {
        double e = a + (double)i * step;  // np.linspace: start + i*step, last point forced to `stop`
        if (i == n_bins - 1 && n_bins > 1) e = b;
        bins[i] = pow(10.0, e);
    }
    return PNX_OK;
}

// model_functions/nnls.py:46-85
int pnx_nnls_regularization_matrix(int n_bins, int order, double mu, double *reg) {
    if (!reg || n_bins < 1) return set_error(PNX_ERR_INVALID, "bad regularization arguments");
    if (order < 0 || order > 3) return set_error(PNX_ERR_UNSUPPORTED, "Regularization order %d not supported. Use 0-3.", order);
    const size_t n = (size_t)n_bins;
    for (size_t i = 0; i < n * n; ++i) reg[i] = 0.0;
    for (size_t i = 0; i < n; ++i) {
        if (order == 1) {
            reg[i * n + i] = -1.0 * mu;
            if (i + 1 < n) reg[i * n + i + 1] = 1.0 * mu;
        } else if (order == 2) {
            reg[i * n + i] = -2.0 * mu;
            if (i + 1 < n) reg[i * n + i + 1] = 1.0 * mu;
            if (i >= 1) reg[i * n + i - 1] = 1.0 * mu;
        } else if (order == 3) {
            reg[i * n + i] = -6.0 * mu;
            if (i + 1 < n) reg[i * n + i + 1] = 2.0 * mu;
            if (i >= 1) reg[i * n + i - 1] = 2.0 * mu;
            if (i + 2 < n) reg[i * n + i + 2] = 1.0 * mu;
            if (i >= 2) reg[i * n + i - 2] = 1.0 * mu;
        }
    }
    return PNX_OK;
}

int pnx_nnls_basis(int n_meas, const double *b, int n_bins, const double *bins, double *basis, int device) {
    if (!b || !bins || !basis || n_meas < 1 || n_bins < 1) return set_error(PNX_ERR_INVALID, "bad basis arguments");
    DeviceInfo *dev;
    int rc = use_device(device, &dev);
    if (rc) return rc;
    return nnls_build_basis(n_meas, b, n_bins, bins, basis);
}

// ---- bulk copies between pageable host arrays and device buffers -----------------------------------------------
// A pageable hipMemcpy is staged by the calling thread (about 10 GB/s of memcpy into the runtime's pinned buffers) and
// a fresh destination array takes its first-touch page faults inside the copy (42 ms per GB).  Here the range is cut into
// 32 MiB pieces handed to a few threads, each with its own stream: staging copies, DMA and page faults overlap.
static int bulk_copy(void *dst, const void *src, size_t bytes, bool to_device, int device, hipStream_t after, int threads) {
    if (!bytes) return PNX_OK;
    if (!dst || !src) return set_error(PNX_ERR_INVALID, "NULL pointer");
    DeviceInfo *dev;
    int rc = use_device(device, &dev);
    if (rc) return rc;
    PNX_HIP(hipStreamSynchronize(after));  // the producer of a device source / the last reader of a device destination
    const size_t piece = (size_t)env_int("PNX_COPY_PIECE_MB", 32, 1, 1024) << 20;
    const size_t n_pieces = (bytes + piece - 1) / piece;
    int nt = threads > 0 ? threads : env_int("PNX_COPY_THREADS", 4, 1, 16);
    if ((size_t)nt > n_pieces) nt = (int)n_pieces;
    std::atomic<size_t> next(0);
    std::atomic<int> code(PNX_OK);
    std::mutex mu;
    std::string msg;
    auto work = [&]() {
        hipStream_t st = nullptr;
        if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
            code.store(PNX_ERR_HIP);
            std::lock_guard<std::mutex> lk(mu);
            msg = "bulk copy: stream setup failed";
            return;
        }
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= n_pieces || code.load() != PNX_OK) break;
            const size_t off = k * piece, len = (bytes - off) < piece ? (bytes - off) : piece;
            if (!to_device) touch_pages((char *)dst + off, len);
            hipError_t e = hipMemcpyAsync((char *)dst + off, (const char *)src + off, len,
                                          to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                code.store(PNX_ERR_HIP);
                std::lock_guard<std::mutex> lk(mu);
                msg = std::string("bulk copy: ") + hipGetErrorString(e);
                break;
            }
        }
        (void)hipStreamDestroy(st);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    if (code.load() != PNX_OK) return set_error(code.load(), "%s", msg.c_str());
    return PNX_OK;
}

int pnx_upload(void *dst_device, const void *src_host, int64_t bytes, int device, void *stream, int threads) {
    if (bytes < 0) return set_error(PNX_ERR_INVALID, "negative byte count");
    return bulk_copy(dst_device, src_host, (size_t)bytes, true, device, (hipStream_t)stream, threads);
}

int pnx_download(void *dst_host, const void *src_device, int64_t bytes, int device, void *stream, int threads) {
    if (bytes < 0) return set_error(PNX_ERR_INVALID, "negative byte count");
    return bulk_copy(dst_host, src_device, (size_t)bytes, false, device, (hipStream_t)stream, threads);
}

}  // extern "C"

// ---- per-label sums of an (n, c) row matrix: the reduction in front of a segmentation-wise fit ---------------------
// Deterministic on purpose (no atomics): wave w owns a contiguous range of rows and adds them, in order, into its own LDS
// table [n_labels][c] (lane k owns column k); a second kernel adds the per-wave tables in wave order.
namespace pnx {
constexpr int kLabelWaves = 2048;
constexpr int kLabelUnroll = 8;

__global__ void __launch_bounds__(64) label_partial_kernel(const double *img, const int32_t *lab, long long n, int c, int n_lab,
                                                           double *part, long long *cnt_part) {
    extern __shared__ double tab[];  // [n_lab][c] doubles, then n_lab counts
    long long *cnt = reinterpret_cast<long long *>(tab + (size_t)n_lab * c);
    const int lane = threadIdx.x;
    for (int e = lane; e < n_lab * c; e += 64) tab[e] = 0.0;
    for (int e = lane; e < n_lab; e += 64) cnt[e] = 0;
    __syncthreads();
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long v0 = (long long)blockIdx.x * per;
    const long long v1 = (v0 + per) < n ? (v0 + per) : n;
    for (int k0 = 0; k0 < c; k0 += 64) {  // one pass per 64 columns (c <= 64: a single pass)
        const int k = k0 + lane;
        const bool on = k < c;
        long long v = v0;
        for (; v + kLabelUnroll <= v1; v += kLabelUnroll) {
            int l[kLabelUnroll];
            double x[kLabelUnroll];
#pragma unroll
            for (int u = 0; u < kLabelUnroll; ++u) {  // the loads of eight rows are in flight together
                l[u] = lab[v + u];
                x[u] = on ? img[(size_t)(v + u) * c + k] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kLabelUnroll; ++u) {
                if ((unsigned)l[u] < (unsigned)n_lab) {
                    if (on) tab[(size_t)l[u] * c + k] += x[u];
                    if (k0 == 0 && lane == 0) cnt[l[u]] += 1;
                }
            }
        }
        for (; v < v1; ++v) {
            const int l = lab[v];
            if ((unsigned)l < (unsigned)n_lab) {
                if (on) tab[(size_t)l * c + k] += img[(size_t)v * c + k];
                if (k0 == 0 && lane == 0) cnt[l] += 1;
            }
        }
    }
    __syncthreads();
    double *dst = part + (size_t)blockIdx.x * n_lab * c;
    for (int e = lane; e < n_lab * c; e += 64) dst[e] = tab[e];
    for (int e = lane; e < n_lab; e += 64) cnt_part[(size_t)blockIdx.x * n_lab + e] = cnt[e];
}

__global__ void label_reduce_kernel(const double *part, const long long *cnt_part, int waves, int n_lab, int c, double *sums,
                                    long long *counts) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_lab * c) {
        double s = 0.0;
        for (int w = 0; w < waves; ++w) s += part[(size_t)w * n_lab * c + e];
        sums[e] = s;
    }
    if (e < n_lab) {
        long long m = 0;
        for (int w = 0; w < waves; ++w) m += cnt_part[(size_t)w * n_lab + e];
        counts[e] = m;
    }
}
}  // namespace pnx

extern "C" int pnx_label_sums_f64(const double *rows, const int32_t *labels, int64_t n, int c, int n_labels, double *sums,
                                  int64_t *counts, int mem, int device, void *stream) {
    using namespace pnx;
    if (n < 0 || c < 1 || n_labels < 1) return set_error(PNX_ERR_INVALID, "bad label-sum sizes (n=%lld, c=%d, n_labels=%d)", (long long)n, c, n_labels);
    if (!sums || !counts || (n && (!rows || !labels))) return set_error(PNX_ERR_INVALID, "NULL pointer");
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem must be PNX_MEM_HOST or PNX_MEM_DEVICE");
    const size_t lds = ((size_t)n_labels * c + n_labels) * sizeof(double);
    if (lds > 64 * 1024) return set_error(PNX_ERR_UNSUPPORTED, "n_labels * (c + 1) = %zu entries do not fit the 64 KB LDS table", lds / 8);
    DeviceInfo *dev;
    int rc = use_device(device, &dev);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool host = mem == PNX_MEM_HOST;
    const size_t tab = (size_t)n_labels * c;
    int waves = (int)((n + 63) / 64);
    if (waves > kLabelWaves) waves = kLabelWaves;
    if (waves < 1) waves = 1;
    DevBuf d_rows, d_lab, d_part, d_cnt, d_sums, d_counts;
    if ((rc = d_part.alloc((size_t)waves * tab * sizeof(double))) || (rc = d_cnt.alloc((size_t)waves * n_labels * sizeof(long long)))) return rc;
    const double *rows_d = rows;
    const int32_t *lab_d = labels;
    double *sums_d = sums;
    long long *counts_d = reinterpret_cast<long long *>(counts);
    if (host) {
        if ((rc = d_rows.alloc((size_t)n * c * sizeof(double))) || (rc = d_lab.alloc((size_t)n * sizeof(int32_t))) ||
            (rc = d_sums.alloc(tab * sizeof(double))) || (rc = d_counts.alloc((size_t)n_labels * sizeof(long long))))
            return rc;
        if ((rc = bulk_copy(d_rows.p, rows, (size_t)n * c * sizeof(double), true, device, st, 0))) return rc;
        if ((rc = bulk_copy(d_lab.p, labels, (size_t)n * sizeof(int32_t), true, device, st, 0))) return rc;
        rows_d = (const double *)d_rows.p;
        lab_d = (const int32_t *)d_lab.p;
        sums_d = (double *)d_sums.p;
        counts_d = (long long *)d_counts.p;
    }
    hipLaunchKernelGGL(label_partial_kernel, dim3(waves), dim3(64), lds, st, rows_d, lab_d, (long long)n, c, n_labels,
                       (double *)d_part.p, (long long *)d_cnt.p);
    PNX_HIP(hipGetLastError());
    hipLaunchKernelGGL(label_reduce_kernel, dim3((unsigned)((tab + 255) / 256)), dim3(256), 0, st, (const double *)d_part.p,
                       (const long long *)d_cnt.p, waves, n_labels, c, sums_d, counts_d);
    PNX_HIP(hipGetLastError());
    if (host) {
        PNX_HIP(hipMemcpyAsync(sums, sums_d, tab * sizeof(double), hipMemcpyDeviceToHost, st));
        PNX_HIP(hipMemcpyAsync(counts, counts_d, (size_t)n_labels * sizeof(long long), hipMemcpyDeviceToHost, st));
    }
    PNX_HIP(hipStreamSynchronize(st));  // the scratch tables are freed on return
    return PNX_OK;
}
