// pnx_nnls.hpp -- internal interface of the batched NNLS solver (see pnx_nnls.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pnx {
constexpr int64_t kAtyChunk = 1 << 20;  // voxels per MFMA Gram step / active-set launch pair


constexpr int kNnlsMaxBins = 256;   // 4 bins per lane: every fast path (block kernel, MFMA Gram step, 16 waves per CU)
constexpr int kNnlsWideBins = 512;  // 8 bins per lane: the wide instantiations of the Gram- and QR-form kernels (257 .. 512 bins)
constexpr int kNnlsMaxMeas = 128;
constexpr int kNnlsBlkMaxMeas = 32;  // measurements the block kernel's LDS copy of the basis holds

// the HIP check of the NNLS translation units: a failed call becomes PNX_ERR_HIP with the call's text
#define PNX_HIPN(call)                                                                             \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess) return set_error(PNX_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

// How a plan solves, decided once by nnls_plan_init (nnls_choose_path)
enum class NnlsPath {
    Qr,        // no (or an all-zero) regulariser: QR-form kernels (pnx_nnls_qr.hip; Q and R in LDS up to 32 measurements, in a global slab beyond)
    Blk,       // banded Toeplitz regulariser, n_reg == n_bins <= 256, <= 32 measurements: block kernels (pnx_nnls_blk.hip)
    Gram,      // anything else up to 256 bins: Gram-form nnls_kernel<4, 4> (pnx_nnls.hip), A^T y from the MFMA Gram step up to 64 measurements
    GramWide,  // anything else, 257 .. 512 bins: nnls_kernel<6|8, 4>, its hand-over pass <8, 8>, A^T y on the VALU
};

struct NnlsPlanData {
    NnlsPath path = NnlsPath::Gram;
    int device = 0;
    int cus = 0;
    int n_meas = 0, n_bins = 0, n_reg = 0;
    double rc[5] = {0, 0, 0, 0, 0};  // banded Toeplitz regulariser (orders 1-3 of the reference): reg[i][j] = rc[j - i + 2]
    int rhb = 0;              // its half bandwidth, 0 = general regulariser
    unsigned long long *queue = nullptr;  // work queue of the persistent kernels (Blk, Gram, GramWide)
    // every path
    double *Bp = nullptr;     // (n_meas, bstride) zero padded copy of the basis (16-byte aligned rows for the kernels)
    int bstride = kNnlsMaxBins;  // row stride of Bp and G: 256, or 512 for a plan of more than 256 bins
    bool mfma_ok = false;     // the MFMA Gram step can run for this plan (n_meas <= 64, n_bins <= 256)
    double *aty = nullptr;    // (kAtyChunk, 256) A^T y of the current chunk: allocated with a Gram plan, on first use of pnx_nnls_aty otherwise
    // Qr
    double *qr_slab = nullptr;  // Q / R of the 33 .. 128 measurement kernel, per resident wave (allocated by its first launch)
    int qr_slab_groups = 0;
    // Blk, Gram, GramWide: the Gram form's inputs (the block kernel gathers columns of G too)
    double *B = nullptr;      // (n_meas, n_bins) row-major: basis
    double *RT = nullptr;     // (n_bins, n_reg)  row-major: reg transposed (column j of reg contiguous)
    double *G = nullptr;      // (n_bins + 1, bstride): A^T A = B^T B + reg^T reg, fp64, zero padded
    double *Mglob = nullptr;  // per-wave overflow rows (>= 48) of the inverse Cholesky factor of nnls_kernel (Blk: the device's shared slab)
    size_t mglob_stride = 0;  // doubles per wave
    int n_waves = 0;          // persistent waves of nnls_kernel the scratch was sized for
    int32_t *blk_bail = nullptr;  // [0]: number of voxels handed over, [1 ..]: their indices -- Blk: block kernel -> four-slot block kernel
                                  // (more than 128 passive bins); GramWide: nnls_kernel<8, 4> -> <8, 8> (more than 256)
    size_t blk_bail_cap = 0;      // voxels the list can hold
    // GramWide
    double *Mwide = nullptr;  // slabs of the hand-over pass nnls_kernel<8, 8> (rows up to 511), one wave per CU
    int wide_waves = 0;
    // Blk
    double *Mblk = nullptr;   // per-wave slabs of the block-distributed inverse Cholesky factor
    int blk_groups = 0;       // its persistent workgroups (12 waves each)
    double *Mblk4 = nullptr;  // the same for the four-slot instantiation (256 positions, eight waves per CU: 270 KB per wave; shared slab)
    int blk4_groups = 0;
    int32_t *blk4_bail = nullptr;  // what the four-slot instantiation hands to the Gram-form kernel (a ninth rejected candidate: test hook only)
    int32_t *route = nullptr;     // [0] the route the pilot of the current call chose (0: block kernel, 1: four-slot block kernel), device
    bool shared_slabs = false;    // Mblk4 and Mglob belong to the device's shared slab set (below), not to the plan
};

// The slabs of the two kernels BEHIND a block-kernel plan's first pass -- the four-slot block kernel (0.55 GB) and the Gram-form
// kernel that remains its last resort (1 GB) -- exist once per device, for every such plan on it: they are only used by the
// hand-over pass (one voxel in 10^4 on the reference workload) and by calls the pilot routes to the four-slot kernel, so N plans
// cost 1.55 GB + N x 0.2 GB (the two-slot kernel's own slabs), not N x 1.8 GB.  Uses are ordered on the device: a launch that
// touches them waits for the event recorded behind the previous one (another plan, another stream), enqueue order = host order
// under the set's mutex; everything stays asynchronous.  The set stays allocated while idle (a plan per call -- api.nnls,
// pnx_nnls_batch_f64 -- would otherwise pay 1.55 GB of hipMalloc + memset each time); pnx_release_staging(device) frees it.
int nnls_shared_slabs_get(int device, size_t blk4_bytes, size_t gram_bytes, double **blk4, double **gram);
void nnls_shared_slabs_put(int device);
int nnls_shared_slabs_trim(int device);  // frees the set unless a plan holds it (returns 0 then, 1 otherwise)
// acquire: locks the plan's set and orders `stream` behind its last use; release: records this use on `stream` and unlocks (also
// when it fails).  An error of either is returned; a failed acquire leaves the set unlocked.
int nnls_shared_acquire(const NnlsPlanData *P, hipStream_t stream);
int nnls_shared_release(const NnlsPlanData *P, hipStream_t stream);
// enqueue() (returns a PNX_* code) between the two when the plan uses the shared set, on its own otherwise
template <class F> int nnls_shared_use(const NnlsPlanData *P, hipStream_t stream, F &&enqueue) {
    if (!P->shared_slabs) return enqueue();
    int r = nnls_shared_acquire(P, stream);
    if (r) return r;
    r = enqueue();
    const int r2 = nnls_shared_release(P, stream);
    return r ? r : r2;
}

int nnls_plan_init(NnlsPlanData *P, int n_meas, int n_bins, const double *basis, const double *reg, int n_reg,
                   int device, int cus);
void nnls_plan_free(NnlsPlanData *P);
int nnls_solve_device(NnlsPlanData *P, int64_t n_vox, const double *y_d, int max_iter, double *coeff_d,
                      double *rnorm_d, int8_t *status_d, int32_t *iters_d, hipStream_t stream);
int nnls_qr_solve_device(NnlsPlanData *P, int64_t n_vox, const double *y_d, int max_iter, double *coeff_d, double *rnorm_d,
                         int8_t *status_d, int32_t *iters_d, hipStream_t stream);
// the general kernel on the voxels list[0 .. *count) of a chunk (A^T y on the VALU)
int nnls_redo_device(NnlsPlanData *P, int64_t n_vox, const double *y_d, int max_iter, double *coeff_d, double *rnorm_d,
                     int8_t *status_d, int32_t *iters_d, const int32_t *list, const int32_t *count, hipStream_t stream);
// block-kernel plans: the voxels list[0 .. min(*count, n_vox)) through the four-slot block kernel (hand-over target of the two-slot one)
int nnls_blk_redo_device(NnlsPlanData *P, int64_t n_vox, const double *y_d, int max_iter, double *coeff_d, double *rnorm_d,
                         int8_t *status_d, int32_t *iters_d, const int32_t *list, const int32_t *count, hipStream_t stream);
int nnls_blk_plan_init(NnlsPlanData *P);
size_t nnls_blk4_slab_bytes(const NnlsPlanData *P);  // of the four-slot kernel's grid on this plan's device (after nnls_blk_plan_init)
// Deferred hand-over (host-array calls made of several chunks, pnx_api.hip): the block kernel appends the voxels it hands over
// to `bail` with their index within the whole call (`base` + index within this chunk), a gather keeps their signal rows in
// `y_side`, and the caller solves them in one pass at the end instead of one pass per chunk.
struct NnlsDefer {
    int32_t *counters;  // device: [0] voxels handed over so far, [1] signal rows gathered so far
    int32_t *bail;      // device: indices within the call, room for every voxel of the call
    double *y_side;     // device: (cap, n_meas) signal rows of the first `cap` handed-over voxels
    int cap;
    int64_t base;       // first voxel of this chunk within the call
};
int nnls_blk_solve_device(NnlsPlanData *P, int64_t n_vox, const double *y_d, int max_iter, double *coeff_d, double *rnorm_d,
                          int8_t *status_d, int32_t *iters_d, hipStream_t stream, const NnlsDefer *defer = nullptr);
int nnls_aty_device(NnlsPlanData *P, int64_t n_vox, const double *y_d, double *aty_d, hipStream_t stream);
int nnls_build_basis(int n_meas, const double *b, int n_bins, const double *bins, double *basis);

}  // namespace pnx
