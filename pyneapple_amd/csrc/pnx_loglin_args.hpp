// pnx_loglin_args.hpp -- the host half of pnx_loglinear_f64 / _f32 that needs no device: the argument checks in front of any
// device work and the by-value form the kernel receives (b-values and bounds as fp64, the mask as bits).  Free of HIP types, like
// pnx_grid_args.hpp: pnx_api.hip and pnx_loglin.hip use it, tests/host_stub/loglin_args_stub.cpp builds the same code for the
// CPU under AddressSanitizer / UBSan.
#pragma once
#include "pnx_args_common.hpp"
#include "pnx_tile.hpp"

namespace pnx {
constexpr int kLogLinMaxReweight = 8;

// What a call hands the kernel by value: 1 KB of b-values, 128 mask bits, the switches and the clip bounds.
struct LogLinOpts {
    int n_b;
    int weighting;   // 0: w = 1, 1: w = y^2
    int n_reweight;  // further passes with w = exp(a - b D)^2
    int clip;
    unsigned long long use[PNX_MAX_BVALUES / 64];  // bit i: b-value i takes part
    double lo[2], hi[2];
    double b[PNX_MAX_BVALUES];
};

// T: the storage type of the entry point (double, or float for pnx_loglinear_f32).  Checks in the order the header lists them;
// nothing is read before the check that makes reading it safe (n_b before b, clip before the bounds).  Fills *o on success.
template <typename T>
inline int loglin_check_args(int64_t n_vox, int n_b, const T *b, const uint8_t *use, int weighting, int n_reweight, int clip, const T *lo,
                             const T *hi, const void *y, const void *params, int mem, LogLinOpts *o) {
    if (n_b < 2 || n_b > PNX_MAX_BVALUES) return set_error(PNX_ERR_INVALID, "loglinear: n_b=%d out of range [2,%d]", n_b, PNX_MAX_BVALUES);
    if (n_vox < 0) return set_error(PNX_ERR_INVALID, "loglinear: n_vox < 0");
    if (!b) return set_error(PNX_ERR_INVALID, "loglinear: b is NULL");
    if (n_vox && !y) return set_error(PNX_ERR_INVALID, "loglinear: y is NULL");
    if (n_vox && !params) return set_error(PNX_ERR_INVALID, "loglinear: params is NULL");
    int rc;
    if ((rc = args_check_b("loglinear", n_b, b)) || (rc = args_check_weighting("loglinear", weighting))) return rc;
    if (n_reweight < 0 || n_reweight > kLogLinMaxReweight)
        return set_error(PNX_ERR_INVALID, "loglinear: n_reweight=%d out of range [0,%d]", n_reweight, kLogLinMaxReweight);
    const MaskRow m = args_mask_row(n_b, b, use);
    if (m.kept < 2) return set_error(PNX_ERR_INVALID, "loglinear: use keeps %d of %d b-values, a line needs 2", m.kept, n_b);
    if (!m.distinct) return set_error(PNX_ERR_INVALID, "loglinear: the b-values that use keeps are all equal (%g), a line needs 2 distinct ones", (double)b[m.first]);
    if ((rc = args_check_clip("loglinear", clip, 2, lo, hi)) || (rc = args_check_mem("loglinear", mem))) return rc;
    o->n_b = n_b;
    o->weighting = weighting;
    o->n_reweight = n_reweight;
    o->clip = clip != 0;
    args_pack_mask(n_b, use, o->use);
    args_copy_b(n_b, b, o->b);
    for (int k = 0; k < 2; ++k) {
        o->lo[k] = clip ? (double)lo[k] : 0.0;
        o->hi[k] = clip ? (double)hi[k] : 0.0;
    }
    return PNX_OK;
}

// LDS of one block: the signal tile and its logarithms (pnx_tile.hpp); 132 KB at 128 b-values, inside a workgroup's 160 KB.
inline size_t loglin_lds_bytes(int n_b) { return tile_lds_bytes(2, n_b); }
}  // namespace pnx
