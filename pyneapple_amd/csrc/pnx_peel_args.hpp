// pnx_peel_args.hpp -- the host half of pnx_peel_f64 / _f32 that needs no device: the argument checks in front of any device work
// and the by-value form the kernel receives (b-values, bounds and fallback as fp64, the K stage masks as bits).  Free of HIP
// types, like pnx_loglin_args.hpp: pnx_api.hip and pnx_peel.hip use it, tests/host_stub/peel_args_stub.cpp builds the same code
// for the CPU under AddressSanitizer / UBSan.
#pragma once
#include "pnx_args_common.hpp"
#include "pnx_tile.hpp"

namespace pnx {
constexpr int kPeelMaxStages = 3;
constexpr int kPeelMaxParams = 6;

// number of exponentials of a layout (0: unknown model) and its number of parameters
inline int peel_n_exp(int model) {
    if (model == PNX_MODEL_MONO) return 1;
    if (model >= PNX_MODEL_BI_REDUCED && model <= PNX_MODEL_BI_FULL) return 2;
    if (model >= PNX_MODEL_TRI_REDUCED && model <= PNX_MODEL_TRI_FULL) return 3;
    return 0;
}
inline int peel_n_params(int model) {
    static const int n[7] = {2, 3, 4, 4, 5, 6, 6};
    return peel_n_exp(model) ? n[model] : 0;
}

// What a call hands the kernel by value: 1 KB of b-values, 3 x 128 mask bits, the switches, the clip bounds and the fallback.
struct PeelOpts {
    int model, n_stage, n_params, n_b;
    int weighting;  // 0: w = 1, 1: w = r^2
    int clip, has_fallback;
    unsigned long long use[kPeelMaxStages][PNX_MAX_BVALUES / 64];  // bit i of row k: b-value i takes part in stage k
    double lo[kPeelMaxParams], hi[kPeelMaxParams], fallback[kPeelMaxParams];
    double b[PNX_MAX_BVALUES];
};

// T: the storage type of the entry point (double, or float for pnx_peel_f32).  Checks in the order the header lists them; nothing
// is read before the check that makes reading it safe (model before n_b, n_b before b and use, clip before the bounds).  Fills *o
// on success.
template <typename T>
inline int peel_check_args(int model, int64_t n_vox, int n_b, const T *b, const uint8_t *use, int weighting, int clip, const T *lo,
                           const T *hi, const T *fallback, const void *y, const void *params, int mem, PeelOpts *o) {
    const int K = peel_n_exp(model), np = peel_n_params(model);
    if (!K) return set_error(PNX_ERR_INVALID, "peel: unknown model %d", model);
    if (n_b < 2 * K || n_b > PNX_MAX_BVALUES)
        return set_error(PNX_ERR_INVALID, "peel: n_b=%d out of range [%d,%d] for %d exponentials", n_b, 2 * K, PNX_MAX_BVALUES, K);
    if (n_vox < 0) return set_error(PNX_ERR_INVALID, "peel: n_vox < 0");
    if (!b) return set_error(PNX_ERR_INVALID, "peel: b is NULL");
    if (!use) return set_error(PNX_ERR_INVALID, "peel: use is NULL");
    if (n_vox && !y) return set_error(PNX_ERR_INVALID, "peel: y is NULL");
    if (n_vox && !params) return set_error(PNX_ERR_INVALID, "peel: params is NULL");
    int rc;
    if ((rc = args_check_b("peel", n_b, b)) || (rc = args_check_weighting("peel", weighting))) return rc;
    for (int k = 0; k < K; ++k) {
        const MaskRow m = args_mask_row(n_b, b, use + (size_t)k * n_b);
        if (m.kept < 2) return set_error(PNX_ERR_INVALID, "peel: use row %d keeps %d of %d b-values, a line needs 2", k, m.kept, n_b);
        if (!m.distinct)
            return set_error(PNX_ERR_INVALID, "peel: the b-values that use row %d keeps are all equal (%g), a line needs 2 distinct ones", k,
                             (double)b[m.first]);
    }
    if ((rc = args_check_clip("peel", clip, np, lo, hi)) || (rc = args_check_mem("peel", mem))) return rc;
    o->model = model;
    o->n_stage = K;
    o->n_params = np;
    o->n_b = n_b;
    o->weighting = weighting;
    o->clip = clip != 0;
    o->has_fallback = fallback != nullptr;
    for (int k = 0; k < kPeelMaxStages; ++k)  // the rows past K: no bits
        args_pack_mask(k < K ? n_b : 0, k < K ? use + (size_t)k * n_b : nullptr, o->use[k]);
    args_copy_b(n_b, b, o->b);
    for (int j = 0; j < kPeelMaxParams; ++j) {
        const bool in = j < np;
        o->lo[j] = clip && in ? (double)lo[j] : 0.0;
        o->hi[j] = clip && in ? (double)hi[j] : 0.0;
        o->fallback[j] = fallback && in ? (double)fallback[j] : 0.0;
    }
    return PNX_OK;
}

// LDS of one block: the signal tile and the running residual (pnx_tile.hpp); 132 KB at 128 b-values, inside a workgroup's 160 KB.
// A third tile for the logarithms would not fit there, so the kernel keeps none at any n_b and evaluates the logarithm in both
// passes of a stage.
inline size_t peel_lds_bytes(int n_b) { return tile_lds_bytes(2, n_b); }
}  // namespace pnx
