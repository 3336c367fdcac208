// pnx_grid_refine_args.hpp -- the half of pnx_curvefit_grid_refine_f64 that needs no device: the checks of its arguments in front of
// any device work, the construction of one axis of a voxel's fine grid (the kernel calls the same function), the admissibility rule
// of an atom and the sizing of the kernel's wave-private LDS.  Free of HIP types, like pnx_grid_posterior_args.hpp: pnx_api.hip and
// pnx_grid_refine.hip use it, tests/host_stub/grid_refine_stub.cpp builds the same code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_args.hpp"

#if defined(__HIPCC__)
#define PNX_REFINE_HD __host__ __device__
#else
#define PNX_REFINE_HD
#endif

namespace pnx {

constexpr int kRefineMaxPoints = 9;

// One axis of a voxel's fine grid: m values a .. b, or the single value a (= b) with m = 1 and step = 0.
struct RefineAxis {
    double a, b, step;
    int m;
};
// a = max(lo, c - hw), b = min(hi, c + hw); n_points == 1 or b <= a gives the single value min(max(c, lo), hi).
PNX_REFINE_HD inline RefineAxis grid_refine_axis(double lo, double hi, double c, double hw, int n_points) {
    RefineAxis r;
    const double a = fmax(lo, c - hw), b = fmin(hi, c + hw);
    if (n_points == 1 || !(b > a)) {
        r.a = r.b = fmin(fmax(c, lo), hi);
        r.step = 0.0;
        r.m = 1;
    } else {
        r.a = a;
        r.b = b;
        r.step = (b - a) / (double)(n_points - 1);
        r.m = n_points;
    }
    return r;
}
// x_j = fma(j, step, a) for j < m - 1; the last value is b itself, so that no value leaves [lo, hi] by a rounding.
PNX_REFINE_HD inline double grid_refine_value(const RefineAxis &r, int j) { return (j == r.m - 1) ? r.b : fma((double)j, r.step, r.a); }

// The fraction-sum rule: the implied last fraction of a reduced layout may not be negative.  f1 <= 1 for [f1, D1, D2 (, S0)],
// f1 + f2 <= 1 (one addition) for [f1, D1, f2, D2, D3 (, S0)]; the layouts that carry every fraction, and mono, admit every atom.
// p: the atom's parameters in the model's order, fixed ones included.
PNX_REFINE_HD inline bool grid_refine_admissible(int model, const double *p) {
    switch (model) {
    case PNX_MODEL_BI_REDUCED:
    case PNX_MODEL_BI_S0: return p[0] <= 1.0;
    case PNX_MODEL_TRI_REDUCED:
    case PNX_MODEL_TRI_S0: return p[0] + p[2] <= 1.0;
    }
    return true;
}

struct GridRefineHost {
    int s0_row = -1;  // row of S0 among the free parameters when the amplitude is projected
    int n_atoms = 1;  // the product of n_points: the most atoms a voxel has
    int mmax = 1;     // the largest n_points
};

// What the entry point checks behind check_curvefit_opts, in front of any device work.  Every refusal names its argument.
inline int grid_refine_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, const double *fixed,
                                  const double *lo, const double *hi, int project_amplitude, double noise_sd, const int32_t *n_points,
                                  const double *centre, const double *half_width, const double *mean, int mem, GridRefineHost *H) {
    if (o->sigma)
        return set_error(PNX_ERR_UNSUPPORTED, "grid refine: sigma is not built (per-b-value weights: the fine grid is evaluated on the "
                                              "unweighted signal)");
    if (o->t1_mode)
        return set_error(PNX_ERR_UNSUPPORTED, "grid refine: t1_mode=%d is not built (the T1 / STEAM factor: T1 would need a table of its own "
                                              "per voxel)", o->t1_mode);
    if (o->per_voxel_p0_bounds) return set_error(PNX_ERR_UNSUPPORTED, "grid refine: per_voxel_p0_bounds is not built (one set of bounds serves the call)");
    if (o->n_fixed && o->fixed_per_voxel) return set_error(PNX_ERR_UNSUPPORTED, "grid refine: fixed_per_voxel is not built");
    if (o->queue_order) return set_error(PNX_ERR_UNSUPPORTED, "grid refine: queue_order is not built (the kernel has no work queue)");
    if (!mean) return set_error(PNX_ERR_INVALID, "grid refine: mean is NULL (the one output that is not optional)");
    if (std::isnan(noise_sd) || std::isinf(noise_sd))
        return set_error(PNX_ERR_INVALID, "grid refine: noise_sd=%g must be finite: > 0 (known noise) or <= 0 (marginalised)", noise_sd);
    if (n_vox < 0) return set_error(PNX_ERR_INVALID, "n_vox < 0");
    if (!b || !lo || !hi || !n_points || (n_vox && (!y || !centre || !half_width))) return set_error(PNX_ERR_INVALID, "grid refine: NULL data pointer");
    if (o->n_fixed && !fixed) return set_error(PNX_ERR_INVALID, "fixed is NULL but n_fixed=%d", o->n_fixed);
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    H->s0_row = -1;
    if (project_amplitude) {
        const int pos = grid_s0_position(o->model);
        for (int k = 0; k < o->n_free && pos >= 0; ++k)
            if (o->free_idx[k] == pos) H->s0_row = k;
        if (H->s0_row < 0)
            return set_error(PNX_ERR_INVALID, "grid refine: project_amplitude needs a free linear amplitude S0 (PNX_MODEL_MONO, "
                                              "PNX_MODEL_BI_S0, PNX_MODEL_TRI_S0), model %d has none free", o->model);
    }
    int64_t atoms = 1;
    H->mmax = 1;
    for (int k = 0; k < o->n_free; ++k) {
        if (!(lo[k] <= hi[k]) || std::isinf(lo[k]) || std::isinf(hi[k]))
            return set_error(PNX_ERR_INVALID, "grid refine: bounds of free parameter %d, [%g, %g], must be finite with lo <= hi", k, lo[k], hi[k]);
        if (n_points[k] < 1 || n_points[k] > kRefineMaxPoints)
            return set_error(PNX_ERR_INVALID, "grid refine: n_points[%d]=%d out of range [1,%d]", k, (int)n_points[k], kRefineMaxPoints);
        if (k == H->s0_row && n_points[k] != 1)
            return set_error(PNX_ERR_INVALID, "grid refine: n_points[%d]=%d on the projected S0 row must be 1 (its value is fitted per atom, "
                                              "not gridded)", k, (int)n_points[k]);
        atoms *= n_points[k];
        H->mmax = n_points[k] > H->mmax ? n_points[k] : H->mmax;
    }
    if (atoms > kGridMaxAtoms)
        return set_error(PNX_ERR_INVALID, "grid refine: n_points spans %lld atoms per voxel, more than %d", (long long)atoms, kGridMaxAtoms);
    H->n_atoms = (int)atoms;
    return PNX_OK;
}

// The kernel's LDS: every wave owns one voxel at a time and keeps, for itself alone, the signal row [n_b], the axis values
// [PNX_MAX_PARAMS][9] and the table E[c][j][i] = exp(-b_i x_j) of the up to three rate rows, [3][mmax][pitch].  pitch = n_b | 1: the
// lanes of one read hold the same i and up to 9 different j, an odd pitch spreads those over the banks.  waves: as many as 64 KB
// hold, at most 4 (2 at 128 b-values and 9 points: 29.5 KB per wave).
struct GridRefineBlock {
    int waves, pitch, per_wave;  // per_wave in doubles
};
inline GridRefineBlock grid_refine_block(int n_b, int mmax) {
    GridRefineBlock r;
    r.pitch = n_b | 1;
    r.per_wave = n_b + PNX_MAX_PARAMS * kRefineMaxPoints + 3 * mmax * r.pitch;
    r.waves = 8192 / r.per_wave;
    r.waves = r.waves > 4 ? 4 : r.waves;  // >= 2: per_wave <= 3683
    return r;
}
}  // namespace pnx
