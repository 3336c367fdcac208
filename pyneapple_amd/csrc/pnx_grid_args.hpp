// pnx_grid_args.hpp -- the host half of pnx_curvefit_grid_start_f64 that needs no device: the argument checks in front of any
// device work and the sizing of the match kernel's LDS slab.  Free of HIP types, like pnx_host_pipeline.hpp: pnx_api.hip and
// pnx_grid.hip use it, tests/host_stub/grid_args_stub.cpp builds the same code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cstdint>

#include "../../include/pnx.h"

namespace pnx {
// records a printf-style message for pnx_last_error() and returns `code` (pnx_api.hip; the stub defines its own)
int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

constexpr int kGridMaxAtoms = 4096;

// position of the linear amplitude S0 among the model's parameters, -1 for the layouts without one
inline int grid_s0_position(int model) {
    switch (model) {
    case PNX_MODEL_MONO: return 0;
    case PNX_MODEL_BI_S0: return 3;
    case PNX_MODEL_TRI_S0: return 5;
    }
    return -1;
}

// What the entry point checks behind check_curvefit_opts (o is consistent: model, n_b, index lists), in front of any device
// work.  *s0_row: the row of S0 among the free parameters when the amplitude is projected, -1 otherwise.
inline int grid_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms, const double *atoms,
                           const double *fixed, const double *lo, const double *hi, int project_amplitude, const double *p0_out, int mem,
                           int *s0_row) {
    *s0_row = -1;
    if (o->per_voxel_p0_bounds) return set_error(PNX_ERR_UNSUPPORTED, "grid start: per_voxel_p0_bounds is not built (one dictionary and one set of bounds serve the call)");
    if (o->n_fixed && o->fixed_per_voxel) return set_error(PNX_ERR_UNSUPPORTED, "grid start: fixed_per_voxel is not built (the dictionary would differ from voxel to voxel)");
    if (o->queue_order) return set_error(PNX_ERR_UNSUPPORTED, "grid start: queue_order is not built (the search has no work queue)");
    if (n_atoms < 1 || n_atoms > kGridMaxAtoms) return set_error(PNX_ERR_INVALID, "grid start: n_atoms=%d out of range [1,%d]", n_atoms, kGridMaxAtoms);
    if (n_vox < 0) return set_error(PNX_ERR_INVALID, "n_vox < 0");
    if (!b || !atoms || !lo || !hi || !p0_out || (n_vox && !y)) return set_error(PNX_ERR_INVALID, "NULL data pointer");
    if (o->n_fixed && !fixed) return set_error(PNX_ERR_INVALID, "fixed is NULL but n_fixed=%d", o->n_fixed);
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    if (project_amplitude) {
        const int pos = grid_s0_position(o->model);
        for (int k = 0; k < o->n_free && pos >= 0; ++k)
            if (o->free_idx[k] == pos) *s0_row = k;
        if (*s0_row < 0)
            return set_error(PNX_ERR_INVALID, "grid start: project_amplitude needs a free linear amplitude S0 (PNX_MODEL_MONO, "
                                              "PNX_MODEL_BI_S0, PNX_MODEL_TRI_S0), model %d has none free", o->model);
    }
    // an atom is a start value: the fit refuses one outside its bounds (status -3), so it is refused here, by name.  The S0 row of
    // a projected call is checked too: it is what a voxel with a non-finite signal receives.
    for (int k = 0; k < o->n_free; ++k)
        for (int g = 0; g < n_atoms; ++g) {
            const double a = atoms[(size_t)k * n_atoms + g];
            if (!(a >= lo[k] && a <= hi[k]))
                return set_error(PNX_ERR_INVALID, "grid start: atom %d, free parameter %d = %g lies outside its bounds [%g, %g]", g, k, a, lo[k], hi[k]);
        }
    return PNX_OK;
}

// The match kernel's LDS image of a slab of the dictionary: [kpad][stride] doubles, then ||s||^2 and its inverse per atom.
// width: atoms per slab, a multiple of 16, as many as 64 KB hold (at most 256); stride = width or width + 16, whichever is
// 16 mod 32: the fragment reads of lanes 0-15 (row 4 s) and 16-31 (row 4 s + 1) then fall into opposite halves of the 64 banks.
struct GridSlab {
    int kpad, width, stride, lds_doubles;
};
inline GridSlab grid_slab(int n_b) {
    GridSlab s;
    s.kpad = (n_b + 3) & ~3;
    s.width = 16;
    for (int w = 16; w <= 256; w += 16) {
        const int stride = (w & 16) ? w : w + 16;
        if (s.kpad * stride + 2 * w <= 8192) s.width = w;
    }
    s.stride = (s.width & 16) ? s.width : s.width + 16;
    s.lds_doubles = s.kpad * s.stride + 2 * s.width;
    return s;
}
}  // namespace pnx
