// pnx_varpro_args.hpp -- the host half of pnx_curvefit_varpro_f64 that needs no device: which parameters of a layout are linear,
// the argument checks in front of any device work and the sizing of the match kernel's LDS slab.  Free of HIP types, like
// pnx_grid_args.hpp: pnx_api.hip and pnx_varpro.hip use it, tests/host_stub/varpro_args_stub.cpp builds the same code for the
// CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_args.hpp"

namespace pnx {

// How the amplitudes of a layout are constrained: free (mono, bi / tri full), sum-to-one (bi / tri reduced),
// sum-to-S0 (bi / tri S0).
enum VarproClass { kVarproFree = 0, kVarproReduced = 1, kVarproS0 = 2 };

// What the host derives from the arguments once per call.
struct VarproLayout {
    int k = 0;        // compartments: columns per atom
    int cls = 0;      // VarproClass
    int n_lin = 0;    // linear parameters of the layout, all free: k (free, S0) or k - 1 (reduced)
    int n_nl = 0;     // free non-linear parameters: rows of nl_atoms
    int lin_pos[3] = {-1, -1, -1};   // model positions of the linear parameters; slot k - 1 of the S0 class is S0
    int rate_pos[3] = {-1, -1, -1};  // model positions of the k rates
    int lin_row[3] = {-1, -1, -1};   // their rows among the free parameters
    int row_src[PNX_MAX_PARAMS] = {};  // per free row: >= 0 the row of nl_atoms, < 0 the linear slot -(1 + j)
    double lin_lo[3] = {0, 0, 0}, lin_hi[3] = {0, 0, 0};
};

inline int varpro_layout(int model, VarproLayout *L) {
    *L = VarproLayout();
    auto set = [&](int k, int cls, int l0, int l1, int l2, int r0, int r1, int r2) {
        L->k = k;
        L->cls = cls;
        L->n_lin = cls == kVarproReduced ? k - 1 : k;
        const int l[3] = {l0, l1, l2}, r[3] = {r0, r1, r2};
        for (int j = 0; j < 3; ++j) {
            L->lin_pos[j] = l[j];
            L->rate_pos[j] = r[j];
        }
    };
    switch (model) {
    case PNX_MODEL_MONO: set(1, kVarproFree, 0, -1, -1, 1, -1, -1); return PNX_OK;
    case PNX_MODEL_BI_REDUCED: set(2, kVarproReduced, 0, -1, -1, 1, 2, -1); return PNX_OK;
    case PNX_MODEL_BI_S0: set(2, kVarproS0, 0, 3, -1, 1, 2, -1); return PNX_OK;
    case PNX_MODEL_BI_FULL: set(2, kVarproFree, 0, 2, -1, 1, 3, -1); return PNX_OK;
    case PNX_MODEL_TRI_REDUCED: set(3, kVarproReduced, 0, 2, -1, 1, 3, 4); return PNX_OK;
    case PNX_MODEL_TRI_S0: set(3, kVarproS0, 0, 2, 5, 1, 3, 4); return PNX_OK;
    case PNX_MODEL_TRI_FULL: set(3, kVarproFree, 0, 2, 4, 1, 3, 5); return PNX_OK;
    }
    return set_error(PNX_ERR_INVALID, "varpro: unknown model %d", model);
}

// What the entry point checks behind check_curvefit_opts (o is consistent: model, n_b, index lists), in front of any device work.
// nl_atoms (n_nl, n_atoms): the free non-linear parameters of every atom in the order of free_idx; fixed (n_fixed,) shared.
inline int varpro_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms, const double *nl_atoms,
                             const double *fixed, const double *lo, const double *hi, const double *fallback, const double *p_out, int mem,
                             VarproLayout *L) {
    if (o->per_voxel_p0_bounds) return set_error(PNX_ERR_UNSUPPORTED, "varpro: per_voxel_p0_bounds is not built (one dictionary and one set of bounds serve the call)");
    if (o->n_fixed && o->fixed_per_voxel) return set_error(PNX_ERR_UNSUPPORTED, "varpro: fixed_per_voxel is not built (the dictionary would differ from voxel to voxel)");
    if (o->queue_order) return set_error(PNX_ERR_UNSUPPORTED, "varpro: queue_order is not built (the search has no work queue)");
    if (int rc = varpro_layout(o->model, L)) return rc;
    if (n_atoms < 1 || n_atoms > kGridMaxAtoms) return set_error(PNX_ERR_INVALID, "varpro: n_atoms=%d out of range [1,%d]", n_atoms, kGridMaxAtoms);
    if (n_vox < 0) return set_error(PNX_ERR_INVALID, "n_vox < 0");
    if (o->n_b <= L->k) return set_error(PNX_ERR_INVALID, "varpro: n_b=%d must exceed the %d amplitudes of an atom", o->n_b, L->k);
    if (!b || !nl_atoms || !lo || !hi || !fallback || !p_out || (n_vox && !y)) return set_error(PNX_ERR_INVALID, "NULL data pointer");
    if (o->n_fixed && !fixed) return set_error(PNX_ERR_INVALID, "fixed is NULL but n_fixed=%d", o->n_fixed);
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    // every linear parameter is free: with a fixed fraction or a fixed S0 the columns of an atom are no longer the one-hot ones
    for (int k = 0; k < o->n_fixed; ++k)
        for (int j = 0; j < L->n_lin; ++j)
            if (o->fixed_idx[k] == L->lin_pos[j])
                return set_error(PNX_ERR_UNSUPPORTED, "varpro: parameter %d (a fraction or S0) is fixed: the linear structure changes, "
                                                      "fix rates or T1 only", L->lin_pos[j]);
    int nl = 0;
    for (int r = 0; r < o->n_free; ++r) {
        int slot = -1;
        for (int j = 0; j < L->n_lin; ++j)
            if (o->free_idx[r] == L->lin_pos[j]) slot = j;
        if (slot >= 0) {
            L->lin_row[slot] = r;
            L->lin_lo[slot] = lo[r];
            L->lin_hi[slot] = hi[r];
            L->row_src[r] = -(1 + slot);
            if (!(lo[r] <= hi[r])) return set_error(PNX_ERR_INVALID, "varpro: free parameter %d has lo=%g > hi=%g", r, lo[r], hi[r]);
        } else {
            L->row_src[r] = nl++;
        }
    }
    L->n_nl = nl;
    if (L->cls == kVarproS0 || o->model == PNX_MODEL_MONO) {
        const double lo_s0 = L->lin_lo[L->k - 1];
        if (!(lo_s0 >= 0.0)) return set_error(PNX_ERR_INVALID, "varpro: lo_S0=%g < 0 is refused (the fraction bounds scale with S0)", lo_s0);
    }
    for (int r = 0; r < o->n_free; ++r)
        if (!(fallback[r] >= lo[r] && fallback[r] <= hi[r]))
            return set_error(PNX_ERR_INVALID, "varpro: fallback[%d] = %g lies outside its bounds [%g, %g]", r, fallback[r], lo[r], hi[r]);
    // the atoms: inside their bounds, and no two rates of an atom equal (fixed ones included): M would be singular
    for (int g = 0; g < n_atoms; ++g) {
        double rate[3] = {0, 0, 0};
        for (int r = 0; r < o->n_free; ++r) {
            if (L->row_src[r] < 0) continue;
            const double a = nl_atoms[(size_t)L->row_src[r] * n_atoms + g];
            if (!(a >= lo[r] && a <= hi[r]))
                return set_error(PNX_ERR_INVALID, "varpro: atom %d, free parameter %d = %g lies outside its bounds [%g, %g]", g, r, a, lo[r], hi[r]);
            for (int j = 0; j < L->k; ++j)
                if (o->free_idx[r] == L->rate_pos[j]) rate[j] = a;
        }
        for (int f = 0; f < o->n_fixed; ++f)
            for (int j = 0; j < L->k; ++j)
                if (o->fixed_idx[f] == L->rate_pos[j]) rate[j] = fixed[f];
        for (int i = 0; i < L->k; ++i)
            for (int j = 0; j < i; ++j)
                if (rate[i] == rate[j])
                    return set_error(PNX_ERR_INVALID, "varpro: atom %d has two equal rates D%d = D%d = %g (its columns are linearly dependent)", g,
                                     j + 1, i + 1, rate[i]);
    }
    return PNX_OK;
}

// rows of per-atom constants behind the dictionary rows of a slab: M packed (k (k + 1) / 2) and as many for the solve -- the
// packed inverse of M, or (reduced) the packed inverse of the difference system and its k - 1 offsets
inline int varpro_const_rows(int k) { return k * (k + 1); }

// The match kernel's LDS image of a slab: k blocks of [kpad][stride] doubles (one per compartment), then varpro_const_rows(k)
// rows of `width` constants.  width and stride follow grid_slab's rule (stride = 16 mod 32); at 128 b-values and three
// compartments sixteen atoms still fit.
inline GridSlab varpro_slab(int n_b, int k) {
    GridSlab s;
    s.kpad = (n_b + 3) & ~3;
    s.width = 16;
    for (int w = 16; w <= 256; w += 16) {
        const int stride = (w & 16) ? w : w + 16;
        if (k * s.kpad * stride + varpro_const_rows(k) * w <= 8192) s.width = w;
    }
    s.stride = (s.width & 16) ? s.width : s.width + 16;
    s.lds_doubles = k * s.kpad * s.stride + varpro_const_rows(k) * s.width;
    return s;
}
}  // namespace pnx
