// pnx_args_common.hpp -- the argument checks the closed-form fits share (pnx_loglin_args.hpp, pnx_peel_args.hpp) and the by-value
// forms of b-values and masks their kernels receive.  Free of HIP types, like the headers that use it.  `who` is the entry point's
// name in front of a message ("loglinear", "peel"); a helper reads nothing but its own arguments, so the caller's order of
// checks decides what is read when.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/pnx.h"

namespace pnx {
// records a printf-style message for pnx_last_error() and returns `code` (pnx_api.hip; the stubs define their own)
int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

template <typename T> inline int args_check_b(const char *who, int n_b, const T *b) {
    for (int i = 0; i < n_b; ++i)
        if (!std::isfinite((double)b[i])) return set_error(PNX_ERR_INVALID, "%s: b[%d] is not finite", who, i);
    return PNX_OK;
}

inline int args_check_weighting(const char *who, int weighting) {
    if (weighting != 0 && weighting != 1) return set_error(PNX_ERR_INVALID, "%s: weighting=%d (0: none, 1: signal^2)", who, weighting);
    return PNX_OK;
}

// What one mask row (n_b bytes, or null: every b-value) keeps: a line needs kept >= 2 and two distinct b-values among them.
// The caller words the refusal; first is the first kept b-value, -1 when there is none.
struct MaskRow {
    int kept, first;
    bool distinct;
};
template <typename T> inline MaskRow args_mask_row(int n_b, const T *b, const uint8_t *row) {
    MaskRow m = {0, -1, false};
    for (int i = 0; i < n_b; ++i) {
        if (row && !row[i]) continue;
        if (m.first < 0) m.first = i;
        m.distinct = m.distinct || b[i] != b[m.first];
        ++m.kept;
    }
    return m;
}

// clip needs lo[j] < hi[j] for j < n; without clip the bounds are not looked at
template <typename T> inline int args_check_clip(const char *who, int clip, int n, const T *lo, const T *hi) {
    if (!clip) return PNX_OK;
    if (!lo || !hi) return set_error(PNX_ERR_INVALID, "%s: clip needs lo and hi, got NULL", who);
    for (int j = 0; j < n; ++j)
        if (!((double)lo[j] < (double)hi[j]))
            return set_error(PNX_ERR_INVALID, "%s: clip needs lo[%d] < hi[%d], got %g and %g", who, j, j, (double)lo[j], (double)hi[j]);
    return PNX_OK;
}

inline int args_check_mem(const char *who, int mem) {
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "%s: mem=%d", who, mem);
    return PNX_OK;
}

// bits[PNX_MAX_BVALUES / 64] <- one mask row: bit i is set where b-value i takes part
inline void args_pack_mask(int n_b, const uint8_t *row, unsigned long long *bits) {
    for (int q = 0; q < PNX_MAX_BVALUES / 64; ++q) bits[q] = 0;
    for (int i = 0; i < n_b; ++i)
        if (!row || row[i]) bits[i >> 6] |= 1ull << (i & 63);
}

// out[PNX_MAX_BVALUES] <- the n_b b-values as fp64, zeros behind them
template <typename T> inline void args_copy_b(int n_b, const T *b, double *out) {
    for (int i = 0; i < PNX_MAX_BVALUES; ++i) out[i] = i < n_b ? (double)b[i] : 0.0;
}
}  // namespace pnx
