// pnx_grid_mrf.hip -- the neighbourhood (MRF) prior of the grid posterior by coloured mean-field sweeps (DESIGN.md 4.1p;
// pnx_curvefit_grid_neighbour_field_f64, pnx_curvefit_grid_posterior_field_f64, pnx_curvefit_grid_posterior_mrf_f64).  A pairwise
// Gaussian prior between neighbouring voxels adds to a voxel's l_g, with its neighbours' posterior means held fixed,
//     sum_k thetac_kg q_vk - 0.5 n_v r_g,      thetac = atoms - centre,  q_vk = precision_k sum_u (mean[k, u] - centre_k),
// one more small product beside y . s_g and one more per-atom row beside ||s_g||^2.
//
//   grid_mrf_gather_kernel        one lane per voxel: q and n from the neighbour table, slots in order, every index bound-checked
//   grid_mrf_colour_check_kernel  one lane per voxel: no neighbour inside the voxel's own colour range, no index out of range
//   grid_mrf_posterior_kernel     (pnx_grid_mrf_kernel.hpp, shared with pnx_grid_tmrf.hip; instantiated here for the Gaussian prior)
//                                 grid_posterior_kernel (pnx_grid_posterior.hip) over a voxel range, copied expression for
//                                 expression: product, lane maps, slab, cost, projection, floor, fold and merge are the posterior's.
//                                 The field product runs on the matrix cores too, (NF + 3) / 4 k-steps into an accumulator of its
//                                 own (A = q of the strip, B = the centred rows the slab already carries), and enters l_g as one
//                                 addend, so a zero field adds exactly +0.0 and the call returns the posterior's bytes.
//   grid_mrf_delta_kernel         the maximum of the blocks' partial maxima of delta (no floating-point atomics)
//
// Lane maps of the MFMA as in pnx_grid.hip: A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom), row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "pnx_grid_mrf.hpp"
#include "pnx_grid_mrf_kernel.hpp"
#include "pnx_internal.hpp"

namespace pnx {

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- per-call inputs --------------------------------------------------------------------------------------------------------
size_t grid_mrf_bytes(int n_atoms, int cus) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15;
    return up256(gp * 8) + up256((size_t)(cus > 0 ? cus : 256) * 2 * 8) + up256(2 * sizeof(int32_t));
}

__global__ void grid_mrf_flags_kernel(int32_t *flags) {
    if (threadIdx.x < 2) flags[threadIdx.x] = INT_MAX;
}

int grid_mrf_prepare(const GridDict &D, const GridPosteriorHost &H, const GridMrfHost &M, const double *atoms_host, const double *precision,
                     int cus, void *buffer_d, GridMrf *F, hipStream_t st) {
    char *p = (char *)buffer_d;
    F->r = (double *)p;
    p += up256((size_t)D.gp * 8);
    F->blocks = (cus > 0 ? cus : 256) * 2;
    F->block = (double *)p;
    p += up256((size_t)F->blocks * 8);
    F->flags = (int32_t *)p;
    F->any = grid_mrf_any_precision(D.n_free, precision);
    grid_mrf_delta_scale(D.n_free, precision, M, F->scale);
    std::vector<double> r((size_t)D.gp);
    grid_mrf_r(D.n_free, D.n_atoms, D.gp, atoms_host, H.centre, precision, r.data());
    GM_HIP(hipMemcpyAsync(F->r, r.data(), (size_t)D.gp * 8, hipMemcpyHostToDevice, st));  // pageable: staged before the call returns, as the atoms
    hipLaunchKernelGGL(grid_mrf_flags_kernel, dim3(1), dim3(64), 0, st, F->flags);
    GM_HIP(hipGetLastError());
    return PNX_OK;
}

// ---- the gather -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) grid_mrf_gather_kernel(const GridMrfFieldArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.count) return;
    const long long v = a.first + i;
    const double inf = __builtin_huge_val();
    double s[PNX_MAX_PARAMS];
#pragma unroll
    for (int k = 0; k < PNX_MAX_PARAMS; ++k) s[k] = 0.0;
    int n = 0;
    bool bad = false;
    for (int slot = 0; slot < a.n_nb; ++slot) {
        const long long u = a.nb[(size_t)v * a.n_nb + slot];
        if (u < -1 || u >= a.n_vox) bad = true;  // reported, never dereferenced
        if (u < 0 || u >= a.n_vox) continue;
        if (!(fabs(a.mean[u]) < inf)) continue;  // a non-finite voxel counts for nobody
        ++n;
#pragma unroll
        for (int k = 0; k < PNX_MAX_PARAMS; ++k)
            if (k < a.n_free) s[k] += a.mean[(size_t)k * a.n_vox + u] - a.centre[k];
    }
#pragma unroll
    for (int k = 0; k < PNX_MAX_PARAMS; ++k)
        if (k < a.n_free) a.q[(size_t)k * a.n_vox + v] = a.precision[k] * s[k];
    a.n[v] = n;
    if (bad && a.flag) atomicMin(a.flag, (int)v);
}

int grid_mrf_field_device(const GridMrfFieldArgs &a, hipStream_t st) {
    if (a.count <= 0) return PNX_OK;
    hipLaunchKernelGGL(grid_mrf_gather_kernel, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, st, a);
    GM_HIP(hipGetLastError());
    return PNX_OK;
}

// ---- the colouring ----------------------------------------------------------------------------------------------------------
struct ColourArgs {
    const int32_t *nb;
    int32_t *flags;
    long long n_vox;
    int n_nb, n_colours;
    long long start[kGridMrfMaxColours + 1];
};

__global__ void __launch_bounds__(256) grid_mrf_colour_check_kernel(const ColourArgs a) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= a.n_vox) return;
    long long lo = 0, hi = 0;
    for (int c = 0; c < a.n_colours; ++c)
        if (v >= a.start[c] && v < a.start[c + 1]) {
            lo = a.start[c];
            hi = a.start[c + 1];
        }
    bool range = false, own = false;
    for (int slot = 0; slot < a.n_nb; ++slot) {
        const long long u = a.nb[(size_t)v * a.n_nb + slot];
        range |= u < -1 || u >= a.n_vox;
        own |= u >= lo && u < hi && u >= 0;
    }
    if (range) atomicMin(a.flags, (int)v);
    if (own) atomicMin(a.flags + 1, (int)v);
}

int grid_mrf_colour_check_device(int64_t n_vox, int n_nb, const int32_t *nb_d, int n_colours, const int64_t *colour_start, int32_t *flags_d,
                                 hipStream_t st) {
    if (n_vox <= 0) return PNX_OK;
    ColourArgs a;
    memset(&a, 0, sizeof(a));
    a.nb = nb_d;
    a.flags = flags_d;
    a.n_vox = n_vox;
    a.n_nb = n_nb;
    a.n_colours = n_colours;
    for (int c = 0; c <= n_colours; ++c) a.start[c] = colour_start[c];
    hipLaunchKernelGGL(grid_mrf_colour_check_kernel, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, st, a);
    GM_HIP(hipGetLastError());
    return PNX_OK;
}

__global__ void __launch_bounds__(256) grid_mrf_delta_kernel(const double *block, int n, double *out, int accumulate) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double mx = 0.0;  // delta is never negative
    for (int i = tid; i < n; i += 256) mx = fmax(mx, block[i]);
    red[tid] = mx;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) *out = accumulate ? fmax(*out, red[0]) : red[0];
}

int grid_mrf_delta_device(const double *block_d, int blocks, double *delta_d, bool accumulate, hipStream_t stream) {
    hipLaunchKernelGGL(grid_mrf_delta_kernel, dim3(1), dim3(256), 0, stream, block_d, blocks, delta_d, accumulate ? 1 : 0);
    GM_HIP(hipGetLastError());
    return PNX_OK;
}

int grid_mrf_posterior_device(const GridDict &D, const GridPosterior &P, const GridMrf &F, int64_t n_vox, int64_t first, int64_t count,
                              const double *y_d, const double *field_q_d, const int32_t *field_n_d, double *mean_d, double *sd_d,
                              int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, double *delta_d, bool accumulate,
                              int cus, hipStream_t stream) {
    return grid_mrf_posterior_run<false>(D, P, F, n_vox, first, count, y_d, field_q_d, field_n_d, nullptr, mean_d, sd_d, map_atom_d, map_p_d,
                                         log_evidence_d, ess_d, delta_d, accumulate, cus, stream);
}

}  // namespace pnx
