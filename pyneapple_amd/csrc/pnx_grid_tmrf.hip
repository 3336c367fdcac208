// pnx_grid_tmrf.hip -- the edge-preserving (Student-t) neighbourhood prior of the grid posterior (DESIGN.md 4.1s;
// pnx_curvefit_grid_neighbour_wfield_f64, pnx_curvefit_grid_posterior_wfield_f64, pnx_curvefit_grid_posterior_tmrf_f64).  The
// Gaussian pair potential of pnx_grid_mrf.hip written as a scale mixture with one latent precision tau_uv per edge; mean field over
// it keeps the voxel update and gives every neighbour a weight w_uv = E[tau_uv] = (nu + K) / (nu + s_uv):
//     sum_k thetac_kg q_vk - 0.5 W_v r_g,      q_vk = precision_k sum_u w_uv (mean[k, u] - centre_k),   W_v = sum_u w_uv.
//
//   grid_tmrf_gather_kernel    one lane per voxel: the weights on the fly from the means and sds at both ends of every edge, q, W, n
//                              and optionally the weights themselves; slots in order, every index bound-checked; nothing is stored
//                              between colour updates, so an edge's weight is always the one of the current moments
//   grid_mrf_posterior_kernel  (pnx_grid_mrf_kernel.hpp) instantiated with WREAL = true: W_v / 2 in doubles where the Gaussian
//                              prior holds n_v / 2 in floats
#include <hip/hip_runtime.h>

#include "pnx_grid_mrf_kernel.hpp"
#include "pnx_grid_tmrf.hpp"

namespace pnx {

// The order of operations (include/pnx.h states it for a restatement): per edge s over the rows with a precision, k ascending, each
// term fma(d, d, fma(sd_u, sd_u, sd_v * sd_v)) entering by fma(precision_k, term, s); w = (nu + K) / (nu + s); then per row
// acc_k = fma(w, mean[k, u] - centre_k, acc_k) and W += w in slot order; q_k = precision_k * acc_k.
__global__ void __launch_bounds__(256) grid_tmrf_gather_kernel(const GridTmrfFieldArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.count) return;
    const long long v = a.first + i;  // < n_vox: the range lies inside the voxels (grid_mrf_check_range)
    const double inf = __builtin_huge_val();
    const bool own = fabs(a.mean[v]) < inf;  // a voxel whose own mean is non-finite: q = 0, W = 0, n = 0
    double mv[PNX_MAX_PARAMS], vv[PNX_MAX_PARAMS], acc[PNX_MAX_PARAMS];
#pragma unroll
    for (int k = 0; k < PNX_MAX_PARAMS; ++k) {
        acc[k] = mv[k] = vv[k] = 0.0;
        if (own && k < a.n_free && a.precision[k] > 0.0) {
            const double sdv = a.sd[(size_t)k * a.n_vox + v];
            mv[k] = a.mean[(size_t)k * a.n_vox + v];
            vv[k] = sdv * sdv;
        }
    }
    double wsum = 0.0;
    int n = 0;
    bool bad = false;
    for (int slot = 0; slot < a.n_nb; ++slot) {
        const long long u = a.nb[(size_t)v * a.n_nb + slot];
        if (u < -1 || u >= a.n_vox) bad = true;  // reported, never dereferenced
        double w = 0.0;
        if (own && u >= 0 && u < a.n_vox && fabs(a.mean[u]) < inf) {  // a non-finite voxel counts for nobody
            double mu[PNX_MAX_PARAMS];
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < PNX_MAX_PARAMS; ++k) {
                mu[k] = k < a.n_free ? a.mean[(size_t)k * a.n_vox + u] : 0.0;
                if (k < a.n_free && a.precision[k] > 0.0) {
                    const double sdu = a.sd[(size_t)k * a.n_vox + u];
                    const double d = mv[k] - mu[k];
                    s = fma(a.precision[k], fma(d, d, fma(sdu, sdu, vv[k])), s);
                }
            }
            w = a.dof_k / (a.dof + s);
            ++n;
            wsum += w;
#pragma unroll
            for (int k = 0; k < PNX_MAX_PARAMS; ++k)
                if (k < a.n_free) acc[k] = fma(w, mu[k] - a.centre[k], acc[k]);
        }
        if (a.edge) a.edge[(size_t)v * a.n_nb + slot] = w;
    }
#pragma unroll
    for (int k = 0; k < PNX_MAX_PARAMS; ++k)
        if (k < a.n_free) a.q[(size_t)k * a.n_vox + v] = a.precision[k] * acc[k];
    a.w[v] = wsum;
    a.n[v] = n;
    if (bad && a.flag) atomicMin(a.flag, (int)v);
}

int grid_tmrf_field_device(const GridTmrfFieldArgs &a, hipStream_t st) {
    if (a.count <= 0) return PNX_OK;
    hipLaunchKernelGGL(grid_tmrf_gather_kernel, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, st, a);
    GM_HIP(hipGetLastError());
    return PNX_OK;
}

int grid_tmrf_posterior_device(const GridDict &D, const GridPosterior &P, const GridMrf &F, int64_t n_vox, int64_t first, int64_t count,
                               const double *y_d, const double *field_q_d, const double *field_w_d, double *mean_d, double *sd_d,
                               int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, double *delta_d, bool accumulate,
                               int cus, hipStream_t stream) {
    return grid_mrf_posterior_run<true>(D, P, F, n_vox, first, count, y_d, field_q_d, nullptr, field_w_d, mean_d, sd_d, map_atom_d, map_p_d,
                                        log_evidence_d, ess_d, delta_d, accumulate, cus, stream);
}

}  // namespace pnx
