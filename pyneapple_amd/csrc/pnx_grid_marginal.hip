// pnx_grid_marginal.hip -- the marginal posterior of every free parameter of every voxel over a dictionary, and quantiles from it
// (pnx_curvefit_grid_marginals_f64).  P_k[v, j] = sum_g W_vg [atom g sits on the j-th grid value of parameter k]:
// the normalised weights of the posterior times a 0/1 indicator matrix, a second product on v_mfma_f64_16x16x4 behind the first.
// Two passes over the product y_v . s_g:
//
//   grid_prior_norm_kernel   the EM's normaliser pass (pnx_grid_prior.hip: grid_prior_normalise), reused: L_v to a work buffer
//   grid_marginal_kernel     voxel-stationary, one strip of 16 voxels per wave, the dictionary through LDS in the EM's slabs.  The
//                            first product is formed TRANSPOSED (dictionary fragment as A, signal fragment as B), so that register
//                            `reg` of the 16 x 16 tile holds atom (l >> 4) + 4 reg, voxel l & 15 -- which is the B operand of k-step
//                            `reg` of  marginal^T[bin, voxel] += Ind[bin, atom] W[atom, voxel]  as it stands: no shuffle, no LDS
//                            transpose.  The A operand of that k-step is 1.0 where one of the atom's global bin indices (a per-slab
//                            LDS table, one int per parameter and atom) is the lane's bin 16 c + (l & 15), else 0.0.  One f64x4 of
//                            accumulators per 16-bin chunk c, NC of them (template), written bin-major at the end: 16 consecutive
//                            voxels per bin row.
//   grid_marginal_quantile_kernel   one lane per voxel and free parameter: the running sum of its bins, the first bin at or above
//                            every level; lane k = 0 of a voxel also writes log_evidence = L_v - log sum exp(log_prior)
//
// No atomics; a voxel's sums depend on the order of the atoms only (header).  Lane maps of the MFMA: A[l & 15][l >> 4],
// B[l >> 4][l & 15], D: col = l & 15, row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "pnx_grid_marginal.hpp"
#include "pnx_launch.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kMargWaves = 4;  // a block: one wave per SIMD, as both EM passes

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

size_t grid_marginal_bytes(int n_free, int n_atoms) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15;
    return up256((size_t)n_free * gp * sizeof(int32_t));
}

int grid_marginal_prepare(const GridDict &D, const GridMarginalHost &M, const int32_t *bin_of_host, void *buffer_d, GridMarginal *G,
                          hipStream_t st) {
    std::vector<int32_t> table((size_t)M.n_rows * D.gp);
    grid_marginal_table(D.n_free, D.n_atoms, D.gp, M, bin_of_host, table.data());
    // the copy from pageable memory is staged before the call returns (as the atoms of the dictionary)
    PNX_HIP(hipMemcpyAsync(buffer_d, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    G->table = (const int32_t *)buffer_d;
    G->host = M;
    return PNX_OK;
}

struct MargArgs {
    const double *y;          // (n_vox, n_b)
    const double *st;         // (kpad, gp)
    const double *nrm, *inv;  // (gp)
    const double *lp;         // (gp)
    const double *wd;         // (kpad)
    const double *max_nrm;
    const double *lv;         // (n_vox) L_v of the normaliser pass, NaN for a non-finite voxel
    const int32_t *table;     // (n_rows, gp)
    double *out;              // (n_bins, n_vox)
    long long n_vox;
    int n_b, kpad, gp, width, stride, marginal, n_rows, n_bins;
    double lo_s0, hi_s0;
    double tol_scale;  // 4 n_b 2^-52
    double gain;       // known noise: 1 / noise_sd^2;  marginalised: nu / 2
};

// LDS: [kpad][stride] | nrm | inv | log_prior, each `W` doubles wide, then the table [n_rows][W] int32.
template <int NS, bool PROJ, int NC> __global__ void __launch_bounds__(kMargWaves * 64) grid_marginal_kernel(const MargArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lnrm = lds + kpad * stride, *linv = lnrm + W, *llp = linv + W;
    int32_t *ltab = reinterpret_cast<int32_t *>(llp + W);
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kMargWaves - 1) / kMargWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double max_nrm = *a.max_nrm;
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        // B fragment of this wave's strip, the posterior's loads: weighted, rows past the end repeat the last voxel (never stored).
        // In the transposed product a lane's accumulator column is voxel v0 + r16: ||y||^2, the floor and L_v are per-lane values.
        const long long v0 = (grp * kMargWaves + wave) * 16, v = v0 + r16;
        double yf[NS], yy;
        {
            const double *row = a.y + (size_t)(v < a.n_vox ? v : a.n_vox - 1) * a.n_b;
            double ss = 0.0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int k = 4 * s + kq;
                const double val = (s < ksteps && k < a.n_b) ? row[k] * a.wd[k] : 0.0;
                ss = fma(val, val, ss);
                yf[s] = val;
            }
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            yy = ss;
        }
        const double tol = a.tol_scale * (yy + max_nrm);
        const double lv = v < a.n_vox ? a.lv[v] : __builtin_nan("");
        const bool ok = fabs(lv) < inf;  // a voxel past the end or with a non-finite signal (L_v = NaN) weighs nothing
        f64x4 m[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) m[c] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                for (int k = wave; k < kpad; k += kMargWaves)
                    for (int j = lane; j < wc; j += 64) lds[k * stride + j] = a.st[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < a.n_rows; k += kMargWaves)
                    for (int j = lane; j < wc; j += 64) ltab[k * W + j] = a.table[(size_t)k * a.gp + g0 + j];
                for (int j = threadIdx.x; j < wc; j += kMargWaves * 64) {
                    lnrm[j] = a.nrm[g0 + j];
                    linv[j] = a.inv[g0 + j];
                    llp[j] = a.lp[g0 + j];
                }
                __syncthreads();
                resident = n_slabs == 1;
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
                const double *ap = lds + kq * stride + t * 16 + r16;  // A fragment: S[g0 + 16 t + r16][4 s + kq]
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (s < ksteps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * s * stride], yf[s], acc, 0, 0, 0);
                }
                // register r: atom j = 16 t + 4 r + kq of the slab against voxel r16 -- l_g with the posterior's expressions term
                // for term, then the normalised weight.  A padded or excluded atom (log_prior = -inf) weighs exactly 0.
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = t * 16 + 4 * r + kq;
                    const double lpg = llp[j];
                    const double nr = lnrm[j];
                    const double dot = acc[r];
                    double c;  // cost - 0.5 ||y||^2, grid start's
                    if constexpr (PROJ) {
                        const double amp = fmin(fmax(dot * linv[j], a.lo_s0), a.hi_s0);
                        c = amp * fma(0.5 * amp, nr, -dot);
                    } else {
                        c = fma(0.5, nr, -dot);
                    }
                    const double cost = fma(0.5, yy, c);
                    const double ell = a.marginal ? fma(-a.gain, log(fmax(cost, tol)), lpg) : fma(-cost, a.gain, lpg);
                    const double w = (ok && lpg > -inf) ? exp(ell - lv) : 0.0;
                    // k-step r of the second product: B[k = kq][n = r16] = w as it stands; A[bin r16 of chunk c][k = kq] is the
                    // indicator of the same atom j.  The bins of different parameters are disjoint: at most one row matches.
                    double ind[NC];
#pragma unroll
                    for (int c2 = 0; c2 < NC; ++c2) ind[c2] = 0.0;
                    for (int p = 0; p < a.n_rows; ++p) {
                        const int d = ltab[p * W + j] - r16;  // 16 c exactly when the atom sits in this lane's bin of chunk c
#pragma unroll
                        for (int c2 = 0; c2 < NC; ++c2) ind[c2] = d == 16 * c2 ? 1.0 : ind[c2];
                    }
#pragma unroll
                    for (int c2 = 0; c2 < NC; ++c2) m[c2] = __builtin_amdgcn_mfma_f64_16x16x4f64(ind[c2], w, m[c2], 0, 0, 0);
                }
            }
        }
        // D of the second product: row = bin 16 c + kq + 4 r, column = voxel r16: 16 consecutive voxels per bin row
        if (v < a.n_vox) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int bin = 16 * c + kq + 4 * r;
                    if (bin < a.n_bins) a.out[(size_t)bin * a.n_vox + v] = ok ? m[c][r] : __builtin_nan("");
                }
        }
    }
}

struct QuantArgs {
    const double *marginal;  // (n_bins, n_vox)
    const double *lv;        // (n_vox)
    double *quantile;        // (n_q, n_free, n_vox) or null
    double *logev;           // (n_vox) or null
    long long n_vox;
    int n_free, n_q;
    double lp_norm;
    int n_bins[PNX_MAX_PARAMS], off[PNX_MAX_PARAMS];
    double probs[kGridMarginalMaxProbs];
    double bin_value[kGridMarginalMaxBins];
};

__global__ void __launch_bounds__(256) grid_marginal_quantile_kernel(const QuantArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n_vox * a.n_free) return;
    const int k = (int)(idx / a.n_vox);
    const long long v = idx - (long long)k * a.n_vox;
    const double qnan = __builtin_nan("");
    const double L = a.lv[v];
    const bool bad = !(fabs(L) < __builtin_huge_val());
    if (k == 0 && a.logev) a.logev[v] = bad ? qnan : L - a.lp_norm;
    if (!a.quantile) return;
    const int nb = a.n_bins[k], off = a.off[k];
    double q[kGridMarginalMaxProbs];
#pragma unroll
    for (int i = 0; i < kGridMarginalMaxProbs; ++i) q[i] = (bad || nb == 0) ? qnan : a.bin_value[off + nb - 1];
    if (!bad && nb) {
        unsigned found = 0;
        double cdf = 0.0;
        for (int j = 0; j < nb; ++j) {  // the running sum in bin order; the first bin at or above a level keeps it
            cdf += a.marginal[(size_t)(off + j) * a.n_vox + v];
            const double val = a.bin_value[off + j];
#pragma unroll
            for (int i = 0; i < kGridMarginalMaxProbs; ++i) {
                const bool hit = i < a.n_q && !(found >> i & 1) && cdf >= a.probs[i];
                q[i] = hit ? val : q[i];
                found |= hit ? 1u << i : 0u;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kGridMarginalMaxProbs; ++i)
        if (i < a.n_q) a.quantile[((size_t)i * a.n_free + k) * a.n_vox + v] = q[i];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
template <int NS, bool PROJ> static void launch_marg(const MargArgs &a, int chunks, unsigned blocks, size_t lds, hipStream_t st) {
    if (chunks == 2)
        hipLaunchKernelGGL((grid_marginal_kernel<NS, PROJ, 2>), dim3(blocks), dim3(kMargWaves * 64), lds, st, a);
    else if (chunks == 4)
        hipLaunchKernelGGL((grid_marginal_kernel<NS, PROJ, 4>), dim3(blocks), dim3(kMargWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((grid_marginal_kernel<NS, PROJ, 8>), dim3(blocks), dim3(kMargWaves * 64), lds, st, a);
}

int grid_marginal_device(const GridDict &D, const GridPosterior &P, const GridMarginal &G, int64_t n_vox, const double *y_d,
                         const GridPriorWork &W, const double *bin_value, int n_q, const double *probs, double *marginal_d, double *quantile_d,
                         double *log_evidence_d, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const GridSlab S = grid_marginal_slab(D.n_b);
    const GridMarginalHost &M = G.host;
    MargArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.nrm = D.nrm;
    a.inv = D.inv;
    a.lp = P.lp;
    a.wd = D.w;
    a.max_nrm = P.max_nrm;
    a.lv = W.lv;
    a.table = G.table;
    a.out = marginal_d;
    a.n_vox = n_vox;
    a.n_b = D.n_b;
    a.kpad = S.kpad;
    a.gp = D.gp;
    a.width = S.width < D.gp ? S.width : D.gp;
    a.stride = S.stride;
    a.marginal = P.noise_sd == 0.0;
    a.n_rows = M.n_rows;
    a.n_bins = M.n_bins_total;
    a.lo_s0 = D.lo_s0;
    a.hi_s0 = D.hi_s0;
    a.tol_scale = 4.0 * D.n_b * 0x1p-52;
    a.gain = a.marginal ? 0.5 * (D.n_b - (D.s0_row >= 0 ? 1 : 0)) : 1.0 / (P.noise_sd * P.noise_sd);
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    const int chunks = grid_marginal_chunks(M.n_bins_total);
    const unsigned blocks = (unsigned)W.blocks;  // the normaliser pass's grid; no sum depends on it
    const bool proj = D.s0_row >= 0;
    if (S.kpad <= 32) {
        if (proj)
            launch_marg<8, true>(a, chunks, blocks, lds, stream);
        else
            launch_marg<8, false>(a, chunks, blocks, lds, stream);
    } else {
        if (proj)
            launch_marg<32, true>(a, chunks, blocks, lds, stream);
        else
            launch_marg<32, false>(a, chunks, blocks, lds, stream);
    }
    PNX_HIP(hipGetLastError());
    if (!quantile_d && !log_evidence_d) return PNX_OK;
    QuantArgs q;
    memset(&q, 0, sizeof(q));
    q.marginal = marginal_d;
    q.lv = W.lv;
    q.quantile = n_q ? quantile_d : nullptr;
    q.logev = log_evidence_d;
    q.n_vox = n_vox;
    q.n_free = D.n_free;
    q.n_q = n_q;
    q.lp_norm = P.log_prior_norm;
    for (int k = 0; k < D.n_free; ++k) {
        q.n_bins[k] = M.n_bins[k];
        q.off[k] = M.off[k];
    }
    for (int i = 0; i < n_q; ++i) q.probs[i] = probs[i];
    for (int j = 0; j < M.n_bins_total; ++j) q.bin_value[j] = bin_value[j];
    const long long total = (long long)n_vox * D.n_free;
    hipLaunchKernelGGL(grid_marginal_quantile_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, q);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

}  // namespace pnx
