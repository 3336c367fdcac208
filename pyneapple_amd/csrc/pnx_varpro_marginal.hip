// pnx_varpro_marginal.hip -- the marginal posterior of every rate (and a free T1) of every voxel over the variable projection's
// dictionary, quantiles and a geometric posterior mean from it (pnx_curvefit_varpro_marginals_f64).
// P_k[v, j] = sum_g W_vg [atom g sits on the j-th grid value of parameter k]: the normalised weights of the posterior of 4.1i times
// a 0/1 indicator matrix, a second product on v_mfma_f64_16x16x4 behind the K chains of the first.  ONE pass over the products
// c = Phi^T y: a normaliser pass would repeat the K x K amplitude solve of every voxel-atom pair, which is what bounds this family
// of kernels, so the weights are formed about a running maximum per voxel and the sums are rescaled when it moves.
//
//   varpro_posterior_prep_kernel    the posterior's (pnx_varpro_posterior.hip: varpro_posterior_prepare), reused: lw per atom and
//                                   the cancellation floor
//   varpro_marginal_kernel          voxel-stationary, one strip of 16 voxels per wave, the dictionary through LDS in the posterior's
//                                   slabs.  The first product is formed TRANSPOSED (column fragment of the dictionary as A, signal
//                                   fragment as B), so that register `reg` of chain i holds atom 16 t + 4 reg + (l >> 4) against
//                                   voxel l & 15 -- and the weight made from it is the B operand of k-step `reg` of
//                                   marginal^T[bin, voxel] += Ind[bin, atom] W[atom, voxel]  as it stands: no shuffle, no LDS
//                                   transpose.  The A operand of that k-step is 1.0 where one of the atom's global bin indices (a
//                                   per-slab LDS table, one int per non-linear row with bins and atom) is the lane's bin
//                                   16 c + (l & 15), else 0.0.  One f64x4 of accumulators per 16-bin chunk c, NC of them (template),
//                                   divided by the voxel's sum of weights and written bin-major at the end.
//   varpro_marginal_quantile_kernel one lane per voxel and free parameter: the running sum of its bins, the first bin at or above
//                                   every level, the geometric mean; lane k = 0 of a voxel also writes log_evidence.  A restatement
//                                   of grid_marginal_quantile_kernel (pnx_grid_marginal.hip, left untouched) with the geometric mean.
//
// No atomics; a voxel's sums depend on the order of the atoms only (header).  Lane maps of the MFMA: A[l & 15][l >> 4],
// B[l >> 4][l & 15], D: col = l & 15, row = (l >> 4) + 4 reg.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "pnx_launch.hpp"
#include "pnx_varpro_marginal.hpp"
#include "pnx_varpro_pair.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int kVpMargWaves = 4;  // a block: one wave per SIMD, as the posterior's

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

size_t varpro_marginal_bytes(int n_free, int n_atoms) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15;
    return up256((size_t)n_free * gp * sizeof(int32_t));
}

int varpro_marginal_prepare(const VarproDict &D, const GridMarginalHost &M, const int32_t *bin_of_host, void *buffer_d, VarproMarginal *G,
                            hipStream_t st) {
    std::vector<int32_t> table((size_t)M.n_rows * D.gp);
    grid_marginal_table(D.n_free, D.n_atoms, D.gp, M, bin_of_host, table.data());
    // the copy from pageable memory is staged before the call returns (as the atoms of the dictionary)
    PNX_HIP(hipMemcpyAsync(buffer_d, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    G->table = (const int32_t *)buffer_d;
    G->host = M;
    return PNX_OK;
}

struct VpMargArgs {
    const double *y;       // (n_vox, n_b)
    const double *st;      // (K kpad, gp)
    const double *cst;     // (crow, gp)
    const double *wd;      // (kpad)
    const double *lw;      // (gp)
    const double *max_nrm;
    const int32_t *table;  // (n_rows, gp)
    double *out;           // (n_bins, n_vox)
    double *lv;            // (n_vox)
    long long n_vox;
    int n_b, kpad, gp, width, stride, noise_marginal, n_rows, n_bins;
    double lo[3], hi[3];  // bounds of the linear slots (S0 class: slot K - 1 is S0)
    double tol_scale;     // 4 n_b 2^-52
    double amp2;          // A^2
    double gain;          // known noise: 1 / noise_sd^2;  marginalised: nu / 2
};

// LDS: the posterior's image of a slab -- [K kpad][stride] | constants [2 NM][W] | lw [W] -- then the table [n_rows][W] int32 in
// the place of its centred non-linear rows.  NS: k-steps the register file is sized for (n_b <= 4 NS).
template <int NS, int K, int CLS, int NC>
__global__ void __launch_bounds__(kVpMargWaves * 64) varpro_marginal_kernel(const VpMargArgs a) {
    constexpr int NM = K * (K + 1) / 2;
    extern __shared__ double lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lc = lds + K * kpad * stride, *llw = lc + 2 * NM * W;
    int32_t *ltab = reinterpret_cast<int32_t *>(llw + W);
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kVpMargWaves - 1) / kVpMargWaves;
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    const double floor_nrm = a.amp2 * *a.max_nrm;
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        // B fragment of this wave's strip, the posterior's loads: weighted, rows past the end repeat the last voxel (never stored).
        // In the transposed product a lane's accumulator column is voxel v0 + r16: ||y||^2, the floor and the finite flag are
        // per-lane values.
        const long long v0 = (grp * kVpMargWaves + wave) * 16, v = v0 + r16;
        double yf[NS], yy;
        bool ok;
        {
            const double *row = a.y + (size_t)(v < a.n_vox ? v : a.n_vox - 1) * a.n_b;
            double ss = 0.0;
            int bad = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int k = 4 * s + kq;
                const double val = (s < ksteps && k < a.n_b) ? row[k] * a.wd[k] : 0.0;
                bad |= !(fabs(val) < inf);  // NaN or Inf, of the signal or through a zero sigma
                ss = fma(val, val, ss);
                yf[s] = val;
            }
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            bad |= __shfl_xor(bad, 16);
            bad |= __shfl_xor(bad, 32);
            yy = ss;
            ok = !bad;
        }
        const double tol = a.tol_scale * (yy + floor_nrm);
        // the voxel's running maximum mx of l (the same in its four lanes), this lane's share sw of the sum of the weights about
        // it, and the bins' sums about it
        double mx = -inf, sw = 0.0;
        f64x4 m[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) m[c] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                for (int k = wave; k < K * kpad; k += kVpMargWaves)
                    for (int j = lane; j < wc; j += 64) lds[k * stride + j] = a.st[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < 2 * NM; k += kVpMargWaves)
                    for (int j = lane; j < wc; j += 64) lc[k * W + j] = a.cst[(size_t)k * a.gp + g0 + j];
                for (int k = wave; k < a.n_rows; k += kVpMargWaves)
                    for (int j = lane; j < wc; j += 64) ltab[k * W + j] = a.table[(size_t)k * a.gp + g0 + j];
                for (int j = threadIdx.x; j < wc; j += kVpMargWaves * 64) llw[j] = a.lw[g0 + j];
                __syncthreads();
                resident = n_slabs == 1;
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc[K];
#pragma unroll
                for (int i = 0; i < K; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
                const double *ap = lds + kq * stride + t * 16 + r16;  // A fragment: phi_i[g0 + 16 t + r16][4 s + kq]
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (s < ksteps) {
#pragma unroll
                        for (int i = 0; i < K; ++i)
                            acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[(i * kpad + 4 * s) * stride], yf[s], acc[i], 0, 0, 0);
                    }
                }
                // register r: atom j = 16 t + 4 r + kq of the slab against voxel r16 -- l_g by the posterior's function.  A padded
                // or excluded atom holds lw = -inf and weighs exactly 0, as does every atom of a non-finite voxel.
                double ell[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = t * 16 + 4 * r + kq;
                    const double lwg = llw[j];
                    double M[NM], I[NM], c[K];
#pragma unroll
                    for (int q = 0; q < NM; ++q) {
                        M[q] = lc[q * W + j];
                        I[q] = lc[(NM + q) * W + j];
                    }
#pragma unroll
                    for (int i = 0; i < K; ++i) c[i] = acc[i][r];
                    const double l = vp_log_weight<K, CLS>(c, M, I, a.lo, a.hi, yy, tol, lwg, a.gain, a.noise_marginal);
                    ell[r] = (ok && lwg > -inf) ? l : -inf;
                }
                // the tile's largest l of this voxel: the four registers, then the four lane groups the second product sums over
                double tm = fmax(fmax(ell[0], ell[1]), fmax(ell[2], ell[3]));
                tm = fmax(tm, __shfl_xor(tm, 16));
                tm = fmax(tm, __shfl_xor(tm, 32));
                const double mn = fmax(mx, tm);
                if (__any(mn != mx)) {  // a maximum moved somewhere in the wave: rescale what has been summed about the old one
                    const double alpha = mn == mx ? 1.0 : exp(mx - mn);  // (-inf) - (-inf) never reaches exp
                    sw *= alpha;
#pragma unroll
                    for (int c2 = 0; c2 < NC; ++c2) m[c2] *= alpha;
                    mx = mn;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = t * 16 + 4 * r + kq;
                    const double w = ell[r] > -inf ? exp(ell[r] - mx) : 0.0;  // mx >= ell[r] is finite where ell[r] is
                    sw += w;
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
        // the voxel's sum of weights: its four lanes' shares in one order (addition commutes: the four lanes hold the same bits)
        double tot = sw;
        tot += __shfl_xor(tot, 16);
        tot += __shfl_xor(tot, 32);
        const bool none = !ok || !(tot > 0.0);  // a non-finite signal, or no atom with a finite l
        // D of the second product: row = bin 16 c + kq + 4 r, column = voxel r16: 16 consecutive voxels per bin row
        if (v < a.n_vox) {
            const double qnan = __builtin_nan("");
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int bin = 16 * c + kq + 4 * r;
                    if (bin < a.n_bins) a.out[(size_t)bin * a.n_vox + v] = none ? qnan : m[c][r] / tot;
                }
            if (kq == 0) a.lv[v] = none ? qnan : mx + log(tot);
        }
    }
}

struct VpQuantArgs {
    const double *marginal;  // (n_bins, n_vox)
    const double *lv;        // (n_vox)
    double *quantile;        // (n_q, n_free, n_vox) or null
    double *geo;             // (n_free, n_vox) or null
    double *logev;           // (n_vox) or null
    long long n_vox;
    int n_free, n_q;
    double lp_norm;
    int n_bins[PNX_MAX_PARAMS], off[PNX_MAX_PARAMS];
    int geo_ok[PNX_MAX_PARAMS];  // the parameter has bins and every bin value is > 0
    double probs[kGridMarginalMaxProbs];
    double bin_value[kGridMarginalMaxBins];
    double log_value[kGridMarginalMaxBins];  // log of a positive bin value, else 0
};

__global__ void __launch_bounds__(256) varpro_marginal_quantile_kernel(const VpQuantArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n_vox * a.n_free) return;
    const int k = (int)(idx / a.n_vox);
    const long long v = idx - (long long)k * a.n_vox;
    const double qnan = __builtin_nan("");
    const double L = a.lv[v];
    const bool bad = !(fabs(L) < __builtin_huge_val());
    if (k == 0 && a.logev) a.logev[v] = bad ? qnan : L - a.lp_norm;
    if (!a.quantile && !a.geo) return;
    const int nb = a.n_bins[k], off = a.off[k];
    double q[kGridMarginalMaxProbs];
#pragma unroll
    for (int i = 0; i < kGridMarginalMaxProbs; ++i) q[i] = (bad || nb == 0) ? qnan : a.bin_value[off + nb - 1];
    double cdf = 0.0, num = 0.0;
    if (!bad && nb) {
        unsigned found = 0;
        for (int j = 0; j < nb; ++j) {  // the running sum in bin order; the first bin at or above a level keeps it
            const double p = a.marginal[(size_t)(off + j) * a.n_vox + v];
            cdf += p;
            num = fma(p, a.log_value[off + j], num);
            const double val = a.bin_value[off + j];
#pragma unroll
            for (int i = 0; i < kGridMarginalMaxProbs; ++i) {
                const bool hit = i < a.n_q && !(found >> i & 1) && cdf >= a.probs[i];
                q[i] = hit ? val : q[i];
                found |= hit ? 1u << i : 0u;
            }
        }
    }
    if (a.quantile) {
#pragma unroll
        for (int i = 0; i < kGridMarginalMaxProbs; ++i)
            if (i < a.n_q) a.quantile[((size_t)i * a.n_free + k) * a.n_vox + v] = q[i];
    }
    if (a.geo) a.geo[(size_t)k * a.n_vox + v] = (bad || !a.geo_ok[k]) ? qnan : exp(num / cdf);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
template <int NS, int K, int CLS> static void launch_vp_marg(const VpMargArgs &a, int chunks, unsigned blocks, size_t lds, hipStream_t st) {
    if (chunks == 4)
        hipLaunchKernelGGL((varpro_marginal_kernel<NS, K, CLS, 4>), dim3(blocks), dim3(kVpMargWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((varpro_marginal_kernel<NS, K, CLS, 8>), dim3(blocks), dim3(kVpMargWaves * 64), lds, st, a);
}

template <int K, int CLS> static void launch_vp_marg_ns(const VpMargArgs &a, int chunks, unsigned blocks, size_t lds, hipStream_t st) {
    if (a.kpad <= 32)
        launch_vp_marg<8, K, CLS>(a, chunks, blocks, lds, st);
    else
        launch_vp_marg<32, K, CLS>(a, chunks, blocks, lds, st);
}

int varpro_marginal_device(const VarproDict &D, const VarproPosterior &P, const VarproMarginal &G, int64_t n_vox, const double *y_d,
                           const double *bin_value, int n_q, const double *probs, double *marginal_d, double *lv_d, double *quantile_d,
                           double *geo_mean_d, double *log_evidence_d, int cus, hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const VarproLayout &L = D.L;
    const GridSlab S = varpro_marginal_slab(D.n_b, L.k);
    const GridMarginalHost &M = G.host;
    VpMargArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.cst = D.cst;
    a.wd = D.w;
    a.lw = P.lw;
    a.max_nrm = P.max_nrm;
    a.table = G.table;
    a.out = marginal_d;
    a.lv = lv_d;
    a.n_vox = n_vox;
    a.n_b = D.n_b;
    a.kpad = S.kpad;
    a.gp = D.gp;
    a.width = S.width < D.gp ? S.width : D.gp;
    a.stride = S.stride;
    a.noise_marginal = P.noise_sd == 0.0;
    a.n_rows = M.n_rows;
    a.n_bins = M.n_bins_total;
    for (int j = 0; j < 3; ++j) {
        a.lo[j] = L.lin_lo[j];
        a.hi[j] = L.lin_hi[j];
    }
    a.tol_scale = 4.0 * D.n_b * 0x1p-52;
    a.amp2 = P.amp_l1 * P.amp_l1;
    a.gain = a.noise_marginal ? 0.5 * (D.n_b - L.n_lin) : 1.0 / (P.noise_sd * P.noise_sd);
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    const int chunks = varpro_marginal_chunks(M.n_bins_total);
    const long long n_strips = (n_vox + 15) / 16;
    long long blocks = (n_strips + kVpMargWaves - 1) / kVpMargWaves;
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;  // the posterior's cap; no sum depends on it
    if (blocks > cap) blocks = cap;
    const unsigned nb = (unsigned)blocks;
    switch (L.k * 4 + L.cls) {
    case 1 * 4 + kVarproFree: launch_vp_marg_ns<1, kVarproFree>(a, chunks, nb, lds, stream); break;
    case 2 * 4 + kVarproFree: launch_vp_marg_ns<2, kVarproFree>(a, chunks, nb, lds, stream); break;
    case 2 * 4 + kVarproReduced: launch_vp_marg_ns<2, kVarproReduced>(a, chunks, nb, lds, stream); break;
    case 2 * 4 + kVarproS0: launch_vp_marg_ns<2, kVarproS0>(a, chunks, nb, lds, stream); break;
    case 3 * 4 + kVarproFree: launch_vp_marg_ns<3, kVarproFree>(a, chunks, nb, lds, stream); break;
    case 3 * 4 + kVarproReduced: launch_vp_marg_ns<3, kVarproReduced>(a, chunks, nb, lds, stream); break;
    case 3 * 4 + kVarproS0: launch_vp_marg_ns<3, kVarproS0>(a, chunks, nb, lds, stream); break;
    default: return set_error(PNX_ERR_INVALID, "varpro marginals: no kernel for %d compartments, class %d", L.k, L.cls);
    }
    PNX_HIP(hipGetLastError());
    if (!(n_q && quantile_d) && !geo_mean_d && !log_evidence_d) return PNX_OK;
    VpQuantArgs q;
    memset(&q, 0, sizeof(q));
    q.marginal = marginal_d;
    q.lv = lv_d;
    q.quantile = n_q ? quantile_d : nullptr;
    q.geo = geo_mean_d;
    q.logev = log_evidence_d;
    q.n_vox = n_vox;
    q.n_free = D.n_free;
    q.n_q = n_q;
    q.lp_norm = P.log_prior_norm;
    for (int k = 0; k < D.n_free; ++k) {
        q.n_bins[k] = M.n_bins[k];
        q.off[k] = M.off[k];
        q.geo_ok[k] = M.n_bins[k] > 0;
        for (int j = 0; j < M.n_bins[k]; ++j) q.geo_ok[k] &= bin_value[M.off[k] + j] > 0.0;
    }
    for (int i = 0; i < n_q; ++i) q.probs[i] = probs[i];
    for (int j = 0; j < M.n_bins_total; ++j) {
        q.bin_value[j] = bin_value[j];
        q.log_value[j] = bin_value[j] > 0.0 ? std::log(bin_value[j]) : 0.0;
    }
    const long long total = (long long)n_vox * D.n_free;
    hipLaunchKernelGGL(varpro_marginal_quantile_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, q);
    PNX_HIP(hipGetLastError());
    return PNX_OK;
}

}  // namespace pnx
