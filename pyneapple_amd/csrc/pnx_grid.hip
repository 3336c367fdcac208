// pnx_grid.hip -- per-voxel start values for the curve fit from a dictionary search (pnx_curvefit_grid_start_f64).
// The cost of a voxel against G candidate parameter vectors ("atoms") is one row of the dense product Y (n_vox, n_b) . S^T
// (n_b, G) followed by a row-wise argmin:  cost_g(v) = 0.5 (||y_v||^2 - 2 y_v . s_g + ||s_g||^2),  s_g = model(b; atom_g).
//
//   grid_dict_finish_kernel   the dictionary rows as model_predict_kernel wrote them (the fit's own arithmetic) -> weighted by
//                             1 / sigma, transposed to k-major, padded with zero rows and zero atoms; ||s_g||^2 and its inverse
//   grid_match_kernel         the product on v_mfma_f64_16x16x4_f64, tiles of 16 voxels x 16 atoms stepping 4 along n_b.  A wave
//                             keeps the y fragments of its voxels in registers, walks every atom tile out of an LDS slab and folds
//                             each accumulator tile into a running (min, argmin) per voxel; one cross-lane reduction at the end.
//                             The (n_vox, G) product never reaches HBM: a voxel costs its signal row in and a few dozen bytes out.
//
// Lane maps of the MFMA (pnx_nnls.hip nnls_aty_mfma_kernel): A[l & 15][l >> 4], B[l >> 4][l & 15], D: col = l & 15 (the atom),
// row = (l >> 4) + 4 * reg (the voxel of the strip).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "pnx_curvefit_kernel.hpp"
#include "pnx_grid.hpp"
#include "pnx_grid_args.hpp"
#include "pnx_internal.hpp"
#include "pnx_predict.hpp"

namespace pnx {

using f64x4 = __attribute__((ext_vector_type(4))) double;

#define GR_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t e__ = (call);                                                                     \
        if (e__ != hipSuccess) return set_error(PNX_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

// ---- dictionary -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) grid_fill_kernel(double *p, int n, double v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

struct FinishArgs {
    const double *raw;  // (n_atoms, n_b) model(b; atom_g)
    double *st;         // (kpad, gp)
    double *nrm, *inv;  // (gp)
    double *wd;         // (kpad)
    int n_atoms, n_b, kpad, gp;
    double w[kMaxB];  // 1 / sigma_i
};

// one lane per atom (padded atoms included: their rows are zero); reads strided, writes coalesced -- 4 MB at the cap, once per call
__global__ void __launch_bounds__(256) grid_dict_finish_kernel(const FinishArgs a) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < a.kpad) a.wd[g] = g < a.n_b ? a.w[g] : 0.0;
    if (g >= a.gp) return;
    double ss = 0.0;
    for (int k = 0; k < a.kpad; ++k) {
        const double v = (g < a.n_atoms && k < a.n_b) ? a.raw[(size_t)g * a.n_b + k] * a.w[k] : 0.0;
        a.st[(size_t)k * a.gp + g] = v;
        ss = fma(v, v, ss);
    }
    a.nrm[g] = ss;
    a.inv[g] = ss > 0.0 ? 1.0 / ss : 0.0;  // an all-zero row costs 0.5 ||y||^2 with any amplitude: the lower bound is taken
}

static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

size_t grid_dict_bytes(int n_free, int n_atoms, int n_b) {
    const size_t gp = ((size_t)n_atoms + 15) & ~(size_t)15, kpad = ((size_t)n_b + 3) & ~(size_t)3;
    return 2 * up256((size_t)n_free * n_atoms * 8) + up256((size_t)n_atoms * n_b * 8) + up256(kpad * gp * 8) + 2 * up256(gp * 8) + up256(kpad * 8);
}

int grid_dict_build(const pnx_curvefit_opts *o, const double *b, int n_atoms, const double *atoms_host, const double *fixed_host,
                    const double *lo, const double *hi, int s0_row, void *buffer_d, GridDict *D, hipStream_t st) {
    const int n = o->n_free, n_b = o->n_b;
    const int gp = (n_atoms + 15) & ~15, kpad = (n_b + 3) & ~3;
    char *p = (char *)buffer_d;
    auto take = [&](size_t bytes) {
        void *q = p;
        p += up256(bytes);
        return (double *)q;
    };
    double *atoms_d = take((size_t)n * n_atoms * 8), *unit_d = take((size_t)n * n_atoms * 8), *raw = take((size_t)n_atoms * n_b * 8);
    double *stt = take((size_t)kpad * gp * 8), *nrm = take((size_t)gp * 8), *inv = take((size_t)gp * 8), *wd = take((size_t)kpad * 8);
    // the copy from pageable memory is staged before the call returns (as the bin centres of a wide spectrum call)
    GR_HIP(hipMemcpyAsync(atoms_d, atoms_host, (size_t)n * n_atoms * 8, hipMemcpyHostToDevice, st));
    const double *params = atoms_d;
    if (s0_row >= 0) {  // projected amplitude: the dictionary is built with S0 = 1, the atoms' own S0 row is not read
        GR_HIP(hipMemcpyAsync(unit_d, atoms_d, (size_t)n * n_atoms * 8, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(grid_fill_kernel, dim3((n_atoms + 255) / 256), dim3(256), 0, st, unit_d + (size_t)s0_row * n_atoms, n_atoms, 1.0);
        GR_HIP(hipGetLastError());
        params = unit_d;
    }
    pnx_curvefit_opts c = *o;
    c.fixed_per_voxel = 0;
    if (int rc = model_predict_device(&c, n_atoms, n_b, b, params, fixed_host, nullptr, raw, nullptr, st)) return rc;
    FinishArgs a;
    memset(&a, 0, sizeof(a));
    a.raw = raw;
    a.st = stt;
    a.nrm = nrm;
    a.inv = inv;
    a.wd = wd;
    a.n_atoms = n_atoms;
    a.n_b = n_b;
    a.kpad = kpad;
    a.gp = gp;
    for (int i = 0; i < n_b; ++i) a.w[i] = o->sigma ? 1.0 / o->sigma[i] : 1.0;  // transform = 1.0 / sigma, as the fit
    const int lanes = gp > kpad ? gp : kpad;
    hipLaunchKernelGGL(grid_dict_finish_kernel, dim3((lanes + 255) / 256), dim3(256), 0, st, a);
    GR_HIP(hipGetLastError());
    D->atoms = atoms_d;
    D->st = stt;
    D->nrm = nrm;
    D->inv = inv;
    D->w = wd;
    D->n_b = n_b;
    D->n_free = n;
    D->n_atoms = n_atoms;
    D->gp = gp;
    D->s0_row = s0_row;
    D->lo_s0 = s0_row >= 0 ? lo[s0_row] : 0.0;
    D->hi_s0 = s0_row >= 0 ? hi[s0_row] : 0.0;
    return PNX_OK;
}

// ---- match ------------------------------------------------------------------------------------------------------------------
// A block is eight waves; a wave owns MS strips of 16 voxels per pass, a block 128 MS voxels.  The dictionary comes through LDS
// in slabs of `width` atoms ([k][stride], pnx_grid_args.hpp grid_slab): one that fits a single slab is copied once per block,
// a larger one once per pass (out of L2: 4 MB at the cap).  NS: k-steps the register file is sized for (n_b <= 4 NS).
constexpr int kGridWaves = 8;

struct GridArgs {
    const double *y;      // (n_vox, n_b)
    const double *st;     // (kpad, gp)
    const double *nrm, *inv;  // (gp)
    const double *wd;     // (kpad)
    const double *atoms;  // (n_free, n_atoms)
    double *p0_out;       // (n_free, n_vox)
    int32_t *best;        // (n_vox) or null
    double *cost;         // (n_vox) or null
    long long n_vox;
    int n_b, kpad, n_atoms, gp, n_free, width, stride, s0_row;
    double lo_s0, hi_s0;
};

template <int NS, int MS, bool PROJ>
__global__ void __launch_bounds__(kGridWaves * 64) grid_match_kernel(const GridArgs a) {
    extern __shared__ double lds[];  // [kpad][stride] | nrm[width] | inv[width]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int n_b = a.n_b, kpad = a.kpad, ksteps = kpad >> 2, stride = a.stride, W = a.width;
    double *lnrm = lds + kpad * stride, *linv = lnrm + W;
    const long long n_strips = (a.n_vox + 15) / 16;
    const long long n_groups = (n_strips + kGridWaves * MS - 1) / (kGridWaves * MS);
    const int n_slabs = (a.gp + W - 1) / W;
    const double inf = __builtin_huge_val();
    bool resident = false;
    for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // uniform per block: the barriers below are safe
        // A fragments of this wave's strips: y[v0 + r16][4 s + kq] / sigma; rows past the end repeat the last voxel, never stored
        double yf[MS][NS], yy[MS];
        int nf[MS];
        long long v0[MS];
#pragma unroll
        for (int m = 0; m < MS; ++m) {
            v0[m] = ((grp * kGridWaves + wave) * MS + m) * 16;
            const long long v = v0[m] + r16;
            const double *row = a.y + (size_t)(v < a.n_vox ? v : a.n_vox - 1) * n_b;
            double ss = 0.0;
            int bad = 0;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int k = 4 * s + kq;
                const double val = (s < ksteps && k < n_b) ? row[k] * a.wd[k] : 0.0;
                bad |= !(fabs(val) < inf);  // NaN or Inf, of the signal or through a zero sigma
                ss = fma(val, val, ss);
                yf[m][s] = val;
            }
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            bad |= __shfl_xor(bad, 16);
            bad |= __shfl_xor(bad, 32);
            yy[m] = ss;  // ||y||^2 of row r16, the same in its four lanes
            nf[m] = bad;
        }
        double bm[MS][4], ba[MS][4];
        int bg[MS][4];
#pragma unroll
        for (int m = 0; m < MS; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bm[m][r] = inf;
                ba[m][r] = 0.0;
                bg[m][r] = INT_MAX;
            }
        for (int slab = 0; slab < n_slabs; ++slab) {
            const int g0 = slab * W;
            const int wc = (a.gp - g0) < W ? (a.gp - g0) : W;  // a multiple of 16
            if (!resident) {
                __syncthreads();  // every wave has left the previous slab behind
                for (int k = wave; k < kpad; k += kGridWaves)
                    for (int j = lane; j < wc; j += 64) lds[k * stride + j] = a.st[(size_t)k * a.gp + g0 + j];
                for (int j = threadIdx.x; j < wc; j += kGridWaves * 64) {
                    lnrm[j] = a.nrm[g0 + j];
                    linv[j] = a.inv[g0 + j];
                }
                __syncthreads();
                resident = n_slabs == 1;
            }
            for (int t = 0; t < (wc >> 4); ++t) {
                f64x4 acc[MS];
#pragma unroll
                for (int m = 0; m < MS; ++m) acc[m] = f64x4{0.0, 0.0, 0.0, 0.0};
                const double *bp = lds + kq * stride + t * 16 + r16;  // B fragment: S[g0 + 16 t + r16][4 s + kq]
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (s < ksteps) {
                        const double bf = bp[4 * s * stride];
#pragma unroll
                        for (int m = 0; m < MS; ++m) acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(yf[m][s], bf, acc[m], 0, 0, 0);
                    }
                }
                // fold: this lane's atom against its four voxels of each strip; atoms arrive in ascending order, so a strict
                // comparison keeps the lowest index among equal costs; a padded atom costs +inf and never wins
                const int g = g0 + t * 16 + r16;
                const bool live = g < a.n_atoms;
                const double nr = lnrm[t * 16 + r16];
                const double iv = PROJ ? linv[t * 16 + r16] : 0.0;
#pragma unroll
                for (int m = 0; m < MS; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double dot = acc[m][r];
                        double amp = 1.0, c;  // c = cost - 0.5 ||y||^2
                        if constexpr (PROJ) {
                            amp = fmin(fmax(dot * iv, a.lo_s0), a.hi_s0);
                            c = amp * fma(0.5 * amp, nr, -dot);
                        } else {
                            c = fma(0.5, nr, -dot);
                        }
                        c = live ? c : inf;
                        if (c < bm[m][r]) {
                            bm[m][r] = c;
                            bg[m][r] = g;
                            ba[m][r] = amp;
                        }
                    }
            }
        }
        // one reduction over the 16 lanes (atoms modulo 16) that share a voxel: lower cost, then lower index -- symmetric, so
        // every lane of the group ends with the same answer and lane r16 writes output row r16
#pragma unroll
        for (int m = 0; m < MS; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double c = bm[m][r], amp = ba[m][r];
                int g = bg[m][r];
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) {
                    const double oc = __shfl_xor(c, off, 16), oa = __shfl_xor(amp, off, 16);
                    const int og = __shfl_xor(g, off, 16);
                    const bool take = oc < c || (oc == c && og < g);
                    c = take ? oc : c;
                    amp = take ? oa : amp;
                    g = take ? og : g;
                }
                const int src = kq + 4 * r;  // this voxel's row of the strip: its ||y||^2 and finite flag live in lane `src`
                const double yyv = __shfl(yy[m], src);
                const int badv = __shfl(nf[m], src);
                const long long v = v0[m] + src;
                if (v < a.n_vox) {
                    const int gi = (badv || g == INT_MAX) ? 0 : g;  // a non-finite signal takes atom 0 as it is
                    if (r16 < a.n_free) {
                        double val = a.atoms[(size_t)r16 * a.n_atoms + gi];
                        if (PROJ && r16 == a.s0_row && !badv) val = amp;
                        a.p0_out[(size_t)r16 * a.n_vox + v] = val;
                    } else if (r16 == 8) {
                        if (a.best) a.best[v] = badv ? -1 : gi;
                    } else if (r16 == 9) {
                        if (a.cost) a.cost[v] = badv ? __builtin_nan("") : fma(0.5, yyv, c);
                    }
                }
            }
    }
}

template <int NS, int MS> static int launch_match(const GridArgs &a, size_t lds, long long blocks, hipStream_t st) {
    if (a.s0_row >= 0)
        hipLaunchKernelGGL((grid_match_kernel<NS, MS, true>), dim3((unsigned)blocks), dim3(kGridWaves * 64), lds, st, a);
    else
        hipLaunchKernelGGL((grid_match_kernel<NS, MS, false>), dim3((unsigned)blocks), dim3(kGridWaves * 64), lds, st, a);
    GR_HIP(hipGetLastError());
    return PNX_OK;
}

int grid_match_device(const GridDict &D, int64_t n_vox, const double *y_d, double *p0_out_d, int32_t *best_d, double *cost_d, int cus,
                      hipStream_t stream) {
    if (n_vox <= 0) return PNX_OK;
    const GridSlab S = grid_slab(D.n_b);
    GridArgs a;
    memset(&a, 0, sizeof(a));
    a.y = y_d;
    a.st = D.st;
    a.nrm = D.nrm;
    a.inv = D.inv;
    a.wd = D.w;
    a.atoms = D.atoms;
    a.p0_out = p0_out_d;
    a.best = best_d;
    a.cost = cost_d;
    a.n_vox = n_vox;
    a.n_b = D.n_b;
    a.kpad = S.kpad;
    a.n_atoms = D.n_atoms;
    a.gp = D.gp;
    a.n_free = D.n_free;
    a.width = S.width < D.gp ? S.width : D.gp;
    a.stride = S.stride;
    a.s0_row = D.s0_row;
    a.lo_s0 = D.lo_s0;
    a.hi_s0 = D.hi_s0;
    const size_t lds = (size_t)S.lds_doubles * sizeof(double);  // <= 64 KB
    const int ms = S.kpad <= 64 ? 2 : 1;
    const long long n_strips = (n_vox + 15) / 16;
    long long blocks = (n_strips + kGridWaves * ms - 1) / (kGridWaves * ms);
    const long long cap = (long long)(cus > 0 ? cus : 256) * 2;
    if (blocks > cap) blocks = cap;
    if (S.kpad <= 32) return launch_match<8, 2>(a, lds, blocks, stream);
    if (S.kpad <= 64) return launch_match<16, 2>(a, lds, blocks, stream);
    return launch_match<32, 1>(a, lds, blocks, stream);
}

}  // namespace pnx
